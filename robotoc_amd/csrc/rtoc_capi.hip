// rtoc_capi.hip -- implementation of the C ABI declared in include/rtoc.h.
// Context, HBM buffers, kernel dispatch by problem dimensions.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtoc.h"
#include "../../include/rtoc_robot.h"
#include "device_buffer.hpp"
#include "kernel_set.hpp"
#include "record_view.hpp"
#include "rigid_body.hpp"
#include "unconstr_constraints.hpp"
#include "state_equation_lin.hpp"
#include "switching_constraint_lin.hpp"
#include "contact_constraints.hpp"
#include "contact_eval_kkt.hpp"
#include "task_space_cost.hpp"
#include "sto.hpp"

using namespace rtoc;

#define HIP_TRY(expr)                       \
  do {                                      \
    hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) {                 \
      ctx_set_err(e_, __LINE__);            \
      return RTOC_ERR_HIP;                  \
    }                                       \
  } while (0)

static thread_local char g_errbuf[256] = "";
static void ctx_set_err(hipError_t e, int line) {
  snprintf(g_errbuf, sizeof(g_errbuf), "HIP error %d (%s) at rtoc_capi.hip:%d", (int)e,
           hipGetErrorString(e), line);
}

// ---- kernel table: one entry per compiled robot shape (shape_inst.hip; SHAPES in the Makefile) ------------
#define RTOC_SHAPE(nv, nu, ns, nw0, nw1) namespace rtoc { KernelSet rtoc_shape_##nv##_##nu##_##ns(); }
#include "shape_table.inc"
#undef RTOC_SHAPE
static const std::vector<KernelSet>& kernel_table() {
  static std::vector<KernelSet> t = {
#define RTOC_SHAPE(nv, nu, ns, nw0, nw1) rtoc::rtoc_shape_##nv##_##nu##_##ns(),
#include "shape_table.inc"
#undef RTOC_SHAPE
  };
  return t;
}

// Shapes beyond the compiled-in table: librtoc_shape_<nv>_<nu>_<ns>.so next to this library (or in $RTOC_SHAPE_DIR),
// built by `make -C robotoc_amd/csrc plugin SHAPE=nv:nu:ns:nw0:nw1`; with RTOC_SHAPE_JIT=1 rtoc_create builds it itself, next to
// this library wherever it lives now (hipcc + the source directory this library was built from must be present; ~1 min, once).
#include <mutex>
static std::vector<KernelSet>& plugin_table() {
  static std::vector<KernelSet> t;
  return t;
}
static std::string library_dir() {
  Dl_info info;
  if (dladdr((const void*)&library_dir, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    const size_t k = p.find_last_of('/');
    return k == std::string::npos ? std::string(".") : p.substr(0, k);
  }
  return ".";
}
static const KernelSet* load_plugin(const rtoc_dims* d) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& k : plugin_table())
    if (k.nv == d->nv && k.nu == d->nu && k.ns == d->ns_max) return &k;
  char name[96];
  snprintf(name, sizeof name, "librtoc_shape_%d_%d_%d.so", d->nv, d->nu, d->ns_max);
  std::vector<std::string> dirs;
  if (const char* e = getenv("RTOC_SHAPE_DIR")) dirs.push_back(e);
  dirs.push_back(library_dir());
  void* h = nullptr;
  for (const auto& dir : dirs)
    if ((h = dlopen((dir + "/" + name).c_str(), RTLD_NOW | RTLD_LOCAL))) break;
#ifdef RTOC_CSRC_DIR
  const char* jit = getenv("RTOC_SHAPE_JIT");
  if (!h && jit && jit[0] == '1') {
    // tile-split wave counts by state dimension, like the compiled-in shapes: one / three waves up to 36, four beyond
    const int nx = 2 * d->nv, nw0 = nx <= 36 ? 1 : 4, nw1 = nx <= 36 ? 3 : (nx > 64 ? 5 : 4);
    char shape[96];
    snprintf(shape, sizeof shape, "SHAPE=%d:%d:%d:%d:%d", d->nv, d->nu, d->ns_max, nw0, nw1);
    const std::string cmd = std::string("make -s -C '") + RTOC_CSRC_DIR + "' plugin " + shape + " PLUGIN_DIR='" + library_dir() + "' >/dev/null 2>&1";
    if (system(cmd.c_str()) == 0) h = dlopen((library_dir() + "/" + name).c_str(), RTLD_NOW | RTLD_LOCAL);
  }
#endif
  if (!h) return nullptr;
  typedef int (*entry_t)(KernelSet*, size_t, size_t);
  entry_t entry = (entry_t)dlsym(h, "rtoc_shape_plugin");
  KernelSet k;
  if (!entry || entry(&k, sizeof(KernelSet), kernel_abi_stamp()) != 0 || k.nv != d->nv || k.nu != d->nu || k.ns != d->ns_max) {
    dlclose(h);
    return nullptr;
  }
  plugin_table().reserve(64);  // handed-out pointers stay valid
  if (plugin_table().size() >= 64) return nullptr;
  plugin_table().push_back(k);
  return &plugin_table().back();
}

static const KernelSet* find_set(const rtoc_dims* d) {
  if (d->nf_max != d->ns_max || d->np != d->nv - d->nu) return nullptr;
  for (const auto& k : kernel_table())
    if (k.nv == d->nv && k.nu == d->nu && k.ns == d->ns_max) return &k;
  return load_plugin(d);
}
// every launch of a kernel of the set: block size and LDS are the descriptor's (extra_lds: what only the launch knows)
template <class A>
static void launch(const Kern<A>& k, dim3 grid, hipStream_t stream, const A& a, int extra_lds = 0) {
  hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), (size_t)(k.lds + extra_lds), stream, a);
}
// role-split kernel where it exists
static int default_bwd_variant(const KernelSet* ks) { return (ks->nvariants >= 3) ? ks->nvariants - 1 : 0; }

static bool model_has_surface_contacts(const rtoc_robot_model& m) {
  for (int k = 0; k < m.ncontacts; ++k)
    if (m.contact_type[k] == RTOC_CONTACT_SURFACE) return true;
  return false;
}
// hipFuncAttributeMaxDynamicSharedMemorySize is per function and process-wide, not per context: two live contexts with
// different models (iCub: 11 tree levels, ANYmal: 4) share it, so it only ever grows (the launch passes its own size)
static hipError_t set_linearize_lds(const rtoc_robot_model& m, int nlevels, int nbranch, int dpp) {
  static std::mutex mu;
  static int max_bytes_of[64] = {};   // the attribute is per DEVICE: one running maximum for each (the current one: callers hipSetDevice first)
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  int& max_bytes = max_bytes_of[dev];
  int bytes = (int)rbd::lin_lds_bytes(nlevels, nbranch, m.njoints, m.ncontacts, m.nv, dpp, false);   // the larger of the two modes
  if (bytes <= max_bytes) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void*)rbd::linearize_contact_dynamics_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)rbd::linearize_contact_dynamics_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)rbd::linearize_contact_dynamics_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)rbd::linearize_contact_dynamics_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)rbd::rbd_values_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * rbd::VAL_SLOTS * (int)sizeof(double));
  if (e == hipSuccess) max_bytes = bytes;
  return e;
}

// ---- context --------------------------------------------------------------------------
#define RTOC_MAX_CHUNK_EVENTS 16
// the backward recursion of one public call, as plan_backward decides it
enum BwdPath { BWD_SCAN, BWD_RV, BWD_RW, BWD_TILE };
struct BwdPlan {
  BwdPath path = BWD_SCAN;  // horizon scan, register-resident, register-wide (iCub-size shapes), tile-split / role-split
  const Kern<BwdArgs>* kern = nullptr;  // the kernel of the path (scan: its policy kernel; register-wide: the one between the one-stage launches)
  int check_fxx = 0;        // BwdArgs::check_fxx of the register-resident kernel: verify the structured rows as it goes
};
// Streams and events of a context.  A base of rtoc_ctx, so that it is destroyed after every member: device memory is freed
// first, streams and events go last.
struct CtxStreams {
  hipStream_t own_stream = nullptr;
  hipStream_t stream2 = nullptr;  // forward half of the pipelined sweep
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_chunk[RTOC_MAX_CHUNK_EVENTS] = {};
  CtxStreams() = default;
  CtxStreams(const CtxStreams&) = delete;
  CtxStreams& operator=(const CtxStreams&) = delete;
  ~CtxStreams() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    for (hipEvent_t e : ev_chunk)
      if (e) (void)hipEventDestroy(e);
  }
};
// The scalar settings rtoc_clone hands to the new context in one assignment (a base of rtoc_ctx: c->writeback etc.)
struct CtxOptions {
  int writeback = 0;
  double max_dts0 = 0.1;  // RiccatiRecursion(ocp, max_dts0 = 0.1), riccati_recursion.hpp:35
  double contact_inv_damping = 0.0;
  int bwd_variant = 0;
  int sweep_chunks = 1;         // measured on MI355X: chunked pipelining does not pay (forward waves do not fit next to the backward waves)
  int condense_split = 0;       // 1: MJtJinv in its own kernel ahead of the condensation
  int keep_qaf = 0;             // RTOC_OPT_CONDENSE_KEEP_QAF
  int fxx_mode = 0;             // RTOC_OPT_FXX_STRUCTURE: 0 auto, 1 dense, 2 caller asserts the structure
  int bwd_register = 1;         // RTOC_OPT_BACKWARD_REGISTER: the register-resident backward kernel where it applies (plan_backward)
  int cond_register = 1;        // RTOC_OPT_CONDENSE_REGISTER: the register-chained condensation of the contact grid points where it applies
  int use_graph = 0;            // RTOC_OPT_GRAPH: launch sequences replayed from captured hipGraphs
  int exact_transport = 0;      // RTOC_OPT_SWITCHING_TRANSPORT
  int unconstr_dense = 0;       // RTOC_OPT_UNCONSTR_DENSE
  int exact_cone_jacobian = 0;  // RTOC_OPT_CONE_JACOBIAN
  int impact_cones = 1;         // RTOC_OPT_IMPACT_CONES
  int linearize_fused = 0;      // RTOC_OPT_LINEARIZE_FUSED
  int lin_dpp = 0;              // RTOC_OPT_LINEARIZE_DOFS_PER_PASS (0 = per model)
  double barrier = 0.0, ftb_rule = 0.0;
  int n_mu = 0;                 // how many of d_mu's RTOC_MAX_CONTACTS entries the caller set
  bool has_cpos = false, has_crot = false;
  // filter line search on the device (rtoc_set_line_search, rtoc_contact_line_search)
  int ls_on = 0;
  double ls_rate = 0.0, ls_min_step = 0.0, ls_cost_rate = 0.0, ls_viol_rate = 0.0;
  int ls_method = 0;  // 0 LineSearchMethod::Filter, 1 MeritBacktracking (rtoc_set_line_search_method)
  double ls_armijo = 0.0, ls_margin = 0.0, ls_eps = 0.0;
};
struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  unsigned long long epoch = 0, warm_epoch = 0;
  double p0 = 0.0, p1 = 0.0;
  bool warm = false;
  ~GraphSlot() {
    if (exec) (void)hipGraphExecDestroy(exec);
  }
};
struct rtoc_ctx : CtxStreams, CtxOptions {
  rtoc_dims dims = {};
  rtoc_layout L = {};
  const KernelSet* ks = nullptr;
  int max_stages = 0, nstages = 0, batch = 0, device = 0;
  hipStream_t stream = nullptr;  // own_stream, or the caller's (rtoc_set_stream)
  DevBuf<double> buf[RTOC_NUM_BUFFERS];
  size_t want[RTOC_NUM_BUFFERS] = {};  // doubles of a buffer at max_stages (rtoc_buffer_count), allocated or not
  bool kkt_exposed = false;  // rtoc_device_ptr(RTOC_BUF_KKT) was handed out: the caller can rewrite the records without the runtime seeing it
  DevBuf<rtoc_grid> d_grid;
  DevBuf<rtoc_box_row> d_rows;
  std::vector<rtoc_box_row> h_rows;  // host copies (stage dump, rtoc_clone)
  std::vector<rtoc_grid> h_grid;
  DevBuf<int> d_nconv;  // instances found converged by the last rtoc_newton_iteration
  DevBuf<int> d_pair;   // first two rows of every primal entry, packed (int4 per entry)
  DevBuf<int> d_entry;  // CSR over the primal entries (q_0..,v_0..,u_0..): [ne+1] offsets, then [nrows] row ids
  int nrows = 0;
  DevBuf<uint32_t> d_status;
  DevBuf<long long> d_prof;
  int num_cus = 0;               // compute units of the device (the register-wide iCub kernel runs where the batch fills them)
  DevBuf<int> d_stage_list;      // [max_stages] grid points 0 .. nstages - 2: the contact ones first (n_stage_contact), then the impact ones
  int n_stage_contact = 0, n_stage_impact = 0;
  int fxx_state = 0;             // auto mode cache: 0 unknown (re-check before the next backward recursion), 1 every Fxx structured, 2 not
  BwdPlan bwd_plan;              // the last plan_backward's answer: the backward kernel baked into captured graphs
  unsigned long long graph_replays = 0;  // hipGraphLaunch count of RTOC_OPT_GRAPH (rtoc_graph_replay_count)
  DevBuf<int> d_fxx_flag;
  DevBuf<double> d_sto;          // rtoc_sto_eval_kkt staging: lt, diag(Qtt), squared error
  DevBuf<double> d_mu;           // rtoc_set_friction_coefficients
  DevBuf<double> d_wcone;        // rtoc_set_wrench_cone_params: [RTOC_MAX_CONTACTS][17 x 6]
  DevBuf<double> d_vals, d_vals2;  // rbd_values_kernel -> linearize_contact_dynamics_kernel<.., PRE>: [batch * max_stages][njoints][64]
  int vals_fresh = 0;            // the values in d_vals belong to the iterate in RTOC_BUF_SOL (consumed by the next launch_linearize)
  unsigned long long epoch = 0;  // bumped by everything that changes a launch parameter baked into a captured graph
  int cone_contacts = 0, cone_dim = 0;  // friction / wrench cones: max contacts (0 = off), force components per contact
  int cone_rows = 0;                    // PDIPM rows per contact: 5 friction cone, 17 contact wrench cone
  DevBuf<double> d_kkterr;              // [batch] + [batch][max_stages] partial sums
  int backward_scan = 0;                // RTOC_OPT_BACKWARD_SCAN
  DevBuf<double> d_scan[3];             // element ping-pong buffers, value records (allocated on first use)
  DevBuf<double> d_scan_sto;            // riccati_scan_sto.hpp: per grid point At, P+ Fx, P+ fx, factors of G
  // rigid-body model (rtoc_set_robot_model) and contact schedule (rtoc_set_contact_schedule)
  DevBuf<rbd::DevModel> d_model;
  std::unique_ptr<rbd::DevModel> h_model;
  DevBuf<unsigned> d_active;
  DevBuf<double> d_cpos;
  DevBuf<double> d_crot;
  // rtoc_line_search_filter: filters [batch][CAP][2], sizes [batch], staging (cost, violation | mask, accepted)
  DevBuf<double> d_cost;      // rtoc_set_configuration_cost: 12 (nv + 1) doubles
  DevBuf<double> d_bounds;    // rtoc_set_constraint_bounds: [nc_max]
  DevBuf<double> d_x0;        // rtoc_set_initial_state: [batch][nq + nv]
  DevBuf<double> d_filter;
  DevBuf<int> d_nfilter;
  DevBuf<double> d_ls_in;
  DevBuf<int> d_ls_flags;
  // switching-time optimisation on the device (rtoc_sto_set_problem; sto.hpp)
  int sto_on = 0, sto_nev = 0;
  double sto_t0 = 0.0, sto_T = 0.0, sto_barrier = 0.0, sto_tau = 0.0, sto_reg = 0.0;
  DevBuf<double> d_ts;         // [batch][nev] event times of every instance
  DevBuf<double> d_dt;         // [batch][max_stages] time steps of every instance (grid_dt)
  DevBuf<double> d_sto_con;    // [batch][RTOC_STO_CON_STRIDE] dwell-time rows
  DevBuf<double> d_min_dwell;  // [RTOC_STO_MAX_EVENTS + 1]
  DevBuf<double> d_sto_cost;   // [2][batch][nev] STO cost gradient / Hessian diagonal handed over by the host, or unallocated
  DevBuf<double> d_sto_out;    // [2][batch][nev] + [batch]: lt, Qtt diagonal as scattered, squared STO KKT term
  DevBuf<double> d_costval;    // [batch][max_stages] cost values of the last rtoc_contact_eval_kkt (rtoc_contact_eval_ocp)
  // task-space cost components (rtoc_set_task_costs; task_space_cost.hpp)
  DevBuf<rtoc_task_cost> d_tasks;  // capacity [batch][RTOC_MAX_TASK_COSTS]; in use [ntasks] or [batch][ntasks]
  int ntasks = 0, tasks_per_instance = 0;
  unsigned h_task_table = 0;       // bit k: term k (of some instance) has ref_kind RTOC_REF_TABLE
  DevBuf<double> d_gt;             // [max_stages] GridInfo::t of a fixed grid (rtoc_set_grid_times)
  std::vector<double> h_gt;        // host copy of the same, its size = the grid it belongs to (empty: none)
  DevBuf<double> d_gt_inst;        // [batch][max_stages] per-instance grid times written by sto_time_steps_kernel, or unallocated
  // reference tables of RTOC_REF_TABLE terms (rtoc_set_task_ref_table), by term index: capacity [max_stages] or [batch][max_stages],
  // in use [nstages] or [batch][nstages]; reftab_n[k] = the nstages table k was set for (0: none), bit k of reftab_inst: per instance
  DevBuf<rtoc_task_ref_entry> d_reftab[RTOC_MAX_TASK_COSTS];
  int reftab_n[RTOC_MAX_TASK_COSTS] = {};
  unsigned reftab_inst = 0;
  int task_rows = 0, task_ext = 0; // LDS rows of the term lists (the largest instance), 1: a 6D term or a table reference among them
  DevBuf<double> d_ls_merit;   // [batch] penalty parameter + [batch] directional derivative
  double ls_unconstr_dt = 0.0; // > 0: the last evalKKT was rtoc_unconstr_eval_kkt(dt) -- trial iterates of the line search are evaluated by it
  DevBuf<double> d_eval;       // [2][2][batch]: (cost + barrier | violation) of the current iterate, of the trial iterate
  DevBuf<double> d_eval_part;  // [batch][max_stages][2]
  DevBuf<double> d_sol_trial;  // trial iterate: SplitSolution records, constraint records, steps
  DevBuf<double> d_con_trial;
  DevBuf<double> d_ls_steps;   // [batch][2] trial steps + [batch] alpha
  DevBuf<int> d_ls_active;     // [batch] active flags + [1] counter
  int ls_trials = 0;           // trial evaluations of the last line search
  // RTOC_OPT_GRAPH: the captured launch sequences.  Declared last: destroyed before the memory their nodes name is freed
  GraphSlot g_sweep, g_newton;
};

extern "C" {

int rtoc_version(void) { return 100; }

int rtoc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- streaming kernels of rtoc_bandwidth_probe: chunk = (block-wave) + k * (waves in the launch), 1 KB per wave-instruction ----
extern "C++" {
template <int U, bool COPY>
static __global__ __launch_bounds__(256) void stream_probe_kernel(const char* __restrict__ src, char* __restrict__ dst, size_t chunks,
                                                                  double* sink) {
  const size_t nwaves = (size_t)gridDim.x * 4, w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  for (size_t c = w; c + (U - 1) * nwaves < chunks; c += U * nwaves) {
    d2 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = *reinterpret_cast<const d2*>(src + (c + k * nwaves) * 1024 + lane * 16);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (COPY) *reinterpret_cast<d2*>(dst + (c + k * nwaves) * 1024 + lane * 16) = v[k];
      else acc += v[k][0] + v[k][1];
    }
  }
  if (!COPY && acc == 1234.5) sink[w] = acc;
}
}  // extern "C++"

int rtoc_bandwidth_probe(int device, size_t bytes, double* read_gbs, double* copy_gbs) {
  constexpr int blocks = 256 * 64;                             // 64 workgroups of 4 waves per CU: 6.2 TB/s read (256 * 8: 5.7)
  constexpr size_t per = (size_t)blocks * 4 * 8;               // chunks consumed per trip of all waves (U = 8)
  static_assert(per * 1024 == RTOC_BANDWIDTH_PROBE_MIN_BYTES, "include/rtoc.h states the probe's minimum size: one trip of every wave");
  if (bytes < per * 1024) return RTOC_ERR_BAD_ARG;             // RTOC_BANDWIDTH_PROBE_MIN_BYTES: one trip of every wave (512 MiB)
  HIP_TRY(hipSetDevice(device));
  const size_t chunks = (bytes / 1024) / per * per;
  DevBuf<char> src, dst;
  DevBuf<double> sink;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = src.reserve(chunks * 1024);
  if (e == hipSuccess) e = dst.reserve(chunks * 1024);
  if (e == hipSuccess) e = sink.reserve((size_t)blocks * 4);
  if (e == hipSuccess) e = hipMemset(src.p, 0, chunks * 1024);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  double best[2] = {0.0, 0.0};
  for (int mode = 0; mode < 2 && e == hipSuccess; ++mode)
    for (int rep = 0; rep < 6 && e == hipSuccess; ++rep) {   // the first launch warms up
      (void)hipEventRecord(e0, nullptr);
      if (mode == 0) hipLaunchKernelGGL((stream_probe_kernel<8, false>), dim3(blocks), dim3(256), 0, nullptr, src.p, dst.p, chunks, sink.p);
      else hipLaunchKernelGGL((stream_probe_kernel<8, true>), dim3(blocks), dim3(256), 0, nullptr, src.p, dst.p, chunks, sink.p);
      (void)hipEventRecord(e1, nullptr);
      e = hipEventSynchronize(e1);
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      const double gbs = (mode + 1) * (double)chunks * 1024.0 / (ms * 1e-3) / 1e9;
      if (rep > 0 && gbs > best[mode]) best[mode] = gbs;
    }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess) {
    ctx_set_err(e, __LINE__);
    return RTOC_ERR_HIP;
  }
  if (read_gbs) *read_gbs = best[0];
  if (copy_gbs) *copy_gbs = best[1];
  return RTOC_OK;
}

int rtoc_dims_supported(const rtoc_dims* dims) { return dims && find_set(dims) ? 1 : 0; }

void rtoc_layout_for_dims(const rtoc_dims* dims, rtoc_layout* out) { rtoc_compute_layout(dims, out); }

const char* rtoc_error_string(int code) {
  switch (code) {
    case RTOC_OK: return "ok";
    case RTOC_ERR_BAD_ARG: return "bad argument";
    case RTOC_ERR_UNSUPPORTED_DIMS: return "no kernel specialisation for these dimensions";
    case RTOC_ERR_NO_DEVICE: return "no HIP device (the HIP path has no CPU fallback)";
    case RTOC_ERR_HIP: return g_errbuf;
    case RTOC_ERR_NOT_READY: return "grid not set";
    case RTOC_ERR_RCCL: return "RCCL error";
    case RTOC_ERR_IO: return "stage dump: file error or malformed file";
    default: return "unknown";
  }
}

// doubles of buffer b that the kernels index on a horizon of `stages` grid points: max_stages gives what is allocated
// (rtoc_buffer_count), nstages what a stage dump holds
static size_t buffer_count(const rtoc_ctx* c, int b, int stages) {
  const size_t per = (size_t)c->batch * stages;
  switch (b) {
    case RTOC_BUF_KKT: return per * c->L.kkt.stride;
    case RTOC_BUF_RIC: return per * c->L.ric.stride;
    case RTOC_BUF_DIR: return per * c->L.dir.stride;
    case RTOC_BUF_CDD: return per * c->L.cdd.stride;
    case RTOC_BUF_CON: return per * c->L.con.stride;
    case RTOC_BUF_DX0: return (size_t)c->batch * c->L.nx;
    case RTOC_BUF_STEP: return (size_t)c->batch * 2;
    case RTOC_BUF_SE3: return per * RTOC_SE3_STRIDE;
    case RTOC_BUF_CONE:   // none until rtoc_set_friction_cones / rtoc_set_wrench_cones
      if (c->cone_contacts <= 0) return 0;
      return per * (c->cone_rows == RTOC_WRENCH_ROWS ? rtoc_wrench_cone_stride(c->cone_contacts)
                                                     : rtoc_cone_stride(c->dims.nv, c->cone_contacts));
    case RTOC_BUF_SOL: return per * c->L.sol.stride;
    default: return 0;
  }
}

int rtoc_destroy(rtoc_ctx* c);
// everything of rtoc_create that can fail after the context object exists; the caller destroys the
// half-built context on failure (members that were never created are null)
static int create_members(rtoc_ctx* c, const rtoc_dims* dims, const KernelSet* ks, int max_stages, int batch, int device) {
  c->dims = *dims;
  rtoc_compute_layout(dims, &c->L);
  // the backward kernels carry their record offsets as immediates: they must be the ones the host
  // (and the caller, through rtoc_get_layout) uses
  if (memcmp(&ks->kl, &c->L.kkt, sizeof(rtoc_record_layout)) != 0 ||
      memcmp(&ks->rl, &c->L.ric, sizeof(rtoc_record_layout)) != 0 ||
      memcmp(&ks->dl, &c->L.dir, sizeof(rtoc_record_layout)) != 0 ||
      memcmp(&ks->cl, &c->L.cdd, sizeof(rtoc_record_layout)) != 0) {
    return RTOC_ERR_BAD_ARG;
  }
  c->ks = ks;
  c->max_stages = max_stages;
  c->batch = batch;
  c->device = device;
  c->bwd_variant = default_bwd_variant(ks);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    c->num_cus = cus;
  }
  if (const char* e = getenv("RTOC_CONDENSE_REGISTER")) c->cond_register = (e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
  HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  for (int i = 0; i < RTOC_MAX_CHUNK_EVENTS; ++i)
    HIP_TRY(hipEventCreateWithFlags(&c->ev_chunk[i], hipEventDisableTiming));
  c->condense_split = c->ks->cond_fused_default ? 0 : 1;   // per robot shape (rtoc.h: RTOC_OPT_CONDENSE_SPLIT)
  // RTOC_CONDENSE_SPLIT=0|1 in the environment: default of RTOC_OPT_CONDENSE_SPLIT for contexts created afterwards (runs the
  // whole test suite / bench on the other condensation pipeline without touching the callers)
  if (const char* e = getenv("RTOC_CONDENSE_SPLIT")) c->condense_split = (e[0] == '0') ? 0 : 1;
  for (int b = 0; b < RTOC_NUM_BUFFERS; ++b) c->want[b] = buffer_count(c, b, max_stages);
  // the CDD / CON buffers are large; they (and SE3, CONE, SOL) are allocated lazily on first use (upload / bind / condense)
  const int eager[] = {RTOC_BUF_KKT, RTOC_BUF_RIC, RTOC_BUF_DIR, RTOC_BUF_DX0, RTOC_BUF_STEP};
  for (int i : eager) {
    HIP_TRY(c->buf[i].reserve(c->want[i]));
    HIP_TRY(hipMemsetAsync(c->buf[i].p, 0, c->want[i] * sizeof(double), c->stream));
  }
  HIP_TRY(c->d_grid.reserve(max_stages));
  HIP_TRY(c->d_stage_list.reserve(max_stages));
  HIP_TRY(c->d_status.reserve(batch));
  HIP_TRY(hipMemsetAsync(c->d_status.p, 0, sizeof(uint32_t) * batch, c->stream));
  // dynamic LDS beyond the default limit: every kernel of the set whose descriptor asks for any (the forward kernel's grid table,
  // four bytes per grid point on top of none, stays under the default)
  hipError_t lds_err = hipSuccess;
  for_each_kernel(*ks, [&](const auto& k) {
    if (k && k.lds > 0 && lds_err == hipSuccess) lds_err = hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
  });
  HIP_TRY(lds_err);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_create(const rtoc_dims* dims, int max_stages, int batch, int device, rtoc_ctx** out) {
  if (!dims || !out || max_stages < 2 || batch < 1) return RTOC_ERR_BAD_ARG;
  const KernelSet* ks = find_set(dims);
  if (!ks) return RTOC_ERR_UNSUPPORTED_DIMS;
  if (rtoc_device_count() <= device || device < 0) return RTOC_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  rtoc_ctx* c = new (std::nothrow) rtoc_ctx();
  if (!c) return RTOC_ERR_BAD_ARG;
  c->device = device;
  int rc = create_members(c, dims, ks, max_stages, batch, device);
  if (rc) {
    (void)rtoc_destroy(c);
    return rc;
  }
  *out = c;
  return RTOC_OK;
}

// the stream drains first; then ~rtoc_ctx: the graph executables, every buffer, and last the streams and events (CtxStreams)
int rtoc_destroy(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
  return RTOC_OK;
}

int rtoc_set_grid(rtoc_ctx* c, const rtoc_grid* grid, int nstages);
int rtoc_set_constraint_rows(rtoc_ctx* c, const rtoc_box_row* rows, int nrows);
int rtoc_set_friction_cones(rtoc_ctx* c, int max_contacts, int contact_dim);
int rtoc_set_wrench_cones(rtoc_ctx* c, int max_contacts);
int rtoc_set_option(rtoc_ctx* c, int option, int64_t value);

int rtoc_clone(rtoc_ctx* c, rtoc_ctx** out) {
  if (!c || !out) return RTOC_ERR_BAD_ARG;
  rtoc_ctx* n = nullptr;
  int rc = rtoc_create(&c->dims, c->max_stages, c->batch, c->device, &n);
  if (rc) return rc;
  if (c->nstages >= 2 && !c->h_grid.empty()) rc = rtoc_set_grid(n, c->h_grid.data(), c->nstages);
  if (!rc && c->nrows > 0 && !c->h_rows.empty()) rc = rtoc_set_constraint_rows(n, c->h_rows.data(), c->nrows);
  if (!rc && c->cone_contacts > 0)
    rc = c->cone_rows == RTOC_WRENCH_ROWS ? rtoc_set_wrench_cones(n, c->cone_contacts)
                                          : rtoc_set_friction_cones(n, c->cone_contacts, c->cone_dim);
  if (!rc) {
    static_cast<CtxOptions&>(*n) = *c;
    if (c->backward_scan) rc = rtoc_set_option(n, RTOC_OPT_BACKWARD_SCAN, c->backward_scan);
  }
  hipError_t e = hipStreamSynchronize(c->stream);
  // the rigid-body model, contact schedule, cost, initial states, constraint bounds and line-search filters (rtoc_robot.h):
  // every buffer with the capacity it has in c, whatever part of it is in use
  auto dup = [&](auto& dst, const auto& src) {
    if (!rc && e == hipSuccess) e = dst.copy_from(src, n->stream);
  };
  if (!rc && c->h_model) {
    n->h_model.reset(new (std::nothrow) rbd::DevModel(*c->h_model));
    if (!n->h_model) rc = RTOC_ERR_HIP;
    dup(n->d_model, c->d_model);
    if (!rc && e == hipSuccess)
      e = set_linearize_lds(n->h_model->m, n->h_model->nlevels, n->h_model->nbranch, n->h_model->dpp);
  }
  dup(n->d_active, c->d_active);
  dup(n->d_cpos, c->d_cpos);
  dup(n->d_crot, c->d_crot);
  dup(n->d_cost, c->d_cost);
  dup(n->d_x0, c->d_x0);
  dup(n->d_bounds, c->d_bounds);
  dup(n->d_mu, c->d_mu);
  dup(n->d_wcone, c->d_wcone);
  if (c->d_filter.p) {
    dup(n->d_filter, c->d_filter);
    dup(n->d_nfilter, c->d_nfilter);
    dup(n->d_ls_in, c->d_ls_in);
    dup(n->d_ls_flags, c->d_ls_flags);
  }
  if (c->sto_on) {
    n->sto_on = 1, n->sto_nev = c->sto_nev, n->sto_t0 = c->sto_t0, n->sto_T = c->sto_T;
    n->sto_barrier = c->sto_barrier, n->sto_tau = c->sto_tau, n->sto_reg = c->sto_reg;
    dup(n->d_ts, c->d_ts);
    dup(n->d_dt, c->d_dt);
    dup(n->d_sto_con, c->d_sto_con);
    dup(n->d_min_dwell, c->d_min_dwell);
    dup(n->d_sto_cost, c->d_sto_cost);
    dup(n->d_sto_out, c->d_sto_out);
    dup(n->d_gt_inst, c->d_gt_inst);
  }
  if (c->ntasks > 0) {
    n->ntasks = c->ntasks, n->tasks_per_instance = c->tasks_per_instance;
    dup(n->d_tasks, c->d_tasks);
  }
  dup(n->d_gt, c->d_gt);
  if (!rc) n->h_gt = c->h_gt;
  n->task_rows = c->task_rows, n->task_ext = c->task_ext, n->reftab_inst = c->reftab_inst, n->h_task_table = c->h_task_table;
  for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) {
    n->reftab_n[k] = c->reftab_n[k];
    dup(n->d_reftab[k], c->d_reftab[k]);
  }
  for (int b = 0; b < RTOC_NUM_BUFFERS; ++b) {
    if (!c->buf[b].p) continue;
    n->want[b] = c->want[b];
    dup(n->buf[b], c->buf[b]);
  }
  dup(n->d_status, c->d_status);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(n->stream);
  if (rc || e != hipSuccess) {
    if (e != hipSuccess) ctx_set_err(e, __LINE__);
    (void)rtoc_destroy(n);
    return rc ? rc : RTOC_ERR_HIP;
  }
  *out = n;
  return RTOC_OK;
}

int rtoc_get_layout(const rtoc_ctx* c, rtoc_layout* out) {
  if (!c || !out) return RTOC_ERR_BAD_ARG;
  *out = c->L;
  return RTOC_OK;
}

int rtoc_set_grid(rtoc_ctx* c, const rtoc_grid* grid, int nstages) {
  if (!c || !grid || nstages < 2 || nstages > c->max_stages) return RTOC_ERR_BAD_ARG;
  if (grid[nstages - 1].type != RTOC_GRID_TERMINAL) return RTOC_ERR_BAD_ARG;
  for (int i = 0; i < nstages; ++i) {
    const rtoc_grid& g = grid[i];
    if (g.dims < 0 || g.dims > c->dims.ns_max || g.dimf < 0 || g.dimf > c->dims.nf_max)
      return RTOC_ERR_BAD_ARG;
    if (i < nstages - 1 && g.type == RTOC_GRID_TERMINAL) return RTOC_ERR_BAD_ARG;
    if (g.type == RTOC_GRID_IMPACT && (i == 0 || i >= nstages - 2)) return RTOC_ERR_BAD_ARG;
    if (g.type == RTOC_GRID_LIFT && i == 0) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->d_grid.p, grid, sizeof(rtoc_grid) * nstages, hipMemcpyHostToDevice, c->stream));
  {
    // the grid points a condensation launch covers, by kind (condense_rv_kernel takes the contact ones, condense_kernel the impact ones)
    std::vector<int> list;
    for (int i = 0; i + 1 < nstages; ++i)
      if (grid[i].type != RTOC_GRID_IMPACT) list.push_back(i);
    c->n_stage_contact = (int)list.size();
    for (int i = 0; i + 1 < nstages; ++i)
      if (grid[i].type == RTOC_GRID_IMPACT) list.push_back(i);
    c->n_stage_impact = (int)list.size() - c->n_stage_contact;
    HIP_TRY(hipMemcpyAsync(c->d_stage_list.p, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the pageable source dies with this scope)
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->h_grid.assign(grid, grid + nstages);
  c->nstages = nstages;
  c->fxx_state = 0;
  c->epoch++;
  if (c->sto_on) {  // the event times on the device belong to the previous grid structure unless the events are the same
    int nev = 0;
    for (int i = 0; i + 1 < nstages; ++i)
      if (grid[i].type == RTOC_GRID_IMPACT || grid[i].type == RTOC_GRID_LIFT) ++nev;
    if (nev != c->sto_nev) c->sto_on = 0;   // rtoc_sto_set_problem again
  }
  c->h_gt.clear();   // the grid times belong to the previous grid: rtoc_set_grid_times again
  for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) c->reftab_n[k] = 0;   // and so do the reference tables: rtoc_set_task_ref_table again
  return RTOC_OK;
}

int rtoc_set_stream(rtoc_ctx* c, void* s) {
  if (!c) return RTOC_ERR_BAD_ARG;
  c->epoch++;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return RTOC_OK;
}

static int ensure_scan_buffers(rtoc_ctx* c);
#define RTOC_SCAN_AUTO_MAX_BATCH 8  // measured on MI355X (profiles/r01_scan_batch_crossover.log): the scan wins up to ~16 ANYmal / ~10 iCub instances

// (re)plans the passes of the tangent walk for the context's model and sends the model to the device
static int apply_linearize_plan(rtoc_ctx* c) {
  rbd::DevModel* h = c->h_model.get();
  const int old_dpp = h->dpp;
  rbd::plan_passes(h, c->lin_dpp);
  if (rbd::lin_lds_bytes(h->nlevels, h->nbranch, h->m.njoints, h->m.ncontacts, h->m.nv, h->dpp, false) > 160 * 1024) {
    rbd::plan_passes(h, old_dpp);
    return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->d_model.p, h, sizeof(rbd::DevModel), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(set_linearize_lds(h->m, h->nlevels, h->nbranch, h->dpp));
  return RTOC_OK;
}

int rtoc_get_option(rtoc_ctx* c, int option, int64_t* value) {
  if (!c || !value) return RTOC_ERR_BAD_ARG;
  switch (option) {
    case RTOC_OPT_WRITEBACK_KKT: *value = c->writeback; return RTOC_OK;
    case RTOC_OPT_SWEEP_CHUNKS: *value = c->sweep_chunks; return RTOC_OK;
    case RTOC_OPT_CONDENSE_SPLIT: *value = c->condense_split; return RTOC_OK;
    case RTOC_OPT_BACKWARD_SCAN: *value = c->backward_scan; return RTOC_OK;
    case RTOC_OPT_CONDENSE_KEEP_QAF: *value = c->keep_qaf; return RTOC_OK;
    case RTOC_OPT_FXX_STRUCTURE: *value = c->fxx_mode; return RTOC_OK;
    case RTOC_OPT_GRAPH: *value = c->use_graph; return RTOC_OK;
    case RTOC_OPT_IMPACT_CONES: *value = c->impact_cones; return RTOC_OK;
    case RTOC_OPT_LINEARIZE_DOFS_PER_PASS: *value = c->h_model ? c->h_model->dpp : 0; return RTOC_OK;
    case RTOC_OPT_BACKWARD_REGISTER: *value = c->bwd_register; return RTOC_OK;
    case RTOC_OPT_CONDENSE_REGISTER: *value = c->cond_register; return RTOC_OK;
    case RTOC_OPT_BACKWARD_WAVES: *value = c->ks->bwd[c->bwd_variant].threads / 64; return RTOC_OK;
    case RTOC_OPT_SWITCHING_TRANSPORT: *value = c->exact_transport; return RTOC_OK;
    case RTOC_OPT_UNCONSTR_DENSE: *value = c->unconstr_dense; return RTOC_OK;
    case RTOC_OPT_LINEARIZE_FUSED: *value = c->linearize_fused; return RTOC_OK;
    case RTOC_OPT_CONE_JACOBIAN: *value = c->exact_cone_jacobian; return RTOC_OK;
    default: return RTOC_ERR_BAD_ARG;   // the double-valued options (RTOC_OPT_MAX_DTS0, RTOC_OPT_CONTACT_INV_DAMPING)
  }
}

int rtoc_set_option(rtoc_ctx* c, int option, int64_t value) {
  if (!c) return RTOC_ERR_BAD_ARG;
  c->epoch++;
  switch (option) {
    case RTOC_OPT_WRITEBACK_KKT:
      c->writeback = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_MAX_DTS0: {
      double d;
      memcpy(&d, &value, sizeof(d));
      if (!(d > 0.0)) return RTOC_ERR_BAD_ARG;
      c->max_dts0 = d;
      return RTOC_OK;
    }
    case RTOC_OPT_CONE_JACOBIAN:
      c->exact_cone_jacobian = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_LINEARIZE_FUSED:
      c->linearize_fused = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_LINEARIZE_DOFS_PER_PASS:
      if (value < 0 || value > rbd::LIN_MAX_DPP) return RTOC_ERR_BAD_ARG;
      {
        const int before = c->lin_dpp;
        c->lin_dpp = (int)value;
        const int rc = c->h_model ? apply_linearize_plan(c) : RTOC_OK;
        if (rc) c->lin_dpp = before;   // refused (LDS): the plan in force is the old one
        return rc;
      }
    case RTOC_OPT_UNCONSTR_DENSE:
      c->unconstr_dense = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_IMPACT_CONES:
      c->impact_cones = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_SWITCHING_TRANSPORT:
      c->exact_transport = value ? 1 : 0;
      return RTOC_OK;
    case RTOC_OPT_CONTACT_INV_DAMPING: {
      double d;
      memcpy(&d, &value, sizeof(d));
      if (!(d >= 0.0)) return RTOC_ERR_BAD_ARG;
      c->contact_inv_damping = d;
      return RTOC_OK;
    }
    case RTOC_OPT_BACKWARD_WAVES: {
      if (value == 0) {
        c->bwd_variant = default_bwd_variant(c->ks);
        return RTOC_OK;
      }
      for (int v = 0; v < c->ks->nvariants; ++v)
        if (c->ks->bwd[v].threads / 64 == (int)value) {
          c->bwd_variant = v;
          return RTOC_OK;
        }
      return RTOC_ERR_BAD_ARG;
    }
    case RTOC_OPT_CONDENSE_SPLIT:
      if (value != 0 && value != 1) return RTOC_ERR_BAD_ARG;
      c->condense_split = (int)value;
      return RTOC_OK;
    case RTOC_OPT_BACKWARD_REGISTER:
      if (value != 0 && value != 1 && value != 2) return RTOC_ERR_BAD_ARG;
      c->bwd_register = (int)value;
      return RTOC_OK;
    case RTOC_OPT_CONDENSE_REGISTER:
      if (value != 0 && value != 1 && value != 2) return RTOC_ERR_BAD_ARG;
      c->cond_register = (int)value;
      return RTOC_OK;
    case RTOC_OPT_GRAPH:
      if (value != 0 && value != 1) return RTOC_ERR_BAD_ARG;
      c->use_graph = (int)value;
      return RTOC_OK;
    case RTOC_OPT_FXX_STRUCTURE:
      if (value < 0 || value > 2) return RTOC_ERR_BAD_ARG;
      c->fxx_mode = (int)value;
      return RTOC_OK;
    case RTOC_OPT_CONDENSE_KEEP_QAF:
      if (value != 0 && value != 1) return RTOC_ERR_BAD_ARG;
      c->keep_qaf = (int)value;
      return RTOC_OK;
    case RTOC_OPT_SWEEP_CHUNKS:
      if (value < 1 || value > RTOC_MAX_CHUNK_EVENTS) return RTOC_ERR_BAD_ARG;
      c->sweep_chunks = (int)value;
      return RTOC_OK;
    case RTOC_OPT_BACKWARD_SCAN:
      if (value < 0 || value > 2) return RTOC_ERR_BAD_ARG;
      c->backward_scan = (int)value;
      // element / value-record buffers now, so that the launches themselves never allocate (stream capture)
      if (value != 0 && !(value == 2 && c->batch > RTOC_SCAN_AUTO_MAX_BATCH)) return ensure_scan_buffers(c);
      return RTOC_OK;
    default:
      return RTOC_ERR_BAD_ARG;
  }
}

static int ensure_buffer(rtoc_ctx* c, int b) {
  if (c->buf[b].p) return RTOC_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->buf[b].reserve(c->want[b]));
  HIP_TRY(hipMemsetAsync(c->buf[b].p, 0, c->want[b] * sizeof(double), c->stream));
  c->epoch++;
  return RTOC_OK;
}

// The context as the evalKKT-side kernels see it (record_view.hpp).  Taken at every launch and never kept: rtoc_bind and the
// trial iterate of the line search (eval_ocp_trial) change the pointers between launches.
static RecView view(const rtoc_ctx* c) {
  RecView v;
  v.sol = c->buf[RTOC_BUF_SOL].p, v.kkt = c->buf[RTOC_BUF_KKT].p, v.cdd = c->buf[RTOC_BUF_CDD].p, v.con = c->buf[RTOC_BUF_CON].p;
  v.dir = c->buf[RTOC_BUF_DIR].p, v.cone = c->buf[RTOC_BUF_CONE].p, v.se3 = c->buf[RTOC_BUF_SE3].p, v.dx0 = c->buf[RTOC_BUF_DX0].p;
  v.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  v.grid = c->d_grid.p, v.active = c->d_active.p;
  v.positions = c->has_cpos ? c->d_cpos.p : nullptr, v.rotations = c->has_crot ? c->d_crot.p : nullptr;
  v.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  v.model = c->d_model.p;
  v.nstages = c->nstages, v.batch = c->batch;
  v.L = c->L;
  return v;
}
// (c->h_model is set)
static ModelDims model_dims(const rtoc_ctx* c) {
  const rtoc_robot_model& m = c->h_model->m;
  ModelDims d;
  d.nq = m.nq, d.njoints = m.njoints, d.ncontacts = m.ncontacts;
  d.nlevels = c->h_model->nlevels, d.nbranch = c->h_model->nbranch, d.dpp = c->h_model->dpp;
  d.gs = 1;
  while (d.gs < m.njoints) d.gs *= 2;
  d.floating = m.type[0] == RTOC_JOINT_FREE_FLYER;
  d.gx = m.gravity[0], d.gy = m.gravity[1], d.gz = m.gravity[2];
  return d;
}
static bool grid_is_impact(const rtoc_grid& g) { return g.type == RTOC_GRID_IMPACT; }
static bool grid_has_switching(const rtoc_grid& g) { return g.switching_constraint != 0; }
// whether one of the first n grid points has the property
static bool any_grid_point(const rtoc_ctx* c, int n, bool (*has)(const rtoc_grid&)) {
  for (int i = 0; i < n; ++i)
    if (has(c->h_grid[i])) return true;
  return false;
}
// The non-terminal grid points with the property, for a kernel that is launched over them alone: their number, their indices in
// sel[16] -- or 0 if there are none or more than 16 (the launch then covers every grid point)
static int select_grid_points(const rtoc_ctx* c, bool (*has)(const rtoc_grid&), int* sel) {
  int k = 0;
  for (int i = 0; i + 1 < c->nstages; ++i)
    if (has(c->h_grid[i])) {
      if (k < 16) sel[k] = i;
      ++k;
    }
  return k <= 16 ? k : 0;
}

// the buffers that more than one entry point allocates on first use
static hipError_t reserve_active(rtoc_ctx* c, bool* fresh = nullptr) { return c->d_active.reserve(c->max_stages, fresh); }
static hipError_t reserve_costval(rtoc_ctx* c) { return c->d_costval.reserve((size_t)c->batch * c->max_stages); }
static hipError_t reserve_kkterr(rtoc_ctx* c) { return c->d_kkterr.reserve((size_t)c->batch * (1 + c->max_stages)); }

// switching-time optimisation on the device (sto.hpp): kernel arguments, one thread per instance
static int sto_count_events(const rtoc_ctx* c) {
  int n = 0;
  for (int i = 0; i + 1 < c->nstages; ++i)
    if (c->h_grid[i].type == RTOC_GRID_IMPACT || c->h_grid[i].type == RTOC_GRID_LIFT) ++n;
  return n;
}

static StoDevArgs sto_args(rtoc_ctx* c) {
  StoDevArgs a;
  memset(&a, 0, sizeof(a));
  const size_t ne = (size_t)c->batch * (c->sto_nev > 0 ? c->sto_nev : 1);
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.grid = c->d_grid.p;
  a.ts = c->d_ts.p;
  a.dt_inst = c->d_dt.p;
  a.t_inst = c->d_gt_inst.p;
  a.con = c->d_sto_con.p;
  a.min_dwell = c->d_min_dwell.p;
  a.cost_lt = c->d_sto_cost.p;
  a.cost_qtt = c->d_sto_cost.p ? c->d_sto_cost.p + ne : nullptr;
  a.lt = c->d_sto_out.p;
  a.qtt = c->d_sto_out.p + ne;
  a.err = c->d_sto_out.p + 2 * ne;
  a.kkterr = c->d_kkterr.p;
  a.steps = c->buf[RTOC_BUF_STEP].p;
  a.nstages = c->nstages, a.batch = c->batch, a.nev = c->sto_nev;
  a.kkt_stride = c->L.kkt.stride, a.scal_off = c->L.kkt.off[RTOC_KKT_SCAL];
  a.dir_stride = c->L.dir.stride, a.dts_off = c->L.dir.off[RTOC_DIR_DTS];
  a.t0 = c->sto_t0, a.T = c->sto_T, a.barrier = c->sto_barrier, a.tau = c->sto_tau, a.sto_reg = c->sto_reg;
  return a;
}
#define STO_LAUNCH(kernel, c)                                                                                   \
  do {                                                                                                          \
    hipLaunchKernelGGL(kernel, dim3(((c)->batch + 63) / 64), dim3(64), 0, (c)->stream, sto_args(c));            \
    HIP_TRY(hipGetLastError());                                                                                 \
  } while (0)

int rtoc_upload(rtoc_ctx* c, int buffer, size_t offset, const double* host, size_t count) {
  if (!c || buffer < 0 || buffer >= RTOC_NUM_BUFFERS || !host) return RTOC_ERR_BAD_ARG;
  if (count > c->want[buffer] || offset > c->want[buffer] - count) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, buffer);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->buf[buffer].p + offset, host, count * sizeof(double), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (buffer == RTOC_BUF_KKT) c->fxx_state = 0;  // re-checked by the next backward recursion (RTOC_OPT_FXX_STRUCTURE)
  if (buffer == RTOC_BUF_SOL) c->vals_fresh = 0;  // the pre-pass kinematics belong to the previous iterate
  return RTOC_OK;
}

int rtoc_download(rtoc_ctx* c, int buffer, size_t offset, double* host, size_t count) {
  if (!c || buffer < 0 || buffer >= RTOC_NUM_BUFFERS || !host) return RTOC_ERR_BAD_ARG;
  if (count > c->want[buffer] || offset > c->want[buffer] - count || !c->buf[buffer].p) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(host, c->buf[buffer].p + offset, count * sizeof(double), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

void* rtoc_device_ptr(rtoc_ctx* c, int buffer) {
  if (!c || buffer < 0 || buffer >= RTOC_NUM_BUFFERS) return nullptr;
  const bool fresh = !c->buf[buffer].p;
  if (ensure_buffer(c, buffer)) return nullptr;
  // the zero fill of a lazily allocated buffer runs on the context's stream: it must have landed before a
  // caller writes through the pointer on a stream of its own
  if (fresh && hipStreamSynchronize(c->stream) != hipSuccess) return nullptr;
  if (buffer == RTOC_BUF_KKT) {
    c->fxx_state = 0;  // the caller may write through the pointer
    c->kkt_exposed = true;
  }
  return c->buf[buffer].p;
}

size_t rtoc_buffer_count(const rtoc_ctx* c, int buffer) {
  if (!c || buffer < 0 || buffer >= RTOC_NUM_BUFFERS) return 0;
  return c->want[buffer];
}

int rtoc_bind(rtoc_ctx* c, int buffer, void* device_ptr) {
  if (!c || buffer < 0 || buffer >= RTOC_NUM_BUFFERS || !device_ptr) return RTOC_ERR_BAD_ARG;
  if (((uintptr_t)device_ptr & 63) != 0) return RTOC_ERR_BAD_ARG;  // records are 64 B aligned
  HIP_TRY(hipSetDevice(c->device));
  if (c->buf[buffer].owned && c->buf[buffer].p) HIP_TRY(hipStreamSynchronize(c->stream));   // ahead of the hipFree
  c->buf[buffer].bind((double*)device_ptr, c->want[buffer]);
  if (buffer == RTOC_BUF_KKT) c->fxx_state = 0;
  c->epoch++;
  return RTOC_OK;
}

// ---- hot path ---------------------------------------------------------------------------
// RTOC_OPT_BACKWARD_SCAN: the scan covers grids without switching-time optimisation; others take the serial kernel
static bool grid_has_sto(const rtoc_ctx* c) {
  for (int i = 0; i < c->nstages; ++i)
    if (c->h_grid[i].sto || c->h_grid[i].sto_next) return true;
  return false;
}
// the backward recursion: every grid (with switching-time optimisation: matrix scan + serial vector pass, riccati_scan_sto.hpp)
static bool scan_applies(const rtoc_ctx* c) {
  if (!c->backward_scan || c->h_grid.empty()) return false;
  if (c->backward_scan == 2 && c->batch > RTOC_SCAN_AUTO_MAX_BATCH) return false;  // auto: latency regime only
  if (c->nstages > SCAN_STO_MAX_STAGES && grid_has_sto(c)) return false;            // the vector pass keeps the grid in LDS
  return true;
}
// the forward recursion as a prefix scan: grids without switching-time optimisation (the dts chain is not a fixed affine map)
static bool forward_scan_applies(const rtoc_ctx* c) { return scan_applies(c) && !grid_has_sto(c); }

// Backward recursion as a horizon scan (riccati_scan.hpp): elements, log2 combination levels, then the
// policies of all grid points at once by the tile-split backward kernel in its one-stage mode.
static int ensure_scan_buffers(rtoc_ctx* c) {
  const KernelSet* ks = c->ks;
  const size_t per = (size_t)c->batch * c->max_stages;
  for (int i = 0; i < 3; ++i) HIP_TRY(c->d_scan[i].reserve(per * (i < 2 ? ks->scan_elt_stride : ks->scan_ps_stride)));
  if (grid_has_sto(c)) HIP_TRY(c->d_scan_sto.reserve(per * ks->sto_scr_stride));  // (grids with STO only)
  return RTOC_OK;
}

// the arguments every backward launch shares (the register-resident and register-wide paths run only without
// RTOC_OPT_WRITEBACK_KKT: writeback is set on the tile-split and scan paths alone)
static BwdArgs bwd_args(const rtoc_ctx* c, int first, int end) {
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.kkt_rw = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.grid = c->d_grid.p;
  a.status = c->d_status.p;
  a.prof = c->d_prof.p;
  a.nstages = c->nstages;
  a.batch = end;
  a.first = first;
  a.writeback = c->writeback;
  a.max_dts0 = c->max_dts0;
  return a;
}

static int launch_backward_scan(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  int rc0 = ensure_scan_buffers(c);
  if (rc0) return rc0;
  const int n = c->nstages, nb = end - first;
  ScanArgs s;
  s.kkt = c->buf[RTOC_BUF_KKT].p;
  s.grid = c->d_grid.p;
  s.status = c->d_status.p;
  s.src = c->d_scan[1].p;
  s.dst = c->d_scan[0].p;
  s.ps = c->d_scan[2].p;
  s.nstages = n;
  s.batch = end;
  s.first = first;
  s.dist = 0;
  launch(ks->scan_elt, dim3(n, nb), stream, s);
  int cur = 0;
  for (int d = 1; d < n; d *= 2) {
    s.src = c->d_scan[cur].p;
    s.dst = c->d_scan[cur ^ 1].p;
    s.dist = d;
    launch(ks->scan_comb, dim3(n - d, nb, 2), stream, s);
    cur ^= 1;
  }
  BwdArgs a = bwd_args(c, first, end);
  a.prof = nullptr;
  a.scan_ps = c->d_scan[2].p;
  a.scan_ps_stride = ks->scan_ps_stride;
  a.scan_ps_soff = ks->scan_ps_soff;
  const bool sto = grid_has_sto(c);
  StoScanArgs t;
  // Grids with switching-time optimisation: the bundles of the vector pass (everything of the vector recursion that does not depend
  // on the chain) are prepared by n - 1 more workgroups per instance of the SAME launch -- unless the policy workgroups write the
  // mutated Quu, lu back into the KKT records (RTOC_OPT_WRITEBACK_KKT), which the preparation reads: then it runs first, by itself.
  const bool ride = sto && !c->writeback && ks->sto_prep.lds <= p.kern->lds;
  if (sto) {
    t.kkt = c->buf[RTOC_BUF_KKT].p, t.ric = c->buf[RTOC_BUF_RIC].p, t.grid = c->d_grid.p, t.status = c->d_status.p;
    t.ps = c->d_scan[2].p, t.scr = c->d_scan_sto.p;
    t.nstages = n, t.batch = end, t.first = first, t.max_dts0 = c->max_dts0, t.prof = c->d_prof.p;
    if (!ride) launch(ks->sto_prep, dim3(n - 1, nb), stream, t);
  }
  a.sto_scr = ride ? c->d_scan_sto.p : nullptr;
  launch(*p.kern, dim3(nb, ride ? 2 * n - 1 : n), stream, a);
  if (sto) launch(ks->sto_vec, dim3(nb), stream, t);   // s, k, m, the STO quantities
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// RTOC_OPT_FXX_STRUCTURE: may the structure-exploiting backward kernel run on the resident records?
static int check_fxx(rtoc_ctx* c) {
  HIP_TRY(c->d_fxx_flag.reserve(1));
  HIP_TRY(hipMemsetAsync(c->d_fxx_flag.p, 0, sizeof(int), c->stream));
  FxxCheckArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.grid = c->d_grid.p;
  a.flag = c->d_fxx_flag.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nv = c->dims.nv;
  a.np = c->dims.np;
  a.fxx_off = c->L.kkt.off[RTOC_KKT_FXX];
  a.stride = c->L.kkt.stride;
  hipLaunchKernelGGL(fxx_structure_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  int bad = 1;
  HIP_TRY(hipMemcpyAsync(&bad, c->d_fxx_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->fxx_state = bad ? 2 : 1;
  return RTOC_OK;
}

// The backward recursion of one public call: the horizon scan (RTOC_OPT_BACKWARD_SCAN), else (RTOC_OPT_BACKWARD_REGISTER) the
// register-resident kernel (riccati_backward_rv.hpp, one launch per horizon; on grids with switching-time optimisation its STO form,
// structured Fxx only), else on the iCub-size shapes the register-wide kernel (riccati_backward_rw.hpp, structured Fxx only; with 1
// on batches of more instances than CUs -- below that the tile-split kernel's four waves per instance finish a horizon sooner --,
// with 2 always), else the tile-split / role-split kernel.  The only code that checks the records (it synchronises) or resets
// fxx_state: the entry points call it once, before any capture, and hand the plan to the launchers.
static int plan_backward(rtoc_ctx* c, BwdPlan* out) {
  const KernelSet* ks = c->ks;
  // the register kernels: the default variant only (an explicit RTOC_OPT_BACKWARD_WAVES keeps its kernel)
  const bool reg = c->bwd_register && !c->h_grid.empty() && c->nstages >= 2 && c->nstages <= RV_MAX_STAGES && !c->writeback &&
                   c->bwd_variant == default_bwd_variant(ks);
  const bool sto = reg && grid_has_sto(c);
  const bool rw = reg && ks->bwd_rw && !sto && (c->bwd_register >= 2 || c->batch > c->num_cus);
  // the caller may have rewritten the records since the runtime last saw them (a bound buffer, or its pointer handed out)
  const bool rewritable = c->fxx_mode == 0 && (!c->buf[RTOC_BUF_KKT].owned || c->kkt_exposed);
  int rc = RTOC_OK;
  auto structured = [&]() {   // a structured kernel to choose, and the records have the structure
    if (!((ks->bwd_sa && c->bwd_variant == 3) || rw) || c->fxx_mode == 1) return false;
    if (c->fxx_mode == 2) return true;
    if (c->fxx_state == 0 && rc == RTOC_OK) rc = check_fxx(c);
    return c->fxx_state == 1;
  };
  BwdPlan p = {BWD_TILE, nullptr, 0};
  if (scan_applies(c)) {
    p = {BWD_SCAN, &ks->bwd[ks->scan_policy_variant], 0};
  } else if (reg && ks->bwd_rv && (!sto || (ks->bwd_rv_sto && structured()))) {
    p.path = BWD_RV;
    p.kern = sto ? &ks->bwd_rv_sto : (ks->bwd_rv_sa && structured()) ? &ks->bwd_rv_sa : &ks->bwd_rv;
    // a rewritable buffer may have changed since the check that chose the structured form: the kernel verifies as it goes
    p.check_fxx = (p.kern != &ks->bwd_rv && rewritable) ? 1 : 0;
  } else {
    // the register-wide kernel never loads the structured rows of Fxx, so it cannot verify them: check them for every call
    if (rw && rewritable) c->fxx_state = 0;
    const bool s = structured();
    p.path = (rw && s) ? BWD_RW : BWD_TILE;
    p.kern = (rw && s) ? &ks->bwd_rw : s ? &ks->bwd_sa : &ks->bwd[c->bwd_variant];
  }
  if (rc) return rc;
  // the plan is part of a captured graph: a new epoch when it changes, not whenever the records are checked again
  if (p.path != c->bwd_plan.path || p.kern != c->bwd_plan.kern || p.check_fxx != c->bwd_plan.check_fxx) c->epoch++;
  c->bwd_plan = *out = p;
  return RTOC_OK;
}

static int launch_backward_rv(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const int N = c->nstages - 1;
  BwdArgs a = bwd_args(c, first, end);
  // one launch for the whole horizon: regular, lift, impact and switching-constraint grid points are all the kernel's own
  a.seg_hi = N - 1;
  a.seg_lo = 0;
  a.check_fxx = p.check_fxx;
#ifdef RTOC_RV_DEBUG_MASK
  if (const char* e = getenv("RTOC_RV_DEBUG")) a.scan_ps_soff = atoi(e);
#endif
  if (N >= 1) launch(*p.kern, dim3(end - first), stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_rw(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  const int N = c->nstages - 1, nb = end - first;
  BwdArgs a = bwd_args(c, first, end);
  auto constrained = [&](int st) { return c->h_grid[st].type != RTOC_GRID_IMPACT && c->h_grid[st].dims > 0; };
  auto one_stage = [&](int st) {   // tile-split kernel, grid point st only (st == N: the terminal record)
    BwdArgs o = a;
    o.scan_ps = c->buf[RTOC_BUF_RIC].p + c->L.ric.off[RTOC_RIC_P];
    o.scan_ps_stride = c->L.ric.stride;
    o.scan_ps_soff = c->L.ric.off[RTOC_RIC_S] - c->L.ric.off[RTOC_RIC_P];
    o.seg_hi = o.seg_lo = st;
    launch(ks->bwd[ks->scan_policy_variant], dim3(nb, 1), stream, o);
  };
  if (N == 0 || constrained(N - 1)) one_stage(N);   // nobody else writes the terminal record then
  int hi = N - 1;
  while (hi >= 0) {
    if (constrained(hi)) {
      one_stage(hi);
      --hi;
      continue;
    }
    int lo = hi;
    while (lo > 0 && !constrained(lo - 1)) --lo;
    a.seg_hi = hi;
    a.seg_lo = lo;
    launch(*p.kern, dim3(nb), stream, a);
    hi = lo - 1;
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_tile(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  launch(*p.kern, dim3((end - first + p.kern->inst - 1) / p.kern->inst), stream, bwd_args(c, first, end));
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_range(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  switch (p.path) {
    case BWD_SCAN: return launch_backward_scan(c, p, first, end, stream);
    case BWD_RV: return launch_backward_rv(c, p, first, end, stream);
    case BWD_RW: return launch_backward_rw(c, p, first, end, stream);
    default: return launch_backward_tile(c, p, first, end, stream);
  }
}
static int launch_backward(rtoc_ctx* c, const BwdPlan& p) { return launch_backward_range(c, p, 0, c->batch, c->stream); }

// Forward recursion as a prefix scan of the closed-loop maps (riccati_scan.hpp): maps of all grid points,
// log2 composition levels (dx of every grid point), then du / dlmdgmm / dxi of all grid points at once.
static int launch_forward_scan(rtoc_ctx* c, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  int rc0 = ensure_scan_buffers(c);
  if (rc0) return rc0;
  const int n = c->nstages, nb = end - first, N = n - 1;
  FwdScanArgs s;
  s.kkt = c->buf[RTOC_BUF_KKT].p;
  s.ric = c->buf[RTOC_BUF_RIC].p;
  s.dir = c->buf[RTOC_BUF_DIR].p;
  s.dx0 = c->buf[RTOC_BUF_DX0].p;
  s.grid = c->d_grid.p;
  s.src = c->d_scan[1].p;
  s.dst = c->d_scan[0].p;
  s.nstages = n;
  s.batch = end;
  s.first = first;
  s.dist = 0;
  launch(ks->fscan_elt, dim3(N, nb), stream, s);
  int cur = 0;
  for (int d = 1; d < N; d *= 2) {
    s.src = c->d_scan[cur].p;
    s.dst = c->d_scan[cur ^ 1].p;
    s.dist = d;
    launch(ks->fscan_comb, dim3(N - d, nb), stream, s);
    cur ^= 1;
  }
  launch(ks->fscan_fin, dim3(n, nb), stream, s);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_forward_range(rtoc_ctx* c, int first, int end, hipStream_t stream) {
  if (forward_scan_applies(c)) return launch_forward_scan(c, first, end, stream);
  FwdArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.dx0 = c->buf[RTOC_BUF_DX0].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = end;
  a.first = first;
  // (a structured-Fxx form of this kernel -- top half of Fxx not read, 15 % fewer bytes -- was measured at 1.27 vs
  // 1.28 ms: the kernel is bound by its load queue, not by the bytes it requests; not kept)
  launch(c->ks->fwd, dim3(end - first), stream, a, ((a.nstages + 3) & ~3) * (int)sizeof(int));  // grid table in LDS
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}
static int launch_forward(rtoc_ctx* c) { return launch_forward_range(c, 0, c->batch, c->stream); }

// Backward + forward sweep of the whole batch as a two-stream pipeline over instance chunks: the
// forward recursion of chunk i (HBM-bound, a few small waves per CU) runs under the backward
// recursion of chunk i+1 (MFMA / LDS-bound, leaves most of the HBM bandwidth idle).  Results are
// those of rtoc_riccati_backward followed by rtoc_riccati_forward.
static int launch_sweep(rtoc_ctx* c, const BwdPlan& p) {
  const int nch = (c->sweep_chunks > 0) ? c->sweep_chunks : 1;
  if (nch == 1 || p.path == BWD_SCAN) {  // the scan's element buffers are not chunked
    int rc = launch_backward(c, p);
    return rc ? rc : launch_forward(c);
  }
  const int per = (((c->batch + nch - 1) / nch) + 3) & ~3;  // whole 4-instance workgroups
  HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
  HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  for (int i = 0; i * per < c->batch; ++i) {
    const int first = i * per, end = (first + per < c->batch) ? first + per : c->batch;
    int rc = launch_backward_range(c, p, first, end, c->stream);
    if (rc) return rc;
    hipEvent_t e = c->ev_chunk[i % RTOC_MAX_CHUNK_EVENTS];
    HIP_TRY(hipEventRecord(e, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, e, 0));
    rc = launch_forward_range(c, first, end, c->stream2);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return RTOC_OK;
}

// RTOC_OPT_CONDENSE_REGISTER: the contact grid points by condense_rv_kernel (one wave per work item, products chained through
// registers), the impact grid points by condense_kernel.  Measured per 4096 ANYmal trot instances: 4.80 -> 4.00 ms without rows,
// 5.16 -> 4.55 ms with 72 joint-limit rows and 4 friction cones.
// friction cones of point contacts are condensed INSIDE condense_rv_kernel (their Gram product's tiles go straight into the seeds and
// operands of the condensation); wrench cones need their own kernel ahead of it
static bool cond_rv_fuses_cones(const rtoc_ctx* c) {
  return c->cone_contacts > 0 && c->cone_rows == RTOC_FRICTION_ROWS && c->cone_dim == 3 && c->ks->cond_fuses_cones && c->ks->cond_rv_cones;
}
static bool cond_register_applies(const rtoc_ctx* c) {
  if (!c->cond_register || !c->ks->cond_rv || c->condense_split || c->keep_qaf) return false;
  if (c->cone_contacts > 0 && !cond_rv_fuses_cones(c) && c->cond_register < 2) return false;
  return c->n_stage_contact + c->n_stage_impact == c->nstages - 1;
}

static int launch_condense(rtoc_ctx* c) {
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  CondArgs a;
  a.stage_list = nullptr;
  a.nlist = 0;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.grid = c->d_grid.p;
  a.status = c->d_status.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.damping = c->contact_inv_damping;
  a.prof = c->d_prof.p;
  a.con = (c->nrows > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.rows = c->d_rows.p;
  a.entry = c->d_entry.p;
  a.pair = reinterpret_cast<const int4*>(c->d_pair.p);
  a.nrows = c->nrows;
  a.nl = c->L.con;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  const int nblocks = c->batch * (c->nstages - 1);
  a.cone_rows = 0;
  a.keep_qaf = c->keep_qaf;
  a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  const bool rv = cond_register_applies(c);
  if ((rv ? cond_rv_fuses_cones(c) : (c->condense_split || c->ks->cond_fuses_cones)) && c->cone_contacts > 0) {  // the cone rows ride with the MJtJinv kernel / in wave 1 of the fused kernel / inside condense_rv_kernel
    if (!c->buf[RTOC_BUF_CONE].p || !c->buf[RTOC_BUF_CON].p) return RTOC_ERR_NOT_READY;
    const bool wrench = c->cone_rows == RTOC_WRENCH_ROWS;
    a.cone_rows = c->cone_rows;
    a.cone_con = c->buf[RTOC_BUF_CON].p;
    a.cone = c->buf[RTOC_BUF_CONE].p;
    a.cone_contacts = c->cone_contacts;
    a.cone_dim = c->cone_dim;
    a.cone_row0 = c->dims.nc_max - c->cone_rows * c->cone_contacts;
    a.cone_stride = wrench ? rtoc_wrench_cone_stride(c->cone_contacts) : rtoc_cone_stride(c->dims.nv, c->cone_contacts);
    a.cone_dgdf_off = rtoc_cone_dgdf_off(c->dims.nv, c->cone_contacts);
    a.cone_impact = c->impact_cones;
  }
  if (rv) {
    a.stage_list = c->d_stage_list.p;
    a.nlist = c->n_stage_contact;
#ifdef RTOC_CRV_DEBUG_LDS_PAD   // occupancy experiments (debug builds only): extra dynamic LDS per work item, clamped to what a launch accepts
    static const int lds_pad_env = getenv("RTOC_CRV_LDS_PAD") ? atoi(getenv("RTOC_CRV_LDS_PAD")) : 0;
    const int lds_room = 64 * 1024 - c->ks->cond_rv.lds;
    const int lds_pad = lds_pad_env < 0 ? 0 : (lds_pad_env > lds_room ? lds_room : lds_pad_env);
#else
    constexpr int lds_pad = 0;
#endif
    if (a.nlist > 0) {
      launch(a.cone_rows ? c->ks->cond_rv : c->ks->cond_rv_nc, dim3(c->batch * a.nlist), c->stream, a, lds_pad);
      HIP_TRY(hipGetLastError());
    }
    a.stage_list = c->d_stage_list.p + c->n_stage_contact;
    a.nlist = c->n_stage_impact;
    if (a.nlist > 0) launch(c->ks->cond, dim3(c->batch * a.nlist), c->stream, a);
  } else if (c->condense_split) {
    launch(c->ks->mjt, dim3(nblocks), c->stream, a);
    launch(c->ks->cond_split, dim3(nblocks), c->stream, a);
  } else {
    launch(c->ks->cond, dim3(nblocks), c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_expand(rtoc_ctx* c, double tau) {
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  ExpArgs a;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.cl = c->L.cdd;
  a.dl = c->L.dir;
  a.tau = tau;
  a.con = (c->nrows > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.rows = c->d_rows.p;
  a.nrows = c->nrows;
  a.nl = c->L.con;
  a.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  a.prof = c->d_prof.p;
  hipLaunchKernelGGL(fill_steps_kernel, dim3((2 * c->batch + 255) / 256), dim3(256), 0, c->stream,
                     c->buf[RTOC_BUF_STEP].p, 2 * c->batch);
  const int nblocks = c->batch * (c->nstages - 1);
  launch(c->ks->expd, dim3(nblocks), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_cones(rtoc_ctx* c, int phase, double tau) {  // 0 condense, 1 expand, 2 update
  if (!c->buf[RTOC_BUF_CONE].p || !c->buf[RTOC_BUF_CON].p) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  ConeArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.con = c->buf[RTOC_BUF_CON].p;
  a.cone = c->buf[RTOC_BUF_CONE].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.grid = c->d_grid.p;
  a.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.max_contacts = c->cone_contacts;
  a.contact_dim = c->cone_dim;
  a.prof = nullptr;
  const bool wrench = c->cone_rows == RTOC_WRENCH_ROWS;
  a.rows_per_contact = c->cone_rows;
  a.row0 = c->dims.nc_max - c->cone_rows * c->cone_contacts;
  a.cone_stride = wrench ? rtoc_wrench_cone_stride(c->cone_contacts) : rtoc_cone_stride(c->dims.nv, c->cone_contacts);
  a.dgdf_off = rtoc_cone_dgdf_off(c->dims.nv, c->cone_contacts);
  a.impact_cones = c->impact_cones;
  a.tau = tau;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  a.nl = c->L.con;
  a.dl = c->L.dir;
  const dim3 grid(c->batch * (c->nstages - 1));
  if (phase == 0)
    launch(wrench ? c->ks->wcond : c->ks->ccond, grid, c->stream, a);
  else if (phase == 1)
    launch(wrench ? c->ks->wexp : c->ks->cexp, grid, c->stream, a);
  else
    hipLaunchKernelGGL(cone_update_kernel, grid, dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

#define CHECK_READY(c)                       \
  if (!(c)) return RTOC_ERR_BAD_ARG;         \
  if ((c)->nstages < 2) return RTOC_ERR_NOT_READY; \
  HIP_TRY(hipSetDevice((c)->device));

static int launch_state_correction(rtoc_ctx* c, int mode) {
  if (!c->buf[RTOC_BUF_SE3].p) return RTOC_ERR_BAD_ARG;
  SeArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.dx0 = c->buf[RTOC_BUF_DX0].p;
  a.se3 = c->buf[RTOC_BUF_SE3].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.kl = c->L.kkt;
  a.dl = c->L.dir;
  a.nx = c->L.nx;
  a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  const int nblocks = (mode == 2) ? c->batch : c->batch * c->nstages;
  if (mode == 0)
    hipLaunchKernelGGL(state_correction_kernel<0>, dim3(nblocks), dim3(64), 0, c->stream, a);
  else if (mode == 1)
    hipLaunchKernelGGL(state_correction_kernel<1>, dim3(nblocks), dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(state_correction_kernel<2>, dim3(nblocks), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_correct_state_equation(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;  // floating base only (hasFloatingBase())
  return launch_state_correction(c, 0);
}

int rtoc_correct_costate_direction(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  return launch_state_correction(c, 1);
}

int rtoc_compute_initial_state_direction(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  return launch_state_correction(c, 2);
}

int rtoc_condense(rtoc_ctx* c) {
  CHECK_READY(c);
  int rc = RTOC_OK;
  if (c->cone_contacts > 0 && (cond_register_applies(c) ? !cond_rv_fuses_cones(c) : (!c->condense_split && !c->ks->cond_fuses_cones)))
    rc = launch_cones(c, 0, 0.0);  // Constraints::condenseSlackAndDual first
  if (!rc) rc = launch_condense(c);
  if (!rc && c->buf[RTOC_BUF_SE3].p && c->dims.np == 6) rc = launch_state_correction(c, 0);
  return rc;
}

int rtoc_riccati_backward(rtoc_ctx* c) {
  CHECK_READY(c);
  BwdPlan p;
  int rc = plan_backward(c, &p);
  return rc ? rc : launch_backward(c, p);
}

int rtoc_riccati_forward(rtoc_ctx* c) {
  CHECK_READY(c);
  return launch_forward(c);
}

// RTOC_OPT_GRAPH: run `body` (a sequence of kernel launches on c->stream, no allocation, no synchronisation; its backward plan
// resolved by the caller) from a captured hipGraph.  The first call at a given configuration epoch runs it plainly (lazy allocations happen there),
// the second captures and instantiates, later calls are one hipGraphLaunch -- a single-OCP Newton iteration is ~25
// small kernels, whose launch gaps are a third of its latency.
extern "C++" {
template <class Body>
static int run_graphed(rtoc_ctx* c, GraphSlot* g, double p0, double p1, Body body) {
  if (!c->use_graph) return body();
  if (g->exec && g->epoch == c->epoch && g->p0 == p0 && g->p1 == p1) {
    HIP_TRY(hipGraphLaunch(g->exec, c->stream));
    c->graph_replays++;
    return RTOC_OK;
  }
  if (!(g->warm && g->warm_epoch == c->epoch)) {
    const int rc = body();
    g->warm = true;
    g->warm_epoch = c->epoch;  // after the body: its lazy allocations bump the epoch
    return rc;
  }
  if (g->exec) {
    (void)hipGraphExecDestroy(g->exec);
    g->exec = nullptr;
  }
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
  const int rc = body();
  const hipError_t e = hipStreamEndCapture(c->stream, &graph);
  if (rc || e != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    if (e != hipSuccess) ctx_set_err(e, __LINE__);
    return rc ? rc : RTOC_ERR_HIP;
  }
  const hipError_t e2 = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e2 != hipSuccess) {
    g->exec = nullptr;
    ctx_set_err(e2, __LINE__);
    return RTOC_ERR_HIP;
  }
  g->epoch = c->epoch;
  g->p0 = p0;
  g->p1 = p1;
  HIP_TRY(hipGraphLaunch(g->exec, c->stream));
  c->graph_replays++;
  return RTOC_OK;
}
}  // extern "C++"

int rtoc_graph_replay_count(rtoc_ctx* c, unsigned long long* out) {
  if (!c || !out) return RTOC_ERR_BAD_ARG;
  *out = c->graph_replays;
  return RTOC_OK;
}

int rtoc_riccati_sweep(rtoc_ctx* c) {
  CHECK_READY(c);
  BwdPlan p;
  int rc = plan_backward(c, &p);
  return rc ? rc : run_graphed(c, &c->g_sweep, 0.0, 0.0, [&]() { return launch_sweep(c, p); });
}

static int launch_fill(rtoc_ctx* c, double dt) {
  FillArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.dt = dt;
  a.kl = c->L.kkt;
  launch(c->ks->fill, dim3(c->batch * c->nstages), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// UnconstrRiccatiRecursion in its structured form (unconstr_riccati.hpp): whenever the shape has the kernels and the
// horizon scan is not asked for (the scan works on the general elements, i.e. on materialised A, B)
static bool unconstr_structured(const rtoc_ctx* c) {
  return c->ks->ubwd && c->dims.nf_max == 0 && !scan_applies(c) && !c->unconstr_dense;
}
static int launch_unconstr_riccati(rtoc_ctx* c, double dt, bool forward) {
  int rc = ensure_buffer(c, RTOC_BUF_RIC);
  if (!rc && forward) rc = ensure_buffer(c, RTOC_BUF_DIR);
  if (rc) return rc;
  if (!c->buf[RTOC_BUF_KKT].p) return RTOC_ERR_NOT_READY;
  UrArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.kkt_rw = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.dx0 = c->buf[RTOC_BUF_DX0].p;
  a.status = c->d_status.p;
  a.nstages = c->nstages, a.batch = c->batch, a.writeback = c->writeback;
  a.dt = dt;
  a.kl = c->L.kkt, a.rl = c->L.ric, a.dl = c->L.dir;
  launch(forward ? c->ks->ufwd : c->ks->ubwd, dim3(c->batch), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_unconstr_backward(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (c->dims.nu != c->dims.nv || !(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (unconstr_structured(c)) return launch_unconstr_riccati(c, dt, false);
  BwdPlan p;
  int rc = launch_fill(c, dt);
  if (!rc) rc = plan_backward(c, &p);
  return rc ? rc : launch_backward(c, p);
}

static int launch_unconstr_dynamics(rtoc_ctx* c, bool expand, double dt) {
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  UdArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.dt = dt;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  a.dl = c->L.dir;
  launch(expand ? c->ks->uexp : c->ks->ucond, dim3(c->batch * (c->nstages - 1)), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_unconstr_condense(rtoc_ctx* c) {
  CHECK_READY(c);
  return launch_unconstr_dynamics(c, false, 1.0);
}

int rtoc_unconstr_expand(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (!(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  return launch_unconstr_dynamics(c, true, dt);
}

int rtoc_unconstr_forward(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (c->dims.nu != c->dims.nv || !(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (unconstr_structured(c)) return launch_unconstr_riccati(c, dt, true);
  return launch_forward(c);
}

int rtoc_expand(rtoc_ctx* c, double tau) {
  CHECK_READY(c);
  if (!(tau > 0.0 && tau <= 1.0)) return RTOC_ERR_BAD_ARG;
  int rc = launch_expand(c, tau);
  if (!rc && c->cone_contacts > 0) rc = launch_cones(c, 1, tau);
  if (!rc && c->buf[RTOC_BUF_SE3].p && c->dims.np == 6) rc = launch_state_correction(c, 1);
  return rc;
}

int rtoc_update(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->cone_contacts > 0) {
    int rc = launch_cones(c, 2, 0.0);
    if (rc) return rc;
  }
  if (c->nrows == 0) return RTOC_OK;
  UpdArgs a;
  a.con = c->buf[RTOC_BUF_CON].p;
  a.rows = c->d_rows.p;
  a.grid = c->d_grid.p;
  a.steps = c->buf[RTOC_BUF_STEP].p;
  a.nrows = c->nrows;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nl = c->L.con;
  hipLaunchKernelGGL(pdipm_update_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int set_cones(rtoc_ctx* c, int max_contacts, int contact_dim, int rows_per_contact, size_t stride) {
  if (!c || max_contacts < 0) return RTOC_ERR_BAD_ARG;
  if (max_contacts == 0) {
    c->cone_contacts = 0;
    c->cone_rows = 0;
    return RTOC_OK;
  }
  if ((contact_dim != 3 && contact_dim != 6) || max_contacts * contact_dim > c->dims.nf_max ||
      c->nrows + rows_per_contact * max_contacts > c->dims.nc_max || rows_per_contact * max_contacts > 64)
    return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const size_t need = (size_t)c->batch * c->max_stages * stride;
  if (c->want[RTOC_BUF_CONE] != need) c->buf[RTOC_BUF_CONE].release();
  c->want[RTOC_BUF_CONE] = need;
  int rc = ensure_buffer(c, RTOC_BUF_CONE);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  c->cone_contacts = max_contacts;
  c->cone_dim = contact_dim;
  c->cone_rows = rows_per_contact;
  c->epoch++;
  return RTOC_OK;
}

int rtoc_set_friction_cones(rtoc_ctx* c, int max_contacts, int contact_dim) {
  if (!c) return RTOC_ERR_BAD_ARG;
  return set_cones(c, max_contacts, contact_dim, RTOC_FRICTION_ROWS, rtoc_cone_stride(c->dims.nv, max_contacts));
}

int rtoc_set_wrench_cones(rtoc_ctx* c, int max_contacts) {
  if (!c) return RTOC_ERR_BAD_ARG;
  return set_cones(c, max_contacts, 6, RTOC_WRENCH_ROWS, rtoc_wrench_cone_stride(max_contacts));
}

int rtoc_wrench_cone_matrix(double X, double Y, double mu, double* out) {
  if (!out || !(X > 0.0) || !(Y > 0.0) || !(mu > 0.0)) return RTOC_ERR_BAD_ARG;  // ctor checks :19-26
  // Rows: unilaterality; four friction-pyramid faces; centre of pressure inside the sole (tau_x, tau_y);
  // eight yaw-torque bounds -- one per sign pattern (sx, sy, sz) of the f_x, f_y and tau_z coefficients.
  const double xymu = (X + Y) * mu;
  double row[RTOC_WRENCH_ROWS][6] = {{0, 0, -1, 0, 0, 0},   {-1, 0, -mu, 0, 0, 0}, {1, 0, -mu, 0, 0, 0},
                                     {0, -1, -mu, 0, 0, 0}, {0, 1, -mu, 0, 0, 0},  {0, 0, -Y, -1, 0, 0},
                                     {0, 0, -Y, 1, 0, 0},   {0, 0, -X, 0, -1, 0},  {0, 0, -X, 0, 1, 0}};
  // (sign of Y f_x, sign of X f_y) for rows 9..12; rows 13..16 mirror them with tau_z = +1
  static const int sg[4][2] = {{-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
  for (int i = 0; i < 4; ++i) {
    double* lo = row[9 + i];
    double* hi = row[13 + i];
    lo[0] = sg[i][0] * Y;  lo[1] = sg[i][1] * X;  lo[2] = -xymu;
    lo[3] = -sg[i][0] * mu; lo[4] = -sg[i][1] * mu; lo[5] = -1;
    hi[0] = -sg[i][0] * Y; hi[1] = -sg[i][1] * X; hi[2] = -xymu;
    hi[3] = -sg[i][0] * mu; hi[4] = -sg[i][1] * mu; hi[5] = 1;
  }
  for (int j = 0; j < RTOC_WRENCH_ROWS; ++j)
    for (int m = 0; m < 6; ++m) out[j + RTOC_WRENCH_ROWS * m] = row[j][m];
  return RTOC_OK;
}

int rtoc_set_constraint_rows(rtoc_ctx* c, const rtoc_box_row* rows, int nrows) {
  if (!c || nrows < 0 || nrows + c->cone_rows * c->cone_contacts > c->dims.nc_max || (nrows > 0 && !rows))
    return RTOC_ERR_BAD_ARG;
  for (int r = 0; r < nrows; ++r) {
    const rtoc_box_row& w = rows[r];
    const int lim = (w.var == RTOC_VAR_U) ? c->dims.nu : c->dims.nv;
    if (w.var < 0 || w.var > RTOC_VAR_A || w.index < 0 || w.index >= lim || (w.sign != 1 && w.sign != -1) ||
        w.level < 0 || w.level > 2)
      return RTOC_ERR_BAD_ARG;
    // acceleration limits are acceleration-level rows of the contact path (the unconstrained path has no `a` beside its control)
    if (w.var == RTOC_VAR_A && (w.level != 0 || c->dims.nf_max == 0)) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (nrows > 0) {
    int rc = ensure_buffer(c, RTOC_BUF_CON);
    if (rc) return rc;
    HIP_TRY(c->d_rows.reserve(c->dims.nc_max));
    HIP_TRY(hipMemcpyAsync(c->d_rows.p, rows, sizeof(rtoc_box_row) * nrows, hipMemcpyHostToDevice, c->stream));
    // rows grouped by the primal entry they act on (ascending row index inside a group, i.e. the
    // order in which the reference's components touch that entry)
    // primal entries: q (nv), v (nv), u (nu), a (nv)
    const int nv = c->dims.nv, ne = 3 * nv + c->dims.nu;
    std::vector<int> csr(ne + 1 + nrows, 0);
    auto entry_of = [&](const rtoc_box_row& w) {
      return w.var == RTOC_VAR_Q ? w.index : (w.var == RTOC_VAR_V ? nv + w.index : (w.var == RTOC_VAR_U ? 2 * nv + w.index : 2 * nv + c->dims.nu + w.index));
    };
    for (int r = 0; r < nrows; ++r) csr[entry_of(rows[r]) + 1]++;
    for (int e = 0; e < ne; ++e) csr[e + 1] += csr[e];
    std::vector<int> fill(csr.begin(), csr.begin() + ne);
    for (int r = 0; r < nrows; ++r) csr[ne + 1 + fill[entry_of(rows[r])]++] = r;
    HIP_TRY(c->d_entry.reserve(ne + 1 + c->dims.nc_max));
    HIP_TRY(hipMemcpyAsync(c->d_entry.p, csr.data(), sizeof(int) * csr.size(), hipMemcpyHostToDevice, c->stream));
    // the first two rows of every entry, packed (condense.hpp)
    std::vector<int> pair(4 * (size_t)ne, -1);
    for (int e = 0; e < ne; ++e)
      for (int k = 0; k < 2 && csr[e] + k < csr[e + 1]; ++k) {
        const int r = csr[ne + 1 + csr[e] + k];
        pair[4 * e + k] = r;
        pair[4 * e + 2 + k] = (rows[r].sign & 0xff) | (rows[r].level << 8);
      }
    HIP_TRY(c->d_pair.reserve(4 * ne));
    HIP_TRY(hipMemcpyAsync(c->d_pair.p, pair.data(), sizeof(int) * pair.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (nrows > 0) c->h_rows.assign(rows, rows + nrows);
  c->nrows = nrows;
  c->epoch++;
  return RTOC_OK;
}

int rtoc_check_fxx_structure(rtoc_ctx* c, int* structured) {
  CHECK_READY(c);
  int rc = check_fxx(c);
  if (rc) return rc;
  if (structured) *structured = c->fxx_state == 1;
  return RTOC_OK;
}

int rtoc_status(rtoc_ctx* c, uint32_t* host_flags, int count) {
  if (!c || !host_flags || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(host_flags, c->d_status.p, sizeof(uint32_t) * count, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_clear_status(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->d_status.p, 0, sizeof(uint32_t) * c->batch, c->stream));
  return RTOC_OK;
}

// Tuning aid (not part of the drop-in surface): attach a device buffer of nstages*16 int64 that
// block 0 of the backward kernel fills with phase cycle stamps; nullptr detaches.
int rtoc_debug_profile(rtoc_ctx* c, long long* host_out) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->max_stages * 32;
  if (!c->d_prof.p) {
    HIP_TRY(c->d_prof.reserve(n));
    HIP_TRY(hipMemsetAsync(c->d_prof.p, 0, n * sizeof(long long), c->stream));
    return RTOC_OK;
  }
  if (host_out) {
    HIP_TRY(hipMemcpyAsync(host_out, c->d_prof.p, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}

int rtoc_sync(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_newton_iteration(rtoc_ctx* c, double kkt_tol, double tau);
int rtoc_linearize_contact_dynamics(rtoc_ctx* c, int augment_residual);
int rtoc_time_phase(rtoc_ctx* c, int phase, int reps, float* ms) {
  CHECK_READY(c);
  if (!ms || reps < 1 || phase < 0 || phase > 8) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int r = 0; r < reps; ++r) {
    BwdPlan p;
    int rc = (phase == 0 || phase == 4) ? plan_backward(c, &p) : RTOC_OK;
    if (rc) return rc;
    switch (phase) {
      case 0: rc = launch_backward(c, p); break;
      case 1: rc = launch_forward(c); break;
      case 2: rc = rtoc_condense(c); break;      // incl. cone rows / state-equation correction if set
      case 3: rc = rtoc_expand(c, 0.995); break;
      case 4: rc = launch_sweep(c, p); break;
      case 5: rc = rtoc_update(c); break;
      case 6: rc = rtoc_newton_iteration(c, 0.0, 0.995); break;  // the whole iteration as one launch sequence
      case 7: rc = rtoc_linearize_contact_dynamics(c, 0); break;
      case 8: rc = rtoc_linearize_contact_dynamics(c, 1); break;
    }
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, c->ev0, c->ev1));
  *ms = t / reps;
  return RTOC_OK;
}

// ---- SplitSolution::integrate ---------------------------------------------------------------
int rtoc_integrate_solution(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  IntArgs a;
  a.sol = c->buf[RTOC_BUF_SOL].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.steps = c->buf[RTOC_BUF_STEP].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nv = c->dims.nv;
  a.nu = c->dims.nu;
  a.np = c->dims.np;
  a.nf_max = c->dims.nf_max;
  a.ns_max = c->dims.ns_max;
  a.sl = c->L.sol;
  a.dl = c->L.dir;
  hipLaunchKernelGGL(integrate_solution_kernel, dim3(c->batch * c->nstages), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// ---- rigid-body linearisation (include/rtoc_robot.h) ------------------------------------------
// The checks of a robot-model table that do not depend on a context, and everything the kernels precompute from it (tree levels,
// packed constants, the tangent walk's storage plan and passes).  out: a new DevModel, or empty.
static int build_dev_model(const rtoc_robot_model* m, int forced_dpp, std::unique_ptr<rbd::DevModel>& out, int* max_dimf_out) {
  out.reset();
  if (!m) return RTOC_ERR_BAD_ARG;
  if (m->njoints < 1 || m->njoints > RTOC_MAX_JOINTS || m->ncontacts < 0 || m->ncontacts > RTOC_MAX_CONTACTS) return RTOC_ERR_BAD_ARG;
  int max_dimf = 0;
  for (int k = 0; k < m->ncontacts; ++k) {
    if (m->contact_type[k] != RTOC_CONTACT_POINT && m->contact_type[k] != RTOC_CONTACT_SURFACE) return RTOC_ERR_BAD_ARG;
    if (k > 0 && m->contact_type[k] < m->contact_type[k - 1]) return RTOC_ERR_BAD_ARG;  // points first
    max_dimf += m->contact_type[k] == RTOC_CONTACT_SURFACE ? 6 : 3;
  }
  if (max_dimf_out) *max_dimf_out = max_dimf;
  const bool ff = m->type[0] == RTOC_JOINT_FREE_FLYER;
  if (m->nv < 1 || m->nv > RTOC_MAX_JOINTS + 8 || m->nq != m->nv + (ff ? 1 : 0)) return RTOC_ERR_BAD_ARG;
  std::unique_ptr<rbd::DevModel> h(new (std::nothrow) rbd::DevModel);
  if (!h) return RTOC_ERR_HIP;
  h->m = *m;
  // depth-first order: when joint i is visited, the joint open one level up must be its parent
  int open[RTOC_MAX_JOINTS], iq = 0, iv = 0, nlev = 0;
  for (int k = 0; k < RTOC_MAX_JOINTS; ++k) open[k] = -1;
  bool ok = true;
  for (int i = 0; i < m->njoints && ok; ++i) {
    const int par = m->parent[i];
    ok = par < i && par >= -1 && (m->type[i] == RTOC_JOINT_REVOLUTE || (m->type[i] == RTOC_JOINT_FREE_FLYER && i == 0 && par == -1));
    if (!ok) break;
    const int d = par < 0 ? 0 : h->depth[par] + 1;
    ok = (d == 0 || open[d - 1] == par) && m->idx_q[i] == iq && m->idx_v[i] == iv;
    h->depth[i] = d;
    open[d] = i;
    for (int k = d + 1; k < RTOC_MAX_JOINTS; ++k) open[k] = -1;   // the levels below are closed for good
    nlev = d + 1 > nlev ? d + 1 : nlev;
    iq += m->type[i] == RTOC_JOINT_FREE_FLYER ? 7 : 1;
    iv += m->type[i] == RTOC_JOINT_FREE_FLYER ? 6 : 1;
  }
  ok = ok && iq == m->nq && iv == m->nv;
  for (int k = 0; k < m->ncontacts && ok; ++k) ok = m->contact_parent[k] >= 0 && m->contact_parent[k] < m->njoints;
  if (!ok) return RTOC_ERR_BAD_ARG;
  h->nlevels = nlev;
  rbd::pack_model(h.get());
  if (forced_dpp) rbd::plan_passes(h.get(), forced_dpp);
  // (the walk's plan word has four bits for a forward-tangent slot: at most 14 branching bodies on a root-to-leaf path)
  if (h->nbranch > 14 || rbd::lin_lds_bytes(nlev, h->nbranch, m->njoints, m->ncontacts, m->nv, h->dpp, false) > 160 * 1024)
    return RTOC_ERR_BAD_ARG;
  out = std::move(h);
  return RTOC_OK;
}

int rtoc_robot_model_plan(const rtoc_robot_model* m, int forced_dofs_per_pass, rtoc_linearize_plan* plan, unsigned long long* pass_bodies) {
  if (!plan || forced_dofs_per_pass < 0 || forced_dofs_per_pass > rbd::LIN_MAX_DPP) return RTOC_ERR_BAD_ARG;
  std::unique_ptr<rbd::DevModel> h;
  const int rc = build_dev_model(m, forced_dofs_per_pass, h, nullptr);
  if (rc) return rc;
  plan->nlevels = h->nlevels, plan->nbranch = h->nbranch, plan->dofs_per_pass = h->dpp, plan->npass = h->npass;
  plan->lds_bytes = (int)rbd::lin_lds_bytes(h->nlevels, h->nbranch, m->njoints, m->ncontacts, m->nv, h->dpp, true);
  if (pass_bodies)
    for (int p = 0; p < RTOC_MAX_JOINTS + 8; ++p) pass_bodies[p] = p < h->npass ? h->pass_bodies[p] : 0ull;
  return RTOC_OK;
}

int rtoc_set_robot_model(rtoc_ctx* c, const rtoc_robot_model* m) {
  if (!c || !m) return RTOC_ERR_BAD_ARG;
  std::unique_ptr<rbd::DevModel> h;
  int max_dimf = 0;
  const int brc = build_dev_model(m, c->lin_dpp, h, &max_dimf);
  if (brc) return brc;
  const bool ff = m->type[0] == RTOC_JOINT_FREE_FLYER;
  if (m->nv != c->dims.nv || max_dimf > c->dims.nf_max || (ff ? m->nv - 6 : m->nv) != c->dims.nu)
    return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_model.reserve(1));
  c->h_model = std::move(h);
  HIP_TRY(hipMemcpyAsync(c->d_model.p, c->h_model.get(), sizeof(rbd::DevModel), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(set_linearize_lds(*m, c->h_model->nlevels, c->h_model->nbranch, c->h_model->dpp));
  c->epoch++;
  return RTOC_OK;
}

int rtoc_set_contact_schedule(rtoc_ctx* c, const unsigned* active, const double* positions, const double* rotations) {
  CHECK_READY(c);
  if (!c->h_model || !active) return RTOC_ERR_BAD_ARG;
  const rtoc_robot_model& m = c->h_model->m;
  const int nc = m.ncontacts;
  for (int i = 0; i < c->nstages; ++i) {
    if (nc < 32 && (active[i] >> nc) != 0) return RTOC_ERR_BAD_ARG;
    int rows = 0;
    for (int k = 0; k < nc; ++k)
      if ((active[i] >> k) & 1u) rows += m.contact_type[k] == RTOC_CONTACT_SURFACE ? 6 : 3;
    if (i < c->nstages - 1 && rows != c->h_grid[i].dimf) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(reserve_active(c));
  HIP_TRY(c->d_cpos.reserve((size_t)c->max_stages * RTOC_MAX_CONTACTS * 3));
  if (rotations) HIP_TRY(c->d_crot.reserve((size_t)c->max_stages * RTOC_MAX_CONTACTS * 9));
  HIP_TRY(hipMemcpyAsync(c->d_active.p, active, sizeof(unsigned) * c->nstages, hipMemcpyHostToDevice, c->stream));
  if (positions)
    HIP_TRY(hipMemcpyAsync(c->d_cpos.p, positions, sizeof(double) * c->nstages * nc * 3, hipMemcpyHostToDevice, c->stream));
  if (rotations)
    HIP_TRY(hipMemcpyAsync(c->d_crot.p, rotations, sizeof(double) * c->nstages * nc * 9, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->has_cpos = positions != nullptr;
  c->has_crot = rotations != nullptr;
  c->epoch++;
  return RTOC_OK;
}

// rbd_values_kernel for the iterate in RTOC_BUF_SOL: the lane-invariant values of the rigid-body recursion per body (and the
// ID rows of RTOC_CDD_IDC), read by the tangent walk and by the friction-cone rows
// scratch of the values pre-pass (hipFree / hipMalloc synchronise the device: callers that fork a stream call this first)
static int ensure_rbd_values(rtoc_ctx* c) {
  if (!c->h_model) return RTOC_ERR_NOT_READY;
  const rtoc_robot_model& m = c->h_model->m;
  const bool any_impact = any_grid_point(c, c->nstages - 1, grid_is_impact);
  const size_t need = (size_t)c->batch * c->max_stages * m.njoints * rbd::VAL_SLOTS;
  if (c->d_vals.n < need) c->d_vals2.release();   // both grow together: the second one only on grids with an impact
  HIP_TRY(c->d_vals.grow(need));
  if (any_impact) HIP_TRY(c->d_vals2.reserve(c->d_vals.n));
  return RTOC_OK;
}

static int launch_rbd_values(rtoc_ctx* c, bool unconstr) {
  if (!c->h_model || !c->d_active.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  if (c->nstages < 2) return RTOC_OK;
  const bool any_impact = any_grid_point(c, c->nstages - 1, grid_is_impact);
  rc = ensure_rbd_values(c);
  if (rc) return rc;
  rbd::ValArgs v;
  v.rv = view(c), v.md = model_dims(c);
  v.unconstr = unconstr ? 1 : 0;
  const int G = 64 / v.md.gs;
  const long long items = (long long)c->batch * (c->nstages - 1);
  const size_t vlds = sizeof(double) * G * v.md.njoints * rbd::VAL_SLOTS;
  for (int trav = 0; trav < (any_impact ? 2 : 1); ++trav) {
    v.trav = trav;
    v.vals = trav == 0 ? c->d_vals.p : c->d_vals2.p;
    // the kinematics traversal exists on impact grids only: launch just those (if they fit the list)
    v.nsel = trav == 1 ? select_grid_points(c, grid_is_impact, v.sel) : 0;
    const long long n = v.nsel > 0 ? (long long)c->batch * v.nsel : items;
    hipLaunchKernelGGL(rbd::rbd_values_kernel, dim3((unsigned)((n + G - 1) / G)), dim3(64), vlds, c->stream, v);
  }
  HIP_TRY(hipGetLastError());
  c->vals_fresh = 1;
  return RTOC_OK;
}

static int launch_linearize(rtoc_ctx* c, int augment_residual, bool unconstr, double scale) {
  if (!c->h_model || !c->d_active.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (augment_residual && !c->buf[RTOC_BUF_KKT].p) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  rbd::LinArgs a;
  a.rv = view(c), a.md = model_dims(c);
  if (!augment_residual) a.rv.kkt = nullptr;
  a.unconstr = unconstr ? 1 : 0;
  a.scale = scale;
  if (c->nstages < 2) return RTOC_OK;
  const size_t lds = rbd::lin_lds_bytes(c->h_model->nlevels, c->h_model->nbranch, c->h_model->m.njoints, c->h_model->m.ncontacts, c->h_model->m.nv, c->h_model->dpp, !c->linearize_fused);
  const bool surf = model_has_surface_contacts(c->h_model->m);
  a.vals = a.vals2 = nullptr;
  if (!c->linearize_fused) {
    // the values of the recursion first (level-parallel, lanes = bodies), then the tangent walk reads them (rigid_body.hpp)
    if (!c->vals_fresh) {
      const int rv = launch_rbd_values(c, unconstr);
      if (rv) return rv;
    }
    c->vals_fresh = 0;
    a.vals = c->d_vals.p, a.vals2 = c->d_vals2.p;
    if (surf)
      hipLaunchKernelGGL((rbd::linearize_contact_dynamics_kernel<true, true>), dim3(c->batch * (c->nstages - 1)), dim3(64), lds, c->stream, a);
    else
      hipLaunchKernelGGL((rbd::linearize_contact_dynamics_kernel<false, true>), dim3(c->batch * (c->nstages - 1)), dim3(64), lds, c->stream, a);
  } else if (surf) {
    hipLaunchKernelGGL(rbd::linearize_contact_dynamics_kernel<true>, dim3(c->batch * (c->nstages - 1)), dim3(64), lds, c->stream, a);
  } else {
    hipLaunchKernelGGL(rbd::linearize_contact_dynamics_kernel<false>, dim3(c->batch * (c->nstages - 1)), dim3(64), lds, c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_linearize_contact_dynamics(rtoc_ctx* c, int augment_residual) {
  CHECK_READY(c);
  return launch_linearize(c, augment_residual, false, 1.0);
}

// ---- the unconstrained (fixed-base, contact-free) solver iteration closed on the device -------
int rtoc_set_configuration_cost(rtoc_ctx* c, const rtoc_configuration_cost* cost) {
  if (!c || !cost) return RTOC_ERR_BAD_ARG;
  const int nv = c->dims.nv, M = nv + 1;
  if (M > RTOC_MAX_JOINTS || (c->dims.np != 0 && c->dims.np != 6)) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<double> h((size_t)12 * M, 0.0);
  const double* src[12] = {cost->q_ref, cost->v_ref, cost->u_ref, cost->q_weight, cost->v_weight, cost->a_weight, cost->u_weight,
                           cost->q_weight_terminal, cost->v_weight_terminal, cost->q_weight_impact, cost->v_weight_impact,
                           cost->dv_weight_impact};
  for (int k = 0; k < 12; ++k) {
    const int n = k == 0 ? nv + (c->dims.np == 6 ? 1 : 0) : (k == 2 || k == 6 ? c->dims.nu : nv);
    for (int i = 0; i < n; ++i) {
      if (k >= 3 && !(src[k][i] >= 0.0)) return RTOC_ERR_BAD_ARG;  // configuration_space_cost.cpp: weights must be non-negative
      h[(size_t)k * M + i] = src[k][i];
    }
  }
  HIP_TRY(c->d_cost.reserve(12 * M));
  HIP_TRY(hipMemcpyAsync(c->d_cost.p, h.data(), sizeof(double) * 12 * M, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_set_initial_state(rtoc_ctx* c, const double* x0, int count) {
  if (!c || !x0 || count != c->batch) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const int nq = c->dims.nv + (c->dims.np == 6 ? 1 : 0);  // a free-flyer base carries a quaternion
  const size_t n = (size_t)c->batch * (nq + c->dims.nv);
  HIP_TRY(c->d_x0.reserve(n));
  HIP_TRY(hipMemcpyAsync(c->d_x0.p, x0, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// linearizeStateEquation / linearizeImpactStateEquation of every non-terminal grid point (state_equation_lin.hpp)
static int launch_state_equation(rtoc_ctx* c, bool zeroed);
int rtoc_linearize_state_equation(rtoc_ctx* c) { return launch_state_equation(c, false); }
// zeroed: the caller has just zeroed the KKT records (rtoc_contact_eval_kkt) -- only the non-zero entries of the Fxx top
// half are written, and the records are known to have the structure RTOC_OPT_FXX_STRUCTURE's check would find
static int launch_state_equation(rtoc_ctx* c, bool zeroed) {
  CHECK_READY(c);
  if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->dims.np != 0 && c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_DX0);
  if (!rc && c->dims.np == 6) rc = ensure_buffer(c, RTOC_BUF_SE3);
  if (rc) return rc;
  SeLinArgs a;
  a.rv = view(c);
  a.x0 = c->d_x0.p;
  a.zeroed = zeroed ? 1 : 0;
  hipLaunchKernelGGL(state_equation_lin_kernel, dim3(c->batch * c->nstages), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fxx_state = zeroed ? 1 : 0;
  return RTOC_OK;
}

int rtoc_set_constraint_bounds(rtoc_ctx* c, const double* bounds, int nrows, double barrier_param, double fraction_to_boundary_rule) {
  if (!c || !bounds || nrows != c->nrows || nrows <= 0) return RTOC_ERR_BAD_ARG;
  if (!(barrier_param > 0.0) || !(fraction_to_boundary_rule > 0.0) || !(fraction_to_boundary_rule < 1.0)) return RTOC_ERR_BAD_ARG;  // constraints.cpp setters
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_bounds.reserve(c->dims.nc_max));
  HIP_TRY(hipMemcpyAsync(c->d_bounds.p, bounds, sizeof(double) * nrows, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->barrier = barrier_param;
  c->ftb_rule = fraction_to_boundary_rule;
  return RTOC_OK;
}

static int launch_ubox(rtoc_ctx* c, int mode, bool contact = false) {
  UboxArgs a;
  a.rv = view(c);
  a.rows = c->d_rows.p;
  a.entry = c->d_entry.p;
  a.bounds = c->d_bounds.p;
  a.nrows = c->nrows, a.mode = mode;
  a.barrier = c->barrier, a.tau = c->ftb_rule;
  a.contact = contact ? 1 : 0;
  a.q_shift = (contact && c->dims.np == 6) ? 1 : 0;
  hipLaunchKernelGGL(unconstr_box_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}
static bool ubox_on(const rtoc_ctx* c) { return c->nrows > 0 && c->d_bounds.p != nullptr; }

// UnconstrOCPSolver::initConstraints (unconstr_ocp_solver.cpp:91-93): setSlackAndDual of every row at the current iterate
int rtoc_unconstr_init_constraints(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!ubox_on(c) || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  return launch_ubox(c, UBOX_INIT);
}

static int task_costs_ready(rtoc_ctx* c, bool unconstr);
static int launch_task_costs(rtoc_ctx* c, double unconstr_dt, double* cost_out);

int rtoc_unconstr_eval_kkt(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (!(dt > 0.0) || c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  if (!c->h_model || !c->d_cost.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->h_model->m.type[0] == RTOC_JOINT_FREE_FLYER || c->h_model->m.ncontacts != 0) return RTOC_ERR_BAD_ARG;  // unconstr_dynamics.cpp:22-29
  int rc = c->ntasks > 0 ? task_costs_ready(c, true) : RTOC_OK;   // ahead of the first launch: a refusal leaves the records alone
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_DX0);
  if (rc) return rc;
  bool fresh = false;
  HIP_TRY(reserve_active(c, &fresh));
  if (fresh) HIP_TRY(hipMemsetAsync(c->d_active.p, 0, sizeof(unsigned) * c->max_stages, c->stream));  // no contacts: an all-zero schedule
  rbd::UkArgs a;
  a.rv = view(c);
  a.cost = c->d_cost.p;
  a.x0 = c->d_x0.p;
  a.dt = dt;
  c->ls_unconstr_dt = dt;
  if (c->ls_on) HIP_TRY(reserve_costval(c));
  a.cost_out = c->ls_on ? c->d_costval.p : nullptr;   // the line search's evalOCP (unconstr_line_search.cpp:56-83)
  hipLaunchKernelGGL(rbd::unconstr_eval_kkt_kernel, dim3(c->batch * c->nstages), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fxx_state = 0;
  // the task-space terms of the cost function (TaskSpace6DCost / TaskSpace3DCost / CoMCost), added to what the configuration cost stored
  if (c->ntasks > 0) {
    rc = launch_task_costs(c, dt, a.cost_out);
    if (rc) return rc;
  }
  rc = launch_linearize(c, 1, true, dt);
  if (!rc && ubox_on(c)) rc = launch_ubox(c, UBOX_LINEARIZE);  // constraints_->linearizeConstraints (unconstr_intermediate_stage.cpp:68-69)
  return rc;
}

// ---- KKT error ------------------------------------------------------------------------------
static int launch_kkt_error(rtoc_ctx* c) {
  HIP_TRY(reserve_kkterr(c));
  KktErrArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.con = (c->nrows > 0 || c->cone_contacts > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.rows = c->d_rows.p;
  a.grid = c->d_grid.p;
  a.out = c->d_kkterr.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nrows = c->nrows;
  a.cone_contacts = c->cone_contacts;
  a.cone_dim = c->cone_dim > 0 ? c->cone_dim : 3;
  a.cone_rows = c->cone_rows;
  a.impact_cones = c->impact_cones;
  a.nc_max = c->dims.nc_max;
  a.nv = c->dims.nv;
  a.nu = c->dims.nu;
  a.np = c->dims.np;
  a.nx = c->L.nx;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  a.nl = c->L.con;
  a.partial = c->d_kkterr.p + c->batch;
  hipLaunchKernelGGL(kkt_error_kernel, dim3(c->nstages, c->batch), dim3(64), 0, c->stream, a);
  hipLaunchKernelGGL(kkt_error_reduce_kernel, dim3((c->batch + 63) / 64), dim3(64), 0, c->stream, a.partial, c->d_kkterr.p,
                     c->nstages, c->batch);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_kkt_error(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  if (!host_out || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  int rc = launch_kkt_error(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(host_out, c->d_kkterr.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// ---- evalKKT / updateSolution of the contact path closed on the device (ConfigurationSpaceCost, no inequality rows) ----
int rtoc_newton_iteration(rtoc_ctx* c, double kkt_tol, double tau);
// ---- inequality rows of the contact path evaluated on the device --------------------------------------------
int rtoc_set_barrier_param(rtoc_ctx* c, double barrier_param, double fraction_to_boundary_rule) {
  if (!c) return RTOC_ERR_BAD_ARG;
  if (!(barrier_param > 0.0) || !(fraction_to_boundary_rule > 0.0) || !(fraction_to_boundary_rule < 1.0)) return RTOC_ERR_BAD_ARG;
  c->barrier = barrier_param;
  c->ftb_rule = fraction_to_boundary_rule;
  c->epoch++;
  return RTOC_OK;
}

int rtoc_set_friction_coefficients(rtoc_ctx* c, const double* mu, int ncontacts) {
  if (!c || !mu || ncontacts < 1 || ncontacts > RTOC_MAX_CONTACTS) return RTOC_ERR_BAD_ARG;
  for (int i = 0; i < ncontacts; ++i)
    if (!(mu[i] > 0.0)) return RTOC_ERR_BAD_ARG;   // ContactStatus::setFrictionCoefficient
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_mu.reserve(RTOC_MAX_CONTACTS));
  double full[RTOC_MAX_CONTACTS] = {0.0};
  memcpy(full, mu, sizeof(double) * ncontacts);
  HIP_TRY(hipMemcpyAsync(c->d_mu.p, full, sizeof(full), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->n_mu = ncontacts;
  return RTOC_OK;
}

static bool device_cones_on(const rtoc_ctx* c) { return c->cone_contacts > 0 && c->cone_rows == RTOC_FRICTION_ROWS && c->d_mu.p != nullptr; }
static bool device_wrench_on(const rtoc_ctx* c) { return c->cone_contacts > 0 && c->cone_rows == RTOC_WRENCH_ROWS && c->d_wcone.p != nullptr; }

int rtoc_set_wrench_cone_params(rtoc_ctx* c, const double* xy_mu, int ncontacts) {
  if (!c || !xy_mu || ncontacts < 1 || ncontacts > RTOC_MAX_CONTACTS) return RTOC_ERR_BAD_ARG;
  std::vector<double> table((size_t)RTOC_MAX_CONTACTS * RTOC_WRENCH_ROWS * 6, 0.0);
  for (int k = 0; k < ncontacts; ++k) {
    const int rc = rtoc_wrench_cone_matrix(xy_mu[3 * k], xy_mu[3 * k + 1], xy_mu[3 * k + 2], &table[(size_t)k * RTOC_WRENCH_ROWS * 6]);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_wcone.reserve(table.size()));
  HIP_TRY(hipMemcpyAsync(c->d_wcone.p, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

static int launch_wrench_cones(rtoc_ctx* c, int mode) {
  const rtoc_robot_model& m = c->h_model->m;
  if (m.ncontacts > c->cone_contacts) return RTOC_ERR_BAD_ARG;
  for (int k = 0; k < m.ncontacts; ++k)
    if (m.contact_type[k] != RTOC_CONTACT_SURFACE) return RTOC_ERR_BAD_ARG;
  WcArgs a;
  a.rv = view(c), a.md = model_dims(c);
  a.table = c->d_wcone.p;
  a.mode = mode;
  a.row0 = c->dims.nc_max - RTOC_WRENCH_ROWS * c->cone_contacts, a.cone_stride = rtoc_wrench_cone_stride(c->cone_contacts);
  a.impact_cones = c->impact_cones;
  a.barrier = c->barrier;
  hipLaunchKernelGGL(wrench_cone_eval_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_contact_cones(rtoc_ctx* c, int mode) {
  const rtoc_robot_model& m = c->h_model->m;
  if (m.ncontacts > c->cone_contacts) return RTOC_ERR_BAD_ARG;
  if (c->n_mu < m.ncontacts) return RTOC_ERR_NOT_READY;  // a friction coefficient for every contact of the model
  for (int k = 0; k < m.ncontacts; ++k)
    if ((m.contact_type[k] == RTOC_CONTACT_SURFACE ? 6 : 3) != c->cone_dim) return RTOC_ERR_BAD_ARG;
  CcArgs a;
  a.rv = view(c), a.md = model_dims(c);
  a.mu = c->d_mu.p;
  a.mode = mode;
  a.contact_dim = c->cone_dim, a.row0 = c->dims.nc_max - RTOC_FRICTION_ROWS * c->cone_contacts;
  a.cone_stride = rtoc_cone_stride(c->dims.nv, c->cone_contacts), a.dgdf_off = rtoc_cone_dgdf_off(c->dims.nv, c->cone_contacts);
  a.impact_cones = c->impact_cones;
  a.exact_jacobian = c->exact_cone_jacobian;
  a.barrier = c->barrier;
  if (mode == CC_LINEARIZE && c->vals_fresh && c->d_vals.p) {   // kinematics already there: no tree walk (contact_cone_vals_kernel)
    CvArgs v;
    v.c = a;
    v.vals = c->d_vals.p;
    hipLaunchKernelGGL(contact_cone_vals_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, v);
    HIP_TRY(hipGetLastError());
    return RTOC_OK;
  }
  const size_t lds = cc_lds_bytes(a.md.nlevels, a.md.njoints, a.md.ncontacts);
  HIP_TRY(hipFuncSetAttribute((const void*)contact_cone_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(contact_cone_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// OCPSolver::initConstraints (src/solver/ocp_solver.cpp:92-96 -> DirectMultipleShooting::initConstraints): setSlackAndDual of
// the joint-limit rows (those with bounds on the device) and of the friction-cone rows (those with friction coefficients)
int rtoc_contact_init_constraints(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->buf[RTOC_BUF_SOL].p || !(c->barrier > 0.0)) return RTOC_ERR_NOT_READY;
  const bool rows = c->nrows > 0 && c->d_bounds.p != nullptr, cones = device_cones_on(c), wrench = device_wrench_on(c);
  if (!rows && !cones && !wrench) return RTOC_ERR_NOT_READY;
  if ((cones || wrench) && (!c->h_model || !c->d_active.p)) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->buf[RTOC_BUF_CON].p, 0, sizeof(double) * c->want[RTOC_BUF_CON], c->stream));
  if (rows) rc = launch_ubox(c, UBOX_INIT, true);
  if (!rc && cones) rc = launch_contact_cones(c, CC_INIT);
  if (!rc && wrench) rc = launch_wrench_cones(c, CC_INIT);
  return rc;
}

// linearizeSwitchingConstraint (src/dynamics/switching_constraint.cpp:26-70) on the grids that carry one
static int launch_switching_constraint(rtoc_ctx* c) {
  SwLinArgs a;
  a.rv = view(c), a.md = model_dims(c);
  a.exact_transport = c->exact_transport;
  for (int i = 0; i < c->nstages; ++i)
    if (c->h_grid[i].switching_constraint && c->h_grid[i].dims > c->dims.ns_max) return RTOC_ERR_BAD_ARG;
  a.nsel = select_grid_points(c, grid_has_switching, a.sel);
  const int per = a.nsel > 0 ? a.nsel : c->nstages - 1;
  const size_t lds = sw_lds_bytes(a.md.nlevels, a.md.njoints, a.md.ncontacts);
  HIP_TRY(hipFuncSetAttribute((const void*)switching_constraint_lin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(switching_constraint_lin_kernel, dim3(c->batch * per), dim3(64), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// ---- TaskSpace3DCost / CoMCost / TaskSpace6DCost (task_space_cost.hpp) ----
static bool task_cost_valid(const rtoc_task_cost& t, int njoints) {
  if (t.kind != RTOC_TASK_FRAME_3D && t.kind != RTOC_TASK_COM && t.kind != RTOC_TASK_FRAME_6D) return false;
  if (t.ref_kind != RTOC_REF_CONST && t.ref_kind != RTOC_REF_PERIODIC_FOOT && t.ref_kind != RTOC_REF_PERIODIC_COM && t.ref_kind != RTOC_REF_TABLE)
    return false;
  if (t.kind != RTOC_TASK_COM && (t.frame_parent < 0 || t.frame_parent >= njoints)) return false;
  for (int k = 0; k < 3; ++k)   // set_weight / set_weight_terminal / set_weight_impact: elements must be non-negative
    if (!(t.weight[k] >= 0.0) || !(t.weight_terminal[k] >= 0.0) || !(t.weight_impact[k] >= 0.0)) return false;
  const bool periodic = t.ref_kind == RTOC_REF_PERIODIC_FOOT || t.ref_kind == RTOC_REF_PERIODIC_COM;
  if (periodic && (!(t.period_active > 0.0) || !(t.period_inactive >= 0.0))) return false;
  if (t.kind == RTOC_TASK_FRAME_6D) {
    if (periodic) return false;   // the periodic references are positions
    for (int k = 0; k < 3; ++k)   // the six weights in the order they multiply d (rtoc_robot.h: WEIGHT ORDER)
      if (!(t.weight_angular[k] >= 0.0) || !(t.weight_angular_terminal[k] >= 0.0) || !(t.weight_angular_impact[k] >= 0.0)) return false;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(t.frame_R[k]) || !std::isfinite(t.ref_R[k])) return false;
  }
  return true;
}

int rtoc_set_task_costs(rtoc_ctx* c, const rtoc_task_cost* terms, int nterms, int per_instance) {
  if (!c || nterms < 0 || nterms > RTOC_MAX_TASK_COSTS || (nterms > 0 && !terms)) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  if (nterms == 0) {
    if (c->ntasks > 0) c->epoch++;   // the kernel leaves the captured launch sequence
    c->ntasks = 0;
    return RTOC_OK;
  }
  if (!c->h_model) return RTOC_ERR_NOT_READY;
  if (c->dims.nv > 64) return RTOC_ERR_UNSUPPORTED_DIMS;
  const size_t n = (size_t)nterms * (per_instance ? c->batch : 1);
  for (size_t i = 0; i < n; ++i)
    if (!task_cost_valid(terms[i], c->h_model->m.njoints)) return RTOC_ERR_BAD_ARG;
  HIP_TRY(c->d_tasks.reserve((size_t)RTOC_MAX_TASK_COSTS * c->batch));   // full capacity: later calls may set more terms
  HIP_TRY(hipMemcpyAsync(c->d_tasks.p, terms, sizeof(rtoc_task_cost) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->ntasks = nterms, c->tasks_per_instance = per_instance ? 1 : 0;
  // which instantiation serves these terms, and the Jacobian rows its LDS holds (the largest term list of the batch)
  c->task_rows = 0, c->task_ext = 0;
  for (size_t i = 0; i < n; i += nterms) {
    int rows = 0;
    for (int k = 0; k < nterms; ++k) {
      rows += task_cost_rows(terms[i + k].kind);
      if (terms[i + k].kind == RTOC_TASK_FRAME_6D || terms[i + k].ref_kind == RTOC_REF_TABLE) c->task_ext = 1;
    }
    if (rows > c->task_rows) c->task_rows = rows;
  }
  c->h_task_table = 0;
  for (size_t i = 0; i < n; ++i)
    if (terms[i].ref_kind == RTOC_REF_TABLE) c->h_task_table |= 1u << (i % nterms);
  c->epoch++;   // launch parameters baked into captured graphs
  return RTOC_OK;
}

int rtoc_set_task_ref_table(rtoc_ctx* c, int term, const rtoc_task_ref_entry* entries, int nstages, int per_instance) {
  if (!c || !entries || term < 0 || term >= RTOC_MAX_TASK_COSTS) return RTOC_ERR_BAD_ARG;
  if (c->nstages < 2) return RTOC_ERR_NOT_READY;   // rtoc_set_grid
  if (nstages != c->nstages) return RTOC_ERR_BAD_ARG;
  const size_t n = (size_t)nstages * (per_instance ? c->batch : 1);
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(entries[i].R[k])) return RTOC_ERR_BAD_ARG;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(entries[i].p[k])) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  bool fresh = false;
  HIP_TRY(c->d_reftab[term].reserve((size_t)c->max_stages * (per_instance ? c->batch : 1), &fresh));
  HIP_TRY(hipMemcpyAsync(c->d_reftab[term].p, entries, sizeof(rtoc_task_ref_entry) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned bit = 1u << term, inst = per_instance ? bit : 0u;
  // captured graphs bake the pointer and the per-instance flag in
  if (fresh || c->reftab_n[term] != nstages || (c->reftab_inst & bit) != inst) c->epoch++;
  c->reftab_n[term] = nstages;
  c->reftab_inst = (c->reftab_inst & ~bit) | inst;
  return RTOC_OK;
}

int rtoc_set_grid_times(rtoc_ctx* c, const double* t, int nstages) {
  if (!c || !t || nstages < 2 || nstages > c->max_stages) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  bool fresh = false;
  HIP_TRY(c->d_gt.reserve(c->max_stages, &fresh));
  if (fresh) c->epoch++;
  c->h_gt.assign(t, t + nstages);
  HIP_TRY(hipMemcpyAsync(c->d_gt.p, t, sizeof(double) * nstages, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// per-instance grid times of a switching-time problem: kept by sto_time_steps_kernel once this buffer exists
static int ensure_grid_times_inst(rtoc_ctx* c) {
  bool fresh = false;
  HIP_TRY(c->d_gt_inst.reserve((size_t)c->batch * c->max_stages, &fresh));
  if (fresh) c->epoch++;   // sto_time_steps_kernel's arguments changed
  return RTOC_OK;
}

int rtoc_get_grid_times(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  if (!host_out || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (c->sto_on) {
    int rc = ensure_grid_times_inst(c);
    if (rc) return rc;
    STO_LAUNCH(sto_time_steps_kernel, c);
    HIP_TRY(hipMemcpyAsync(host_out, c->d_gt_inst.p, sizeof(double) * count * c->nstages, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTOC_OK;
  }
  if ((int)c->h_gt.size() != c->nstages) return RTOC_ERR_NOT_READY;
  for (int b = 0; b < count; ++b) memcpy(host_out + (size_t)b * c->nstages, c->h_gt.data(), sizeof(double) * c->nstages);
  return RTOC_OK;
}

// what the task kernel reads besides the records: the grid times (the contact path's switching-time problems write their own
// on the device; the unconstrained path has none) and the table of every RTOC_REF_TABLE term, set for the current grid
static int task_costs_ready(rtoc_ctx* c, bool unconstr) {
  if (!c->h_model || !c->d_model.p || !c->d_tasks.p) return RTOC_ERR_NOT_READY;
  const bool sto = c->sto_on && !unconstr;
  if (!sto && (int)c->h_gt.size() != c->nstages) return RTOC_ERR_NOT_READY;   // rtoc_set_grid_times
  if (sto && !c->d_gt_inst.p) return RTOC_ERR_NOT_READY;   // allocated by rtoc_contact_eval_kkt ahead of the time steps
  for (int k = 0; k < c->ntasks; ++k)
    if (((c->h_task_table >> k) & 1u) && (c->reftab_n[k] != c->nstages || !c->d_reftab[k].p)) return RTOC_ERR_NOT_READY;   // rtoc_set_task_ref_table
  return RTOC_OK;
}

// unconstr_dt > 0: from rtoc_unconstr_eval_kkt(dt) -- always the extended instantiation, which knows that path's scaling
static int launch_task_costs(rtoc_ctx* c, double unconstr_dt, double* cost_out) {
  const bool unconstr = unconstr_dt > 0.0;
  int rc = task_costs_ready(c, unconstr);
  if (rc) return rc;
  const bool sto = c->sto_on && !unconstr;
  TaskCostArgs a;
  a.rv = view(c);
  a.cost_out = cost_out;
  a.terms = c->d_tasks.p;
  a.t_fixed = sto ? nullptr : c->d_gt.p;
  a.t_inst = sto ? c->d_gt_inst.p : nullptr;
  a.nterms = c->ntasks, a.per_instance = c->tasks_per_instance;
  for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) a.tab[k] = (k < c->ntasks && ((c->h_task_table >> k) & 1u)) ? c->d_reftab[k].p : nullptr;
  a.tab_inst = c->reftab_inst;
  a.nrows = c->task_rows;
  a.unconstr_dt = unconstr ? unconstr_dt : 0.0;
  // the 16-byte row pairs of Qqq need an even record stride and column length and an even field offset
  if ((c->L.kkt.stride | c->L.kkt.off[RTOC_KKT_QXX]) & 1) return RTOC_ERR_BAD_ARG;
  const long long items = (long long)c->batch * c->nstages;
  const bool ext = c->task_ext || unconstr;
  const size_t lds1 = sizeof(double) * task_cost_lds_doubles(c->h_model->m.njoints, ext ? c->task_rows : 3 * c->ntasks, c->dims.nv);
  if (2 * lds1 > 64 * 1024) return RTOC_ERR_UNSUPPORTED_DIMS;   // (48 joints, eight 6D terms, 64 dofs: 30 KB per grid point)
  const dim3 grid2((unsigned)((items + 1) / 2)), grid1((unsigned)items);
  if (c->dims.nv <= 32) {
    if (ext) hipLaunchKernelGGL((task_space_cost_kernel<2, true>), grid2, dim3(64), 2 * lds1, c->stream, a);
    else hipLaunchKernelGGL((task_space_cost_kernel<2, false>), grid2, dim3(64), 2 * lds1, c->stream, a);
  } else {
    if (ext) hipLaunchKernelGGL((task_space_cost_kernel<1, true>), grid1, dim3(64), lds1, c->stream, a);
    else hipLaunchKernelGGL((task_space_cost_kernel<1, false>), grid1, dim3(64), lds1, c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_contact_eval_kkt(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->h_model || !c->d_active.p || !c->d_cost.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  const bool switching = any_grid_point(c, c->nstages, grid_has_switching);
  int rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  c->ls_unconstr_dt = 0.0;
  // the periodic references of the task-space costs read the per-instance grid times that the time steps below then write
  if (c->sto_on && c->ntasks > 0) {
    rc = ensure_grid_times_inst(c);
    if (rc) return rc;
  }
  // PhaseBased discretisation: time_discretization_.correctTimeSteps(contact_sequence_, t) ahead of evalKKT (ocp_solver.cpp:115-117)
  if (c->sto_on) STO_LAUNCH(sto_time_steps_kernel, c);
  HIP_TRY(reserve_costval(c));
  CostArgs a;
  a.rv = view(c);
  a.cost = c->d_cost.p;
  a.cost_out = c->d_costval.p;
  {
    // setZero of the KKT records (+ the constant diagonals of the cost) as one stream on the context's second stream (rtoc_riccati_sweep's), BESIDE
    // the values pre-pass of the rigid-body linearisation (lanes = bodies; writes its scratch and RTOC_CDD_IDC, which nothing
    // here zeroes): the one is bound by HBM writes, the other by latency -- 1.1 ms each per 4096 x 47 grid points, one after the
    // other on one stream.  The cost kernel and everything behind it wait for both.
    InitArgs ia;
    ia.rv = a.rv, ia.cost = c->d_cost.p;
    const long long nrec = (long long)c->batch * c->nstages;
    // four workgroups per CU: half of the wave slots, so that the pre-pass's waves are resident beside them
    // (CUs from the device: four workgroups each)
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    const int blocks = (int)(nrec < (long long)cus * 4 ? nrec : (long long)cus * 4);
    // init_records_kernel moves 16-byte pairs that must not straddle a field: record stride, the three fields it writes constants
    // into and the state dimension are even (rtoc_compute_layout pads fields to 64 B; checked here so that a layout change cannot
    // silently misplace the cost diagonals)
    if ((c->L.kkt.stride | c->L.kkt.off[RTOC_KKT_QXX] | c->L.kkt.off[RTOC_KKT_QUU] | c->L.kkt.off[RTOC_KKT_FXX]) & 1) return RTOC_ERR_BAD_ARG;
    // the (re)allocation of the pre-pass's scratch synchronises the device: ahead of the fork, never under it
    if (!c->linearize_fused) {
      rc = ensure_rbd_values(c);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    hipLaunchKernelGGL(init_records_kernel, dim3(blocks), dim3(256), 0, c->stream2, ia);
    // from here on the second stream is forked: whatever fails below, c->stream is joined to it before this call returns
    hipError_t ej = hipEventRecord(c->ev_join, c->stream2);
    c->vals_fresh = 0;
    if (ej == hipSuccess && !c->linearize_fused) rc = launch_rbd_values(c, false);   // shared by the cone rows and the tangent walk below
    if (ej == hipSuccess) ej = hipStreamWaitEvent(c->stream, c->ev_join, 0);
    else (void)hipStreamSynchronize(c->stream2);   // no event to wait on: drain the fork on the host
    if (ej != hipSuccess) {
      ctx_set_err(ej, __LINE__);
      return RTOC_ERR_HIP;
    }
    if (rc) return rc;
  }
  hipLaunchKernelGGL(contact_cost_kernel, dim3((c->batch * c->nstages + COST_GP - 1) / COST_GP), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  // TaskSpace3DCost / CoMCost: added to what the configuration cost stored, ahead of the constraints and the dynamics
  if (c->ntasks > 0) {
    rc = launch_task_costs(c, 0.0, c->d_costval.p);
    if (rc) {
      c->vals_fresh = 0;
      return rc;
    }
  }
  // constraints_->linearizeConstraints (intermediate_stage.cpp:109-110, impact_stage.cpp:95-96) of the rows evaluated here
  if (c->nrows > 0 && c->d_bounds.p && c->buf[RTOC_BUF_CON].p) rc = launch_ubox(c, UBOX_LINEARIZE, true);
  if (!rc && device_cones_on(c) && c->buf[RTOC_BUF_CON].p) rc = launch_contact_cones(c, CC_LINEARIZE);
  if (!rc && device_wrench_on(c) && c->buf[RTOC_BUF_CON].p) rc = launch_wrench_cones(c, CC_LINEARIZE);
  if (!rc) rc = launch_state_equation(c, true);
  if (!rc) rc = launch_linearize(c, 1, false, 1.0);
  if (!rc && switching) rc = launch_switching_constraint(c);
  if (rc) c->vals_fresh = 0;  // a failed sequence leaves no kinematics a later stand-alone linearisation may reuse
  return rc;
}

// OCPSolver::solve's iteration schedule (ocp_solver.cpp:169-213), shared by the host shells (include/rtoc_robot.h)
int rtoc_solve_loop(const rtoc_solve_options* o, const rtoc_solve_callbacks* cb, rtoc_solve_stats* st) {
  if (!o || !cb || !st || !cb->update_solution || o->max_iter < 0) return RTOC_ERR_BAD_ARG;
  if (o->sto_enabled && (!cb->max_time_step || !cb->mesh_refinement)) return RTOC_ERR_BAD_ARG;
  st->convergence = 0, st->iter = 0, st->num_mesh_refinements = 0;
  int inner_iter = 0;
  for (int iter = 0; iter < o->max_iter; ++iter, ++inner_iter) {
    if (o->sto_enabled && cb->set_sto_regularization) {                                         // :171-177
      const int rc = cb->set_sto_regularization(cb->user, inner_iter < o->initial_sto_reg_iter ? o->initial_sto_reg : 0.0);
      if (rc) return rc;
    }
    double kkt_error = 0.0;
    int rc = cb->update_solution(cb->user, &kkt_error);                                         // :178-180
    if (rc) return rc;
    st->iter = iter + 1;
    if (o->sto_enabled && kkt_error < o->kkt_tol_mesh) {                                        // :181
      double max_dt = 0.0;
      rc = cb->max_time_step(cb->user, &max_dt);
      if (rc) return rc;
      if (max_dt > o->max_dt_mesh) {                                                            // :182-199
        rc = cb->mesh_refinement(cb->user);
        if (rc) return rc;
        inner_iter = 0;   // (the loop header makes it 1 for the next iteration, as in the reference)
        if (st->num_mesh_refinements < RTOC_SOLVE_MAX_REFINEMENTS) st->mesh_refinement_iter[st->num_mesh_refinements] = iter + 1;
        ++st->num_mesh_refinements;
      } else if (kkt_error < o->kkt_tol) {                                                      // :200-204
        st->convergence = 1;
        break;
      }
    } else if (kkt_error < o->kkt_tol) {                                                        // :206-210
      st->convergence = 1;
      break;
    }
  }
  if (!st->convergence) st->iter = o->max_iter;                                                 // :212-214
  return RTOC_OK;
}

int rtoc_contact_update_solution(rtoc_ctx* c, double tau, double* host_kkt_error, int count) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch || (count > 0 && !host_kkt_error)) return RTOC_ERR_BAD_ARG;
  int rc = rtoc_contact_eval_kkt(c);
  if (!rc) rc = rtoc_newton_iteration(c, 0.0, tau);  // KKT error, condensation, sweep, expansion, steps, update, integrate
  if (rc) return rc;
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(host_kkt_error, c->d_kkterr.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}

// UnconstrOCPSolver::updateSolution (src/solver/unconstr_ocp_solver.cpp:96-118) of every instance, one launch
// sequence, no host synchronisation unless host_kkt_error is asked for
static int ensure_line_search(rtoc_ctx* c);
static int launch_eval_ocp(rtoc_ctx* c, double* out);

int rtoc_unconstr_update_solution(rtoc_ctx* c, double dt, double* host_kkt_error, int count) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch || (count > 0 && !host_kkt_error)) return RTOC_ERR_BAD_ARG;
  const bool rows = ubox_on(c);
  int rc = rtoc_unconstr_eval_kkt(c, dt);            // dms_.evalKKT up to the condensation, + computeInitialStateDirection
  if (!rc) rc = launch_kkt_error(c);                  // performance_index.kkt_error (pre-condensation, like :74-75)
  if (!rc && c->ls_on) {                              // dms_.getEval() of the iterate: what UnconstrLineSearch::computeStepSize reads first
    rc = ensure_line_search(c);
    if (!rc) rc = launch_eval_ocp(c, c->d_eval.p);
  }
  if (!rc && rows) rc = launch_ubox(c, UBOX_CONDENSE);  // constraints_->condenseSlackAndDual (:76-77), ahead of the dynamics
  if (!rc) rc = rtoc_unconstr_condense(c);
  if (!rc) rc = rtoc_unconstr_backward(c, dt);
  if (!rc) rc = rtoc_unconstr_forward(c, dt);
  if (!rc) rc = rtoc_unconstr_expand(c, dt);
  if (rc) return rc;
  rc = ensure_buffer(c, RTOC_BUF_STEP);
  if (rc) return rc;
  hipLaunchKernelGGL(fill_steps_kernel, dim3((2 * c->batch + 255) / 256), dim3(256), 0, c->stream, c->buf[RTOC_BUF_STEP].p, 2 * c->batch);
  HIP_TRY(hipGetLastError());
  if (rows) rc = launch_ubox(c, UBOX_EXPAND);         // expandSlackAndDual + maxSlack/DualStepSize (:80-97)
  // line_search_.computeStepSize (unconstr_ocp_solver.cpp:107-111, unconstr_line_search.cpp:37-67): the filter's backtracking loop of
  // every instance over trial iterates evaluated on the device; the accepted primal steps replace the maximum ones
  if (!rc && c->ls_on) rc = rtoc_contact_line_search(c, nullptr);
  if (!rc && rows) rc = rtoc_update(c);               // updateSlack / updateDual (:106-118)
  if (rc) return rc;
  rc = rtoc_integrate_solution(c);
  if (rc) return rc;
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(host_kkt_error, c->d_kkterr.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}

// ---- SwitchingTimeOptimization::evalKKT: scatter + STO KKT-error term ----------------------
int rtoc_sto_eval_kkt(rtoc_ctx* c, const double* host_lt, const double* host_qtt, int nev, double* host_err_sq, int count) {
  CHECK_READY(c);
  if (nev < 0 || nev > 31 || count < 0 || count > c->batch || (nev > 0 && (!host_lt || !host_qtt))) return RTOC_ERR_BAD_ARG;
  const size_t n = (size_t)c->batch * (nev > 0 ? nev : 1);
  HIP_TRY(c->d_sto.grow(2 * n + c->batch));
  double* d_lt = c->d_sto.p;
  double* d_qtt = c->d_sto.p + n;
  double* d_err = c->d_sto.p + 2 * n;
  if (nev > 0) {
    HIP_TRY(hipMemcpyAsync(d_lt, host_lt, (size_t)c->batch * nev * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_qtt, host_qtt, (size_t)c->batch * nev * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  StoArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.grid = c->d_grid.p;
  a.lt = d_lt;
  a.qtt = d_qtt;
  a.err = d_err;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nev = nev;
  a.stride = c->L.kkt.stride;
  a.scal_off = c->L.kkt.off[RTOC_KKT_SCAL];
  hipLaunchKernelGGL(sto_eval_kkt_kernel, dim3((c->batch + 63) / 64), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  if (host_err_sq && count > 0)
    HIP_TRY(hipMemcpyAsync(host_err_sq, d_err, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// ---- switching-time optimisation resident on the device (sto.hpp) ------------------------------------------------
int rtoc_sto_set_problem(rtoc_ctx* c, double t0, double T, const double* event_times, int num_events, int per_instance,
                         const double* min_dwell_times, double barrier_param, double fraction_to_boundary_rule) {
  CHECK_READY(c);
  if (num_events == 0) {  // no discrete events on this horizon: nothing to optimise (switching_time_optimization.cpp:85-90)
    c->sto_on = 0;
    c->epoch++;
    return RTOC_OK;
  }
  if (num_events < 0 || num_events > RTOC_STO_MAX_EVENTS || !event_times || !min_dwell_times || !(T > 0.0)) return RTOC_ERR_BAD_ARG;
  if (!(barrier_param > 0.0) || !(fraction_to_boundary_rule > 0.0) || !(fraction_to_boundary_rule < 1.0)) return RTOC_ERR_BAD_ARG;  // sto_constraints.cpp:44-59
  if (c->h_grid.empty() || num_events != sto_count_events(c)) return RTOC_ERR_BAD_ARG;
  for (int p = 0; p <= num_events; ++p)
    if (!(min_dwell_times[p] >= 0.0)) return RTOC_ERR_BAD_ARG;  // :38-43
  const size_t ne = (size_t)c->batch * num_events;
  std::vector<double> ts(ne);
  for (int b = 0; b < c->batch; ++b)
    for (int e = 0; e < num_events; ++e) {
      const double te = event_times[(per_instance ? (size_t)b * num_events : 0) + e];
      const double prev = e > 0 ? ts[(size_t)b * num_events + e - 1] : t0;
      if (!(te > prev) || !(te < t0 + T)) return RTOC_ERR_BAD_ARG;  // events ordered, inside the horizon
      ts[(size_t)b * num_events + e] = te;
    }
  if (c->sto_nev != num_events) c->d_sto_cost.release();   // (d_ts and d_sto_out are resized below)
  HIP_TRY(c->d_ts.reserve(ne));
  HIP_TRY(c->d_sto_out.reserve(2 * ne + c->batch));
  HIP_TRY(c->d_dt.reserve((size_t)c->batch * c->max_stages));
  HIP_TRY(c->d_sto_con.reserve((size_t)c->batch * RTOC_STO_CON_STRIDE));
  HIP_TRY(c->d_min_dwell.reserve(RTOC_STO_MAX_EVENTS + 1));
  HIP_TRY(reserve_kkterr(c));
  int rc = ensure_buffer(c, RTOC_BUF_STEP);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_ts.p, ts.data(), sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_min_dwell.p, min_dwell_times, sizeof(double) * (num_events + 1), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_sto_con.p, 0, sizeof(double) * c->batch * RTOC_STO_CON_STRIDE, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->sto_on = 1, c->sto_nev = num_events, c->sto_t0 = t0, c->sto_T = T;
  c->sto_barrier = barrier_param, c->sto_tau = fraction_to_boundary_rule;
  c->epoch++;
  STO_LAUNCH(sto_time_steps_kernel, c);  // the time steps that belong to these event times
  return RTOC_OK;
}

int rtoc_sto_set_regularization(rtoc_ctx* c, double sto_reg) {
  if (!c || !(sto_reg >= 0.0)) return RTOC_ERR_BAD_ARG;
  if (c->sto_reg != sto_reg) c->epoch++;
  c->sto_reg = sto_reg;
  return RTOC_OK;
}

int rtoc_sto_set_cost_terms(rtoc_ctx* c, const double* lt, const double* qtt_diag) {
  CHECK_READY(c);
  if (!c->sto_on || (!lt) != (!qtt_diag)) return RTOC_ERR_BAD_ARG;
  const size_t ne = (size_t)c->batch * c->sto_nev;
  if (!lt) {
    c->d_sto_cost.release();
    c->epoch++;
    return RTOC_OK;
  }
  bool fresh = false;
  HIP_TRY(c->d_sto_cost.reserve(2 * ne, &fresh));
  if (fresh) c->epoch++;
  HIP_TRY(hipMemcpyAsync(c->d_sto_cost.p, lt, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_sto_cost.p + ne, qtt_diag, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_sto_init_constraints(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;  // sto_.initConstraints returns when STO is disabled (:47)
  STO_LAUNCH(sto_init_kernel, c);
  return RTOC_OK;
}

// the dwell-time rows' slack / dual handed over by the host ([batch][num_events + 1] each): a warm start, or a test's iterate
int rtoc_sto_set_slack_dual(rtoc_ctx* c, const double* slack, const double* dual) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_ERR_NOT_READY;
  if (!slack || !dual) return RTOC_ERR_BAD_ARG;
  const int np = c->sto_nev + 1, NP = RTOC_STO_MAX_EVENTS + 1;
  std::vector<double> h((size_t)c->batch * RTOC_STO_CON_STRIDE, 0.0);
  for (int b = 0; b < c->batch; ++b)
    for (int p = 0; p < np; ++p) {
      if (!(slack[(size_t)b * np + p] > 0.0) || !(dual[(size_t)b * np + p] > 0.0)) return RTOC_ERR_BAD_ARG;
      h[(size_t)b * RTOC_STO_CON_STRIDE + 0 * NP + p] = slack[(size_t)b * np + p];
      h[(size_t)b * RTOC_STO_CON_STRIDE + 1 * NP + p] = dual[(size_t)b * np + p];
    }
  HIP_TRY(hipMemcpyAsync(c->d_sto_con.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_sto_correct_time_steps(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  STO_LAUNCH(sto_time_steps_kernel, c);
  return RTOC_OK;
}

static int sto_download(rtoc_ctx* c, const double* src, size_t per, double* host_out, int count) {
  if (!c->sto_on) return RTOC_ERR_NOT_READY;
  if (!host_out || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipMemcpyAsync(host_out, src, sizeof(double) * per * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}
int rtoc_sto_get_event_times(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  return sto_download(c, c->d_ts.p, c->sto_nev, host_out, count);
}
int rtoc_sto_get_time_steps(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  return sto_download(c, c->d_dt.p, c->nstages, host_out, count);
}
int rtoc_sto_get_constraint_data(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  return sto_download(c, c->d_sto_con.p, RTOC_STO_CON_STRIDE, host_out, count);
}
int rtoc_sto_get_kkt_terms(rtoc_ctx* c, double* host_lt, double* host_qtt, double* host_err_sq, int count) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_ERR_NOT_READY;
  const size_t ne = (size_t)c->batch * c->sto_nev;
  int rc = RTOC_OK;
  if (host_lt) rc = sto_download(c, c->d_sto_out.p, c->sto_nev, host_lt, count);
  if (!rc && host_qtt) rc = sto_download(c, c->d_sto_out.p + ne, c->sto_nev, host_qtt, count);
  if (!rc && host_err_sq) rc = sto_download(c, c->d_sto_out.p + 2 * ne, 1, host_err_sq, count);
  return rc;
}

// SwitchingTimeOptimization::evalKKT of every instance from the event times on the device (after rtoc_condense, like
// ocp_solver.cpp:118-119); rtoc_kkt_error's result (RTOC's d_kkterr) becomes OCPSolver::KKTError() incl. the STO term
int rtoc_sto_eval_kkt_device(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  STO_LAUNCH(sto_eval_kkt_dev_kernel, c);
  return RTOC_OK;
}
int rtoc_sto_compute_step_sizes(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  STO_LAUNCH(sto_step_sizes_kernel, c);
  return RTOC_OK;
}
int rtoc_sto_integrate_solution(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  STO_LAUNCH(sto_integrate_kernel, c);
  return RTOC_OK;
}

// ---- filter line search (line_search_filter.cpp), batched ---------------------------------------
static int ensure_filter(rtoc_ctx* c) {
  if (c->d_filter.p) return RTOC_OK;
  HIP_TRY(c->d_filter.reserve((size_t)2 * RTOC_LINE_SEARCH_FILTER_CAPACITY * c->batch));
  HIP_TRY(c->d_nfilter.reserve(c->batch));
  HIP_TRY(c->d_ls_in.reserve((size_t)2 * c->batch));
  HIP_TRY(c->d_ls_flags.reserve((size_t)2 * c->batch));
  HIP_TRY(hipMemsetAsync(c->d_nfilter.p, 0, sizeof(int) * c->batch, c->stream));
  return RTOC_OK;
}

int rtoc_line_search_clear(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_filter(c);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->d_nfilter.p, 0, sizeof(int) * c->batch, c->stream));
  return RTOC_OK;
}

int rtoc_line_search_filter(rtoc_ctx* c, const double* cost, const double* violation, const int* mask, int count,
                            double cost_rate, double viol_rate, int* accepted) {
  if (!c || !cost || !violation || !accepted || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!(cost_rate > 0.0) || !(viol_rate > 0.0)) return RTOC_ERR_BAD_ARG;  // line_search_filter.cpp:14-19
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_filter(c);
  if (rc) return rc;
  if (count == 0) return RTOC_OK;
  HIP_TRY(hipMemcpyAsync(c->d_ls_in.p, cost, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_ls_in.p + c->batch, violation, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
  if (mask) HIP_TRY(hipMemcpyAsync(c->d_ls_flags.p, mask, sizeof(int) * count, hipMemcpyHostToDevice, c->stream));
  FilterArgs a;
  a.filt = c->d_filter.p;
  a.nfilt = c->d_nfilter.p;
  a.cost = c->d_ls_in.p;
  a.viol = c->d_ls_in.p + c->batch;
  a.mask = mask ? c->d_ls_flags.p : nullptr;
  a.accepted = c->d_ls_flags.p + c->batch;
  a.count = count;
  a.cap = RTOC_LINE_SEARCH_FILTER_CAPACITY;
  a.cost_rate = cost_rate;
  a.viol_rate = viol_rate;
  a.seed_empty = 0;
  hipLaunchKernelGGL(line_search_filter_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(accepted, c->d_ls_flags.p + c->batch, sizeof(int) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// ---- DirectMultipleShooting::evalOCP's performance index and the filter line search on the device ----------------------
static int ensure_line_search(rtoc_ctx* c) {
  int rc = ensure_filter(c);
  if (rc) return rc;
  HIP_TRY(c->d_eval.reserve((size_t)4 * c->batch));
  HIP_TRY(c->d_eval_part.reserve((size_t)2 * c->batch * c->max_stages));
  HIP_TRY(c->d_ls_steps.reserve((size_t)3 * c->batch));
  HIP_TRY(c->d_ls_active.reserve((size_t)c->batch + 1));
  HIP_TRY(c->d_ls_merit.reserve((size_t)2 * c->batch));
  return RTOC_OK;
}

// (cost + cost_barrier | primal_feasibility) of every instance from the records rtoc_contact_eval_kkt has just written
// (pre-condensation) into out[2][batch]
static int launch_eval_ocp(rtoc_ctx* c, double* out) {
  if (!c->d_costval.p || !c->buf[RTOC_BUF_KKT].p || !c->buf[RTOC_BUF_CDD].p) return RTOC_ERR_NOT_READY;
  EvalOcpArgs a;
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.con = (c->nrows > 0 || c->cone_contacts > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.costval = c->d_costval.p;
  a.rows = c->d_rows.p;
  a.grid = c->d_grid.p;
  a.partial = c->d_eval_part.p;
  a.nstages = c->nstages, a.batch = c->batch, a.nrows = c->nrows;
  a.cone_contacts = c->cone_contacts, a.cone_dim = c->cone_dim > 0 ? c->cone_dim : 3, a.cone_rows = c->cone_rows;
  a.nc_max = c->dims.nc_max, a.impact_cones = c->impact_cones;
  a.nv = c->dims.nv, a.nx = c->L.nx;
  a.barrier = c->barrier;
  a.kl = c->L.kkt, a.cl = c->L.cdd, a.nl = c->L.con;
  hipLaunchKernelGGL(eval_ocp_kernel, dim3(c->nstages, c->batch), dim3(64), 0, c->stream, a);
  hipLaunchKernelGGL(eval_ocp_reduce_kernel, dim3((c->batch + 63) / 64), dim3(64), 0, c->stream, c->d_eval_part.p, out, c->nstages, c->batch);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_set_line_search(rtoc_ctx* c, int enable, double step_size_reduction_rate, double min_step_size, double filter_cost_reduction_rate,
                         double filter_constraint_violation_reduction_rate) {
  if (!c) return RTOC_ERR_BAD_ARG;
  if (enable && (!(step_size_reduction_rate > 0.0 && step_size_reduction_rate < 1.0) || !(min_step_size > 0.0) ||
                 !(filter_cost_reduction_rate > 0.0) || !(filter_constraint_violation_reduction_rate > 0.0)))
    return RTOC_ERR_BAD_ARG;
  c->ls_on = enable ? 1 : 0;
  c->ls_rate = step_size_reduction_rate, c->ls_min_step = min_step_size;
  c->ls_cost_rate = filter_cost_reduction_rate, c->ls_viol_rate = filter_constraint_violation_reduction_rate;
  c->epoch++;
  return RTOC_OK;
}

// trial = 0: DirectMultipleShooting::getEval() of the iterate rtoc_contact_eval_kkt has just linearised (records not yet condensed).
// trial = 1: dms_trial_.integratePrimalSolution(step) + evalOCP (line_search.cpp:65-71) at SOL (+) step DIR with the slacks moved
// by step x dslack, step = the primal entry of RTOC_BUF_STEP of every instance; RTOC_BUF_SOL / CON / DIR / STEP keep their
// contents, the KKT / CDD records are overwritten (the next rtoc_contact_eval_kkt rewrites them anyway).
static int eval_ocp_trial(rtoc_ctx* c, const double* steps, double* out) {
  const size_t nsol = c->want[RTOC_BUF_SOL], ncon = c->want[RTOC_BUF_CON];
  const bool has_con = c->buf[RTOC_BUF_CON].p != nullptr;
  HIP_TRY(c->d_sol_trial.reserve(nsol));
  if (has_con) HIP_TRY(c->d_con_trial.reserve(ncon));
  HIP_TRY(hipMemcpyAsync(c->d_sol_trial.p, c->buf[RTOC_BUF_SOL].p, sizeof(double) * nsol, hipMemcpyDeviceToDevice, c->stream));
  if (has_con) HIP_TRY(hipMemcpyAsync(c->d_con_trial.p, c->buf[RTOC_BUF_CON].p, sizeof(double) * ncon, hipMemcpyDeviceToDevice, c->stream));
  double* const sol = c->buf[RTOC_BUF_SOL].p;
  double* const con = c->buf[RTOC_BUF_CON].p;
  double* const stp = c->buf[RTOC_BUF_STEP].p;
  c->buf[RTOC_BUF_SOL].p = c->d_sol_trial.p;
  if (has_con) c->buf[RTOC_BUF_CON].p = c->d_con_trial.p;
  c->buf[RTOC_BUF_STEP].p = const_cast<double*>(steps);
  int rc = rtoc_update(c);                       // slack += step dslack (dual step 0)
  if (!rc) rc = rtoc_integrate_solution(c);      // SplitSolution::integrate with the trial step
  if (!rc) rc = c->ls_unconstr_dt > 0.0 ? rtoc_unconstr_eval_kkt(c, c->ls_unconstr_dt) : rtoc_contact_eval_kkt(c);   // evalOCP's quantities (and, unused here, the derivatives)
  if (!rc) rc = launch_eval_ocp(c, out);
  c->buf[RTOC_BUF_SOL].p = sol, c->buf[RTOC_BUF_CON].p = con, c->buf[RTOC_BUF_STEP].p = stp;
  c->vals_fresh = 0;
  c->fxx_state = 0;
  return rc;
}

int rtoc_contact_eval_ocp(rtoc_ctx* c, int trial, double* host_cost, double* host_violation, int count) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch || (count > 0 && (!host_cost || !host_violation))) return RTOC_ERR_BAD_ARG;
  int rc = ensure_line_search(c);
  if (rc) return rc;
  double* out = c->d_eval.p + (trial ? 2 * c->batch : 0);
  rc = trial ? eval_ocp_trial(c, c->buf[RTOC_BUF_STEP].p, out) : launch_eval_ocp(c, out);
  if (rc) return rc;
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(host_cost, out, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(host_violation, out + c->batch, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}

static int launch_filter_device(rtoc_ctx* c, const double* eval, const int* mask, int seed_empty) {
  FilterArgs a;
  a.filt = c->d_filter.p, a.nfilt = c->d_nfilter.p;
  a.cost = eval, a.viol = eval + c->batch;
  a.mask = mask;
  a.accepted = c->d_ls_flags.p + c->batch;
  a.count = c->batch, a.cap = RTOC_LINE_SEARCH_FILTER_CAPACITY;
  a.cost_rate = c->ls_cost_rate, a.viol_rate = c->ls_viol_rate;
  a.seed_empty = seed_empty;
  hipLaunchKernelGGL(line_search_filter_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// LineSearch::computeStepSize, filter method (line_search.cpp:31-83), for every instance: on entry RTOC_BUF_STEP holds the
// maximum primal steps (fraction-to-boundary), d_eval[0] the current iterates' (cost + barrier, violation) -- rtoc_newton_iteration
// evaluates them right after the linearisation; on exit the primal entries of RTOC_BUF_STEP are the accepted steps.
int rtoc_set_line_search_method(rtoc_ctx* c, int method, double armijo_control_rate, double margin_rate, double eps) {
  if (!c) return RTOC_ERR_BAD_ARG;
  if (method != 0 && method != 1) return RTOC_ERR_BAD_ARG;
  if (method == 1 && (!(armijo_control_rate > 0.0) || !(margin_rate >= 0.0) || !(eps > 0.0))) return RTOC_ERR_BAD_ARG;
  c->ls_method = method;
  if (method == 1) c->ls_armijo = armijo_control_rate, c->ls_margin = margin_rate, c->ls_eps = eps;
  c->epoch++;
  return RTOC_OK;
}

int rtoc_line_search_trials(rtoc_ctx* c, int* trials) {
  if (!c || !trials) return RTOC_ERR_BAD_ARG;
  *trials = c->ls_trials;
  return RTOC_OK;
}

int rtoc_line_search_merit_terms(rtoc_ctx* c, double* host_penalty, double* host_directional_derivative, int count) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch || !c->d_ls_merit.p) return RTOC_ERR_BAD_ARG;
  if (host_penalty) HIP_TRY(hipMemcpyAsync(host_penalty, c->d_ls_merit.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  if (host_directional_derivative)
    HIP_TRY(hipMemcpyAsync(host_directional_derivative, c->d_ls_merit.p + c->batch, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_contact_line_search(rtoc_ctx* c, int* host_trials) {
  CHECK_READY(c);
  if (!c->ls_on) return RTOC_ERR_NOT_READY;
  int rc = ensure_line_search(c);
  if (rc) return rc;
  // UnconstrLineSearch (src/line_search/unconstr_line_search.cpp) has the filter method only and ignores line_search_method: an
  // unconstrained context takes the filter path whatever rtoc_set_line_search_method said (its SOL records have no beta / mu / xi)
  const bool merit = c->ls_method == 1 && !(c->ls_unconstr_dt > 0.0);
  LsMeritArgs ma;
  if (!merit) {
    rc = launch_filter_device(c, c->d_eval.p, nullptr, 1);   // an empty filter is seeded with the current iterate (:58-62)
    if (rc) return rc;
  } else {
    // meritBacktrackingLineSearch (:87-109): penalty parameter from the multipliers of the iterate, directional derivative of the
    // merit function from ONE more trial at step eps for every instance
    if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
    LsPenaltyArgs pa;
    pa.sol = c->buf[RTOC_BUF_SOL].p, pa.grid = c->d_grid.p, pa.penalty = c->d_ls_merit.p;
    pa.nstages = c->nstages, pa.batch = c->batch, pa.nv = c->dims.nv, pa.np = c->dims.np, pa.sl = c->L.sol, pa.margin = c->ls_margin;
    hipLaunchKernelGGL(ls_penalty_kernel, dim3(c->batch), dim3(64), 0, c->stream, pa);
    ma.cur = c->d_eval.p, ma.trial = c->d_eval.p + 2 * c->batch, ma.penalty = c->d_ls_merit.p, ma.dd = c->d_ls_merit.p + c->batch;
    ma.trial_steps = c->d_ls_steps.p, ma.alpha = c->d_ls_steps.p + 2 * c->batch, ma.active = c->d_ls_active.p, ma.accepted = c->d_ls_flags.p + c->batch;
    ma.batch = c->batch, ma.eps = c->ls_eps, ma.armijo = c->ls_armijo;
    ma.phase = 0;
    hipLaunchKernelGGL(ls_merit_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, ma);
    rc = eval_ocp_trial(c, c->d_ls_steps.p, c->d_eval.p + 2 * c->batch);
    if (rc) return rc;
    ma.phase = 1;
    hipLaunchKernelGGL(ls_merit_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, ma);
    HIP_TRY(hipGetLastError());
  }
  LsArgs a;
  a.steps = c->buf[RTOC_BUF_STEP].p;
  a.trial_steps = c->d_ls_steps.p;
  a.alpha = c->d_ls_steps.p + 2 * c->batch;
  a.active = c->d_ls_active.p;
  a.accepted = c->d_ls_flags.p + c->batch;
  a.nactive = c->d_ls_active.p + c->batch;
  a.batch = c->batch;
  a.rate = c->ls_rate, a.min_step = c->ls_min_step;
  const dim3 grid((c->batch + 255) / 256), block(256);
  HIP_TRY(hipMemsetAsync(a.nactive, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(ls_begin_kernel, grid, block, 0, c->stream, a);
  int nactive = 0, trials = merit ? 1 : 0;   // (the trial at step eps counts as an evaluation)
  HIP_TRY(hipMemcpyAsync(&nactive, a.nactive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the backtracking of one instance ends once its step falls below min_step_size (line_search.cpp:64-80): at most
  // log(min_step) / log(rate) reductions from a full step; the bound only guards against a loop that never drains
  const int max_trials = (int)ceil(log(c->ls_min_step < 1.0 ? c->ls_min_step : 1.0) / log(c->ls_rate)) + 2;
  while (nactive > 0 && trials < max_trials + (merit ? 1 : 0)) {
    rc = eval_ocp_trial(c, c->d_ls_steps.p, c->d_eval.p + 2 * c->batch);
    if (rc) return rc;
    if (!merit) {
      rc = launch_filter_device(c, c->d_eval.p + 2 * c->batch, c->d_ls_active.p, 0);   // isAccepted + augment of the active instances
      if (rc) return rc;
    } else {
      ma.phase = 2;   // armijoCondition of the active instances
      hipLaunchKernelGGL(ls_merit_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream, ma);
    }
    HIP_TRY(hipMemsetAsync(a.nactive, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(ls_advance_kernel, grid, block, 0, c->stream, a);
    HIP_TRY(hipMemcpyAsync(&nactive, a.nactive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++trials;
  }
  c->ls_trials = trials;
  if (host_trials) *host_trials = trials;
  return RTOC_OK;
}

// ---- one Newton iteration of the whole batch as a single launch sequence ----------
// steps[b] <- 0 for instances whose KKT error is already below the tolerance: they keep their iterate
// kkterr holds OCPSolver::KKTError() itself (the sqrt, kkt_error.hpp); the reference tests KKTError() < kkt_tol
// (ocp_solver.cpp:200,206)
__global__ void mask_converged_kernel(double* steps, const double* kkterr, int* nconv, double tol, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  if (kkterr[b] < tol) {
    steps[2 * b] = 0.0;
    steps[2 * b + 1] = 0.0;
    atomicAdd(nconv, 1);
  }
}

static int newton_iteration_body(rtoc_ctx* c, const BwdPlan& p, double kkt_tol, double tau) {
  HIP_TRY(hipMemsetAsync(c->d_nconv.p, 0, sizeof(int), c->stream));
  int rc = launch_kkt_error(c);  // on the freshly linearised (pre-condensation) records
  if (!rc && c->ls_on) rc = launch_eval_ocp(c, c->d_eval.p);   // dms_.getEval(): cost + barrier, violation of the current iterate
  if (!rc) rc = rtoc_condense(c);
  if (!rc && c->sto_on) STO_LAUNCH(sto_eval_kkt_dev_kernel, c);   // sto_.evalKKT (ocp_solver.cpp:119); KKTError() gains the STO term
  if (!rc) rc = launch_sweep(c, p);
  if (!rc) rc = rtoc_expand(c, tau);  // directions + fraction-to-boundary step sizes, on the device
  if (rc) return rc;
  if (c->sto_on) STO_LAUNCH(sto_step_sizes_kernel, c);             // sto_.computeStepSizes, min with the stages' steps (:128-132)
  hipLaunchKernelGGL(mask_converged_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream,
                     c->buf[RTOC_BUF_STEP].p, c->d_kkterr.p, c->d_nconv.p, kkt_tol, c->batch);
  HIP_TRY(hipGetLastError());
  if (c->ls_on) {   // line_search_.computeStepSize (:133-139): the accepted primal steps replace the maximum ones
    rc = rtoc_contact_line_search(c, nullptr);
    if (rc) return rc;
  }
  rc = rtoc_update(c);
  if (!rc && c->buf[RTOC_BUF_SOL].p) rc = rtoc_integrate_solution(c);
  if (!rc && c->sto_on) STO_LAUNCH(sto_integrate_kernel, c);       // sto_.integrateSolution (:143)
  return rc;
}

int rtoc_newton_iteration(rtoc_ctx* c, double kkt_tol, double tau) {
  CHECK_READY(c);
  if (!(kkt_tol >= 0.0) || !(tau > 0.0 && tau <= 1.0)) return RTOC_ERR_BAD_ARG;
  HIP_TRY(c->d_nconv.reserve(1));
  BwdPlan p;
  int rc = plan_backward(c, &p);   // (the condensation ahead of the sweep leaves the rows of Fxx the check reads as they are)
  if (rc) return rc;
  if (c->ls_on) {   // the backtracking loop synchronises with the host: no graph replay
    rc = ensure_line_search(c);
    return rc ? rc : newton_iteration_body(c, p, kkt_tol, tau);
  }
  return run_graphed(c, &c->g_newton, kkt_tol, tau, [&]() { return newton_iteration_body(c, p, kkt_tol, tau); });
}

int rtoc_converged_count(rtoc_ctx* c, int* host_count) {
  CHECK_READY(c);
  if (!host_count) return RTOC_ERR_BAD_ARG;
  if (!c->d_nconv.p) return RTOC_ERR_NOT_READY;
  HIP_TRY(hipMemcpyAsync(host_count, c->d_nconv.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// ---- stage dump / replay --------------------------------------------------------------------
int rtoc_save_stage_dump(rtoc_ctx* c, const char* path, unsigned int mask) {
  CHECK_READY(c);
  if (!path || c->h_grid.empty()) return RTOC_ERR_BAD_ARG;
  rtoc_dump_header h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, "RTOCDMP1", 8);
  h.version = 1;
  h.header_bytes = (unsigned)sizeof(h);
  h.dims = c->dims;
  h.nstages = c->nstages;
  h.batch = c->batch;
  h.nrows = c->nrows;
  h.cone_contacts = c->cone_contacts;
  h.cone_dim = c->cone_dim;
  h.cone_rows = c->cone_contacts > 0 ? c->cone_rows : 0;
  for (int b = 0; b < RTOC_NUM_BUFFERS; ++b)
    if ((mask >> b & 1u) && c->buf[b].p) h.count[b] = buffer_count(c, b, c->nstages);
  FILE* f = fopen(path, "wb");
  if (!f) return RTOC_ERR_IO;
  bool ok = fwrite(&h, sizeof(h), 1, f) == 1 &&
            fwrite(c->h_grid.data(), sizeof(rtoc_grid), c->nstages, f) == (size_t)c->nstages &&
            (c->nrows == 0 || fwrite(c->h_rows.data(), sizeof(rtoc_box_row), c->nrows, f) == (size_t)c->nrows);
  std::vector<double> stage;
  for (int b = 0; ok && b < RTOC_NUM_BUFFERS; ++b) {
    if (!h.count[b]) continue;
    stage.resize(h.count[b]);
    if (hipMemcpyAsync(stage.data(), c->buf[b].p, h.count[b] * sizeof(double), hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      fclose(f);
      return RTOC_ERR_HIP;
    }
    ok = fwrite(stage.data(), sizeof(double), h.count[b], f) == h.count[b];
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? RTOC_OK : RTOC_ERR_IO;
}

int rtoc_load_stage_dump(const char* path, int device, rtoc_ctx** out) {
  if (!path || !out) return RTOC_ERR_BAD_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return RTOC_ERR_IO;
  rtoc_dump_header h;
  if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "RTOCDMP1", 8) != 0 || h.version != 1 ||
      h.header_bytes != sizeof(h) || h.nstages < 2 || h.batch < 1 || h.nrows < 0 || h.nrows > h.dims.nc_max) {
    fclose(f);
    return RTOC_ERR_IO;
  }
  std::vector<rtoc_grid> grid(h.nstages);
  std::vector<rtoc_box_row> rows(h.nrows > 0 ? h.nrows : 1);
  if (fread(grid.data(), sizeof(rtoc_grid), h.nstages, f) != (size_t)h.nstages ||
      (h.nrows > 0 && fread(rows.data(), sizeof(rtoc_box_row), h.nrows, f) != (size_t)h.nrows)) {
    fclose(f);
    return RTOC_ERR_IO;
  }
  rtoc_ctx* c = nullptr;
  int rc = rtoc_create(&h.dims, h.nstages, h.batch, device, &c);
  if (!rc) rc = rtoc_set_grid(c, grid.data(), h.nstages);
  if (!rc && h.nrows > 0) rc = rtoc_set_constraint_rows(c, rows.data(), h.nrows);
  if (!rc && h.cone_contacts > 0)
    rc = h.cone_rows == RTOC_WRENCH_ROWS ? rtoc_set_wrench_cones(c, h.cone_contacts)
                                         : rtoc_set_friction_cones(c, h.cone_contacts, h.cone_dim);
  std::vector<double> stage;
  for (int b = 0; !rc && b < RTOC_NUM_BUFFERS; ++b) {
    if (!h.count[b]) continue;
    if (h.count[b] != buffer_count(c, b, c->nstages)) {
      rc = RTOC_ERR_IO;
      break;
    }
    stage.resize(h.count[b]);
    if (fread(stage.data(), sizeof(double), h.count[b], f) != h.count[b]) {
      rc = RTOC_ERR_IO;
      break;
    }
    rc = rtoc_upload(c, b, 0, stage.data(), h.count[b]);
  }
  fclose(f);
  if (rc) {
    if (c) rtoc_destroy(c);
    return rc;
  }
  *out = c;
  return RTOC_OK;
}

// ---- multi-GPU: RCCL all-gather of the step directions over xGMI -----------------------------
// RCCL is resolved at run time (dlopen) so that the library has no link-time dependency on a
// particular librccl and shares the copy a host process (e.g. torch.distributed) already loaded.
int rtoc_gather_directions(rtoc_ctx* c, void* nccl_comm, double* out) {
  CHECK_READY(c);
  if (!nccl_comm || !out) return RTOC_ERR_BAD_ARG;
  typedef int (*allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
  static allgather_t fn = nullptr;
  if (!fn) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return RTOC_ERR_RCCL;
    fn = (allgather_t)dlsym(h, "ncclAllGather");
    if (!fn) return RTOC_ERR_RCCL;
  }
  const size_t count = (size_t)c->batch * c->nstages * c->L.dir.stride;
  const int nccl_float64 = 8;  // ncclFloat64 / ncclDouble
  const int rc = fn(c->buf[RTOC_BUF_DIR].p, out, count, nccl_float64, nccl_comm, c->stream);
  return rc == 0 ? RTOC_OK : RTOC_ERR_RCCL;
}

}  // extern "C"
