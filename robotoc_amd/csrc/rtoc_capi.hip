// rtoc_capi.hip -- implementation of the C ABI declared in include/rtoc.h.
// Context, HBM buffers, kernel dispatch by problem dimensions.  No CPU fallback.
// The subsystems live in the rt_*.hip units beside this one; rt_context.hpp holds the context they share.
#include <dlfcn.h>

#include "rt_context.hpp"
#include "device_utils.hpp"  // d2 (stream_probe_kernel)

using namespace rtoc;

static thread_local char g_errbuf[256] = "";
void rtoc::ctx_set_err(hipError_t e, const char* file, int line) {
  snprintf(g_errbuf, sizeof(g_errbuf), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
}

int rtoc_version(void) { return 100; }

int rtoc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- streaming kernels of rtoc_bandwidth_probe: chunk = (block-wave) + k * (waves in the launch), 1 KB per wave-instruction ----
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
    ctx_set_err(e, __FILE_NAME__, __LINE__);
    return RTOC_ERR_HIP;
  }
  if (read_gbs) *read_gbs = best[0];
  if (copy_gbs) *copy_gbs = best[1];
  return RTOC_OK;
}

int rtoc_dims_supported(const rtoc_dims* dims) { return dims && find_set(dims) ? 1 : 0; }

extern "C" void rtoc_layout_for_dims(const rtoc_dims* dims, rtoc_layout* out) { rtoc_compute_layout(dims, out); }

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

int rtoc_clone(rtoc_ctx* c, rtoc_ctx** out) {
  if (!c || !out) return RTOC_ERR_BAD_ARG;
  rtoc_ctx* n = nullptr;
  int rc = rtoc_create(&c->dims, c->max_stages, c->batch, c->device, &n);
  if (rc) return rc;
  if (c->parnmpc) rc = rtoc_parnmpc_set_horizon(n, c->nstages);
  else if (c->nstages >= 2 && !c->h_grid.empty()) rc = rtoc_set_grid(n, c->h_grid.data(), c->nstages);
  if (!rc && c->nrows > 0 && !c->h_rows.empty()) rc = rtoc_set_constraint_rows(n, c->h_rows.data(), c->nrows);
  if (!rc && c->cone_contacts > 0)
    rc = c->cone_rows == RTOC_WRENCH_ROWS ? rtoc_set_wrench_cones(n, c->cone_contacts)
                                          : rtoc_set_friction_cones(n, c->cone_contacts, c->cone_dim);
  if (!rc) {
    static_cast<CtxOptions&>(*n) = *c;
    if (c->backward_scan) rc = rtoc_set_option(n, RTOC_OPT_BACKWARD_SCAN, c->backward_scan);
  }
  // what of every subsystem is state (its clone_from in rt_context.hpp), then the record buffers and the status words
  CopyChain dup{n->stream, hipStreamSynchronize(c->stream)};
  if (!rc && !n->ModelState::clone_from(*c, dup)) rc = RTOC_ERR_HIP;
  if (!rc) {
    n->ConstraintState::clone_from(*c, dup);
    n->LineSearchState::clone_from(*c, dup);
    n->StoState::clone_from(*c, dup);
    n->TaskState::clone_from(*c, dup);
    n->ParnmpcState::clone_from(*c, dup);
    n->InterpState::clone_from(*c, dup);
    n->FootStepState::clone_from(*c, dup);
    n->clone_records(*c, dup);
    if (dup.e == hipSuccess) dup.e = hipStreamSynchronize(n->stream);
  }
  if (rc || dup.e != hipSuccess) {
    if (dup.e != hipSuccess) ctx_set_err(dup.e, __FILE_NAME__, __LINE__);
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
  // the schedule and the STO time steps belong to the previous grid, unless this is the grid in force set again (a shell that
  // hands the grid over with every iteration)
  const bool same = !c->parnmpc && (int)c->h_grid.size() == nstages && c->nstages == nstages &&
                    memcmp(c->h_grid.data(), grid, sizeof(rtoc_grid) * nstages) == 0;
  if (!same) c->active_current = false, c->dt_current = false;
  c->h_grid.assign(grid, grid + nstages);
  c->nstages = nstages;
  c->parnmpc = 0;   // a grid with a terminal point: no longer the stages of rtoc_parnmpc_set_horizon
  c->fxx_state = 0;
  c->epoch++;
  if (c->sto_on) {  // the event times on the device belong to the previous grid structure unless the events are the same
    int nev = 0;
    for (int i = 0; i + 1 < nstages; ++i)
      if (grid[i].type == RTOC_GRID_IMPACT || grid[i].type == RTOC_GRID_LIFT) ++nev;
    if (nev != c->sto_nev) c->sto_on = 0;   // rtoc_sto_set_problem again
  }
  c->h_gt.clear();   // the grid times belong to the previous grid: rtoc_set_grid_times again
  forget_grid_tables(c);   // and so do the reference tables and the rows of the q_ref table (not the fact that one is in use)
  return RTOC_OK;
}

int rtoc_set_stream(rtoc_ctx* c, void* s) {
  if (!c) return RTOC_ERR_BAD_ARG;
  c->epoch++;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return RTOC_OK;
}

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

int rtoc::ensure_buffer(rtoc_ctx* c, int b) {
  if (c->buf[b].p) return RTOC_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->buf[b].reserve(c->want[b]));
  HIP_TRY(hipMemsetAsync(c->buf[b].p, 0, c->want[b] * sizeof(double), c->stream));
  c->epoch++;
  return RTOC_OK;
}

// The context as the runtime kernels see it (record_view.hpp).  Taken at every launch and never kept: rtoc_bind and the
// trial iterate of the line search (eval_ocp_trial) change the pointers between launches.
RecView rtoc::view(const rtoc_ctx* c) {
  RecView v{};
  v.sol = c->buf[RTOC_BUF_SOL].p, v.kkt = c->buf[RTOC_BUF_KKT].p, v.cdd = c->buf[RTOC_BUF_CDD].p, v.con = c->buf[RTOC_BUF_CON].p;
  v.dir = c->buf[RTOC_BUF_DIR].p, v.cone = c->buf[RTOC_BUF_CONE].p, v.se3 = c->buf[RTOC_BUF_SE3].p, v.dx0 = c->buf[RTOC_BUF_DX0].p;
  v.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  v.grid = c->d_grid.p, v.active = c->d_active.p;
  v.positions = c->cpos.rows(), v.rotations = c->crot.rows();
  v.placement_stride = c->cpos.per_instance ? c->cpos.nstages : 0;   // (the grid the rows were set for)
  v.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  v.model = c->d_model.p;
  v.nstages = c->nstages, v.batch = c->batch;
  v.all_stages = c->parnmpc ? 1 : 0;
  v.L = c->L;
  return v;
}

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
extern "C" int rtoc_debug_profile(rtoc_ctx* c, long long* host_out) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->max_stages * 32;
  if (!c->d_prof.p) {
    HIP_TRY(c->d_prof.reserve(n));
    HIP_TRY(hipMemsetAsync(c->d_prof.p, 0, n * sizeof(long long), c->stream));
    c->epoch++;   // the condensation, expansion and backward launches carry the pointer: a graph captured before holds nullptr
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
