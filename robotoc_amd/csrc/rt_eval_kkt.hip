// rt_eval_kkt.hip -- evalKKT on the device: rigid-body model, linearisation, cost and its q_ref table, constraint rows and
// cones at the iterate, KKT error, SplitSolution::integrate; updateSolution of the unconstrained path.  (The contact schedule
// and the contact placements: rt_placements.hip.)
#include <cmath>
#include <mutex>

#include "rt_context.hpp"
#include "rigid_body.hpp"
#include "kkt_error.hpp"
#include "integrate_solution.hpp"
#include "unconstr_constraints.hpp"
#include "state_equation_lin.hpp"
#include "switching_constraint_lin.hpp"
#include "contact_constraints.hpp"
#include "contact_eval_kkt.hpp"

using namespace rtoc;

static bool model_has_surface_contacts(const rtoc_robot_model& m) {
  for (int k = 0; k < m.ncontacts; ++k)
    if (m.contact_type[k] == RTOC_CONTACT_SURFACE) return true;
  return false;
}
// hipFuncAttributeMaxDynamicSharedMemorySize is per function and process-wide, not per context: two live contexts with
// different models (iCub: 11 tree levels, ANYmal: 4) share it, so it only ever grows (the launch passes its own size).
// Every rigid-body kernel whose LDS is sized by the model is granted it here, once per model.
hipError_t rtoc::set_linearize_lds(const rtoc_robot_model& m, int nlevels, int nbranch, int dpp) {
  const size_t lin = rbd::lin_lds_bytes(nlevels, nbranch, m.njoints, m.ncontacts, m.nv, dpp, false);   // the larger of the two modes
  const struct { const void* kernel; size_t bytes; bool may_not_fit; } want[] = {
      {(const void*)rbd::linearize_contact_dynamics_kernel<true>, lin, false},       {(const void*)rbd::linearize_contact_dynamics_kernel<false>, lin, false},
      {(const void*)rbd::linearize_contact_dynamics_kernel<true, true>, lin, false}, {(const void*)rbd::linearize_contact_dynamics_kernel<false, true>, lin, false},
      {(const void*)rbd::rbd_values_kernel, 64 * rbd::VAL_DOUBLES * sizeof(double), false},
      // over the per-level carve: a tree too deep for them is accepted as long as the walk fits -- they fail where they are launched
      {(const void*)contact_cone_kernel, cc_lds_bytes(nlevels, m.njoints, m.ncontacts), true},
      {(const void*)switching_constraint_lin_kernel, sw_lds_bytes(nlevels, m.njoints, m.ncontacts), true}};
  constexpr int N = sizeof(want) / sizeof(want[0]);
  static std::mutex mu;
  static size_t granted_of[64][N] = {};   // the attribute is per DEVICE: one running maximum for each (the current one: callers hipSetDevice first)
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  for (int k = 0; k < N; ++k) {
    if (want[k].bytes <= granted_of[dev][k] || (want[k].may_not_fit && want[k].bytes > 160 * 1024)) continue;
    const hipError_t e = hipFuncSetAttribute(want[k].kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want[k].bytes);
    if (e != hipSuccess) return e;
    granted_of[dev][k] = want[k].bytes;
  }
  return hipSuccess;
}

ModelDims rtoc::model_dims(const rtoc_ctx* c) {
  const rtoc_robot_model& m = c->h_model->m;
  ModelDims d{};
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
hipError_t rtoc::reserve_active(rtoc_ctx* c, bool* fresh) { return c->d_active.reserve(c->max_stages, fresh); }
static hipError_t reserve_costval(rtoc_ctx* c) { return c->d_costval.reserve((size_t)c->batch * c->max_stages); }
hipError_t rtoc::reserve_kkterr(rtoc_ctx* c) { return c->d_kkterr.reserve((size_t)c->batch * (1 + c->max_stages)); }

// ---- SplitSolution::integrate ---------------------------------------------------------------
int rtoc_integrate_solution(rtoc_ctx* c) {
  CHECK_STAGES(c);
  if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  const auto a = view_args<IntArgs>(c);
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
  if (c->cpos.per_instance) {
    // a per-instance placement table is sized by the contacts of the model it was set for: it goes with that model
    c->cpos = {}, c->crot = {};
  }
  c->fs_on = 0, c->fs_init = 0, c->fs_size = 0;   // a foot-step planner belongs to the feet of the model it was set for
  c->h_model = std::move(h);
  HIP_TRY(hipMemcpyAsync(c->d_model.p, c->h_model.get(), sizeof(rbd::DevModel), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(set_linearize_lds(*m, c->h_model->nlevels, c->h_model->nbranch, c->h_model->dpp));
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
  const size_t need = (size_t)c->batch * c->max_stages * m.njoints * rbd::VAL_DOUBLES;
  if (c->d_vals.n < need) c->d_vals2.release();   // both grow together: the second one only on grids with an impact
  HIP_TRY(c->d_vals.grow(need));
  if (any_impact) HIP_TRY(c->d_vals2.reserve(c->d_vals.n));
  return RTOC_OK;
}

static int launch_rbd_values(rtoc_ctx* c, bool unconstr) {
  if (!c->h_model || !c->d_active.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  if (dynamics_records(c) < 1) return RTOC_OK;
  const bool any_impact = any_grid_point(c, c->nstages - 1, grid_is_impact);
  rc = ensure_rbd_values(c);
  if (rc) return rc;
  auto v = view_args<rbd::ValArgs>(c);
  v.md = model_dims(c);
  v.unconstr = unconstr ? 1 : 0;
  const int G = 64 / v.md.gs;
  const long long items = (long long)c->batch * dynamics_records(c);
  const size_t vlds = sizeof(double) * G * v.md.njoints * rbd::VAL_DOUBLES;
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
  auto a = view_args<rbd::LinArgs>(c);
  a.md = model_dims(c);
  if (!augment_residual) a.rv.kkt = nullptr;
  a.unconstr = unconstr ? 1 : 0;
  a.scale = scale;
  const int nlin = dynamics_records(c);
  if (nlin < 1) return RTOC_OK;
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
      hipLaunchKernelGGL((rbd::linearize_contact_dynamics_kernel<true, true>), dim3(c->batch * nlin), dim3(64), lds, c->stream, a);
    else
      hipLaunchKernelGGL((rbd::linearize_contact_dynamics_kernel<false, true>), dim3(c->batch * nlin), dim3(64), lds, c->stream, a);
  } else if (surf) {
    hipLaunchKernelGGL(rbd::linearize_contact_dynamics_kernel<true>, dim3(c->batch * nlin), dim3(64), lds, c->stream, a);
  } else {
    hipLaunchKernelGGL(rbd::linearize_contact_dynamics_kernel<false>, dim3(c->batch * nlin), dim3(64), lds, c->stream, a);
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
    const int n = k == 0 ? config_dim(c) : (k == 2 || k == 6 ? c->dims.nu : nv);
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

// ConfigurationSpaceCost::set_ref(std::shared_ptr<ConfigurationSpaceRefBase>) (configuration_space_cost.cpp:84-89): the answers of
// the object per grid point.  Everything is checked and staged before the context changes: a refused call leaves the table in force.
int rtoc_set_configuration_ref_table(rtoc_ctx* c, const double* q_ref, const int* active, int nstages, int per_instance) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  if (!q_ref) {
    (void)c->qtab.stage(0), (void)c->qtab_active.stage(0);   // (nothing staged)
    commit_rows(c, c->qtab, c->qtab.per_instance, 0), commit_rows(c, c->qtab_active, c->qtab.per_instance, 0);
    return RTOC_OK;
  }
  if (c->nstages < 2) return RTOC_ERR_NOT_READY;   // rtoc_set_grid
  if (nstages != c->nstages || (per_instance != 0 && per_instance != 1)) return RTOC_ERR_BAD_ARG;
  if (c->dims.np != 0 && c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  const size_t nq = config_dim(c), rows = (size_t)nstages * (per_instance ? c->batch : 1);
  std::vector<int> flags(rows, 1);
  for (size_t r = 0; r < rows; ++r) {
    if (active) flags[r] = active[r] != 0;
    if (!flags[r]) continue;   // an inactive row is never read, here or on the device
    for (size_t k = 0; k < nq; ++k)
      if (!std::isfinite(q_ref[r * nq + k])) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(stage_rows(c, c->qtab, nq, per_instance));   // both halves staged, then both committed
  HIP_TRY(stage_rows(c, c->qtab_active, 1, per_instance));
  HIP_TRY(hipMemcpyAsync(c->qtab.target(), q_ref, sizeof(double) * rows * nq, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->qtab_active.target(), flags.data(), sizeof(int) * rows, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  commit_rows(c, c->qtab, per_instance), commit_rows(c, c->qtab_active, per_instance);
  return RTOC_OK;
}
int rtoc_get_configuration_ref_table(rtoc_ctx* c, double* q_ref, int* active, int count, int* per_instance) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!c->qtab.in_force(c->nstages) || !c->qtab_active.in_force(c->nstages)) return RTOC_ERR_NOT_READY;
  if (per_instance) *per_instance = c->qtab.per_instance;
  HIP_TRY(c->qtab.download(q_ref, config_dim(c), count, c->stream));
  HIP_TRY(c->qtab_active.download(active, 1, count, c->stream));
  return RTOC_OK;
}
// The table for the kernels that read the cost table (q = nullptr without one).  RTOC_ERR_NOT_READY: a table is in use but its rows
// belong to a grid rtoc_set_grid has replaced -- never the constant q_ref in their place.
static int configuration_ref_table(const rtoc_ctx* c, QRefTable* t) {
  t->q = nullptr, t->active = nullptr, t->per_instance = 0, t->nq = 0;
  if (!c->qtab.on) return RTOC_OK;
  if (!c->qtab.in_force(c->nstages) || !c->qtab_active.in_force(c->nstages)) return RTOC_ERR_NOT_READY;
  t->q = c->qtab.buf.p, t->active = c->qtab_active.buf.p, t->per_instance = c->qtab.per_instance;
  t->nq = config_dim(c);
  return RTOC_OK;
}


int rtoc_set_initial_state(rtoc_ctx* c, const double* x0, int count) {
  if (!c || !x0 || count != c->batch) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->batch * (config_dim(c) + c->dims.nv);
  HIP_TRY(c->d_x0.reserve(n));
  HIP_TRY(hipMemcpyAsync(c->d_x0.p, x0, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// linearizeStateEquation / linearizeImpactStateEquation of every non-terminal grid point (state_equation_lin.hpp)
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
  auto a = view_args<SeLinArgs>(c);
  a.x0 = c->d_x0.p;
  a.zeroed = zeroed ? 1 : 0;
  hipLaunchKernelGGL(state_equation_lin_kernel, dim3(c->batch * c->nstages), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fxx_state = zeroed ? 1 : 0;
  return RTOC_OK;
}
int rtoc_linearize_state_equation(rtoc_ctx* c) { return launch_state_equation(c, false); }

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
  auto a = view_args<UboxArgs>(c);
  a.rows = c->d_rows.p;
  a.entry = c->d_entry.p;
  a.bounds = c->d_bounds.p;
  a.nrows = c->nrows, a.mode = mode;
  a.barrier = c->barrier, a.tau = c->ftb_rule;
  a.contact = contact ? 1 : 0;
  a.q_shift = (contact && c->dims.np == 6) ? 1 : 0;
  hipLaunchKernelGGL(unconstr_box_kernel, dim3(c->batch * dynamics_records(c)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}
static bool ubox_on(const rtoc_ctx* c) { return c->nrows > 0 && c->d_bounds.p != nullptr; }
// ... for rt_parnmpc.hip, which runs the same rows and the same dynamics on every stage of its horizon
static_assert(ROWS_INIT == UBOX_INIT && ROWS_LINEARIZE == UBOX_LINEARIZE && ROWS_CONDENSE == UBOX_CONDENSE && ROWS_EXPAND == UBOX_EXPAND,
              "UnconstrRowsPhase (rt_context.hpp) names the modes of unconstr_box_kernel");
bool rtoc::unconstr_rows_on(const rtoc_ctx* c) { return ubox_on(c); }
int rtoc::launch_unconstr_rows(rtoc_ctx* c, UnconstrRowsPhase phase) { return launch_ubox(c, (int)phase); }
int rtoc::launch_unconstr_linearize(rtoc_ctx* c, double dt) { return launch_linearize(c, 1, true, dt); }
int rtoc::reserve_empty_schedule(rtoc_ctx* c) {
  bool fresh = false;
  HIP_TRY(reserve_active(c, &fresh));
  if (fresh) HIP_TRY(hipMemsetAsync(c->d_active.p, 0, sizeof(unsigned) * c->max_stages, c->stream));  // no contacts: an all-zero schedule
  return RTOC_OK;
}

// UnconstrOCPSolver::initConstraints (unconstr_ocp_solver.cpp:91-93): setSlackAndDual of every row at the current iterate
int rtoc_unconstr_init_constraints(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!ubox_on(c) || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  return launch_ubox(c, UBOX_INIT);
}

int rtoc_unconstr_eval_kkt(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (!(dt > 0.0) || c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  if (!c->h_model || !c->d_cost.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->h_model->m.type[0] == RTOC_JOINT_FREE_FLYER || c->h_model->m.ncontacts != 0) return RTOC_ERR_BAD_ARG;  // unconstr_dynamics.cpp:22-29
  QRefTable qtab{};
  int rc = configuration_ref_table(c, &qtab);   // ahead of the first launch: a refusal leaves the records alone
  if (!rc && c->ntasks > 0) rc = task_costs_ready(c, true);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_DX0);
  if (rc) return rc;
  bool fresh = false;
  HIP_TRY(reserve_active(c, &fresh));
  if (fresh) HIP_TRY(hipMemsetAsync(c->d_active.p, 0, sizeof(unsigned) * c->max_stages, c->stream));  // no contacts: an all-zero schedule
  auto a = view_args<rbd::UkArgs>(c);
  a.cost = c->d_cost.p;
  a.x0 = c->d_x0.p;
  a.dt = dt;
  a.qtab = qtab;
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
int rtoc::launch_kkt_error(rtoc_ctx* c) {
  HIP_TRY(reserve_kkterr(c));
  auto a = view_args<KktErrArgs>(c);
  if (!(c->nrows > 0 || c->cone_contacts > 0)) a.rv.con = nullptr;   // the constraint records may exist: nothing of them counts
  a.rows = c->d_rows.p, a.nrows = c->nrows;
  a.cone = view_cones(c);
  a.partial = c->d_kkterr.p + c->batch;
  hipLaunchKernelGGL(kkt_error_kernel, dim3(c->nstages, c->batch), dim3(64), 0, c->stream, a);
  hipLaunchKernelGGL(kkt_error_reduce_kernel, dim3((c->batch + 63) / 64), dim3(64), 0, c->stream, a.partial, c->d_kkterr.p,
                     c->nstages, c->batch);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_kkt_error(rtoc_ctx* c, double* host_out, int count) {
  CHECK_STAGES(c);
  if (!host_out || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  int rc = launch_kkt_error(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(host_out, c->d_kkterr.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// the per-grid-point cost values the last evalKKT stored for evalOCP
int rtoc_get_stage_costs(rtoc_ctx* c, double* host_out, int count) {
  CHECK_READY(c);
  if (!host_out || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!c->d_costval.p) return RTOC_ERR_NOT_READY;
  HIP_TRY(hipMemcpyAsync(host_out, c->d_costval.p, sizeof(double) * count * c->nstages, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

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
  const ConeRows cone = view_cones(c);
  auto a = view_args<WcArgs>(c);
  a.md = model_dims(c);
  a.table = c->d_wcone.p;
  a.mode = mode;
  a.row0 = cone.row0, a.cone_stride = cone.stride, a.impact_cones = cone.impact;
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
  const ConeRows cone = view_cones(c);
  auto a = view_args<CcArgs>(c);
  a.md = model_dims(c);
  a.mu = c->d_mu.p;
  a.mode = mode;
  a.contact_dim = cone.dim, a.row0 = cone.row0, a.cone_stride = cone.stride, a.dgdf_off = cone.dgdf_off, a.impact_cones = cone.impact;
  a.exact_jacobian = c->exact_cone_jacobian;
  a.barrier = c->barrier;
  if (mode == CC_LINEARIZE && c->vals_fresh && c->d_vals.p) {   // kinematics already there: no tree walk (contact_cone_vals_kernel)
    CvArgs v{};
    v.c = a;
    v.vals = c->d_vals.p;
    hipLaunchKernelGGL(contact_cone_vals_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, v);
    HIP_TRY(hipGetLastError());
    return RTOC_OK;
  }
  const size_t lds = cc_lds_bytes(a.md.nlevels, a.md.njoints, a.md.ncontacts);
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
  auto a = view_args<SwLinArgs>(c);
  a.md = model_dims(c);
  a.exact_transport = c->exact_transport;
  for (int i = 0; i < c->nstages; ++i)
    if (c->h_grid[i].switching_constraint && c->h_grid[i].dims > c->dims.ns_max) return RTOC_ERR_BAD_ARG;
  a.nsel = select_grid_points(c, grid_has_switching, a.sel);
  const int per = a.nsel > 0 ? a.nsel : c->nstages - 1;
  const size_t lds = sw_lds_bytes(a.md.nlevels, a.md.njoints, a.md.ncontacts);
  hipLaunchKernelGGL(switching_constraint_lin_kernel, dim3(c->batch * per), dim3(64), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_contact_eval_kkt(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->h_model || !c->d_active.p || !c->d_cost.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  const bool switching = any_grid_point(c, c->nstages, grid_has_switching);
  QRefTable qtab{};
  int rc = configuration_ref_table(c, &qtab);   // ahead of the first launch: a refusal leaves the records alone
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  c->ls_unconstr_dt = 0.0;
  // the periodic references of the task-space costs read the per-instance grid times that the time steps below then write
  if (c->sto_on && c->ntasks > 0) {
    rc = ensure_grid_times_inst(c);
    if (rc) return rc;
  }
  // PhaseBased discretisation: time_discretization_.correctTimeSteps(contact_sequence_, t) ahead of evalKKT (ocp_solver.cpp:115-117)
  if (c->sto_on) rc = launch_sto(c, STO_TIME_STEPS);
  if (rc) return rc;
  HIP_TRY(reserve_costval(c));
  auto a = view_args<CostArgs>(c);
  a.cost = c->d_cost.p;
  a.cost_out = c->d_costval.p;
  a.qtab = qtab;
  {
    // setZero of the KKT records (+ the constant diagonals of the cost) as one stream on the context's second stream (rtoc_riccati_sweep's), BESIDE
    // the values pre-pass of the rigid-body linearisation (lanes = bodies; writes its scratch and RTOC_CDD_IDC, which nothing
    // here zeroes): the one is bound by HBM writes, the other by latency -- 1.1 ms each per 4096 x 47 grid points, one after the
    // other on one stream.  The cost kernel and everything behind it wait for both.
    auto ia = view_args<InitArgs>(c);
    ia.cost = c->d_cost.p, ia.qtab = qtab;
    const long long nrec = (long long)c->batch * c->nstages;
    // four workgroups per CU: half of the wave slots, so that the pre-pass's waves are resident beside them
    const int blocks = (int)(nrec < (long long)c->num_cus * 4 ? nrec : (long long)c->num_cus * 4);
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
      ctx_set_err(ej, __FILE_NAME__, __LINE__);
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
  // LocalContactForceCost: into the lf, Qff and hf the cost kernel has just zeroed, ahead of the cones' cone^T dual
  if (c->fcost_on) {
    rc = launch_force_cost(c, c->d_costval.p);
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

// UnconstrOCPSolver::updateSolution (src/solver/unconstr_ocp_solver.cpp:96-118) of every instance, one launch
// sequence, no host synchronisation unless host_kkt_error is asked for (here, beside the evalKKT and the box rows of that path)
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
  launch_fill_steps(c);
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
