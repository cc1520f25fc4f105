// rt_task_costs.hip -- the task-space cost terms of evalKKT: terms, grid times, reference tables, the launch; the contact-force
// cost term of the contact path.
#include "rt_context.hpp"
#include "task_space_cost.hpp"
#include "contact_force_cost.hpp"

using namespace rtoc;

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
  c->h_task_table = 0, c->h_task_3d = c->h_task_com = (1u << nterms) - 1u;
  for (size_t i = 0; i < n; ++i) {
    const unsigned bit = 1u << (i % nterms);
    if (terms[i].ref_kind == RTOC_REF_TABLE) c->h_task_table |= bit;
    if (terms[i].kind != RTOC_TASK_FRAME_3D) c->h_task_3d &= ~bit;
    if (terms[i].kind != RTOC_TASK_COM) c->h_task_com &= ~bit;
  }
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
  HIP_TRY(stage_rows(c, c->reftab[term], 1, per_instance));
  HIP_TRY(hipMemcpyAsync(c->reftab[term].target(), entries, sizeof(rtoc_task_ref_entry) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  commit_rows(c, c->reftab[term], per_instance ? 1 : 0);
  return RTOC_OK;
}

int rtoc_get_task_ref_table(rtoc_ctx* c, int term, rtoc_task_ref_entry* entries, int count, int* per_instance) {
  CHECK_READY(c);
  if (term < 0 || term >= RTOC_MAX_TASK_COSTS || count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!c->reftab[term].in_force(c->nstages)) return RTOC_ERR_NOT_READY;
  if (per_instance) *per_instance = c->reftab[term].per_instance;
  HIP_TRY(c->reftab[term].download(entries, 1, count, c->stream));
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
int rtoc::ensure_grid_times_inst(rtoc_ctx* c) {
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
    rc = launch_sto(c, STO_TIME_STEPS);
    if (rc) return rc;
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
int rtoc::task_costs_ready(rtoc_ctx* c, bool unconstr) {
  if (!c->h_model || !c->d_model.p || !c->d_tasks.p) return RTOC_ERR_NOT_READY;
  const bool sto = c->sto_on && !unconstr;
  if (!sto && (int)c->h_gt.size() != c->nstages) return RTOC_ERR_NOT_READY;   // rtoc_set_grid_times
  if (sto && !c->d_gt_inst.p) return RTOC_ERR_NOT_READY;   // allocated by rtoc_contact_eval_kkt ahead of the time steps
  for (int k = 0; k < c->ntasks; ++k)
    if (((c->h_task_table >> k) & 1u) && !c->reftab[k].in_force(c->nstages)) return RTOC_ERR_NOT_READY;   // rtoc_set_task_ref_table
  return RTOC_OK;
}

// unconstr_dt > 0: from rtoc_unconstr_eval_kkt(dt) -- always the extended instantiation, which knows that path's scaling
int rtoc::launch_task_costs(rtoc_ctx* c, double unconstr_dt, double* cost_out) {
  const bool unconstr = unconstr_dt > 0.0;
  int rc = task_costs_ready(c, unconstr);
  if (rc) return rc;
  const bool sto = c->sto_on && !unconstr;
  auto a = view_args<TaskCostArgs>(c);
  a.cost_out = cost_out;
  a.terms = c->d_tasks.p;
  a.t_fixed = sto ? nullptr : c->d_gt.p;
  a.t_inst = sto ? c->d_gt_inst.p : nullptr;
  a.nterms = c->ntasks, a.per_instance = c->tasks_per_instance;
  for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) a.tab[k] = (k < c->ntasks && ((c->h_task_table >> k) & 1u)) ? c->reftab[k].buf.p : nullptr;
  for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) a.tab_inst |= (unsigned)c->reftab[k].per_instance << k;
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

// ---- LocalContactForceCost (contact_force_cost.hpp) ----
int rtoc_set_contact_force_cost(rtoc_ctx* c, const rtoc_contact_force_cost* cost, int per_instance) {
  if (!c) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  if (!cost) {
    if (c->fcost_on) c->epoch++;   // the kernel leaves the captured launch sequence
    c->fcost_on = 0;
    return RTOC_OK;
  }
  if (!c->h_model) return RTOC_ERR_NOT_READY;
  if (c->dims.nf_max == 0) return RTOC_ERR_BAD_ARG;
  const int n = per_instance ? c->batch : 1, nc = c->h_model->m.ncontacts;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < nc; ++k)
      for (int j = 0; j < 3; ++j) {
        const double w = cost[i].f_weight[k][j], wi = cost[i].fi_weight[k][j];
        if (!(w >= 0.0) || !std::isfinite(w) || !(wi >= 0.0) || !std::isfinite(wi)) return RTOC_ERR_BAD_ARG;
        if (!std::isfinite(cost[i].f_ref[k][j]) || !std::isfinite(cost[i].fi_ref[k][j])) return RTOC_ERR_BAD_ARG;
      }
  bool fresh = false;
  HIP_TRY(c->d_fcost.reserve((size_t)c->batch, &fresh));   // full capacity: a later call may switch to per-instance terms
  HIP_TRY(hipMemcpyAsync(c->d_fcost.p, cost, sizeof(rtoc_contact_force_cost) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // captured graphs bake the launch, the pointer and the per-instance flag in
  if (fresh || !c->fcost_on || c->fcost_per_instance != (per_instance ? 1 : 0)) c->epoch++;
  c->fcost_on = 1, c->fcost_per_instance = per_instance ? 1 : 0;
  return RTOC_OK;
}

int rtoc::launch_force_cost(rtoc_ctx* c, double* cost_out) {
  if (!c->h_model || !c->d_fcost.p || !c->d_active.p) return RTOC_ERR_NOT_READY;
  const rtoc_robot_model& m = c->h_model->m;
  auto a = view_args<ForceCostArgs>(c);
  a.cost = c->d_fcost.p;
  a.cost_out = cost_out;
  a.per_instance = c->fcost_per_instance;
  a.ncontacts = m.ncontacts;
  a.surface = 0;
  for (int k = 0; k < m.ncontacts; ++k)
    if (m.contact_type[k] == RTOC_CONTACT_SURFACE) a.surface |= 1u << k;
  const long long items = (long long)c->batch * c->nstages;
  hipLaunchKernelGGL(contact_force_cost_kernel, dim3((unsigned)((items + FCOST_GP - 1) / FCOST_GP)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}
