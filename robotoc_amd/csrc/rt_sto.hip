// rt_sto.hip -- switching-time optimisation on the device (sto.hpp).
#include "rt_context.hpp"
#include "sto.hpp"

using namespace rtoc;

// switching-time optimisation on the device (sto.hpp): kernel arguments, one thread per instance
static int sto_count_events(const rtoc_ctx* c) {
  int n = 0;
  for (int i = 0; i + 1 < c->nstages; ++i)
    if (c->h_grid[i].type == RTOC_GRID_IMPACT || c->h_grid[i].type == RTOC_GRID_LIFT) ++n;
  return n;
}

static StoDevArgs sto_args(rtoc_ctx* c) {
  auto a = view_args<StoDevArgs>(c);
  const size_t ne = (size_t)c->batch * (c->sto_nev > 0 ? c->sto_nev : 1);
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
  a.nev = c->sto_nev;
  a.t0 = c->sto_t0, a.T = c->sto_T, a.barrier = c->sto_barrier, a.tau = c->sto_tau, a.sto_reg = c->sto_reg;
  return a;
}

// The only launches of the kernels of sto.hpp: the units that run one inside their own sequences (evalKKT, the Newton iteration,
// the grid times of the task costs) come here
int rtoc::launch_sto(rtoc_ctx* c, StoKernel k) {
  const dim3 grid((c->batch + 63) / 64), block(64);
  const StoDevArgs a = sto_args(c);
  switch (k) {
    case STO_TIME_STEPS: hipLaunchKernelGGL(sto_time_steps_kernel, grid, block, 0, c->stream, a); break;
    case STO_INIT: hipLaunchKernelGGL(sto_init_kernel, grid, block, 0, c->stream, a); break;
    case STO_EVAL_KKT: hipLaunchKernelGGL(sto_eval_kkt_dev_kernel, grid, block, 0, c->stream, a); break;
    case STO_STEP_SIZES: hipLaunchKernelGGL(sto_step_sizes_kernel, grid, block, 0, c->stream, a); break;
    case STO_INTEGRATE: hipLaunchKernelGGL(sto_integrate_kernel, grid, block, 0, c->stream, a); break;
  }
  HIP_TRY(hipGetLastError());
  if (k == STO_TIME_STEPS) c->dt_current = true;
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
  auto a = view_args<StoArgs>(c);
  a.lt = d_lt, a.qtt = d_qtt, a.err = d_err;
  a.nev = nev;
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
  return launch_sto(c, STO_TIME_STEPS);  // the time steps that belong to these event times
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
  return launch_sto(c, STO_INIT);
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
  return launch_sto(c, STO_TIME_STEPS);
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
  return launch_sto(c, STO_EVAL_KKT);
}
int rtoc_sto_compute_step_sizes(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  return launch_sto(c, STO_STEP_SIZES);
}
int rtoc_sto_integrate_solution(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->sto_on) return RTOC_OK;
  return launch_sto(c, STO_INTEGRATE);
}
