// rt_line_search.hip -- evalOCP's performance index, the filter and the backtracking line search on the device.
#include "rt_context.hpp"
#include "line_search.hpp"

using namespace rtoc;

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
  FilterArgs a{};
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
int rtoc::ensure_line_search(rtoc_ctx* c) {
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
int rtoc::launch_eval_ocp(rtoc_ctx* c, double* out) {
  if (!c->d_costval.p || !c->buf[RTOC_BUF_KKT].p || !c->buf[RTOC_BUF_CDD].p) return RTOC_ERR_NOT_READY;
  auto a = view_args<EvalOcpArgs>(c);
  if (!(c->nrows > 0 || c->cone_contacts > 0)) a.rv.con = nullptr;   // the constraint records may exist: nothing of them counts
  a.costval = c->d_costval.p;
  a.rows = c->d_rows.p, a.nrows = c->nrows;
  a.cone = view_cones(c);
  a.partial = c->d_eval_part.p;
  a.barrier = c->barrier;
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
  FilterArgs a{};
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
  LsMeritArgs ma{};
  if (!merit) {
    rc = launch_filter_device(c, c->d_eval.p, nullptr, 1);   // an empty filter is seeded with the current iterate (:58-62)
    if (rc) return rc;
  } else {
    // meritBacktrackingLineSearch (:87-109): penalty parameter from the multipliers of the iterate, directional derivative of the
    // merit function from ONE more trial at step eps for every instance
    if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
    auto pa = view_args<LsPenaltyArgs>(c);
    pa.penalty = c->d_ls_merit.p, pa.margin = c->ls_margin;
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
  LsArgs a{};
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
