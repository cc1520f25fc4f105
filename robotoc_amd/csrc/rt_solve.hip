// rt_solve.hip -- the solver iterations: the iteration schedule, updateSolution of the contact path, the Newton iteration.
#include "rt_context.hpp"

using namespace rtoc;

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

// ---- one Newton iteration of the whole batch as a single launch sequence ----------
// steps[b] <- 0 for instances whose KKT error is already below the tolerance: they keep their iterate
// kkterr holds OCPSolver::KKTError() itself (the sqrt, kkt_error.hpp); the reference tests KKTError() < kkt_tol
// (ocp_solver.cpp:200,206).  C linkage: the name the kernel has always had in the library's code object.
extern "C" __global__ void mask_converged_kernel(double* steps, const double* kkterr, int* nconv, double tol, int batch) {
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
  if (!rc && c->sto_on) rc = launch_sto(c, STO_EVAL_KKT); // sto_.evalKKT (ocp_solver.cpp:119); KKTError() gains the STO term
  if (!rc) rc = launch_sweep(c, p);
  if (!rc) rc = rtoc_expand(c, tau);  // directions + fraction-to-boundary step sizes, on the device
  if (rc) return rc;
  if (c->sto_on) rc = launch_sto(c, STO_STEP_SIZES);        // sto_.computeStepSizes, min with the stages' steps (:128-132)
  if (rc) return rc;
  hipLaunchKernelGGL(mask_converged_kernel, dim3((c->batch + 255) / 256), dim3(256), 0, c->stream,
                     c->buf[RTOC_BUF_STEP].p, c->d_kkterr.p, c->d_nconv.p, kkt_tol, c->batch);
  HIP_TRY(hipGetLastError());
  if (c->ls_on) {   // line_search_.computeStepSize (:133-139): the accepted primal steps replace the maximum ones
    rc = rtoc_contact_line_search(c, nullptr);
    if (rc) return rc;
  }
  rc = rtoc_update(c);
  if (!rc && c->buf[RTOC_BUF_SOL].p) rc = rtoc_integrate_solution(c);
  if (!rc && c->sto_on) rc = launch_sto(c, STO_INTEGRATE); // sto_.integrateSolution (:143)
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
