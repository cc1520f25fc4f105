// rt_parnmpc.hip -- UnconstrParNMPCSolver on the device: the horizon of N stages, the backward-Euler stage evaluation, the backward
// correction, and updateSolution as one launch sequence (include/rtoc_robot.h).
#include "rt_context.hpp"
#include "parnmpc_stage.hpp"

using namespace rtoc;

// what every entry point below needs: a ParNMPC horizon and the kernels of a fixed-base, contact-free shape
static int parnmpc_ready(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0 || c->dims.np != 0 || !c->ks->pcoarse || !c->ks->pcorrect) return RTOC_ERR_BAD_ARG;
  if (!c->parnmpc || c->nstages < 1) return RTOC_ERR_NOT_READY;
  HIP_TRY(hipSetDevice(c->device));
  return RTOC_OK;
}

static size_t aux_doubles(const rtoc_ctx* c) { return (size_t)4 * c->dims.nv * c->dims.nv; }

// the state of the backward correction, owned by the context; the auxiliary matrices start at zero
static int reserve_parnmpc(rtoc_ctx* c) {
  const size_t per = (size_t)c->batch * c->max_stages, nv = c->dims.nv;
  bool fresh = false;
  HIP_TRY(c->d_aux.reserve(per * aux_doubles(c), &fresh));
  if (fresh) {
    HIP_TRY(hipMemsetAsync(c->d_aux.p, 0, sizeof(double) * per * aux_doubles(c), c->stream));
    c->epoch++;
  }
  HIP_TRY(c->d_snew.reserve(per * 5 * nv));
  HIP_TRY(c->d_xres.reserve(per * 2 * nv));
  HIP_TRY(c->d_kinv.reserve(per * 16 * nv * nv));
  return RTOC_OK;
}

// The N stages of UnconstrParNMPCSolver's horizon (unconstr_parnmpc_solver.cpp:10-51): stage i sits at t + (i + 1) dt, every one of
// them an intermediate grid point to the kernels that ask -- dynamics and rows on all of them.  The constraint mask level is the
// one the reference's stages create their data with: stage + 1 of time_discretization[i + 1] on the intermediate stages
// (parnmpc_intermediate_stage.cpp:49), stage itself on the last one (parnmpc_terminal_stage.cpp:47).
int rtoc_parnmpc_set_horizon(rtoc_ctx* c, int N) {
  if (!c || N < 1 || N > c->max_stages) return RTOC_ERR_BAD_ARG;
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0 || c->dims.np != 0 || !c->ks->pcoarse || !c->ks->pcorrect) return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<rtoc_grid> grid((size_t)N);
  for (int i = 0; i < N; ++i) {
    rtoc_grid g = {};
    g.type = RTOC_GRID_INTERMEDIATE;
    g.num_grids_in_phase = N;
    g.time_stage = i < N - 1 ? i + 2 : N;
    grid[i] = g;
  }
  HIP_TRY(hipMemcpyAsync(c->d_grid.p, grid.data(), sizeof(rtoc_grid) * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->h_grid = grid;
  c->nstages = N;
  c->parnmpc = 1;
  c->n_stage_contact = c->n_stage_impact = 0;
  c->fxx_state = 0;
  c->vals_fresh = 0;
  c->sto_on = 0;
  c->h_gt.clear();
  forget_grid_tables(c);
  c->epoch++;
  return reserve_parnmpc(c);
}

int rtoc_parnmpc_set_aux_mat(rtoc_ctx* c, const double* host, int count) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!host || count < 1 || count > c->batch) return RTOC_ERR_BAD_ARG;
  rc = reserve_parnmpc(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_aux.p, host, sizeof(double) * count * c->nstages * aux_doubles(c), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

int rtoc_parnmpc_get_aux_mat(rtoc_ctx* c, double* host, int count) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!host || count < 1 || count > c->batch) return RTOC_ERR_BAD_ARG;
  rc = reserve_parnmpc(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(host, c->d_aux.p, sizeof(double) * count * c->nstages * aux_doubles(c), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// the checks of the entry points that evaluate the stages (rtoc_robot.h: refusals), ahead of the first launch
static int parnmpc_problem_ready(rtoc_ctx* c, double dt) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (!c->h_model || !c->d_cost.p || !c->buf[RTOC_BUF_SOL].p || !c->d_x0.p) return RTOC_ERR_NOT_READY;
  if (c->h_model->m.type[0] == RTOC_JOINT_FREE_FLYER || c->h_model->m.ncontacts != 0) return RTOC_ERR_BAD_ARG;  // unconstr_dynamics.cpp:22-29
  if (c->ntasks > 0 || c->qtab.on || c->ls_on) return RTOC_ERR_BAD_ARG;   // task-space costs, a q_ref table, the line search: not in this mode
  return RTOC_OK;
}

// UnconstrBackwardCorrection::initConstraints (unconstr_backward_correction.cpp:74-89): setSlackAndDual of every row on all N stages
int rtoc_parnmpc_init_constraints(rtoc_ctx* c) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!unconstr_rows_on(c) || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  return launch_unconstr_rows(c, ROWS_INIT);
}

// UnconstrBackwardCorrection::initAuxMat (unconstr_backward_correction.cpp:57-71)
int rtoc_parnmpc_init_backward_correction(rtoc_ctx* c) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!c->d_cost.p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  rc = reserve_parnmpc(c);
  if (rc) return rc;
  const long long nmat = (long long)c->batch * c->nstages, n = nmat * (long long)aux_doubles(c);
  hipLaunchKernelGGL(parnmpc_init_aux_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_aux.p, c->d_cost.p, c->dims.nv, nmat);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// ParNMPCIntermediateStage / ParNMPCTerminalStage::evalKKT of every stage up to (excluding) the condensations
// (parnmpc_terminal_stage.cpp:84-99; UnconstrBackwardCorrection::evalKKT, unconstr_backward_correction.cpp:123-151)
int rtoc_parnmpc_eval_kkt(rtoc_ctx* c, double dt) {
  int rc = parnmpc_problem_ready(c, dt);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_KKT);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (!rc) rc = reserve_empty_schedule(c);
  if (rc) return rc;
  auto a = view_args<PnStageArgs>(c);
  a.cost = c->d_cost.p;
  a.x0 = c->d_x0.p;
  a.dt = dt;
  c->ls_unconstr_dt = 0.0;
  hipLaunchKernelGGL(parnmpc_eval_kkt_kernel, dim3(c->batch * c->nstages), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fxx_state = 0;
  rc = launch_unconstr_linearize(c, dt);                                              // linearizeUnconstrDynamics (unconstr_dynamics.cpp:53-64)
  if (!rc && unconstr_rows_on(c)) rc = launch_unconstr_rows(c, ROWS_LINEARIZE);       // constraints_->linearizeConstraints (:94-95)
  return rc;
}

static int launch_backward_correction(rtoc_ctx* c, double dt) {
  int rc = reserve_parnmpc(c);
  if (rc) return rc;
  PbcArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.sol = c->buf[RTOC_BUF_SOL].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.aux = c->d_aux.p, a.snew = c->d_snew.p, a.xres = c->d_xres.p, a.kinv = c->d_kinv.p;
  a.status = c->d_status.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.dt = dt;
  a.kl = c->L.kkt, a.sl = c->L.sol, a.dl = c->L.dir;
  launch(c->ks->pcoarse, dim3(c->batch * c->nstages), c->stream, a);
  launch(c->ks->pcorrect, dim3(c->batch), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// UnconstrBackwardCorrection::coarseUpdate (without its evalKKT) + backwardCorrection (without its expansion)
// (unconstr_backward_correction.cpp:154-228) on the condensed records and the solution that are on the device
int rtoc_parnmpc_backward_correction(rtoc_ctx* c, double dt) {
  int rc = parnmpc_ready(c);
  if (rc) return rc;
  if (!(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  return launch_backward_correction(c, dt);
}

// UnconstrParNMPCSolver::updateSolution (unconstr_parnmpc_solver.cpp:97-119) of every instance, one launch sequence, no host
// synchronisation unless host_kkt_error is asked for
int rtoc_parnmpc_update_solution(rtoc_ctx* c, double dt, double* host_kkt_error, int count) {
  if (!c || count < 0 || count > c->batch || (count > 0 && !host_kkt_error)) return RTOC_ERR_BAD_ARG;
  int rc = parnmpc_problem_ready(c, dt);
  if (rc) return rc;
  const bool rows = unconstr_rows_on(c);
  if (rows && !c->buf[RTOC_BUF_CON].p) return RTOC_ERR_NOT_READY;   // rtoc_parnmpc_init_constraints
  rc = ensure_buffer(c, RTOC_BUF_STEP);
  if (!rc) rc = rtoc_parnmpc_eval_kkt(c, dt);                         // evalKKT of coarseUpdate (:163-179)
  if (!rc) rc = launch_kkt_error(c);                                  // performance_index.kkt_error, pre-condensation (parnmpc_terminal_stage.cpp:104-105)
  if (!rc && rows) rc = launch_unconstr_rows(c, ROWS_CONDENSE);       // constraints_->condenseSlackAndDual (:106-107)
  if (!rc) rc = rtoc_unconstr_condense(c);                            // condenseUnconstrDynamics (:108)
  if (!rc) rc = launch_backward_correction(c, dt);                    // coarseUpdate + the four passes
  if (!rc) rc = rtoc_unconstr_expand(c, dt);                          // expandPrimal / expandDual (:117-118)
  if (rc) return rc;
  launch_fill_steps(c);
  HIP_TRY(hipGetLastError());
  if (rows) rc = launch_unconstr_rows(c, ROWS_EXPAND);                // expandSlackAndDual + the step sizes (:119, :123-132)
  if (!rc && rows) rc = rtoc_update(c);                               // updateSlack / updateDual (:143, :151)
  if (!rc) rc = rtoc_integrate_solution(c);                           // s.integrate (:142)
  if (rc) return rc;
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(host_kkt_error, c->d_kkterr.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}
