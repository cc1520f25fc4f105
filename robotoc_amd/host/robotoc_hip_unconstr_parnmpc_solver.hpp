// robotoc_hip_unconstr_parnmpc_solver.hpp -- robotoc::UnconstrParNMPCSolver over the C ABI, the whole iteration on the device.
//
// Mirrors include/robotoc/solver/unconstr_parnmpc_solver.hpp / src/solver/unconstr_parnmpc_solver.cpp: same method names,
// argument order and checks, the solve() loop (:122-158) and its convergence test.  Backward Euler + backward correction: the
// horizon is N stages, stage i at t + (i + 1) dt, every one with dynamics and constraint rows (rtoc_parnmpc_set_horizon), and all
// of updateSolution (:97-119) runs in rtoc_parnmpc_update_solution (include/rtoc_robot.h): stage evaluation, condensation, the
// stage-parallel KKT inversions, the four correction passes with their lagged auxiliary matrices, expansion, step sizes, update.
// The OCP is robotoc_hip_unconstr_solver.hpp's UnconstrOCP: robot, ConfigurationSpaceCost, the six joint-limit components.
// Not in this mode: the line search on the backward correction (UnconstrLineSearch's second overload) -- enable_line_search
// throws --, task-space costs and a time-varying q_ref.
#ifndef ROBOTOC_HIP_UNCONSTR_PARNMPC_SOLVER_HPP_
#define ROBOTOC_HIP_UNCONSTR_PARNMPC_SOLVER_HPP_

#include <chrono>
#include <cmath>
#include <string>

#include "../../include/rtoc_robot.h"
#include "robotoc_hip_unconstr_solver.hpp"

namespace robotoc {

class UnconstrParNMPCSolver {
 public:
  explicit UnconstrParNMPCSolver(const UnconstrOCP& ocp, const SolverOptions& solver_options = SolverOptions())
      : ocp_(ocp), dt_(ocp.N > 0 ? ocp.T / ocp.N : 0.0) {
    if (ocp.T <= 0) throw std::out_of_range("[UnconstrParNMPCSolver] invalid argument: ocp.T must be positive!");  // :29-34
    if (ocp.N <= 0) throw std::out_of_range("[UnconstrParNMPCSolver] invalid argument: ocp.N must be positive!");
    if (!ocp.task_costs.empty() || ocp.configuration_ref)
      throw std::invalid_argument("[UnconstrParNMPCSolver] task-space costs and a time-varying q_ref are not part of the ParNMPC mode");
    if (ocp.constraint_rows.size() != ocp.constraint_bounds.size()) throw std::invalid_argument("[UnconstrParNMPCSolver] one bound per constraint row");
    const int nv = ocp.robot.nv;
    dims_.dimv = nv, dims_.dimu = nv, dims_.dim_passive = 0, dims_.max_dimf = 0;
    rtoc_dims d = {nv, nv, 0, 0, 0, static_cast<int>((ocp.constraint_rows.size() + 7) / 8 * 8)};
    rtoc_ctx* c = nullptr;
    check(rtoc_create(&d, ocp.N < 2 ? 2 : ocp.N, 1, ocp.device, &c), "rtoc_create");
    ctx_.reset(c, [](rtoc_ctx* p) { rtoc_destroy(p); });
    check(rtoc_get_layout(c, &L_), "rtoc_get_layout");
    check(rtoc_parnmpc_set_horizon(c, ocp.N), "rtoc_parnmpc_set_horizon");
    check(rtoc_set_robot_model(c, &ocp.robot), "rtoc_set_robot_model");
    check(rtoc_set_configuration_cost(c, &ocp.cost), "rtoc_set_configuration_cost");
    if (!ocp.constraint_rows.empty())
      check(rtoc_set_constraint_rows(c, ocp.constraint_rows.data(), static_cast<int>(ocp.constraint_rows.size())), "rtoc_set_constraint_rows");
    s_.assign(ocp.N, SplitSolution(dims_));
    setSolverOptions(solver_options);
    discretize(0.0);
    initConstraints();   // :50
  }
  UnconstrParNMPCSolver() {}
  // value semantics like the reference (unconstr_parnmpc_solver.hpp): a copy owns a deep copy of the device context (rtoc_clone:
  // buffers, model, cost, bounds, slack / dual state, the auxiliary matrices of the backward correction)
  UnconstrParNMPCSolver(const UnconstrParNMPCSolver& o)
      : ocp_(o.ocp_), dt_(o.dt_), t_(o.t_), dims_(o.dims_), L_(o.L_), s_(o.s_), time_discretization_(o.time_discretization_), solver_options_(o.solver_options_),
        solver_statistics_(o.solver_statistics_), kkt_error_(o.kkt_error_), host_solution_valid_(o.host_solution_valid_),
        device_solution_valid_(o.device_solution_valid_) {
    if (o.ctx_) {
      rtoc_ctx* c = nullptr;
      check(rtoc_clone(o.ctx_.get(), &c), "rtoc_clone");
      ctx_.reset(c, [](rtoc_ctx* p) { rtoc_destroy(p); });
    }
  }
  UnconstrParNMPCSolver& operator=(const UnconstrParNMPCSolver& o) {
    if (this != &o) {
      UnconstrParNMPCSolver tmp(o);
      *this = std::move(tmp);
    }
    return *this;
  }
  UnconstrParNMPCSolver(UnconstrParNMPCSolver&&) = default;
  UnconstrParNMPCSolver& operator=(UnconstrParNMPCSolver&&) = default;

  void setSolverOptions(const SolverOptions& solver_options) {  // :69-75
    if (solver_options.enable_line_search)
      throw std::invalid_argument("[UnconstrParNMPCSolver] enable_line_search: the line search on the backward correction "
                                  "(UnconstrLineSearch::computeStepSize over UnconstrBackwardCorrection) is not implemented on the device");
    solver_options_ = solver_options;
    if (!ocp_.constraint_rows.empty())
      check(rtoc_set_constraint_bounds(ctx_.get(), ocp_.constraint_bounds.data(), static_cast<int>(ocp_.constraint_bounds.size()),
                                       ocp_.barrier_param, solver_options.fraction_to_boundary_rule), "rtoc_set_constraint_bounds");
  }
  // discretize (:78-83): time_discretization_[i].t = dt i (the reference does not add t either)
  void discretize(const double t) {
    time_discretization_.assign(ocp_.N + 1, GridInfo());
    for (int i = 0; i <= ocp_.N; ++i) {
      GridInfo& g = time_discretization_[i];
      g.type = i == ocp_.N ? GridType::Terminal : GridType::Intermediate;   // ctor :38-49
      g.t = dt_ * i, g.dt = dt_, g.stage = i, g.stage_in_phase = i, g.num_grids_in_phase = ocp_.N;
    }
    t_ = t;
  }
  // initConstraints (:86-88): setSlackAndDual of the joint-limit rows on all N stages at the current iterate
  void initConstraints() {
    if (ocp_.constraint_rows.empty()) return;
    if (!device_solution_valid_) uploadSolution();
    check(rtoc_parnmpc_init_constraints(ctx_.get()), "rtoc_parnmpc_init_constraints");
  }
  // initBackwardCorrection (:91-94): every auxiliary matrix = the terminal-cost Hessian at the last stage's iterate
  void initBackwardCorrection() {
    if (!device_solution_valid_) uploadSolution();
    check(rtoc_parnmpc_init_backward_correction(ctx_.get()), "rtoc_parnmpc_init_backward_correction");
  }

  // updateSolution (:97-119)
  void updateSolution(const double t, const Vec& q, const Vec& v) {
    setInitialState(q, v);
    discretize(t);
    if (!device_solution_valid_) uploadSolution();
    double err = 0.0;
    check(rtoc_parnmpc_update_solution(ctx_.get(), dt_, &err, 1), "rtoc_parnmpc_update_solution");
    kkt_error_ = err;
    host_solution_valid_ = false;
    double steps[2] = {1.0, 1.0};
    if (!ocp_.constraint_rows.empty()) check(rtoc_download(ctx_.get(), RTOC_BUF_STEP, 0, steps, 2), "rtoc_download(RTOC_BUF_STEP)");
    solver_statistics_.primal_step_size.push_back(steps[0]);   // :115-116
    solver_statistics_.dual_step_size.push_back(steps[1]);
  }

  // solve (:122-158)
  void solve(const double t, const Vec& q, const Vec& v, const bool init_solver = true) {
    checkState(q, v);   // :125-130
    const auto t0 = std::chrono::high_resolution_clock::now();
    if (init_solver) {   // :134-139
      discretize(t);
      initConstraints();
      initBackwardCorrection();
    }
    solver_statistics_.clear();
    for (int iter = 0; iter < solver_options_.max_iter; ++iter) {
      updateSolution(t, q, v);
      solver_statistics_.performance_index.push_back(kkt_error_ * kkt_error_);
      if (KKTError() < solver_options_.kkt_tol) {   // :144-149
        solver_statistics_.convergence = true;
        solver_statistics_.iter = iter + 1;
        break;
      }
    }
    if (!solver_statistics_.convergence) solver_statistics_.iter = solver_options_.max_iter;   // :151-153
    if (solver_options_.enable_benchmark)
      solver_statistics_.cpu_time = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
  }

  const SolverStatistics& getSolverStatistics() const { return solver_statistics_; }
  const SplitSolution& getSolution(const int stage) {  // :166-170
    syncSolution();
    return s_.at(stage);
  }
  std::vector<Vec> getSolution(const std::string& name) {  // :173-197: N entries, not N + 1
    syncSolution();
    std::vector<Vec> out;
    for (int i = 0; i < ocp_.N; ++i) {
      if (name == "q") out.push_back(s_[i].q);
      else if (name == "v") out.push_back(s_[i].v);
      else if (name == "a") out.push_back(s_[i].a);
      else if (name == "u") out.push_back(s_[i].u);
    }
    return out;
  }
  void setSolution(const std::string& name, const Vec& value) {  // :200-218
    if (name != "q" && name != "v" && name != "a" && name != "u")
      throw std::invalid_argument("[UnconstrParNMPCSolver] invalid arugment: name must be q, v, a, or u!");
    syncSolution();
    for (int i = 0; i < ocp_.N; ++i) {
      Vec& dst = name == "q" ? s_[i].q : name == "v" ? s_[i].v : name == "a" ? s_[i].a : s_[i].u;
      if (value.size() != dst.size()) throw std::out_of_range("[UnconstrParNMPCSolver] invalid argument: value has the wrong size!");
      dst = value;
    }
    device_solution_valid_ = false;
    initConstraints();   // :217
  }
  // KKTError(t, q, v) (:221-233): evalKKT at the current iterate, without updating it
  double KKTError(const double t, const Vec& q, const Vec& v) {
    checkState(q, v);
    setInitialState(q, v);
    discretize(t);
    if (!device_solution_valid_) uploadSolution();
    check(rtoc_parnmpc_eval_kkt(ctx_.get(), dt_), "rtoc_parnmpc_eval_kkt");
    check(rtoc_kkt_error(ctx_.get(), &kkt_error_, 1), "rtoc_kkt_error");
    return kkt_error_;
  }
  double KKTError() const { return kkt_error_; }  // :236-238, of the iterate the last evalKKT linearised at
  const std::vector<GridInfo>& getTimeDiscretization() const { return time_discretization_; }  // :241-243
  double T() const { return ocp_.T; }
  int N() const { return ocp_.N; }
  rtoc_ctx* context() const { return ctx_.get(); }

 private:
  static void check(const int rc, const char* what) {
    if (rc != RTOC_OK) throw std::runtime_error(std::string("[UnconstrParNMPCSolver] ") + what + ": " + rtoc_error_string(rc));
  }
  void checkState(const Vec& q, const Vec& v) const {
    const int nv = dims_.dimv;
    if (q.size() != nv) throw std::out_of_range("[UnconstrParNMPCSolver] invalid argument: q.size() must be " + std::to_string(nv) + "!");
    if (v.size() != nv) throw std::out_of_range("[UnconstrParNMPCSolver] invalid argument: v.size() must be " + std::to_string(nv) + "!");
  }
  void setInitialState(const Vec& q, const Vec& v) {
    checkState(q, v);
    const int nv = dims_.dimv;
    std::vector<double> x0(2 * nv);
    for (int i = 0; i < nv; ++i) x0[i] = q(i), x0[nv + i] = v(i);
    check(rtoc_set_initial_state(ctx_.get(), x0.data(), 1), "rtoc_set_initial_state");
  }
  void uploadSolution() {
    std::vector<double> b(static_cast<size_t>(ocp_.N) * L_.sol.stride, 0.0);
    for (int i = 0; i < ocp_.N; ++i) StageDumpSource::packSolution(L_, s_[i], &b[static_cast<size_t>(i) * L_.sol.stride]);
    check(rtoc_upload(ctx_.get(), RTOC_BUF_SOL, 0, b.data(), b.size()), "rtoc_upload(RTOC_BUF_SOL)");
    device_solution_valid_ = host_solution_valid_ = true;
  }
  void syncSolution() {
    if (host_solution_valid_) return;
    std::vector<double> b(static_cast<size_t>(ocp_.N) * L_.sol.stride);
    check(rtoc_download(ctx_.get(), RTOC_BUF_SOL, 0, b.data(), b.size()), "rtoc_download(RTOC_BUF_SOL)");
    for (int i = 0; i < ocp_.N; ++i) StageDumpSource::unpackSolution(L_, &b[static_cast<size_t>(i) * L_.sol.stride], s_[i]);
    host_solution_valid_ = true;
  }

  UnconstrOCP ocp_;
  double dt_ = 0.0, t_ = 0.0;
  RobotDims dims_;
  std::shared_ptr<rtoc_ctx> ctx_;
  rtoc_layout L_;
  Solution s_;
  std::vector<GridInfo> time_discretization_;
  SolverOptions solver_options_;
  SolverStatistics solver_statistics_;
  double kkt_error_ = 0.0;
  bool host_solution_valid_ = true, device_solution_valid_ = false;
};

}  // namespace robotoc
#endif
