// robotoc_hip_device_source.hpp -- a StageDataSource that linearises ON THE DEVICE.
//
// The OCPSolver shell (robotoc_hip_solver.hpp) takes the Pinocchio / cost half of evalKKT from a StageDataSource.  For an
// OCP whose cost is a ConfigurationSpaceCost and whose Constraints object holds joint limits and friction cones
// (examples/anymal/trot.cpp:131-146), that half exists on the device as well (include/rtoc_robot.h: rtoc_contact_eval_kkt =
// cost + inequality rows + state equation on the manifold + rigid-body linearisation + switching constraints): with this
// source nothing of OCPSolver::updateSolution (src/solver/ocp_solver.cpp:111-145) runs on the host -- the solution stays
// resident in RTOC_BUF_SOL, the host sees KKT errors and, on request, the iterate.
#ifndef ROBOTOC_HIP_DEVICE_SOURCE_HPP_
#define ROBOTOC_HIP_DEVICE_SOURCE_HPP_

#include "../../include/rtoc_robot.h"
#include "robotoc_hip_solver.hpp"
#include "robotoc_hip_task_costs.hpp"

namespace robotoc {

class ConfigurationCostSource : public StageDataSource {
 public:
  // grid: the discretisation (TimeDiscretization of the contact sequence); active[i]: contact mask of grid point i;
  // contact_positions: [grid point][contact][3]; s0: initial guess
  ConfigurationCostSource(const rtoc_robot_model& model, const rtoc_configuration_cost& cost, const std::vector<GridInfo>& grid,
                          const std::vector<unsigned>& active, const std::vector<double>& contact_positions, const Solution& s0)
      : model_(model), cost_(cost), td_(grid), active_(active), cpos_(contact_positions), s0_(s0) {
    if (active.size() != grid.size() || contact_positions.size() != grid.size() * static_cast<size_t>(model.ncontacts) * 3)
      throw std::invalid_argument("[ConfigurationCostSource] one contact mask and ncontacts positions per grid point");
  }
  // The same with TaskSpace3DCost / CoMCost / TaskSpace6DCost components beside the ConfigurationSpaceCost (the cost function's
  // other components, evaluated on the device by rtoc_contact_eval_kkt); their periodic references read GridInfo::t of `grid`, a
  // user's TaskSpace6DRefBase is asked once per grid point of `grid` (a table on the device).
  ConfigurationCostSource(const rtoc_robot_model& model, const rtoc_configuration_cost& cost,
                          const std::vector<std::shared_ptr<TaskCostComponent>>& task_costs, const std::vector<GridInfo>& grid,
                          const std::vector<unsigned>& active, const std::vector<double>& contact_positions, const Solution& s0)
      : ConfigurationCostSource(model, cost, grid, active, contact_positions, s0) {
    setTaskCosts(task_costs);
  }
  // The same OCP described like the reference describes it: contact sequence + horizon (OCP::contact_sequence, T, N) instead of
  // a ready-made grid, optionally with STOConstraints (an OCP with an STO problem: PhaseBased discretisation, ocp_solver.cpp:46-48).
  // The source then owns the discretisation: OCPSolver::discretize(t) re-runs TimeDiscretization::discretize at the sequence's
  // current event times (mesh refinement).  s0: initial guess over the N + 1 + lifts + 2 impacts grid points of discretize(t = 0).
  ConfigurationCostSource(const rtoc_robot_model& model, const rtoc_configuration_cost& cost, const ContactSequence& contact_sequence,
                          const double T, const int N, const Solution& s0, const std::shared_ptr<STOConstraints>& sto_constraints = nullptr)
      : model_(model), cost_(cost), s0_(s0), cs_(new ContactSequence(contact_sequence)), sto_(sto_constraints), T_(T), N_(N) {
    if (!(T > 0.0)) throw std::out_of_range("[OCPSolver] invalid argument: ocp.T must be positive!");
    if (N <= 0) throw std::out_of_range("[OCPSolver] invalid argument: ocp.N must be positive!");
    if (contact_sequence.numContacts() != model.ncontacts) throw std::invalid_argument("[ConfigurationCostSource] the contact sequence is for another robot");
    discretize(0.0);
  }
  // the task-space components of the cost (before the solver is constructed); empty: the configuration cost alone
  void setTaskCosts(const std::vector<std::shared_ptr<TaskCostComponent>>& task_costs) {
    if (task_costs.size() > static_cast<size_t>(RTOC_MAX_TASK_COSTS)) throw std::invalid_argument("[ConfigurationCostSource] at most RTOC_MAX_TASK_COSTS task-space costs");
    tasks_.clear();
    for (const auto& c : task_costs) {
      if (!c) throw std::invalid_argument("[ConfigurationCostSource] null task-space cost");
      tasks_.push_back(c->term());
    }
    task_costs_ = task_costs;
  }
  // a LocalContactForceCost component of the cost (before the solver is constructed); null: none
  void setContactForceCost(const std::shared_ptr<LocalContactForceCost>& force_cost) { force_cost_ = force_cost; }
  // ConfigurationSpaceCost::set_ref (configuration_space_cost.cpp:84-89): a time-varying q_ref in place of cost.q_ref, asked at every
  // grid point of the grid in force after every (re-)discretisation -- with switching-time optimisation at the grid's own times,
  // which the switching times then move without the object being asked again until the next mesh refinement.  nullptr: back to
  // the constant reference (set_q_ref's use_nonconst_ref_ = false)
  void setConfigurationRef(const std::shared_ptr<ConfigurationSpaceRefBase>& ref) {
    config_ref_ = ref;
    config_ref_dirty_ = true;
  }
  // Every instance of the context's batch on its own footholds (rtoc_set_contact_placements, per_instance = 1), in place of the
  // placements the batch shares: positions [batch][grid point][contact][3], rotations the same with [9] (row-major) or empty
  // (identity), for the grid in force; the contact masks stay those of the schedule.  batch = 0: back to the shared placements.
  // A source that owns its discretisation forgets them at the next discretize(): they belong to the grid they were given for.
  void setContactPlacements(const std::vector<double>& positions, const std::vector<double>& rotations, const int batch) {
    const size_t rows = static_cast<size_t>(batch < 0 ? 0 : batch) * td_.size() * static_cast<size_t>(model_.ncontacts);
    if (batch < 0 || positions.size() != rows * 3 || (!rotations.empty() && rotations.size() != rows * 9))
      throw std::invalid_argument("[ConfigurationCostSource] per-instance placements: batch x grid points x ncontacts positions (x 3) and rotations (x 9) or none");
    cpos_inst_ = positions, crot_inst_ = rotations, batch_inst_ = batch;
    scheduled_ = false;
  }
  ContactSequence* contactSequence() override { return cs_.get(); }
  const STOConstraints* stoConstraints() const override { return sto_.get(); }
  double horizonLength() const override { return T_; }
  const std::vector<unsigned>* contactMasks() const override { return &active_; }
  int maxGridPoints() const override {
    return cs_ ? N_ + 1 + cs_->numLiftEvents() + 2 * cs_->numImpactEvents() : td_.size();
  }
  bool discretize(const double t) override {
    config_ref_dirty_ = true;   // the solver sets the grid again after this, whoever owns the discretisation
    if (!cs_) return false;
    td_ = robotoc::discretize(*cs_, T_, N_, t, static_cast<bool>(sto_));
    contactSchedule(*cs_, td_, active_, cpos_, &crot_);
    cpos_inst_.clear(), crot_inst_.clear(), batch_inst_ = 0;
    scheduled_ = false;
    return true;
  }
  RobotDims robot() const override {
    const bool ff = model_.type[0] == RTOC_JOINT_FREE_FLYER;
    int dimf = 0;
    for (int k = 0; k < model_.ncontacts; ++k) dimf += model_.contact_type[k] == RTOC_CONTACT_SURFACE ? 6 : 3;
    RobotDims r;
    r.dimv = model_.nv, r.dimu = ff ? model_.nv - 6 : model_.nv, r.dim_passive = ff ? 6 : 0, r.max_dimf = dimf;
    return r;
  }
  // ---- the Constraints object (before the solver is constructed) ----
  // JointPosition{Lower,Upper}Limit, JointVelocity{Lower,Upper}Limit, JointTorques{Lower,Upper}Limit in the order
  // examples/anymal/trot.cpp:134-146 adds them; every vector has dimu entries (the actuated joints)
  void setJointLimits(const std::vector<double>& q_min, const std::vector<double>& q_max, const std::vector<double>& v_max,
                      const std::vector<double>& u_max) {
    const RobotDims r = robot();
    const size_t nu = static_cast<size_t>(r.dimu);
    if (q_min.size() != nu || q_max.size() != nu || v_max.size() != nu || u_max.size() != nu)
      throw std::invalid_argument("[ConfigurationCostSource] joint limits: dimu entries each");
    rows_.clear(), bounds_.clear();
    const int vars[3] = {RTOC_VAR_Q, RTOC_VAR_V, RTOC_VAR_U}, levels[3] = {2, 1, 0};
    for (int k = 0; k < 3; ++k)
      for (int sign = -1; sign <= 1; sign += 2)
        for (int j = 0; j < r.dimu; ++j) {
          rtoc_box_row w;
          w.var = vars[k], w.index = k == 2 ? j : r.dim_passive + j, w.sign = sign, w.level = levels[k];
          rows_.push_back(w);
          // g = sign z - bound <= 0: upper z - z_max, lower z_min - z
          bounds_.push_back(k == 0 ? (sign > 0 ? q_max[j] : -q_min[j]) : (k == 1 ? v_max[j] : u_max[j]));
        }
  }
  // FrictionCone with ContactStatus::frictionCoefficient mu[k]; impact_cone: ImpactFrictionCone as well
  void setFrictionCone(const std::vector<double>& mu, const bool impact_cone = false) {
    if (mu.size() != static_cast<size_t>(model_.ncontacts)) throw std::invalid_argument("[ConfigurationCostSource] one friction coefficient per contact");
    mu_ = mu, impact_cone_ = impact_cone;
  }
  void setBarrierParam(const double barrier_param, const double fraction_to_boundary_rule) {
    barrier_ = barrier_param, ftb_ = fraction_to_boundary_rule;
  }
  int ncMax() const override {
    const int n = static_cast<int>(rows_.size()) + (mu_.empty() ? 0 : 5 * model_.ncontacts);
    return (n + 7) & ~7;
  }
  const TimeDiscretization& timeDiscretization() const override { return td_; }
  void configure(rtoc_ctx* ctx) override {
    chk(rtoc_set_robot_model(ctx, &model_), "rtoc_set_robot_model");
    chk(rtoc_set_configuration_cost(ctx, &cost_), "rtoc_set_configuration_cost");
    if (!tasks_.empty()) chk(rtoc_set_task_costs(ctx, tasks_.data(), static_cast<int>(tasks_.size()), 0), "rtoc_set_task_costs");
    if (force_cost_) {
      const rtoc_contact_force_cost fc = force_cost_->term();
      chk(rtoc_set_contact_force_cost(ctx, &fc, 0), "rtoc_set_contact_force_cost");
    }
    if (!rows_.empty()) {
      chk(rtoc_set_constraint_rows(ctx, rows_.data(), static_cast<int>(rows_.size())), "rtoc_set_constraint_rows");
      chk(rtoc_set_constraint_bounds(ctx, bounds_.data(), static_cast<int>(bounds_.size()), barrier_, ftb_), "rtoc_set_constraint_bounds");
    }
    if (!mu_.empty()) {
      const int cd = model_.contact_type[0] == RTOC_CONTACT_SURFACE ? 6 : 3;
      chk(rtoc_set_friction_cones(ctx, model_.ncontacts, cd), "rtoc_set_friction_cones");
      chk(rtoc_set_friction_coefficients(ctx, mu_.data(), model_.ncontacts), "rtoc_set_friction_coefficients");
      chk(rtoc_set_option(ctx, RTOC_OPT_IMPACT_CONES, impact_cone_ ? 1 : 0), "rtoc_set_option");
      chk(rtoc_set_barrier_param(ctx, barrier_, ftb_), "rtoc_set_barrier_param");
    }
    scheduled_ = false;
    config_ref_dirty_ = true;
  }
  void setContactSchedule(rtoc_ctx* ctx) override { schedule(ctx); }
  void initConstraints(rtoc_ctx* ctx, const Solution&) override {
    schedule(ctx);
    if (!rows_.empty() || !mu_.empty()) chk(rtoc_contact_init_constraints(ctx), "rtoc_contact_init_constraints");
  }
  void setInitialState(rtoc_ctx* ctx, const Vec& q, const Vec& v) override {
    std::vector<double> x0(q.size() + v.size());
    for (int i = 0; i < q.size(); ++i) x0[i] = q(i);
    for (int i = 0; i < v.size(); ++i) x0[q.size() + i] = v(i);
    chk(rtoc_set_initial_state(ctx, x0.data(), 1), "rtoc_set_initial_state");
  }
  void linearize(rtoc_ctx* ctx, const Solution&) override {
    schedule(ctx);
    if (!tasks_.empty()) {   // GridInfo::t of the grid in force (rtoc_set_grid forgets them; with STO the device keeps its own)
      std::vector<double> t(td_.size());
      for (int i = 0; i < td_.size(); ++i) t[i] = td_[i].t;
      chk(rtoc_set_grid_times(ctx, t.data(), td_.size()), "rtoc_set_grid_times");
      // references that are the user's objects, and the DiscreteTime references: updateRef / isActive at every grid point of the
      // grid in force -- after every (re-)discretisation, mesh refinement included; stage_in_phase / num_grids_in_phase are
      // structural, so the tables stay valid while the switching times move
      for (size_t k = 0; k < task_costs_.size(); ++k) {
        if (!task_costs_[k]->usesTable()) continue;
        std::vector<GridInfo> grid(td_.size());
        for (int i = 0; i < td_.size(); ++i) grid[i] = td_[i];
        const std::vector<rtoc_task_ref_entry> tab = task_costs_[k]->refTable(grid);
        chk(rtoc_set_task_ref_table(ctx, static_cast<int>(k), tab.data(), static_cast<int>(tab.size()), 0), "rtoc_set_task_ref_table");
      }
    }
    // the q_ref table, where the task tables are filled: rtoc_set_grid forgot its rows, and evalKKT refuses to run without them
    if (config_ref_dirty_) {
      if (config_ref_) {
        std::vector<GridInfo> grid(td_.size());
        for (int i = 0; i < td_.size(); ++i) grid[i] = td_[i];
        const ConfigurationRefTable tab = configurationRefTable(*config_ref_, model_, cost_, grid);
        chk(rtoc_set_configuration_ref_table(ctx, tab.q_ref.data(), tab.active.data(), td_.size(), 0), "rtoc_set_configuration_ref_table");
      } else {
        chk(rtoc_set_configuration_ref_table(ctx, nullptr, nullptr, 0, 0), "rtoc_set_configuration_ref_table");
      }
      config_ref_dirty_ = false;
    }
    chk(rtoc_contact_eval_kkt(ctx), "rtoc_contact_eval_kkt");
  }
  // computed on the device with the linearisation (state_equation.cpp:99-109, Fqq_prev_inv correction included)
  bool initialStateDirectionOnDevice() const override { return true; }
  bool needsHostSolution() const override { return false; }
  void initialStateDirection(const Vec&, const Vec&, const Solution&, Vec&) const override {}
  void initialSolution(Solution& s) const override {
    for (size_t i = 0; i < s.size() && i < s0_.size(); ++i) s[i] = s0_[i];
  }

 private:
  void schedule(rtoc_ctx* ctx) {
    if (scheduled_) return;  // needs the grid, which the solver sets after configure()
    chk(rtoc_set_contact_schedule(ctx, active_.data(), cpos_.data(), crot_.empty() ? nullptr : crot_.data()), "rtoc_set_contact_schedule");
    if (batch_inst_ > 0)   // the masks above, the placements of every instance here
      chk(rtoc_set_contact_placements(ctx, cpos_inst_.data(), crot_inst_.empty() ? nullptr : crot_inst_.data(), 1), "rtoc_set_contact_placements");
    scheduled_ = true;
  }
  static void chk(const int rc, const char* what) {
    if (rc != RTOC_OK) throw std::runtime_error(std::string("[ConfigurationCostSource] ") + what + ": " + rtoc_error_string(rc));
  }
  rtoc_robot_model model_;
  rtoc_configuration_cost cost_;
  TimeDiscretization td_;
  std::vector<unsigned> active_;
  std::vector<double> cpos_;
  std::vector<double> crot_;   // [grid point][contact][9] or empty (surface contacts: ContactSequence rotations)
  std::vector<double> cpos_inst_, crot_inst_;   // setContactPlacements: the same with a leading [batch_inst_]; batch_inst_ = 0: none
  int batch_inst_ = 0;
  Solution s0_;
  std::vector<rtoc_task_cost> tasks_;
  std::vector<std::shared_ptr<TaskCostComponent>> task_costs_;
  std::shared_ptr<LocalContactForceCost> force_cost_;
  std::shared_ptr<ConfigurationSpaceRefBase> config_ref_;
  bool config_ref_dirty_ = false;   // the device's table (or its absence) is not what config_ref_ says
  std::vector<rtoc_box_row> rows_;
  std::vector<double> bounds_, mu_;
  bool impact_cone_ = false;
  double barrier_ = 1.0e-3, ftb_ = 0.995;
  bool scheduled_ = false;
  std::shared_ptr<ContactSequence> cs_;
  std::shared_ptr<STOConstraints> sto_;
  double T_ = 0.0;
  int N_ = 0;
};

}  // namespace robotoc
#endif
