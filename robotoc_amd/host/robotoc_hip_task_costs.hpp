// robotoc_hip_task_costs.hpp -- TaskSpace3DCost, CoMCost, TaskSpace6DCost, PeriodicSwingFootRef, PeriodicCoMRef,
// DiscreteTimeSwingFootRef, DiscreteTimeCoMRef, TaskSpace6DRefBase and LocalContactForceCost with the reference's constructors
// and setters (src/cost/task_space_3d_cost.cpp, com_cost.cpp, task_space_6d_cost.cpp, periodic_swing_foot_ref.cpp,
// periodic_com_ref.cpp, discrete_time_swing_foot_ref.cpp, discrete_time_com_ref.cpp, local_contact_force_cost.cpp,
// include/robotoc/cost/task_space_6d_ref_base.hpp).
// They describe the terms; rtoc_contact_eval_kkt / rtoc_unconstr_eval_kkt evaluate them on the device (include/rtoc_robot.h:
// rtoc_task_cost).  Hand them to the ConfigurationCostSource overload of robotoc_hip_device_source.hpp or to UnconstrOCP::task_costs
// (robotoc_hip_unconstr_solver.hpp).  Header-only, C++11.
//
// A TaskSpace6DRefBase is the user's own class (the reference ships no concrete one): the shells call its updateRef / isActive
// once per grid point when they discretise and hand the device a table (rtoc_set_task_ref_table).  The DiscreteTime references
// reach the device the same way: they are functions of a grid point's place in its contact phase, not of its time.  The table
// fill asks a reference only where the term's weight for that kind of grid point is non-zero and isActive holds (com_cost.cpp:95,
// 137, 178), and refuses a reference that is not finite: on impact and terminal grid points num_grids_in_phase is 0 and the
// DiscreteTime references' rate is 0 / 0.
//
// A frame is a contact frame of the model table (its index k: contact_parent[k], contact_p[k]) or a parent joint with an offset
// in that joint's frame: the world position of a frame depends on its origin only.  isActive / updateRef restate the reference's
// loops on the host (set-up and checks); the device runs the same loops.
#ifndef ROBOTOC_HIP_TASK_COSTS_HPP_
#define ROBOTOC_HIP_TASK_COSTS_HPP_

#include <array>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include <vector>

#include "../../include/rtoc_robot.h"
#include "robotoc_hip.hpp"
#include "robotoc_hip_planner.hpp"

namespace robotoc {

typedef std::array<double, 3> Vector3d;
typedef std::array<double, 9> Matrix3d;   // row-major

// pinocchio::SE3 as the cost classes use it: SE3(rotation, translation)
struct SE3 {
  Matrix3d R;
  Vector3d p;
  SE3() : R(Matrix3d{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}}), p(Vector3d{{0.0, 0.0, 0.0}}) {}
  SE3(const Matrix3d& rotation, const Vector3d& translation) : R(rotation), p(translation) {}
  const Matrix3d& rotation() const { return R; }
  const Vector3d& translation() const { return p; }
};

// include/robotoc/cost/task_space_6d_ref_base.hpp
class TaskSpace6DRefBase {
 public:
  virtual ~TaskSpace6DRefBase() {}
  virtual void updateRef(const GridInfo& grid_info, SE3& ref_6d) const = 0;
  virtual bool isActive(const GridInfo& grid_info) const = 0;
};

class TaskSpace3DRefBase {
 public:
  virtual ~TaskSpace3DRefBase() {}
  virtual bool isActive(const double t) const = 0;
  virtual Vector3d updateRef(const double t) const = 0;
  virtual void fill(rtoc_task_cost& s) const = 0;
  // The reference's own signatures (task_space_3d_ref_base.hpp, com_ref_base.hpp): what the table fill calls.  A reference
  // of the grid time alone keeps overriding the forms above.
  virtual bool isActive(const GridInfo& grid_info) const { return isActive(grid_info.t); }
  virtual Vector3d updateRef(const GridInfo& grid_info) const { return updateRef(grid_info.t); }
  // true: served to the device as a table with one entry per grid point (fill then sets RTOC_REF_TABLE)
  virtual bool usesTable() const { return false; }
};
typedef TaskSpace3DRefBase CoMRefBase;

namespace detail {
inline bool allZero(const double* w, const int n) {
  for (int k = 0; k < n; ++k)
    if (w[k] != 0.0) return false;
  return true;
}
inline void checkFiniteRef(const char* name, const GridInfo& g, const double* x, const int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(x[k]))
      throw std::invalid_argument(std::string("[") + name + "] the reference at grid point " + std::to_string(g.stage) + " (phase " +
                                  std::to_string(g.phase) + ", stage " + std::to_string(g.stage_in_phase) + " of " +
                                  std::to_string(g.num_grids_in_phase) + " in it) is not finite");
}
// stage_in_phase / num_grids_in_phase as the reference divides them (0 / 0 on impact and terminal grid points)
inline double phaseRate(const GridInfo& g) { return static_cast<double>(g.stage_in_phase) / static_cast<double>(g.num_grids_in_phase); }
}  // namespace detail

// include/robotoc/cost/configuration_space_ref_base.hpp: a time-varying q_ref of the ConfigurationSpaceCost
// (ConfigurationSpaceCost::set_ref), the model table in place of Robot.  The user's own class: the shells call updateRef /
// isActive once per grid point when they discretise and hand the device a table (rtoc_set_configuration_ref_table).
// q_ref arrives sized nq: [x y z qx qy qz qw, joints] with a free-flyer base.
class ConfigurationSpaceRefBase {
 public:
  virtual ~ConfigurationSpaceRefBase() {}
  virtual void updateRef(const rtoc_robot_model& robot, const GridInfo& grid_info, Vec& q_ref) const = 0;
  virtual bool isActive(const GridInfo& grid_info) const = 0;
};

// The table of a ConfigurationSpaceRefBase over `grid`: q_ref[grid point][nq], active[grid point].  The reference's order of
// questions (configuration_space_cost.cpp:251-442, configuration_space_cost.hpp:166-216): isActive only where the q weight of the
// grid point's kind is not all zero (enable_q_cost_ / _terminal_ / _impact_), updateRef only where the reference is active; a
// reference that is not finite is refused.  Rows that were not asked for stay zero and inactive.
struct ConfigurationRefTable {
  std::vector<double> q_ref;
  std::vector<int> active;
};
inline ConfigurationRefTable configurationRefTable(const ConfigurationSpaceRefBase& ref, const rtoc_robot_model& robot,
                                                   const rtoc_configuration_cost& cost, const std::vector<GridInfo>& grid) {
  ConfigurationRefTable tab;
  const size_t nq = static_cast<size_t>(robot.nq);
  tab.q_ref.assign(grid.size() * nq, 0.0), tab.active.assign(grid.size(), 0);
  for (size_t i = 0; i < grid.size(); ++i) {
    const GridInfo& g = grid[i];
    const double* const w = g.type == GridType::Terminal ? cost.q_weight_terminal : (g.type == GridType::Impact ? cost.q_weight_impact : cost.q_weight);
    if (detail::allZero(w, robot.nv) || !ref.isActive(g)) continue;
    Vec q(robot.nq);
    ref.updateRef(robot, g, q);
    if (q.size() != robot.nq) throw std::invalid_argument("[ConfigurationSpaceCost] the reference at grid point " + std::to_string(g.stage) + " has the wrong size");
    detail::checkFiniteRef("ConfigurationSpaceCost", g, q.data(), robot.nq);
    tab.active[i] = 1;
    for (size_t k = 0; k < nq; ++k) tab.q_ref[i * nq + k] = q(static_cast<int>(k));
  }
  return tab;
}

class PeriodicSwingFootRef : public TaskSpace3DRefBase {
 public:
  PeriodicSwingFootRef(const Vector3d& x3d0, const Vector3d& step_length, const double step_height, const double t0,
                       const double period_swing, const double period_stance, const bool is_first_step_half) {
    setFootTrackRef(x3d0, step_length, step_height, t0, period_swing, period_stance, is_first_step_half);
  }
  void setFootTrackRef(const Vector3d& x3d0, const Vector3d& step_length, const double step_height, const double t0,
                       const double period_swing, const double period_stance, const bool is_first_step_half) {
    x3d0_ = x3d0, step_length_ = step_length, step_height_ = step_height, t0_ = t0;
    period_swing_ = period_swing, period_stance_ = period_stance, period_ = period_swing + period_stance;
    is_first_step_half_ = is_first_step_half;
  }
  Vector3d updateRef(const double t) const override {
    Vector3d x = x3d0_;
    double rate;
    if (t < t0_ + period_swing_) {
      rate = (t - t0_) / period_swing_;
      for (int k = 0; k < 3; ++k) x[k] += (is_first_step_half_ ? 0.5 * rate : rate) * step_length_[k];
    } else {
      int i = 1;
      while (!(t < t0_ + i * period_ + period_swing_)) ++i;
      rate = (t - t0_ - i * period_) / period_swing_;
      for (int k = 0; k < 3; ++k) x[k] += (is_first_step_half_ ? (i - 0.5 + rate) : (i + rate)) * step_length_[k];
    }
    if (rate < 0.5) x[2] += 2 * rate * step_height_;
    else x[2] += 2 * (1 - rate) * step_height_;
    return x;
  }
  bool isActive(const double t) const override {
    for (int i = 0;; ++i) {
      if (t < t0_ + i * period_) return false;
      if (t < t0_ + i * period_ + period_swing_) return true;
    }
  }
  void fill(rtoc_task_cost& s) const override {
    s.ref_kind = RTOC_REF_PERIODIC_FOOT, s.first_half = is_first_step_half_ ? 1 : 0;
    for (int k = 0; k < 3; ++k) s.x0[k] = x3d0_[k], s.rate[k] = step_length_[k];
    s.step_height = step_height_, s.t0 = t0_, s.period_active = period_swing_, s.period_inactive = period_stance_;
  }

 private:
  Vector3d x3d0_, step_length_;
  double step_height_, t0_, period_swing_, period_stance_, period_;
  bool is_first_step_half_;
};

class PeriodicCoMRef : public CoMRefBase {
 public:
  PeriodicCoMRef(const Vector3d& com_ref0, const Vector3d& vcom_ref, const double t0, const double period_active,
                 const double period_inactive, const bool is_first_move_half) {
    setCoMRef(com_ref0, vcom_ref, t0, period_active, period_inactive, is_first_move_half);
  }
  void setCoMRef(const Vector3d& com_ref0, const Vector3d& vcom_ref, const double t0, const double period_active,
                 const double period_inactive, const bool is_first_move_half) {
    com_ref0_ = com_ref0, vcom_ref_ = vcom_ref, t0_ = t0;
    period_active_ = period_active, period_inactive_ = period_inactive, period_ = period_active + period_inactive;
    is_first_move_half_ = is_first_move_half;
  }
  Vector3d updateRef(const double t) const override {
    double tau;
    if (t < t0_ + period_active_) {
      tau = is_first_move_half_ ? 0.5 * (t - t0_) : (t - t0_);
    } else {
      int i = 1;
      while (!(t < t0_ + i * period_ + period_active_)) ++i;
      const double t1 = t - t0_ - i * period_;
      tau = is_first_move_half_ ? ((i - 0.5) * period_active_ + t1) : (i * period_active_ + t1);
    }
    Vector3d x;
    for (int k = 0; k < 3; ++k) x[k] = com_ref0_[k] + tau * vcom_ref_[k];
    return x;
  }
  bool isActive(const double t) const override {
    for (int i = 0;; ++i) {
      if (t < t0_ + i * period_) return false;
      if (t < t0_ + i * period_ + period_active_) return true;
    }
  }
  void fill(rtoc_task_cost& s) const override {
    s.ref_kind = RTOC_REF_PERIODIC_COM, s.first_half = is_first_move_half_ ? 1 : 0;
    for (int k = 0; k < 3; ++k) s.x0[k] = com_ref0_[k], s.rate[k] = vcom_ref_[k];
    s.step_height = 0.0, s.t0 = t0_, s.period_active = period_active_, s.period_inactive = period_inactive_;
  }

 private:
  Vector3d com_ref0_, vcom_ref_;
  double t0_, period_active_, period_inactive_, period_;
  bool is_first_move_half_;
};

// src/cost/discrete_time_swing_foot_ref.cpp
class DiscreteTimeSwingFootRef : public TaskSpace3DRefBase {
 public:
  DiscreteTimeSwingFootRef(const int contact_index, const double swing_height)
      : contact_index_(contact_index), num_contact_phases_(1), step_height_(swing_height), first_rate_(0.0), last_rate_(0.0) {}
  void setSwingFootRef(const ContactSequence& contact_sequence) {
    contact_position_.clear(), is_contact_active_.clear();
    num_contact_phases_ = contact_sequence.numContactPhases();
    for (int phase = 0; phase < num_contact_phases_; ++phase) {
      const std::vector<double>& p = contact_sequence.phasePositions(phase);
      contact_position_.push_back(Vector3d{{p.at(3 * contact_index_), p.at(3 * contact_index_ + 1), p.at(3 * contact_index_ + 2)}});
      is_contact_active_.push_back(((contact_sequence.phaseMask(phase) >> contact_index_) & 1u) != 0);
    }
    contact_position_.push_back(contact_position_.back());
    first_rate_ = 1.0, last_rate_ = 1.0;
  }
  void setSwingFootRef(const ContactSequence& contact_sequence, const Vector3d& first_contact_position, const Vector3d& last_contact_position,
                       const double first_rate, const double last_rate) {
    setSwingFootRef(contact_sequence);
    contact_position_[0] = first_contact_position;
    contact_position_[num_contact_phases_] = last_contact_position;
    first_rate_ = first_rate, last_rate_ = last_rate;
  }
  void setSwingFootRef(const std::shared_ptr<ContactSequence>& contact_sequence) { setSwingFootRef(*contact_sequence); }
  void setSwingFootRef(const std::shared_ptr<ContactSequence>& contact_sequence, const Vector3d& first_contact_position,
                       const Vector3d& last_contact_position, const double first_rate, const double last_rate) {
    setSwingFootRef(*contact_sequence, first_contact_position, last_contact_position, first_rate, last_rate);
  }
  Vector3d updateRef(const GridInfo& grid_info) const override {
    Vector3d x = Vector3d{{0.0, 0.0, 0.0}};
    if (is_contact_active_.at(grid_info.phase)) return x;   // the reference leaves its argument alone where the foot stands
    double rate = detail::phaseRate(grid_info);
    if (grid_info.phase == 0) rate = first_rate_ * (1.0 - rate) + rate;
    else if (grid_info.phase == num_contact_phases_ - 1) rate = last_rate_ * (1.0 - rate) + rate;
    const Vector3d& a = contact_position_[grid_info.phase == 0 ? 0 : grid_info.phase - 1];
    const Vector3d& b = contact_position_[grid_info.phase == 0 ? 1 : grid_info.phase + 1];
    for (int k = 0; k < 3; ++k) x[k] = (1.0 - rate) * a[k] + rate * b[k];
    if (rate < 0.5) x[2] += 2.0 * rate * step_height_;
    else x[2] += 2.0 * (1.0 - rate) * step_height_;
    return x;
  }
  bool isActive(const GridInfo& grid_info) const override { return !is_contact_active_.at(grid_info.phase); }
  // not a function of the time
  bool isActive(const double) const override { throw std::logic_error("[DiscreteTimeSwingFootRef] isActive needs the GridInfo"); }
  Vector3d updateRef(const double) const override { throw std::logic_error("[DiscreteTimeSwingFootRef] updateRef needs the GridInfo"); }
  bool usesTable() const override { return true; }
  void fill(rtoc_task_cost& s) const override { s.ref_kind = RTOC_REF_TABLE; }

 private:
  int contact_index_, num_contact_phases_;
  double step_height_, first_rate_, last_rate_;
  std::vector<Vector3d> contact_position_;
  std::vector<bool> is_contact_active_;
};

// src/cost/discrete_time_com_ref.cpp
class DiscreteTimeCoMRef : public CoMRefBase {
 public:
  explicit DiscreteTimeCoMRef(const std::vector<Vector3d>& com_to_contact_position)
      : com_to_contact_position_(com_to_contact_position), num_contact_phases_(1), first_rate_(0.0), last_rate_(0.0) {}
  void setCoMRef(const ContactSequence& contact_sequence) {
    com_position_.clear(), has_inactive_contacts_.clear();
    num_contact_phases_ = contact_sequence.numContactPhases();
    const int nc = contact_sequence.numContacts();
    if (com_to_contact_position_.size() != static_cast<size_t>(nc)) throw std::invalid_argument("[DiscreteTimeCoMRef] one com_to_contact_position per contact");
    bool has_active_contacts_prev = true;
    for (int phase = 0; phase < num_contact_phases_; ++phase) {
      const std::vector<double>& p = contact_sequence.phasePositions(phase);
      const unsigned mask = contact_sequence.phaseMask(phase);
      int num_active_contacts = 0;
      Vector3d com_avg = Vector3d{{0.0, 0.0, 0.0}};
      for (int i = 0; i < nc; ++i) {
        if ((mask >> i) & 1u) {
          for (int k = 0; k < 3; ++k) com_avg[k] += p.at(3 * i + k);
          for (int k = 0; k < 3; ++k) com_avg[k] -= com_to_contact_position_[i][k];
          ++num_active_contacts;
        }
      }
      if (num_active_contacts > 0)
        for (int k = 0; k < 3; ++k) com_avg[k] *= (1.0 / static_cast<double>(num_active_contacts));
      com_position_.push_back(com_avg);
      has_inactive_contacts_.push_back(num_active_contacts < nc);
      if (!has_active_contacts_prev && phase > 1) com_position_[phase - 1] = mean(com_position_[phase - 2], com_position_[phase]);
      has_active_contacts_prev = num_active_contacts > 0;
    }
    com_position_.push_back(com_position_.back());
  }
  void setCoMRef(const ContactSequence& contact_sequence, const Vector3d& first_com_ref, const Vector3d& last_com_ref, const double first_rate,
                 const double last_rate) {
    setCoMRef(contact_sequence);
    const int n = num_contact_phases_;
    com_position_[0] = first_com_ref;
    com_position_[n] = last_com_ref;
    if (n > 1) {
      if (contact_sequence.phaseMask(1) == 0u) com_position_[1] = mean(com_position_[0], com_position_[2]);
      if (contact_sequence.phaseMask(n - 1) == 0u) com_position_[n - 1] = mean(com_position_[n - 2], com_position_[n]);
    }
    first_rate_ = first_rate, last_rate_ = last_rate;
  }
  void setCoMRef(const std::shared_ptr<ContactSequence>& contact_sequence) { setCoMRef(*contact_sequence); }
  void setCoMRef(const std::shared_ptr<ContactSequence>& contact_sequence, const Vector3d& first_com_ref, const Vector3d& last_com_ref,
                 const double first_rate, const double last_rate) {
    setCoMRef(*contact_sequence, first_com_ref, last_com_ref, first_rate, last_rate);
  }
  Vector3d updateRef(const GridInfo& grid_info) const override {
    const int ph = grid_info.phase;
    if (!has_inactive_contacts_.at(ph)) return com_position_[ph];
    double rate = detail::phaseRate(grid_info);
    if (ph == 0) rate = first_rate_ * (1.0 - rate) + rate;
    else if (ph == num_contact_phases_ - 1) rate = last_rate_ * (1.0 - rate) + rate;
    Vector3d x;
    for (int k = 0; k < 3; ++k) x[k] = (1.0 - rate) * com_position_[ph][k] + rate * com_position_[ph + 1][k];
    return x;
  }
  bool isActive(const GridInfo&) const override { return true; }
  bool isActive(const double) const override { return true; }
  Vector3d updateRef(const double) const override { throw std::logic_error("[DiscreteTimeCoMRef] updateRef needs the GridInfo"); }
  bool usesTable() const override { return true; }
  void fill(rtoc_task_cost& s) const override { s.ref_kind = RTOC_REF_TABLE; }

 private:
  static Vector3d mean(const Vector3d& a, const Vector3d& b) { return Vector3d{{0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1]), 0.5 * (a[2] + b[2])}}; }
  std::vector<Vector3d> com_position_, com_to_contact_position_;
  std::vector<bool> has_inactive_contacts_;
  int num_contact_phases_;
  double first_rate_, last_rate_;
};

// the weights, references and checks the two components share (CostFunctionComponentBase's part of them)
class TaskCostComponent {
 public:
  virtual ~TaskCostComponent() {}
  void set_ref(const std::shared_ptr<TaskSpace3DRefBase>& ref) { ref_ = ref; }
  void set_const_ref(const Vector3d& const_ref) { const_ref_ = const_ref, ref_.reset(); }
  void set_weight(const Vector3d& weight) { check(weight, "weight"), weight_ = weight; }
  void set_weight_terminal(const Vector3d& weight_terminal) { check(weight_terminal, "weight_terminal"), weight_terminal_ = weight_terminal; }
  void set_weight_impact(const Vector3d& weight_impact) { check(weight_impact, "weight_impact"), weight_impact_ = weight_impact; }
  bool isCostActive(const double t) const { return ref_ ? ref_->isActive(t) : true; }
  bool isCostActive(const GridInfo& grid_info) const { return ref_ ? ref_->isActive(grid_info) : true; }
  // the device description of the term
  virtual rtoc_task_cost term() const {
    rtoc_task_cost s = rtoc_task_cost();
    for (int k = 0; k < 3; ++k) s.weight[k] = weight_[k], s.weight_terminal[k] = weight_terminal_[k], s.weight_impact[k] = weight_impact_[k];
    if (ref_) {
      ref_->fill(s);
    } else {
      s.ref_kind = RTOC_REF_CONST;
      for (int k = 0; k < 3; ++k) s.x0[k] = const_ref_[k];
    }
    return s;
  }
  // a reference that is the user's object: one rtoc_task_ref_entry per grid point (rtoc_set_task_ref_table)
  virtual bool usesTable() const { return ref_ && ref_->usesTable(); }
  virtual std::vector<rtoc_task_ref_entry> refTable(const std::vector<GridInfo>& grid) const {
    std::vector<rtoc_task_ref_entry> out(usesTable() ? grid.size() : 0);
    for (size_t i = 0; i < out.size(); ++i) {
      out[i] = rtoc_task_ref_entry();
      out[i].R[0] = out[i].R[4] = out[i].R[8] = 1.0;
      const GridInfo& g = grid[i];
      const Vector3d& w = g.type == GridType::Terminal ? weight_terminal_ : (g.type == GridType::Impact ? weight_impact_ : weight_);
      if (detail::allZero(w.data(), 3)) continue;   // enable_cost_ / _terminal_ / _impact_: the reference is not asked
      out[i].active = ref_->isActive(g) ? 1 : 0;
      if (!out[i].active) continue;                 // updateRef is only called where the reference is active
      const Vector3d x = ref_->updateRef(g);
      detail::checkFiniteRef(name_, g, x.data(), 3);
      for (int k = 0; k < 3; ++k) out[i].p[k] = x[k];
    }
    return out;
  }

 protected:
  explicit TaskCostComponent(const char* name) : name_(name) {}
  void check(const Vector3d& w, const char* what) const {
    if (w[0] < 0.0 || w[1] < 0.0 || w[2] < 0.0)
      throw std::invalid_argument(std::string("[") + name_ + "] invalid argument: elements of '" + what + "' must be non-negative!");
  }
  const char* name_;
  Vector3d const_ref_ = Vector3d{{0.0, 0.0, 0.0}}, weight_ = Vector3d{{0.0, 0.0, 0.0}};
  Vector3d weight_terminal_ = Vector3d{{0.0, 0.0, 0.0}}, weight_impact_ = Vector3d{{0.0, 0.0, 0.0}};
  std::shared_ptr<TaskSpace3DRefBase> ref_;
};

class TaskSpace3DCost : public TaskCostComponent {
 public:
  // TaskSpace3DCost(robot, frame_id): a contact frame of the model table
  TaskSpace3DCost(const rtoc_robot_model& robot, const int contact_frame) : TaskCostComponent("TaskSpace3DCost") {
    if (contact_frame < 0 || contact_frame >= robot.ncontacts) throw std::out_of_range("[TaskSpace3DCost] no such contact frame");
    parent_ = robot.contact_parent[contact_frame];
    for (int k = 0; k < 3; ++k) offset_[k] = robot.contact_p[contact_frame][k];
  }
  TaskSpace3DCost(const rtoc_robot_model& robot, const int contact_frame, const std::shared_ptr<TaskSpace3DRefBase>& ref)
      : TaskSpace3DCost(robot, contact_frame) { set_ref(ref); }
  TaskSpace3DCost(const rtoc_robot_model& robot, const int contact_frame, const Vector3d& const_ref)
      : TaskSpace3DCost(robot, contact_frame) { set_const_ref(const_ref); }
  // any other frame: its parent joint and its origin in that joint's frame
  TaskSpace3DCost(const rtoc_robot_model& robot, const int parent_joint, const Vector3d& offset, const std::shared_ptr<TaskSpace3DRefBase>& ref)
      : TaskCostComponent("TaskSpace3DCost"), parent_(parent_joint), offset_(offset) {
    if (parent_joint < 0 || parent_joint >= robot.njoints) throw std::out_of_range("[TaskSpace3DCost] no such joint");
    set_ref(ref);
  }
  rtoc_task_cost term() const override {
    rtoc_task_cost s = TaskCostComponent::term();
    s.kind = RTOC_TASK_FRAME_3D, s.frame_parent = parent_;
    for (int k = 0; k < 3; ++k) s.frame_p[k] = offset_[k];
    return s;
  }

 private:
  int parent_ = 0;
  Vector3d offset_ = Vector3d{{0.0, 0.0, 0.0}};
};

class CoMCost : public TaskCostComponent {
 public:
  explicit CoMCost(const rtoc_robot_model&) : TaskCostComponent("CoMCost") {}
  CoMCost(const rtoc_robot_model& robot, const std::shared_ptr<CoMRefBase>& ref) : CoMCost(robot) { set_ref(ref); }
  CoMCost(const rtoc_robot_model& robot, const Vector3d& const_ref) : CoMCost(robot) { set_const_ref(const_ref); }
  rtoc_task_cost term() const override {
    rtoc_task_cost s = TaskCostComponent::term();
    s.kind = RTOC_TASK_COM;
    return s;
  }
};

// src/cost/task_space_6d_cost.cpp.  The model table keeps no frames beyond the contacts, so a frame is its parent joint and its
// placement in that joint's frame (model.frames[frame_id].parent / .placement).
class TaskSpace6DCost : public TaskCostComponent {
 public:
  TaskSpace6DCost(const rtoc_robot_model& robot, const int parent_joint, const SE3& frame_placement)
      : TaskCostComponent("TaskSpace6DCost"), parent_(parent_joint), frame_(frame_placement) {
    if (parent_joint < 0 || parent_joint >= robot.njoints) throw std::out_of_range("[TaskSpace6DCost] no such joint");
    for (int k = 0; k < 6; ++k) weight6_[k] = weight6_terminal_[k] = weight6_impact_[k] = 0.0;
  }
  TaskSpace6DCost(const rtoc_robot_model& robot, const int parent_joint, const SE3& frame_placement, const std::shared_ptr<TaskSpace6DRefBase>& ref)
      : TaskSpace6DCost(robot, parent_joint, frame_placement) { set_ref(ref); }
  TaskSpace6DCost(const rtoc_robot_model& robot, const int parent_joint, const SE3& frame_placement, const SE3& const_ref)
      : TaskSpace6DCost(robot, parent_joint, frame_placement) { set_const_ref(const_ref); }
  TaskSpace6DCost(const rtoc_robot_model& robot, const int parent_joint, const SE3& frame_placement, const Vector3d& const_position_ref,
                  const Matrix3d& const_rotation_ref)
      : TaskSpace6DCost(robot, parent_joint, frame_placement) { set_const_ref(const_position_ref, const_rotation_ref); }

  void set_ref(const std::shared_ptr<TaskSpace6DRefBase>& ref) { ref6_ = ref; }
  void set_const_ref(const SE3& const_ref) { const_ref6_ = const_ref, ref6_.reset(); }
  void set_const_ref(const Vector3d& const_position_ref, const Matrix3d& const_rotation_ref) { set_const_ref(SE3(const_rotation_ref, const_position_ref)); }
  void set_weight(const Vector3d& weight_position, const Vector3d& weight_rotation) {
    fill(weight6_, weight_position, weight_rotation, "weight_position", "weight_rotation");
  }
  void set_weight_terminal(const Vector3d& weight_position_terminal, const Vector3d& weight_rotation_terminal) {
    fill(weight6_terminal_, weight_position_terminal, weight_rotation_terminal, "weight_position_terminal", "weight_rotation_terminal");
  }
  void set_weight_impact(const Vector3d& weight_position_impact, const Vector3d& weight_rotation_impact) {
    fill(weight6_impact_, weight_position_impact, weight_rotation_impact, "weight_position_impact", "weight_rotation_impact");
  }
  bool isCostActive(const GridInfo& grid_info) const { return ref6_ ? ref6_->isActive(grid_info) : true; }

  rtoc_task_cost term() const override {
    rtoc_task_cost s = rtoc_task_cost();
    s.kind = RTOC_TASK_FRAME_6D, s.frame_parent = parent_;
    for (int k = 0; k < 3; ++k) s.frame_p[k] = frame_.p[k];
    for (int k = 0; k < 9; ++k) s.frame_R[k] = frame_.R[k], s.ref_R[k] = k % 4 == 0 ? 1.0 : 0.0;
    // the six weights in the order they multiply d = [linear; angular] (include/rtoc_robot.h: WEIGHT ORDER): the first triple is
    // what the caller passed as weight_rotation, the second what they passed as weight_position -- the reference as written
    for (int k = 0; k < 3; ++k) {
      s.weight[k] = weight6_[k], s.weight_angular[k] = weight6_[3 + k];
      s.weight_terminal[k] = weight6_terminal_[k], s.weight_angular_terminal[k] = weight6_terminal_[3 + k];
      s.weight_impact[k] = weight6_impact_[k], s.weight_angular_impact[k] = weight6_impact_[3 + k];
    }
    if (ref6_) {
      s.ref_kind = RTOC_REF_TABLE;
    } else {
      s.ref_kind = RTOC_REF_CONST;
      for (int k = 0; k < 3; ++k) s.x0[k] = const_ref6_.p[k];
      for (int k = 0; k < 9; ++k) s.ref_R[k] = const_ref6_.R[k];
    }
    return s;
  }
  bool usesTable() const override { return static_cast<bool>(ref6_); }
  std::vector<rtoc_task_ref_entry> refTable(const std::vector<GridInfo>& grid) const override {
    std::vector<rtoc_task_ref_entry> out(ref6_ ? grid.size() : 0);
    for (size_t i = 0; i < out.size(); ++i) {
      SE3 ref;   // updateRef is only called where the reference is active (task_space_6d_cost.hpp:200-209)
      const GridInfo& g = grid[i];
      const double* const w = g.type == GridType::Terminal ? weight6_terminal_ : (g.type == GridType::Impact ? weight6_impact_ : weight6_);
      out[i].active = (!detail::allZero(w, 6) && ref6_->isActive(g)) ? 1 : 0, out[i].pad = 0;
      if (out[i].active) {
        ref6_->updateRef(g, ref);
        detail::checkFiniteRef(name_, g, ref.R.data(), 9), detail::checkFiniteRef(name_, g, ref.p.data(), 3);
      }
      for (int k = 0; k < 9; ++k) out[i].R[k] = ref.R[k];
      for (int k = 0; k < 3; ++k) out[i].p[k] = ref.p[k];
    }
    return out;
  }

 private:
  // task_space_6d_cost.cpp:114-127, as written: weight_.head<3>() = weight_rotation, weight_.tail<3>() = weight_position, and
  // weight_ multiplies Log6Map(...) = [linear; angular] componentwise -- `weight_rotation` weights the linear components
  void fill(double* w6, const Vector3d& wp, const Vector3d& wr, const char* np, const char* nr) const {
    check(wp, np), check(wr, nr);
    for (int k = 0; k < 3; ++k) w6[k] = wr[k], w6[3 + k] = wp[k];
  }
  int parent_ = 0;
  SE3 frame_, const_ref6_;
  double weight6_[6], weight6_terminal_[6], weight6_impact_[6];
  std::shared_ptr<TaskSpace6DRefBase> ref6_;
};

// src/cost/local_contact_force_cost.cpp: weights on the first three components of every active contact's force (wrench) in the
// contact's local frame; f_* on intermediate / lift grid points, fi_* on impact grid points.  Evaluated on the device by
// rtoc_contact_eval_kkt (rtoc_set_contact_force_cost); hand it to ConfigurationCostSource::setContactForceCost.
class LocalContactForceCost {
 public:
  explicit LocalContactForceCost(const rtoc_robot_model& robot)
      : max_num_contacts_(robot.ncontacts), f_ref_(robot.ncontacts, zero()), f_weight_(robot.ncontacts, zero()),
        fi_ref_(robot.ncontacts, zero()), fi_weight_(robot.ncontacts, zero()) {}
  void set_f_ref(const std::vector<Vector3d>& f_ref) { check(f_ref, "f_ref", false), f_ref_ = f_ref; }
  void set_f_weight(const std::vector<Vector3d>& f_weight) { check(f_weight, "f_weight", true), f_weight_ = f_weight; }
  void set_fi_ref(const std::vector<Vector3d>& fi_ref) { check(fi_ref, "fi_ref", false), fi_ref_ = fi_ref; }
  void set_fi_weight(const std::vector<Vector3d>& fi_weight) { check(fi_weight, "fi_weight", true), fi_weight_ = fi_weight; }
  // the device description of the term
  rtoc_contact_force_cost term() const {
    rtoc_contact_force_cost s = rtoc_contact_force_cost();
    for (int i = 0; i < max_num_contacts_; ++i)
      for (int k = 0; k < 3; ++k)
        s.f_ref[i][k] = f_ref_[i][k], s.f_weight[i][k] = f_weight_[i][k], s.fi_ref[i][k] = fi_ref_[i][k], s.fi_weight[i][k] = fi_weight_[i][k];
    return s;
  }

 private:
  static Vector3d zero() { return Vector3d{{0.0, 0.0, 0.0}}; }
  void check(const std::vector<Vector3d>& v, const char* what, const bool weight) const {
    if (v.size() != static_cast<size_t>(max_num_contacts_))
      throw std::invalid_argument(std::string("[LocalContactForceCost] invalid argument: ") + what + ".size() must be " + std::to_string(max_num_contacts_) + "!");
    for (const Vector3d& x : v) {
      if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2]))   // rtoc_set_contact_force_cost would refuse it
        throw std::invalid_argument(std::string("[LocalContactForceCost] invalid argument: elements of '") + what + "' must be finite!");
      if (weight && (x[0] < 0.0 || x[1] < 0.0 || x[2] < 0.0))
        throw std::invalid_argument(std::string("[LocalContactForceCost] invalid argument: elements of '") + what + "' must be non-negative!");
    }
  }
  int max_num_contacts_;
  std::vector<Vector3d> f_ref_, f_weight_, fi_ref_, fi_weight_;
};

}  // namespace robotoc
#endif
