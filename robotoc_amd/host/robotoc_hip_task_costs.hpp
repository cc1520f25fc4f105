// robotoc_hip_task_costs.hpp -- TaskSpace3DCost, CoMCost, TaskSpace6DCost, PeriodicSwingFootRef, PeriodicCoMRef and
// TaskSpace6DRefBase with the reference's constructors and setters (src/cost/task_space_3d_cost.cpp, com_cost.cpp,
// task_space_6d_cost.cpp, periodic_swing_foot_ref.cpp, periodic_com_ref.cpp, include/robotoc/cost/task_space_6d_ref_base.hpp).
// They describe the terms; rtoc_contact_eval_kkt / rtoc_unconstr_eval_kkt evaluate them on the device (include/rtoc_robot.h:
// rtoc_task_cost).  Hand them to the ConfigurationCostSource overload of robotoc_hip_device_source.hpp or to UnconstrOCP::task_costs
// (robotoc_hip_unconstr_solver.hpp).  Header-only, C++11.
//
// A TaskSpace6DRefBase is the user's own class (the reference ships no concrete one): the shells call its updateRef / isActive
// once per grid point when they discretise and hand the device a table (rtoc_set_task_ref_table).
//
// A frame is a contact frame of the model table (its index k: contact_parent[k], contact_p[k]) or a parent joint with an offset
// in that joint's frame: the world position of a frame depends on its origin only.  isActive / updateRef restate the reference's
// loops on the host (set-up and checks); the device runs the same loops.
#ifndef ROBOTOC_HIP_TASK_COSTS_HPP_
#define ROBOTOC_HIP_TASK_COSTS_HPP_

#include <array>
#include <memory>
#include <stdexcept>
#include <string>

#include <vector>

#include "../../include/rtoc_robot.h"
#include "robotoc_hip.hpp"

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
};
typedef TaskSpace3DRefBase CoMRefBase;

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
  virtual bool usesTable() const { return false; }
  virtual std::vector<rtoc_task_ref_entry> refTable(const std::vector<GridInfo>&) const { return std::vector<rtoc_task_ref_entry>(); }

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
      out[i].active = ref6_->isActive(grid[i]) ? 1 : 0, out[i].pad = 0;
      if (out[i].active) ref6_->updateRef(grid[i], ref);
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

}  // namespace robotoc
#endif
