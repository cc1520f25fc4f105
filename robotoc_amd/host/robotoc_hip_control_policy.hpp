// robotoc::ControlPolicy (reference include/robotoc/mpc/control_policy.hpp, src/mpc/control_policy.cpp) over the OCPSolver mirror of
// robotoc_hip_solver.hpp: what an MPC hands to the robot or the simulator -- the feed-forward joint torque tauJ, the joint references
// qJ, dqJ and the gains Kp, Kd at the inquired time, for u = tauJ - Kp (qJ - q) - Kd (dqJ - v).
// set() is ONE rtoc_control_policy call on the solver's context (include/rtoc_robot.h): the solution and the Riccati records stay on
// the device, 3 nu + 2 nu^2 doubles come back.  N = getTimeDiscretization().N(), the grid times run from the t of the solver's last
// discretize(t) over the time steps the device holds.  Where the reference would read u and K of an impact grid point the call does not:
// INTEGRATION.md, "ControlPolicy".
#ifndef ROBOTOC_HIP_CONTROL_POLICY_HPP_
#define ROBOTOC_HIP_CONTROL_POLICY_HPP_

#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rtoc_layout.h"
#include "../../include/rtoc_robot.h"
#include "robotoc_hip_solver.hpp"

namespace robotoc {

struct ControlPolicy {
  ControlPolicy() : t(0) {}                                                                    // control_policy.cpp:8-15
  ControlPolicy(const OCPSolver& ocp_solver, const double t) : ControlPolicy() { set(ocp_solver, t); }   // :18-21
  ~ControlPolicy() = default;
  ControlPolicy(const ControlPolicy&) = default;
  ControlPolicy& operator=(const ControlPolicy&) = default;
  ControlPolicy(ControlPolicy&&) noexcept = default;
  ControlPolicy& operator=(ControlPolicy&&) noexcept = default;

  void set(const OCPSolver& ocp_solver, const double _t) {                                     // :24-60
    rtoc_ctx* ctx = ocp_solver.context();
    if (!ctx) throw std::logic_error("[ControlPolicy] the solver has no device context");
    const TimeDiscretization& time_discretization = ocp_solver.getTimeDiscretization();
    if (time_discretization.size() < 2) throw std::logic_error("[ControlPolicy] the solver has not discretised its horizon yet");
    rtoc_layout L;
    chk(rtoc_get_layout(ctx, &L), "rtoc_get_layout");
    const int dimu = L.dims.nu;
    std::vector<double> rec(rtoc_control_policy_stride(dimu));
    chk(rtoc_control_policy(ctx, ocp_solver.discretizationTime(), &_t, 0, time_discretization.N(), rec.data(), 1, 0), "rtoc_control_policy");
    t = _t;
    tauJ = Vec(dimu), qJ = Vec(dimu), dqJ = Vec(dimu), Kp = Mat(dimu, dimu), Kd = Mat(dimu, dimu);
    for (int i = 0; i < dimu; ++i) {
      tauJ(i) = rec[rtoc_control_policy_tauj_off(dimu) + i];
      qJ(i) = rec[rtoc_control_policy_qj_off(dimu) + i];
      dqJ(i) = rec[rtoc_control_policy_dqj_off(dimu) + i];
    }
    for (int i = 0; i < dimu * dimu; ++i) {   // both column-major with leading dimension dimu
      Kp.data()[i] = rec[rtoc_control_policy_kp_off(dimu) + i];
      Kd.data()[i] = rec[rtoc_control_policy_kd_off(dimu) + i];
    }
  }

  double t;        // inquired time of the control
  Vec tauJ;        // joint torques, Robot::dimu()
  Vec qJ;          // joint positions
  Vec dqJ;         // joint velocities
  Mat Kp;          // joint position gain, dimu x dimu
  Mat Kd;          // joint velocity gain

  void disp(std::ostream& os) const {                                                          // :63-71
    auto row = [&os](const Vec& v) {
      for (int i = 0; i < v.size(); ++i) os << (i ? " " : "") << v(i);
    };
    auto mat = [&os](const Mat& m) {
      for (int i = 0; i < m.rows(); ++i) {
        for (int j = 0; j < m.cols(); ++j) os << (j ? " " : "") << m(i, j);
        os << "\n";
      }
    };
    os << "ControlPolicy: \n";
    os << "  t:    " << t << " \n";
    os << "  tauJ: ", row(tauJ), os << " \n";
    os << "  qJ:   ", row(qJ), os << " \n";
    os << "  dqJ:  ", row(dqJ), os << " \n";
    os << "  Kp: \n", mat(Kp), os << " \n";
    os << "  Kd: \n", mat(Kd), os << " \n";
  }
  friend std::ostream& operator<<(std::ostream& os, const ControlPolicy& control_policy) {    // :74-78
    control_policy.disp(os);
    return os;
  }

 private:
  static void chk(int rc, const char* what) {
    if (rc != RTOC_OK) throw std::runtime_error(std::string("[ControlPolicy] ") + what + ": " + rtoc_error_string(rc));
  }
};

}  // namespace robotoc

#endif  // ROBOTOC_HIP_CONTROL_POLICY_HPP_
