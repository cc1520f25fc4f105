// robotoc::UnconstrOCPSolver with a TaskSpace6DCost (robotoc_amd/host/robotoc_hip_unconstr_solver.hpp, robotoc_hip_task_costs.hpp)
// on the GPU: the reference's examples/iiwa14/task_space_ocp.cpp -- iiwa14, ConfigurationSpaceCost + TaskSpace6DCost on the
// end-effector frame.
// usage: unconstr_task_space_ocp_test <problem.bin> <out.bin>
//   problem.bin (written by tests/test_task_space_6d_closed_loop.py): rtoc_robot_model, rtoc_configuration_cost, double T, int N,
//   double q0[nv], v0[nv], int frame_parent, double frame_R[9], frame_p[3], const reference R[9], p[3], weight_position[3],
//   weight_rotation[3] (stage and terminal alike), then the circular reference of the example: rotm[9], pos0[3], radius, and the
//   number of iterations of its leg.
//   out.bin: leg 1 (constant reference, solve() under default SolverOptions): iterations, converged, KKT error, initial KKT
//   error, then q, v of every grid point; leg 2 (the circle through a reference table, a fixed number of iterations): q, v of
//   every grid point.  The Python side issues the same iterations through ctypes and compares bit for bit.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_unconstr_solver.hpp"

// examples/iiwa14/task_space_ocp.cpp:27-57
class TaskSpace6DRef final : public robotoc::TaskSpace6DRefBase {
 public:
  TaskSpace6DRef(const robotoc::Matrix3d& rotm, const robotoc::Vector3d& pos0, const double radius) : radius_(radius), rotm_(rotm), pos0_(pos0) {}
  void updateRef(const robotoc::GridInfo& grid_info, robotoc::SE3& ref) const override {
    robotoc::Vector3d pos(pos0_);
    pos[1] += radius_ * std::sin(M_PI * grid_info.t);
    pos[2] += radius_ * std::cos(M_PI * grid_info.t);
    ref = robotoc::SE3(rotm_, pos);
  }
  bool isActive(const robotoc::GridInfo&) const override { return true; }

 private:
  double radius_;
  robotoc::Matrix3d rotm_;
  robotoc::Vector3d pos0_;
};

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

static void trajectory(robotoc::UnconstrOCPSolver& solver, const int N, const int nv, std::vector<double>& out) {
  const std::vector<robotoc::Vec> qs = solver.getSolution("q"), vs = solver.getSolution("v");
  for (int i = 0; i <= N; ++i) {
    for (int k = 0; k < nv; ++k) out.push_back(qs[i](k));
    for (int k = 0; k < nv; ++k) out.push_back(vs[i](k));
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  robotoc::UnconstrOCP ocp;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double q0[RTOC_MAX_JOINTS], v0[RTOC_MAX_JOINTS], radius = 0.0;
  int parent = 0, circle_iters = 0;
  robotoc::SE3 frame, ref;
  robotoc::Vector3d wp, wr, pos0;
  robotoc::Matrix3d rotm;
  bool ok = rd(f, &ocp.robot, 1) && rd(f, &ocp.cost, 1) && rd(f, &ocp.T, 1) && rd(f, &ocp.N, 1);
  const int nv = ok ? ocp.robot.nv : 0;
  ok = ok && rd(f, q0, nv) && rd(f, v0, nv) && rd(f, &parent, 1) && rd(f, frame.R.data(), 9) && rd(f, frame.p.data(), 3) &&
       rd(f, ref.R.data(), 9) && rd(f, ref.p.data(), 3) && rd(f, wp.data(), 3) && rd(f, wr.data(), 3) && rd(f, rotm.data(), 9) &&
       rd(f, pos0.data(), 3) && rd(f, &radius, 1) && rd(f, &circle_iters, 1);
  std::fclose(f);
  if (!ok) return 4;
  try {
    robotoc::Vec q(nv), v(nv);
    for (int i = 0; i < nv; ++i) q(i) = q0[i], v(i) = v0[i];
    std::vector<double> out;
    bool converged = false;
    // ---- leg 1: a constant reference, solve() under default SolverOptions ----
    auto task_cost = std::make_shared<robotoc::TaskSpace6DCost>(ocp.robot, parent, frame, ref);
    task_cost->set_weight(wp, wr);
    task_cost->set_weight_terminal(wp, wr);
    ocp.task_costs.push_back(task_cost);
    {
      robotoc::UnconstrOCPSolver solver(ocp, robotoc::SolverOptions());
      solver.discretize(0.0);
      solver.setSolution("q", q);
      solver.setSolution("v", v);
      const double e0 = solver.KKTError(0.0, q, v);
      solver.solve(0.0, q, v);
      const robotoc::SolverStatistics& st = solver.getSolverStatistics();
      std::printf("constant reference: KKT error %.3e -> %.3e in %d iterations, converged %d\n", e0, solver.KKTError(), st.iter, (int)st.convergence);
      out.push_back(st.iter), out.push_back(st.convergence ? 1.0 : 0.0), out.push_back(solver.KKTError()), out.push_back(e0);
      trajectory(solver, ocp.N, nv, out);
      converged = st.convergence;
    }
    // ---- leg 2: the example's circle through a reference table, a fixed number of iterations (no convergence claim) ----
    {
      task_cost->set_ref(std::make_shared<TaskSpace6DRef>(rotm, pos0, radius));
      robotoc::SolverOptions opt;
      opt.max_iter = circle_iters;
      opt.kkt_tol = 0.0;   // never met: exactly max_iter iterations
      robotoc::UnconstrOCPSolver solver(ocp, opt);
      solver.discretize(0.0);
      solver.setSolution("q", q);
      solver.setSolution("v", v);
      solver.solve(0.0, q, v);
      std::printf("circular reference: KKT error %.3e after %d iterations\n", solver.KKTError(), solver.getSolverStatistics().iter);
      if (solver.getSolverStatistics().iter != circle_iters) return 8;
      trajectory(solver, ocp.N, nv, out);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return converged ? 0 : 6;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 7;
  }
}
