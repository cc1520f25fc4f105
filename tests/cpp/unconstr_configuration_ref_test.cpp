// robotoc::UnconstrOCPSolver::setConfigurationRef (robotoc_amd/host/robotoc_hip_unconstr_solver.hpp) on the GPU: iiwa14 tracking
// q0 + t v, the reference's test helper ConfigurationSpaceRef (test/test_helper/cost_factory.hpp) restated as a subclass.
// usage: unconstr_configuration_ref_test <problem.bin>   (the file tests/test_cpp_solver.py writes for unconstr_ocp_solver_test)
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_unconstr_solver.hpp"

using namespace robotoc;

class ConfigurationSpaceRef : public ConfigurationSpaceRefBase {
 public:
  ConfigurationSpaceRef(const double* q0_ref, const double v_scale) : q0_(q0_ref), v_scale_(v_scale) {}
  void updateRef(const rtoc_robot_model& robot, const GridInfo& g, Vec& q_ref) const override {
    ++asked;
    for (int i = 0; i < robot.nq; ++i) q_ref(i) = q0_[i] + g.t * v_scale_ * (i - 3);
  }
  bool isActive(const GridInfo&) const override { return true; }
  mutable int asked = 0;

 private:
  const double* q0_;
  double v_scale_;
};

#define REQUIRE(cond)                                             \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static std::vector<double> trajectory(UnconstrOCPSolver& s) {
  std::vector<double> out;
  for (const Vec& q : s.getSolution("q"))
    for (int i = 0; i < q.size(); ++i) out.push_back(q(i));
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  UnconstrOCP ocp;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double q0[RTOC_MAX_JOINTS], v0[RTOC_MAX_JOINTS];
  bool ok = std::fread(&ocp.robot, sizeof(ocp.robot), 1, f) == 1 && std::fread(&ocp.cost, sizeof(ocp.cost), 1, f) == 1 &&
            std::fread(&ocp.T, sizeof(double), 1, f) == 1 && std::fread(&ocp.N, sizeof(int), 1, f) == 1;
  const int nv = ok ? ocp.robot.nv : 0;
  ok = ok && std::fread(q0, sizeof(double), nv, f) == (size_t)nv && std::fread(v0, sizeof(double), nv, f) == (size_t)nv;
  std::fclose(f);
  if (!ok) return 4;
  try {
    SolverOptions opt;
    opt.max_iter = 30;
    opt.kkt_tol = 1.0e-9;
    Vec q(nv), v(nv);
    for (int i = 0; i < nv; ++i) q(i) = q0[i], v(i) = v0[i];
    // the constant reference
    UnconstrOCPSolver fixed(ocp, opt);
    fixed.setSolution("q", q), fixed.setSolution("v", v);
    fixed.solve(0.0, q, v, true);
    REQUIRE(fixed.getSolverStatistics().convergence);
    const std::vector<double> q_fixed = trajectory(fixed);
    // the moving one, set on a solver that exists already: the table is filled at once
    auto ref = std::make_shared<ConfigurationSpaceRef>(ocp.cost.q_ref, 0.2);
    UnconstrOCPSolver moving(ocp, opt);
    moving.setConfigurationRef(ref);
    REQUIRE(ref->asked == ocp.N + 1);
    moving.setSolution("q", q), moving.setSolution("v", v);
    moving.solve(0.0, q, v, true);
    const SolverStatistics& st = moving.getSolverStatistics();
    std::printf("moving reference: KKT error %.3e in %d iterations, converged %d\n", moving.KKTError(), st.iter, (int)st.convergence);
    REQUIRE(st.convergence && st.iter <= 20);
    const std::vector<double> q_moving = trajectory(moving);
    double diff = 0.0;
    for (size_t i = 0; i < q_moving.size(); ++i) diff = std::fmax(diff, std::fabs(q_moving[i] - q_fixed[i]));
    std::printf("largest difference to the constant reference's trajectory %.3e\n", diff);
    REQUIRE(diff > 1.0e-2);
    // given in the OCP: the constructor's discretize fills the table; a copy (rtoc_clone) carries it
    UnconstrOCP ocp2 = ocp;
    ocp2.setConfigurationRef(ref);
    UnconstrOCPSolver built(ocp2, opt);
    built.setSolution("q", q), built.setSolution("v", v);
    UnconstrOCPSolver copy(built);
    built.solve(0.0, q, v, true);
    copy.solve(0.0, q, v, true);
    REQUIRE(trajectory(built) == q_moving && trajectory(copy) == q_moving);
    // nullptr: the constant reference again, bit for bit
    moving.setConfigurationRef(nullptr);
    moving.setSolution("q", q), moving.setSolution("v", v);
    Vec zero(nv);
    moving.setSolution("a", zero), moving.setSolution("u", zero);
    moving.solve(0.0, q, v, true);
    REQUIRE(moving.getSolverStatistics().convergence);
    double back = 0.0;
    const std::vector<double> q_back = trajectory(moving);
    for (size_t i = 0; i < q_back.size(); ++i) back = std::fmax(back, std::fabs(q_back[i] - q_fixed[i]));
    std::printf("after setConfigurationRef(nullptr): largest difference to the constant reference's trajectory %.3e\n", back);
    // (the multipliers start from the other problem's optimum, so the iterates differ: both end within the KKT tolerance of the same
    // optimum, four orders below what separates the two problems)
    REQUIRE(back < 1.0e-6);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 5;
  }
  std::printf("ok\n");
  return 0;
}
