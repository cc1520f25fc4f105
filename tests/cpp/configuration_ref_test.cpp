// configurationRefTable of robotoc_amd/host/robotoc_hip_task_costs.hpp (the table a ConfigurationSpaceRefBase is served to the
// device through) on the one-cycle ANYmal trot (t0 = 0.11, swing 0.2, double support 0.1; N = 40, T = 0.8) with a stub
// reference: prints the active flag and the row of every grid point, which tests/test_cpp_configuration_ref.py compares with the
// Python fill's.  Also the fill's order of questions and its refusal of a reference that is not finite.  Host code only: no
// device call.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_device_source.hpp"
#include "../../robotoc_amd/host/robotoc_hip_unconstr_solver.hpp"

using namespace robotoc;

#define REQUIRE(cond)                                             \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// the same arithmetic, in the same order, as the stub of tests/test_configuration_ref_host.py
class StubRef : public ConfigurationSpaceRefBase {
 public:
  void updateRef(const rtoc_robot_model& robot, const GridInfo& g, Vec& q_ref) const override {
    updated.push_back(g.stage);
    for (int k = 0; k < robot.nq; ++k) q_ref(k) = g.t * (k + 1) * 0.1 + g.phase * 0.01 - 0.001 * g.stage_in_phase;
    if (bad_stage == g.stage) q_ref(2) = std::nan("");
  }
  bool isActive(const GridInfo& g) const override {
    asked.push_back(g.stage);
    return g.phase != 1;
  }
  int bad_stage = -1;
  mutable std::vector<int> asked, updated;
};

static std::vector<double> flat(const double feet[4][3]) {
  std::vector<double> p;
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) p.push_back(feet[i][k]);
  return p;
}

int main() {
  double feet[4][3] = {{0.35, 0.2, 0.0}, {-0.35, 0.2, 0.0}, {0.35, -0.2, 0.0}, {-0.35, -0.2, 0.0}};
  ContactSequence cs(std::vector<int>(4, 3));
  cs.init(0xFu, flat(feet));
  cs.push_back(0x9u, flat(feet), 0.11);
  cs.push_back(0xFu, flat(feet), 0.31);
  cs.push_back(0x6u, flat(feet), 0.41);
  cs.push_back(0xFu, flat(feet), 0.61);
  const TimeDiscretization td = discretize(cs, 0.8, 40, 0.0, false);
  std::vector<GridInfo> grid(td.size());
  for (int i = 0; i < td.size(); ++i) grid[i] = td[i];
  rtoc_robot_model robot = rtoc_robot_model();
  robot.njoints = 13, robot.nq = 19, robot.nv = 18, robot.ncontacts = 4;
  rtoc_configuration_cost cost = rtoc_configuration_cost();
  for (int k = 0; k < robot.nv; ++k) cost.q_weight[k] = 1.0 + k, cost.q_weight_terminal[k] = 2.0;   // no impact weight
  StubRef ref;
  const ConfigurationRefTable tab = configurationRefTable(ref, robot, cost, grid);
  REQUIRE(tab.active.size() == grid.size() && tab.q_ref.size() == grid.size() * 19);
  std::printf("grid %d\n", td.size());
  size_t expect_asked = 0, expect_updated = 0;
  for (size_t i = 0; i < grid.size(); ++i) {
    const bool impact = grid[i].type == GridType::Impact;
    expect_asked += impact ? 0 : 1;
    expect_updated += (!impact && grid[i].phase != 1) ? 1 : 0;
    REQUIRE(tab.active[i] == ((!impact && grid[i].phase != 1) ? 1 : 0));
    std::printf("row %d %d", static_cast<int>(i), tab.active[i]);
    for (int k = 0; k < 19; ++k) std::printf(" %.17g", tab.q_ref[i * 19 + k]);
    std::printf("\n");
  }
  // isActive only where the q weight of the kind is not all zero, updateRef only where active
  REQUIRE(ref.asked.size() == expect_asked && ref.updated.size() == expect_updated);
  for (int s : ref.asked) REQUIRE(grid[s].type != GridType::Impact);
  for (int s : ref.updated) REQUIRE(grid[s].phase != 1);
  // all q weights zero: the object is not asked at all
  rtoc_configuration_cost none = rtoc_configuration_cost();
  StubRef quiet;
  const ConfigurationRefTable empty = configurationRefTable(quiet, robot, none, grid);
  REQUIRE(quiet.asked.empty() && quiet.updated.empty());
  for (int a : empty.active) REQUIRE(a == 0);
  // a reference that is not finite is refused, the grid point named
  StubRef bad;
  bad.bad_stage = 3;
  bool refused = false;
  try {
    (void)configurationRefTable(bad, robot, cost, grid);
  } catch (const std::invalid_argument& e) {
    refused = true;
    std::printf("refused: %s\n", e.what());
  }
  REQUIRE(refused);
  // the shells take the object and let go of it again
  UnconstrOCP ocp;
  ocp.setConfigurationRef(std::make_shared<StubRef>());
  REQUIRE(static_cast<bool>(ocp.configuration_ref));
  ocp.setConfigurationRef(nullptr);
  REQUIRE(!ocp.configuration_ref);
  std::printf("ok\n");
  return 0;
}
