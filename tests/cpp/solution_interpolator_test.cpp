// solution_interpolator_test.cpp -- robotoc::SolutionInterpolator (robotoc_hip_planner.hpp) on a case given on stdin, for
// tests/test_solution_interpolator_restatement.py.  Input: the six rtoc_dims, the number of contacts and their stack rows, the
// stored grid (n0, then type t dt mask per point, then n0 packed records) and the grid to interpolate onto (n1, then type t mask
// per point); output: the n1 interpolated records, one per line with 17 digits, then "ok n1".  Host code only.
#include <cstdio>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_planner.hpp"

static bool rd(double* x) { return std::scanf("%lf", x) == 1; }
static bool ri(int* x) { return std::scanf("%d", x) == 1; }

int main() {
  rtoc_dims d;
  int nc = 0;
  if (!(ri(&d.nv) && ri(&d.nu) && ri(&d.np) && ri(&d.nf_max) && ri(&d.ns_max) && ri(&d.nc_max) && ri(&nc))) return 2;
  std::vector<int> rows(nc);
  for (int c = 0; c < nc; ++c)
    if (!ri(&rows[c])) return 2;
  rtoc_layout L;
  rtoc_compute_layout(&d, &L);
  auto read_grid = [&](bool with_dt, std::vector<robotoc::GridInfo>& g, std::vector<unsigned>& masks) {
    int n = 0;
    if (!ri(&n) || n < 2) return false;
    g.assign(n, robotoc::GridInfo()), masks.assign(n, 0u);
    for (int i = 0; i < n; ++i) {
      int type = 0, mask = 0;
      if (!ri(&type) || !rd(&g[i].t) || (with_dt && !rd(&g[i].dt)) || !ri(&mask)) return false;
      g[i].type = static_cast<robotoc::GridType>(type), masks[i] = static_cast<unsigned>(mask), g[i].stage = i;
    }
    return true;
  };
  std::vector<robotoc::GridInfo> g0, g1;
  std::vector<unsigned> m0, m1;
  if (!read_grid(true, g0, m0)) return 2;
  std::vector<double> sol0(g0.size() * L.sol.stride);
  for (double& x : sol0)
    if (!rd(&x)) return 2;
  if (!read_grid(false, g1, m1)) return 2;
  robotoc::SolutionInterpolator interpolator;
  interpolator.store(robotoc::TimeDiscretization(g0), m0, sol0);
  std::vector<double> sol1(g1.size() * L.sol.stride, 0.0);
  interpolator.interpolate(L, nc, d.np == 6, robotoc::TimeDiscretization(g1), m1, sol1, rows);
  for (size_t i = 0; i < g1.size(); ++i) {
    for (int j = 0; j < L.sol.stride; ++j) std::printf("%.17g ", sol1[i * L.sol.stride + j]);
    std::printf("\n");
  }
  std::printf("ok %d\n", static_cast<int>(g1.size()));
  return 0;
}
