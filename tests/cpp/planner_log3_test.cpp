// planner_log3_test.cpp -- SolutionInterpolator::interpolateConfiguration on placements given on stdin, for
// tests/test_lie_branch_points_host.py: the header's log3 is private, and the interpolation q1 (+) alpha (q2 (-) q1) is its only
// caller.  Each input line holds q1 [7], q2 [7] and alpha; each output line the interpolated [x y z qx qy qz qw] with 17
// digits.  Host code only.
#include <cstdio>

#include "../../robotoc_amd/host/robotoc_hip_planner.hpp"

int main() {
  double q1[7], q2[7], alpha, q[7];
  int n = 0;
  for (;;) {
    int got = 0;
    for (int k = 0; k < 7; ++k) got += std::scanf("%lf", &q1[k]) == 1;
    for (int k = 0; k < 7; ++k) got += std::scanf("%lf", &q2[k]) == 1;
    got += std::scanf("%lf", &alpha) == 1;
    if (got != 15) break;
    robotoc::SolutionInterpolator::interpolateConfiguration(q1, q2, alpha, 7, true, q);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
    ++n;
  }
  std::printf("ok %d\n", n);
  return 0;
}
