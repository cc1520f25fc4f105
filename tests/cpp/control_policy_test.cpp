// robotoc::ControlPolicy (robotoc_amd/host/robotoc_hip_control_policy.hpp) over the OCPSolver mirror on the GPU:
//   control_policy_test <stage dump>
// One OCPSolver::updateSolution on the recorded stage data of the ANYmal trot (tests/test_cpp_control_policy.py writes the dump: lifts,
// touch-downs, 47 grid points), then ControlPolicy(solver, t) against a loop over getSolution(), getLQRPolicy() and
// getTimeDiscretization() written out here from the semantics of include/rtoc_robot.h (control_policy.cpp:24-60 with the two
// departures at impact grid points): two interior times and the edge branches -- before t0, exactly t0 and exactly on a later grid
// time (alpha = 1), the interval that ends at an impact (hold), far beyond the horizon (fallback to record N - 1, N = 40 of the 47
// grid points).  The grid times start at the t given to discretize(t).  Bounds: a copy, alpha = 1 included, bit for bit; a blended entry within
// 4 eps (|alpha| |a| + |1 - alpha| |b|), two rounded products and one rounded sum with or without a fused multiply-add.
// Copy and move construction keep the values.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <utility>

#include "../../robotoc_amd/host/robotoc_hip_control_policy.hpp"

using namespace robotoc;

static int fail(const char* what) {
  std::fprintf(stderr, "FAILED: %s\n", what);
  return 1;
}

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

struct Expected {
  std::vector<double> v, scale;   // [tauJ | qJ | dqJ | Kp | Kd] (the matrices column-major); scale < 0: a copy
};

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: control_policy_test <stage dump>");
  if (rtoc_device_count() < 1) {
    std::fprintf(stderr, "no HIP device\n");
    return 2;
  }
  try {
    auto source = std::make_shared<StageDumpSource>(argv[1]);
    SolverOCP ocp(source);
    OCPSolver solver(ocp, SolverOptions());
    const RobotDims robot = source->robot();
    const int nv = robot.dimv, nu = robot.dimu, nq = nv + (robot.dim_passive > 0 ? 1 : 0);
    Vec q(nq), v(nv);
    const double t_start = 0.25;   // the replayed grid carries no times of its own: they start where discretize(t) says
    solver.discretize(t_start);
    solver.initConstraints();
    solver.updateSolution(t_start, q, v);
    if (solver.status() != 0) return fail("numerical status bits set");
    const Solution& s = solver.getSolution();
    const std::vector<LQRPolicy>& lqr = solver.getLQRPolicy();
    const TimeDiscretization& td = solver.getTimeDiscretization();
    const int n = td.size(), N = td.N();
    // a discretisation from a list of grid points counts the time stages back: one grid point per lift, two per impact
    int events = 0;
    for (int i = 0; i < n; ++i) events += td[i].type == GridType::Impact ? 2 : (td[i].type == GridType::Lift ? 1 : 0);
    if (events < 3 || N != n - 1 - events) return fail("N() of a discretisation from a list of grid points");
    if (solver.discretizationTime() != t_start) return fail("discretizationTime()");
    std::vector<double> tg(n);
    tg[0] = t_start;
    for (int i = 0; i + 1 < n; ++i) tg[i + 1] = tg[i] + td[i].dt;
    int k = -1;
    for (int i = 0; i < n && k < 0; ++i)
      if (td[i].type == GridType::Impact) k = i;
    if (k < 3 || k > N - 2) return fail("the dump has no impact grid point to hold in front of");

    const double eps = std::ldexp(1.0, -52);
    auto record = [&](const int i, std::vector<double>& out) {
      out.clear();
      for (int j = 0; j < nu; ++j) out.push_back(s[i].u(j));
      for (int j = 0; j < nu; ++j) out.push_back(s[i].q(nq - nu + j));
      for (int j = 0; j < nu; ++j) out.push_back(s[i].v(nv - nu + j));
      for (int c = 0; c < nu; ++c)
        for (int r = 0; r < nu; ++r) out.push_back(lqr[i].K(r, nv - nu + c));
      for (int c = 0; c < nu; ++c)
        for (int r = 0; r < nu; ++r) out.push_back(lqr[i].K(r, 2 * nv - nu + c));
    };
    auto expected = [&](const double t) -> Expected {
      Expected e;
      int a = -1, b = -1;
      double alpha = 1.0;
      if (t < tg[0]) {
        a = 0;
      } else {
        for (int i = 1; i < N - 1 && a < 0; ++i)
          if (t < tg[i] && td[i - 1].type != GridType::Impact) {
            a = i - 1;
            if (td[i].type != GridType::Impact) b = i, alpha = (tg[i] - t) / (tg[i] - tg[i - 1]);
          }
        if (a < 0) a = td[N - 1].type == GridType::Impact ? N - 2 : N - 1;
      }
      std::vector<double> ra, rb;
      record(a, ra);
      if (b < 0 || alpha == 1.0) {   // alpha = 1: 1 a + 0 b is a, bit for bit
        e.v = ra, e.scale.assign(ra.size(), -1.0);
        return e;
      }
      record(b, rb);
      for (size_t j = 0; j < ra.size(); ++j) {
        e.v.push_back(alpha * ra[j] + (1.0 - alpha) * rb[j]);
        e.scale.push_back(std::fabs(alpha) * std::fabs(ra[j]) + std::fabs(1.0 - alpha) * std::fabs(rb[j]));
      }
      return e;
    };
    auto flat = [&](const ControlPolicy& p) -> std::vector<double> {
      std::vector<double> out;
      for (int j = 0; j < nu; ++j) out.push_back(p.tauJ(j));
      for (int j = 0; j < nu; ++j) out.push_back(p.qJ(j));
      for (int j = 0; j < nu; ++j) out.push_back(p.dqJ(j));
      for (int c = 0; c < nu; ++c)
        for (int r = 0; r < nu; ++r) out.push_back(p.Kp(r, c));
      for (int c = 0; c < nu; ++c)
        for (int r = 0; r < nu; ++r) out.push_back(p.Kd(r, c));
      return out;
    };

    struct Query {
      const char* name;
      double t;
      bool copy;
    };
    const Query queries[] = {
        {"interior of the second interval", 0.3 * tg[1] + 0.7 * tg[2], false},
        {"interior of an interval behind the impact", 0.6 * tg[k + 1] + 0.4 * tg[k + 2], false},
        {"before t0", tg[0] - 1.0, true},
        {"exactly t0 (alpha = 1)", tg[0], true},
        {"exactly on a grid time behind the impact (alpha = 1)", tg[k + 2], true},
        {"in front of the impact (hold)", 0.5 * (tg[k - 1] + tg[k]), true},
        {"far beyond the horizon (fallback)", tg[n - 1] + 100.0, true},
    };
    double worst = 0.0;
    for (const Query& qy : queries) {
      const ControlPolicy policy(solver, qy.t);
      if (policy.t != qy.t || policy.tauJ.size() != nu || policy.Kp.rows() != nu || policy.Kd.cols() != nu) return fail("sizes");
      const Expected e = expected(qy.t);
      const std::vector<double> got = flat(policy);
      if ((e.scale[0] < 0.0) != qy.copy) return fail("the query does not take the branch it was written for");
      double norm = 0.0;
      for (size_t j = 0; j < got.size(); ++j) {
        norm += std::fabs(got[j]);
        if (e.scale[j] < 0.0) {
          if (!same_bits(got[j], e.v[j])) {
            std::fprintf(stderr, "%s: entry %zu: %.17g != %.17g\n", qy.name, j, got[j], e.v[j]);
            return fail("a copy is not bit-identical");
          }
        } else {
          const double err = std::fabs(got[j] - e.v[j]), bound = 4.0 * eps * e.scale[j];
          if (err > 0.0) worst = std::fmax(worst, err / bound);
          if (!(err <= bound)) {
            std::fprintf(stderr, "%s: entry %zu: %.17g vs %.17g, bound %.3e\n", qy.name, j, got[j], e.v[j], bound);
            return fail("a blended entry misses its bound");
          }
        }
      }
      if (!(norm > 0.0)) return fail("an all-zero policy");
    }
    // copy and move construction keep the values
    ControlPolicy first(solver, queries[0].t);
    const std::vector<double> want = flat(first);
    ControlPolicy copy(first);
    ControlPolicy moved(std::move(first));
    ControlPolicy assigned;
    assigned = copy;
    const ControlPolicy* all[] = {&copy, &moved, &assigned};
    for (const ControlPolicy* p : all) {
      const std::vector<double> got = flat(*p);
      if (p->t != queries[0].t || got.size() != want.size()) return fail("copy / move lost the sizes");
      for (size_t j = 0; j < got.size(); ++j)
        if (!same_bits(got[j], want[j])) return fail("copy / move changed a value");
    }
    std::ostringstream os;
    os << copy;
    if (os.str().find("ControlPolicy:") != 0 || os.str().find("Kd:") == std::string::npos) return fail("disp");
    std::printf("control_policy_test passed: %d grid points, impact at %d; blends: worst error / bound %.2e (4 eps (|alpha| |a| + |1 - alpha| |b|))\n",
                n, k, worst);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 7;
  }
}
