// robotoc::UnconstrParNMPCSolver (robotoc_amd/host/robotoc_hip_unconstr_parnmpc_solver.hpp) on the GPU: the scenario of the
// reference's test/solver/unconstr_parnmpc_solver_test.cpp -- iiwa14, ConfigurationSpaceCost, N = 20, T = 1.
// usage: unconstr_parnmpc_solver_test <problem.bin> <out.bin>
//   problem.bin: rtoc_robot_model, rtoc_configuration_cost, double T, int N, double q0[nv], double v0[nv], int nrows,
//   rtoc_box_row rows[nrows], double bounds[nrows] (written by tests/test_cpp_parnmpc_solver.py); out.bin: iterations, converged,
//   KKT error, then q, v of every stage -- the Python side compares them with the same iterations issued through ctypes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_unconstr_parnmpc_solver.hpp"

template <class E, class F>
static bool throws(F f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
    return false;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  robotoc::UnconstrOCP ocp;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double q0[RTOC_MAX_JOINTS], v0[RTOC_MAX_JOINTS];
  int nrows = 0;
  bool ok = std::fread(&ocp.robot, sizeof(ocp.robot), 1, f) == 1 && std::fread(&ocp.cost, sizeof(ocp.cost), 1, f) == 1 &&
            std::fread(&ocp.T, sizeof(double), 1, f) == 1 && std::fread(&ocp.N, sizeof(int), 1, f) == 1;
  const int nv = ok ? ocp.robot.nv : 0;
  ok = ok && std::fread(q0, sizeof(double), nv, f) == (size_t)nv && std::fread(v0, sizeof(double), nv, f) == (size_t)nv;
  ok = ok && std::fread(&nrows, sizeof(int), 1, f) == 1 && nrows >= 0;
  if (ok && nrows > 0) {
    ocp.constraint_rows.resize(nrows), ocp.constraint_bounds.resize(nrows);
    ok = std::fread(ocp.constraint_rows.data(), sizeof(rtoc_box_row), nrows, f) == (size_t)nrows &&
         std::fread(ocp.constraint_bounds.data(), sizeof(double), nrows, f) == (size_t)nrows;
  }
  std::fclose(f);
  if (!ok) return 4;
  try {
    robotoc::Vec q(nv), v(nv);
    for (int i = 0; i < nv; ++i) q(i) = q0[i], v(i) = v0[i];
    // the argument checks of the reference (unconstr_parnmpc_solver.cpp:29-34, :125-130, :215) and the stated limitation
    {
      robotoc::UnconstrOCP bad = ocp;
      bad.T = 0.0;
      if (!throws<std::out_of_range>([&] { robotoc::UnconstrParNMPCSolver s(bad); })) return 10;
      bad = ocp, bad.N = 0;
      if (!throws<std::out_of_range>([&] { robotoc::UnconstrParNMPCSolver s(bad); })) return 11;
      robotoc::SolverOptions ls;
      ls.enable_line_search = true;
      if (!throws<std::invalid_argument>([&] { robotoc::UnconstrParNMPCSolver s(ocp, ls); })) return 12;
      robotoc::UnconstrParNMPCSolver s(ocp);
      robotoc::Vec shortq(nv - 1);
      if (!throws<std::out_of_range>([&] { s.solve(0.0, shortq, v); })) return 13;
      if (!throws<std::out_of_range>([&] { s.KKTError(0.0, q, shortq); })) return 14;
      if (!throws<std::invalid_argument>([&] { s.setSolution("f", q); })) return 15;
      if (!throws<std::invalid_argument>([&] { s.setSolverOptions(ls); })) return 16;
    }
    robotoc::SolverOptions opt;   // the reference's test runs the defaults: max_iter 100, kkt_tol 1e-7
    robotoc::UnconstrParNMPCSolver solver(ocp, opt);
    solver.discretize(0.0);
    solver.setSolution("q", q);
    solver.setSolution("v", v);
    solver.initConstraints();
    solver.initBackwardCorrection();
    const double e0 = solver.KKTError(0.0, q, v);
    // value semantics: two iterations, then a copy; original and copy continue identically on their own device contexts
    for (int it = 0; it < 2; ++it) solver.updateSolution(0.0, q, v);
    robotoc::UnconstrParNMPCSolver copy(solver);
    solver.solve(0.0, q, v, false);
    copy.solve(0.0, q, v, false);
    const robotoc::SolverStatistics& st = solver.getSolverStatistics();
    if (copy.getSolverStatistics().iter != st.iter || copy.KKTError() != solver.KKTError()) {
      std::fprintf(stderr, "copy diverged from the original: %d vs %d iterations, %.3e vs %.3e\n", copy.getSolverStatistics().iter, st.iter,
                   copy.KKTError(), solver.KKTError());
      return 8;
    }
    std::vector<robotoc::Vec> qs = solver.getSolution("q"), vs = solver.getSolution("v"), qc = copy.getSolution("q");
    if ((int)qs.size() != ocp.N || (int)solver.getSolution("a").size() != ocp.N || (int)solver.getSolution("u").size() != ocp.N) return 5;
    if ((int)solver.getTimeDiscretization().size() != ocp.N + 1) return 5;
    for (int i = 0; i < ocp.N; ++i)
      for (int k = 0; k < nv; ++k)
        if (qs[i](k) != qc[i](k)) return 9;
    std::printf("KKT error %.3e -> %.3e in 2 + %d iterations, converged %d\n", e0, solver.KKTError(), st.iter, (int)st.convergence);
    std::vector<double> out;
    out.push_back(2 + st.iter), out.push_back(st.convergence ? 1.0 : 0.0), out.push_back(solver.KKTError()), out.push_back(e0);
    for (int i = 0; i < ocp.N; ++i) {
      for (int k = 0; k < nv; ++k) out.push_back(qs[i](k));
      for (int k = 0; k < nv; ++k) out.push_back(vs[i](k));
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return st.convergence ? 0 : 6;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 7;
  }
}
