// examples/anymal/trot.cpp through the C++ shell: robotoc::OCPSolver over ConfigurationCostSource with the example's
// TaskSpace3DCost / PeriodicSwingFootRef foot costs and CoMCost / PeriodicCoMRef (robotoc_hip_task_costs.hpp) beside the
// ConfigurationSpaceCost, joint limits and friction cones -- OCPSolver::solve, nothing of the iteration on the host.
//   usage: ocp_solver_trot_task_cost_test <problem.bin> <out.bin>
//   problem.bin (tests/test_task_space_cost_trot.py writes it): rtoc_robot_model, rtoc_configuration_cost, int n, rtoc_grid[n],
//   double t[n], unsigned mask[n], double positions[n][ncontacts][3], double q0[nq], v0[nv], double f_init[n][max_dimf],
//   double q_max, v_max, u_max, mu, barrier, kkt_tol, max_iter, int nterms, rtoc_task_cost terms[nterms] (the components'
//   parameters: rebuilt here with the C++ classes)
//   out.bin: iter, convergence, KKT error per iteration, q[n][nq]
#include <cstdio>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_device_source.hpp"

using namespace robotoc;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  rtoc_robot_model model;
  rtoc_configuration_cost cost;
  int n = 0;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  if (!rd(f, &model, 1) || !rd(f, &cost, 1) || !rd(f, &n, 1) || n < 2) return 4;
  const int nv = model.nv, nq = model.nq, nc = model.ncontacts, nu = nv - 6, dimf = 3 * nc;
  std::vector<rtoc_grid> g(n);
  std::vector<unsigned> mask(n);
  std::vector<double> tg(n), pos((size_t)n * nc * 3), q0(nq), v0(nv), finit((size_t)n * dimf);
  double lim[7];
  int nterms = 0;
  bool ok = rd(f, g.data(), n) && rd(f, tg.data(), n) && rd(f, mask.data(), n) && rd(f, pos.data(), pos.size()) && rd(f, q0.data(), nq) &&
            rd(f, v0.data(), nv) && rd(f, finit.data(), finit.size()) && rd(f, lim, 7) && rd(f, &nterms, 1) && nterms >= 0 && nterms <= RTOC_MAX_TASK_COSTS;
  std::vector<rtoc_task_cost> terms(nterms > 0 ? nterms : 1);
  ok = ok && rd(f, terms.data(), nterms);
  std::fclose(f);
  if (!ok) return 4;
  try {
    std::vector<GridInfo> grid(n);
    for (int i = 0; i < n; ++i) {
      grid[i].type = static_cast<GridType>(g[i].type);
      grid[i].dt = g[i].dt;
      grid[i].t = tg[i];
      grid[i].switching_constraint = g[i].switching_constraint != 0;
      grid[i].dimf = g[i].dimf, grid[i].dims = g[i].dims;
      grid[i].num_grids_in_phase = g[i].num_grids_in_phase;
      grid[i].stage = g[i].time_stage < 0 ? 0 : g[i].time_stage;
    }
    RobotDims dims;
    dims.dimv = nv, dims.dimu = nu, dims.dim_passive = 6, dims.max_dimf = dimf;
    Solution s0(n, SplitSolution(dims));
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < nq; ++k) s0[i].q(k) = q0[k];
      for (int k = 0; k < dimf; ++k) s0[i].f_full(k) = finit[(size_t)i * dimf + k];
    }
    std::vector<std::shared_ptr<TaskCostComponent>> costs;
    for (const rtoc_task_cost& s : terms) {
      if (static_cast<int>(costs.size()) == nterms) break;
      const Vector3d x0{{s.x0[0], s.x0[1], s.x0[2]}}, rate{{s.rate[0], s.rate[1], s.rate[2]}};
      std::shared_ptr<TaskCostComponent> c;
      if (s.kind == RTOC_TASK_COM) {
        c = std::make_shared<CoMCost>(model, std::make_shared<PeriodicCoMRef>(x0, rate, s.t0, s.period_active, s.period_inactive, s.first_half != 0));
      } else {
        auto ref = std::make_shared<PeriodicSwingFootRef>(x0, rate, s.step_height, s.t0, s.period_active, s.period_inactive, s.first_half != 0);
        c = std::make_shared<TaskSpace3DCost>(model, s.frame_parent, Vector3d{{s.frame_p[0], s.frame_p[1], s.frame_p[2]}}, ref);
      }
      c->set_weight(Vector3d{{s.weight[0], s.weight[1], s.weight[2]}});
      c->set_weight_terminal(Vector3d{{s.weight_terminal[0], s.weight_terminal[1], s.weight_terminal[2]}});
      c->set_weight_impact(Vector3d{{s.weight_impact[0], s.weight_impact[1], s.weight_impact[2]}});
      costs.push_back(c);
    }
    auto source = std::make_shared<ConfigurationCostSource>(model, cost, costs, grid, mask, pos, s0);
    const std::vector<double> qmax(nu, lim[0]), qmin(nu, -lim[0]), vmax(nu, lim[1]), umax(nu, lim[2]);
    bool threw = false;   // the reference's argument check
    try {
      CoMCost(model).set_weight(Vector3d{{1.0, -1.0, 0.0}});
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    if (!threw) return 8;
    source->setJointLimits(qmin, qmax, vmax, umax);
    source->setFrictionCone(std::vector<double>(nc, lim[3]), false);
    source->setBarrierParam(lim[4], 0.995);
    SolverOCP ocp(source);
    SolverOptions opt;
    opt.kkt_tol = lim[5];
    opt.max_iter = static_cast<int>(lim[6]);
    OCPSolver solver(ocp, opt);
    Vec q(nq), v(nv);
    for (int k = 0; k < nq; ++k) q(k) = q0[k];
    for (int k = 0; k < nv; ++k) v(k) = v0[k];
    solver.solve(0.0, q, v, true);
    const SolverStatistics& st = solver.getSolverStatistics();
    std::printf("OCPSolver::solve, trot with foot and CoM costs on the device: KKT error %.3e -> %.3e in %d iterations, converged %d\n",
                std::sqrt(st.performance_index.front()), solver.KKTError(), st.iter, (int)st.convergence);
    if (solver.status() != 0) return 5;
    const Solution& s = solver.getSolution();
    std::vector<double> out;
    out.push_back(st.iter), out.push_back(st.convergence ? 1.0 : 0.0), out.push_back(static_cast<double>(st.performance_index.size()));
    for (double e : st.performance_index) out.push_back(std::sqrt(e));
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < nq; ++k) out.push_back(s[i].q(k));
    f = std::fopen(argv[2], "wb");
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return st.convergence ? 0 : 6;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 7;
  }
}
