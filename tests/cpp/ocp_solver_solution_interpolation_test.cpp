// robotoc::OCPSolver (robotoc_amd/host/robotoc_hip_solver.hpp) with SolverOptions::solution_interpolation_on_device off and on, on the
// ANYmal jump with switching-time optimisation at N = 40: three iterations without a refinement, then one iteration whose
// mesh-refinement branch is forced (kkt_tol_mesh huge, max_dt_mesh = 0) -- store, discretize, interpolate on the host
// (robotoc_hip_planner.hpp) or on the device (rtoc_solution_store / rtoc_solution_interpolate).
//   usage: ocp_solver_solution_interpolation_test <problem.bin> <out.bin>
//   problem.bin (tests/test_solution_interpolation_closed_loop.py writes it): as for ocp_solver_jump_sto_test, without max_dt_mesh
// Then, with the option on, the receding-horizon warm start: solve(t = 1.5 T / N, init_solver = true) with max_iter = 0 --
// discretize, rtoc_solution_interpolate from what the previous solve stored at its end, initConstraints, store.
//   out.bin: grid points n, record stride, the n records of RTOC_BUF_SOL behind the refinement: option off, option on; the n grid
//   times the host path interpolated at (TimeDiscretization::t); then the warm start: t of the second solve, and for the stored
//   and for the new grid: grid points m, m types, m masks, m time steps (the device's), m records
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
  int N = 0;
  double hdr[3];
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  if (!rd(f, &model, 1) || !rd(f, &cost, 1) || !rd(f, &N, 1) || !rd(f, hdr, 3)) return 4;
  const int nv = model.nv, nq = model.nq, nc = model.ncontacts, nu = nv - 6, dimf = 3 * nc;
  std::vector<double> feet(nc * 3), landed(nc * 3), q0(nq), v0(nv), fstand(dimf), min_dwell(3);
  double lim[4];
  const bool ok = rd(f, feet.data(), feet.size()) && rd(f, landed.data(), landed.size()) && rd(f, q0.data(), nq) && rd(f, v0.data(), nv) &&
                  rd(f, fstand.data(), dimf) && rd(f, min_dwell.data(), 3) && rd(f, lim, 4);
  std::fclose(f);
  if (!ok) return 4;
  try {
    const double T = hdr[0], t_lift = hdr[1], t_land = hdr[2];
    const unsigned all = (1u << nc) - 1u;
    std::vector<double> out, t_host;
    for (int on = 0; on < 2; ++on) {
      ContactSequence cs(std::vector<int>(nc, 3));
      cs.init(all, feet);
      cs.push_back(0u, feet, t_lift, true);
      cs.push_back(all, landed, t_land, true);
      const TimeDiscretization td0 = discretize(cs, T, N, 0.0, true);
      const int n0 = td0.size();
      RobotDims dims;
      dims.dimv = nv, dims.dimu = nu, dims.dim_passive = 6, dims.max_dimf = dimf;
      Solution s0(n0, SplitSolution(dims));
      for (int i = 0; i < n0; ++i) {
        for (int k = 0; k < nq; ++k) s0[i].q(k) = q0[k];
        for (int k = 0; k < nv; ++k) s0[i].v(k) = v0[k];
        const bool stand = td0[i].dimf == dimf && td0[i].type != GridType::Impact && i + 1 < n0;
        for (int k = 0; k < dimf; ++k) s0[i].f_full(k) = stand ? fstand[k] : 0.0;
      }
      auto sto = std::make_shared<STOConstraints>(min_dwell, 1.0e-3, 0.995);
      auto source = std::make_shared<ConfigurationCostSource>(model, cost, cs, T, N, s0, sto);
      source->setJointLimits(std::vector<double>(nu, -lim[0]), std::vector<double>(nu, lim[0]), std::vector<double>(nu, lim[1]), std::vector<double>(nu, lim[2]));
      source->setFrictionCone(std::vector<double>(nc, lim[3]), false);
      source->setBarrierParam(1.0e-3, 0.995);
      SolverOCP ocp(source);
      SolverOptions opt;
      opt.solution_interpolation_on_device = on != 0;
      opt.max_iter = 3;
      opt.kkt_tol = 1.0e-7;
      opt.kkt_tol_mesh = 0.0;   // no refinement yet
      opt.max_dt_mesh = T / N;
      OCPSolver solver(ocp, opt);
      Vec q(nq), v(nv);
      for (int k = 0; k < nq; ++k) q(k) = q0[k];
      for (int k = 0; k < nv; ++k) v(k) = v0[k];
      solver.solve(0.0, q, v, true);
      opt.max_iter = 1, opt.kkt_tol_mesh = 1.0e30, opt.max_dt_mesh = 0.0;   // one more iteration, and its refinement
      solver.setSolverOptions(opt);
      solver.solve(0.0, q, v, false);
      const SolverStatistics& st = solver.getSolverStatistics();
      if (st.mesh_refinement_iter.size() != 1 || solver.status() != 0) return 5;
      int stored = -1;
      if (rtoc_solution_stored(solver.context(), &stored) != RTOC_OK || (stored > 0) != (on != 0)) return 6;   // off: the kernels never ran
      rtoc_layout L;
      rtoc_get_layout(solver.context(), &L);
      const int n = solver.getTimeDiscretization().size();
      if (on == 0) out.push_back(n), out.push_back(L.sol.stride);
      else if (n != static_cast<int>(out[0])) return 8;
      std::vector<double> rec(static_cast<size_t>(n) * L.sol.stride);
      if (rtoc_download(solver.context(), RTOC_BUF_SOL, 0, rec.data(), rec.size()) != RTOC_OK) return 9;
      out.insert(out.end(), rec.begin(), rec.end());
      if (on == 0) {
        for (int i = 0; i < n; ++i) t_host.push_back(solver.getTimeDiscretization()[i].t);
      } else {
        out.insert(out.end(), t_host.begin(), t_host.end());
        // a grid with the time steps the device holds, and its records
        auto dump = [&]() {
          const TimeDiscretization& td = solver.getTimeDiscretization();
          const int m = td.size();
          std::vector<double> dt(m), r(static_cast<size_t>(m) * L.sol.stride);
          if (rtoc_sto_get_time_steps(solver.context(), dt.data(), 1) != RTOC_OK) return false;
          if (rtoc_download(solver.context(), RTOC_BUF_SOL, 0, r.data(), r.size()) != RTOC_OK) return false;
          out.push_back(m);
          for (int i = 0; i < m; ++i) out.push_back(static_cast<int>(td[i].type));
          for (int i = 0; i < m; ++i) out.push_back((*source->contactMasks())[i]);
          out.insert(out.end(), dt.begin(), dt.end());
          out.insert(out.end(), r.begin(), r.end());
          return true;
        };
        const double t1 = 1.5 * T / N;
        out.push_back(t1);
        if (!dump()) return 10;   // what the solve above stored at its end
        opt.max_iter = 0;
        solver.setSolverOptions(opt);
        solver.solve(t1, q, v, true);
        if (!dump()) return 10;
      }
      std::printf("OCPSolver, solution interpolation on the %s: %d grid points behind the refinement\n", on ? "device" : "host", n);
    }
    f = std::fopen(argv[2], "wb");
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 7;
  }
}
