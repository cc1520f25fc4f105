// kkt_error.hpp -- squared KKT residual of every OCP instance, evaluated at the evalKKT boundary.
//
// Replaces the kkt_error accumulation of IntermediateStage / ImpactStage / TerminalStage::evalKKT
// (reference src/ocp/intermediate_stage.cpp:132: data.KKTError() + kkt_residual.KKTError(), summed over
// the horizon by DirectMultipleShooting::evalKKT, direct_multiple_shooting.cpp:129-159) and the final
// sqrt of OCPSolver::KKTError() (src/solver/ocp_solver.cpp:429-431; the STO term is not part of it here):
//   SplitKKTResidual::KKTError()      Fx^2 + P^2 + lx^2 + lu^2 + la^2 + ldv^2 + lf^2     (split_kkt_residual.hxx:90-104)
//   ContactDynamicsData::KKTError()   IDC^2 + lu_passive^2                               (contact_dynamics_data.hpp:204-206)
//   ConstraintComponentData::KKTError() residual^2 + cmpl^2 of the active rows           (constraint_component_data.hpp:122-124)
// on the PRE-condensation records (the reference evaluates it before condenseSlackAndDual /
// condenseContactDynamics).  One wave per instance, stages in order, fixed lane-strided summation
// order and a butterfly at the end: deterministic.  Pure streaming read (HBM-bound, ~11 KB/stage).
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"

namespace rtoc {

struct KktErrArgs {
  RecView rv;          // cdd == nullptr: no contact-dynamics terms; con == nullptr: neither box rows nor cone rows
  const rtoc_box_row* rows;
  double* partial;     // [batch][nstages] squared residual per grid point
  int nrows;
  ConeRows cone;
};

// One wave per (grid point, instance): the squared residual of that grid point into partial[b][st]; the second kernel
// adds the grid points of an instance in grid order and takes the root -- the same fixed summation order for every
// launch geometry (deterministic), and a single OCP no longer walks its horizon serially (0.2 ms -> a few us).
static __global__ __launch_bounds__(64) void kkt_error_kernel(KktErrArgs a) {
  const int lane = threadIdx.x;
  const int st = blockIdx.x, b = blockIdx.y;
  if (b >= a.rv.batch || st >= a.rv.nstages) return;
  const rtoc_record_layout &kl = a.rv.L.kkt, &cl = a.rv.L.cdd, &nl = a.rv.L.con;
  const int nv = a.rv.nv(), nx = a.rv.L.nx;
  double acc = 0.0;
  auto sq = [&](const double* p, int n) {
    for (int i = lane; i < n; i += 64) {
      const double v = p[i];
      acc += v * v;
    }
  };
  {
    const rtoc_grid g = a.rv.grid[st];
    const size_t rec = (size_t)b * a.rv.nstages + st;
    const double* kr = a.rv.kkt_at(rec);
    const bool terminal = g.type == RTOC_GRID_TERMINAL, impact = g.type == RTOC_GRID_IMPACT;
    sq(kr + kl.off[RTOC_KKT_LX], nx);
    if (!terminal) {
      sq(kr + kl.off[RTOC_KKT_FX], nx);
      if (!impact) {
        sq(kr + kl.off[RTOC_KKT_LU], a.rv.nu());
        if (g.dims > 0) sq(kr + kl.off[RTOC_KKT_PRES], g.dims);
      }
      if (a.rv.cdd) {
        const double* cr = a.rv.cdd_at(rec);
        sq(cr + cl.off[RTOC_CDD_LA], nv);  // la (contact grids) / ldv (impact grids)
        sq(cr + cl.off[RTOC_CDD_LF], g.dimf);
        sq(cr + cl.off[RTOC_CDD_IDC], nv + g.dimf);
        if (!impact) sq(cr + cl.off[RTOC_CDD_LUP], a.rv.L.dims.np);
      }
      if (a.rv.con) {
        const double* nr = a.rv.con_at(rec);
        if (!impact)
          for (int r = lane; r < a.nrows; r += 64)
            if (g.time_stage >= a.rows[r].level) {
              const double x = nr[nl.off[RTOC_CON_RESIDUAL] + r], y = nr[nl.off[RTOC_CON_CMPL] + r];
              acc += x * x + y * y;
            }
        if (a.cone.contacts > 0 && (!impact || a.cone.impact)) {
          const int row0 = a.cone.row0, n = a.cone.rows * (g.dimf / a.cone.dim);
          for (int r = lane; r < n; r += 64) {
            const double x = nr[nl.off[RTOC_CON_RESIDUAL] + row0 + r], y = nr[nl.off[RTOC_CON_CMPL] + row0 + r];
            acc += x * x + y * y;
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) a.partial[(size_t)b * a.rv.nstages + st] = acc;
}

static __global__ void kkt_error_reduce_kernel(const double* partial, double* out, int nstages, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double acc = 0.0;
  for (int st = 0; st < nstages; ++st) acc += partial[(size_t)b * nstages + st];
  out[b] = sqrt(acc);
}

}  // namespace rtoc
