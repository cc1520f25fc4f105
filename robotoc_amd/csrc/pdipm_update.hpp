// pdipm_update.hpp -- the primal-dual interior point rows after the step sizes are known: updateSlack / updateDual of the box
// rows and of the cone rows, and the reset of the step buffer.  Runtime kernels (not per shape): rt_condense.hip launches
// them and is the one unit that includes this header.
#pragma once
#include "friction_cone.hpp"  // cone_nact, ConeArgs
#include "record_view.hpp"

namespace rtoc {

struct UpdArgs {
  RecView rv;  // steps: [batch][2] doubles
  const rtoc_box_row* rows;
  int nrows;
};

// updateSlack / updateDual (constraints_impl.hxx:167-182) with the per-instance step sizes
static __global__ __launch_bounds__(64) void pdipm_update_kernel(UpdArgs a) {
  const int item = blockIdx.x;
  const int nst1 = a.rv.nlin();
  const int b = item / nst1, st = item % nst1;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  if (g.type == RTOC_GRID_IMPACT) return;
  double* nr = a.rv.con_at((size_t)b * a.rv.nstages + st);
  const int* no = a.rv.L.con.off;
  const double* steps = reinterpret_cast<const double*>(a.rv.steps);
  const double ps = steps[2 * b], ds = steps[2 * b + 1];
  for (int r = threadIdx.x; r < a.nrows; r += 64) {
    if (g.time_stage >= a.rows[r].level) {
      nr[no[RTOC_CON_SLACK] + r] += ps * nr[no[RTOC_CON_DSLACK] + r];
      nr[no[RTOC_CON_DUAL] + r] += ds * nr[no[RTOC_CON_DDUAL] + r];
    }
  }
}

static __global__ void fill_steps_kernel(double* steps, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) steps[i] = 1.0;
}

// updateSlack / updateDual of the cone rows (constraints_impl.hxx:167-182)
static __global__ __launch_bounds__(64) void cone_update_kernel(ConeArgs a) {
  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int nst1 = a.nstages - 1;
  const int b = item / nst1, st = item % nst1;
  if (b >= a.batch) return;
  const int nact = cone_nact(a.grid[st], a.contact_dim, a.impact_cones);
  if (lane >= a.rows_per_contact * nact) return;  // <= 5*4 friction rows, <= 17*2 wrench rows
  double* nr = a.con + ((size_t)b * a.nstages + st) * a.nl.stride;
  const double* steps = reinterpret_cast<const double*>(a.steps);
  const int r = a.row0 + lane;
  nr[a.nl.off[RTOC_CON_SLACK] + r] += steps[2 * b] * nr[a.nl.off[RTOC_CON_DSLACK] + r];
  nr[a.nl.off[RTOC_CON_DUAL] + r] += steps[2 * b + 1] * nr[a.nl.off[RTOC_CON_DDUAL] + r];
}

}  // namespace rtoc
