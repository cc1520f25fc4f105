// contact_force_cost.hpp -- LocalContactForceCost in the contact path's evalKKT (reference src/cost/local_contact_force_cost.cpp).
//
// Per contact i that is active at the grid point (intermediate / lift grids: the contact status, :98-144; impact grids: the
// impact status with fi_weight / fi_ref, :184-230; the terminal grid: nothing, :147-166), with d = f_i[0:3] - f_ref[i] and
// o_i the offset of contact i in the compacted stack of the active contacts (3 rows per point contact, 6 per surface contact,
// of which only the first 3 carry a cost):
//   lf[o_i : o_i+3] += s w_i d,   diag(Qff)[o_i : o_i+3] += s w_i,   value += s/2 sum w_i d^2,   s = dt (impact grids: 1)
// and on intermediate / lift grids the STO sensitivities of intermediate_stage.cpp:104-108, taken before constraints and
// dynamics add to lf: hf[o_i : o_i+3] = w_i d, h += 1/2 sum w_i d^2.
// Launched behind contact_cost_kernel, whose last act is the zero fill of LF / QFF / HF, and ahead of the box rows, the cones
// and the dynamics, which add to lf.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "../../include/rtoc_robot.h"

namespace rtoc {

struct ForceCostArgs {
  RecView rv;
  const rtoc_contact_force_cost* cost;   // [1], or [batch] with per_instance
  double* cost_out;                      // [batch][nstages] cost values, added to
  int per_instance;
  int ncontacts;                         // of the model: contacts at and beyond it are ignored
  unsigned surface;                      // bit k: contact k of the model is a surface contact (6 rows of the stack)
};

// A lane per contact, FCOST_GP grid points per wave: a contact's three components are three independent chains of one load, one
// multiply-add and one store each, and its offset in the stack is two population counts -- a wave per grid point would idle 56
// lanes.  Grid points beyond the batch are masked, not repeated: the term ADDS to what is there.
constexpr int FCOST_LW = RTOC_MAX_CONTACTS, FCOST_GP = 64 / FCOST_LW;
static_assert(FCOST_GP * FCOST_LW == 64 && (FCOST_LW & (FCOST_LW - 1)) == 0, "a power-of-two number of lanes per grid point");

static __global__ __launch_bounds__(64) void contact_force_cost_kernel(ForceCostArgs a) {
  const int lane = threadIdx.x % FCOST_LW, grp = threadIdx.x / FCOST_LW;   // `lane`: the contact
  const long long nitems = (long long)a.rv.batch * a.rv.nstages;
  const long long item = (long long)blockIdx.x * FCOST_GP + grp;
  const bool valid = item < nitems;
  const long long it = valid ? item : nitems - 1;
  const int b = (int)(it / a.rv.nstages), st = (int)(it % a.rv.nstages);
  const bool impact = a.rv.grid[st].type == RTOC_GRID_IMPACT, terminal = st == a.rv.nstages - 1;
  const int nf = a.rv.L.dims.nf_max;
  const unsigned all = a.ncontacts >= 32 ? ~0u : ((1u << a.ncontacts) - 1u);
  // the contact status of an intermediate / lift grid, the impact status of an impact grid (rtoc_set_contact_schedule)
  const unsigned active = (valid && !terminal) ? (a.rv.active[st] & all) : 0u;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double scale = impact ? 1.0 : grid_dt(a.rv.grid, a.rv.dt_inst, b, a.rv.nstages, st);
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  // rows of the active contacts ahead of this one: 3 each, 3 more for a surface contact
  const unsigned below = active & ((1u << lane) - 1u);
  const int o = 3 * (__popc(below) + __popc(below & a.surface));
  double hval = 0.0;   // this contact's share of 1/2 sum w d^2
  if (((active >> lane) & 1u) && o + 3 <= nf) {
    const rtoc_contact_force_cost* const fc = a.cost + (a.per_instance ? b : 0);
    const double* const ref = impact ? fc->fi_ref[lane] : fc->f_ref[lane];
    const double* const w = impact ? fc->fi_weight[lane] : fc->f_weight[lane];
    const double* const f = a.rv.sol_at(rec) + a.rv.sol_off(RTOC_SOL_F) + o;
    double* const lf = cr + a.rv.cdd_off(RTOC_CDD_LF) + o;
    double* const hf = cr + a.rv.cdd_off(RTOC_CDD_HF) + o;
    double* const Qff = cr + a.rv.cdd_off(RTOC_CDD_QFF) + (size_t)o * (nf + 1);   // the diagonal, leading dimension nf_max
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double d = f[k] - ref[k], wd = w[k] * d;
      lf[k] += scale * wd;
      Qff[(size_t)k * (nf + 1)] += scale * w[k];
      if (!impact) hf[k] = wd;
      hval += 0.5 * wd * d;
    }
  }
#pragma unroll
  for (int off = FCOST_LW / 2; off > 0; off >>= 1) hval += __shfl_xor(hval, off, 64);   // within the grid point's lanes
  if (lane == 0 && active != 0u) {
    if (!impact) kr[a.rv.kkt_off(RTOC_KKT_SCAL) + RTOC_KKT_SCAL_H] += hval;
    if (a.cost_out) a.cost_out[rec] += scale * hval;
  }
}

}  // namespace rtoc
