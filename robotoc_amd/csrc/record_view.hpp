// record_view.hpp -- what a kernel may read of a context: the record buffers, the grid, the contact schedule, the model and
// the record layout (include/rtoc_layout.h), as ONE value.  The evalKKT-side kernels (cost, constraints, state equation,
// rigid-body linearisation, switching constraint, task costs) take it as the first member of their argument struct and name
// a field by its RTOC_SOL_* / RTOC_KKT_* / RTOC_CDD_* / RTOC_CON_* / RTOC_DIR_* enum; what else such a struct holds belongs
// to the launch alone.  The runtime fills a view at every launch (view() in rtoc_capi.hip) and never keeps one: buffers are
// rebound (rtoc_bind) and swapped for the trial iterate of the line search between launches.
//
// Record conventions the enums do not tell:
//   * contact path: Qaa / la / lf / ha ... live in RTOC_BUF_CDD until the condensation; on impact grids the A slot of the
//     solution holds dv and CDD.la holds ldv
//   * unconstrained path (rtoc_unconstr_condense): la lives in KKT.lu and Qaa in KKT.Quu; lu lives in CDD.la and
//     diag(Quu) in CDD.Qaa
// Not for the headers kernel_set.hpp reaches: the per-shape kernels bake their layout into immediates (StaticLayout).
#pragma once
#include "../../include/rtoc_layout.h"
#include "../../include/rtoc.h"
#include <stddef.h>

namespace rtoc {
namespace rbd {
struct DevModel;
}

struct RecView {
  const double* sol;
  double* kkt;
  double* cdd;
  double* con;
  const double* dir;
  double* cone;
  double* se3;
  double* dx0;
  unsigned long long* steps;  // RTOC_BUF_STEP: [batch][2] bit patterns
  const rtoc_grid* grid;
  const unsigned* active;     // [nstages] contact schedule
  const double* positions;    // [nstages][ncontacts][3] or nullptr
  const double* rotations;    // [nstages][ncontacts][9] or nullptr (surface contacts: desired rotation)
  const double* dt_inst;      // per-instance time steps or nullptr (grid_dt)
  const rbd::DevModel* model;
  int nstages, batch;
  int all_stages;             // 1: the records are the stages of a ParNMPC horizon (rtoc_parnmpc_set_horizon), none of them terminal
  rtoc_layout L;

  // records per instance that carry dynamics and constraint rows: all but the terminal one, or every stage of a ParNMPC horizon
  RTOC_HD int nlin() const { return nstages - 1 + all_stages; }
  RTOC_HD int nv() const { return L.dims.nv; }
  RTOC_HD int nu() const { return L.dims.nu; }
  RTOC_HD int floating() const { return L.dims.np == 6; }
  // field offsets within a record, by the enums of rtoc_layout.h
  RTOC_HD int sol_off(int f) const { return L.sol.off[f]; }
  RTOC_HD int kkt_off(int f) const { return L.kkt.off[f]; }
  RTOC_HD int cdd_off(int f) const { return L.cdd.off[f]; }
  RTOC_HD int dir_off(int f) const { return L.dir.off[f]; }
  // record rec = instance * nstages + grid point
  RTOC_HD const double* sol_at(size_t rec) const { return sol + rec * L.sol.stride; }
  RTOC_HD double* kkt_at(size_t rec) const { return kkt + rec * L.kkt.stride; }
  RTOC_HD double* cdd_at(size_t rec) const { return cdd + rec * L.cdd.stride; }
  RTOC_HD double* con_at(size_t rec) const { return con + rec * L.con.stride; }
  RTOC_HD const double* dir_at(size_t rec) const { return dir + rec * L.dir.stride; }
};

// The numbers of the robot model a kernel's control flow and LDS carving depend on, as kernel arguments (the tangent walk
// of rigid_body.hpp reads them on its critical path: not from memory).  nv and nu are the view's: rtoc_set_robot_model
// accepts a model only if they agree with the context's dimensions.
struct ModelDims {
  int nq, njoints, ncontacts, nlevels, nbranch, dpp;
  int gs;        // lanes per grid point of rbd_values_kernel: the next power of two >= njoints
  int floating;  // the root joint is a free-flyer
  double gx, gy, gz;  // gravity
};

}  // namespace rtoc
