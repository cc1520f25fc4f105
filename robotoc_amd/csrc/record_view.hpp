// record_view.hpp -- what a kernel may read of a context: the record buffers, the grid, the contact schedule, the model and
// the record layout (include/rtoc_layout.h), as ONE value.  Every runtime kernel that reads a record takes it as the first
// member `rv` of its argument struct (takes_view below holds the launchers to it) and names a field by its RTOC_SOL_* /
// RTOC_KKT_* / RTOC_CDD_* / RTOC_CON_* / RTOC_DIR_* enum; what else such a struct holds belongs to the launch alone.  The
// runtime fills a view at every launch (view() in rtoc_capi.hip, through view_args() of rt_context.hpp) and never keeps
// one: buffers are rebound (rtoc_bind) and swapped for the trial iterate of the line search between launches.
// Filled by hand, on purpose: the blocks of a robot shape (kernel_args.hpp: their layout is part of what a plugin agrees
// on, and their kernels bake the record layout into immediates), and Ls*Args / FilterArgs / *TimesArgs, which read no record.
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

#include <type_traits>

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
  // the desired contact placements (rtoc_set_contact_schedule: shared by the batch; rtoc_set_contact_placements /
  // rtoc_hold_contact_placements: every instance its own), one row per (grid point, contact): read through placement() alone
  const double* positions;    // [nstages][ncontacts][3] or [batch][nstages][ncontacts][3] or nullptr (zeros)
  const double* rotations;    // the same with [9] (row-major; surface contacts: desired rotation) or nullptr (identity)
  const double* dt_inst;      // per-instance time steps or nullptr (grid_dt)
  const rbd::DevModel* model;
  int nstages, batch;
  int all_stages;             // 1: the records are the stages of a ParNMPC horizon (rtoc_parnmpc_set_horizon), none of them terminal
  int placement_stride;       // grid points between the placement tables of two instances: nstages, or 0 for a table the batch shares
  rtoc_layout L;

  // row of `positions` (x 3 doubles) and of `rotations` (x 9) that holds the placement of contact c at grid point st of instance b.
  // A shared table is the per-instance one with a stride of zero: one multiply-add, no branch
  RTOC_HD size_t placement(int b, int st, int ncontacts, int c) const {
    return ((size_t)b * (size_t)placement_stride + (size_t)st) * (size_t)ncontacts + (size_t)c;
  }

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

// The convention, held by the compiler where a launcher names its block: the view comes first, and the block is copied into
// the kernarg segment as it stands.
template <class A>
constexpr bool takes_view = offsetof(A, rv) == 0 && std::is_same_v<decltype(A::rv), RecView> && std::is_trivially_copyable_v<A>;

// The friction / wrench cone rows of a context (rtoc_set_friction_cones, rtoc_set_wrench_cones) as a kernel walks them: a member
// of the runtime blocks that do (kkt_error.hpp, line_search.hpp), and what the fillers of the shape blocks copy their cone
// numbers from.  Filled by view_cones() (rt_condense.hip) alone.  contacts == 0: no cone rows.
struct ConeRows {
  int contacts;  // most contacts that carry cones
  int dim;       // force components of a contact (3 or 6): a grid point has g.dimf / dim active ones; 3 where none is set
  int rows;      // PDIPM rows per contact: RTOC_FRICTION_ROWS, RTOC_WRENCH_ROWS
  int row0;      // the first cone row of a constraint record: nc_max - rows * contacts
  int stride;    // doubles of a RTOC_BUF_CONE record
  int dgdf_off;  // of dg_df within it (friction cones)
  int impact;    // RTOC_OPT_IMPACT_CONES: 0 = no rows on impact grids
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

// rtoc_set_configuration_ref_table: the q_ref of a ConfigurationSpaceRefBase and its isActive per GRID POINT, for the kernels that
// read the cost table (contact_eval_kkt.hpp, rigid_body.hpp).  q == nullptr: no table, the constant q_ref of the cost table is the
// reference of every grid point (and `active` is not read).
struct QRefTable {
  const double* q;     // [nstages][nq] or [batch][nstages][nq]; a row has the layout of rtoc_configuration_cost::q_ref
  const int* active;   // same leading shape: isActive(grid_info)
  int per_instance, nq;
  RTOC_HD size_t row(int b, int nstages, int st) const { return (size_t)(per_instance ? b : 0) * nstages + st; }
};

}  // namespace rtoc
