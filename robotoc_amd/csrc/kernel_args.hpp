// kernel_args.hpp -- the argument blocks the host runtime fills for the kernels of a robot shape (kernel_table.hpp): the ones
// kernel_abi_stamp() names, with the limits the host checks for them, and nothing of a runtime kernel (a runtime kernel's block is
// defined beside the kernel and starts with the view of record_view.hpp).  Plain structs and no kernel: the host units see these
// through rt_context.hpp, a kernel header includes this one and defines the kernel beside its own configuration.  The blocks are
// part of what a shape plugin must agree on with the runtime that loads it: no field is added, removed or reordered without the
// plugins being rebuilt, and the host fills them field by field, from zero.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtoc.h"

namespace rtoc {

// ---- riccati_backward.hpp, _rs.hpp, _rv.hpp, _rw.hpp, _rw2.hpp ----
struct BwdArgs {
  const double* kkt;       // [batch][nstages][kkt stride]
  double* kkt_rw;          // same buffer, writable (writeback of F,H,G,lu)
  double* ric;             // [batch][nstages][ric stride]
  const rtoc_grid* grid;   // [nstages] (device)
  uint32_t* status;        // [batch]
  long long* prof;         // optional [nstages][16] cycle stamps of block 0 (tuning aid), or nullptr
  int nstages;
  int batch;  // instances [first, batch) are processed by this launch
  int first;
  int writeback;
  double max_dts0;
  // horizon-scan mode of riccati_backward_kernel (riccati_scan.hpp): value records [P | s] of every
  // grid point, [batch][nstages][scan_ps_stride]; workgroup (b, st) then does the ONE stage st from
  // P_{st+1}, s_{st+1} read there.  nullptr = serial recursion.
  const double* scan_ps;
  int scan_ps_stride;
  int scan_ps_soff;  // offset of s inside a value record
  // Scan on a grid with switching-time optimisation (riccati_scan_sto.hpp): workgroups (b, nstages + st) of the same launch prepare
  // the bundle of grid point st for the serial vector pass -- they read what the policy workgroups read (the scan's value records,
  // the KKT records), none of their output, so they need neither a launch nor an event of their own.  nullptr: no such workgroups.
  double* sto_scr;   // [batch][nstages][scan::StoScratch::STRIDE]
  // Segment of the horizon: the register kernels (riccati_backward_rv.hpp, _rw.hpp) walk the grid points seg_hi .. seg_lo and take
  // P+ / s+ of grid point seg_hi + 1 from the Riccati records unless that is the terminal one -- the quadruped kernel is launched
  // once per horizon (seg_hi = N - 1, seg_lo = 0), the iCub one between its switching-constraint grid points; in the one-stage
  // mode above the tile-split kernel does grid point blockIdx.y + seg_lo.  Zero in every other launch.
  int seg_hi, seg_lo;
  // Structured-Fxx forms on records the runtime cannot vouch for (a bound buffer the caller may have rewritten since the last
  // device check, RTOC_OPT_FXX_STRUCTURE = 0): the kernel verifies the rows it does NOT multiply -- it has them in LDS anyway --
  // and raises RTOC_STAT_FXX_UNSTRUCTURED on the instance instead of returning a silently wrong factorisation.
  int check_fxx;
};
// the host launches a register kernel (riccati_backward_rv.hpp, _rw.hpp, _rw2.hpp) on horizons up to this long
constexpr int RV_MAX_STAGES = 64;   // grid points of a horizon the kernel keeps a kind table for (in the slack of its LDS carve)

// ---- riccati_forward.hpp ----
struct FwdArgs {
  const double* kkt;
  const double* ric;
  double* dir;
  const double* dx0;  // [batch][nx] or nullptr (then dir[...][0].dx is used as given)
  const rtoc_grid* grid;
  int nstages;
  int batch;  // instances [first, batch) are processed by this launch
  int first;
};

struct FillArgs {
  double* kkt;
  int nstages, batch;
  double dt;
  rtoc_record_layout kl;
};

// ---- unconstr_dynamics.hpp ----
struct UdArgs {
  double* kkt;
  double* cdd;
  double* dir;
  int nstages, batch;
  int nlin;   // records per instance with dynamics: nstages - 1, or nstages on a ParNMPC horizon (rtoc_parnmpc_set_horizon)
  double dt;
  rtoc_record_layout kl, cl, dl;
};

// ---- friction_cone.hpp ----
struct ConeArgs {
  double* kkt;
  double* cdd;
  double* con;
  const double* cone;
  const double* dir;
  const rtoc_grid* grid;
  unsigned long long* steps;  // [batch][2] bit patterns (expand) / doubles (update)
  int nstages, batch;
  int max_contacts, contact_dim, row0, rows_per_contact;
  int cone_stride, dgdf_off;
  int impact_cones;  // RTOC_OPT_IMPACT_CONES: 0 = no rows on impact grids (a Constraints object without ImpactFrictionCone)
  double tau;
  rtoc_record_layout kl, cl, nl, dl;
  long long* prof;
};

// ---- condense.hpp, condense_rv.hpp ----
struct CondArgs {
  double* kkt;
  double* cdd;
  const rtoc_grid* grid;
  uint32_t* status;
  int nstages, batch;
  double damping;  // RobotModelInfo::contact_inv_damping (robot_model_info.hpp:95)
  long long* prof;  // optional cycle stamps of work item 0 (tuning aid)
  double* con;               // constraint records or nullptr
  const rtoc_box_row* rows;  // [nrows] joint-limit rows (device)
  const int* entry;          // CSR of the rows per primal entry: [2nv+nu+1] offsets, then row ids
  const int4* pair;          // per primal entry: {row0, row1, sign0 | level0 << 8, sign1 | level1 << 8}, row = -1: none
  int nrows;
  rtoc_record_layout nl;
  rtoc_record_layout kl, cl;
  // friction / wrench cone rows condensed by mjtjinv_kernel (split condensation): 0 = none (or done by their
  // own kernel), RTOC_FRICTION_ROWS, RTOC_WRENCH_ROWS
  int cone_rows;
  const double* cone;
  double* cone_con;  // constraint records (the box rows' `con` may be null when only cones are set)
  int cone_contacts, cone_dim, cone_row0, cone_stride, cone_dgdf_off, cone_impact;
  int keep_qaf;  // RTOC_OPT_CONDENSE_KEEP_QAF: also store Qafqv / Qafu_full in the ContactDynamicsData record
  const double* dt_inst;  // [batch][nstages] per-instance time steps (switching-time optimisation) or nullptr (device_utils.hpp: grid_dt)
  // work items = batch x these grid points (nullptr: all of 0 .. nstages - 2): the impact grid points behind condense_rv_kernel
  const int* stage_list;
  int nlist;
};

struct ExpArgs {
  double* cdd;
  double* dir;
  double* con;               // constraint records or nullptr
  const rtoc_box_row* rows;
  int nrows;
  rtoc_record_layout nl;
  unsigned long long* steps; // [batch][2] max primal / dual step (bit patterns of positive doubles)
  const rtoc_grid* grid;
  int nstages, batch;
  rtoc_record_layout cl, dl;
  double tau;
  const double* dt_inst;  // per-instance time steps or nullptr (grid_dt)
  long long* prof;        // optional cycle stamps (slots 32..39) of the work item in the middle of the launch (tuning aid)
};

// ---- riccati_scan.hpp ----
struct ScanArgs {
  const double* kkt;      // [batch][nstages][kkt stride]
  const rtoc_grid* grid;  // [nstages] (device)
  uint32_t* status;       // [batch]
  const double* src;      // elements before this level [batch][nstages][EltLayout::STRIDE]
  double* dst;            // elements after this level
  double* ps;             // value records [batch][nstages][EltLayout::PS_STRIDE]
  int nstages;
  int batch;  // instances [first, batch) are processed by this launch
  int first;
  int dist;   // distance d of this combination level
};

struct StoScanArgs {
  const double* kkt;
  double* ric;
  const rtoc_grid* grid;
  uint32_t* status;
  const double* ps;   // the scan's value records [batch][nstages][PS_STRIDE]
  double* scr;        // [batch][nstages][StoScratch::STRIDE]
  int nstages, batch, first;
  double max_dts0;
  long long* prof;    // phase stamps of instance 0 (RTOC_ENABLE_PROF builds), else nullptr
  double* kkt_rw;     // RTOC_OPT_WRITEBACK_KKT: the KKT records, writable (the vector pass writes the mutated lu), else nullptr
};
constexpr int SCAN_STO_MAX_STAGES = 512;   // = scan::StoVecCfg::MAX_STAGES (grids beyond take the serial kernel)

struct FwdScanArgs {
  const double* kkt;
  const double* ric;
  double* dir;
  const double* dx0;  // [batch][nx] or nullptr (then dir[...][0].dx is used as given)
  const rtoc_grid* grid;
  const double* src;  // maps before this level [batch][nstages][EltLayout::STRIDE]
  double* dst;
  int nstages;
  int batch;
  int first;
  int dist;
};

// ---- unconstr_riccati.hpp ----
struct UrArgs {
  const double* kkt;
  double* kkt_rw;      // writeback of the mutated Qxx, Qxu, Qaa, la (RTOC_OPT_WRITEBACK_KKT), else unused
  double* ric;
  double* dir;
  const double* dx0;   // [batch][nx] or nullptr
  uint32_t* status;
  int nstages, batch, writeback;
  double dt;
  rtoc_record_layout kl, rl, dl;
};

// ---- parnmpc_backward_correction.hpp ----
struct PbcArgs {
  const double* kkt;   // condensed records of a ParNMPC horizon: [batch][nstages][kkt stride], every record a stage with dynamics
  const double* sol;
  double* dir;
  double* aux;         // [batch][nstages][2nv x 2nv] auxiliary matrices, column-major (read: the previous call's; written: this call's)
  double* snew;        // [batch][nstages][5nv] s_new in the order (lmd, gmm, a, q, v)
  double* xres;        // [batch][nstages][2nv] x_res the last serial pass left at the stage
  double* kinv;        // [batch][nstages][16 nv^2] K^-1[0:2nv, :] (ld 2nv), then K^-1[2nv:5nv, 3nv:5nv] (ld 3nv)
  uint32_t* status;    // [batch]
  int nstages, batch;
  double dt;
  rtoc_record_layout kl, sl, dl;
};

}  // namespace rtoc
