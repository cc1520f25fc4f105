// rt_context.hpp -- the context of the host runtime (rtoc_ctx) and what its translation units share.  Private: included by
// rtoc_capi.hip and the rt_*.hip units alone.  The state of a context is grouped by subsystem; every group that rtoc_clone
// copies says so itself, in a clone_from directly under its members.  Functions one unit calls in another are declared at
// the end, in namespace rtoc; everything else in a unit is static.
// No header included here defines a kernel: the context needs the descriptor table of a shape with its argument blocks
// (kernel_table.hpp) and the host half of the rigid-body model (rigid_body_model.hpp).  A kernel header is included by the one
// unit that launches from it: the device compiler emits every static kernel a unit sees, launched from it or not
// (tests/test_kernel_units.py reads the objects for it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtoc.h"
#include "../../include/rtoc_robot.h"
#include "device_buffer.hpp"
#include "grid_table.hpp"
#include "kernel_table.hpp"
#include "record_view.hpp"
#include "rigid_body_model.hpp"

#define HIP_TRY(expr)                                 \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) {                           \
      rtoc::ctx_set_err(e_, __FILE_NAME__, __LINE__); \
      return RTOC_ERR_HIP;                            \
    }                                                 \
  } while (0)

#define CHECK_READY(c)                       \
  if (!(c)) return RTOC_ERR_BAD_ARG;         \
  if ((c)->parnmpc) return RTOC_ERR_BAD_ARG; /* a ParNMPC horizon (no terminal record): CHECK_STAGES, rt_parnmpc.hip */ \
  if ((c)->nstages < 2) return RTOC_ERR_NOT_READY; \
  HIP_TRY(hipSetDevice((c)->device));
// ... of the few entry points that serve a grid of rtoc_set_grid and the N stages of rtoc_parnmpc_set_horizon alike
#define CHECK_STAGES(c)                      \
  if (!(c)) return RTOC_ERR_BAD_ARG;         \
  if ((c)->nstages < ((c)->parnmpc ? 1 : 2)) return RTOC_ERR_NOT_READY; \
  HIP_TRY(hipSetDevice((c)->device));

#define RTOC_MAX_CHUNK_EVENTS 16
#define RTOC_SCAN_AUTO_MAX_BATCH 8  // measured on MI355X (profiles/r01_scan_batch_crossover.log): the scan wins up to ~16 ANYmal / ~10 iCub instances

namespace rtoc {

// the text rtoc_error_string returns for RTOC_ERR_HIP (rtoc_capi.hip; per thread)
void ctx_set_err(hipError_t e, const char* file, int line);

// the device-to-device copies of rtoc_clone, in a row: the first error ends them
struct CopyChain {
  hipStream_t stream;
  hipError_t e;
  template <class T>
  void operator()(DevBuf<T>& dst, const DevBuf<T>& src) {
    if (e == hipSuccess) e = dst.copy_from(src, stream);
  }
};

// hipFuncAttributeMaxDynamicSharedMemorySize of the linearisation kernels for a model (rt_eval_kkt.hip)
hipError_t set_linearize_lds(const rtoc_robot_model& m, int nlevels, int nbranch, int dpp);

// the backward recursion of one public call, as plan_backward decides it
enum BwdPath { BWD_SCAN, BWD_RV, BWD_RW, BWD_TILE };
struct BwdPlan {
  BwdPath path = BWD_SCAN;  // horizon scan, register-resident, register-wide (iCub-size shapes), tile-split / role-split
  const Kern<BwdArgs>* kern = nullptr;  // the kernel of the path (scan: its policy kernel; register-wide: the one between the one-stage launches)
  int check_fxx = 0;        // BwdArgs::check_fxx of the register-resident kernel: verify the structured rows as it goes
};
// Streams and events of a context.  A base of rtoc_ctx, so that it is destroyed after every member: device memory is freed
// first, streams and events go last.
struct CtxStreams {
  hipStream_t own_stream = nullptr;
  hipStream_t stream2 = nullptr;  // forward half of the pipelined sweep
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_chunk[RTOC_MAX_CHUNK_EVENTS] = {};
  CtxStreams() = default;
  CtxStreams(const CtxStreams&) = delete;
  CtxStreams& operator=(const CtxStreams&) = delete;
  ~CtxStreams() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    for (hipEvent_t e : ev_chunk)
      if (e) (void)hipEventDestroy(e);
  }
};
// The scalar settings rtoc_clone hands to the new context in one assignment (a base of rtoc_ctx: c->writeback etc.)
struct CtxOptions {
  int writeback = 0;
  double max_dts0 = 0.1;  // RiccatiRecursion(ocp, max_dts0 = 0.1), riccati_recursion.hpp:35
  double contact_inv_damping = 0.0;
  int bwd_variant = 0;
  int sweep_chunks = 1;         // measured on MI355X: chunked pipelining does not pay (forward waves do not fit next to the backward waves)
  int condense_split = 0;       // 1: MJtJinv in its own kernel ahead of the condensation
  int keep_qaf = 0;             // RTOC_OPT_CONDENSE_KEEP_QAF
  int fxx_mode = 0;             // RTOC_OPT_FXX_STRUCTURE: 0 auto, 1 dense, 2 caller asserts the structure
  int bwd_register = 1;         // RTOC_OPT_BACKWARD_REGISTER: the register-resident backward kernel where it applies (plan_backward)
  int cond_register = 1;        // RTOC_OPT_CONDENSE_REGISTER: the register-chained condensation of the contact grid points where it applies
  int use_graph = 0;            // RTOC_OPT_GRAPH: launch sequences replayed from captured hipGraphs
  int exact_transport = 0;      // RTOC_OPT_SWITCHING_TRANSPORT
  int unconstr_dense = 0;       // RTOC_OPT_UNCONSTR_DENSE
  int exact_cone_jacobian = 0;  // RTOC_OPT_CONE_JACOBIAN
  int impact_cones = 1;         // RTOC_OPT_IMPACT_CONES
  int linearize_fused = 0;      // RTOC_OPT_LINEARIZE_FUSED
  int lin_dpp = 0;              // RTOC_OPT_LINEARIZE_DOFS_PER_PASS (0 = per model)
  double barrier = 0.0, ftb_rule = 0.0;
  int n_mu = 0;                 // how many of d_mu's RTOC_MAX_CONTACTS entries the caller set
  // filter line search on the device (rtoc_set_line_search, rtoc_contact_line_search)
  int ls_on = 0;
  double ls_rate = 0.0, ls_min_step = 0.0, ls_cost_rate = 0.0, ls_viol_rate = 0.0;
  int ls_method = 0;  // 0 LineSearchMethod::Filter, 1 MeritBacktracking (rtoc_set_line_search_method)
  double ls_armijo = 0.0, ls_margin = 0.0, ls_eps = 0.0;
};
struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  unsigned long long epoch = 0, warm_epoch = 0;
  double p0 = 0.0, p1 = 0.0;
  bool warm = false;
  ~GraphSlot() {
    if (exec) (void)hipGraphExecDestroy(exec);
  }
};

// ---- the state of a context by subsystem: bases of rtoc_ctx (c->sto_on etc.).  A clone_from copies the members listed ahead of
// it, every buffer with the capacity it has in src, whatever part of it is in use; what follows it is scratch, not copied ----

// Riccati recursion (rt_sweep.hip).  Nothing here is cloned: rtoc_clone replays RTOC_OPT_BACKWARD_SCAN through rtoc_set_option
struct SweepState {
  int fxx_state = 0;             // auto mode cache: 0 unknown (re-check before the next backward recursion), 1 every Fxx structured, 2 not
  BwdPlan bwd_plan;              // the last plan_backward's answer: the backward kernel baked into captured graphs
  DevBuf<int> d_fxx_flag;
  int backward_scan = 0;         // RTOC_OPT_BACKWARD_SCAN
  DevBuf<double> d_scan[3];      // element ping-pong buffers, value records (allocated on first use)
  DevBuf<double> d_scan_sto;     // riccati_scan_sto.hpp: per grid point At, P+ Fx, P+ fx, factors of G
};

// box rows and cones (rt_condense.hip; their values at the iterate: rt_eval_kkt.hip)
struct ConstraintState {
  DevBuf<double> d_bounds;    // rtoc_set_constraint_bounds: [nc_max]
  DevBuf<double> d_mu;        // rtoc_set_friction_coefficients
  DevBuf<double> d_wcone;     // rtoc_set_wrench_cone_params: [RTOC_MAX_CONTACTS][17 x 6]
  void clone_from(const ConstraintState& src, CopyChain& dup) {
    dup(d_bounds, src.d_bounds);
    dup(d_mu, src.d_mu);
    dup(d_wcone, src.d_wcone);
  }
  // not copied: rtoc_clone replays the rows and the cones through their public setters
  DevBuf<rtoc_box_row> d_rows;
  std::vector<rtoc_box_row> h_rows;  // host copy (stage dump, rtoc_clone)
  DevBuf<int> d_pair;   // first two rows of every primal entry, packed (int4 per entry)
  DevBuf<int> d_entry;  // CSR over the primal entries (q_0..,v_0..,u_0..): [ne+1] offsets, then [nrows] row ids
  int nrows = 0;
  int cone_contacts = 0, cone_dim = 0;  // friction / wrench cones: max contacts (0 = off), force components per contact
  int cone_rows = 0;                    // PDIPM rows per contact: 5 friction cone, 17 contact wrench cone
};

// rigid-body model (rtoc_set_robot_model), contact schedule (rtoc_set_contact_schedule), cost and initial state, and the
// results of evalKKT (rt_eval_kkt.hip)
struct ModelState {
  DevBuf<rbd::DevModel> d_model;
  std::unique_ptr<rbd::DevModel> h_model;
  DevBuf<unsigned> d_active;
  bool active_current = false;  // the schedule was set since the last rtoc_set_grid: its masks belong to the grid in force
  std::vector<unsigned> h_active;  // host copy of the masks (which placements rtoc_set_contact_placements checks)
  // desired contact placements (rt_placements.hip), rows of [ncontacts][3 | 9]: always committed together -- one mode, one grid, that
  // of the schedule (active_current); on: positions / rotations were given (else zeros / identities)
  GridTable<double> cpos, crot;
  DevBuf<double> d_cost;      // rtoc_set_configuration_cost: 12 (nv + 1) doubles
  DevBuf<double> d_x0;        // rtoc_set_initial_state: [batch][nq + nv]
  // rtoc_set_configuration_ref_table: q_ref rows of nq doubles and their isActive (capacity: max_stages rows, or [batch] of them),
  // always committed together; qtab.on: a table is in use
  GridTable<double> qtab;
  GridTable<int> qtab_active;
  // false: no memory for the host copy of the model (no HIP error to report)
  bool clone_from(const ModelState& src, CopyChain& dup) {
    if (src.h_model) {
      h_model.reset(new (std::nothrow) rbd::DevModel(*src.h_model));
      if (!h_model) return false;
      dup(d_model, src.d_model);
      if (dup.e == hipSuccess) dup.e = set_linearize_lds(h_model->m, h_model->nlevels, h_model->nbranch, h_model->dpp);
    }
    dup(d_active, src.d_active);
    active_current = src.active_current;
    h_active = src.h_active;
    cpos.clone_from(src.cpos, dup);
    crot.clone_from(src.crot, dup);
    dup(d_cost, src.d_cost);
    dup(d_x0, src.d_x0);
    qtab.clone_from(src.qtab, dup);
    qtab_active.clone_from(src.qtab_active, dup);
    return true;
  }
  // not copied: scratch and results of the last evaluation
  DevBuf<double> d_vals, d_vals2;  // rbd_values_kernel -> linearize_contact_dynamics_kernel<.., PRE>: [batch * max_stages][njoints][rbd::VAL_DOUBLES]
  int vals_fresh = 0;            // the values in d_vals belong to the iterate in RTOC_BUF_SOL (consumed by the next launch_linearize)
  DevBuf<double> d_costval;      // [batch][max_stages] cost values of the last rtoc_contact_eval_kkt (rtoc_contact_eval_ocp)
  DevBuf<double> d_kkterr;       // [batch] + [batch][max_stages] partial sums
  DevBuf<int> d_nconv;           // instances found converged by the last rtoc_newton_iteration
  DevBuf<double> d_fk;           // rtoc_contact_frame_placements: [batch][RTOC_MAX_CONTACTS][9 + 3] + [batch][3] ahead of the download
};

// task-space cost components (rtoc_set_task_costs; task_space_cost.hpp; rt_task_costs.hip)
struct TaskState {
  DevBuf<rtoc_task_cost> d_tasks;  // capacity [batch][RTOC_MAX_TASK_COSTS]; in use [ntasks] or [batch][ntasks]
  int ntasks = 0, tasks_per_instance = 0;
  unsigned h_task_table = 0;       // bit k: term k (of some instance) has ref_kind RTOC_REF_TABLE
  unsigned h_task_3d = 0, h_task_com = 0;   // bit k: term k of EVERY instance is a RTOC_TASK_FRAME_3D / a RTOC_TASK_COM term
  DevBuf<double> d_gt;             // [max_stages] GridInfo::t of a fixed grid (rtoc_set_grid_times)
  std::vector<double> h_gt;        // host copy of the same, its size = the grid it belongs to (empty: none)
  // reference tables of RTOC_REF_TABLE terms (rtoc_set_task_ref_table), by term index: capacity [max_stages] or [batch][max_stages] entries
  GridTable<rtoc_task_ref_entry> reftab[RTOC_MAX_TASK_COSTS];
  int task_rows = 0, task_ext = 0; // LDS rows of the term lists (the largest instance), 1: a 6D term or a table reference among them
  // LocalContactForceCost (rtoc_set_contact_force_cost; contact_force_cost.hpp): capacity [batch]; in use [1] or [batch]
  DevBuf<rtoc_contact_force_cost> d_fcost;
  int fcost_on = 0, fcost_per_instance = 0;
  void clone_from(const TaskState& src, CopyChain& dup) {
    if (src.ntasks > 0) {
      ntasks = src.ntasks, tasks_per_instance = src.tasks_per_instance;
      dup(d_tasks, src.d_tasks);
    }
    dup(d_gt, src.d_gt);
    h_gt = src.h_gt;
    task_rows = src.task_rows, task_ext = src.task_ext, h_task_table = src.h_task_table;
    h_task_3d = src.h_task_3d, h_task_com = src.h_task_com;
    for (int k = 0; k < RTOC_MAX_TASK_COSTS; ++k) reftab[k].clone_from(src.reftab[k], dup);
    if (src.fcost_on) {
      fcost_on = 1, fcost_per_instance = src.fcost_per_instance;
      dup(d_fcost, src.d_fcost);
    }
  }
};

// switching-time optimisation on the device (rtoc_sto_set_problem; sto.hpp; rt_sto.hip)
struct StoState {
  int sto_on = 0, sto_nev = 0;
  double sto_t0 = 0.0, sto_T = 0.0, sto_barrier = 0.0, sto_tau = 0.0, sto_reg = 0.0;
  DevBuf<double> d_ts;         // [batch][nev] event times of every instance
  DevBuf<double> d_dt;         // [batch][max_stages] time steps of every instance (grid_dt)
  bool dt_current = false;     // sto_time_steps_kernel ran since the last rtoc_set_grid: d_dt belongs to the grid in force
  DevBuf<double> d_sto_con;    // [batch][RTOC_STO_CON_STRIDE] dwell-time rows
  DevBuf<double> d_min_dwell;  // [RTOC_STO_MAX_EVENTS + 1]
  DevBuf<double> d_sto_cost;   // [2][batch][nev] STO cost gradient / Hessian diagonal handed over by the host, or unallocated
  DevBuf<double> d_sto_out;    // [2][batch][nev] + [batch]: lt, Qtt diagonal as scattered, squared STO KKT term
  DevBuf<double> d_gt_inst;    // [batch][max_stages] per-instance grid times written by sto_time_steps_kernel, or unallocated
  void clone_from(const StoState& src, CopyChain& dup) {
    if (!src.sto_on) return;
    sto_on = 1, sto_nev = src.sto_nev, sto_t0 = src.sto_t0, sto_T = src.sto_T;
    sto_barrier = src.sto_barrier, sto_tau = src.sto_tau, sto_reg = src.sto_reg;
    dt_current = src.dt_current;
    dup(d_ts, src.d_ts);
    dup(d_dt, src.d_dt);
    dup(d_sto_con, src.d_sto_con);
    dup(d_min_dwell, src.d_min_dwell);
    dup(d_sto_cost, src.d_sto_cost);
    dup(d_sto_out, src.d_sto_out);
    dup(d_gt_inst, src.d_gt_inst);
  }
  // not copied
  DevBuf<double> d_sto;        // rtoc_sto_eval_kkt staging: lt, diag(Qtt), squared error
};

// line search (rt_line_search.hip).  rtoc_line_search_filter: filters [batch][CAP][2], sizes [batch], staging (cost, violation |
// mask, accepted)
struct LineSearchState {
  DevBuf<double> d_filter;
  DevBuf<int> d_nfilter;
  DevBuf<double> d_ls_in;
  DevBuf<int> d_ls_flags;
  void clone_from(const LineSearchState& src, CopyChain& dup) {
    if (!src.d_filter.p) return;
    dup(d_filter, src.d_filter);
    dup(d_nfilter, src.d_nfilter);
    dup(d_ls_in, src.d_ls_in);
    dup(d_ls_flags, src.d_ls_flags);
  }
  // not copied: the state and scratch of one line search
  DevBuf<double> d_ls_merit;   // [batch] penalty parameter + [batch] directional derivative
  double ls_unconstr_dt = 0.0; // > 0: the last evalKKT was rtoc_unconstr_eval_kkt(dt) -- trial iterates of the line search are evaluated by it
  DevBuf<double> d_eval;       // [2][2][batch]: (cost + barrier | violation) of the current iterate, of the trial iterate
  DevBuf<double> d_eval_part;  // [batch][max_stages][2]
  DevBuf<double> d_sol_trial;  // trial iterate: SplitSolution records, constraint records, steps
  DevBuf<double> d_con_trial;
  DevBuf<double> d_ls_steps;   // [batch][2] trial steps + [batch] alpha
  DevBuf<int> d_ls_active;     // [batch] active flags + [1] counter
  int ls_trials = 0;           // trial evaluations of the last line search
};

// ParNMPC (rtoc_parnmpc_set_horizon; parnmpc_backward_correction.hpp; rt_parnmpc.hip).  parnmpc: the context's records are the N
// stages of a ParNMPC horizon -- every one carries dynamics and rows, none is terminal; 0 again after rtoc_set_grid
struct ParnmpcState {
  int parnmpc = 0;
  DevBuf<double> d_aux;    // [batch][max_stages][2nv x 2nv] auxiliary matrices (in use: [batch][nstages])
  DevBuf<double> d_snew;   // [batch][max_stages][5nv] s_new
  DevBuf<double> d_xres;   // [batch][max_stages][2nv] x_res
  DevBuf<double> d_kinv;   // [batch][max_stages][16 nv^2] the blocks of K^-1 the correction passes read
  void clone_from(const ParnmpcState& src, CopyChain& dup) {
    parnmpc = src.parnmpc;
    dup(d_aux, src.d_aux);
    dup(d_snew, src.d_snew);
    dup(d_xres, src.d_xres);
    dup(d_kinv, src.d_kinv);
  }
};

// SolutionInterpolator on the device (rtoc_solution_store / rtoc_solution_interpolate; solution_interpolate.hpp; rt_interpolate.hip).
// A copy of everything the interpolation reads of the grid the solution belongs to: rtoc_set_grid, rtoc_set_contact_schedule and
// rtoc_sto_set_problem come between the store and the interpolation.  Capacities are those of max_stages; in use: isol_n points
struct InterpState {
  int isol_n = 0;             // grid points of the stored solution; 0: nothing stored
  int isol_per_instance = 0;  // the times and time steps are every instance's own (stored with an STO problem set)
  int isol_ncontacts = 0;     // what packed the stored stacks: the model's contacts and which of them have 6 rows
  unsigned isol_six_rows = 0;
  DevBuf<double> d_isol;         // [batch][isol_n] SplitSolution records
  DevBuf<double> d_isol_t;       // [batch][max_stages] grid times ([isol_n] or [batch][isol_n] in use), then as many time steps
  DevBuf<int> d_isol_type;       // [max_stages] RTOC_GRID_*
  DevBuf<unsigned> d_isol_mask;  // [max_stages] contact schedule
  void clone_from(const InterpState& src, CopyChain& dup) {
    if (!src.isol_n) return;
    isol_n = src.isol_n, isol_per_instance = src.isol_per_instance;
    isol_ncontacts = src.isol_ncontacts, isol_six_rows = src.isol_six_rows;
    dup(d_isol, src.d_isol);
    dup(d_isol_t, src.d_isol_t);
    dup(d_isol_type, src.d_isol_type);
    dup(d_isol_mask, src.d_isol_mask);
  }
  // not copied: the times of the grid being interpolated onto
  DevBuf<double> d_interp_t;     // [batch][max_stages]
};

// ControlPolicy on the device (rtoc_control_policy / rtoc_control_input; control_policy.hpp; rt_control_policy.hip).  The calls hold
// no state: nothing here is cloned, all of it is scratch of one call
struct PolicyState {
  DevBuf<double> d_policy_tg;     // grid times: [max_stages], with an STO problem [batch][max_stages] ([nstages] or [count][nstages] in use)
  DevBuf<double> d_policy_stage;  // host-pointer calls: t [batch], x [batch][nq + nv], the result [batch][policy stride]
};

// TrotFootStepPlanner and the MPC references on the device (rtoc_set_foot_step_planner ..; foot_step_planner.hpp; rt_foot_steps.hip).
// The device layouts ([slot][batch]) are the kernel header's
struct FootStepState {
  int fs_on = 0;             // a planner is set
  int fs_init = 0;           // rtoc_foot_step_planner_init ran since
  rtoc_foot_step_planner fs_shared = {};   // mode, projection, timing, gain, enable_stance_phase: what the batch shares
  int fs_current_step = 0;   // current_step_: kept once, on the host
  int fs_size = 0;           // steps of the plan on the device; 0: none
  DevBuf<double> d_fs_cmd;   // [FS_CMD_SLOTS][batch] commands
  DevBuf<double> d_fs_state; // [FS_STATE_SLOTS][batch] rotation, local offsets (the biped walk: leg distance, CoM height), filter
  DevBuf<double> d_fs_plan;  // [RTOC_MAX_PLAN_STEPS + 2][FS_PLAN_SLOTS | FS_BIPED_SLOTS][batch]
  DevBuf<double> d_fs_q0;    // [batch][nq] the q of the init
  DevBuf<double> d_fs_qgoal; // the jump: [batch][nq] q_goal of init(q), which the second kinematics pass reads
  DevBuf<double> d_fs_qref;  // the jump: [batch][nq] the q_ref of MPCJump::init
  void clone_from(const FootStepState& src, CopyChain& dup) {
    if (!src.fs_on) return;
    fs_on = 1, fs_init = src.fs_init, fs_shared = src.fs_shared, fs_current_step = src.fs_current_step, fs_size = src.fs_size;
    dup(d_fs_cmd, src.d_fs_cmd);
    dup(d_fs_state, src.d_fs_state);
    dup(d_fs_plan, src.d_fs_plan);
    dup(d_fs_q0, src.d_fs_q0);
    dup(d_fs_qgoal, src.d_fs_qgoal);
    dup(d_fs_qref, src.d_fs_qref);
  }
  // not copied: the scratch of one call
  DevBuf<double> d_fs_fk;    // [batch][4][3] foot positions + [batch][3] centre of mass (contact_frame_placements_kernel); the biped
                             // walk: [batch][2][3] + [batch][3] + [batch][2][9] frame rotations
  DevBuf<int> d_fs_phase;    // [max_stages] phase of every grid point + [RTOC_MAX_PLAN_STEPS + 2] masks of the phases
};

}  // namespace rtoc

struct rtoc_ctx : rtoc::CtxStreams, rtoc::CtxOptions, rtoc::SweepState, rtoc::ConstraintState, rtoc::ModelState, rtoc::TaskState,
                  rtoc::StoState, rtoc::LineSearchState, rtoc::ParnmpcState, rtoc::InterpState, rtoc::PolicyState, rtoc::FootStepState {
  rtoc_dims dims = {};
  rtoc_layout L = {};
  const rtoc::KernelSet* ks = nullptr;
  int max_stages = 0, nstages = 0, batch = 0, device = 0;
  hipStream_t stream = nullptr;  // own_stream, or the caller's (rtoc_set_stream)
  rtoc::DevBuf<double> buf[RTOC_NUM_BUFFERS];
  size_t want[RTOC_NUM_BUFFERS] = {};  // doubles of a buffer at max_stages (rtoc_buffer_count), allocated or not
  bool kkt_exposed = false;  // rtoc_device_ptr(RTOC_BUF_KKT) was handed out: the caller can rewrite the records without the runtime seeing it
  rtoc::DevBuf<rtoc_grid> d_grid;
  std::vector<rtoc_grid> h_grid;  // host copy (stage dump, rtoc_clone)
  rtoc::DevBuf<uint32_t> d_status;
  rtoc::DevBuf<long long> d_prof;
  int num_cus = 0;               // compute units of the device (the register-wide iCub kernel runs where the batch fills them)
  rtoc::DevBuf<int> d_stage_list;  // [max_stages] grid points 0 .. nstages - 2: the contact ones first (n_stage_contact), then the impact ones
  int n_stage_contact = 0, n_stage_impact = 0;
  unsigned long long graph_replays = 0;  // hipGraphLaunch count of RTOC_OPT_GRAPH (rtoc_graph_replay_count)
  unsigned long long epoch = 0;  // bumped by everything that changes a launch parameter baked into a captured graph
  // rtoc_clone: the record buffers that exist in src, and the status words
  void clone_records(const rtoc_ctx& src, rtoc::CopyChain& dup) {
    for (int b = 0; b < RTOC_NUM_BUFFERS; ++b) {
      if (!src.buf[b].p) continue;
      want[b] = src.want[b];
      dup(buf[b], src.buf[b]);
    }
    dup(d_status, src.d_status);
  }
  // RTOC_OPT_GRAPH: the captured launch sequences.  Declared last: destroyed before the memory their nodes name is freed
  rtoc::GraphSlot g_sweep, g_newton;
};

namespace rtoc {

// every launch of a kernel of the set: block size and LDS are the descriptor's (extra_lds: what only the launch knows)
template <class A>
static void launch(const Kern<A>& k, dim3 grid, hipStream_t stream, const A& a, int extra_lds = 0) {
  hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), (size_t)(k.lds + extra_lds), stream, a);
}
// nq of the context's robot: a free-flyer base carries a quaternion
static inline int config_dim(const rtoc_ctx* c) { return c->dims.nv + (c->dims.np == 6 ? 1 : 0); }
// A table writer's two steps around filling t.target(), on the host or on the device: an allocation of `row` elements per grid point
// of the largest grid (per instance: of each); then the rows are the table of the grid in force -- a new epoch where commit says so
template <class T>
static inline hipError_t stage_rows(const rtoc_ctx* c, GridTable<T>& t, size_t row, int inst) { return t.stage((size_t)c->max_stages * (inst ? c->batch : 1) * row); }
template <class T>
static inline void commit_rows(rtoc_ctx* c, GridTable<T>& t, int inst, int on = 1) { c->epoch += t.commit(c->nstages, inst, on) ? 1 : 0; }
// The tables a new grid outdates (rtoc_set_grid, rtoc_parnmpc_set_horizon).  The placements go with the schedule: active_current
static inline void forget_grid_tables(rtoc_ctx* c) {
  for (auto& t : c->reftab) t.forget();
  c->qtab.forget(), c->qtab_active.forget();
}
// role-split kernel where it exists
static inline int default_bwd_variant(const KernelSet* ks) { return (ks->nvariants >= 3) ? ks->nvariants - 1 : 0; }

// RTOC_OPT_GRAPH: run `body` (a sequence of kernel launches on c->stream, no allocation, no synchronisation; its backward plan
// resolved by the caller) from a captured hipGraph.  The first call at a given configuration epoch runs it plainly (lazy allocations happen there),
// the second captures and instantiates, later calls are one hipGraphLaunch -- a single-OCP Newton iteration is ~25
// small kernels, whose launch gaps are a third of its latency.
template <class Body>
static int run_graphed(rtoc_ctx* c, GraphSlot* g, double p0, double p1, Body body) {
  if (!c->use_graph) return body();
  if (g->exec && g->epoch == c->epoch && g->p0 == p0 && g->p1 == p1) {
    HIP_TRY(hipGraphLaunch(g->exec, c->stream));
    c->graph_replays++;
    return RTOC_OK;
  }
  if (!(g->warm && g->warm_epoch == c->epoch)) {
    const int rc = body();
    g->warm = true;
    g->warm_epoch = c->epoch;  // after the body: its lazy allocations bump the epoch
    return rc;
  }
  if (g->exec) {
    (void)hipGraphExecDestroy(g->exec);
    g->exec = nullptr;
  }
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
  const int rc = body();
  const hipError_t e = hipStreamEndCapture(c->stream, &graph);
  if (rc || e != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    if (e != hipSuccess) ctx_set_err(e, __FILE_NAME__, __LINE__);
    return rc ? rc : RTOC_ERR_HIP;
  }
  const hipError_t e2 = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e2 != hipSuccess) {
    g->exec = nullptr;
    ctx_set_err(e2, __FILE_NAME__, __LINE__);
    return RTOC_ERR_HIP;
  }
  g->epoch = c->epoch;
  g->p0 = p0;
  g->p1 = p1;
  HIP_TRY(hipGraphLaunch(g->exec, c->stream));
  c->graph_replays++;
  return RTOC_OK;
}

// ---- what one unit calls in another ----
// rt_shapes.hip
const KernelSet* find_set(const rtoc_dims* d);
// rtoc_capi.hip
int ensure_buffer(rtoc_ctx* c, int b);
RecView view(const rtoc_ctx* c);
// The argument block of a kernel that takes the view (record_view.hpp), as its launcher starts it: every field zero, the view as
// the context stands now.  Called at the launch, never earlier: rtoc_bind and eval_ocp_trial change the pointers between launches
template <class A>
static A view_args(const rtoc_ctx* c) {
  static_assert(takes_view<A>, "a runtime kernel's block starts with `RecView rv` and is copied into the kernarg segment as it stands");
  A a{};
  a.rv = view(c);
  return a;
}
// rt_sweep.hip
int ensure_scan_buffers(rtoc_ctx* c);
int plan_backward(rtoc_ctx* c, BwdPlan* out);
int launch_backward(rtoc_ctx* c, const BwdPlan& p);
int launch_forward(rtoc_ctx* c);
int launch_sweep(rtoc_ctx* c, const BwdPlan& p);
// rt_condense.hip
ConeRows view_cones(const rtoc_ctx* c);
void launch_fill_steps(rtoc_ctx* c);
// rt_eval_kkt.hip
hipError_t reserve_active(rtoc_ctx* c, bool* fresh = nullptr);
ModelDims model_dims(const rtoc_ctx* c);   // (c->h_model is set)
hipError_t reserve_kkterr(rtoc_ctx* c);
int launch_kkt_error(rtoc_ctx* c);
// records per instance that carry dynamics and rows: all but the terminal one, or all of a ParNMPC horizon
static inline int dynamics_records(const rtoc_ctx* c) { return c->nstages - 1 + (c->parnmpc ? 1 : 0); }
// the unconstrained path's pieces rt_parnmpc.hip strings together: the all-zero contact schedule, linearizeUnconstrDynamics with
// its dt-scaled multiplier terms, one phase of the joint-limit rows (unconstr_constraints.hpp: UBOX_*)
enum UnconstrRowsPhase { ROWS_INIT = 0, ROWS_LINEARIZE = 1, ROWS_CONDENSE = 2, ROWS_EXPAND = 3 };
int reserve_empty_schedule(rtoc_ctx* c);
int launch_unconstr_linearize(rtoc_ctx* c, double dt);
bool unconstr_rows_on(const rtoc_ctx* c);
int launch_unconstr_rows(rtoc_ctx* c, UnconstrRowsPhase phase);
// rt_placements.hip, for rt_foot_steps.hip: a schedule that belongs to the grid in force (else RTOC_ERR_NOT_READY); the per-instance
// placement table from whatever is in force, every instance starting from the shared values (need_rot: a rotation table too, created
// if there is none); contact_frame_placements_kernel at the q of rtoc_set_initial_state, out_p[batch][ncontacts][3], out_com[batch][3]
// (nullptr: left out) and, for the contact surfaces of the biped walk, out_R[batch][ncontacts][9] row-major
int placements_ready(const rtoc_ctx* c);
int placements_per_instance(rtoc_ctx* c, bool need_rot);
int launch_frame_positions(rtoc_ctx* c, double* out_p, double* out_com, double* out_R = nullptr, const double* q = nullptr, size_t q_stride = 0);
// rt_task_costs.hip
int ensure_grid_times_inst(rtoc_ctx* c);
int task_costs_ready(rtoc_ctx* c, bool unconstr);
int launch_task_costs(rtoc_ctx* c, double unconstr_dt, double* cost_out);
int launch_force_cost(rtoc_ctx* c, double* cost_out);
// rt_sto.hip
// one kernel of sto.hpp over the instances of the context
enum StoKernel { STO_TIME_STEPS, STO_INIT, STO_EVAL_KKT, STO_STEP_SIZES, STO_INTEGRATE };
int launch_sto(rtoc_ctx* c, StoKernel k);
// rt_line_search.hip
int ensure_line_search(rtoc_ctx* c);
int launch_eval_ocp(rtoc_ctx* c, double* out);

}  // namespace rtoc
