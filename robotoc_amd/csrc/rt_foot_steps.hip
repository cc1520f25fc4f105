// rt_foot_steps.hip -- the foot-step planners (trot, crawl, pace, flying trot; the biped walk on two contact surfaces; the jump on either kind of feet) and the MPC references of every instance on the device: planner and commands, init,
// plan, the read-back of the plan, the placements of every contact phase, the three periodic references (foot_step_planner.hpp).
#include <cmath>

#include "rt_context.hpp"
#include "foot_step_planner.hpp"

using namespace rtoc;

#define CHECK_NO_PARNMPC(c)          \
  if (!(c)) return RTOC_ERR_BAD_ARG; \
  if ((c)->parnmpc) return RTOC_ERR_BAD_ARG;

static constexpr int FS_MAX_STEPS = RTOC_MAX_PLAN_STEPS + 2;
// the kinematics' scratch per instance: [4][3] + the centre of mass, or the biped walk's [2][3] + [3] + [2][9]; the jump's init
// keeps a second centre of mass (at q_goal) behind them
static constexpr int FS_FK_DOUBLES = 30;

// the gait of the reference's quadrupeds: exactly four point contacts (LF, LH, RF, RH = contacts 0..3)
static bool four_point_feet(const rtoc_ctx* c) {
  const rtoc_robot_model& m = c->h_model->m;
  if (m.ncontacts != 4) return false;
  for (int k = 0; k < 4; ++k)
    if (m.contact_type[k] != RTOC_CONTACT_POINT) return false;
  return true;
}
// the biped of the reference's walk: exactly two surface contacts (left, right = contacts 0, 1 = surfaceContactFrames()[0], [1])
static bool two_surface_feet(const rtoc_ctx* c) {
  const rtoc_robot_model& m = c->h_model->m;
  return m.ncontacts == 2 && m.contact_type[0] == RTOC_CONTACT_SURFACE && m.contact_type[1] == RTOC_CONTACT_SURFACE;
}
static bool jump(const rtoc_ctx* c) { return c->fs_shared.gait == RTOC_GAIT_JUMP; }
// the feet of the planner in force, which choose the plan's layout and the kernels' form: the biped walk has two, the jump as many as
// the model it was set for (a planner does not outlive its model), every other gait four
static int plan_feet(const rtoc_ctx* c) {
  if (c->fs_shared.gait == RTOC_GAIT_BIPED_WALK) return 2;
  return jump(c) && two_surface_feet(c) ? 2 : 4;
}
static bool biped(const rtoc_ctx* c) { return plan_feet(c) == 2; }
// doubles per (instance, step) of the plan on the device
static int plan_slots(const rtoc_ctx* c) { return biped(c) ? FS_BIPED_SLOTS : FS_PLAN_SLOTS; }
// setGaitPattern has no checks; setRaibertGaitPattern: trot_foot_step_planner.cpp:68-76 (the period of raibert_heuristic.cpp:39 is
// positive with them, its gain check is the same one; biped_walk_foot_step_planner.cpp:66-74 are the same three)
static bool planner_valid(const rtoc_foot_step_planner& p) {
  if (p.gait < RTOC_GAIT_TROT || p.gait > RTOC_GAIT_JUMP) return false;
  if (p.mode != RTOC_FOOT_STEP_FIXED && p.mode != RTOC_FOOT_STEP_RAIBERT) return false;
  if (p.gait == RTOC_GAIT_JUMP && p.mode != RTOC_FOOT_STEP_FIXED) return false;   // setJumpPattern alone: there is no Raibert form of a jump
  if (p.projection != RTOC_PROJECT_AS_REFERENCE && p.projection != RTOC_PROJECT_YAW) return false;
  if (p.enable_stance_phase != 0 && p.enable_stance_phase != 1) return false;
  if (p.mode == RTOC_FOOT_STEP_RAIBERT && (!(p.swing_time > 0.0) || !(p.stance_time >= 0.0) || !(p.gain > 0.0))) return false;
  // flying_trot_foot_step_planner.cpp:66: the flying trot has no gait without a stance
  if (p.gait == RTOC_GAIT_FLYING_TROT && p.mode == RTOC_FOOT_STEP_RAIBERT && !(p.stance_time > 0.0)) return false;
  return true;
}
// what decides the step-case sequence: shared structure, like the grid
static bool same_structure(const rtoc_foot_step_planner& a, const rtoc_foot_step_planner& b) {
  return a.gait == b.gait && a.mode == b.mode && a.projection == b.projection && a.enable_stance_phase == b.enable_stance_phase &&
         a.swing_time == b.swing_time && a.stance_time == b.stance_time && a.gain == b.gain;
}
static bool stance_phase_enabled(const rtoc_foot_step_planner& p) {
  if (p.gait == RTOC_GAIT_FLYING_TROT) return false;   // no such option: one step sequence (flying_trot_foot_step_planner.cpp:190-230)
  return p.mode == RTOC_FOOT_STEP_RAIBERT ? p.stance_time > 0.0 : p.enable_stance_phase != 0;   // :58, :86
}

// What tells the gaits' case chains apart, by RTOC_GAIT_*.  Index [0]: without the stance phase, [1]: with it.
struct GaitSwing {
  unsigned status;   // a contact status with feet in the air ...
  int at[2];         // ... is the step with current_step_ % cycle == at: otherwise current_step_ advances and R turns
};
struct GaitRules {
  int cycle[2];                // the steps repeat with this period
  unsigned char move[2][8];    // the feet that step at step % cycle (0: nothing moves, nothing turns)
  GaitSwing swing[4];
  int nswing;
  int flight;                  // 1: 0b0000 is a status (current_step_ to the next even number, no rotation)
  int incremental;             // 1: feet advance from where they are
  double com_scale;            // the CoM's share of step_length_ per moving step
  double periods;              // the Raibert period in units of swing_time + stance_time
  unsigned full = 0b1111u;     // every foot on the ground
};
static const GaitRules GAITS[5] = {
    // trot (trot_foot_step_planner.cpp:161-202, :212-277): LH + RF first
    {{2, 4}, {{0b1001, 0b0110}, {0, 0b0110, 0, 0b1001}}, {{0b1001u, {1, 1}}, {0b0110u, {0, 3}}}, 2, 0, 0, 0.5, 2.0},
    // crawl (crawl_foot_step_planner.cpp:159-250, :260-359): RH, RF, LH, LF
    {{4, 8}, {{0b0001, 0b1000, 0b0100, 0b0010}, {0, 0b1000, 0, 0b0100, 0, 0b0010, 0, 0b0001}},
     {{0b0111u, {1, 1}}, {0b1011u, {2, 3}}, {0b1101u, {3, 5}}, {0b1110u, {0, 7}}}, 4, 0, 1, 0.25, 4.0},
    // pace (pace_foot_step_planner.cpp:160-201, :211-276): RF + RH first
    {{2, 4}, {{0b0011, 0b1100}, {0, 0b1100, 0, 0b0011}}, {{0b0011u, {1, 1}}, {0b1100u, {0, 3}}}, 2, 0, 0, 0.5, 2.0},
    // flying trot (flying_trot_foot_step_planner.cpp:148-183, :190-230): a flight on every odd step
    {{4, 4}, {{0b1001, 0, 0b0110, 0}, {0b1001, 0, 0b0110, 0}}, {{0b1001u, {1, 1}}, {0b0110u, {3, 3}}}, 2, 1, 0, 0.5, 2.0},
    // biped walk (biped_walk_foot_step_planner.cpp:136-191, :201-266): two feet, the right one (contact 1) first; 0b01: the left stands.
    // Only the chain is shared with the quadrupeds: the recurrence itself is biped_walk_plan_kernel
    {{2, 4}, {{0b01, 0b10}, {0, 0b10, 0, 0b01}}, {{0b01u, {1, 1}}, {0b10u, {0, 3}}}, 2, 0, 1, 0.5, 2.0, 0b11u},
};

int rtoc_set_foot_step_planner(rtoc_ctx* c, const rtoc_foot_step_planner* p, int per_instance) {
  CHECK_NO_PARNMPC(c);
  if (!p) {
    c->fs_on = 0, c->fs_init = 0, c->fs_size = 0;   // the state goes with the planner: init again after the next one is set
    return RTOC_OK;
  }
  if (per_instance != 0 && per_instance != 1) return RTOC_ERR_BAD_ARG;
  if (!c->h_model) return RTOC_ERR_NOT_READY;
  const int B = c->batch, n = per_instance ? B : 1;
  for (int b = 0; b < n; ++b)
    if (!planner_valid(p[b]) || !same_structure(p[b], p[0])) return RTOC_ERR_BAD_ARG;
  // a gait and the feet it is written for: the quadrupeds' on four point contacts, the biped walk on two contact surfaces
  // (the jump on either: jump_foot_step_planner.cpp:25-31, with exact counts here)
  const bool feet_fit = p[0].gait == RTOC_GAIT_BIPED_WALK ? two_surface_feet(c)
                        : p[0].gait == RTOC_GAIT_JUMP     ? two_surface_feet(c) || four_point_feet(c)
                                                          : four_point_feet(c);
  if (!feet_fit) return RTOC_ERR_BAD_ARG;
  std::vector<double> cmd((size_t)FS_CMD_SLOTS * B, 0.0);
  for (int b = 0; b < B; ++b) {
    const rtoc_foot_step_planner& q = p[per_instance ? b : 0];
    const bool raibert = q.mode == RTOC_FOOT_STEP_RAIBERT;
    for (int k = 0; k < 3; ++k) cmd[(size_t)(FS_CMD_STEP + k) * B + b] = raibert ? 0.0 : q.step_length[k];
    cmd[(size_t)FS_CMD_YAW * B + b] = raibert ? q.yaw_rate_cmd * (q.swing_time + q.stance_time) : q.step_yaw;   // :81
    for (int k = 0; k < 2; ++k) cmd[(size_t)(FS_CMD_VCOM + k) * B + b] = raibert ? q.vcom_cmd[k] : 0.0;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->d_fs_cmd.reserve(cmd.size()));
  HIP_TRY(hipMemcpyAsync(c->d_fs_cmd.p, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the jump's plan is its init's and nobody else's: going to or from it ends the state (among the other gaits init is one and the same)
  if (c->fs_on && c->fs_shared.gait != p[0].gait && (jump(c) || p[0].gait == RTOC_GAIT_JUMP)) c->fs_init = 0, c->fs_size = 0;
  c->fs_shared = p[0];
  c->fs_on = 1;
  return RTOC_OK;
}

static int reserve_planner(rtoc_ctx* c) {
  const size_t B = c->batch, nq = c->h_model->m.nq;
  HIP_TRY(c->d_fs_fk.reserve(B * FS_FK_DOUBLES));
  HIP_TRY(c->d_fs_state.reserve(B * FS_STATE_SLOTS));
  HIP_TRY(c->d_fs_plan.reserve(B * plan_slots(c) * FS_MAX_STEPS));
  HIP_TRY(c->d_fs_q0.reserve(B * nq));
  return RTOC_OK;
}

// JumpFootStepPlanner::init(q) (:68-124) and the q_ref of MPCJump::init (mpc_jump.cpp:141-145): the kinematics at q, q_goal, the
// kinematics at q_goal, then the three steps of the plan
static int jump_init(rtoc_ctx* c) {
  if (!c->d_fs_cmd.p) return RTOC_ERR_NOT_READY;
  const size_t B = c->batch, nf = plan_feet(c), nq = c->h_model->m.nq;
  HIP_TRY(c->d_fs_qgoal.reserve(B * nq));
  HIP_TRY(c->d_fs_qref.reserve(B * nq));
  double* const feet = c->d_fs_fk.p;
  double* const com = feet + B * nf * 3;
  double* const com_goal = com + B * 3;
  double* const feet_R = nf == 2 ? com_goal + B * 3 : nullptr;
  JumpInitArgs a{};
  a.x0 = c->d_x0.p, a.cmd = c->d_fs_cmd.p, a.feet = feet, a.feet_R = feet_R, a.com = com, a.com_goal = com_goal;
  a.plan = c->d_fs_plan.p, a.qgoal = c->d_fs_qgoal.p, a.qref = c->d_fs_qref.p;
  a.batch = (int)B, a.nq = (int)nq, a.nx = (int)nq + c->h_model->m.nv;
  a.projection = c->fs_shared.projection;
  const unsigned per = 64 / (unsigned)nf;
  const dim3 grid((unsigned)((B + per - 1) / per));
  auto launch = [&](int phase) {
    a.phase = phase;
    if (nf == 2)
      hipLaunchKernelGGL(jump_init_kernel<2>, grid, dim3(64), 0, c->stream, a);
    else
      hipLaunchKernelGGL(jump_init_kernel<4>, grid, dim3(64), 0, c->stream, a);
  };
  int rc = launch_frame_positions(c, feet, com, feet_R);
  if (rc) return rc;
  launch(0);
  HIP_TRY(hipGetLastError());
  rc = launch_frame_positions(c, nullptr, com_goal, nullptr, c->d_fs_qgoal.p, nq);
  if (rc) return rc;
  launch(1);
  HIP_TRY(hipGetLastError());
  c->fs_init = 1, c->fs_current_step = 0, c->fs_size = 3;   // MPCJump::init reads CoM(2) and R(2) before it plans
  return RTOC_OK;
}

int rtoc_foot_step_planner_init(rtoc_ctx* c) {
  CHECK_READY(c);
  if (!c->fs_on || !c->h_model || !c->d_x0.p) return RTOC_ERR_NOT_READY;
  int rc = reserve_planner(c);
  if (rc) return rc;
  if (jump(c)) return jump_init(c);
  const int B = c->batch, nf = plan_feet(c);
  double* const com = c->d_fs_fk.p + (size_t)B * nf * 3;
  rc = launch_frame_positions(c, c->d_fs_fk.p, com);
  if (rc) return rc;
  FsInitArgs a{};
  a.x0 = c->d_x0.p, a.feet = c->d_fs_fk.p, a.com = com;
  a.state = c->d_fs_state.p, a.plan = c->d_fs_plan.p, a.q0 = c->d_fs_q0.p;
  a.batch = B, a.nq = c->h_model->m.nq, a.nx = c->h_model->m.nq + c->h_model->m.nv;
  a.projection = c->fs_shared.projection;
  if (nf == 2)
    hipLaunchKernelGGL(biped_walk_init_kernel, dim3((unsigned)((B + 31) / 32)), dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(foot_step_init_kernel, dim3((unsigned)((B + 15) / 16)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fs_init = 1, c->fs_current_step = 0, c->fs_size = 0;
  return RTOC_OK;
}

// The case chain of plan() (:145-277): current_step_ and the contact status are shared by the batch, so the host walks it once.
// false: a contact status the reference answers with `return false`
// The gait's rules are a table walk (GAITS); what is left to code are the first steps of all, which every gait scales its own way.
// false: a contact status the reference answers with `return false`, or a flight with no plan behind it
static bool plan_cases(const rtoc_foot_step_planner& p, unsigned status, int planning_steps, bool has_plan, int* current_step, FsPlanArgs* a) {
  const GaitRules& g = GAITS[p.gait];
  const int sp = stance_phase_enabled(p) ? 1 : 0;
  const bool raibert = p.mode == RTOC_FOOT_STEP_RAIBERT;
  int cur = *current_step;
  a->stance = status, a->pre_rotate = 0, a->flight = 0, a->incremental = g.incremental;
  if (status == g.full) {
    if (sp) {
      if (cur % 2 != 0) ++cur;
    } else {
      cur = 0;
    }
  } else if (status == 0u && g.flight) {
    if (!has_plan) return false;   // contact_position_ref_[0] of a planner that has not planned (flying_trot_foot_step_planner.cpp:181)
    if (cur % 2 != 0) ++cur;
    a->flight = 1;
  } else {
    int k = 0;
    while (k < g.nswing && g.swing[k].status != status) ++k;
    if (k == g.nswing) return false;
    if (cur % g.cycle[sp] != g.swing[k].at[sp]) ++cur, a->pre_rotate = 1;
  }
  a->nloop = planning_steps + 1;
  for (int s = 0; s <= planning_steps; ++s) {
    const int step = cur + s;
    const unsigned char mv = step == 0 ? 0 : g.move[sp][step % g.cycle[sp]];
    double cs = g.com_scale, fs = 1.0;
    if (p.gait == RTOC_GAIT_CRAWL) {
      // crawl_foot_step_planner.cpp:265-284, :315-334: tested on `step` alone
      if (step == 1 || step == (sp ? 3 : 2)) cs = raibert ? 0.25 : 0.125, fs = 0.5;
    } else if (p.gait == RTOC_GAIT_FLYING_TROT) {
      // flying_trot_foot_step_planner.cpp:194-207: the first flight moves nothing (as every odd step), the step behind it is the first of all
      if (cur == 0 && step == 2) cs = raibert ? 0.5 : 0.25;
    } else if (cur == 0 && step == 1) {
      cs = raibert ? 0.5 : 0.25;   // trot_foot_step_planner.cpp:217-227, pace_foot_step_planner.cpp:216-226
      if (p.gait == RTOC_GAIT_BIPED_WALK) fs = 0.5;   // biped_walk_foot_step_planner.cpp:206-216, :239-249: the right foot by half a step
    }
    a->move[s] = mv, a->com_scale[s] = cs, a->foot_scale[s] = fs;
  }
  if (p.gait == RTOC_GAIT_FLYING_TROT) {
    // flying_trot_foot_step_planner.cpp:231-233: the last step once more
    a->move[a->nloop] = 0, a->com_scale[a->nloop] = 0.0, a->foot_scale[a->nloop] = 0.0;
    ++a->nloop;
  }
  *current_step = cur;
  return true;
}

// JumpFootStepPlanner::plan (:127-170): current_step_ and the contact status are shared by the batch, the host walks the cases
static int jump_plan(rtoc_ctx* c, unsigned status) {
  const int B = c->batch, nf = plan_feet(c);
  if (status >> nf) return RTOC_ERR_BAD_ARG;   // a contact the model does not have
  JumpPlanArgs a{};
  a.plan = c->d_fs_plan.p, a.batch = B;
  int cur = c->fs_current_step, size = c->fs_size;
  if (status) {
    // hasActiveContacts (:132-148)
    if (cur == 1) cur = 2;
    HIP_TRY(c->d_fs_fk.reserve((size_t)B * FS_FK_DOUBLES));   // scratch: a clone starts without it
    double* const feet_R = nf == 2 ? c->d_fs_fk.p + (size_t)B * 6 : nullptr;
    const int rc = launch_frame_positions(c, c->d_fs_fk.p, nullptr, feet_R);
    if (rc) return rc;
    a.feet = c->d_fs_fk.p, a.feet_R = feet_R, a.landed = 1;
  } else {
    if (cur != 0) return RTOC_OK;   // in the air or landed: nothing changes (:150)
    cur = 1, size = 2;
  }
  const unsigned per = 64 / (unsigned)nf;
  const dim3 grid((unsigned)((B + per - 1) / per));
  if (nf == 2)
    hipLaunchKernelGGL(jump_plan_kernel<2>, grid, dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(jump_plan_kernel<4>, grid, dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fs_current_step = cur, c->fs_size = size;
  return RTOC_OK;
}

int rtoc_foot_step_plan(rtoc_ctx* c, double t, unsigned contact_status0, int planning_steps) {
  CHECK_READY(c);
  if (!c->fs_on || !c->fs_init || !c->h_model || !c->d_x0.p || !c->d_fs_state.p || !c->d_fs_plan.p || !c->d_fs_cmd.p) return RTOC_ERR_NOT_READY;
  const bool flying = c->fs_shared.gait == RTOC_GAIT_FLYING_TROT;   // its plan is one step longer
  if (planning_steps < 0 || planning_steps > RTOC_MAX_PLAN_STEPS - (flying ? 1 : 0) || !std::isfinite(t)) return RTOC_ERR_BAD_ARG;
  if (jump(c)) return jump_plan(c, contact_status0);   // t, v and planning_steps are not read (:127-131)
  FsPlanArgs a{};
  int cur = c->fs_current_step;
  if (!plan_cases(c->fs_shared, contact_status0, planning_steps, c->fs_size > 0, &cur, &a)) return RTOC_ERR_BAD_ARG;
  const int B = c->batch;
  HIP_TRY(c->d_fs_fk.reserve((size_t)B * FS_FK_DOUBLES));   // scratch: a clone starts without it
  // the biped walk reads the frames' rotations, behind the centre of mass (which its plan() does not read)
  double* const fk_R = biped(c) ? c->d_fs_fk.p + (size_t)B * 9 : nullptr;
  int rc = biped(c) ? launch_frame_positions(c, c->d_fs_fk.p, nullptr, fk_R)
                    : launch_frame_positions(c, c->d_fs_fk.p, c->d_fs_fk.p + (size_t)B * 12);
  if (rc) return rc;
  a.x0 = c->d_x0.p, a.feet = c->d_fs_fk.p, a.feet_R = fk_R, a.cmd = c->d_fs_cmd.p, a.state = c->d_fs_state.p, a.plan = c->d_fs_plan.p;
  a.batch = B, a.nq = c->h_model->m.nq, a.nx = c->h_model->m.nq + c->h_model->m.nv;
  a.raibert = c->fs_shared.mode == RTOC_FOOT_STEP_RAIBERT;
  a.t = t;
  a.period = GAITS[c->fs_shared.gait].periods * (c->fs_shared.swing_time + c->fs_shared.stance_time);   // :77-79 (of every gait)
  a.min_period = 0.1 * a.period, a.gain = c->fs_shared.gain;
  if (biped(c))
    hipLaunchKernelGGL(biped_walk_plan_kernel, dim3((unsigned)((B + 31) / 32)), dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(foot_step_plan_kernel, dim3((unsigned)((B + 15) / 16)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->fs_current_step = cur, c->fs_size = a.nloop + 1;
  return RTOC_OK;
}

int rtoc_foot_step_plan_get(rtoc_ctx* c, double* positions, double* com, double* R, double* step_length, int* ok, int count, int* size,
                            int* current_step) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!c->fs_on || !c->fs_init || !c->d_fs_plan.p) return RTOC_ERR_NOT_READY;
  if (size) *size = c->fs_size;
  if (current_step) *current_step = c->fs_current_step;
  const size_t B = c->batch, ns = c->fs_size;
  // where the plan keeps what, by the feet: four point feet's positions are [4][3]; two surfaces' 24 doubles are contactPositions(step)[2][3]
  // and contactSurfaces(step)[2][9] behind them, adjacent in the plan too
  const bool two = biped(c);
  const size_t slots = plan_slots(c);
  const int npos = two ? 24 : 12, at_pos = two ? FS_BIPED_POS : FS_PLAN_POS, at_com = two ? FS_BIPED_COM : FS_PLAN_COM, at_R = two ? FS_BIPED_R : FS_PLAN_R;
  static_assert(FS_BIPED_SURF == FS_BIPED_POS + 6, "translations and rotations are read back as one run");
  std::vector<double> h(ns * slots * B), sl(3 * B);
  if (ns) HIP_TRY(hipMemcpyAsync(h.data(), c->d_fs_plan.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  // the length in force: the planner state's; a jump has none but its command, jump_length_
  const double* const sl_src = jump(c) ? c->d_fs_cmd.p + (size_t)FS_CMD_STEP * B : c->d_fs_state.p + (size_t)FS_ST_STEP * B;
  HIP_TRY(hipMemcpyAsync(sl.data(), sl_src, sizeof(double) * 3 * B, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < (size_t)count; ++b) {
    bool fin = true;
    for (size_t s = 0; s < ns; ++s) {
      const double* const src = h.data() + s * slots * B + b;
      for (size_t k = 0; k < slots; ++k) fin = fin && std::isfinite(src[k * B]);
      for (int k = 0; positions && k < npos; ++k) positions[(b * ns + s) * npos + k] = src[(size_t)(at_pos + k) * B];
      for (int k = 0; com && k < 3; ++k) com[(b * ns + s) * 3 + k] = src[(size_t)(at_com + k) * B];
      for (int k = 0; R && k < 9; ++k) R[(b * ns + s) * 9 + k] = src[(size_t)(at_R + k) * B];
    }
    for (int k = 0; step_length && k < 3; ++k) step_length[b * 3 + k] = sl[(size_t)k * B + b];
    if (ok) ok[b] = fin ? 1 : 0;
  }
  return RTOC_OK;
}

// the phases of the grid points (and the masks of the phases behind them) where the kernels read them
static int upload_phases(rtoc_ctx* c, const int* phase, int nstages, const unsigned* masks, int nphases) {
  HIP_TRY(c->d_fs_phase.reserve((size_t)c->max_stages + FS_MAX_STEPS));
  HIP_TRY(hipMemcpyAsync(c->d_fs_phase.p, phase, sizeof(int) * nstages, hipMemcpyHostToDevice, c->stream));
  if (masks) HIP_TRY(hipMemcpyAsync(c->d_fs_phase.p + c->max_stages, masks, sizeof(unsigned) * nphases, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // (pageable sources of the caller)
  return RTOC_OK;
}
static unsigned blocks_for(size_t total) { return (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

int rtoc_foot_step_place(rtoc_ctx* c, const int* phase_of_grid_point, int nstages) {
  CHECK_READY(c);
  if (!phase_of_grid_point) return RTOC_ERR_BAD_ARG;
  if (!c->fs_on || !c->fs_init || c->fs_size < 2 || !c->d_fs_plan.p) return RTOC_ERR_NOT_READY;
  int rc = placements_ready(c);
  if (rc) return rc;
  const bool two = biped(c);
  if (nstages != c->nstages || !(two ? two_surface_feet(c) : four_point_feet(c))) return RTOC_ERR_BAD_ARG;
  for (int i = 0; i < nstages; ++i)
    if (phase_of_grid_point[i] < 0 || phase_of_grid_point[i] > c->fs_size - 2) return RTOC_ERR_BAD_ARG;
  rc = upload_phases(c, phase_of_grid_point, nstages, nullptr, 0);
  if (rc) return rc;
  rc = placements_per_instance(c, two);   // contact surfaces: a rotation table too, as rtoc_hold_contact_placements has it
  if (rc) return rc;
  auto a = view_args<FsPlaceArgs>(c);
  a.plan = c->d_fs_plan.p, a.phase = c->d_fs_phase.p, a.tab_pos = c->cpos.rows(), a.tab_rot = two ? c->crot.rows() : nullptr;
  if (two)
    hipLaunchKernelGGL(foot_step_place_kernel<2>, dim3(blocks_for((size_t)c->batch * nstages * 24)), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(foot_step_place_kernel<4>, dim3(blocks_for((size_t)c->batch * nstages * 12)), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->vals_fresh = 0;   // the contact rows of the values pre-pass belong to the previous placements
  return RTOC_OK;
}

// The jump's configuration reference: the q_ref of MPCJump::init (mpc_jump.cpp:141-145) on every grid row.  It does not depend on
// the grid times, so a grid with switching-time optimisation is served and rtoc_set_grid_times is not needed
static int jump_refs(rtoc_ctx* c, const rtoc_foot_step_ref_params* r, int nstages) {
  if (!c->fs_init || !c->h_model || !c->d_fs_qref.p) return RTOC_ERR_NOT_READY;
  if (nstages != c->nstages || !r->configuration || r->com_term >= 0 || c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k)
    if (r->foot_term[k] >= 0) return RTOC_ERR_BAD_ARG;   // MPCJump has no swing-foot or CoM reference
  const size_t nq = c->h_model->m.nq;
  HIP_TRY(stage_rows(c, c->qtab, nq, 1));
  HIP_TRY(stage_rows(c, c->qtab_active, 1, 1));
  JumpRefsArgs a{};
  a.qref = c->d_fs_qref.p, a.qtab = c->qtab.target(), a.qtab_active = c->qtab_active.target();
  a.batch = c->batch, a.nstages = nstages, a.nq = (int)nq;
  hipLaunchKernelGGL(jump_refs_kernel, dim3(blocks_for((size_t)c->batch * nstages * nq)), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  commit_rows(c, c->qtab, 1), commit_rows(c, c->qtab_active, 1);
  return RTOC_OK;
}

int rtoc_foot_step_refs(rtoc_ctx* c, const rtoc_foot_step_ref_params* r, const int* phase_of_grid_point, const unsigned* phase_masks,
                        int nphases, int nstages) {
  CHECK_READY(c);
  if (r && c->fs_on && jump(c)) return jump_refs(c, r, nstages);
  if (!r || !phase_of_grid_point || !phase_masks) return RTOC_ERR_BAD_ARG;
  if (c->sto_on) return RTOC_ERR_BAD_ARG;   // every instance its own grid times: out of scope
  if (!c->fs_on || !c->fs_init || c->fs_size < 1 || !c->d_fs_q0.p || !c->d_fs_plan.p) return RTOC_ERR_NOT_READY;
  if (nstages != c->nstages || nphases < 1 || nphases > FS_MAX_STEPS) return RTOC_ERR_BAD_ARG;
  if ((int)c->h_gt.size() != c->nstages || !c->d_gt.p) return RTOC_ERR_NOT_READY;   // rtoc_set_grid_times
  // ---- the feet of the gait: a biped has no third and fourth swing-foot reference, and no mask bit for them ----
  const int nf = plan_feet(c);
  const unsigned full = nf == 2 ? 0x3u : 0xFu;
  for (int k = nf; k < 4; ++k)
    if (r->foot_term[k] >= 0) return RTOC_ERR_BAD_ARG;
  for (int k = 0; nf == 2 && k < nphases; ++k)
    if (phase_masks[k] & ~full) return RTOC_ERR_BAD_ARG;
  // ---- the six references as the kernel takes them; the arguments the reference's constructors refuse ----
  FsRefsArgs a{};
  int term_of[5];
  unsigned named = 0;
  for (int k = 0; k < 5; ++k) {
    const int term = k < 4 ? r->foot_term[k] : r->com_term;
    term_of[k] = term;
    if (term < 0) continue;
    if (term >= c->ntasks || !((c->h_task_table >> term) & 1u) || ((named >> term) & 1u)) return RTOC_ERR_BAD_ARG;
    if (!(((k < 4 ? c->h_task_3d : c->h_task_com) >> term) & 1u)) return RTOC_ERR_BAD_ARG;   // a foot: TaskSpace3DCost; the CoM: CoMCost
    named |= 1u << term;
    FsPeriod& p = a.per[k];
    p.on = 1;
    if (k < 4) {
      p.t0 = r->swing_start_time[k], p.period_active = r->period_swing[k], p.period_inactive = r->period_stance[k];
      p.height = r->swing_height[k], p.nph = r->swing_num_phases_in_period[k];
      if (!(p.height >= 0.0) || !(p.period_active > 0.0) || !(p.period_inactive > 0.0)) return RTOC_ERR_BAD_ARG;
    } else {
      p.t0 = r->com_swing_start_time, p.period_active = r->com_period_active, p.period_inactive = r->com_period_inactive;
      p.nph = r->com_num_phases_in_period;
      if (!(p.period_active >= 0.0) || !(p.period_inactive >= 0.0)) return RTOC_ERR_BAD_ARG;
    }
    if (p.nph < 1 || !std::isfinite(p.t0)) return RTOC_ERR_BAD_ARG;
  }
  if (r->configuration) {
    FsPeriod& p = a.per[5];
    p.on = 1, p.t0 = r->q_swing_start_time, p.period_active = r->q_period_active, p.period_inactive = r->q_period_inactive;
    p.nph = r->q_num_phases_in_period;
    if (!(p.period_active >= 0.0) || !(p.period_inactive >= 0.0) || p.nph < 1 || !std::isfinite(p.t0)) return RTOC_ERR_BAD_ARG;
    if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  }
  // ---- every plan step a grid point reads lies inside the plan ----
  for (int i = 0; i < nstages; ++i) {
    const int ph = phase_of_grid_point[i];
    if (ph < 0 || ph >= nphases || ph >= c->fs_size) return RTOC_ERR_BAD_ARG;
    const unsigned mask = phase_masks[ph];
    for (int k = 0; k < 6; ++k) {
      const FsPeriod& p = a.per[k];
      if (!p.on) continue;
      const bool reads_ahead = c->h_gt[i] > p.t0 && (k < 4 ? !((mask >> k) & 1u) : (mask & full) != full);
      if (reads_ahead && ph + p.nph >= c->fs_size) return RTOC_ERR_BAD_ARG;
    }
  }
  // ---- the per-instance tables the kernel writes: all of them staged first ----
  for (int k = 0; k < 5; ++k)
    if (term_of[k] >= 0) HIP_TRY(stage_rows(c, c->reftab[term_of[k]], 1, 1));
  const size_t nq = c->h_model->m.nq;
  if (r->configuration) HIP_TRY(stage_rows(c, c->qtab, nq, 1));
  if (r->configuration) HIP_TRY(stage_rows(c, c->qtab_active, 1, 1));
  int rc = upload_phases(c, phase_of_grid_point, nstages, phase_masks, nphases);
  if (rc) return rc;
  a.plan = c->d_fs_plan.p, a.q0 = c->d_fs_q0.p, a.t = c->d_gt.p;
  a.phase = c->d_fs_phase.p, a.masks = (const unsigned*)(c->d_fs_phase.p + c->max_stages);
  for (int k = 0; k < 5; ++k) a.tab[k] = term_of[k] >= 0 ? c->reftab[term_of[k]].target() : nullptr;
  a.qtab = r->configuration ? c->qtab.target() : nullptr, a.qtab_active = r->configuration ? c->qtab_active.target() : nullptr;
  a.batch = c->batch, a.nstages = nstages, a.nq = (int)nq;
  const size_t most = (size_t)c->batch * nstages * (nq > (size_t)FS_ENTRY_WORDS ? nq : (size_t)FS_ENTRY_WORDS);
  if (nf == 2)
    hipLaunchKernelGGL(foot_step_refs_kernel<2>, dim3(blocks_for(most), 6), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(foot_step_refs_kernel<4>, dim3(blocks_for(most), 6), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  // the tables are per instance and belong to the grid in force
  for (int k = 0; k < 5; ++k)
    if (term_of[k] >= 0) commit_rows(c, c->reftab[term_of[k]], 1);
  if (r->configuration) commit_rows(c, c->qtab, 1), commit_rows(c, c->qtab_active, 1);
  return RTOC_OK;
}
