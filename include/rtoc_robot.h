/* rtoc_robot.h -- rigid-body model table + batched linearisation of the contact / impact dynamics.
 *
 * What the reference's Robot gets from Pinocchio (include/robotoc/robot/robot.hxx:524-583 RNEA / RNEADerivatives /
 * RNEAImpact / RNEAImpactDerivatives, :291-360 Baumgarte residual and derivatives, src/robot/point_contact.cpp,
 * include/robotoc/robot/point_contact.hxx:14-140) restated for the device: one model table per context, every
 * (instance, grid point) of RTOC_BUF_SOL linearised in one launch into the pre-condensation fields of RTOC_BUF_CDD.
 * Pinocchio (3rd party, not vendored in the reference tree; robotoc's CMake asks for pinocchio >= 2.x) is absent here:
 * the algorithm is Featherstone's recursive Newton-Euler in body coordinates ([linear; angular] spatial vectors,
 * Pinocchio's convention), its partial derivatives by forward-mode differentiation of that recursion along the
 * 3 nv tangent directions (q on the configuration manifold, v, a) -- parity with Pinocchio itself is UNPINNED
 * (DESIGN.md); the derivatives are validated against finite differences of the CPU restatement.
 *
 * Conventions (Pinocchio's): q = [x y z qx qy qz qw, joint angles] for a floating base, v = [linear; angular] of the
 * base in the BASE frame followed by joint rates; joints in depth-first order, children in name order (what
 * pinocchio::urdf::buildModel produces; tools/urdf_to_model.py restates it).  3x3 matrices row-major.
 */
#ifndef RTOC_ROBOT_H_
#define RTOC_ROBOT_H_

#include "rtoc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTOC_MAX_JOINTS 48
#define RTOC_MAX_CONTACTS 8

enum rtoc_joint_type { RTOC_JOINT_FREE_FLYER = 0, RTOC_JOINT_REVOLUTE = 1 };
enum rtoc_contact_type { RTOC_CONTACT_POINT = 0, RTOC_CONTACT_SURFACE = 1 }; /* ContactType::PointContact / SurfaceContact */

typedef struct rtoc_robot_model {
  int njoints, nq, nv, ncontacts;
  int parent[RTOC_MAX_JOINTS];             /* index of the parent joint, -1: the world; parent[i] < i                 */
  int type[RTOC_MAX_JOINTS];               /* rtoc_joint_type; a free flyer only as joint 0                           */
  int idx_q[RTOC_MAX_JOINTS];              /* first entry of the joint in q / v                                       */
  int idx_v[RTOC_MAX_JOINTS];
  double placement_R[RTOC_MAX_JOINTS][9];  /* joint frame in the parent joint's frame (pinocchio jointPlacements)     */
  double placement_p[RTOC_MAX_JOINTS][3];
  double axis[RTOC_MAX_JOINTS][3];         /* revolute: unit axis in the joint frame                                  */
  double mass[RTOC_MAX_JOINTS];            /* body of the joint (links behind fixed joints welded in)                 */
  double com[RTOC_MAX_JOINTS][3];          /* centre of mass in the joint frame                                       */
  double inertia[RTOC_MAX_JOINTS][9];      /* rotational inertia about the centre of mass, joint-frame axes           */
  int contact_type[RTOC_MAX_CONTACTS];     /* rtoc_contact_type: 3 rows (force) or 6 rows (wrench); points first, as
                                            * the reference stacks them (robot.hxx:291-320)                           */
  int contact_parent[RTOC_MAX_CONTACTS];   /* joint the contact frame is attached to (PointContact / SurfaceContact)  */
  double contact_R[RTOC_MAX_CONTACTS][9];  /* contact frame in that joint's frame (model.frames[id].placement)        */
  double contact_p[RTOC_MAX_CONTACTS][3];
  double contact_kp[RTOC_MAX_CONTACTS];    /* ContactModelInfo::baumgarte_position_gain / velocity_gain               */
  double contact_kd[RTOC_MAX_CONTACTS];
  double gravity[3];                       /* world frame, (0, 0, -9.81)                                              */
} rtoc_robot_model;

/* Copies the table to the device.  RTOC_ERR_BAD_ARG unless nv == dims.nv, nq is nv (fixed base) or nv + 1 (free-flyer
 * root), joints are depth-first ordered, 3 * ncontacts <= dims.nf_max. */
int rtoc_set_robot_model(rtoc_ctx* ctx, const rtoc_robot_model* model);

/* What rtoc_set_robot_model would plan for rtoc_linearize_contact_dynamics' tangent walk, without a context or a device (host
 * arithmetic only): tree levels, LDS slots for forward tangents (= the largest number of branching joints on a root-to-leaf
 * path), tangent directions per pass (RTOC_OPT_LINEARIZE_DOFS_PER_PASS; forced_dofs_per_pass = 0: the library's choice),
 * passes, LDS bytes per wave of the walk behind the values pre-pass, and pass_bodies[p] = bit i set if pass p visits joint i
 * (room for RTOC_MAX_JOINTS + 8 passes; may be NULL).  RTOC_ERR_BAD_ARG for a table rtoc_set_robot_model would refuse on its
 * own grounds (joints not depth first, index maps inconsistent, more LDS than a CU has). */
typedef struct rtoc_linearize_plan {
  int nlevels, nbranch, dofs_per_pass, npass, lds_bytes;
} rtoc_linearize_plan;
int rtoc_robot_model_plan(const rtoc_robot_model* model, int forced_dofs_per_pass, rtoc_linearize_plan* plan,
                          unsigned long long* pass_bodies);

/* Per grid point: bit k of active[i] = contact k is active (ContactStatus::isContactActive; on impact grids:
 * ImpactStatus::isImpactActive), positions[i][k][0..2] = ContactStatus::contactPosition(k) (world frame; NULL: zeros),
 * rotations[i][k][0..8] = ContactStatus::contactRotation(k) (row-major; only read for surface contacts; NULL: identity).
 * The rows of the active contacts (3 per point, 6 per surface contact) must add up to the grid's dimf.
 * The placements given here are SHARED by the batch, and a per-instance table ends with this call; every instance on its own
 * footholds: see rtoc_set_contact_placements / rtoc_hold_contact_placements below. */
int rtoc_set_contact_schedule(rtoc_ctx* ctx, const unsigned* active, const double* positions, const double* rotations);

/* ---- contact placements of every instance: each OCP of a batch on its own footholds ----
 * rtoc_set_contact_placements replaces the placements of the schedule in force and keeps its `active` masks.
 * per_instance = 0: positions[nstages][ncontacts][3], rotations[nstages][ncontacts][9], as for rtoc_set_contact_schedule;
 * per_instance = 1: the same with a leading [batch].  rotations = NULL: identity; positions = NULL: zeros.  Every kernel that reads
 * a placement (the Baumgarte rows of rtoc_linearize_contact_dynamics, the switching constraint's impact grid two points ahead, the
 * cone rows in the contact surface's frame; hence rtoc_contact_eval_kkt, rtoc_contact_eval_ocp and the trial evaluations of the
 * line searches) reads the table of its own instance.  Entries of INACTIVE contacts are never read, on the host or on the device
 * (INACTIVE ENTRIES below).  A refused call launches nothing and leaves the table in force: RTOC_ERR_NOT_READY without
 * rtoc_set_robot_model or before a rtoc_set_contact_schedule that belongs to the grid in force (rtoc_set_grid with another grid
 * invalidates the placements with the schedule); RTOC_ERR_BAD_ARG for a non-finite entry of an ACTIVE contact at its grid point,
 * for per_instance outside {0, 1}, for a model without contacts and on a ParNMPC horizon.  rtoc_clone copies the table and its
 * mode; rtoc_set_robot_model ends a per-instance table (it is sized by batch * max_stages * the model's contacts).
 * Not per instance: the `active` masks (the grid's dimf is shared structure), friction coefficients and wrench-cone sizes.
 *
 * rtoc_contact_frame_placements: Robot::updateFrameKinematics + frameRotation / framePosition / CoM of every instance on the
 * device -- world rotation (row-major) and position of every contact frame of the model and the centre of mass, at the q of
 * rtoc_set_initial_state (source = 0; grid_point ignored) or at q of grid point `grid_point` of RTOC_BUF_SOL (source = 1).
 * host_R[count][ncontacts][9], host_p[count][ncontacts][3], host_com[count][3], count <= batch; any of them may be NULL.
 *
 * rtoc_hold_contact_placements: the same kinematics, but the result never leaves the device -- for every instance the placements
 * of the contacts in the bit mask `contacts` are written into grid points [first, last) of the per-instance table: what the
 * reference's foot-step planners do with the feet on the ground (src/mpc/trot_foot_step_planner.cpp:94-98, :138-141), for a batch.
 * A shared table becomes per instance first, every instance starting from the shared values.  Rotations are written for surface
 * contacts only, into the rotation table if there is one; if there is none and the mask holds a surface contact, one is created,
 * identity elsewhere.  An empty mask holds nothing.  RTOC_ERR_BAD_ARG: an empty or out-of-range [first, last), mask bits at or
 * beyond ncontacts, source outside {0, 1}, grid_point outside the grid (source = 1), a ParNMPC horizon; RTOC_ERR_NOT_READY without
 * the model, the schedule of the grid in force, or the source (no initial state / no RTOC_BUF_SOL).
 *
 * rtoc_get_contact_placements: the table as the instances read it -- host_positions[count][nstages][ncontacts][3],
 * host_rotations[count][nstages][ncontacts][9], count <= batch (a shared table repeated, zeros / identities where none was set;
 * either may be NULL) and *per_instance (may be NULL) = the mode in force. */
int rtoc_get_contact_placements(rtoc_ctx* ctx, double* host_positions, double* host_rotations, int count, int* per_instance);
int rtoc_set_contact_placements(rtoc_ctx* ctx, const double* positions, const double* rotations, int per_instance);
int rtoc_contact_frame_placements(rtoc_ctx* ctx, int source, int grid_point, double* host_R, double* host_p, double* host_com,
                                  int count);
int rtoc_hold_contact_placements(rtoc_ctx* ctx, int source, int grid_point, int first, int last, unsigned contacts);

/* ---- TrotFootStepPlanner and the MPC references of every instance on the device ----
 * What MPCTrot::resetContactPlacements does per control tick (src/mpc/mpc_trot.cpp:357-372) for a batch, each instance with its own
 * command: TrotFootStepPlanner::plan (src/mpc/trot_foot_step_planner.cpp) with RaibertHeuristic (src/mpc/raibert_heuristic.cpp) and
 * MovingWindowFilter<2> (include/robotoc/mpc/moving_window_filter.hpp), the placements of every contact phase, and
 * MPCPeriodicSwingFootRef x 4, MPCPeriodicCoMRef, MPCPeriodicConfigurationRef (src/mpc/mpc_periodic_*_ref.cpp).  The plan, the
 * placement table and the reference tables are written on the device and stay there.  The gait wrapper itself (addStep, pop_front,
 * the solve call) stays with the caller: the contact sequence is structure the batch shares.  The crawl, the pace and the flying
 * trot (MPCCrawl, MPCPace, MPCFlyingTrot: their resetContactPlacements is the trot's line for line) plan through the same entry
 * points, chosen by rtoc_foot_step_planner::gait -- THE OTHER GAITS below.  So does BipedWalkFootStepPlanner with what
 * MPCBipedWalk::resetContactPlacements does (src/mpc/mpc_biped_walk.cpp:347-359), on a model of two contact surfaces, whose
 * placements carry rotations -- THE BIPED WALK below -- and JumpFootStepPlanner with what MPCJump::init and
 * MPCJump::resetContactPlacements do (src/mpc/mpc_jump.cpp:141-145, :301-317), on either kind of feet -- THE JUMP below.  Not here:
 * the periodic references on grids with switching-time optimisation, ParNMPC horizons (every entry point below refuses one with RTOC_ERR_BAD_ARG).
 *
 * rtoc_set_foot_step_planner: setGaitPattern (mode RTOC_FOOT_STEP_FIXED: step_length, step_yaw, enable_stance_phase) or
 * setRaibertGaitPattern (RTOC_FOOT_STEP_RAIBERT: vcom_cmd, yaw_rate_cmd, swing_time, stance_time, gain; enable_stance_phase is
 * stance_time > 0 as in :86 and the member is ignored), p[1] for the batch (per_instance = 0) or p[batch].  step_length, step_yaw,
 * vcom_cmd and yaw_rate_cmd are each instance's own; gait, mode, projection, swing_time, stance_time, gain and enable_stance_phase decide
 * the step-case sequence, which is shared structure like the grid, and must agree across the instances.  RTOC_ERR_BAD_ARG: they do
 * not; an unknown gait, mode or projection; enable_stance_phase outside {0, 1}; per_instance outside {0, 1}; in Raibert mode the checks of
 * the reference's setters (:63-76, raibert_heuristic.cpp:38-47): swing_time <= 0, stance_time < 0, gain <= 0; a model that has not
 * exactly four contacts, all of them point contacts, in the reference's order LF, LH, RF, RH = contacts 0..3 (RTOC_GAIT_BIPED_WALK:
 * that has not exactly two contacts, both contact surfaces; it is refused on four point feet as they are on two surfaces).  RTOC_ERR_NOT_READY
 * without rtoc_set_robot_model.  p = NULL removes the planner with its state and plan (rtoc_foot_step_planner_init again after the next one is set).  A refused call leaves the planner in force.  Setting a planner keeps
 * the state of rtoc_foot_step_planner_init (the reference's setters do not touch it either).
 *
 * BASE-ROTATION PROJECTION.  rotation::ProjectRotationMatrix(R, Z) of the reference (include/robotoc/utils/rotation.hpp:103-111)
 * divides R by R00^2 + R01 + R01, not by the norm of the row.  For a pure yaw theta that is cos^2 theta - 2 sin theta: 1 at
 * theta = 0, zero at sin theta = sqrt(2) - 1 (theta = 0.427 rad), where the planner's rotation and with it the plan become non-finite.  Parity with the
 * reference is this project's definition of correct: RTOC_PROJECT_AS_REFERENCE (0, the default of a zeroed struct) reproduces that
 * arithmetic literally; RTOC_PROJECT_YAW is the rotation about z by atan2(R10, R00).  An instance whose plan went non-finite shows
 * in ok[] of rtoc_foot_step_plan_get; no status bit is raised.
 *
 * rtoc_foot_step_planner_init: TrotFootStepPlanner::init(q) (:91-106) of every instance at the q of rtoc_set_initial_state -- the
 * projected base rotation, com_to_contact_position_local_[4], com_ref_[0], a cleared filter, and a copy of q (the configuration
 * reference starts from it); current_step_ = 0 is kept once, on the host.  The plan's size is 0 afterwards.
 *
 * rtoc_foot_step_plan: plan(t, q, v, contact_status, planning_steps) (:125-284) of every instance from the q, v of
 * rtoc_set_initial_state as it stands now.  contact_status0: the active contacts of the first phase, 0b1111, 0b1001 (LF + RH) or
 * 0b0110 (LH + RF) -- the reference returns false otherwise, here RTOC_ERR_BAD_ARG and nothing is launched; planning_steps in
 * [0, RTOC_MAX_PLAN_STEPS], else RTOC_ERR_BAD_ARG.  The plan has planning_steps + 2 steps: contactPositions(step)[4][3], CoM(step)[3],
 * R(step)[9] per instance.  Every instance's planner state (R_.front(), the filter) advances; the host's current_step_ advances by
 * the reference's rules.  RTOC_ERR_NOT_READY without a planner, its init or an initial state.
 *
 * THE OTHER GAITS (rtoc_foot_step_planner::gait; line numbers: src/mpc/{pace,crawl,flying_trot}_foot_step_planner.cpp).  Init, the
 * filter, the heuristic, the plan's layout, place and refs are the trot's.  A contact status is matched exactly against the
 * gait's own set; any other, another gait's legal ones included, is RTOC_ERR_BAD_ARG and nothing is launched.
 *   RTOC_GAIT_PACE: the trot with the pairs (LF, LH) = 0b0011 and (RF, RH) = 0b1100.  Statuses 0b1111, 0b0011, 0b1100.  With the
 *   stance phase 0b0011 is the step with current_step_ % 4 == 1 and 0b1100 the one with % 4 == 3, without it % 2 == 1 and
 *   % 2 == 0 (:160-201); feet 2 and 3 move first (:216-226).  Raibert period 2 (swing_time + stance_time) (:77).
 *   RTOC_GAIT_CRAWL: three feet stand.  Statuses 0b1111, 0b0111 (RH swings), 0b1011 (RF), 0b1101 (LH), 0b1110 (LF): the steps with
 *   current_step_ % 8 == 1, 3, 5, 7 with the stance phase, % 4 == 1, 2, 3, 0 without (:143-253).  The CoM is the sum over the three
 *   stance feet divided by 3.0, the swing foot is placed at com + R (local - 0.5 step_length).  The loop (:260-359) is incremental:
 *   a moving foot advances by p += s R step_length and the CoM by c R step_length with s = 1, c = 0.25, except on step == 1 and
 *   step == 3 (with the stance phase; step == 2 without), where s = 0.5 and c = 0.125 without the heuristic, 0.25 with it.  Those
 *   two steps are tested on `step` alone, not on current_step_ == 0, as in the reference.  With the stance phase nothing moves or
 *   turns on even steps.  Raibert period 4 (swing_time + stance_time) (:77); the yaw per step is yaw_rate_cmd (swing_time +
 *   stance_time).
 *   RTOC_GAIT_FLYING_TROT: statuses 0b1111 (current_step_ = 0, :140), 0b1001 (advances and turns unless current_step_ % 4 == 1),
 *   0b0110 (unless % 4 == 3) and 0b0000, the flight (:176-183): current_step_ goes to the next even number without a rotation, the
 *   CoM is the previous plan's CoM(0) and the footholds are the previous plan's contactPositions(0).  A flight as the first plan
 *   after rtoc_foot_step_planner_init is RTOC_ERR_BAD_ARG (the reference reads an empty vector there).  Loop (:190-230): nothing
 *   moves on step == 0, on current_step_ == 0 && step == 1, or on odd step % 4; current_step_ == 0 && step == 2 moves feet 1 and 2
 *   with the first-step scale (0.5 with the heuristic, 0.25 without); % 4 == 2 moves feet 1 and 2, % 4 == 0 feet 0 and 3, placed
 *   absolutely as in the trot.  :231-233 push one more copy of the last step: the plan has planning_steps + 3 steps, and
 *   planning_steps is limited to [0, RTOC_MAX_PLAN_STEPS - 1] so that it fits the arrays of rtoc_foot_step_plan_get.  There is no
 *   stance-phase option (enable_stance_phase is ignored).  In Raibert mode swing_time carries flying_time and stance_time <= 0 is
 *   refused by rtoc_set_foot_step_planner (:66); period 2 (flying_time + stance_time).
 *
 * THE BIPED WALK (gait = RTOC_GAIT_BIPED_WALK; line numbers: src/mpc/biped_walk_foot_step_planner.cpp).  The model has exactly two
 * contacts, both RTOC_CONTACT_SURFACE: contact 0 is the left foot and contact 1 the right one (surfaceContactFrames()[0], [1]).
 * enable_stance_phase carries enable_double_support_phase and stance_time double_support_time (checks :66-74, period
 * 2 (swing_time + double_support_time), step yaw yaw_rate_cmd (swing_time + double_support_time), :75-84).
 *   init (:89-108): the projected base rotation (BASE-ROTATION PROJECTION applies as above), left_to_right_leg_distance_ and
 *   foot_height_to_com_height_, the feet measured relative to q.head<3>(), the base -- not to the centre of mass --, a cleared
 *   filter and the copy of q.
 *   plan (:111-277): statuses 0b11, 0b01 (the left foot stands, the right one swings) and 0b10; any other is RTOC_ERR_BAD_ARG and
 *   nothing is launched.  0b11: current_step_ to the next even number with double support, to 0 without.  0b01 advances and turns
 *   unless current_step_ % 4 == 1 (% 2 == 1 without double support), 0b10 unless % 4 == 3 (% 2 == 0).  Step 0: both feet from this
 *   tick's kinematics with their full frame rotations; in single support the swing foot is placed at
 *   R (local_stance - 0.5 R_yaw^T step_length -/+ distance e_y) + q.head<3>() with rotation R, local_stance measured in R_.front()
 *   before the turn; the CoM is the midpoint of the two translations plus the stored height.  The loop is incremental: the moving
 *   foot advances by p += s R step_length and takes the rotation R, the CoM by c R step_length, s = 1, c = 0.5; the right foot
 *   moves on step % 4 == 1 and the left on % 4 == 3 with double support (nothing moves or turns on even steps), on odd and even
 *   steps without; the first step of all (current_step_ == 0 && step == 1) has s = 0.5, and c = 0.5 with the heuristic, 0.25
 *   without.  The plan has planning_steps + 2 steps: contactPositions(step)[2][3], contactSurfaces(step)[2][9], CoM(step)[3],
 *   R(step)[9] per instance.
 *   rtoc_foot_step_plan_get: `positions` holds 24 doubles per (instance, step), the [2][3] translations and then the [2][9]
 *   rotations, row-major; the caller's array holds (RTOC_MAX_PLAN_STEPS + 2) * 24 doubles per instance; ok[] covers the rotations.
 *   rtoc_foot_step_place: contactPlacements(phase + 1) of both feet -- the translations into the per-instance position table, the
 *   rotations into the per-instance rotation table, which is created, or converted from a shared one, exactly as
 *   rtoc_hold_contact_placements does it.
 *   rtoc_foot_step_refs: foot_term[0..1] are the two feet; foot_term[2..3] must be negative.  "Some contact is inactive"
 *   (mpc_periodic_com_ref.cpp:69-79, the configuration reference alike) is judged against the model's two contacts: 0b11 is every
 *   contact.  A bit at or beyond 2 in any of phase_masks[nphases] is RTOC_ERR_BAD_ARG.
 *
 * THE JUMP (gait = RTOC_GAIT_JUMP; line numbers: src/mpc/jump_foot_step_planner.cpp, and src/mpc/mpc_jump.cpp where named).  The
 * model has exactly four point contacts (the quadruped form) or exactly two contact surfaces (is_biped_, :29-31); the feet choose
 * the plan's layout: the quadrupeds' for four, the biped walk's, with rotations, for two.
 *   rtoc_set_foot_step_planner: setJumpPattern(jump_length, step_yaw) (:43-49) -- step_length[3] carries jump_length and step_yaw
 *   the yaw, each instance's own.  mode must be RTOC_FOOT_STEP_FIXED: the reference has no Raibert form of a jump, and
 *   RTOC_FOOT_STEP_RAIBERT is RTOC_ERR_BAD_ARG.  projection applies as above; enable_stance_phase must be 0 or 1 and is ignored, as
 *   are swing_time, stance_time and gain.  Going to or from this gait ends the state of rtoc_foot_step_planner_init.
 *   rtoc_foot_step_planner_init: init(q) (:68-124).  R = the projected base rotation; local_k = (R^T R_k, R^T (p_k - q.head<3>()))
 *   of every contact frame; R_goal = R_yaw R; q_goal = q with head<3>() += R_yaw jump_length and the quaternion
 *   Quaterniond(R_goal).coeffs() (Eigen's conversion, not normalised); goal_k = (R_goal Rl_k, q.head<3>() + R_goal tl_k + R_yaw
 *   jump_length).  The plan holds three steps: steps 0 and 1 are the placements the kinematics measured at q, step 2 the goal; on
 *   four point feet every rotation is the identity (:99-105); CoM(0) = CoM(1) is the centre of mass at q and CoM(2) the one at
 *   q_goal (a second kinematics pass); R(0) = R(1) = R, R(2) = R_goal.  Init also stores the q_ref of MPCJump::init
 *   (mpc_jump.cpp:141-145) per instance: q with head<3>() += CoM(2) - CoM(0) and the quaternion Quaterniond(R(2)).coeffs().
 *   current_step_ = 0 and the plan's size is 3 afterwards (every other gait: 0): MPCJump::init reads CoM(2) and R(2) before it plans.
 *   rtoc_foot_step_plan: plan() (:127-170).  t, v and planning_steps are not read (planning_steps keeps its range check).
 *   contact_status0 != 0 (hasActiveContacts): current_step_ 1 becomes 2; step 1 takes this tick's kinematics at q -- the full
 *   frame placement on two surfaces, the translation alone on four point feet --, step 0 becomes a copy of step 1, step 2, if still
 *   there, is untouched.  contact_status0 == 0: at current_step_ == 0 it becomes 1, step 1 takes placements, CoM and R of step 2
 *   and the plan shrinks to size 2; at any other current_step_ nothing changes.  A bit at or beyond the model's contacts is
 *   RTOC_ERR_BAD_ARG and nothing is launched.
 *   rtoc_foot_step_plan_get: the layout of the feet, as above; step_length returns jump_length; size is 3 or 2.
 *   rtoc_foot_step_place: unchanged -- grid point i gets step phase_of_grid_point[i] + 1.  MPCJump::resetContactPlacements
 *   (mpc_jump.cpp:301-317) maps phase 0 to step 1 and phases 1 and 2 to step 2 before the flight, every phase to step 1 after it:
 *   the caller passes min(phase, size - 2).  Grids with switching-time optimisation are served.
 *   rtoc_foot_step_refs: the configuration reference alone.  r->configuration must be non-zero, every foot_term and com_term
 *   negative, else RTOC_ERR_BAD_ARG; dims.np must be 6; nstages the grid's.  phase_of_grid_point and phase_masks may be NULL;
 *   nphases and the periods are not read.  Every grid row of the per-instance q_ref table receives the stored q_ref, active
 *   everywhere.  The reference does not depend on time: for this gait alone the call serves a grid with switching-time
 *   optimisation, and needs no rtoc_set_grid_times.  RTOC_ERR_NOT_READY before rtoc_foot_step_planner_init.
 *   The receding horizon of MPCJump::updateSolution (mpc_jump.cpp:206-222: it pops an event and re-sizes the problem) stays with the
 *   caller, as the gait wrappers above do.
 *   Where this departs from the reference.  (1) init never clears com_ref_ there (:115-118 push onto whatever is there), so a
 *   planner initialised twice keeps answering with the first init's centres of mass; here a second init starts over.
 *   (2) contact_position_ref_ and contact_surface_ref_ hold feet 0 and 1 alone there (:110-113, :163-166), for quadrupeds as well;
 *   here contactPositions and contactSurfaces are the two parts of contactPlacements for every foot (MPCJump reads
 *   contactPlacements).  (3) The reference takes any robot with at least four point contacts or at least two surfaces; here the
 *   counts are exact, as for the other gaits.
 *
 * rtoc_foot_step_plan_get: the plan of the first count <= batch instances -- positions[count][size][4][3], com[count][size][3],
 * R[count][size][9] (row-major), step_length[count][3] (the length in force; Raibert mode: what the heuristic planned),
 * ok[count] (1 iff every number of that instance's plan is finite), *size, *current_step.  Any pointer may be NULL; the arrays must
 * hold RTOC_MAX_PLAN_STEPS + 2 steps unless the caller knows the size.
 *
 * rtoc_foot_step_place: the loop of resetContactPlacements (mpc_trot.cpp:361-365) -- grid point i of instance b gets
 * contactPositions(phase_of_grid_point[i] + 1) of b's plan, all four contacts, as the reference writes them.  phase_of_grid_point:
 * GridInfo::phase relative to the first grid point.  The target is the per-instance placement table; a shared one is converted
 * first, exactly as rtoc_hold_contact_placements does.  RTOC_ERR_BAD_ARG: nstages is not the grid's, a phase outside [0, size - 2];
 * RTOC_ERR_NOT_READY without a plan or the schedule of the grid in force.
 *
 * rtoc_foot_step_refs: the three references at every (instance, grid point), written where the cost kernels read them: the
 * per-instance forms of the tables of rtoc_set_task_ref_table and rtoc_set_configuration_ref_table (tables that were shared become
 * per instance).  phase_masks[nphases]: the active contacts of every contact phase (what setSwingFootRef / setCoMRef keep as
 * is_contact_active_ / has_inactive_contacts_).  Swing foot k (r->foot_term[k] >= 0: the index of its RTOC_TASK_FRAME_3D term):
 * isActive = t > swing_start_time and the foot is in the air; then cycle = floor((t - start) / (period_swing + period_stance)),
 * rate = (t - start - cycle period) / period_swing, p = (1 - rate) contactPositions(phase)[k] + rate contactPositions(phase +
 * num_phases_in_period)[k] with the swing height added (mpc_periodic_swing_foot_ref.cpp:90-110); the reference leaves an inactive
 * entry as it was, here it is contactPositions(phase)[k] with active = 0.  CoM (r->com_term >= 0, a RTOC_TASK_COM term): the same
 * blend of CoM(phase) and CoM(phase + num_phases_in_period) where t > swing_start_time and some foot is in the air, else the else
 * branch of updateRef, CoM(phase), with active = 0 (mpc_periodic_com_ref.cpp:90-110).  Configuration (r->configuration != 0): q of
 * rtoc_foot_step_planner_init with the quaternion replaced by Quaterniond(R(phase)).slerp(rate, Quaterniond(R(phase +
 * num_phases_in_period))) under the same condition, else Quaterniond(R(phase)); active everywhere
 * (mpc_periodic_configuration_ref.cpp:92-115); Eigen's matrix-to-quaternion conversion and Eigen's slerp with its sign flip and
 * near-parallel branch.  Entries are written whole: R = identity, pad = 0.  Times: rtoc_set_grid_times.
 * RTOC_ERR_BAD_ARG: nstages is not the grid's; a phase outside [0, nphases) or at or beyond the plan's size; phase +
 * num_phases_in_period at or beyond the plan's size at a grid point that reads it; a term outside the terms set, named twice, whose
 * ref_kind is not RTOC_REF_TABLE, or whose kind is not RTOC_TASK_FRAME_3D (a foot) / RTOC_TASK_COM (the CoM) in every instance; nphases outside [1, RTOC_MAX_PLAN_STEPS + 2]; the arguments the reference's constructors refuse (swing_height < 0, period_swing or
 * period_stance <= 0, a negative period of the CoM or configuration reference, num_phases_in_period < 1); a grid with switching-time
 * optimisation (per-instance times are out of scope).  RTOC_ERR_NOT_READY without a plan or the grid times.
 *
 * rtoc_get_task_ref_table / rtoc_get_configuration_ref_table: the tables as the instances read them, entries[count][nstages],
 * q_ref[count][nstages][nq] and active[count][nstages], count <= batch (a shared table repeated; any pointer may be NULL) and
 * *per_instance = the mode in force.  RTOC_ERR_NOT_READY where no table is set for the grid in force.
 *
 * rtoc_set_grid leaves the planner, its state and the plan alone (the plan does not depend on the grid), but forgets the tables:
 * place and refs again (the jump's stored q_ref stays).  rtoc_set_robot_model ends the planner.  rtoc_clone copies planner, state,
 * plan and the jump's q_goal and q_ref. */
#define RTOC_MAX_PLAN_STEPS 32
#define RTOC_FOOT_STEP_FIXED 0          /* TrotFootStepPlanner::setGaitPattern        */
#define RTOC_FOOT_STEP_RAIBERT 1        /* TrotFootStepPlanner::setRaibertGaitPattern */
#define RTOC_PROJECT_AS_REFERENCE 0     /* BASE-ROTATION PROJECTION above             */
#define RTOC_PROJECT_YAW 1
#define RTOC_GAIT_TROT 0                /* TrotFootStepPlanner                        */
#define RTOC_GAIT_CRAWL 1               /* CrawlFootStepPlanner                       */
#define RTOC_GAIT_PACE 2                /* PaceFootStepPlanner                        */
#define RTOC_GAIT_FLYING_TROT 3         /* FlyingTrotFootStepPlanner                  */
#define RTOC_GAIT_BIPED_WALK 4          /* BipedWalkFootStepPlanner: two contact surfaces */
#define RTOC_GAIT_JUMP 5                /* JumpFootStepPlanner: four point feet or two contact surfaces */
typedef struct rtoc_foot_step_planner {
  int mode;                    /* RTOC_FOOT_STEP_*                                                       */
  int projection;              /* RTOC_PROJECT_*: the reference's ProjectRotationMatrix divides by R00^2 + 2 R01, which is
                                * NOT the row's norm and crosses zero at a yaw of 0.427 rad (see above); 0 keeps it */
  int enable_stance_phase;     /* fixed mode (ignored by the flying trot; the biped walk: enable_double_support_phase) */
  int gait;                    /* RTOC_GAIT_*: 0, the value of a zeroed struct, is the trot              */
  double swing_time, stance_time, gain;   /* Raibert mode (gait timing; shared by the batch)             */
  double step_length[3], step_yaw;        /* fixed mode, per instance (the jump: jump_length, step_yaw)  */
  double vcom_cmd[3], yaw_rate_cmd;       /* Raibert mode, per instance                                  */
} rtoc_foot_step_planner;
typedef struct rtoc_foot_step_ref_params {
  int foot_term[4];            /* index of the RTOC_TASK_FRAME_3D term of LF, LH, RF, RH; negative: left out
                                * (the biped walk: of the left and the right foot; [2..3] negative)        */
  int com_term;                /* index of the RTOC_TASK_COM term; negative: left out                       */
  int configuration;           /* != 0: the configuration reference                                         */
  double swing_height[4], swing_start_time[4], period_swing[4], period_stance[4];   /* MPCPeriodicSwingFootRef */
  int swing_num_phases_in_period[4];
  double com_swing_start_time, com_period_active, com_period_inactive;              /* MPCPeriodicCoMRef */
  int com_num_phases_in_period, pad0;
  double q_swing_start_time, q_period_active, q_period_inactive;                    /* MPCPeriodicConfigurationRef */
  int q_num_phases_in_period, pad1;
} rtoc_foot_step_ref_params;
int rtoc_set_foot_step_planner(rtoc_ctx* ctx, const rtoc_foot_step_planner* p, int per_instance);
int rtoc_foot_step_planner_init(rtoc_ctx* ctx);
int rtoc_foot_step_plan(rtoc_ctx* ctx, double t, unsigned contact_status0, int planning_steps);
int rtoc_foot_step_plan_get(rtoc_ctx* ctx, double* positions, double* com, double* R, double* step_length, int* ok, int count,
                            int* size, int* current_step);
int rtoc_foot_step_place(rtoc_ctx* ctx, const int* phase_of_grid_point, int nstages);
int rtoc_foot_step_refs(rtoc_ctx* ctx, const rtoc_foot_step_ref_params* r, const int* phase_of_grid_point, const unsigned* phase_masks,
                        int nphases, int nstages);

/* linearizeContactDynamics (src/dynamics/contact_dynamics.cpp:12-33) on intermediate / lift grids and
 * linearizeImpactDynamics (src/dynamics/impact_dynamics.cpp:12-27) on impact grids, for every (instance, grid point)
 * but the terminal one: from RTOC_BUF_SOL (q, v, a | dv, f_stack, u) to RTOC_BUF_CDD
 *   IDC      [ID; C]            ID = RNEA(q, v, a, f) - [0; u]        C = Baumgarte residual (impact: contact velocity);
 *                               point contact: 3 rows, classical linear acceleration (point_contact.hxx:14-31); surface
 *                               contact: 6 rows, spatial acceleration + kp Log6(X_ref^-1 X) (surface_contact.hxx:12-29)
 *   DIDDA    dID/da  (= M(q); impact: dID/ddv)          DCDA   dC/da  (impact: unused, dC/dv is in DIDCDQV)
 *   DIDCDQV  [dID/dq dID/dv; dC/dq dC/dv]
 * i.e. everything computeMJtJinv / condenseContactDynamics read.
 * augment_residual != 0: also the multiplier terms of the same functions (contact_dynamics.cpp:35-52,
 * impact_dynamics.cpp:19-27), ADDED to what the cost / constraint stages left in the residuals (so once per iteration):
 *   lq += dIDdq^T beta + dCdq^T mu   lv += dIDdv^T beta + dCdv^T mu   la += dIDda^T beta + dCda^T mu   lf -= dCda beta
 *   lu -= beta (actuated part)       lu_passive = nu_passive - beta (floating base)
 * (impact grids: ldv instead of la, dCdv instead of dCda, lu_passive = 0); beta, mu_stack, nu_passive from RTOC_BUF_SOL,
 * lq / lv / lu in RTOC_BUF_KKT, la / lf / lu_passive in RTOC_BUF_CDD. */
int rtoc_linearize_contact_dynamics(rtoc_ctx* ctx, int augment_residual);

/* INACTIVE ENTRIES (include/rtoc.h, ahead of rtoc_condense, lists them): the entry points of this header keep to the same contract.
 * Of the iterate in RTOC_BUF_SOL they use q, v, lmd, gmm on every grid point; a, beta and f / mu of the dimf stacked rows of the
 * ACTIVE contacts on every grid point but the last (a foot that lifted leaves its f behind); u, nu_passive and xi[0..dims) where
 * the grid point has controls.  initConstraints sets slack and dual of the active rows from the iterate alone; the linearisation
 * reads slack and dual of the active rows; the line search's trial evaluation reads dx, du and daf[0..nv + dimf) of the direction
 * and slack, dslack of the active rows; rtoc_sto_compute_step_sizes reads dts[0] of the impact and lift grid points. */

/* ---- evalKKT of the contact path on the device (no inequality rows) ----
 * {Intermediate,Impact,Terminal}Stage::evalKKT up to the condensation (src/ocp/intermediate_stage.cpp:94-132,
 * impact_stage.cpp:82-114, terminal_stage.cpp:72-100) for an OCP whose cost is the ConfigurationSpaceCost of
 * rtoc_set_configuration_cost: setZero, quadratize{Stage,Impact,Terminal}Cost, linearize{,Impact,Terminal}StateEquation
 * (rtoc_linearize_state_equation), linearizeContactDynamics / linearizeImpactDynamics with the multiplier terms
 * (rtoc_linearize_contact_dynamics(ctx, 1)) and, on grids with GridInfo::switching_constraint, linearizeSwitchingConstraint
 * (src/dynamics/switching_constraint.cpp:26-70: P, Phix, Phia, Phit, the xi terms of lx / la and the STO terms of h, Qtt,
 * hv, ha; the impacting contacts and their positions are those of the impact grid two points ahead in the contact
 * schedule; free-flyer transport: RTOC_OPT_SWITCHING_TRANSPORT) -- RTOC_BUF_SOL in, the pre-condensation records
 * RTOC_BUF_KKT / RTOC_BUF_CDD, RTOC_BUF_SE3 and RTOC_BUF_DX0 out; rtoc_newton_iteration takes it from there.  Needs
 * rtoc_set_robot_model, rtoc_set_contact_schedule, rtoc_set_configuration_cost, rtoc_set_initial_state. */
int rtoc_contact_eval_kkt(rtoc_ctx* ctx);

/* ---- task-space cost components evaluated by rtoc_contact_eval_kkt beside the ConfigurationSpaceCost ----
 * TaskSpace3DCost (src/cost/task_space_3d_cost.cpp: the world position of a frame) and CoMCost (src/cost/com_cost.cpp: the
 * centre of mass), each with a constant reference (set_const_ref) or a periodic one: PeriodicSwingFootRef
 * (src/cost/periodic_swing_foot_ref.cpp) / PeriodicCoMRef (src/cost/periodic_com_ref.cpp), evaluated on the device from the
 * grid time (isActive / updateRef, the reference's loops).  Per active term: diff = x(q) - x_ref(t),
 * lq += s J^T W diff, Qqq += s J^T W J (Gauss-Newton), the cost value s/2 sum W diff^2 into what evalOCP sums; s = dt on
 * intermediate / lift grids with `weight`, 1 on impact grids with `weight_impact` and on the terminal grid with
 * `weight_terminal`; on intermediate / lift grids also hx += J^T W diff and h += 1/2 sum W diff^2 (the STO sensitivities).
 * A term whose weight of the grid's kind is zero is off there, as in the reference (enable_cost_).
 * A 3D frame term needs only the frame's origin in its parent joint's frame: the world-aligned linear Jacobian does not depend
 * on the frame's rotation.
 * TaskSpace6DCost (src/cost/task_space_6d_cost.cpp, include/robotoc/cost/task_space_6d_cost.hpp:184-214: the world placement of
 * a frame): X = X_ref^-1 oMf, d = log6(X) in Pinocchio's Motion order [linear(3); angular(3)], JJ = Jlog6(X) J_frame with J_frame
 * the LOCAL frame Jacobian; lq += s JJ^T W d, Qqq += s JJ^T W JJ, the value s/2 sum W d^2, s and W by the rules above.  Parity
 * with Pinocchio's log6 / Jlog6 / getFrameJacobian is UNPINNED (Pinocchio is absent): the term is validated against a numpy
 * restatement that is itself pinned by finite differences (tests/task_cost_6d_restatement.py).
 * WEIGHT ORDER: the reference stores weight_.head<3>() = weight_rotation, tail<3>() = weight_position
 * (task_space_6d_cost.cpp:124-125) and multiplies Log6Map(...) componentwise, whose first three components are the LINEAR part: the
 * argument called "rotation" weights the linear components.  This struct carries the six weights in the order they multiply d
 * (weight*: components 0..2, weight_angular*: components 3..5); the host classes fill them exactly as the reference's setters do.
 * A per-grid-point reference table (RTOC_REF_TABLE, rtoc_set_task_ref_table) serves references that are the user's objects
 * (TaskSpace6DRefBase / TaskSpace3DRefBase / CoMRefBase have no concrete class in the reference library): the host calls the
 * object's updateRef / isActive once per grid point and hands the results over. */
#define RTOC_TASK_FRAME_3D 0       /* TaskSpace3DCost                                                   */
#define RTOC_TASK_COM 1            /* CoMCost                                                           */
#define RTOC_TASK_FRAME_6D 2       /* TaskSpace6DCost                                                   */
#define RTOC_REF_CONST 0           /* set_const_ref: x0 is the reference, always active                 */
#define RTOC_REF_PERIODIC_FOOT 1   /* PeriodicSwingFootRef(x3d0 = x0, step_length = rate, step_height, t0,
                                    *   period_swing = period_active, period_stance = period_inactive, is_first_step_half) */
#define RTOC_REF_PERIODIC_COM 2    /* PeriodicCoMRef(com_ref0 = x0, vcom_ref = rate, t0, period_active, period_inactive,
                                    *   is_first_move_half)                                              */
#define RTOC_REF_TABLE 3           /* rtoc_set_task_ref_table: placement and active flag per grid point  */
#define RTOC_MAX_TASK_COSTS 8
typedef struct rtoc_task_cost {
  int kind, ref_kind;
  int frame_parent;            /* RTOC_TASK_FRAME_3D / _6D: joint the frame is attached to             */
  int first_half;              /* is_first_step_half / is_first_move_half                              */
  double frame_p[3];           /* frame origin in that joint's frame                                   */
  double weight[3], weight_terminal[3], weight_impact[3];
  double x0[3];                /* const ref / x3d0 / com_ref0                                          */
  double rate[3];              /* step_length (foot) / vcom_ref (CoM)                                  */
  double step_height, t0, period_active, period_inactive;   /* swing | stance, active | inactive       */
  /* RTOC_TASK_FRAME_6D (appended: everything above is the layout the 3D terms have always had) */
  double frame_R[9];           /* frame axes in that joint's frame (row-major)                         */
  double ref_R[9];             /* const ref: rotation (x0 is its position)                             */
  double weight_angular[3], weight_angular_terminal[3], weight_angular_impact[3];   /* components 3..5 of d: what the
                                * reference's setters call weight_position (WEIGHT ORDER above); weight* multiply 0..2 */
} rtoc_task_cost;
/* one grid point of a reference table: what the user's updateRef / isActive returned there.  A 3D / CoM term reads only p. */
typedef struct rtoc_task_ref_entry {
  double R[9], p[3];           /* reference placement (R row-major)                                    */
  int active, pad;             /* isActive(grid_info)                                                  */
} rtoc_task_ref_entry;
/* terms[nterms] shared by the batch (per_instance = 0) or terms[batch][nterms] (per_instance = 1: every instance its own
 * references).  RTOC_ERR_BAD_ARG: nterms outside [0, RTOC_MAX_TASK_COSTS], a negative weight, a frame parent outside the
 * model's joints, a non-positive period of a periodic reference, an unknown kind / ref_kind; needs rtoc_set_robot_model.
 * A RTOC_TASK_FRAME_6D term: all 18 weights non-negative, frame_R / ref_R finite.
 * nterms = 0 (terms may be NULL) removes the terms: rtoc_contact_eval_kkt then launches exactly what it launched before.
 * rtoc_unconstr_eval_kkt (and what calls it) evaluates the terms as well: s = its dt on every grid point but the last, 1 and
 * weight_terminal on the last, no impact kind, hx / h untouched (unconstr_intermediate_stage.cpp has no Hamiltonian terms),
 * the cost value only when the line search asks for it; times from rtoc_set_grid_times under the same readiness rule.
 * The kernel takes the subtree of a joint as the joints after it in the table down to the next one no deeper, which holds
 * because rtoc_set_robot_model only accepts depth-first ordered tables. */
int rtoc_set_task_costs(rtoc_ctx* ctx, const rtoc_task_cost* terms, int nterms, int per_instance);
/* GridInfo::t of every grid point of a fixed grid (t[nstages], shared by the batch): what the periodic references read.
 * With switching-time optimisation (rtoc_sto_set_problem) the times come from the device instead: correctTimeSteps
 * (time_discretization.cpp:186-222) per instance, prev_event_time + (j - prev_event_stage) dt, the event time on impact grids,
 * t + T on the terminal one.  rtoc_get_grid_times: the times rtoc_contact_eval_kkt uses, host_out[count <= batch][nstages]. */
/* rtoc_set_grid forgets the times of a fixed grid: set them again after it, or rtoc_contact_eval_kkt returns
 * RTOC_ERR_NOT_READY while terms are set. */
int rtoc_set_grid_times(rtoc_ctx* ctx, const double* t, int nstages);
/* The reference table of term `term` (its ref_kind must be RTOC_REF_TABLE): entries[nstages] shared by the batch
 * (per_instance = 0) or entries[batch][nstages], indexed by GRID POINT, not by time; nstages must be the current grid's.
 * RTOC_ERR_BAD_ARG: term outside [0, RTOC_MAX_TASK_COSTS), a wrong nstages, a non-finite entry.  rtoc_set_grid forgets every
 * table, as it forgets the grid times; rtoc_set_task_costs keeps them (a table belongs to the term INDEX).  Evaluating a
 * RTOC_REF_TABLE term without a table returns RTOC_ERR_NOT_READY.  rtoc_clone copies the tables. */
int rtoc_set_task_ref_table(rtoc_ctx* ctx, int term, const rtoc_task_ref_entry* entries, int nstages, int per_instance);
/* the table of term `term` as the instances read it (see rtoc_foot_step_refs above, which fills such tables on the device) */
int rtoc_get_task_ref_table(rtoc_ctx* ctx, int term, rtoc_task_ref_entry* entries, int count, int* per_instance);
int rtoc_get_grid_times(rtoc_ctx* ctx, double* host_out, int count);
/* LocalContactForceCost (src/cost/local_contact_force_cost.cpp) evaluated by rtoc_contact_eval_kkt behind the terms above and
 * ahead of the constraints and the dynamics.  Per contact i active at the grid point, d = f_i[0:3] - f_ref[i], o_i its offset
 * in the stack of the active contacts (3 rows per point contact, 6 per surface contact, only the first 3 of which are touched):
 * intermediate / lift grids (:81-144): lf[o_i:o_i+3] += dt f_weight[i] d, diag(Qff)[o_i:o_i+3] += dt f_weight[i], the cost value
 * += dt/2 sum f_weight[i] d^2, and the STO sensitivities hf[o_i:o_i+3] = f_weight[i] d, h += 1/2 sum f_weight[i] d^2
 * (intermediate_stage.cpp:104-108), dt the instance's own time step with switching-time optimisation; impact grids (:169-230):
 * the same with fi_ref / fi_weight over the impacting contacts, scale 1, hf and h untouched; the terminal grid (:147-166):
 * nothing.  Written: RTOC_CDD_LF, the diagonal of RTOC_CDD_QFF, RTOC_CDD_HF, RTOC_KKT_SCAL[RTOC_KKT_SCAL_H] and the cost value
 * rtoc_contact_eval_ocp sums.
 * cost[1] shared by the batch (per_instance = 0) or cost[batch] (per_instance = 1); cost = NULL removes the term:
 * rtoc_contact_eval_kkt then launches exactly what it launched before.  Contacts at and beyond the model's ncontacts are
 * ignored.  RTOC_ERR_NOT_READY without rtoc_set_robot_model; RTOC_ERR_BAD_ARG: a negative or non-finite weight, a non-finite
 * reference, a context with dims.nf_max == 0 -- a refused call leaves the term that was set in force.  rtoc_clone copies the
 * term; rtoc_unconstr_eval_kkt has no contacts and ignores it. */
typedef struct rtoc_contact_force_cost {
  double f_ref[RTOC_MAX_CONTACTS][3], f_weight[RTOC_MAX_CONTACTS][3];     /* set_f_ref / set_f_weight   */
  double fi_ref[RTOC_MAX_CONTACTS][3], fi_weight[RTOC_MAX_CONTACTS][3];   /* set_fi_ref / set_fi_weight */
} rtoc_contact_force_cost;
int rtoc_set_contact_force_cost(rtoc_ctx* ctx, const rtoc_contact_force_cost* cost, int per_instance);

/* ---- inequality rows of the contact path evaluated on the device (the Constraints object of examples/anymal/trot.cpp:
 * six joint-limit components + FrictionCone) ----
 * Joint limits: the rows of rtoc_set_constraint_rows with their bounds from rtoc_set_constraint_bounds.  Friction cones: the
 * rows of rtoc_set_friction_cones with ContactStatus::frictionCoefficient(k) from rtoc_set_friction_coefficients
 * (mu[k] > 0, k < ncontacts <= RTOC_MAX_CONTACTS) and contactRotation(k) from rtoc_set_contact_schedule's rotations; whether
 * impact grids carry them: RTOC_OPT_IMPACT_CONES.  Once bounds / coefficients are on the device, rtoc_contact_eval_kkt also
 * runs Constraints::linearizeConstraints for those rows -- residual = g + slack, cmpl = slack dual - barrier, the cone
 * Jacobians into RTOC_BUF_CONE, l += dg^T dual (joint_position_lower_limit.cpp:58-77 and its siblings, friction_cone.cpp:
 * 119-191) -- and rtoc_newton_iteration condenses, expands and updates them as before.  Rows without bounds / cones without
 * coefficients stay host-evaluated (RTOC_BUF_CON / RTOC_BUF_CONE uploaded by the caller).
 * rtoc_set_barrier_param: Constraints::setBarrierParam / setFractionToBoundaryRule (also set by rtoc_set_constraint_bounds).
 * rtoc_contact_init_constraints: OCPSolver::initConstraints (src/solver/ocp_solver.cpp:92-96) -- slack = -g clipped at
 * sqrt(barrier), dual = barrier / slack (pdipm.hxx:12-23) at the iterate in RTOC_BUF_SOL; zeroes RTOC_BUF_CON first. */
int rtoc_set_barrier_param(rtoc_ctx* ctx, double barrier_param, double fraction_to_boundary_rule);
int rtoc_set_friction_coefficients(rtoc_ctx* ctx, const double* mu, int ncontacts);
int rtoc_contact_init_constraints(rtoc_ctx* ctx);
/* Contact wrench cones of surface contacts on the device (rtoc_set_wrench_cones rows; ContactWrenchCone,
 * src/constraints/contact_wrench_cone.cpp:114-204): xy_mu[k] = {X, Y, mu} of contact k -- the sole rectangle 2X x 2Y and
 * ContactStatus::frictionCoefficient -- from which the 17 x 6 cone matrices are built (rtoc_wrench_cone_matrix).  Once set,
 * rtoc_contact_init_constraints also writes the matrices into RTOC_BUF_CONE and initialises these rows, and
 * rtoc_contact_eval_kkt evaluates them (g = cone f on the local contact wrench; lf += cone^T dual). */
int rtoc_set_wrench_cone_params(rtoc_ctx* ctx, const double* xy_mu, int ncontacts);
/* OCPSolver::updateSolution (src/solver/ocp_solver.cpp:111-145) for that OCP, one launch sequence: rtoc_contact_eval_kkt,
 * then rtoc_newton_iteration(ctx, 0, fraction_to_boundary_rule).  host_kkt_error[count <= batch] (may be NULL / 0): the KKT
 * error of the iterate it linearised at. */
int rtoc_contact_update_solution(rtoc_ctx* ctx, double fraction_to_boundary_rule, double* host_kkt_error, int count);

/* ---- OCPSolver::solve (src/solver/ocp_solver.cpp:169-213): the iteration schedule, ONE owner for every host shell ----
 * The loop of solve() between its `init_solver` prologue and its epilogue: the STO regularisation of the first
 * initial_sto_reg_iter iterations since the last (re-)discretisation (:171-177), updateSolution, the mesh-refinement branch
 * (KKT error below kkt_tol_mesh and TimeDiscretization::maxTimeStep above max_dt_mesh, :181-199; `inner_iter` restarts at 0 and is
 * incremented by the loop header like the reference's), convergence (:200-210), `iter = max_iter` without it (:212-214).  Pure host
 * logic -- what an iteration, a refinement and the largest time step ARE is the shell's business (callbacks; a non-zero return
 * aborts the loop and is returned): robotoc_amd/solver.py (batched: the KKT error it reports is the largest of the batch) and
 * robotoc::OCPSolver::solve of robotoc_amd/host/robotoc_hip_solver.hpp both run THIS function.  No device call, no context. */
#define RTOC_SOLVE_MAX_REFINEMENTS 64
typedef struct rtoc_solve_options {
  int max_iter;              /* SolverOptions::max_iter */
  double kkt_tol;            /* SolverOptions::kkt_tol */
  int sto_enabled;           /* ocp_.sto_cost && ocp_.sto_constraints (and at least one discrete event) */
  int initial_sto_reg_iter;  /* SolverOptions::initial_sto_reg_iter */
  double initial_sto_reg;    /* SolverOptions::initial_sto_reg */
  double kkt_tol_mesh;       /* SolverOptions::kkt_tol_mesh */
  double max_dt_mesh;        /* SolverOptions::max_dt_mesh */
} rtoc_solve_options;
typedef struct rtoc_solve_callbacks {
  void* user;
  int (*set_sto_regularization)(void* user, double sto_reg);  /* sto_.setRegularization + the statistics' event times; STO problems only */
  int (*update_solution)(void* user, double* kkt_error);      /* updateSolution; *kkt_error = KKTError() */
  int (*max_time_step)(void* user, double* max_dt);           /* time_discretization_.maxTimeStep(); STO problems only */
  int (*mesh_refinement)(void* user);                         /* :185-196: store, discretize, interpolate, initConstraints, clearHistory */
} rtoc_solve_callbacks;
typedef struct rtoc_solve_stats {
  int convergence, iter;
  int num_mesh_refinements;
  int mesh_refinement_iter[RTOC_SOLVE_MAX_REFINEMENTS];       /* iter + 1 of every refinement (the first RTOC_SOLVE_MAX_REFINEMENTS) */
} rtoc_solve_stats;
int rtoc_solve_loop(const rtoc_solve_options* options, const rtoc_solve_callbacks* callbacks, rtoc_solve_stats* stats);

/* ---- SolutionInterpolator on the device (src/solver/solution_interpolator.cpp:22-230): the warm start of a re-discretised grid ----
 * What OCPSolver::solve does around a re-discretisation -- store (:22-27), discretize, interpolate (:30-113) -- in the mesh-refinement
 * branch (ocp_solver.cpp:184-199) and for the receding-horizon warm start of every solve(t, q, v, init_solver = true) (:159-163,
 * :215-220), for every instance of the batch at once and without the records leaving the device.
 * rtoc_solution_store(ctx, t0): copies into memory of the context RTOC_BUF_SOL ([batch][nstages] records), the grid's types and time
 * steps, the masks of rtoc_set_contact_schedule and the grid times t[0] = t0, t[i + 1] = t[i] + dt[i] (summed in this order, in
 * double).  With an STO problem set (rtoc_sto_set_problem) the time steps and hence the times are every instance's own, as the device
 * holds them: call rtoc_sto_correct_time_steps first, like ocp_solver.cpp:186-189 and :216-219; without one they are the grid's and
 * shared by the batch.  A copy, not a view: rtoc_set_grid, rtoc_set_contact_schedule and rtoc_sto_set_problem come between the store
 * and the interpolation, and the store survives them.  A second store replaces the first.
 * rtoc_solution_interpolate(ctx, t0): writes EVERY double of every record of RTOC_BUF_SOL for the current grid, schedule and time
 * steps (times from t0 by the same sum) from the store, one wave per (instance, grid point).  Per new grid point at time t (:33-110):
 * t at or before the first stored time: stored record 0; at or behind the last: the last stored record; an impact / lift with a stored
 * event of the same type within 1e-9: that record (:59-72), at an impact with u, the a | dv slot and nu_passive zeroed
 * (modifyImpactSolution, :201-208) and xi of the new grid point two BEFORE it taken from the stored record two before the stored
 * impact; an impact / lift without one: initEventSolution (:175-198) between the stored neighbours, or interpolatePartial
 * (:149-172; plus the impact zeroing) when the later neighbour is the stored terminal point; every other grid point: interpolate
 * (:119-146) when the later neighbour is an intermediate point, interpolatePartial otherwise; on the last record
 * modifyTerminalSolution (:211-224).  The earlier neighbour is findStoredGridIndexBeforeTime's, stepped back over stored points
 * whose dt <= 0 (an impact has no extent in time); alpha = (t - t_a) / dt_a clamped to [0, 1].  The f / mu stacks are compacted by
 * the active contacts of their own grid point: each is expanded by the stored mask and re-packed by the new grid point's, 3 or 6
 * rows per contact; stack entries beyond the packed rows, xi of a blended grid point and the padding of a blended record are zero.
 * q follows Robot::interpolateConfiguration: joints linearly, a free-flyer base along the screw motion q1 (+) alpha (q2 (-) q1), the
 * quaternion that of the rotation matrix (w > 0 where its trace is positive), normalised.
 * Not the reference's: at a COPIED impact the a | dv slot is zeroed like at a blended one (the host mirrors do; the reference keeps
 * dv there) -- INTEGRATION.md.  InterpolationOrder::Zero is not implemented.
 * With nothing stored rtoc_solution_interpolate returns RTOC_OK and writes nothing (:34) -- in a context it would not refuse: the
 * refusals come first.  Both calls refuse ahead of their first launch, and a refused call writes nothing: RTOC_ERR_NOT_READY
 * without a grid, without RTOC_BUF_SOL (store), in a context with dims.nf_max > 0 without rtoc_set_robot_model (the rows per
 * contact come from its contact_type) or without a contact schedule set since rtoc_set_grid last changed the grid (the masks
 * belong to a grid; shapes without contact rows need neither), and with an STO problem whose time steps date from before that
 * (rtoc_sto_set_problem or rtoc_sto_correct_time_steps again; setting the grid in force again changes nothing);
 * RTOC_ERR_BAD_ARG on a ParNMPC horizon (rtoc_parnmpc_set_horizon), for a non-finite t0, and for a store whose contacts are not
 * those of the model now set.  Both are asynchronous on the context's stream.
 * rtoc_solution_stored: *nstages = the grid points of the stored solution, 0 if none.  rtoc_solution_forget: nothing is stored any
 * more.  rtoc_clone copies the store. */
int rtoc_solution_store(rtoc_ctx* ctx, double t0);
int rtoc_solution_interpolate(rtoc_ctx* ctx, double t0);
int rtoc_solution_stored(const rtoc_ctx* ctx, int* nstages);
int rtoc_solution_forget(rtoc_ctx* ctx);

/* ---- ControlPolicy on the device (src/mpc/control_policy.cpp:24-60): what an MPC hands to the robot or the simulator ----
 * The feed-forward joint torque tauJ, the joint references qJ, dqJ and the gains Kp, Kd cut out of the LQR policy of the Riccati
 * recursion, of every instance at its own query time, from RTOC_BUF_SOL and RTOC_BUF_RIC as they stand and without either leaving the
 * device; and the law the simulator applies with them at every control tick, u = tauJ - Kp (qJ - q) - Kd (dqJ - v)
 * (bindings/python/robotoc_sim/mpc_simulation.py:6-11).
 * Grid times: tg[0] = t0, tg[i + 1] = tg[i] + dt[i], summed in this order in double (the sum of rtoc_solution_store); with an STO
 * problem set the time steps are every instance's own, as the device holds them, else the grid's and shared by the batch.
 * N: the reference's time_discretization.N() (:28), the number of time stages, not of grid points.  Per query time t:
 * t < tg[0]: record 0 (:31-38); else the first i in 1 .. N - 2 with t < tg[i] whose record i - 1 is no impact grid point (:39-40):
 * alpha = (tg[i] - t) / (tg[i] - tg[i - 1]), not clamped, and every output alpha rec[i - 1] + (1 - alpha) rec[i] (:41-52); else
 * record N - 1 (:55-59).  Of a record: tauJ = RTOC_SOL_U; qJ, dqJ = the last nu entries of RTOC_SOL_Q (nq of them: nv + 1 with a
 * free-flyer) and RTOC_SOL_V; Kp = columns nv - nu .. nv - 1 and Kd = columns 2nv - nu .. 2nv - 1 of RTOC_RIC_K (Kq().rightCols,
 * Kv().rightCols).  These doubles of the one or two records are read and nothing else.
 * Not the reference's, which reads u and K of impact grid points there, where they are undefined: where record i of
 * the chosen interval is an impact grid point the policy is record i - 1 unblended; where the fallback record N - 1 is one, it is
 * record N - 2.
 * rtoc_control_policy: out[count][stride] = [tauJ | qJ | dqJ | Kp | Kd] (rtoc_layout.h: rtoc_control_policy_stride and the field offsets;
 * every field on a 64-byte boundary, Kp and Kd nu x nu column-major with leading dimension nu, the padding zero).
 * rtoc_control_input: u[count][nu] at the measured states x[count][nq + nv] (laid out as for rtoc_set_initial_state); Kp and Kd are
 * not written anywhere.
 * t[1] is shared by the batch (per_instance = 0) or t[count] is given per instance (1); the calls act on the first count <= batch
 * instances.  flags = 0: host pointers; t (and x) are validated as finite and the call returns with the result on the host.
 * flags = RTOC_POLICY_DEVICE_PTRS: every pointer is a device pointer, nothing is inspected, the call is asynchronous on the
 * context's stream, and an instance with a non-finite t gets NaN in all of its outputs.  (The first call of a context, and the
 * first with an STO problem set, allocates the scratch for the grid times, which synchronises the device; later calls only launch.)
 * Refusals come ahead of any launch, and a refused call writes nothing: RTOC_ERR_NOT_READY without a grid, without RTOC_BUF_RIC or
 * RTOC_BUF_SOL, and with an STO problem whose time steps date from before the last change of the grid (the rule of
 * rtoc_solution_store); RTOC_ERR_BAD_ARG on a ParNMPC horizon, for N < 1 or N > nstages - 1, count outside 1 .. batch, per_instance
 * outside {0, 1}, a null pointer, an unknown flag bit, a non-finite t0, a shape with dims.nu < 1 and, with host pointers, a
 * non-finite t or x.
 * The calls hold no state (rtoc_clone has nothing to copy). */
#define RTOC_POLICY_DEVICE_PTRS 1
int rtoc_control_policy(rtoc_ctx* ctx, double t0, const double* t, int per_instance, int N, double* out, int count, int flags);
int rtoc_control_input(rtoc_ctx* ctx, double t0, const double* t, int per_instance, int N, const double* x, double* u, int count,
                       int flags);

/* ---- filter line search on the device (src/line_search/line_search.cpp:31-83, LineSearchSettings) ----
 * rtoc_contact_eval_ocp: DirectMultipleShooting::evalOCP's performance index (direct_multiple_shooting.cpp:100-126) of every
 * instance -- host_cost[count] = cost + cost_barrier, host_violation[count] = primal_feasibility (l1).  trial = 0: of the iterate
 * rtoc_contact_eval_kkt has just linearised (records not yet condensed: dms_.getEval()); trial = 1: of the trial iterate
 * SOL (+) step DIR with slack + step dslack, step = the primal entry of RTOC_BUF_STEP of every instance
 * (dms_trial_.integratePrimalSolution + evalOCP, line_search.cpp:65-71) -- RTOC_BUF_SOL / CON / DIR / STEP keep their contents, the
 * KKT / CDD records are overwritten (the next rtoc_contact_eval_kkt rewrites them).
 * rtoc_set_line_search: SolverOptions::enable_line_search with LineSearchSettings::step_size_reduction_rate (0.75), min_step_size
 * (0.05), filter_cost_reduction_rate / filter_constraint_violation_reduction_rate (0.005): rtoc_newton_iteration (and
 * rtoc_contact_update_solution) then run LineSearch::computeStepSize between the step-size computation and the update
 * (ocp_solver.cpp:133-139) -- rtoc_contact_line_search: every instance backtracks from its maximum primal step until its filter
 * (rtoc_line_search_filter's, cleared by rtoc_line_search_clear) accepts the trial pair; *host_trials = trial evaluations run. */
int rtoc_contact_eval_ocp(rtoc_ctx* ctx, int trial, double* host_cost, double* host_violation, int count);
/* What rtoc_contact_eval_ocp sums, grid point by grid point: host_out[count <= batch][nstages] = the value of the stage / impact /
 * terminal cost (every component of the cost function) as the last rtoc_contact_eval_kkt stored it -- or the last
 * rtoc_unconstr_eval_kkt with the line search enabled, which is when that path stores them.  RTOC_ERR_NOT_READY before either. */
int rtoc_get_stage_costs(rtoc_ctx* ctx, double* host_out, int count);
int rtoc_set_line_search(rtoc_ctx* ctx, int enable, double step_size_reduction_rate, double min_step_size,
                         double filter_cost_reduction_rate, double filter_constraint_violation_reduction_rate);
int rtoc_contact_line_search(rtoc_ctx* ctx, int* host_trials);
/* LineSearchSettings::line_search_method (include/robotoc/line_search/line_search_settings.hpp:13-29): 0 = LineSearchMethod::Filter
 * (default), 1 = MeritBacktracking -- LineSearch::meritBacktrackingLineSearch (src/line_search/line_search.cpp:87-128): penalty
 * parameter (1 + margin_rate) x max over the grid of SplitSolution::lagrangeMultiplierLinfNorm (:120-128), directional derivative of
 * cost + barrier + penalty x violation from one trial at step eps, then backtracking until armijoCondition (:111-117) holds with
 * armijo_control_rate; the reference's defaults are 0.001, 0.05, 1e-8.  rtoc_line_search_merit_terms: the penalty parameters and
 * directional derivatives of the last rtoc_contact_line_search (either pointer may be NULL).
 * The unconstrained solver is filter-only, like UnconstrLineSearch (src/line_search/unconstr_line_search.cpp, which never reads
 * line_search_method): after rtoc_unconstr_eval_kkt the line search takes the filter path whatever `method` says. */
int rtoc_set_line_search_method(rtoc_ctx* ctx, int method, double armijo_control_rate, double margin_rate, double eps);
int rtoc_line_search_merit_terms(rtoc_ctx* ctx, double* host_penalty, double* host_directional_derivative, int count);
/* trial evaluations (dms_trial_.evalOCP calls, line_search.cpp:70, :99, :109) of the last line search, whichever entry point ran it */
int rtoc_line_search_trials(rtoc_ctx* ctx, int* trials);

/* ---- the unconstrained solver iteration closed on the device (BASELINE configuration 1: fixed base, no contacts) ----
 * ConfigurationSpaceCost (src/cost/configuration_space_cost.cpp:274-470): diagonal weights on q - q_ref (on the manifold:
 * q_ref has nq entries, the first 7 a free-flyer placement if dims.np == 6; weights nv entries, the first 6 on the base's
 * log6 difference), v - v_ref, a, u - u_ref, the terminal and the impact weights; all weights non-negative. */
typedef struct rtoc_configuration_cost {
  double q_ref[RTOC_MAX_JOINTS], v_ref[RTOC_MAX_JOINTS], u_ref[RTOC_MAX_JOINTS];
  double q_weight[RTOC_MAX_JOINTS], v_weight[RTOC_MAX_JOINTS], a_weight[RTOC_MAX_JOINTS], u_weight[RTOC_MAX_JOINTS];
  double q_weight_terminal[RTOC_MAX_JOINTS], v_weight_terminal[RTOC_MAX_JOINTS];
  double q_weight_impact[RTOC_MAX_JOINTS], v_weight_impact[RTOC_MAX_JOINTS], dv_weight_impact[RTOC_MAX_JOINTS];
} rtoc_configuration_cost;
int rtoc_set_configuration_cost(rtoc_ctx* ctx, const rtoc_configuration_cost* cost);
/* A time-varying q_ref: ConfigurationSpaceCost::set_ref(std::shared_ptr<ConfigurationSpaceRefBase>)
 * (src/cost/configuration_space_cost.cpp:84-89, include/robotoc/cost/configuration_space_cost.hpp:166-216).  The host asks the
 * object once per grid point (updateRef / isActive) and hands the answers over: q_ref[nstages][nq] and active[nstages] shared by
 * the batch (per_instance = 0), or q_ref[batch][nstages][nq] and active[batch][nstages] (per_instance = 1: every instance tracks
 * its own posture); nq = nv, or nv + 1 with a free-flyer base, a row laid out like rtoc_configuration_cost::q_ref; rows are indexed
 * by GRID POINT, not by time, like rtoc_set_task_ref_table's; nstages must be the current grid's.  active = NULL: active
 * everywhere.  Per grid point (configuration_space_cost.cpp:251-442): the q terms -- lq, Qqq, the cost value and, on
 * intermediate and lift grids, hx[0:nv] and the q share of h -- use that grid point's row (that instance's with per_instance = 1)
 * and are absent altogether where the row is inactive (enable_q_cost_ && isCostConfigActive); the v, a / dv and u terms are
 * unchanged: v_ref, u_ref and all weights stay those of rtoc_set_configuration_cost, as in the reference, where only q_ref
 * varies.  Both rtoc_contact_eval_kkt and rtoc_unconstr_eval_kkt read the table, hence the line search's trial evaluations too.
 * q_ref = NULL removes the table: the constant q_ref is in force again and both entry points launch exactly what they launched
 * before.  RTOC_ERR_BAD_ARG: a wrong nstages, a non-finite entry of an ACTIVE row (inactive rows are not inspected, here or on
 * the device: they may hold anything), per_instance outside {0, 1} -- a refused call leaves the table that was set in force.
 * rtoc_set_grid forgets the rows but not that a table is in use: until it is set again or removed, both entry points return
 * RTOC_ERR_NOT_READY before anything is launched, never the constant reference in its place (the rule of the task tables).
 * rtoc_set_configuration_cost keeps the table, and its q_ref member is ignored while one is in force.  rtoc_clone copies it. */
int rtoc_set_configuration_ref_table(rtoc_ctx* ctx, const double* q_ref, const int* active, int nstages, int per_instance);
/* the table as the instances read it: q_ref[count][nstages][nq], active[count][nstages] (see rtoc_foot_step_refs above) */
int rtoc_get_configuration_ref_table(rtoc_ctx* ctx, double* q_ref, int* active, int count, int* per_instance);
/* (q, v) of OCPSolver / UnconstrOCPSolver::updateSolution(t, q, v) for every instance: x0[batch][nq + nv], nq = nv, or
 * nv + 1 with a free-flyer base (dims.np == 6: [x y z qx qy qz qw, joints]). */
int rtoc_set_initial_state(rtoc_ctx* ctx, const double* x0, int count);
/* linearizeStateEquation (src/dynamics/state_equation.cpp:29-66) on intermediate / lift grids, linearizeImpactStateEquation
 * (impact_state_equation.cpp:27-57) on impact grids, from RTOC_BUF_SOL (q, v, a | dv, lmd, gmm of the grid point, its
 * successor and -- for Fqq_prev -- its predecessor; the initial state of rtoc_set_initial_state ahead of grid point 0):
 * Fx and the top half of Fxx are written, the multiplier and STO terms are ADDED to lx, la (CDD.la), h, hv, ha, fx like
 * the reference adds them to what the cost left there.  Floating base: the SE(3) difference and its Jacobians
 * (Pinocchio's difference / dDifference restated: log6 and Jlog6 by forward mode), and RTOC_BUF_SE3 = {Fqq_inv,
 * Fqq_prev_inv} as correctLinearizeStateEquation computes them -- rtoc_condense then applies the corrections.  With an
 * initial state set: RTOC_BUF_DX0 = computeInitialStateDirection (state_equation.cpp:99-109). */
int rtoc_linearize_state_equation(rtoc_ctx* ctx);
/* UnconstrDirectMultipleShooting::evalKKT up to the condensation, on every grid point: kkt_matrix / kkt_residual zeroed,
 * quadratizeStageCost / TerminalCost of the cost above, linearizeUnconstrForwardEuler(+Terminal)
 * (src/dynamics/unconstr_state_equation.cpp:8-24), linearizeUnconstrDynamics (src/dynamics/unconstr_dynamics.cpp:52-64:
 * RNEA, its derivatives, the dt-scaled multiplier terms), and computeInitialStateDirection (x0 - s[0].x into
 * RTOC_BUF_DX0) -- from RTOC_BUF_SOL into RTOC_BUF_KKT / RTOC_BUF_CDD in the record convention of rtoc_unconstr_condense.
 * With joint-limit rows and bounds set (below): constraints_->linearizeConstraints as well (residual, cmpl into
 * RTOC_BUF_CON, the duals into the gradients).  With task-space terms set (rtoc_set_task_costs): those components of the cost
 * function as well, right behind the configuration cost (s = dt, the last grid point terminal; needs rtoc_set_grid_times and
 * the table of every RTOC_REF_TABLE term, else RTOC_ERR_NOT_READY before anything is launched). */
int rtoc_unconstr_eval_kkt(rtoc_ctx* ctx, double dt);
/* The joint-limit rows of this path live on the device for their whole life.  After rtoc_set_constraint_rows: the bound
 * of every row, g(z) = sign * z - bound <= 0 (lower limit zmin: sign -1, bound -zmin; upper limit zmax: sign +1, bound
 * zmax), the barrier parameter and the fraction-to-boundary rule (ConstraintsBase setters; 1e-3 / 0.995 in the
 * reference).  rtoc_unconstr_init_constraints = initConstraints (setSlackAndDual at the current iterate). */
int rtoc_set_constraint_bounds(rtoc_ctx* ctx, const double* bounds, int nrows, double barrier_param, double fraction_to_boundary_rule);
int rtoc_unconstr_init_constraints(rtoc_ctx* ctx);
/* UnconstrOCPSolver::updateSolution (src/solver/unconstr_ocp_solver.cpp:96-118): rtoc_unconstr_eval_kkt, the KKT error
 * of the iterate it linearised at (host_kkt_error[count <= batch], may be NULL / 0), rtoc_unconstr_condense, backward,
 * forward, rtoc_unconstr_expand, and SplitSolution::integrate -- RTOC_BUF_SOL holds the next iterate.  Step size 1, or,
 * with joint-limit rows, condenseSlackAndDual / expandSlackAndDual, the fraction-to-boundary step sizes and the slack / dual
 * update as well (unconstr_intermediate_stage.cpp:76-118).  With rtoc_set_line_search(enable = 1): the filter line search of
 * UnconstrLineSearch::computeStepSize (src/line_search/unconstr_line_search.cpp:37-67; unconstr_ocp_solver.cpp:107-111) between
 * the step sizes and the update -- every instance backtracks from its maximum primal step over trial iterates evaluated on
 * the device (integratePrimalSolution + UnconstrDirectMultipleShooting::evalOCP: cost value + log barrier, l1 norm of the
 * state-equation, inverse-dynamics and row residuals); RTOC_BUF_STEP then holds the accepted primal steps.
 * rtoc_contact_eval_ocp / rtoc_contact_line_search serve this path as well: they evaluate with whichever of
 * rtoc_unconstr_eval_kkt / rtoc_contact_eval_kkt ran last. */
int rtoc_unconstr_update_solution(rtoc_ctx* ctx, double dt, double* host_kkt_error, int count);

/* ---- UnconstrParNMPCSolver on the device (backward Euler + backward correction; fixed base, no contacts, nu == nv) ----
 * rtoc_parnmpc_set_horizon: the context's records become the N stages (1 <= N <= max_stages) of UnconstrParNMPCSolver's horizon
 * (src/solver/unconstr_parnmpc_solver.cpp:10-51) in place of a grid of rtoc_set_grid: record i is the reference's stage i at
 * t + (i + 1) dt, EVERY record carries dynamics and constraint rows (the last one too: there is no terminal record), and
 * (q, v) of rtoc_set_initial_state are q_prev, v_prev of stage 0.  A row is active on stage i iff its level is at most the stage
 * number the reference creates the stage's constraint data with (i + 2, N on the last stage; parnmpc_intermediate_stage.cpp:49,
 * parnmpc_terminal_stage.cpp:47).  Buffers hold [batch][N] records as on any grid; rtoc_set_grid ends the mode.  While it lasts,
 * rtoc_unconstr_condense, rtoc_unconstr_expand (expandDual's / dt included), rtoc_update, rtoc_kkt_error and
 * rtoc_integrate_solution act on all N records; every other entry point that works on a grid (the Riccati recursions, the contact
 * path, rtoc_unconstr_eval_kkt / _update_solution, switching-time optimisation, the line search, stage dumps) refuses with
 * RTOC_ERR_BAD_ARG.  rtoc_clone keeps the mode.
 * RTOC_ERR_BAD_ARG on a shape without the kernels (nu != nv, contacts, a free-flyer, 3 nv outside 17..32 or 2 nv > 16).
 * rtoc_parnmpc_init_constraints: UnconstrBackwardCorrection::initConstraints (src/parnmpc/unconstr_backward_correction.cpp:74-89) --
 * setSlackAndDual of the rows of rtoc_set_constraint_rows / rtoc_set_constraint_bounds on all N records.
 * rtoc_parnmpc_init_backward_correction: initAuxMat (:57-71) -- every auxiliary matrix = the terminal-cost Hessian at the last
 * stage's iterate (diag(q_weight_terminal, v_weight_terminal) of rtoc_set_configuration_cost).
 * rtoc_parnmpc_set_aux_mat / rtoc_parnmpc_get_aux_mat: host[count <= batch][N][2nv x 2nv], column-major (tests, warm starts); the
 * matrices are zero until one of the calls above sets them.
 * rtoc_parnmpc_eval_kkt: ParNMPCIntermediateStage / ParNMPCTerminalStage::evalKKT of every stage up to, excluding, the
 * condensations (src/unconstr/parnmpc_terminal_stage.cpp:84-105): the stage cost scaled by dt on every record with the terminal
 * cost ADDED on the last (:88-93), linearizeUnconstrBackwardEuler / ...Terminal (src/dynamics/unconstr_state_equation.cpp:27-53,
 * 65-72), linearizeUnconstrDynamics (src/dynamics/unconstr_dynamics.cpp:53-64) and, with rows, linearizeConstraints, in the record
 * convention of rtoc_unconstr_condense.  rtoc_kkt_error then gives sqrt(sum_i data.KKTError() + kkt_residual.KKTError())
 * (unconstr_parnmpc_solver.cpp:236-238).
 * rtoc_parnmpc_backward_correction: coarseUpdate (without its evalKKT) and backwardCorrection (without its expansion)
 * (unconstr_backward_correction.cpp:154-228; UnconstrSplitBackwardCorrection, unconstr_split_backward_correction.cpp:57-133;
 * UnconstrKKTMatrixInverter::invert, unconstr_kkt_matrix_inverter.hxx:39-79) on whatever condensed records and solution are on the
 * device: H of stage i < N - 1 takes the auxiliary matrix i + 1 the previous call left, the four passes run in the reference's
 * order, aux_mat[i] = -K^-1[0:2nv, 0:2nv] for i > 0, and the direction goes to RTOC_BUF_DIR (dx = (dq, dv), du = da, dlmdgmm).
 * A non-SPD H or S raises RTOC_STAT_PARNMPC_H_NOT_SPD / RTOC_STAT_PARNMPC_S_NOT_SPD on the instance (rtoc.h).
 * rtoc_parnmpc_update_solution: UnconstrParNMPCSolver::updateSolution (unconstr_parnmpc_solver.cpp:97-119) as one launch sequence:
 * rtoc_parnmpc_eval_kkt, the KKT error of the iterate it linearised at (host_kkt_error[count <= batch], may be NULL / 0: then no
 * host synchronisation), condenseSlackAndDual, rtoc_unconstr_condense, the backward correction, rtoc_unconstr_expand, the
 * fraction-to-boundary step sizes, updateSlack / updateDual, SplitSolution::integrate.
 * Refusals of rtoc_parnmpc_eval_kkt and rtoc_parnmpc_update_solution (rtoc_parnmpc_backward_correction, which evaluates nothing,
 * checks dt, the horizon and the solution alone): RTOC_ERR_BAD_ARG for dt <= 0, a free-flyer model or contacts, and while task-space costs, a
 * configuration-reference table or the line search are set on the context (not part of this mode); RTOC_ERR_NOT_READY before
 * rtoc_parnmpc_set_horizon, the model, the cost, the solution or the initial state.  A refused call launches nothing. */
int rtoc_parnmpc_set_horizon(rtoc_ctx* ctx, int N);
int rtoc_parnmpc_init_constraints(rtoc_ctx* ctx);
int rtoc_parnmpc_init_backward_correction(rtoc_ctx* ctx);
int rtoc_parnmpc_set_aux_mat(rtoc_ctx* ctx, const double* host, int count);
int rtoc_parnmpc_get_aux_mat(rtoc_ctx* ctx, double* host, int count);
int rtoc_parnmpc_eval_kkt(rtoc_ctx* ctx, double dt);
int rtoc_parnmpc_backward_correction(rtoc_ctx* ctx, double dt);
int rtoc_parnmpc_update_solution(rtoc_ctx* ctx, double dt, double* host_kkt_error, int count);

#ifdef __cplusplus
}
#endif
#endif
