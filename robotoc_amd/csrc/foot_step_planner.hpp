// foot_step_planner.hpp -- TrotFootStepPlanner (src/mpc/trot_foot_step_planner.cpp) with its RaibertHeuristic
// (src/mpc/raibert_heuristic.cpp) and MovingWindowFilter<2> (include/robotoc/mpc/moving_window_filter.hpp), and what
// MPCTrot::resetContactPlacements (src/mpc/mpc_trot.cpp:357-372) does with the plan -- the placements of every contact phase,
// MPCPeriodicSwingFootRef x 4, MPCPeriodicCoMRef, MPCPeriodicConfigurationRef -- for every instance of a batch, each with its own
// command; and the plan recurrences of PaceFootStepPlanner, CrawlFootStepPlanner and FlyingTrotFootStepPlanner
// (src/mpc/{pace,crawl,flying_trot}_foot_step_planner.cpp), whose MPC shells build the same references; JumpFootStepPlanner
// (src/mpc/jump_foot_step_planner.cpp) with the q_ref of MPCJump::init.  Nothing here leaves the device: the plan is read by the two kernels behind it, which write the per-instance table of
// contact placements and the per-instance reference tables where the cost kernels read them.
//
// foot_step_init_kernel / foot_step_plan_kernel.  Mapping: one lane per (instance, foot), FOOT-MAJOR within the wave -- lane l is
// foot l / 16 of instance 16 blockIdx.x + l % 16 -- so that the 16 lanes of a foot write 16 consecutive doubles of every array
// below, all of which carry the batch index innermost.  The sums over the feet (the centre of mass of the stance feet) are
// gathered across the four 16-lane groups by __shfl and added in the reference's order; R <- R_yaw R and the centre of mass are
// held redundantly by the four lanes of an instance.  The recurrence over the steps is serial per instance and its case chain
// (:145-277) depends on current_step_ and the contact status alone, which the batch shares: the host decides it once and passes
// it in as arguments (FsPlanArgs::stance / pre_rotate / move[] / com_scale[] / foot_scale[]), so no lane branches on its own data.
// No LDS, no atomics.  The same kernel plans the pace (other pairs), the crawl (three stance feet, feet advanced incrementally:
// FsPlanArgs::incremental) and the flying trot (a flight phase, FsPlanArgs::flight: foot and CoM come from step 0 of the previous
// plan, 6 more doubles per lane loaded ahead of every store, in runs of 16 like the rest); both flags are wave-uniform.
// Loads: 24 doubles of state, at most 12 x 3 of the filter ring, 3 of the foot position, 8 of the command per lane, each a run
// of 16 consecutive doubles per foot group.  Stores: per step every lane writes its foot's position (3) and a quarter of
// [CoM | R] (3), again 16 consecutive doubles per group and slot; the lanes of foot 0 write the planner state back.
// The filter ring: 12 slots of (t, x, y) per instance, summed front to back as the deque of the reference is (:129-131), the new
// sample last; all four lanes of an instance evaluate it from the same loads, the stores come after the last load.
//
// biped_walk_init_kernel / biped_walk_plan_kernel.  BipedWalkFootStepPlanner (src/mpc/biped_walk_foot_step_planner.cpp:89-277) on two
// surface contacts (left = contact 0, right = contact 1).  Its step 0 places the swing foot from the STANCE foot's base-relative
// offset (:161-166, :183-188), its feet carry a rotation each, and its centre of mass is the midpoint of the feet plus a stored
// height: none of that is the quadrupeds' recurrence, so it has kernels of its own.  Mapping: one lane per (instance, foot),
// FOOT-MAJOR within the wave -- lane l is foot l / 32 of instance 32 blockIdx.x + l % 32 -- so that the 32 lanes of a foot write 32
// consecutive doubles (256 bytes) of every [slot][batch] array.  The other foot's translation arrives by __shfl across the two
// halves (lane ^ 32), once as measured and once more after the swing foot is placed; R and the centre of mass are held by both
// lanes of an instance.  The case chain comes in as the same FsPlanArgs the quadrupeds use (stance, pre_rotate, move[], com_scale[],
// foot_scale[]): wave-uniform, no lane branches on its own data.  No LDS, no atomics.  The filter ring and the heuristic are
// fs_filter_step_length / fs_filter_store, shared with foot_step_plan_kernel.
// Loads per lane: 11 doubles of state (R, leg distance, CoM height), at most 12 x 3 of the filter ring and 8 of the command, each
// a run of 32 consecutive doubles per half; 3 of the base position and (Raibert) 2 of the base velocity from x0, a state apart; 3 + 9
// of its foot's frame placement from the kinematics' [batch][2][3 | 9], i.e. runs of 3 and 9 doubles 6 and 18 apart.  Stores per
// step and lane: its foot's translation (3), its foot's rotation (9) and its half of [CoM | R] (6), all runs of 32 consecutive
// doubles per half and slot; the lanes of foot 0 write the planner state back after the last load.  Lanes beyond the batch follow
// the last instance and store nothing.
//
// jump_init_kernel<NF> / jump_plan_kernel<NF>.  JumpFootStepPlanner (src/mpc/jump_foot_step_planner.cpp:68-170) on four point feet (NF = 4,
// the quadrupeds' 24-slot plan) or two contact surfaces (NF = 2, the biped walk's 36-slot plan with its rotations).  Mapping: one
// lane per (instance, foot), FOOT-MAJOR within the wave -- lane l is foot l / (64 / NF) of instance (64 / NF) blockIdx.x + l % (64 / NF),
// 16 instances per wave for four feet and 32 for two -- so that a foot group's lanes write consecutive doubles of every [slot][batch]
// array.  What an instance shares across its feet (R, R_goal, R_yaw jump_length, the quaternion of R_goal) is computed redundantly by
// its lanes: no __shfl, no LDS, no atomics, and a lane beyond the batch returns at once and stores nothing.  The init runs in two
// phases around the second kinematics pass (JumpInitArgs::phase, wave-uniform): phase 0 writes q_goal[batch][nq], the kinematics
// then give CoM at q_goal, phase 1 writes the three steps and the q_ref of MPCJump::init (mpc_jump.cpp:141-145).  Every case of
// plan() is one wave-uniform flag (JumpPlanArgs::landed) the host decides; a tick that changes nothing launches nothing.
// Loads per lane, init: 7 doubles of q (a state apart) and 4 of the command (runs of 16 | 32 consecutive doubles); phase 1: 3 of
// its foot's position, NF = 2 also 9 of its rotation, from the kinematics' [batch][NF][3 | 9], and 3 + 3 of the two centres of
// mass; the nq / NF entries of q a lane copies lie NF apart.  Stores, phase 0: nq / NF doubles of q_goal; phase 1: per step what
// fs_store_step / fs_store_biped_step write (runs of 16 | 32 consecutive doubles per group and slot), three steps, and nq / NF
// doubles of q_ref.  Plan, landed: 3 (NF = 2: 12) doubles loaded from the kinematics and stored into steps 1 and 0; take-off: the
// 6 (NF = 2: 18) slots a lane owns of step 2 loaded and stored into step 1.
//
// foot_step_place_kernel / foot_step_refs_kernel.  Mapping: one lane per DOUBLE written, the doubles of an (instance, grid point)
// pair adjacent and the pairs in table order, so that a wave writes one contiguous run of 512 bytes whatever the record size: 12
// doubles per pair of the placement table (through RecView::placement), 13 per rtoc_task_ref_entry (its two ints as one 8-byte
// word), nq per row of the configuration reference.  The lanes of a pair recompute its few scalars (cycle, rate) from the same
// grid time.  Loads of the plan are gathers with the batch stride; the plan of a wave's instances is a few hundred bytes and
// stays in L2.  blockIdx.y of the refs kernel selects the table (wave-uniform).  No LDS, no atomics.  Both are templates over the
// number of feet (FsPlanLayout): <4> is the quadrupeds' form; <2> reads the biped walk's plan, tests "some contact is inactive"
// against 0b11, and its place form writes 6 + 18 doubles per pair, the translations into the position table and the rotations
// into the rotation table (two runs per wave, one per table).
//
// Included by rt_foot_steps.hip alone (a kernel header belongs to the unit that launches from it).
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "../../include/rtoc_robot.h"

namespace rtoc {

// ---- layouts, all [slot][batch] (the batch index innermost) ----
// plan: [step][FS_PLAN_SLOTS][batch]
constexpr int FS_PLAN_POS = 0;     // contactPositions(step)[4][3]
constexpr int FS_PLAN_COM = 12;    // CoM(step)[3]
constexpr int FS_PLAN_R = 15;      // R(step)[9] row-major
constexpr int FS_PLAN_SLOTS = 24;
// the biped walk's plan: [step][FS_BIPED_SLOTS][batch]
constexpr int FS_BIPED_POS = 0;    // contactPositions(step)[2][3]
constexpr int FS_BIPED_SURF = 6;   // contactSurfaces(step)[2][9] row-major
constexpr int FS_BIPED_COM = 24;   // CoM(step)[3]
constexpr int FS_BIPED_R = 27;     // R(step)[9] row-major (behind the CoM: the two lanes of an instance halve [CoM | R])
constexpr int FS_BIPED_SLOTS = 36;
// where the place and refs kernels find a gait's plan, by the number of feet
template <int NF> struct FsPlanLayout;
template <> struct FsPlanLayout<4> {
  static constexpr int POS = FS_PLAN_POS, COM = FS_PLAN_COM, R = FS_PLAN_R, SLOTS = FS_PLAN_SLOTS;
  static constexpr unsigned FULL = 0xFu;
};
template <> struct FsPlanLayout<2> {
  static constexpr int POS = FS_BIPED_POS, SURF = FS_BIPED_SURF, COM = FS_BIPED_COM, R = FS_BIPED_R, SLOTS = FS_BIPED_SLOTS;
  static constexpr unsigned FULL = 0x3u;
};
// planner state: [FS_STATE_SLOTS][batch]
constexpr int FS_ST_R = 0;         // R_.front(): the projected base rotation, advanced by every plan
constexpr int FS_ST_LOCAL = 9;     // com_to_contact_position_local_[4][3]
constexpr int FS_ST_LEGS = 9;      // the biped walk, in their place: left_to_right_leg_distance_, foot_height_to_com_height_
constexpr int FS_ST_HEIGHT = 10;
constexpr int FS_ST_LAST = 21;     // MovingWindowFilter: last_sampling_time_
constexpr int FS_ST_AVG = 22;      // average_[2]
constexpr int FS_ST_COUNT = 24;    // samples in the ring, and the slot of the oldest (both as doubles)
constexpr int FS_ST_HEAD = 25;
constexpr int FS_ST_STEP = 26;     // step_length_[3] in force (Raibert mode: what the heuristic planned)
constexpr int FS_ST_RING = 29;     // [FS_RING][3]: t, x, y
constexpr int FS_RING = 12;        // samples lie within time_length and >= 0.1 time_length apart: at most 11 alive, 12 during a push
constexpr int FS_STATE_SLOTS = FS_ST_RING + 3 * FS_RING;
// command: [FS_CMD_SLOTS][batch]
constexpr int FS_CMD_STEP = 0;     // fixed mode: step_length[3]
constexpr int FS_CMD_YAW = 3;      // step_yaw (Raibert mode: yaw_rate_cmd (swing_time + stance_time))
constexpr int FS_CMD_VCOM = 4;     // Raibert mode: vcom_cmd[0..1] (the heuristic reads the head<2>, :134)
constexpr int FS_CMD_SLOTS = 8;

struct FsInitArgs {
  const double* x0;      // [batch][nq + nv]
  const double* feet;    // [batch][4][3] world positions of the contact frames, com [batch][3] (contact_frame_placements_kernel)
  const double* com;     // (the biped walk: feet [batch][2][3])
  double* state;         // [FS_STATE_SLOTS][batch]
  double* plan;          // step 0 receives com_ref_[0] and R_[0]
  double* q0;            // [batch][nq]: the q the configuration reference starts from
  int batch, nq, nx;     // nx = nq + nv
  int projection;        // RTOC_PROJECT_*
};

struct FsPlanArgs {
  const double* x0;
  const double* feet;
  const double* feet_R;  // the biped walk alone: [batch][2][9] world rotations of the contact frames, row-major
  const double* cmd;     // [FS_CMD_SLOTS][batch]
  double* state;
  double* plan;
  int batch, nq, nx;
  int raibert;           // 1: the filter and the heuristic run first
  double t;              // Raibert mode: the sampling time, time_length = period, min_sampling_period = 0.1 period, gain
  double period, min_period, gain;
  // the case chain of the gait's plan() as the host resolved it (trot :145-277; plan_cases in rt_foot_steps.hip walks the gait's table)
  unsigned stance;       // feet on the ground now: two of a trot or pace, three of a crawl, all four, or none (flight)
  int pre_rotate;        // 1: R = R_yaw R ahead of the stance centre of mass (trot :165, :171, :186, :192)
  int nloop;             // passes of the loop: planning_steps + 1 (the flying trot: one more, which repeats the last step, :231-233)
  int incremental;       // 1: a stepping foot advances from where it is, p += foot_scale R step_length (the crawl); 0: p = com + R local
  int flight;            // 1: nothing on the ground (the flying trot, :176-183): the CoM and the footholds are step 0 of the previous plan
  unsigned char move[RTOC_MAX_PLAN_STEPS + 4];   // per pass: the feet that step, or 0 (nothing moves, nothing turns)
  double com_scale[RTOC_MAX_PLAN_STEPS + 4];     // per pass: the CoM's share of step_length_ (trot: 0.5; on the first step of all 0.5 with
                                                 // the heuristic, 0.25 without, :219-224)
  double foot_scale[RTOC_MAX_PLAN_STEPS + 4];    // per pass, incremental alone: the stepping foot's share (crawl: 1, 0.5 on its two first steps)
};

static __device__ __forceinline__ rbd::M3 fs_yaw_times(double s, double c, const rbd::M3& R) {
  rbd::M3 out;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    out.m[j] = c * R.m[j] - s * R.m[3 + j];
    out.m[3 + j] = s * R.m[j] + c * R.m[3 + j];
    out.m[6 + j] = R.m[6 + j];
  }
  return out;
}
// what every lane of an instance stores of a plan step: its foot's position, and its quarter of [CoM | R]
static __device__ __forceinline__ void fs_store_step(double* plan, int step, int B, int b, int f, rbd::V3 p, rbd::V3 com, const rbd::M3& R) {
  double* const s = plan + (size_t)step * FS_PLAN_SLOTS * B + b;
  s[(size_t)(FS_PLAN_POS + 3 * f) * B] = p.x, s[(size_t)(FS_PLAN_POS + 3 * f + 1) * B] = p.y, s[(size_t)(FS_PLAN_POS + 3 * f + 2) * B] = p.z;
  // (selects, not an index into R: the rotation stays in registers)
  const double w0 = f == 0 ? com.x : f == 1 ? R.m[0] : f == 2 ? R.m[3] : R.m[6];
  const double w1 = f == 0 ? com.y : f == 1 ? R.m[1] : f == 2 ? R.m[4] : R.m[7];
  const double w2 = f == 0 ? com.z : f == 1 ? R.m[2] : f == 2 ? R.m[5] : R.m[8];
  s[(size_t)(FS_PLAN_COM + 3 * f) * B] = w0, s[(size_t)(FS_PLAN_COM + 3 * f + 1) * B] = w1, s[(size_t)(FS_PLAN_COM + 3 * f + 2) * B] = w2;
}

// the base rotation of q projected onto the z axis, as every planner's init does first (RTOC_PROJECT_*)
static __device__ __forceinline__ rbd::M3 fs_projected_base_rotation(const double* q, int projection) {
  using namespace rbd;
  M3 R = quat_R(q + 3);
  if (projection == RTOC_PROJECT_YAW) {
    const double th = atan2(R.m[3], R.m[0]), s = sin(th), c = cos(th);
    R.m[0] = c, R.m[1] = -s, R.m[3] = s, R.m[4] = c;
  } else {
    // rotation::ProjectRotationMatrix(R, Z) as it stands (rotation.hpp:103-111): not the norm of the row
    const double norm = R.m[0] * R.m[0] + R.m[1] + R.m[1];
#pragma unroll
    for (int k = 0; k < 9; ++k) R.m[k] /= norm;
  }
  R.m[2] = 0.0, R.m[5] = 0.0, R.m[6] = 0.0, R.m[7] = 0.0, R.m[8] = 1.0;
  return R;
}

// Quaterniond(R): Eigen's conversion (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), q = (x, y, z, w)
// One copy for the refs kernel (R(phase) of the plan) and the jump's init (R_goal)
static __device__ __forceinline__ void fs_eigen_quat(const rbd::M3& M, double* q) {
  const double* const m = M.m;
  double t = m[0] + m[4] + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t, q[1] = (m[2] - m[6]) * t, q[2] = (m[3] - m[1]) * t;
  } else {
    // i = the largest diagonal entry as Eigen picks it, j = (i + 1) % 3, k = (j + 1) % 3; the three cases written out, so that
    // nothing is indexed by a register
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
    if (i == 0) {
      t = sqrt(m[0] - m[4] - m[8] + 1.0);
      q[0] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[7] - m[5]) * t, q[1] = (m[3] + m[1]) * t, q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
      t = sqrt(m[4] - m[8] - m[0] + 1.0);
      q[1] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[2] - m[6]) * t, q[2] = (m[7] + m[5]) * t, q[0] = (m[1] + m[3]) * t;
    } else {
      t = sqrt(m[8] - m[0] - m[4] + 1.0);
      q[2] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[3] - m[1]) * t, q[0] = (m[2] + m[6]) * t, q[1] = (m[5] + m[7]) * t;
    }
  }
}

// R(step) of a plan: nine doubles a batch apart
static __device__ __forceinline__ rbd::M3 fs_load_plan_R(const double* plan_R, size_t B) {
  rbd::M3 M;
#pragma unroll
  for (int k = 0; k < 9; ++k) M.m[k] = plan_R[(size_t)k * B];
  return M;
}

// TrotFootStepPlanner::init(q) (:91-106) at the q of rtoc_set_initial_state
static __global__ __launch_bounds__(64) void foot_step_init_kernel(FsInitArgs a) {
  using namespace rbd;
  const int lane = threadIdx.x, f = lane >> 4, B = a.batch;
  const int b = blockIdx.x * 16 + (lane & 15);
  if (b >= B) return;
  const double* const q = a.x0 + (size_t)b * a.nx;
  const M3 R = fs_projected_base_rotation(q, a.projection);
  const V3 com = ldv3(a.com + (size_t)b * 3);
  const V3 foot = ldv3(a.feet + (size_t)b * 12 + 3 * f);
  const V3 local = mulT(R, foot - com);
  double* const st = a.state + b;
  st[(size_t)(FS_ST_LOCAL + 3 * f) * B] = local.x, st[(size_t)(FS_ST_LOCAL + 3 * f + 1) * B] = local.y, st[(size_t)(FS_ST_LOCAL + 3 * f + 2) * B] = local.z;
  if (f == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) st[(size_t)(FS_ST_R + k) * B] = R.m[k];
    for (int k = FS_ST_LAST; k < FS_ST_RING; ++k) st[(size_t)k * B] = 0.0;   // vcom_moving_window_filter_.clear(); no step length yet
  }
  // com_ref_[0] and R_[0] (:101-103) where the plan keeps them (beside them: where the feet are now; the plan's size stays 0)
  fs_store_step(a.plan, 0, B, b, f, foot, com, R);
  for (int k = f; k < a.nq; k += 4) a.q0[(size_t)b * a.nq + k] = q[k];
}

// ---- MovingWindowFilter::push_back (:113-135), RaibertHeuristic::planStepLength (raibert_heuristic.cpp:50-55), the head of every
// gait's plan(): one copy for foot_step_plan_kernel and biped_walk_plan_kernel.  st, cmd: the state and the command at instance b ----
struct FsFilter {
  double last = 0.0, ax = 0.0, ay = 0.0, t = 0.0, x = 0.0, y = 0.0;
  int count = 0, head = 0, slot = 0;
  bool push = false;
};
static __device__ __forceinline__ rbd::V3 fs_filter_step_length(const FsPlanArgs& a, const double* st, const double* cmd, int b, FsFilter& F) {
  const int B = a.batch;
  const double* const v = a.x0 + (size_t)b * a.nx + a.nq;   // vcom_ = v.head<3>() (:131)
  F.t = a.t, F.x = v[0], F.y = v[1];
  F.last = st[(size_t)FS_ST_LAST * B], F.ax = st[(size_t)FS_ST_AVG * B], F.ay = st[(size_t)(FS_ST_AVG + 1) * B];
  F.count = (int)st[(size_t)FS_ST_COUNT * B], F.head = (int)st[(size_t)FS_ST_HEAD * B];
  if (F.count == 0) {
    F.push = true, F.slot = 0, F.head = 0, F.count = 1;
    F.ax = F.x, F.ay = F.y, F.last = F.t;
  } else if (F.t - F.last >= a.min_period) {
    F.push = true;
    if (F.count == FS_RING) F.head = (F.head + 1) % FS_RING, --F.count;   // cannot happen with the window's own spacing
    F.slot = (F.head + F.count) % FS_RING;
    // pop_front while the front is older than the window (the new sample is never popped: t - t = 0)
    while (F.count > 0 && F.t - st[(size_t)(FS_ST_RING + 3 * F.head) * B] > a.period) F.head = (F.head + 1) % FS_RING, --F.count;
    double sx = 0.0, sy2 = 0.0;
    for (int k = 0; k < F.count; ++k) {
      const int slot = (F.head + k) % FS_RING;
      sx += st[(size_t)(FS_ST_RING + 3 * slot + 1) * B], sy2 += st[(size_t)(FS_ST_RING + 3 * slot + 2) * B];
    }
    sx += F.x, sy2 += F.y;
    ++F.count;
    F.ax = sx / F.count, F.ay = sy2 / F.count, F.last = F.t;
  }
  const double pg = a.period * a.gain;
  return rbd::mk(a.period * F.ax + pg * (cmd[(size_t)FS_CMD_VCOM * B] - F.ax), a.period * F.ay + pg * (cmd[(size_t)(FS_CMD_VCOM + 1) * B] - F.ay), 0.0);
}
// the filter's part of the state the next tick starts from; after the last load of the call
static __device__ __forceinline__ void fs_filter_store(double* st, int B, const FsFilter& F) {
  if (!F.push) return;
  st[(size_t)(FS_ST_RING + 3 * F.slot) * B] = F.t, st[(size_t)(FS_ST_RING + 3 * F.slot + 1) * B] = F.x, st[(size_t)(FS_ST_RING + 3 * F.slot + 2) * B] = F.y;
  st[(size_t)FS_ST_LAST * B] = F.last, st[(size_t)FS_ST_AVG * B] = F.ax, st[(size_t)(FS_ST_AVG + 1) * B] = F.ay;
  st[(size_t)FS_ST_COUNT * B] = (double)F.count, st[(size_t)FS_ST_HEAD * B] = (double)F.head;
}

// TrotFootStepPlanner::plan (:125-284), and with other arguments PaceFootStepPlanner::plan (:124-283), CrawlFootStepPlanner::plan
// (:123-366) and FlyingTrotFootStepPlanner::plan (:118-240): the filter, the heuristic, the stance sum and the stores are shared
static __global__ __launch_bounds__(64) void foot_step_plan_kernel(FsPlanArgs a) {
  using namespace rbd;
  const int lane = threadIdx.x, f = lane >> 4, B = a.batch;
  const int bl = lane & 15;
  const int b_raw = blockIdx.x * 16 + bl;
  const bool valid = b_raw < B;
  const int b = valid ? b_raw : B - 1;   // the lanes beyond the batch follow the last instance (the shuffles need every lane) and store nothing
  double* const st = a.state + b;
  M3 R;
#pragma unroll
  for (int k = 0; k < 9; ++k) R.m[k] = st[(size_t)(FS_ST_R + k) * B];
  const V3 local = mk(st[(size_t)(FS_ST_LOCAL + 3 * f) * B], st[(size_t)(FS_ST_LOCAL + 3 * f + 1) * B], st[(size_t)(FS_ST_LOCAL + 3 * f + 2) * B]);
  const double* const cmd = a.cmd + b;
  V3 sl = mk(cmd[(size_t)FS_CMD_STEP * B], cmd[(size_t)(FS_CMD_STEP + 1) * B], cmd[(size_t)(FS_CMD_STEP + 2) * B]);
  const double yaw = cmd[(size_t)FS_CMD_YAW * B];
  const double sy = sin(yaw), cy = cos(yaw);
  FsFilter flt;
  if (a.raibert) sl = fs_filter_step_length(a, st, cmd, b, flt);
  V3 p = ldv3(a.feet + (size_t)b * 12 + 3 * f);
  V3 com = mk(0, 0, 0);
  if (a.flight) {
    // ---- nothing on the ground: carried over from step 0 of the previous plan, loaded ahead of every store of this call ----
    const double* const s0 = a.plan + b;
    p = mk(s0[(size_t)(FS_PLAN_POS + 3 * f) * B], s0[(size_t)(FS_PLAN_POS + 3 * f + 1) * B], s0[(size_t)(FS_PLAN_POS + 3 * f + 2) * B]);
    com = mk(s0[(size_t)FS_PLAN_COM * B], s0[(size_t)(FS_PLAN_COM + 1) * B], s0[(size_t)(FS_PLAN_COM + 2) * B]);
  } else {
    // ---- the feet on the ground fix the centre of mass (:145-202) ----
    if (a.pre_rotate) R = fs_yaw_times(sy, cy, R);
    const V3 r = mul(R, local);
    int n = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int src = g * 16 + bl;
      const V3 pg = mk(__shfl(p.x, src, 64), __shfl(p.y, src, 64), __shfl(p.z, src, 64));
      const V3 rg = mk(__shfl(r.x, src, 64), __shfl(r.y, src, 64), __shfl(r.z, src, 64));
      if ((a.stance >> g) & 1u) com = (com + pg) - rg, ++n;
    }
    com = mk(com.x / n, com.y / n, com.z / n);
    if (!((a.stance >> f) & 1u)) p = com + mul(R, local - 0.5 * sl);
  }
  if (valid) {
    fs_store_step(a.plan, 0, B, b, f, p, com, R);
    if (f == 0) {
      // the state the next tick starts from: R_.front(), the filter, the step length in force
#pragma unroll
      for (int k = 0; k < 9; ++k) st[(size_t)(FS_ST_R + k) * B] = R.m[k];
      st[(size_t)FS_ST_STEP * B] = sl.x, st[(size_t)(FS_ST_STEP + 1) * B] = sl.y, st[(size_t)(FS_ST_STEP + 2) * B] = sl.z;
      fs_filter_store(st, B, flt);
    }
  }
  // ---- the steps ahead (:212-277) ----
  for (int s = 0; s < a.nloop; ++s) {
    const unsigned mv = a.move[s];
    if (mv) {
      R = fs_yaw_times(sy, cy, R);
      const V3 d = mul(R, sl);
      com = com + a.com_scale[s] * d;
      if ((mv >> f) & 1u) p = a.incremental ? p + a.foot_scale[s] * d : com + mul(R, local);
    }
    if (valid) fs_store_step(a.plan, s + 1, B, b, f, p, com, R);
  }
}

// ---- BipedWalkFootStepPlanner (src/mpc/biped_walk_foot_step_planner.cpp) ----
// what the lane of foot f stores of a plan step: its foot's translation and rotation, and its half of [CoM | R]
static __device__ __forceinline__ void fs_store_biped_step(double* plan, int step, int B, int b, int f, rbd::V3 p, const rbd::M3& S, rbd::V3 com,
                                                           const rbd::M3& R) {
  double* const s = plan + (size_t)step * FS_BIPED_SLOTS * B + b;
  s[(size_t)(FS_BIPED_POS + 3 * f) * B] = p.x, s[(size_t)(FS_BIPED_POS + 3 * f + 1) * B] = p.y, s[(size_t)(FS_BIPED_POS + 3 * f + 2) * B] = p.z;
#pragma unroll
  for (int k = 0; k < 9; ++k) s[(size_t)(FS_BIPED_SURF + 9 * f + k) * B] = S.m[k];
  // (selects, not an index into R: the rotation stays in registers)
  const double w[6] = {f == 0 ? com.x : R.m[3], f == 0 ? com.y : R.m[4], f == 0 ? com.z : R.m[5],
                       f == 0 ? R.m[0] : R.m[6], f == 0 ? R.m[1] : R.m[7], f == 0 ? R.m[2] : R.m[8]};
#pragma unroll
  for (int k = 0; k < 6; ++k) s[(size_t)(FS_BIPED_COM + 6 * f + k) * B] = w[k];
}

// init(q) (:89-108) at the q of rtoc_set_initial_state.  The plan is left alone: com_ref_ is cleared there, not seeded
static __global__ __launch_bounds__(64) void biped_walk_init_kernel(FsInitArgs a) {
  using namespace rbd;
  const int lane = threadIdx.x, f = lane >> 5, B = a.batch;
  const int b_raw = blockIdx.x * 32 + (lane & 31);
  const bool valid = b_raw < B;
  const int b = valid ? b_raw : B - 1;   // the lanes beyond the batch follow the last instance (the shuffles need every lane) and store nothing
  const double* const q = a.x0 + (size_t)b * a.nx;
  const M3 R = fs_projected_base_rotation(q, a.projection);
  const V3 foot = ldv3(a.feet + (size_t)b * 6 + 3 * f);
  const V3 local = mulT(R, foot - ldv3(q));   // relative to the base, q.head<3>() (:94-95)
  const double other_y = __shfl(local.y, lane ^ 32, 64), other_z = __shfl(foot.z, lane ^ 32, 64);
  const double distance = f == 0 ? local.y - other_y : other_y - local.y;                        // :96-97: left - right
  const double foot_height = 0.5 * (f == 0 ? foot.z + other_z : other_z + foot.z);               // :98-99
  const double height = a.com[(size_t)b * 3 + 2] - foot_height;                                  // :100
  if (!valid) return;
  if (f == 0) {
    double* const st = a.state + b;
#pragma unroll
    for (int k = 0; k < 9; ++k) st[(size_t)(FS_ST_R + k) * B] = R.m[k];
    st[(size_t)FS_ST_LEGS * B] = distance, st[(size_t)FS_ST_HEIGHT * B] = height;
    for (int k = FS_ST_LAST; k < FS_ST_RING; ++k) st[(size_t)k * B] = 0.0;   // vcom_moving_window_filter_.clear(); no step length yet
  }
  for (int k = f; k < a.nq; k += 2) a.q0[(size_t)b * a.nq + k] = q[k];
}

// plan (:111-277)
static __global__ __launch_bounds__(64) void biped_walk_plan_kernel(FsPlanArgs a) {
  using namespace rbd;
  const int lane = threadIdx.x, f = lane >> 5, B = a.batch;
  const int other = lane ^ 32;
  const int b_raw = blockIdx.x * 32 + (lane & 31);
  const bool valid = b_raw < B;
  const int b = valid ? b_raw : B - 1;
  double* const st = a.state + b;
  M3 R;
#pragma unroll
  for (int k = 0; k < 9; ++k) R.m[k] = st[(size_t)(FS_ST_R + k) * B];
  const double distance = st[(size_t)FS_ST_LEGS * B], height = st[(size_t)FS_ST_HEIGHT * B];
  const double* const cmd = a.cmd + b;
  V3 sl = mk(cmd[(size_t)FS_CMD_STEP * B], cmd[(size_t)(FS_CMD_STEP + 1) * B], cmd[(size_t)(FS_CMD_STEP + 2) * B]);
  const double yaw = cmd[(size_t)FS_CMD_YAW * B];
  const double sy = sin(yaw), cy = cos(yaw);
  FsFilter flt;
  if (a.raibert) sl = fs_filter_step_length(a, st, cmd, b, flt);   // :116-123
  // ---- this tick's kinematics: both feet with their full frame rotations (:124-128) ----
  const V3 base = ldv3(a.x0 + (size_t)b * a.nx);
  V3 p = ldv3(a.feet + (size_t)b * 6 + 3 * f);
  M3 S = ldm3(a.feet_R + (size_t)b * 18 + 9 * f);
  V3 po = mk(__shfl(p.x, other, 64), __shfl(p.y, other, 64), __shfl(p.z, other, 64));
  if (a.stance != 0x3u) {
    // ---- single support (:148-191): the swing foot from the stance foot's offset in R_.front() (:131-135), then the turn ----
    V3 loc = mulT(R, po - base);
    if (a.pre_rotate) R = fs_yaw_times(sy, cy, R);
    const V3 back = mk(cy * sl.x + sy * sl.y, cy * sl.y - sy * sl.x, sl.z);   // R_yaw^T step_length_
    loc = loc - 0.5 * back;
    loc.y += f == 1 ? -distance : distance;   // :163 the right foot, :185 the left
    if (!((a.stance >> f) & 1u)) p = mul(R, loc) + base, S = R;
    po = mk(__shfl(p.x, other, 64), __shfl(p.y, other, 64), __shfl(p.z, other, 64));
  }
  // com = 0.5 (left + right), the stored height on top (:145-146, :167-168, :189-190)
  V3 com = 0.5 * (f == 0 ? p + po : po + p);
  com.z += height;
  if (valid) {
    fs_store_biped_step(a.plan, 0, B, b, f, p, S, com, R);
    if (f == 0) {
      // the state the next tick starts from: R_.front(), the filter, the step length in force
#pragma unroll
      for (int k = 0; k < 9; ++k) st[(size_t)(FS_ST_R + k) * B] = R.m[k];
      st[(size_t)FS_ST_STEP * B] = sl.x, st[(size_t)(FS_ST_STEP + 1) * B] = sl.y, st[(size_t)(FS_ST_STEP + 2) * B] = sl.z;
      fs_filter_store(st, B, flt);
    }
  }
  // ---- the steps ahead (:201-266): the moving foot advances from where it is and takes R ----
  for (int s = 0; s < a.nloop; ++s) {
    const unsigned mv = a.move[s];
    if (mv) {
      R = fs_yaw_times(sy, cy, R);
      const V3 d = mul(R, sl);
      com = com + a.com_scale[s] * d;
      if ((mv >> f) & 1u) p = p + a.foot_scale[s] * d, S = R;
    }
    if (valid) fs_store_biped_step(a.plan, s + 1, B, b, f, p, S, com, R);
  }
}

// ---- JumpFootStepPlanner (src/mpc/jump_foot_step_planner.cpp) ----
struct JumpInitArgs {
  const double* x0;        // [batch][nq + nv]
  const double* cmd;       // [FS_CMD_SLOTS][batch]: jump_length in FS_CMD_STEP, the yaw in FS_CMD_YAW
  const double* feet;      // phase 1: [batch][NF][3] world positions of the contact frames at q
  const double* feet_R;    // phase 1, NF = 2: [batch][2][9] their rotations, row-major
  const double* com;       // phase 1: [batch][3] the centre of mass at q ...
  const double* com_goal;  // ... and at q_goal (the second kinematics pass)
  double* plan;            // phase 1: steps 0, 1, 2
  double* qgoal;           // phase 0: [batch][nq] q_goal, which the second kinematics pass reads
  double* qref;            // phase 1: [batch][nq] the q_ref of MPCJump::init (mpc_jump.cpp:141-145)
  int batch, nq, nx;       // nx = nq + nv
  int projection;          // RTOC_PROJECT_*
  int phase;               // 0: q_goal alone; 1: the plan and q_ref (wave-uniform)
};
// init(q) (:68-124) at the q of rtoc_set_initial_state, around the second kinematics pass.  Both phases derive R, R_goal = R_yaw R,
// R_yaw jump_length and Quaterniond(R_goal) from the same loads by the same arithmetic, so q_goal and the plan agree to the bit
template <int NF>
static __global__ __launch_bounds__(64) void jump_init_kernel(JumpInitArgs a) {
  using namespace rbd;
  constexpr int PER = 64 / NF;   // instances per wave
  const int lane = threadIdx.x, f = lane / PER, B = a.batch;
  const int b = blockIdx.x * PER + lane % PER;
  if (b >= B) return;   // no lane reads another's registers
  const double* const q = a.x0 + (size_t)b * a.nx;
  const double* const cmd = a.cmd + b;
  const V3 jl = mk(cmd[(size_t)FS_CMD_STEP * B], cmd[(size_t)(FS_CMD_STEP + 1) * B], cmd[(size_t)(FS_CMD_STEP + 2) * B]);
  const double yaw = cmd[(size_t)FS_CMD_YAW * B];
  const double sy = sin(yaw), cy = cos(yaw);
  const M3 R = fs_projected_base_rotation(q, a.projection);   // :69-70
  const M3 Rg = fs_yaw_times(sy, cy, R);                       // R_goal (:82)
  const V3 hop = mk(cy * jl.x - sy * jl.y, sy * jl.x + cy * jl.y, jl.z);   // R_yaw_ jump_length_
  double qg[4];
  fs_eigen_quat(Rg, qg);   // :83, and Quaterniond(R(2)) of mpc_jump.cpp:144: the same matrix
  V3 shift = hop;          // what the head<3>() of q moves by: q_goal (:85); q_ref: CoM(2) - CoM(0)
  V3 com0 = mk(0, 0, 0), com2 = mk(0, 0, 0);
  if (a.phase == 1) {
    com0 = ldv3(a.com + (size_t)b * 3), com2 = ldv3(a.com_goal + (size_t)b * 3);
    shift = com2 - com0;
  }
  // ---- q_goal or q_ref: q with the head moved and the quaternion replaced (not normalised, as in the reference) ----
  double* const qout = (a.phase == 0 ? a.qgoal : a.qref) + (size_t)b * a.nq;
  for (int k = f; k < a.nq; k += NF) {
    double x = q[k];
    if (k < 3)
      x += k == 0 ? shift.x : k == 1 ? shift.y : shift.z;
    else if (k < 7)
      x = k == 3 ? qg[0] : k == 4 ? qg[1] : k == 5 ? qg[2] : qg[3];
    qout[k] = x;
  }
  if (a.phase == 0) return;
  // ---- the three steps (:72-122): where the feet are, twice, and the goal ----
  const V3 base = ldv3(q);
  const V3 p = ldv3(a.feet + ((size_t)b * NF + f) * 3);
  const V3 local = mulT(R, p - base);            // :80
  const V3 goal = (base + mul(Rg, local)) + hop; // :92-93
  if constexpr (NF == 4) {
    // point feet: every rotation is the identity (:99-105), which the 24-slot layout leaves unwritten
    fs_store_step(a.plan, 0, B, b, f, p, com0, R);
    fs_store_step(a.plan, 1, B, b, f, p, com0, R);
    fs_store_step(a.plan, 2, B, b, f, goal, com2, Rg);
  } else {
    const M3 S = ldm3(a.feet_R + ((size_t)b * NF + f) * 9);
    const M3 Sg = mul(Rg, mul(transpose(R), S));   // R_goal (R^T R_k) (:79, :91)
    fs_store_biped_step(a.plan, 0, B, b, f, p, S, com0, R);
    fs_store_biped_step(a.plan, 1, B, b, f, p, S, com0, R);
    fs_store_biped_step(a.plan, 2, B, b, f, goal, Sg, com2, Rg);
  }
}

struct JumpPlanArgs {
  const double* feet;    // landed: [batch][NF][3] this tick's kinematics at q
  const double* feet_R;  // landed, NF = 2: [batch][2][9]
  double* plan;
  int batch;
  int landed;            // 1: feet on the ground (:132-148); 0: the first tick of the flight (:150-158).  Wave-uniform
};
// plan (:127-170).  The host resolved the case; a tick that changes nothing launches nothing
template <int NF>
static __global__ __launch_bounds__(64) void jump_plan_kernel(JumpPlanArgs a) {
  using L = FsPlanLayout<NF>;
  constexpr int PER = 64 / NF;
  constexpr int SHARE = NF == 4 ? 3 : 6;   // a lane's part of [CoM | R]
  const int lane = threadIdx.x, f = lane / PER, B = a.batch;
  const int b = blockIdx.x * PER + lane % PER;
  if (b >= B) return;
  double* const s0 = a.plan + b;
  double* const s1 = s0 + (size_t)L::SLOTS * B;
  if (a.landed) {
    // step 1 <- the kinematics (a biped: the frame placement; a quadruped: the translation, its rotation stays); step 0 <- step 1
    const double* const p = a.feet + ((size_t)b * NF + f) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = p[k];
      s1[(size_t)(L::POS + 3 * f + k) * B] = x, s0[(size_t)(L::POS + 3 * f + k) * B] = x;
    }
    if constexpr (NF == 2) {
      const double* const S = a.feet_R + ((size_t)b * NF + f) * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double x = S[k];
        s1[(size_t)(L::SURF + 9 * f + k) * B] = x, s0[(size_t)(L::SURF + 9 * f + k) * B] = x;
      }
    }
  } else {
    // step 1 <- step 2: placements, CoM and R (:152-157); the host shrinks the plan to two steps.  A lane moves the slots it owns
    const double* const s2 = s1 + (size_t)L::SLOTS * B;
#pragma unroll
    for (int k = 0; k < 3; ++k) s1[(size_t)(L::POS + 3 * f + k) * B] = s2[(size_t)(L::POS + 3 * f + k) * B];
    if constexpr (NF == 2) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s1[(size_t)(L::SURF + 9 * f + k) * B] = s2[(size_t)(L::SURF + 9 * f + k) * B];
    }
#pragma unroll
    for (int k = 0; k < SHARE; ++k) s1[(size_t)(L::COM + SHARE * f + k) * B] = s2[(size_t)(L::COM + SHARE * f + k) * B];
  }
}

// rtoc_foot_step_refs of the jump: every grid row of the per-instance q_ref table <- the stored q_ref, active everywhere.  One lane
// per double written, as foot_step_refs_kernel has it
struct JumpRefsArgs {
  const double* qref;    // [batch][nq]
  double* qtab;          // [batch][nstages][nq]
  int* qtab_active;      // [batch][nstages]
  int batch, nstages, nq;
};
static __global__ __launch_bounds__(256) void jump_refs_kernel(JumpRefsArgs a) {
  const int n = a.nstages, nq = a.nq;
  const size_t total = (size_t)a.batch * n * nq;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % nq), st = (int)((e / nq) % n), b = (int)(e / nq / n);
    if (k == 0) a.qtab_active[(size_t)b * n + st] = 1;
    a.qtab[e] = a.qref[(size_t)b * nq + k];
  }
}

// the loop of MPCTrot::resetContactPlacements (mpc_trot.cpp:361-365): grid point i <- contactPositions(phase_i + 1); NF = 2, the
// loop of MPCBipedWalk::resetContactPlacements (mpc_biped_walk.cpp:347-359): contactPlacements(phase_i + 1), rotations included
struct FsPlaceArgs {
  RecView rv;            // placement() of the per-instance table
  const double* plan;
  const int* phase;      // [nstages] GridInfo::phase relative to the first grid point
  double* tab_pos;       // [batch][nstages][NF][3]
  double* tab_rot;       // NF = 2 alone: [batch][nstages][2][9]
};
template <int NF>
static __global__ __launch_bounds__(256) void foot_step_place_kernel(FsPlaceArgs a) {
  using L = FsPlanLayout<NF>;
  constexpr int PER = NF == 4 ? 12 : 24;   // doubles per (instance, grid point): [NF][3], and for surface contacts [NF][9] behind them
  const int B = a.rv.batch, n = a.rv.nstages;
  const size_t total = (size_t)B * n * PER;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % PER), st = (int)((e / PER) % n), b = (int)(e / PER / n);
    const int step = a.phase[st] + 1;
    const double* const src = a.plan + (size_t)step * L::SLOTS * B + b;
    if constexpr (NF == 4) {
      a.tab_pos[a.rv.placement(b, st, 4, k / 3) * 3 + k % 3] = src[(size_t)(L::POS + k) * B];
    } else {
      const int r = k - 3 * NF;
      if (r < 0)
        a.tab_pos[a.rv.placement(b, st, NF, k / 3) * 3 + k % 3] = src[(size_t)(L::POS + k) * B];
      else
        a.tab_rot[a.rv.placement(b, st, NF, r / 9) * 9 + r % 9] = src[(size_t)(L::SURF + r) * B];
    }
  }
}

// MPCPeriodicSwingFootRef (mpc_periodic_swing_foot_ref.cpp:90-110), MPCPeriodicCoMRef (mpc_periodic_com_ref.cpp:90-110),
// MPCPeriodicConfigurationRef (mpc_periodic_configuration_ref.cpp:92-115) at every (instance, grid point)
struct FsPeriod {
  double t0, period_active, period_inactive, height;   // swing_start_time, period_swing | period_active, period_stance | period_inactive, swing_height
  int nph, on;                                         // num_phases_in_period; 0: this reference is left out
};
struct FsRefsArgs {
  const double* plan;
  const double* q0;          // [batch][nq]
  const double* t;           // [nstages] grid times
  const int* phase;          // [nstages]
  const unsigned* masks;     // [nphases] active contacts of every contact phase
  rtoc_task_ref_entry* tab[5];   // feet 0..3 (the biped walk: 0..1), CoM: [batch][nstages] or nullptr
  double* qtab;              // [batch][nstages][nq] or nullptr
  int* qtab_active;          // [batch][nstages]
  FsPeriod per[6];           // feet 0..3, CoM, configuration
  int batch, nstages, nq;
};
constexpr int FS_ENTRY_WORDS = (int)(sizeof(rtoc_task_ref_entry) / 8);   // 9 R, 3 p, 1 (active, pad)
static_assert(sizeof(rtoc_task_ref_entry) == 13 * 8, "an entry is written as 13 eight-byte words");

template <int NF>
static __global__ __launch_bounds__(256) void foot_step_refs_kernel(FsRefsArgs a) {
  using L = FsPlanLayout<NF>;
  const int which = blockIdx.y, B = a.batch, n = a.nstages;
  const FsPeriod pr = a.per[which];
  if (!pr.on) return;
  const double period = pr.period_active + pr.period_inactive;
  if (which < 5) {
    // ---- a table of rtoc_task_ref_entry: R = identity (a 3D / CoM term reads p alone), p, (active, pad = 0) ----
    unsigned long long* const out = (unsigned long long*)a.tab[which];
    const size_t total = (size_t)B * n * FS_ENTRY_WORDS;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
      const int w = (int)(e % FS_ENTRY_WORDS), st = (int)((e / FS_ENTRY_WORDS) % n), b = (int)(e / FS_ENTRY_WORDS / n);
      const int ph = a.phase[st];
      const double t = a.t[st];
      const unsigned mask = a.masks[ph];
      // isActive: the foot swings (:107-110) / some foot is in the air (mpc_periodic_com_ref.cpp:106-108)
      const bool active = t > pr.t0 && (which < 4 ? !((mask >> which) & 1u) : (mask & L::FULL) != L::FULL);
      if (w < 9) {
        out[e] = (unsigned long long)__double_as_longlong((w % 4 == 0) ? 1.0 : 0.0);
      } else if (w == 12) {
        out[e] = active ? 1ull : 0ull;   // little endian: active in the low word, pad = 0
      } else {
        const int k = w - 9;
        const int slot = which < 4 ? L::POS + 3 * which + k : L::COM + k;
        const double x0 = a.plan[((size_t)ph * L::SLOTS + slot) * B + b];
        double x = x0;   // inactive: the CoM reference's else branch (:100-102); a swing-foot reference is not updated, this stands in
        if (active) {
          const int cycle = (int)floor((t - pr.t0) / period);
          const double rate = (t - pr.t0 - cycle * period) / pr.period_active;
          const double x1 = a.plan[((size_t)(ph + pr.nph) * L::SLOTS + slot) * B + b];
          x = (1.0 - rate) * x0 + rate * x1;
          if (which < 4 && k == 2) x += (rate < 0.5) ? 2 * rate * pr.height : 2 * (1 - rate) * pr.height;
        }
        out[e] = (unsigned long long)__double_as_longlong(x);
      }
    }
    return;
  }
  // ---- the configuration reference: q of the planner's init with the base quaternion slerped between R(phase), R(phase + nph) ----
  const int nq = a.nq;
  const size_t total = (size_t)B * n * nq;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % nq), st = (int)((e / nq) % n), b = (int)(e / nq / n);
    if (k == 0) a.qtab_active[(size_t)b * n + st] = 1;   // isActive: everywhere (:111-115)
    double x = a.q0[(size_t)b * nq + k];
    if (k >= 3 && k < 7) {
      const int ph = a.phase[st];
      const double t = a.t[st];
      double qa[4];
      fs_eigen_quat(fs_load_plan_R(a.plan + ((size_t)ph * L::SLOTS + L::R) * B + b, B), qa);
      const int c = k - 3;
      const double xa = c == 0 ? qa[0] : c == 1 ? qa[1] : c == 2 ? qa[2] : qa[3];
      x = xa;
      if (t > pr.t0 && (a.masks[ph] & L::FULL) != L::FULL) {
        const int cycle = (int)floor((t - pr.t0) / period);
        const double rate = (t - pr.t0 - cycle * period) / pr.period_active;
        double qb[4];
        fs_eigen_quat(fs_load_plan_R(a.plan + ((size_t)(ph + pr.nph) * L::SLOTS + L::R) * B + b, B), qb);
        // Eigen's slerp (QuaternionBase::slerp): the near-parallel branch, the sign flip of the shorter arc
        const double one = 1.0 - 2.220446049250313e-16;
        const double d = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3];
        const double ad = fabs(d);
        double s0, s1;
        if (ad >= one) {
          s0 = 1.0 - rate, s1 = rate;
        } else {
          const double theta = acos(ad), sin_theta = sin(theta);
          s0 = sin((1.0 - rate) * theta) / sin_theta;
          s1 = sin(rate * theta) / sin_theta;
        }
        if (d < 0.0) s1 = -s1;
        const double xb = c == 0 ? qb[0] : c == 1 ? qb[1] : c == 2 ? qb[2] : qb[3];
        x = s0 * xa + s1 * xb;
      }
    }
    a.qtab[e] = x;
  }
}

}  // namespace rtoc
