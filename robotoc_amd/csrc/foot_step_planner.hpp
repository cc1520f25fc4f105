// foot_step_planner.hpp -- TrotFootStepPlanner (src/mpc/trot_foot_step_planner.cpp) with its RaibertHeuristic
// (src/mpc/raibert_heuristic.cpp) and MovingWindowFilter<2> (include/robotoc/mpc/moving_window_filter.hpp), and what
// MPCTrot::resetContactPlacements (src/mpc/mpc_trot.cpp:357-372) does with the plan -- the placements of every contact phase,
// MPCPeriodicSwingFootRef x 4, MPCPeriodicCoMRef, MPCPeriodicConfigurationRef -- for every instance of a batch, each with its own
// command; and the plan recurrences of PaceFootStepPlanner, CrawlFootStepPlanner and FlyingTrotFootStepPlanner
// (src/mpc/{pace,crawl,flying_trot}_foot_step_planner.cpp), whose MPC shells build the same references.  Nothing here leaves the device: the plan is read by the two kernels behind it, which write the per-instance table of
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
// foot_step_place_kernel / foot_step_refs_kernel.  Mapping: one lane per DOUBLE written, the doubles of an (instance, grid point)
// pair adjacent and the pairs in table order, so that a wave writes one contiguous run of 512 bytes whatever the record size: 12
// doubles per pair of the placement table (through RecView::placement), 13 per rtoc_task_ref_entry (its two ints as one 8-byte
// word), nq per row of the configuration reference.  The lanes of a pair recompute its few scalars (cycle, rate) from the same
// grid time.  Loads of the plan are gathers with the batch stride; the plan of a wave's instances is a few hundred bytes and
// stays in L2.  blockIdx.y of the refs kernel selects the table (wave-uniform).  No LDS, no atomics.
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
// planner state: [FS_STATE_SLOTS][batch]
constexpr int FS_ST_R = 0;         // R_.front(): the projected base rotation, advanced by every plan
constexpr int FS_ST_LOCAL = 9;     // com_to_contact_position_local_[4][3]
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
  const double* com;
  double* state;         // [FS_STATE_SLOTS][batch]
  double* plan;          // step 0 receives com_ref_[0] and R_[0]
  double* q0;            // [batch][nq]: the q the configuration reference starts from
  int batch, nq, nx;     // nx = nq + nv
  int projection;        // RTOC_PROJECT_*
};

struct FsPlanArgs {
  const double* x0;
  const double* feet;
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

// TrotFootStepPlanner::init(q) (:91-106) at the q of rtoc_set_initial_state
static __global__ __launch_bounds__(64) void foot_step_init_kernel(FsInitArgs a) {
  using namespace rbd;
  const int lane = threadIdx.x, f = lane >> 4, B = a.batch;
  const int b = blockIdx.x * 16 + (lane & 15);
  if (b >= B) return;
  const double* const q = a.x0 + (size_t)b * a.nx;
  M3 R = quat_R(q + 3);
  if (a.projection == RTOC_PROJECT_YAW) {
    const double th = atan2(R.m[3], R.m[0]), s = sin(th), c = cos(th);
    R.m[0] = c, R.m[1] = -s, R.m[3] = s, R.m[4] = c;
  } else {
    // rotation::ProjectRotationMatrix(R, Z) as it stands (rotation.hpp:103-111): not the norm of the row
    const double norm = R.m[0] * R.m[0] + R.m[1] + R.m[1];
#pragma unroll
    for (int k = 0; k < 9; ++k) R.m[k] /= norm;
  }
  R.m[2] = 0.0, R.m[5] = 0.0, R.m[6] = 0.0, R.m[7] = 0.0, R.m[8] = 1.0;
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
  // ---- MovingWindowFilter::push_back (:113-135), RaibertHeuristic::planStepLength (raibert_heuristic.cpp:50-55) ----
  double f_last = 0.0, f_ax = 0.0, f_ay = 0.0, f_t = 0.0, f_x = 0.0, f_y = 0.0;
  int f_count = 0, f_head = 0, f_slot = 0;
  bool f_push = false;
  if (a.raibert) {
    const double* const v = a.x0 + (size_t)b * a.nx + a.nq;   // vcom_ = v.head<3>() (:131)
    f_t = a.t, f_x = v[0], f_y = v[1];
    f_last = st[(size_t)FS_ST_LAST * B], f_ax = st[(size_t)FS_ST_AVG * B], f_ay = st[(size_t)(FS_ST_AVG + 1) * B];
    f_count = (int)st[(size_t)FS_ST_COUNT * B], f_head = (int)st[(size_t)FS_ST_HEAD * B];
    if (f_count == 0) {
      f_push = true, f_slot = 0, f_head = 0, f_count = 1;
      f_ax = f_x, f_ay = f_y, f_last = f_t;
    } else if (f_t - f_last >= a.min_period) {
      f_push = true;
      if (f_count == FS_RING) f_head = (f_head + 1) % FS_RING, --f_count;   // cannot happen with the window's own spacing
      f_slot = (f_head + f_count) % FS_RING;
      // pop_front while the front is older than the window (the new sample is never popped: t - t = 0)
      while (f_count > 0 && f_t - st[(size_t)(FS_ST_RING + 3 * f_head) * B] > a.period) f_head = (f_head + 1) % FS_RING, --f_count;
      double sx = 0.0, sy2 = 0.0;
      for (int k = 0; k < f_count; ++k) {
        const int slot = (f_head + k) % FS_RING;
        sx += st[(size_t)(FS_ST_RING + 3 * slot + 1) * B], sy2 += st[(size_t)(FS_ST_RING + 3 * slot + 2) * B];
      }
      sx += f_x, sy2 += f_y;
      ++f_count;
      f_ax = sx / f_count, f_ay = sy2 / f_count, f_last = f_t;
    }
    const double pg = a.period * a.gain;
    sl = mk(a.period * f_ax + pg * (cmd[(size_t)FS_CMD_VCOM * B] - f_ax), a.period * f_ay + pg * (cmd[(size_t)(FS_CMD_VCOM + 1) * B] - f_ay), 0.0);
  }
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
      if (f_push) {
        st[(size_t)(FS_ST_RING + 3 * f_slot) * B] = f_t, st[(size_t)(FS_ST_RING + 3 * f_slot + 1) * B] = f_x, st[(size_t)(FS_ST_RING + 3 * f_slot + 2) * B] = f_y;
        st[(size_t)FS_ST_LAST * B] = f_last, st[(size_t)FS_ST_AVG * B] = f_ax, st[(size_t)(FS_ST_AVG + 1) * B] = f_ay;
        st[(size_t)FS_ST_COUNT * B] = (double)f_count, st[(size_t)FS_ST_HEAD * B] = (double)f_head;
      }
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

// the loop of MPCTrot::resetContactPlacements (mpc_trot.cpp:361-365): grid point i <- contactPositions(phase_i + 1)
struct FsPlaceArgs {
  RecView rv;            // placement() of the per-instance table
  const double* plan;
  const int* phase;      // [nstages] GridInfo::phase relative to the first grid point
  double* tab_pos;       // [batch][nstages][4][3]
};
static __global__ __launch_bounds__(256) void foot_step_place_kernel(FsPlaceArgs a) {
  const int B = a.rv.batch, n = a.rv.nstages;
  const size_t total = (size_t)B * n * 12;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % 12), st = (int)((e / 12) % n), b = (int)(e / 12 / n);
    const int step = a.phase[st] + 1;
    a.tab_pos[a.rv.placement(b, st, 4, k / 3) * 3 + k % 3] = a.plan[((size_t)step * FS_PLAN_SLOTS + FS_PLAN_POS + k) * B + b];
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
  rtoc_task_ref_entry* tab[5];   // feet 0..3, CoM: [batch][nstages] or nullptr
  double* qtab;              // [batch][nstages][nq] or nullptr
  int* qtab_active;          // [batch][nstages]
  FsPeriod per[6];           // feet 0..3, CoM, configuration
  int batch, nstages, nq;
};
constexpr int FS_ENTRY_WORDS = (int)(sizeof(rtoc_task_ref_entry) / 8);   // 9 R, 3 p, 1 (active, pad)
static_assert(sizeof(rtoc_task_ref_entry) == 13 * 8, "an entry is written as 13 eight-byte words");

// Quaterniond(R): Eigen's conversion (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), q = (x, y, z, w)
static __device__ __forceinline__ void fs_eigen_quat(const double* plan_R, size_t B, double* q) {
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = plan_R[(size_t)k * B];
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

static __global__ __launch_bounds__(256) void foot_step_refs_kernel(FsRefsArgs a) {
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
      const bool active = t > pr.t0 && (which < 4 ? !((mask >> which) & 1u) : (mask & 0xFu) != 0xFu);
      if (w < 9) {
        out[e] = (unsigned long long)__double_as_longlong((w % 4 == 0) ? 1.0 : 0.0);
      } else if (w == 12) {
        out[e] = active ? 1ull : 0ull;   // little endian: active in the low word, pad = 0
      } else {
        const int k = w - 9;
        const int slot = which < 4 ? FS_PLAN_POS + 3 * which + k : FS_PLAN_COM + k;
        const double x0 = a.plan[((size_t)ph * FS_PLAN_SLOTS + slot) * B + b];
        double x = x0;   // inactive: the CoM reference's else branch (:100-102); a swing-foot reference is not updated, this stands in
        if (active) {
          const int cycle = (int)floor((t - pr.t0) / period);
          const double rate = (t - pr.t0 - cycle * period) / pr.period_active;
          const double x1 = a.plan[((size_t)(ph + pr.nph) * FS_PLAN_SLOTS + slot) * B + b];
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
      fs_eigen_quat(a.plan + ((size_t)ph * FS_PLAN_SLOTS + FS_PLAN_R) * B + b, B, qa);
      const int c = k - 3;
      const double xa = c == 0 ? qa[0] : c == 1 ? qa[1] : c == 2 ? qa[2] : qa[3];
      x = xa;
      if (t > pr.t0 && (a.masks[ph] & 0xFu) != 0xFu) {
        const int cycle = (int)floor((t - pr.t0) / period);
        const double rate = (t - pr.t0 - cycle * period) / pr.period_active;
        double qb[4];
        fs_eigen_quat(a.plan + ((size_t)(ph + pr.nph) * FS_PLAN_SLOTS + FS_PLAN_R) * B + b, B, qb);
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
