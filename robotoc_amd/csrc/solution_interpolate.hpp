// solution_interpolate.hpp -- SolutionInterpolator on the device: the solution of one grid re-gridded onto another.
//
// Replaces SolutionInterpolator::interpolate (reference src/solver/solution_interpolator.cpp:30-113, with interpolate :119-146,
// interpolatePartial :149-172, initEventSolution :175-198, modifyImpactSolution :201-208, modifyTerminalSolution :211-224 and
// findStoredGridIndexBeforeTime) on the packed SplitSolution records of RTOC_BUF_SOL, with the conventions of the host mirrors
// (robotoc_amd/host/robotoc_hip_planner.hpp: SolutionInterpolator, robotoc_amd/solver.py: OCPSolver._interpolate): the f / mu
// stacks are compacted by the active contacts of their own grid point, so every stack is expanded by the stored mask and
// re-packed by the new grid point's; the search steps back over stored points without extent in time; alpha is clamped to [0, 1].
// One wave per (instance, new grid point): it decides its branch from the stored times (the lanes share the two searches), reads
// at most two stored records and writes EVERY double of its own record -- the buffer still holds the old grid's data, so what the
// host leaves at the zero of a fresh array is written as zero here.  The one write of the reference that goes to another grid
// point's record (xi of point i - 2 at a matched impact i) is a gather: the wave of grid point j looks at j + 2.
// Robot::interpolateConfiguration: joints linearly, a free-flyer base along the screw motion q1 (+) alpha (q2 (-) q1) -- log6 of the
// relative placement (rbd::log6_fwd: its near-pi branch), the SE(3) exponential of alpha times it, the quaternion of the rotation
// matrix with w > 0 where the trace is positive, normalised.  Pure streaming: no LDS.
#pragma once
#include "record_view.hpp"
#include "rigid_body_math.hpp"

namespace rtoc {

// the snapshot of rtoc_solution_store (rt_context.hpp: InterpState)
struct StoredSolution {
  const double* sol;     // [batch][n][sol stride]
  const double* t;       // [n] or [batch][n] grid times
  const double* dt;      // same shape: time steps
  const int* type;       // [n] RTOC_GRID_*
  const unsigned* mask;  // [n] contact schedule, or nullptr (no contacts)
  int n, per_instance;
};

struct InterpArgs {
  RecView rv;          // the grid and the schedule to interpolate onto; rv.sol is not read
  StoredSolution st;
  double* out;         // RTOC_BUF_SOL: [batch][rv.nstages][sol stride]
  const double* t;     // [rv.nstages] or [batch][rv.nstages] times of the new grid
  int t_per_instance;
  int ncontacts;
  unsigned six_rows;   // bit c: contact c is a surface contact (6 stack rows), else a point contact (3)
};

// grid times as the running sum t[i + 1] = t[i] + dt[i] from t0, per instance from dt_inst or once from the grid's dt; the time
// steps and the grid types beside them where asked for (the store)
struct InterpTimesArgs {
  const rtoc_grid* grid;
  const double* dt_inst;  // [batch][nstages] or nullptr
  double* t;              // [batch][nstages] with dt_inst, else [nstages]
  double* dt_out;         // same shape, or nullptr
  int* type_out;          // [nstages], or nullptr
  int nstages, batch;
  double t0;
};

static __global__ __launch_bounds__(64) void interp_times_kernel(InterpTimesArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= (a.dt_inst ? a.batch : 1)) return;
  const size_t o = (size_t)b * a.nstages;
  double t = a.t0;
  for (int i = 0; i < a.nstages; ++i) {
    const double d = a.dt_inst ? a.dt_inst[o + i] : a.grid[i].dt;
    a.t[o + i] = t;
    if (a.dt_out) a.dt_out[o + i] = d;
    if (a.type_out && b == 0) a.type_out[i] = a.grid[i].type;
    t = t + d;
  }
}

namespace interp {
using rbd::M3;
using rbd::SV;
using rbd::V3;

enum Mode { COPY = 0, FULL = 1, PARTIAL = 2, EVENT = 3 };
struct Branch {
  int mode;         // Mode
  int a;            // stored record copied, or the first of the two blended (the second is a + 1)
  int zero_impact;  // modifyImpactSolution: u, the a | dv slot and nu_passive are zero
  int matched;      // a matched impact (the xi transfer)
  double alpha;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

// the branch of a grid point of type `type` at time tt (solution_interpolator.cpp:33-110); uniform over the wave
__device__ inline Branch decide(const StoredSolution& st, const double* T0, const double* D0, double tt, int type, int lane) {
  const int n0 = st.n;
  Branch r;
  r.mode = COPY, r.a = 0, r.zero_impact = 0, r.matched = 0, r.alpha = 0.0;
  if (tt <= T0[0]) return r;
  if (tt >= T0[n0 - 1]) {
    r.a = n0 - 1;
    return r;
  }
  if (type == RTOC_GRID_IMPACT || type == RTOC_GRID_LIFT) {
    int k = n0;  // the first stored event of this type at this time
    for (int j = lane; j + 1 < n0; j += 64)
      if (st.type[j] == type && fabs(T0[j] - tt) < 1e-9) {
        k = j;
        break;
      }
    k = wave_min(k);
    if (k < n0) {
      r.a = k;
      r.zero_impact = r.matched = type == RTOC_GRID_IMPACT;
      return r;
    }
  }
  // findStoredGridIndexBeforeTime: the last stored point not after tt, not the terminal one, and none without extent in time
  int k = n0;
  for (int j = 1 + lane; j < n0; j += 64)
    if (!(T0[j] <= tt)) {
      k = j;
      break;
    }
  k = wave_min(k) - 1;
  k = k > n0 - 2 ? n0 - 2 : k;
  k = k < 0 ? 0 : k;
  // (kept for parity with the host mirrors and dead here: the device's times are running sums of non-negative steps, so a point
  // with dt <= 0 shares its time with its successor and the search above never stops on it; tested on the CPU restatement alone)
  while (k > 0 && D0[k] <= 0.0) --k;
  r.a = k;
  r.alpha = fmin(fmax((tt - T0[k]) / D0[k], 0.0), 1.0);
  const int next = st.type[k + 1];
  if (type == RTOC_GRID_IMPACT || type == RTOC_GRID_LIFT) {
    r.mode = next == RTOC_GRID_TERMINAL ? PARTIAL : EVENT;
    r.zero_impact = next == RTOC_GRID_TERMINAL && type == RTOC_GRID_IMPACT;
  } else {
    r.mode = next == RTOC_GRID_INTERMEDIATE ? FULL : PARTIAL;
  }
  return r;
}

// the free-flyer part [x y z qx qy qz qw] of interpolateConfiguration: M1 exp6(alpha log6(M1^-1 M2))
struct BasePose {
  double px, py, pz, x, y, z, w;
};
__device__ __forceinline__ BasePose interpolate_base(const double* q1, const double* q2, double alpha) {
  const M3 R1 = rbd::quat_R(q1 + 3);
  const V3 p1 = rbd::ldv3(q1);
  M3 Rx, Ra;
  V3 px, pa;
  rbd::rel(R1, p1, rbd::quat_R(q2 + 3), rbd::ldv3(q2), Rx, px);
  SV lg, unused;
  rbd::log6_fwd(Rx, px, rbd::sv0(), lg, unused);
  rbd::exp6(alpha * lg.l, alpha * lg.a, Ra, pa);
  const V3 p = p1 + rbd::mul(R1, pa);
  double qt[4];
  rbd::R_quat(rbd::mul(R1, Ra), qt);
  return BasePose{p.x, p.y, p.z, qt[0], qt[1], qt[2], qt[3]};
}

__device__ __forceinline__ int contact_rows(unsigned six_rows, int c) { return 3 + 3 * (int)((six_rows >> c) & 1u); }

// entry r of contact c of a stack compacted by `mask`; zero where the contact is not active there
__device__ __forceinline__ double stack_at(const double* stack, unsigned mask, unsigned six_rows, int c, int r) {
  if (!((mask >> c) & 1u)) return 0.0;
  int k = 0;
  for (int cc = 0; cc < c; ++cc)
    if ((mask >> cc) & 1u) k += contact_rows(six_rows, cc);
  return stack[k + r];
}
}  // namespace interp

static __global__ __launch_bounds__(64) void solution_interpolate_kernel(InterpArgs a) {
  using namespace interp;
  const int lane = threadIdx.x;
  const int N = a.rv.nstages, n0 = a.st.n;
  const int b = blockIdx.x / N, i = blockIdx.x % N;
  if (b >= a.rv.batch) return;
  const rtoc_record_layout& sl = a.rv.L.sol;
  const rtoc_dims& d = a.rv.L.dims;
  const int nv = d.nv, floating = d.np == 6, nq = nv + floating;
  const double* T0 = a.st.t + (a.st.per_instance ? (size_t)b * n0 : 0);
  const double* D0 = a.st.dt + (a.st.per_instance ? (size_t)b * n0 : 0);
  const double* T1 = a.t + (a.t_per_instance ? (size_t)b * N : 0);
  const double* __restrict__ S0 = a.st.sol + (size_t)b * n0 * sl.stride;
  double* __restrict__ out = a.out + (size_t)blockIdx.x * sl.stride;

  const Branch br = decide(a.st, T0, D0, T1[i], a.rv.grid[i].type, lane);
  // xi of this record at a matched impact two grid points ahead (:66-69): from the stored record two ahead of that impact's
  int xi_from = -1;
  if (i + 2 < N && a.rv.grid[i + 2].type == RTOC_GRID_IMPACT) {
    const Branch b2 = decide(a.st, T0, D0, T1[i + 2], RTOC_GRID_IMPACT, lane);
    if (b2.matched && b2.a >= 2) xi_from = b2.a - 2;
  }
  const double* __restrict__ ra = S0 + (size_t)br.a * sl.stride;
  const double* __restrict__ rb = br.mode == COPY ? ra : ra + sl.stride;
  const unsigned ma = a.st.mask ? a.st.mask[br.a] : 0u, mb = a.st.mask ? a.st.mask[br.a + (br.mode == COPY ? 0 : 1)] : 0u;
  const unsigned mi = a.rv.active ? a.rv.active[i] : 0u;
  const bool terminal = i == N - 1;
  const double alpha = br.alpha, beta = 1.0 - alpha;
  BasePose qb = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  if (br.mode != COPY && floating) qb = interpolate_base(ra + sl.off[RTOC_SOL_Q], rb + sl.off[RTOC_SOL_Q], alpha);

  // one entry of the record: entry j of field f
  auto entry = [&](const int e) __attribute__((always_inline)) -> double {
    int f = 0;
#pragma unroll
    for (int g = 1; g < RTOC_SOL_NFIELDS; ++g) f = e >= sl.off[g] ? g : f;   // the offsets ascend
    const int off = sl.off[f], j = e - off;
    const bool stack = f == RTOC_SOL_F || f == RTOC_SOL_MU;
    // entries in use: what the reference's vectors hold; the rest of the slot is padding
    const int n = f == RTOC_SOL_Q ? nq : f == RTOC_SOL_U ? d.nu : stack ? d.nf_max : f == RTOC_SOL_NUP ? d.np : f == RTOC_SOL_XI ? d.ns_max : nv;
    const bool acc = f == RTOC_SOL_U || f == RTOC_SOL_A || f == RTOC_SOL_NUP;   // modifyImpactSolution's members
    const bool zeroed = (br.zero_impact && acc) || (terminal && (acc || stack || f == RTOC_SOL_BETA));
    if (j >= n) return br.mode == COPY ? ra[e] : 0.0;
    if (zeroed) return 0.0;
    if (f == RTOC_SOL_XI) return xi_from >= 0 ? S0[(size_t)xi_from * sl.stride + e] : (br.mode == COPY ? ra[e] : 0.0);
    if (stack) {
      // row j of the stack compacted by this grid point's mask: entry r of contact c, or beyond the packed rows
      int c = -1, r = 0, k = 0;
      for (int cc = 0; cc < a.ncontacts; ++cc)
        if ((mi >> cc) & 1u) {
          const int rows = contact_rows(a.six_rows, cc);
          if (c < 0 && j < k + rows) c = cc, r = j - k;
          k += rows;
        }
      if (c < 0) return 0.0;
      const double xa = stack_at(ra + off, ma, a.six_rows, c, r);
      if (br.mode == COPY || br.mode == PARTIAL) return xa;
      if (br.mode == EVENT) return stack_at(rb + off, mb, a.six_rows, c, r);
      return ((mb >> c) & 1u) ? beta * xa + alpha * stack_at(rb + off, mb, a.six_rows, c, r) : xa;
    }
    if (br.mode == COPY) return ra[e];
    if (f == RTOC_SOL_Q && floating && j < 7) {
      return j == 0 ? qb.px : j == 1 ? qb.py : j == 2 ? qb.pz : j == 3 ? qb.x : j == 4 ? qb.y : j == 5 ? qb.z : qb.w;
    }
    const bool blend = f == RTOC_SOL_Q || f == RTOC_SOL_V || f == RTOC_SOL_LMD || f == RTOC_SOL_GMM || br.mode == FULL ||
                       (br.mode == EVENT && f == RTOC_SOL_A);
    return blend ? beta * ra[e] + alpha * rb[e] : (br.mode == EVENT ? rb[e] : ra[e]);
  };
  // four entries per lane and trip, every load of a trip ahead of its stores: the records are read once and never written
  for (int e0 = lane; e0 < sl.stride; e0 += 256) {
    double x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = e0 + 64 * u < sl.stride ? entry(e0 + 64 * u) : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + 64 * u < sl.stride) out[e0 + 64 * u] = x[u];
  }
}

}  // namespace rtoc
