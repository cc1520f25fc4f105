// control_policy.hpp -- ControlPolicy on the device: the feedback law an MPC hands to the robot, at each instance's own time.
//
// Replaces ControlPolicy::set (reference src/mpc/control_policy.cpp:24-60) and the law the simulator applies with it,
// u = tauJ - Kp (qJ - q) - Kd (dqJ - v) (bindings/python/robotoc_sim/mpc_simulation.py:6-11), on the packed records of RTOC_BUF_SOL
// and RTOC_BUF_RIC.  Per instance and query time t, with the grid times tg of policy_times_kernel:
//   t < tg[0]: record 0 (:31-38);
//   else the first i in 1 .. N - 2 with t < tg[i] whose record i - 1 is no impact (:39-40): alpha = (tg[i] - t) / (tg[i] - tg[i - 1]),
//   not clamped, and every output alpha rec[i - 1] + (1 - alpha) rec[i] (:41-52);
//   else record N - 1 (:55-59).
// Not the reference's (an impact grid point's u and K are never read, include/rtoc.h): where record i of the interval is an impact,
// the policy is record i - 1 unblended; where the fallback record N - 1 is an impact, it is record N - 2.
// Of a record: tauJ = u, qJ / dqJ = the last nu entries of q / v, Kp / Kd = the last nu columns of the Kq / Kv halves of K
// (nu x 2nv, row-major) -- these doubles of at most two records and nothing else.  A non-finite t gives NaN in every output.
// One wave per instance.  Both kernels are launch- and latency-bound (a few KB per instance), so the loads are laid out for few
// instructions, not for bytes: the lanes of a trip run along the row runs of K (nu contiguous doubles at column nv - nu and
// 2nv - nu), 8 bytes a lane -- the Kd run of nv = 35 starts at 328 bytes, so a 16-byte load per lane would straddle -- and every
// load of a trip is issued ahead of its first use.  No LDS in control_policy_kernel; 2 nu doubles of it in control_input_kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "record_view.hpp"

namespace rtoc {

// grid times as the running sum t[i + 1] = t[i] + dt[i] from t0 (the sum of rtoc_solution_store: in this order, in double), per
// instance from dt_inst or once from the grid's dt.  The arithmetic of interp_times_kernel, restated: including
// solution_interpolate.hpp for it would define that header's kernels in a second unit (rt_context.hpp, on kernel headers)
struct PolicyTimesArgs {
  const rtoc_grid* grid;
  const double* dt_inst;  // [batch][nstages] or nullptr
  double* t;              // [count][nstages] with dt_inst, else [nstages]
  int nstages, count;
  double t0;
};

static __global__ __launch_bounds__(64) void policy_times_kernel(PolicyTimesArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= (a.dt_inst ? a.count : 1)) return;
  const size_t o = (size_t)b * a.nstages;
  double t = a.t0;
  for (int i = 0; i < a.nstages; ++i) {
    a.t[o + i] = t;
    t = t + (a.dt_inst ? a.dt_inst[o + i] : a.grid[i].dt);
  }
}

struct PolicyArgs {
  RecView rv;             // sol: RTOC_BUF_SOL, [batch][nstages][sol stride]
  const double* ric;      // RTOC_BUF_RIC: [batch][nstages][ric stride] (the view has no Riccati records)
  const double* tg;       // grid times, [nstages] or [count][nstages]
  const double* t;        // query times, [1] or [count]
  const double* x;        // control_input_kernel: measured states [count][nq + nv]
  double* out;            // control_policy_kernel: [count][rtoc_control_policy_stride(nu)]; control_input_kernel: [count][nu]
  int count, N;
  int tg_per_instance, t_per_instance;
  int nq;
};

namespace policy {

// what a query time selects: record a alone (b < 0), or alpha rec[a] + (1 - alpha) rec[b]
struct Pick {
  int a, b;
  double alpha;
};

// control_policy.cpp:31-59 with the two departures above; uniform over the wave.  The interval search takes the candidates
// 1 .. N - 2 sixty-four at a time, one per lane
__device__ inline Pick pick(const PolicyArgs& p, const double* tg, double t, int lane) {
  Pick r;
  r.a = 0, r.b = -1, r.alpha = 1.0;
  if (t < tg[0]) return r;
  for (int base = 1; base <= p.N - 2; base += 64) {
    const int i = base + lane;
    const bool hit = i <= p.N - 2 && t < tg[i] && p.rv.grid[i - 1].type != RTOC_GRID_IMPACT;
    const unsigned long long m = __ballot(hit);
    if (m) {
      const int k = base + __ffsll((long long)m) - 1;
      r.a = k - 1;
      if (p.rv.grid[k].type == RTOC_GRID_IMPACT) return r;   // hold: the impact's u and K are not defined
      r.b = k;
      r.alpha = (tg[k] - t) / (tg[k] - tg[k - 1]);
      return r;
    }
  }
  r.a = p.N - 1;
  if (r.a > 0 && p.rv.grid[r.a].type == RTOC_GRID_IMPACT) r.a = p.N - 2;   // (rtoc_set_grid takes no impact at grid point 0)
  return r;
}

__device__ __forceinline__ double blend(double alpha, double a, double b) { return alpha * a + (1.0 - alpha) * b; }

}  // namespace policy

// [tauJ | qJ | dqJ | Kp | Kd] of every instance (include/rtoc_layout.h: rtoc_control_policy_*), padding zero
static __global__ __launch_bounds__(64) void control_policy_kernel(PolicyArgs p) {
  using namespace policy;
  const int lane = threadIdx.x, b = blockIdx.x;
  if (b >= p.count) return;
  const int nu = p.rv.nu(), nv = p.rv.nv(), nx = 2 * nv, nn = nu * nu;
  const int stride = rtoc_control_policy_stride(nu);
  double* __restrict__ out = p.out + (size_t)b * stride;
  const double t = p.t[p.t_per_instance ? b : 0];
  if (!isfinite(t)) {
    for (int e = lane; e < stride; e += 64) out[e] = __builtin_nan("");
    return;
  }
  const Pick k = pick(p, p.tg + (p.tg_per_instance ? (size_t)b * p.rv.nstages : 0), t, lane);
  const bool two = k.b >= 0;
  const size_t r0 = (size_t)b * p.rv.nstages + k.a, r1 = (size_t)b * p.rv.nstages + (two ? k.b : k.a);
  const double* __restrict__ sa = p.rv.sol_at(r0);
  const double* __restrict__ sb = p.rv.sol_at(r1);
  const double* __restrict__ ka = p.ric + r0 * p.rv.L.ric.stride + p.rv.L.ric.off[RTOC_RIC_K];
  const double* __restrict__ kb = p.ric + r1 * p.rv.L.ric.stride + p.rv.L.ric.off[RTOC_RIC_K];
  const int pad = rtoc_pad8(nu);
  const int oq = p.rv.sol_off(RTOC_SOL_Q) + p.nq - nu, ov = p.rv.sol_off(RTOC_SOL_V) + nv - nu, ou = p.rv.sol_off(RTOC_SOL_U);
  // tauJ, qJ, dqJ and their padding
  for (int c = lane; c < pad; c += 64) {
    double u = 0.0, q = 0.0, v = 0.0;
    if (c < nu) {
      u = sa[ou + c], q = sa[oq + c], v = sa[ov + c];
      if (two) {
        const double u1 = sb[ou + c], q1 = sb[oq + c], v1 = sb[ov + c];
        u = blend(k.alpha, u, u1), q = blend(k.alpha, q, q1), v = blend(k.alpha, v, v1);
      }
    }
    out[c] = u, out[pad + c] = q, out[2 * pad + c] = v;
  }
  // Kp, Kd: entry e = (row r, column c) along the row runs of K; written transposed (column-major)
  double* __restrict__ kp = out + rtoc_control_policy_kp_off(nu);
  double* __restrict__ kd = out + rtoc_control_policy_kd_off(nu);
  for (int e = lane; e < nn; e += 64) {
    const int r = e / nu, c = e - r * nu;
    const int ip = r * nx + (nv - nu) + c, id = ip + nv;
    double gp = ka[ip], gd = ka[id];
    if (two) {
      const double gp1 = kb[ip], gd1 = kb[id];
      gp = blend(k.alpha, gp, gp1), gd = blend(k.alpha, gd, gd1);
    }
    kp[r + c * nu] = gp, kd[r + c * nu] = gd;
  }
  for (int e = nn + lane; e < rtoc_pad8(nn); e += 64) kp[e] = 0.0, kd[e] = 0.0;
}

// u = tauJ - Kp (qJ - q) - Kd (dqJ - v) of every instance at its measured state x = [q | v], Kp and Kd never in memory.
// The errors qJ - q, dqJ - v go through LDS (dynamic: 2 nu doubles).  A row of K belongs to P = 2^k <= 64 / nu neighbouring lanes
// (64 / P rows a pass): lane (r, j) takes the columns j, j + P, ... of both runs, the P partial sums meet by butterfly
static __global__ __launch_bounds__(64) void control_input_kernel(PolicyArgs p) {
  using namespace policy;
  extern __shared__ double err[];   // [nu] qJ - q, then [nu] dqJ - v
  const int lane = threadIdx.x, b = blockIdx.x;
  if (b >= p.count) return;
  const int nu = p.rv.nu(), nv = p.rv.nv(), nx = 2 * nv;
  double* __restrict__ out = p.out + (size_t)b * nu;
  const double t = p.t[p.t_per_instance ? b : 0];
  if (!isfinite(t)) {
    for (int e = lane; e < nu; e += 64) out[e] = __builtin_nan("");
    return;
  }
  const Pick k = pick(p, p.tg + (p.tg_per_instance ? (size_t)b * p.rv.nstages : 0), t, lane);
  const bool two = k.b >= 0;
  const size_t r0 = (size_t)b * p.rv.nstages + k.a, r1 = (size_t)b * p.rv.nstages + (two ? k.b : k.a);
  const double* __restrict__ sa = p.rv.sol_at(r0);
  const double* __restrict__ sb = p.rv.sol_at(r1);
  const double* __restrict__ ka = p.ric + r0 * p.rv.L.ric.stride + p.rv.L.ric.off[RTOC_RIC_K];
  const double* __restrict__ kb = p.ric + r1 * p.rv.L.ric.stride + p.rv.L.ric.off[RTOC_RIC_K];
  const double* __restrict__ x = p.x + (size_t)b * (p.nq + nv);
  const int oq = p.rv.sol_off(RTOC_SOL_Q) + p.nq - nu, ov = p.rv.sol_off(RTOC_SOL_V) + nv - nu, ou = p.rv.sol_off(RTOC_SOL_U);
  for (int c = lane; c < nu; c += 64) {
    double q = sa[oq + c], v = sa[ov + c];
    const double xq = x[p.nq - nu + c], xv = x[p.nq + nv - nu + c];
    if (two) {
      const double q1 = sb[oq + c], v1 = sb[ov + c];
      q = blend(k.alpha, q, q1), v = blend(k.alpha, v, v1);
    }
    err[c] = q - xq, err[nu + c] = v - xv;
  }
  __syncthreads();
  int P = 1;
  while (2 * P * nu <= 64) P *= 2;
  const int rows = 64 / P, j = lane & (P - 1);
  for (int rb = 0; rb < nu; rb += rows) {
    const int r = rb + lane / P;
    double acc = 0.0;
    if (r < nu) {
      const int ip = r * nx + (nv - nu);
      for (int c = j; c < nu; c += P) {
        double gp = ka[ip + c], gd = ka[ip + nv + c];
        if (two) {
          const double gp1 = kb[ip + c], gd1 = kb[ip + nv + c];
          gp = blend(k.alpha, gp, gp1), gd = blend(k.alpha, gd, gd1);
        }
        acc += gp * err[c] + gd * err[nu + c];
      }
    }
    for (int m = P >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (r < nu && j == 0) {
      double u = sa[ou + r];
      if (two) u = blend(k.alpha, u, sb[ou + r]);
      out[r] = u - acc;
    }
  }
}

}  // namespace rtoc
