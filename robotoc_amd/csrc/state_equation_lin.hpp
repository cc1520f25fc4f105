// state_equation_lin.hpp -- linearisation of the (forward-Euler) state equation on the device.
//
// Replaces linearizeStateEquation (reference src/dynamics/state_equation.cpp:29-66) on intermediate / lift grids and
// linearizeImpactStateEquation (src/dynamics/impact_state_equation.cpp:27-57) on impact grids, and produces what the
// correctLinearize* steps (state_equation.cpp:69-90, impact :60-75; rtoc_condense applies them) take from
// StateEquationData: Fqq_inv and Fqq_prev_inv (RTOC_BUF_SE3).  For a floating base the configuration difference and its
// Jacobians are Pinocchio's difference / dDifference on SE(3):
//   Fq (base) = log6(M_next^-1 M)                      [+ dt v]            (Robot::subtractConfiguration(q, q_next))
//   Fqq       = d/dM      = Jlog6(X1),  X1 = M_next^-1 M                   (dSubtractConfiguration_dqf)
//   Fqq_prev  = d/dM of log6(M^-1 M_prev) = -Jlog6(X0) Ad_{X0^-1},  X0 = M^-1 M_prev   (dSubtractConfiguration_dq0(q_prev, q))
//   Fqq_inv   = [ -Jlog6(X1) Ad_{X1^-1} ]^-1           (dSubtractConfiguration_dq0(q, q_next), state_equation.cpp:78-79)
// Jlog6 x twist is evaluated by forward mode through the log (rbd::log6_fwd); Ad_{X^-1} is the motion actInv.  Six lanes
// carry the six unit twists, lane 0 inverts the two 6 x 6 Jacobians by their block-triangular shape (3 x 3 cofactor inverses,
// like the reference's SE3JacobianInverse).  Everything else is elementwise.
// One wave per (instance, grid point).  Records: the un-condensed contact-path convention (la in CDD.la).
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"

namespace rtoc {

struct SeLinArgs {
  RecView rv;            // se3: written on a floating base only; dx0: computeInitialStateDirection (state_equation.cpp:99-109), with x0 only
  const double* x0;      // [batch][nq + nv]: q_prev of grid point 0 (the initial state), may be nullptr -> q_prev = q
  int zeroed;            // the KKT record was initialised just before (init_records_kernel: zeros, Fqq = I, Fqv = dt I): only the base corner is written
};


static __global__ __launch_bounds__(64) void state_equation_lin_kernel(SeLinArgs a) {
  using rbd::M3;
  using rbd::SV;
  using rbd::V3;
  __shared__ double J[3][36];  // Fqq, Fqq_prev, d/dq0 of (q (-) q_next): 6 x 6, column-major
  const int lane = threadIdx.x;
  const int b = blockIdx.x / a.rv.nstages, st = blockIdx.x % a.rv.nstages;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  const bool impact = g.type == RTOC_GRID_IMPACT;
  if (st == a.rv.nstages - 1) {
    // linearizeTerminalStateEquation (src/dynamics/terminal_state_equation.cpp:8-28): lq -= lmd (base: += Fqq_prev^T lmd),
    // lv -= gmm; Fqq_prev_inv for correctCostateDirection / correctLinearizeTerminalStateEquation
    const int nv = a.rv.nv(), nb = a.rv.floating() ? 6 : 0;
    const size_t rec = (size_t)b * a.rv.nstages + st;
    const double* const s = a.rv.sol_at(rec);
    double* const kr = a.rv.kkt_at(rec);
    for (int i = lane; i < nv; i += 64) {
      if (i >= nb) kr[a.rv.kkt_off(RTOC_KKT_LX) + i] -= s[a.rv.sol_off(RTOC_SOL_LMD) + i];
      kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + i] -= s[a.rv.sol_off(RTOC_SOL_GMM) + i];
    }
    if (a.rv.floating()) {
      const double* q = s + a.rv.sol_off(RTOC_SOL_Q);
      const double* qp = s - a.rv.L.sol.stride + a.rv.sol_off(RTOC_SOL_Q);
      M3 R0;
      V3 p0;
      rbd::rel(rbd::quat_R(q + 3), rbd::ldv3(q), rbd::quat_R(qp + 3), rbd::ldv3(qp), R0, p0);
      if (lane < 6) {
        SV val, der;
        rbd::log6_fwd(R0, p0, rbd::sv0() - rbd::act_inv(R0, p0, rbd::unit_twist(lane)), val, der);
        const double c0[6] = {der.l.x, der.l.y, der.l.z, der.a.x, der.a.y, der.a.z};
#pragma unroll
        for (int r = 0; r < 6; ++r) J[1][r + 6 * lane] = c0[r];
      }
      __syncthreads();
      if (lane < 6) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) t += J[1][r + 6 * lane] * s[a.rv.sol_off(RTOC_SOL_LMD) + r];
        kr[a.rv.kkt_off(RTOC_KKT_LX) + lane] += t;
      }
      if (lane == 0 && a.rv.se3) {
        double* const se = a.rv.se3 + rec * RTOC_SE3_STRIDE;
        double A[36];
        rbd::inv6_block_ut(J[1], A);
#pragma unroll
        for (int e = 0; e < 36; ++e) se[e] = 0.0, se[36 + e] = A[e];
      }
    }
    return;
  }
  const double dt = impact ? 0.0 : grid_dt(a.rv.grid, a.rv.dt_inst, b, a.rv.nstages, st);
  const int nv = a.rv.nv(), nx = 2 * nv, nb = a.rv.floating() ? 6 : 0, nq = nv + (a.rv.floating() ? 1 : 0);
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  const double* const sn = s + a.rv.L.sol.stride;
  const double* const qp = st > 0 ? s - a.rv.L.sol.stride + a.rv.sol_off(RTOC_SOL_Q) : (a.x0 ? a.x0 + (size_t)b * (nq + nv) : s + a.rv.sol_off(RTOC_SOL_Q));
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  const double *q = s + a.rv.sol_off(RTOC_SOL_Q), *v = s + a.rv.sol_off(RTOC_SOL_V), *acc = s + a.rv.sol_off(RTOC_SOL_A), *lmd = s + a.rv.sol_off(RTOC_SOL_LMD), *gmm = s + a.rv.sol_off(RTOC_SOL_GMM);
  const double *qn = sn + a.rv.sol_off(RTOC_SOL_Q), *vn = sn + a.rv.sol_off(RTOC_SOL_V), *lmdn = sn + a.rv.sol_off(RTOC_SOL_LMD), *gmmn = sn + a.rv.sol_off(RTOC_SOL_GMM);
  // ---- Fxx top half: Fqq = I (joints), Fqv = dt I; the bottom half belongs to the dynamics condensation ----
  if (a.zeroed) {
    // rtoc_contact_eval_kkt: init_records_kernel has just written the record, zeros and the diagonals Fqq = I, Fqv = dt I with
    // them (scattered 8-byte stores from here were a partial line each)
  } else {
    int r = lane % nx, c = lane / nx;
    for (int e = lane; e < nx * nx; e += 64) {
      if (r < nv) kr[a.rv.kkt_off(RTOC_KKT_FXX) + e] = (c == r) ? 1.0 : (c == nv + r ? dt : 0.0);
      r += 64;
      while (r >= nx) r -= nx, ++c;
    }
  }
  // ---- joints and velocities ----
  for (int i = lane; i < nv; i += 64) {
    if (i >= nb) {
      kr[a.rv.kkt_off(RTOC_KKT_FX) + i] = q[(nb ? 1 : 0) + i] + dt * v[i] - qn[(nb ? 1 : 0) + i];   // Fq (:17-18), joints; q carries 7 base entries
      kr[a.rv.kkt_off(RTOC_KKT_LX) + i] += lmdn[i] - lmd[i];                                         // (:47-48 / :52)
    }
    kr[a.rv.kkt_off(RTOC_KKT_FX) + nv + i] = v[i] + (impact ? acc[i] : dt * acc[i]) - vn[i];         // Fv (:19; impact :15)
    kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + i] += dt * lmdn[i] + gmmn[i] - gmm[i];                       // lv (:55; impact :53)
    cr[a.rv.cdd_off(RTOC_CDD_LA) + i] += impact ? gmmn[i] : dt * gmmn[i];                            // la (:56) / ldv (impact :54)
    if (!impact) {                                                                 // STO sensitivities (:58-63)
      kr[a.rv.kkt_off(RTOC_KKT_HX) + nv + i] += lmdn[i];
      cr[a.rv.cdd_off(RTOC_CDD_HA) + i] += gmmn[i];
      kr[a.rv.kkt_off(RTOC_KKT_FFX) + i] = v[i];
      kr[a.rv.kkt_off(RTOC_KKT_FFX) + nv + i] = acc[i];
    }
  }
  if (!impact) {
    double h = 0.0;
    for (int i = lane; i < nv; i += 64) h += lmdn[i] * v[i] + gmmn[i] * acc[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, 64);
    if (lane == 0) kr[a.rv.kkt_off(RTOC_KKT_SCAL) + RTOC_KKT_SCAL_H] += h;
  }
  if (st == 0 && a.rv.dx0 && !a.rv.floating() && a.x0)
    for (int i = lane; i < nx; i += 64) a.rv.dx0[(size_t)b * nx + i] = a.x0[(size_t)b * nx + i] - (i < nv ? q[i] : v[i - nv]);
  if (!a.rv.floating()) return;
  // ---- the free-flyer base: differences on SE(3) ----
  const M3 R = rbd::quat_R(q + 3), Rn = rbd::quat_R(qn + 3), Rp = rbd::quat_R(qp + 3);
  const V3 p = rbd::ldv3(q), pn = rbd::ldv3(qn), pp = rbd::ldv3(qp);
  M3 R1, R0;
  V3 p1, p0;
  rbd::rel(Rn, pn, R, p, R1, p1);  // X1 = M_next^-1 M
  rbd::rel(R, p, Rp, pp, R0, p0);  // X0 = M^-1 M_prev
  __shared__ double sLog[2][6];  // log6(X1), log6(X0)
  if (lane < 18) {
    // 18 lanes, one forward-mode evaluation through the log each: matrix m, column c
    //   m = 0: Fqq[:, c] = Jlog6(X1) e_c      m = 1: Fqq_prev[:, c] = -Jlog6(X0) Ad_{X0^-1} e_c      m = 2: d/dq0 of q (-) q_next
    const int m = lane / 6, c = lane % 6;
    const M3& Rm = m == 1 ? R0 : R1;
    const V3 pm = m == 1 ? p0 : p1;
    const SV e = rbd::unit_twist(c);
    const SV tw = m == 0 ? e : rbd::sv0() - rbd::act_inv(Rm, pm, e);
    SV val, der;
    rbd::log6_fwd(Rm, pm, tw, val, der);
    const double col[6] = {der.l.x, der.l.y, der.l.z, der.a.x, der.a.y, der.a.z};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      J[m][r + 6 * c] = col[r];
      if (m == 0) kr[a.rv.kkt_off(RTOC_KKT_FXX) + r + (size_t)c * nx] = col[r];  // Fqq top-left corner
    }
    if (c == 0 && m < 2) {
      const double l6[6] = {val.l.x, val.l.y, val.l.z, val.a.x, val.a.y, val.a.z};
#pragma unroll
      for (int r = 0; r < 6; ++r) sLog[m][r] = l6[r];
      if (m == 0) {   // Fq (base) = log6(X1) + dt v
#pragma unroll
        for (int r = 0; r < 6; ++r) kr[a.rv.kkt_off(RTOC_KKT_FX) + r] = l6[r] + dt * v[r];
      }
    }
  }
  __syncthreads();
  if (lane < 6) {
    // lq[:6] += Fqq^T lmd_next[:6] + Fqq_prev^T lmd[:6]   (:41-46)
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) t += J[0][r + 6 * lane] * lmdn[r] + J[1][r + 6 * lane] * lmd[r];
    kr[a.rv.kkt_off(RTOC_KKT_LX) + lane] += t;
  }
  if (a.rv.se3 && lane >= 32 && lane < 34) {
    // two lanes, one block-triangular inverse each: Fqq_inv (from the d/dq0 Jacobian), Fqq_prev_inv
    const int which = lane - 32;
    double* const se = a.rv.se3 + rec * RTOC_SE3_STRIDE;
    double A[36];
    rbd::inv6_block_ut(J[which == 0 ? 2 : 1], A);
#pragma unroll
    for (int e = 0; e < 36; ++e) se[36 * which + e] = A[e];
    if (which == 1 && st == 0 && a.rv.dx0 && a.x0) {
      // computeInitialStateDirection (:99-109): dq0 = q0 (-) s0.q = log6(M^-1 M0) = log6(X0) for the base, with the
      // -Fqq_prev_inv correction rtoc_compute_initial_state_direction would apply; joints and velocities plain
      double* const o = a.rv.dx0 + (size_t)b * nx;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) t += A[r + 6 * c] * sLog[1][c];
        o[r] = -t;
      }
      const double* x0 = a.x0 + (size_t)b * (nq + nv);
      for (int i = 6; i < nv; ++i) o[i] = x0[1 + i] - q[1 + i];
      for (int i = 0; i < nv; ++i) o[nv + i] = x0[nq + i] - v[i];
    }
  }
}

}  // namespace rtoc
