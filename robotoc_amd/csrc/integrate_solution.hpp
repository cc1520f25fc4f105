// integrate_solution.hpp -- SplitSolution::integrate.
//
// Replaces SplitSolution::integrate (reference src/core/split_solution.cpp:58-90) as called by
// {Intermediate,Impact,Terminal}Stage::updatePrimal (intermediate_stage.cpp:187-195, impact_stage.cpp:155-162,
// terminal_stage.cpp:139-148) from DirectMultipleShooting::integrateSolution
// (direct_multiple_shooting.cpp:212-241): every member is advanced by primal_step x direction.
// robot.integrateConfiguration (:62) is Pinocchio's manifold update: joints additively, a free-flyer base by the SE(3)
// exponential -- M <- M exp6(step dq_base): rotation exp(w), translation R V(w) v, quaternion product and
// re-normalisation (restated from the Lie-group formulas; Pinocchio absent).  Pure streaming: HBM-bound.
// The coefficients of V(w) are rbd::exp_coefficients (rigid_body_math.hpp): the series below |w| = 1e-3, 2 sin^2(t/2) / t^2
// above, since (1 - cos t) / t^2 put the position off by 1e-16 |v| / t -- what step dq_b of a nearly converged iteration meets.
// Held to a 50-digit reference from angle 0 to 4 (tests/test_lie_exp_branch_points.py): position within 0.0036 of
// 1e-13 max(1, |p|, |v|) (4.1e+04 of it at 1.01e-8 before), quaternion within 0.22 of 1e-15.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"

namespace rtoc {

struct IntArgs {
  RecView rv;  // sol: the one kernel that writes the iterate; steps: [batch][2] doubles, the primal one is read
};

static __global__ __launch_bounds__(64) void integrate_solution_kernel(IntArgs a) {
  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int b = item / a.rv.nstages, st = item % a.rv.nstages;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  const bool impact = g.type == RTOC_GRID_IMPACT;
  const double step = reinterpret_cast<const double*>(a.rv.steps)[2 * b];
  double* s = const_cast<double*>(a.rv.sol_at(item));
  const double* d = a.rv.dir_at(item);
  const int nv = a.rv.nv(), nu = a.rv.nu(), np = a.rv.L.dims.np;
  auto axpy = [&](int sfield, int n, const double* dv) {
    double* dst = s + a.rv.sol_off(sfield);
    for (int i = lane; i < n; i += 64) dst[i] += step * dv[i];
  };
  const double* dx = d + a.rv.dir_off(RTOC_DIR_DX);
  const double* dl = d + a.rv.dir_off(RTOC_DIR_DLMDGMM);
  const double* daf = d + a.rv.dir_off(RTOC_DIR_DAF);
  const double* dbm = d + a.rv.dir_off(RTOC_DIR_DBETAMU);
  // q (:62): fixed base q += step dq; floating base: q[7+j] += step dq[6+j] and the base by the SE(3) exponential
  {
    double* q = s + a.rv.sol_off(RTOC_SOL_Q);
    const int nb = np == 6 ? 6 : 0;
    for (int i = lane; i < nv - nb; i += 64) q[(nb ? 7 : 0) + i] += step * dx[nb + i];
    // step 0 (instances the convergence mask froze): the iterate is kept bit for bit, no re-normalisation
    if (nb && lane == 0 && step != 0.0) {
      const rbd::V3 v = step * rbd::ldv3(dx), wv = step * rbd::ldv3(dx + 3);
      const double th2 = rbd::dot(wv, wv), th = sqrt(th2);
      double S, A, B;
      rbd::exp_coefficients(th2, th, S, A, B);
      const double x = q[3], y = q[4], z = q[5], w = q[6];
      // R(quat) (V(w) v)
      const rbd::V3 dp = rbd::mul(rbd::quat_R(q + 3), rbd::exp6_translation(v, wv, A, B));
      q[0] += dp.x, q[1] += dp.y, q[2] += dp.z;
      // quat (x) (sin(t/2)/t w, cos(t/2)), normalised: the product, not the quaternion of R exp3(w), is what holds it to 1e-15
      const double sc = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(0.5 * th) / th, ew = cos(0.5 * th);
      const double e0 = sc * wv.x, e1 = sc * wv.y, e2 = sc * wv.z;
      const double r0 = w * e0 + x * ew + y * e2 - z * e1, r1 = w * e1 - x * e2 + y * ew + z * e0,
                   r2 = w * e2 + x * e1 - y * e0 + z * ew, r3 = w * ew - x * e0 - y * e1 - z * e2;
      const double n = 1.0 / sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
      q[3] = r0 * n, q[4] = r1 * n, q[5] = r2 * n, q[6] = r3 * n;
    }
  }
  axpy(RTOC_SOL_V, nv, dx + nv);                                   // (:63)
  if (!impact) {
    axpy(RTOC_SOL_A, nv, daf);                                     // a += step da (:65)
    axpy(RTOC_SOL_U, nu, d + a.rv.dir_off(RTOC_DIR_DU));           // (:67)
  } else {
    axpy(RTOC_SOL_A, nv, daf);                                     // dv += step ddv (:71); slot A holds dv
    for (int i = lane; i < nu; i += 64) s[a.rv.sol_off(RTOC_SOL_U) + i] = 0.0;  // u.setZero() (:72)
  }
  axpy(RTOC_SOL_LMD, nv, dl);                                      // (:74)
  axpy(RTOC_SOL_GMM, nv, dl + nv);                                 // (:75)
  axpy(RTOC_SOL_BETA, nv, dbm);                                    // (:76)
  if (np == 6 && !impact) axpy(RTOC_SOL_NUP, np, d + a.rv.dir_off(RTOC_DIR_DNUP));  // (:77-79)
  if (g.dimf > 0) {
    axpy(RTOC_SOL_F, g.dimf, daf + nv);                            // (:81)
    axpy(RTOC_SOL_MU, g.dimf, dbm + nv);                           // (:83)
  }
  if (g.dims > 0 && !impact) axpy(RTOC_SOL_XI, g.dims, d + a.rv.dir_off(RTOC_DIR_DXI));  // (:86-89)
}

}  // namespace rtoc
