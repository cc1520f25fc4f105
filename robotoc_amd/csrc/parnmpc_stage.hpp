// parnmpc_stage.hpp -- ParNMPCIntermediateStage / ParNMPCTerminalStage::evalKKT up to the dynamics (reference src/unconstr/
// parnmpc_intermediate_stage.cpp, parnmpc_terminal_stage.cpp:84-98), one wave per (instance, stage): kkt_matrix / kkt_residual.setZero(),
// the ConfigurationSpaceCost of a fixed-base robot scaled by dt on EVERY stage, the terminal cost ADDED on the last one
// (parnmpc_terminal_stage.cpp:88-93), and linearizeUnconstrBackwardEuler / ...Terminal (src/dynamics/unconstr_state_equation.cpp:
// 27-53, 65-72): Fq = q_prev - q + dt v, Fv = v_prev - v + dt a with (q_prev, v_prev) the previous stage's or, on stage 0, the
// initial state; lq += lmd_next - lmd, lv += dt lmd - gmm + gmm_next, la += dt gmm, the _next terms absent on the last stage.
// linearizeUnconstrDynamics then adds its terms on every stage (linearize_contact_dynamics_kernel in unconstrained mode).
// Records in the convention of rtoc_unconstr_condense: KKT.Quu := Qaa, KKT.lu := la, CDD.Qaa := diag(Quu), CDD.la := lu.
// Runtime kernels (not per shape): rt_parnmpc.hip launches them and is the one unit that includes this header.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"

namespace rtoc {

struct PnStageArgs {
  RecView rv;
  const double* cost;   // the table of rtoc_set_configuration_cost: 12 rows of nv + 1 doubles (contact_eval_kkt.hpp)
  const double* x0;     // [batch][2 nv] (q, v) of updateSolution(t, q, v): q_prev, v_prev of stage 0
  double dt;
};

static __global__ __launch_bounds__(64) void parnmpc_eval_kkt_kernel(PnStageArgs a) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / a.rv.nstages, st = blockIdx.x % a.rv.nstages;
  if (b >= a.rv.batch) return;
  const int nv = a.rv.nv(), nx = 2 * nv;
  const bool last = st == a.rv.nstages - 1;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  const double* const sn = s + a.rv.L.sol.stride;   // next stage (not read on the last one)
  const double* const sp = s - a.rv.L.sol.stride;   // previous stage (not read on stage 0)
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  const int M = nv + 1;
  const double *qr = a.cost, *vr = qr + M, *ur = vr + M, *wq = ur + M, *wv = wq + M, *wa = wv + M, *wu = wa + M, *wqf = wu + M, *wvf = wqf + M;
  const double dt = a.dt;
  for (int e = lane; e < nx * nx; e += 64) {
    const int r = e % nx, c = e / nx;
    double v = 0.0;
    if (r == c) v = r < nv ? dt * wq[r] + (last ? wqf[r] : 0.0) : dt * wv[r - nv] + (last ? wvf[r - nv] : 0.0);
    kr[a.rv.kkt_off(RTOC_KKT_QXX) + e] = v;
  }
  for (int e = lane; e < nx * nv; e += 64) kr[a.rv.kkt_off(RTOC_KKT_QXU) + e] = 0.0;
  for (int e = lane; e < nv * nv; e += 64) kr[a.rv.kkt_off(RTOC_KKT_QUU) + e] = (e % nv == e / nv) ? dt * wa[e % nv] : 0.0;
  for (int e = lane; e < nv * nv; e += 64) cr[a.rv.cdd_off(RTOC_CDD_MJTJINV) + e] = 0.0;  // off-diagonal part of Quu: a diagonal cost
  for (int i = lane; i < nv; i += 64) {
    const double q = s[a.rv.sol_off(RTOC_SOL_Q) + i], v = s[a.rv.sol_off(RTOC_SOL_V) + i], acc = s[a.rv.sol_off(RTOC_SOL_A) + i];
    const double u = s[a.rv.sol_off(RTOC_SOL_U) + i], lmd = s[a.rv.sol_off(RTOC_SOL_LMD) + i], gmm = s[a.rv.sol_off(RTOC_SOL_GMM) + i];
    const double qp = st == 0 ? a.x0[(size_t)b * nx + i] : sp[a.rv.sol_off(RTOC_SOL_Q) + i];
    const double vp = st == 0 ? a.x0[(size_t)b * nx + nv + i] : sp[a.rv.sol_off(RTOC_SOL_V) + i];
    const double lmdn = last ? 0.0 : sn[a.rv.sol_off(RTOC_SOL_LMD) + i], gmmn = last ? 0.0 : sn[a.rv.sol_off(RTOC_SOL_GMM) + i];
    double lq = dt * wq[i] * (q - qr[i]), lv = dt * wv[i] * (v - vr[i]);
    if (last) lq += wqf[i] * (q - qr[i]), lv += wvf[i] * (v - vr[i]);
    kr[a.rv.kkt_off(RTOC_KKT_FX) + i] = qp - q + dt * v;                          // Fq (:70)
    kr[a.rv.kkt_off(RTOC_KKT_FX) + nv + i] = vp - v + dt * acc;                   // Fv (:71)
    kr[a.rv.kkt_off(RTOC_KKT_LX) + i] = lq + (lmdn - lmd);                        // lq (:36, :50)
    kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + i] = lv + (dt * lmd - gmm + gmmn);        // lv (:37, :51)
    kr[a.rv.kkt_off(RTOC_KKT_LU) + i] = dt * wa[i] * acc + dt * gmm;              // la, in the lu slot (:38, :52)
    cr[a.rv.cdd_off(RTOC_CDD_LA) + i] = dt * wu[i] * (u - ur[i]);                 // lu (in CDD.la)
    cr[a.rv.cdd_off(RTOC_CDD_QAA) + i] = dt * wu[i];                              // diag(Quu)
  }
}

// initAuxMat (src/parnmpc/unconstr_backward_correction.cpp:57-71): every auxiliary matrix = the Hessian of the terminal cost at the
// last stage's iterate -- diag(q_weight_terminal, v_weight_terminal) for the ConfigurationSpaceCost of a fixed-base robot
static __global__ void parnmpc_init_aux_kernel(double* aux, const double* cost, int nv, long long nmat) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nx = 2 * nv, per = nx * nx;
  if (e >= nmat * per) return;
  const int k = (int)(e % per), r = k % nx, c = k / nx;
  const double *wqf = cost + 7 * (nv + 1), *wvf = wqf + (nv + 1);
  aux[e] = r != c ? 0.0 : (r < nv ? wqf[r] : wvf[r - nv]);
}

}  // namespace rtoc
