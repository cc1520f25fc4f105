// switching_constraint_lin.hpp -- linearizeSwitchingConstraint on the device.
//
// Replaces linearizeSwitchingConstraint (reference src/dynamics/switching_constraint.cpp:26-70) on the grid point two ahead
// of an impact (GridInfo::switching_constraint): the contacts that become active at the impact must sit at their desired
// positions at the configuration predicted two steps ahead,
//     q+ = q (+) dq,   dq = (dt1 + dt2) v + dt1 dt2 a,   P = position(q+) - desired          (:14-23)
//     (surface contacts: P = Log6(X_desired^-1 X_frame(q+)), six rows, Pq = Jlog6 J_frame,local: surface_contact.hxx:106-128)
//     Pq = R_of J_frame,lin at q+ (point_contact.hxx:133-142),  Phiq = Pq dIntegrate_dq(q, dq),  Phiv = (dt1+dt2) Pq dIntegrate_dv(q, dq),
//     Phia = dt1 dt2 Pq dIntegrate_dv(q, dq)                                                  (:41-51)
// with Pinocchio's dIntegrate on the free-flyer base restated: dIntegrate_dq = Ad_{exp(dq_b)}^-1 (the motion actInv),
// dIntegrate_dv = Jexp6(dq_b) = Jlog6(exp6(dq_b))^-1 (six forward-mode evaluations through the log, one 6 x 6 inverse);
// identities on the joints.  Then the multiplier terms (:52-53) and the STO sensitivities (:54-62).
// Base-block transport: see RTOC_OPT_SWITCHING_TRANSPORT (rtoc.h) -- the reference's composition by default.
// exp6(dq_b) is rbd::exp6 (rigid_body_math.hpp), its coefficients rbd::exp_coefficients: the series below |w| = 1e-3,
// 2 sin^2(t/2) / t^2 above.  dq_b of a base that translates and barely turns has |w| of 1e-7 to 1e-5, where (1 - cos t) / t^2
// put q+, P and, through log6_fwd(E, pe), both transports off by 1e-16 |v| / t.  Held to a 50-digit reference from angle 0 to
// pi - 1e-3 (tests/test_lie_exp_branch_points.py): P within 0.0044 of 1e-13 max(1, |p|, |v|, |r_c|), Phiq within 0.0089 and
// Phiv, Phia within 0.073 of their bounds (4.1e+04 and 9.7e+03 of them at 1.01e-8 before).
// Mapping: one wave per (instance, switching grid point), one lane per dof: the lane carries its column of every body's
// Jacobian along the depth-first walk (body-frame twist per unit rate of the dof), values once per tree level in LDS.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"

namespace rtoc {

struct SwLinArgs {
  RecView rv;
  ModelDims md;
  int exact_transport;  // RTOC_OPT_SWITCHING_TRANSPORT
  int nsel, sel[16];    // the grid points with a switching constraint (nsel == 0: all grid points are launched)
};

__host__ __device__ constexpr size_t sw_lds_bytes(int nlevels, int njoints, int ncontacts) {
  return sizeof(double) * (rbd::LevelCarve(nlevels, njoints, ncontacts).doubles() + 3 * (RTOC_MAX_JOINTS + 8) +
                           6 * RTOC_MAX_CONTACTS * 8 + 2 * 36 + 6 * RTOC_MAX_CONTACTS * (RTOC_MAX_JOINTS + 8));
}

static __global__ __launch_bounds__(64) void switching_constraint_lin_kernel(SwLinArgs a) {
  using namespace rbd::slots;
  using rbd::M3;
  using rbd::SV;
  using rbd::V3;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  // launched over the grid points that carry a switching constraint only (sel), or over all of them (nsel == 0)
  const int nst1 = a.nsel > 0 ? a.nsel : a.rv.nstages - 1;
  const int b = blockIdx.x / nst1, st = a.nsel > 0 ? a.sel[blockIdx.x % nst1] : blockIdx.x % nst1;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  if (!g.switching_constraint || st + 2 >= a.rv.nstages) return;
  const int nv = a.rv.nv(), nx = 2 * nv, nb = a.md.njoints, ncon = a.md.ncontacts, nlev = a.md.nlevels, ns = g.dims, LDSW = a.rv.L.dims.ns_max;
  const double dt1 = grid_dt(a.rv.grid, a.rv.dt_inst, b, a.rv.nstages, st), dt2 = grid_dt(a.rv.grid, a.rv.dt_inst, b, a.rv.nstages, st + 1);
  const unsigned impact = a.rv.active[st + 2];  // ImpactStatus of the impact two grid points ahead
  const rbd::LevelCarve carve(nlev, nb, ncon);
  double* const lval = smem;                               // [nlev][LVL_VAL]: V_R .. V_OP of a value block
  double* const ltan = lval + carve.val;                   // [nlev][LVL_TAN][LVL_LANES]
  double* const sjm = ltan + carve.tan;
  double* const scm = sjm + carve.joint;
  double* const sqp = scm + carve.contact;                 // q+
  double* const sdq = sqp + RTOC_MAX_JOINTS + 8;           // dq
  double* const sxi = sdq + RTOC_MAX_JOINTS + 8;
  double* const spq = sxi + RTOC_MAX_JOINTS + 8;           // Pq base block [rows][8], then P residual etc.
  double* const sT = spq + 6 * RTOC_MAX_CONTACTS * 8;      // Tq (36) | Jr (36), column-major
  double* const sPq = sT + 72;                             // Pq [3 ncontacts][nv] row-major
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  {
    const double* const gj = &a.rv.model->joint[0][0];
    const double* const gc = &a.rv.model->contact[0][0];
    for (int e = lane; e < nb * JP; e += 64) sjm[e] = gj[e];
    for (int e = lane; e < ncon * CP; e += 64) scm[e] = gc[e];
  }
  for (int i = lane; i < nv; i += 64) sdq[i] = (dt1 + dt2) * s[a.rv.sol_off(RTOC_SOL_V) + i] + dt1 * dt2 * s[a.rv.sol_off(RTOC_SOL_A) + i];   // (:19)
  for (int i = lane; i < ns; i += 64) sxi[i] = s[a.rv.sol_off(RTOC_SOL_XI) + i];
  __syncthreads();
  // ---- q+ = q (+) dq (:20): joints additively, the base by the SE(3) exponential; X = exp6(dq_b) for the transports ----
  const int nbase = a.md.floating ? 6 : 0;
  for (int i = lane; i < nv - nbase; i += 64) sqp[(nbase ? 7 : 0) + i] = s[a.rv.sol_off(RTOC_SOL_Q) + (nbase ? 7 : 0) + i] + sdq[nbase + i];
  M3 E;     // rotation of exp6(dq_b)
  V3 pe = rbd::mk(0, 0, 0);
#pragma unroll
  for (int e = 0; e < 9; ++e) E.m[e] = (e % 4 == 0) ? 1.0 : 0.0;
  M3 Rb;    // base rotation at q+
  V3 pb = rbd::mk(0, 0, 0);
  if (a.md.floating) {
    rbd::exp6(rbd::ldv3(sdq), rbd::ldv3(sdq + 3), E, pe);
    const M3 R0 = rbd::quat_R(s + a.rv.sol_off(RTOC_SOL_Q) + 3);
    Rb = rbd::mul(R0, E);
    pb = rbd::ldv3(s + a.rv.sol_off(RTOC_SOL_Q)) + rbd::mul(R0, pe);
  }
  __syncthreads();
  // ---- depth-first walk at q+: values per level, this lane's Jacobian column (body-frame twist per unit rate of dof j) ----
  const int j = lane;
  const bool lane_on = j < nv;
  auto LV = [&](int lev, int k) -> double& { return lval[lev * LVL_VAL + k]; };
  auto LT = [&](int lev, int k) -> double& { return ltan[((size_t)lev * LVL_TAN + k) * LVL_LANES + lane]; };   // 0: linear, 3: angular
  auto JM = [&](int i, int k) -> const double& { return sjm[i * JP + k]; };
  for (int i = 0; i < nb; ++i) {
    const int d = (int)JM(i, J_DEPTH), iq = (int)JM(i, J_IDXQ), iv = (int)JM(i, J_IDXV);
    const bool ff = (int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER;
    const bool own = lane_on && j >= iv && j < iv + (ff ? 6 : 1);
    M3 Rj;
    V3 pj = rbd::mk(0, 0, 0);
    if (ff) {
      Rj = Rb;
      pj = pb;
    } else {
      const double th = sqp[iq];
      Rj = rbd::revolute_R(rbd::ldv3(&JM(i, J_AXIS)), sin(th), cos(th));
    }
    M3 R;
    V3 p;
    rbd::joint_placement(&JM(i, J_R), Rj, pj, R, p);
    M3 oR = R;
    V3 op = p;
    SV Jc = rbd::sv0();
    if (d > 0) {
      const M3 oRp = rbd::ldm3(&LV(d - 1, V_OR));
      oR = rbd::mul(oRp, R);
      op = rbd::ldv3(&LV(d - 1, V_OP)) + rbd::mul(oRp, p);
      Jc = rbd::act_inv(R, p, SV{rbd::mk(LT(d - 1, 0), LT(d - 1, 1), LT(d - 1, 2)), rbd::mk(LT(d - 1, 3), LT(d - 1, 4), LT(d - 1, 5))});
    }
    if (own) Jc = Jc + (ff ? rbd::unit_twist(j - iv) : SV{rbd::mk(0, 0, 0), rbd::ldv3(&JM(i, J_AXIS))});
#pragma unroll
    for (int k = 0; k < 9; ++k) LV(d, V_R + k) = R.m[k], LV(d, V_OR + k) = oR.m[k];
    rbd::stv3(&LV(d, V_P), p), rbd::stv3(&LV(d, V_OP), op);
    LT(d, 0) = Jc.l.x, LT(d, 1) = Jc.l.y, LT(d, 2) = Jc.l.z, LT(d, 3) = Jc.a.x, LT(d, 4) = Jc.a.y, LT(d, 5) = Jc.a.z;
    // impacting contacts carried by this body: P rows and this lane's column of Pq
    int r0 = 0;
    for (int c = 0; c < ncon; ++c) {
      const bool on = (impact >> c) & 1u;
      const bool surf = (int)scm[c * CP + C_TYPE] == RTOC_CONTACT_SURFACE;
      if (on && (int)scm[c * CP + C_PARENT] == i) {
        const M3 Rf = rbd::ldm3(&scm[c * CP + C_R]);
        const V3 pf = rbd::ldv3(&scm[c * CP + C_P]);
        const M3 oRf = rbd::mul(oR, Rf);
        const V3 pw = op + rbd::mul(oR, pf);
        const V3 pr = a.rv.positions ? rbd::ldv3(a.rv.positions + a.rv.placement(b, st + 2, ncon, c) * 3) : rbd::mk(0, 0, 0);
        const SV jf = rbd::act_inv(Rf, pf, Jc);   // this lane's column of the LOCAL frame Jacobian
        double* const Pres = spq + 6 * RTOC_MAX_CONTACTS * 4;
        if (!surf) {
          const V3 col = rbd::mul(oRf, jf.l);     // R_of J_frame,lin (point_contact.hxx:133-142)
          if (lane == 0) Pres[r0] = pw.x - pr.x, Pres[r0 + 1] = pw.y - pr.y, Pres[r0 + 2] = pw.z - pr.z;
          if (lane_on) sPq[(r0 + 0) * nv + j] = col.x, sPq[(r0 + 1) * nv + j] = col.y, sPq[(r0 + 2) * nv + j] = col.z;
        } else {
          // P = Log6(X_desired^-1 X_frame), Pq = Jlog6(X_diff) J_frame,local (surface_contact.hxx:106-128): forward mode
          M3 Rdt;   // transpose of the desired rotation (identity if none was set)
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
              Rdt.m[3 * r + cc] = a.rv.rotations ? a.rv.rotations[a.rv.placement(b, st + 2, ncon, c) * 9 + 3 * cc + r] : (r == cc ? 1.0 : 0.0);
          SV lg, dlg;
          rbd::log6_fwd(rbd::mul(Rdt, oRf), rbd::mul(Rdt, pw - pr), jf, lg, dlg);
          const double pv[6] = {lg.l.x, lg.l.y, lg.l.z, lg.a.x, lg.a.y, lg.a.z}, dv6[6] = {dlg.l.x, dlg.l.y, dlg.l.z, dlg.a.x, dlg.a.y, dlg.a.z};
#pragma unroll
          for (int t = 0; t < 6; ++t) {
            if (lane == 0) Pres[r0 + t] = pv[t];
            if (lane_on) sPq[(r0 + t) * nv + j] = dv6[t];
          }
        }
      }
      r0 += on ? (surf ? 6 : 3) : 0;
    }
  }
  // ---- transports of the base block: Tq = Ad_{exp(dq_b)}^-1, Jr = Jlog6(exp6(dq_b))^-1 ----
  if (a.md.floating && lane < 6) {
    const SV t = rbd::act_inv(E, pe, rbd::unit_twist(lane));
    const double tc[6] = {t.l.x, t.l.y, t.l.z, t.a.x, t.a.y, t.a.z};
    SV val, der;
    rbd::log6_fwd(E, pe, rbd::unit_twist(lane), val, der);
    const double jc[6] = {der.l.x, der.l.y, der.l.z, der.a.x, der.a.y, der.a.z};
#pragma unroll
    for (int r = 0; r < 6; ++r) sT[r + 6 * lane] = tc[r], sT[36 + r + 6 * lane] = jc[r];
  }
  __syncthreads();
  if (a.md.floating && lane == 0) {   // Jlog6 is block upper-triangular in the (linear, angular) ordering: 3 x 3 cofactor inverses
    double A[36];
    rbd::inv6_block_ut(sT + 36, A);
#pragma unroll
    for (int e = 0; e < 36; ++e) sT[36 + e] = A[e];
  }
  __syncthreads();
  // ---- Phiq, Phiv, Phia, P, Phit and the multiplier / STO terms ----
  const double* const P = spq + 6 * RTOC_MAX_CONTACTS * 4;
  if (lane_on) {
    double lq = 0.0, lvv = 0.0, laa = 0.0, pqxi = 0.0;
    for (int r = 0; r < ns; ++r) {
      double pq = sPq[r * nv + j], pqq = pq, pqv = pq;
      if (a.md.floating && j < 6) {
        pqq = 0.0, pqv = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          // the reference hands pinocchio::dIntegrateTransport the TRANSPOSED Jacobian (robot.hxx:69-72, :88-91), which
          // left-multiplies by dIntegrate: Phi^T = dIntegrate Pq^T, i.e. Phi = Pq dIntegrate^T; the chain rule is Pq dIntegrate
          const int e = a.exact_transport ? k + 6 * j : j + 6 * k;
          pqq += sPq[r * nv + k] * sT[e], pqv += sPq[r * nv + k] * sT[36 + e];
        }
      }
      kr[a.rv.kkt_off(RTOC_KKT_PHIX) + r + (size_t)j * LDSW] = pqq;                           // Phiq
      kr[a.rv.kkt_off(RTOC_KKT_PHIX) + r + (size_t)(nv + j) * LDSW] = (dt1 + dt2) * pqv;      // Phiv (:45-46)
      cr[a.rv.cdd_off(RTOC_CDD_PHIA) + r + (size_t)j * LDSW] = dt1 * dt2 * pqv;               // Phia
      lq += pqq * sxi[r], lvv += (dt1 + dt2) * pqv * sxi[r], laa += dt1 * dt2 * pqv * sxi[r], pqxi += pq * sxi[r];
    }
    kr[a.rv.kkt_off(RTOC_KKT_LX) + j] += lq;                 // lx += Phix^T xi (:52)
    kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + j] += lvv;
    cr[a.rv.cdd_off(RTOC_CDD_LA) + j] += laa;                // la += Phia^T xi (:53)
    kr[a.rv.kkt_off(RTOC_KKT_HX) + nv + j] += 2.0 * pqxi;    // hv += 2 Pq^T xi (:61)
    cr[a.rv.cdd_off(RTOC_CDD_HA) + j] += 2.0 * dt1 * pqxi;   // ha += 2 dt1 Pq^T xi (:62)
  }
  // Phit = Pq (2 (v + dt1 a)) (:56-57); h += xi . Phit (:58); Qtt += 2 (Pq^T xi) . a (:60)
  double hacc = 0.0, qacc = 0.0;
  for (int r = lane; r < ns; r += 64) {
    double t = 0.0, ta = 0.0;
    for (int k = 0; k < nv; ++k) t += sPq[r * nv + k] * 2.0 * (s[a.rv.sol_off(RTOC_SOL_V) + k] + dt1 * s[a.rv.sol_off(RTOC_SOL_A) + k]), ta += sPq[r * nv + k] * s[a.rv.sol_off(RTOC_SOL_A) + k];
    kr[a.rv.kkt_off(RTOC_KKT_PHIT) + r] = t;
    kr[a.rv.kkt_off(RTOC_KKT_PRES) + r] = P[r];
    hacc += sxi[r] * t;
    qacc += 2.0 * sxi[r] * ta;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) hacc += __shfl_xor(hacc, off, 64), qacc += __shfl_xor(qacc, off, 64);
  if (lane == 0) {
    kr[a.rv.kkt_off(RTOC_KKT_SCAL) + RTOC_KKT_SCAL_H] += hacc;
    kr[a.rv.kkt_off(RTOC_KKT_SCAL) + RTOC_KKT_SCAL_QTT] += qacc;
  }
}

}  // namespace rtoc
