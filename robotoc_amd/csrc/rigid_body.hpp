// rigid_body.hpp -- batched linearisation of the contact / impact dynamics.
//
// Replaces, per (instance, grid point): Robot::RNEA / RNEADerivatives / RNEAImpact / RNEAImpactDerivatives (reference
// include/robotoc/robot/robot.hxx:524-624, thin wrappers over pinocchio::rnea / computeRNEADerivatives), setContactForces
// (:455-517), computeBaumgarteResidual / Derivatives (:291-360 -> point_contact.hxx:14-83) and computeImpactVelocity
// Residual / Derivatives (point_contact.hxx:84-117), i.e. linearizeContactDynamics (src/dynamics/contact_dynamics.cpp:12-33)
// and linearizeImpactDynamics (impact_dynamics.cpp:8-27) up to the multiplier terms.
//
// Mapping: one wave per grid point, one LANE per tangent direction (dof j, kind in {q, v, a}): 21 dofs per pass.  Every
// lane walks the kinematic tree depth first and carries the forward-mode derivative of Featherstone's recursive
// Newton-Euler along its direction:
//     v_i = X v_p + S vq                      dv_i = X dv_p - [own q] S_k x (X v_p) + [own v] S_k
//     a_i = X a_p + S aq + v_i x S vq         da_i = X da_p - [own q] S_k x (X a_p) + [own a] S_k + dv_i x S vq + [own v] v_i x S_k
//     f_i = Y (a_i + g_i) + v_i x* Y v_i - fext_i
//     f_p += X* f_i                           df_p += X* df_i + [own q] X* (S_k x* f_i)          tau_i = S^T f_i
// (d(X m)/dq_k = -S_k x (X m), d(X* f)/dq_k = X* (S_k x* f) for the joint's own coordinate k; q perturbed on the
// manifold, q (+) dq: local translation / rotation of a free-flyer root.)  The VALUES are the same in every lane and
// live once per tree level in LDS; the TANGENTS (dv, da, dg, df: 21 doubles) live per lane and level in LDS,
// lane-strided (conflict-free).  Only the current root-to-body path is live: LDS = levels x (21 x 64 + ~60) doubles.
// The contact rows ride on the visit of the body that carries the frame; d(position)/dq = R_of * (frame Jacobian), whose
// column j is the v-tangent of the frame velocity -- held by the neighbouring lane (point_contact.hxx:78-80).
//
// The kernels and their argument blocks: rt_eval_kkt.hip launches them and is the one unit that includes this header.  The
// model they read and the plan of the walk are rigid_body_model.hpp (host), the spatial arithmetic is rigid_body_math.hpp.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"
#include "../../include/rtoc_robot.h"

#ifndef RTOC_RBD_WAVES
#define RTOC_RBD_WAVES
#endif

namespace rtoc {
namespace rbd {

struct LinArgs {
  RecView rv;           // kkt == nullptr: the multiplier terms of linearizeContactDynamics / linearizeImpactDynamics are left out
  ModelDims md;
  // UnconstrDynamics::linearizeUnconstrDynamics (unconstr_dynamics.cpp:52-64): the multiplier terms carry dt, and the
  // records follow the convention of rtoc_unconstr_condense (la lives in KKT.lu, lu in CDD.la)
  int unconstr;
  double scale;
  const double* vals;   // PRE: [batch * nstages][njoints][VAL_DOUBLES] of the dynamics traversal (rbd_values_kernel)
  const double* vals2;  //      the same for the kinematics traversal of impact grids
};

// ---------------------------------------------------------------------------------------------------------------------
// Values of the recursion, ahead of the tangent walk (PRE mode of linearize_contact_dynamics_kernel).
//
// The walk below is one dependent instruction stream per wave, and the lane-invariant VALUES of the recursion (joint
// transforms incl. a sincos per joint, placements, velocities, accelerations, forces) were ~40 % of it, recomputed by every
// lane, body after body.  They are level-parallel instead: here lanes = bodies, one pass down the levels of the tree
// (placements, v, a, own force) and one pass up the bodies in reverse depth-first order (forces of the children), several
// grid points per wave (64 / next power of two >= njoints).  Out: the value block of every body (V_R .. V_H, VAL_DOUBLES doubles:
// rigid_body_model.hpp) -- the block the walk copies into its per-level value slots when it visits the body -- and the inverse-dynamics residual ID
// (the value part of RTOC_CDD_IDC).  trav: 0 = the dynamics traversal, 1 = the kinematics traversal at v + dv of impact
// grids (impact_stage.cpp:61), other grids idle.
struct ValArgs {
  RecView rv;           // positions / rotations: the desired contact placements (the value rows of C below)
  ModelDims md;
  double* vals;         // [batch * nstages][njoints][VAL_DOUBLES]
  int trav, unconstr;
  int nsel, sel[16];    // nsel > 0: only the grid points sel[0..nsel) of every instance (the impact grids of trav 1)
};

static __global__ __launch_bounds__(64) void rbd_values_kernel(ValArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];   // [G][njoints][VAL_DOUBLES]
  const int lane = threadIdx.x, GS = a.md.gs, G = 64 / GS, nb = a.md.njoints, ncon = a.md.ncontacts;
  const int grp = lane / GS, i = lane % GS;
  const int nst1 = a.nsel > 0 ? a.nsel : a.rv.nlin();   // grid points per instance this launch covers
  const long long item = (long long)blockIdx.x * G + grp, nitems = (long long)a.rv.batch * nst1;
  const bool gvalid = item < nitems;
  const int b = gvalid ? (int)(item / nst1) : 0;
  const int st = !gvalid ? 0 : (a.nsel > 0 ? a.sel[item % nst1] : (int)(item % nst1));
  const rtoc_grid g = a.rv.grid[st];
  const bool impact = g.type == RTOC_GRID_IMPACT;
  const bool dyn = a.trav == 0;
  const bool on = gvalid && i < nb && (dyn || impact);
  const int ib = i < nb ? i : 0;
  double* const V = smem + (size_t)grp * nb * VAL_DOUBLES;
  double* const me = V + (size_t)ib * VAL_DOUBLES;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const sr = a.rv.sol_at(rec);
  const unsigned active = a.rv.active[st];
  const int nv = a.rv.nv(), nu = a.rv.nu();
  // ---- this body's constants and joint state ----
  const double* const jm = &a.rv.model->joint[ib][0];
  const int type = (int)jm[J_TYPE], iq = (int)jm[J_IDXQ], iv = (int)jm[J_IDXV], depth = (int)jm[J_DEPTH];
  const int par = a.rv.model->m.parent[ib];
  const bool ff = type == RTOC_JOINT_FREE_FLYER;
  const V3 ax = ldv3(jm + J_AXIS);
  M3 Rj;
  V3 pj = mk(0, 0, 0);
  SV vj, aj;
  if (ff) {
    Rj = quat_R(sr + a.rv.sol_off(RTOC_SOL_Q) + iq + 3);
    pj = ldv3(sr + a.rv.sol_off(RTOC_SOL_Q) + iq);
    vj = SV{ldv3(sr + a.rv.sol_off(RTOC_SOL_V) + iv), ldv3(sr + a.rv.sol_off(RTOC_SOL_V) + iv + 3)};
    aj = SV{ldv3(sr + a.rv.sol_off(RTOC_SOL_A) + iv), ldv3(sr + a.rv.sol_off(RTOC_SOL_A) + iv + 3)};
    if (impact && !dyn) vj = vj + aj;  // kinematics at v + dv
  } else {
    const double th = sr[a.rv.sol_off(RTOC_SOL_Q) + iq];
    Rj = revolute_R(ax, sin(th), cos(th));
    const double vq = (impact && !dyn) ? sr[a.rv.sol_off(RTOC_SOL_V) + iv] + sr[a.rv.sol_off(RTOC_SOL_A) + iv] : sr[a.rv.sol_off(RTOC_SOL_V) + iv];
    vj = SV{mk(0, 0, 0), vq * ax};
    aj = SV{mk(0, 0, 0), sr[a.rv.sol_off(RTOC_SOL_A) + iv] * ax};
  }
  if (impact && dyn) vj = sv0();   // impact model: v = 0
  if (impact && !dyn) aj = sv0();  // velocity-level rows only
  M3 R;
  V3 p;
  joint_placement(jm + J_R, Rj, pj, R, p);
  const double mass = jm[J_MASS];
  const V3 com = ldv3(jm + J_COM);
  const M3 I = ldm3(jm + J_INERTIA);
  // ---- down the levels: placements, velocities, accelerations, own forces ----
  for (int d = 0; d < a.md.nlevels; ++d) {
    if (on && depth == d) {
      M3 oR = R;
      V3 op = p;
      SV vpar = sv0(), apar = sv0();
      V3 gi = mulT(R, mk(-a.md.gx, -a.md.gy, -a.md.gz));
      if (d > 0) {
        const double* const pa = V + (size_t)par * VAL_DOUBLES;
        const M3 oRp = ldm3(pa + V_OR);
        oR = mul(oRp, R);
        op = ldv3(pa + V_OP) + mul(oRp, p);
        vpar = act_inv(R, p, ldsv(pa + V_V));
        apar = act_inv(R, p, ldsv(pa + V_A));
        gi = mulT(R, ldv3(pa + V_G));
      }
      if (impact) gi = mk(0, 0, 0);  // the impact model has no gravity
      const SV v = vpar + vj;
      const SV acc = apar + aj + mcross(v, vj);
      const SV h = inertia_mul(mass, com, I, v);
      SV f = inertia_mul(mass, com, I, SV{acc.l + gi, acc.a}) + fcross(v, h);
      int roff = 0;
      for (int c = 0; c < ncon; ++c) {
        const double* const cm = &a.rv.model->contact[c][0];
        const bool con_on = (active >> c) & 1u;
        const bool surf = (int)cm[C_TYPE] == RTOC_CONTACT_SURFACE;
        if (con_on && (int)cm[C_PARENT] == ib) {
          const SV fc = SV{ldv3(sr + a.rv.sol_off(RTOC_SOL_F) + roff), surf ? ldv3(sr + a.rv.sol_off(RTOC_SOL_F) + roff + 3) : mk(0, 0, 0)};
          f = f - act_f(ldm3(cm + C_R), ldv3(cm + C_P), fc);
        }
        roff += con_on ? (surf ? 6 : 3) : 0;
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) me[V_R + k] = R.m[k], me[V_OR + k] = oR.m[k];
      stv3(me + V_P, p), stv3(me + V_OP, op);
      stsv(me + V_V, v), stsv(me + V_A, acc);
      stv3(me + V_G, gi);
      stsv(me + V_F, f);
      me[V_BODY] = (double)ib;
      stsv(me + V_VPAR, vpar), stsv(me + V_APAR, apar), stsv(me + V_H, h);
    }
    __syncthreads();
  }
  // ---- up the bodies, children before parents (reverse depth-first order): total forces ----
  for (int k = nb - 1; k >= 1; --k) {
    const int pk = a.rv.model->m.parent[k];
    if (on && ib == pk) {
      const double* const ch = V + (size_t)k * VAL_DOUBLES;
      stsv(me + V_F, ldsv(me + V_F) + act_f(ldm3(ch + V_R), ldv3(ch + V_P), ldsv(ch + V_F)));
    }
    __syncthreads();
  }
  // ---- ID = S^T f - [0; u] (the value rows of RTOC_CDD_IDC; contact_dynamics.cpp:21-24, impact_dynamics.cpp:12-14) ----
  if (on && dyn) {
    double* const cr = a.rv.cdd_at(rec);
    const SV f = ldsv(me + V_F);
    if (ff) {
      const double fv[6] = {f.l.x, f.l.y, f.l.z, f.a.x, f.a.y, f.a.z};
#pragma unroll
      for (int k = 0; k < 6; ++k) cr[a.rv.cdd_off(RTOC_CDD_IDC) + iv + k] = fv[k] - ((!impact && iv + k >= nv - nu) ? sr[a.rv.sol_off(RTOC_SOL_U) + iv + k - (nv - nu)] : 0.0);
    } else {
      cr[a.rv.cdd_off(RTOC_CDD_IDC) + iv] = dot(ax, f.a) - ((!impact && iv >= nv - nu) ? sr[a.rv.sol_off(RTOC_SOL_U) + iv - (nv - nu)] : 0.0);
    }
  }
  // ---- C = the Baumgarte residual of the contacts this body carries (point_contact.hxx:14-31, surface_contact.hxx:12-29), on
  //      impact grids the contact velocity at v + dv from the kinematics traversal (point_contact.hxx:84-96): the value rows
  //      nv.. of RTOC_CDD_IDC.  Lane-invariant in the tangent walk, which used to evaluate them in every lane. ----
  if (on && (impact ? !dyn : dyn)) {
    double* const cr = a.rv.cdd_at(rec);
    const SV v = ldsv(me + V_V), acc = ldsv(me + V_A);
    const M3 oR = ldm3(me + V_OR);
    const V3 op = ldv3(me + V_OP);
    int roff = 0;
    for (int c = 0; c < ncon; ++c) {
      const double* const cm = &a.rv.model->contact[c][0];
      const bool con_on = (active >> c) & 1u;
      const bool surf = (int)cm[C_TYPE] == RTOC_CONTACT_SURFACE;
      const int nr = surf ? 6 : 3;
      if (con_on && (int)cm[C_PARENT] == ib) {
        const M3 Rf = ldm3(cm + C_R);
        const V3 pf = ldv3(cm + C_P);
        const SV vf = act_inv(Rf, pf, v);
        SV C = vf;
        if (!impact) {
          const SV af = act_inv(Rf, pf, acc);
          const double kp = cm[C_KP], kd = cm[C_KD];
          const V3 pw = op + mul(oR, pf);
          const V3 pr = a.rv.positions ? ldv3(a.rv.positions + a.rv.placement(b, st, ncon, c) * 3) : mk(0, 0, 0);
          if (!surf) {
            C.l = af.l + cross(vf.a, vf.l) + kd * vf.l + kp * (pw - pr);
          } else {
            M3 Rdt;   // transpose of the desired rotation
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) Rdt.m[3 * r + cc] = a.rv.rotations ? a.rv.rotations[a.rv.placement(b, st, ncon, c) * 9 + 3 * cc + r] : (r == cc ? 1.0 : 0.0);
            SV lg, dlg;
            log6_fwd(mul(Rdt, mul(oR, Rf)), mul(Rdt, pw - pr), sv0(), lg, dlg);
            C = SV{af.l + kd * vf.l + kp * lg.l, af.a + kd * vf.a + kp * lg.a};
          }
        }
        const double Cv[6] = {C.l.x, C.l.y, C.l.z, C.a.x, C.a.y, C.a.z};
        for (int t = 0; t < nr; ++t) cr[a.rv.cdd_off(RTOC_CDD_IDC) + nv + roff + t] = Cv[t];
      }
      roff += con_on ? nr : 0;
    }
  }
  // ---- the blocks out, coalesced ----
  const int per = nb * VAL_DOUBLES;
  for (int e = lane; e < G * per; e += 64) {
    const int g2 = e / per;
    const long long it2 = (long long)blockIdx.x * G + g2;
    if (it2 >= nitems) continue;
    const int b2 = (int)(it2 / nst1), st2 = a.nsel > 0 ? a.sel[it2 % nst1] : (int)(it2 % nst1);
    if (!dyn && a.rv.grid[st2].type != RTOC_GRID_IMPACT) continue;
    a.vals[((size_t)b2 * a.rv.nstages + st2) * per + (e - g2 * per)] = smem[e];
  }
}

// SURF: the model has surface contacts (6 rows, Log6 of the placement error); compiled out for point-contact robots, where
// its registers and branches cost 10 % of the kernel
// PRE: the values of the recursion come from rbd_values_kernel (a.vals / a.vals2): the visit copies the body's block into
// the level's value slots instead of computing it, and the force accumulation / ID rows are not repeated here.
template <bool SURF, bool PRE = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((PRE && !SURF) ? 2 : 1))) void linearize_contact_dynamics_kernel(LinArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int nst1 = a.rv.nlin();
  const int b = item / nst1, st = item % nst1;
  if (b >= a.rv.batch) return;
  const int nlev = a.md.nlevels, nv = a.rv.nv(), nb = a.md.njoints, ncon = a.md.ncontacts;
  const rtoc_grid g = a.rv.grid[st];
  const bool impact = g.type == RTOC_GRID_IMPACT;
  const unsigned active = a.rv.active[st];
  double* const lval = smem;                                      // [nlev][VAL_DOUBLES]
  const int LW = lin_lane_stride(a.md.dpp);
  double* const lfwd = lval + (size_t)nlev * VAL_DOUBLES;         // [nbranch][FWD_SLOTS][LW]: dv, da, dg of the branching bodies
  double* const ldf = lfwd + (size_t)a.md.nbranch * FWD_SLOTS * LW;  // [nlev - 1][DF_SLOTS][LW]: df of the open non-leaf levels
  double* const sq = ldf + (size_t)(nlev > 1 ? nlev - 1 : 0) * DF_SLOTS * LW;   // q, v, a, f, u of the grid point
  double* const sv = sq + (PRE ? 0 : lin_pad8(nv + 1));   // (PRE: the staging vectors of the values are not allocated)
  double* const sa = sv + (PRE ? 0 : lin_pad8(nv));
  double* const sf = sa + (PRE ? 0 : lin_pad8(nv));
  double* const su = sf + (PRE ? 0 : lin_pad8(6 * ncon));
  double* const sbeta = su + (PRE ? 0 : lin_pad8(nv));  // multipliers of the dynamics (beta) and of the contact rows (mu)
  double* const smu = sbeta + lin_pad8(nv);
  double* const slf = smu + lin_pad8(6 * ncon);         // dC/da beta, accumulated over the passes
  constexpr int JPW = PRE ? JP_PRE : JP, JOFF = PRE ? JP_PRE_OFF : 0;
  double* const sjm = slf + lin_pad8(6 * ncon);         // model: [njoints][JPW] (PRE: axis .. depth only), then [ncontacts][CP]
  double* const scm = sjm + a.md.njoints * JPW;
  const bool aug = a.rv.kkt != nullptr;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const sr = a.rv.sol_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  const int nu = a.rv.nu();
  {
    const double* const gj = &a.rv.model->joint[0][0];
    const double* const gc = &a.rv.model->contact[0][0];
    for (int e = lane; e < nb * JPW; e += 64) sjm[e] = gj[(e / JPW) * JP + JOFF + e % JPW];
    for (int e = lane; e < ncon * CP; e += 64) scm[e] = gc[e];
  }
  if constexpr (!PRE) {
    for (int e = lane; e < a.md.nq; e += 64) sq[e] = sr[a.rv.sol_off(RTOC_SOL_Q) + e];
    for (int e = lane; e < nv; e += 64) {
      sv[e] = sr[a.rv.sol_off(RTOC_SOL_V) + e];
      sa[e] = sr[a.rv.sol_off(RTOC_SOL_A) + e];
    }
    for (int e = lane; e < g.dimf; e += 64) sf[e] = sr[a.rv.sol_off(RTOC_SOL_F) + e];
    for (int e = lane; e < nu; e += 64) su[e] = sr[a.rv.sol_off(RTOC_SOL_U) + e];
  }
  if (aug) {
    for (int e = lane; e < nv; e += 64) sbeta[e] = sr[a.rv.sol_off(RTOC_SOL_BETA) + e];
    for (int e = lane; e < g.dimf; e += 64) smu[e] = sr[a.rv.sol_off(RTOC_SOL_MU) + e];
    for (int e = lane; e < 6 * ncon; e += 64) slf[e] = 0.0;
  }
  __syncthreads();
  const V3 grav = mk(a.md.gx, a.md.gy, a.md.gz);
  // impact grids: a dynamics traversal (zero gravity, zero velocity, acceleration = dv; robot.hxx:590-624) and a
  // kinematics traversal at v + dv for the contact-velocity rows (impact_stage.cpp:61); other grids: one traversal
  const int ntrav = impact ? 2 : 1;
  for (int trav = 0; trav < ntrav; ++trav) {
    const bool dyn = trav == 0;                 // writes ID and its derivatives
    const bool rows = !impact || trav == 1;     // writes C and its derivatives
    for (int j0 = 0, ps = 0; j0 < nv; j0 += a.md.dpp, ++ps) {
      const int j = j0 + lane / 3, kind = lane % 3;  // 0: q, 1: v, 2: a
      const bool lane_on = lane < 3 * a.md.dpp && j < nv;
      // (without the values pre-pass every pass accumulates the forces of all bodies: no skipping)
      const unsigned long long visit_mask = PRE ? a.rv.model->pass_bodies[ps] : ~0ull;
      int top = -1;
      double wsum = 0.0;  // this lane's column of [dID; dC] against [beta; mu]
      // body of the level that is being closed / visited is kept in LDS as an int in the value block
      auto LV = [&](int lev, int k) -> double& { return lval[lev * VAL_DOUBLES + k]; };
      // forward-tangent slot / force-tangent level of this lane; lanes beyond the stride (idle ones) share the last column
      const int ln = lane < LW ? lane : LW - 1;
      auto FT = [&](int slot, int k) -> double& { return lfwd[((size_t)slot * FWD_SLOTS + k) * LW + ln]; };
      auto DT = [&](int lev, int k) -> double& { return ldf[((size_t)lev * DF_SLOTS + k) * LW + ln]; };
      auto ld_sv = [&](int lev, int k0) { return ldsv(&LV(lev, k0)); };
      auto st_sv = [&](int lev, int k0, SV x) { stsv(&LV(lev, k0), x); };
      auto ld_ft = [&](int slot, int k0) { return SV{mk(FT(slot, k0), FT(slot, k0 + 1), FT(slot, k0 + 2)), mk(FT(slot, k0 + 3), FT(slot, k0 + 4), FT(slot, k0 + 5))}; };
      auto st_ft = [&](int slot, int k0, SV x) {
        FT(slot, k0) = x.l.x, FT(slot, k0 + 1) = x.l.y, FT(slot, k0 + 2) = x.l.z, FT(slot, k0 + 3) = x.a.x, FT(slot, k0 + 4) = x.a.y, FT(slot, k0 + 5) = x.a.z;
      };
      auto ld_dt = [&](int lev) { return SV{mk(DT(lev, 0), DT(lev, 1), DT(lev, 2)), mk(DT(lev, 3), DT(lev, 4), DT(lev, 5))}; };
      auto st_dt = [&](int lev, SV x) { DT(lev, 0) = x.l.x, DT(lev, 1) = x.l.y, DT(lev, 2) = x.l.z, DT(lev, 3) = x.a.x, DT(lev, 4) = x.a.y, DT(lev, 5) = x.a.z; };
      // value slots: V_R .. V_BODY (PRE: the whole block, .. V_H) of rigid_body_model.hpp; forward-tangent slots: 0 dv, 6 da, 12 dg
      SV tdv = sv0(), tda = sv0(), cdf = sv0();   // forward tangents of the body visited last; force tangent of an open leaf
      V3 tdg = mk(0, 0, 0);
      bool topreg = false;                        // the force tangent of level `top` is cdf (a leaf), not in LDS
      auto JM = [&](int i, int k) -> const double& { return sjm[i * JPW + k - JOFF]; };
      auto unit_twist = [&](int i, int k) -> SV {  // S_k of joint i
        if ((int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER) return rbd::unit_twist(k);
        return SV{mk(0, 0, 0), ldv3(&JM(i, J_AXIS))};
      };
      auto close = [&](int lev, bool from_reg) {
        const int i = (int)LV(lev, V_BODY);
        const M3 R = ldm3(&LV(lev, V_R));
        const V3 p = ldv3(&LV(lev, V_P));
        const SV f = ld_sv(lev, V_F), df = from_reg ? cdf : ld_dt(lev);
        const int iv = (int)JM(i, J_IDXV);
        const bool cff = (int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER;
        const bool own = lane_on && j >= iv && j < iv + (cff ? 6 : 1);
        if (dyn) {
          // tau = S^T f: value (lane 0) and this lane's column
          double* const dcol = kind == 2 ? cr + a.rv.cdd_off(RTOC_CDD_DIDDA) + (size_t)j * nv : cr + a.rv.cdd_off(RTOC_CDD_DIDCDQV) + (size_t)(kind == 1 ? nv + j : j) * a.rv.L.nvf_max;
          if (cff) {
            const double fv[6] = {f.l.x, f.l.y, f.l.z, f.a.x, f.a.y, f.a.z}, dv6[6] = {df.l.x, df.l.y, df.l.z, df.a.x, df.a.y, df.a.z};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
              if (!PRE && lane == 0 && j0 == 0) cr[a.rv.cdd_off(RTOC_CDD_IDC) + iv + k] = fv[k] - ((!impact && iv + k >= nv - nu) ? su[iv + k - (nv - nu)] : 0.0);
              if (lane_on) dcol[iv + k] = dv6[k];
              if (aug) wsum += dv6[k] * sbeta[iv + k];
            }
          } else {
            const V3 ax = ldv3(&JM(i, J_AXIS));
            if (!PRE && lane == 0 && j0 == 0) cr[a.rv.cdd_off(RTOC_CDD_IDC) + iv] = dot(ax, f.a) - ((!impact && iv >= nv - nu) ? su[iv - (nv - nu)] : 0.0);
            if (lane_on) dcol[iv] = dot(ax, df.a);
            if (aug) wsum += dot(ax, df.a) * sbeta[iv];
          }
        }
        if (lev > 0) {
          SV dfp = act_f(R, p, df);
          if (own && kind == 0) {   // a body with a parent is a revolute joint: S = (0, axis)
            const V3 ax = ldv3(&JM(i, J_AXIS));
            dfp = dfp + act_f(R, p, SV{cross(ax, f.l), cross(ax, f.a)});
          }
          if (!PRE) st_sv(lev - 1, V_F, ld_sv(lev - 1, V_F) + act_f(R, p, f));   // PRE: the block already holds the total force
          st_dt(lev - 1, ld_dt(lev - 1) + dfp);
        }
      };
      // bodies no direction of this pass moves or loads: their entries of the pass's columns are zero
      if (PRE && ps > 0)
        for (int i = 0; i < nb; ++i) {
          if ((visit_mask >> i) & 1ull) continue;
          const int iv = (int)JM(i, J_IDXV);
          if (dyn && lane_on) {
            double* const dcol = kind == 2 ? cr + a.rv.cdd_off(RTOC_CDD_DIDDA) + (size_t)j * nv : cr + a.rv.cdd_off(RTOC_CDD_DIDCDQV) + (size_t)(kind == 1 ? nv + j : j) * a.rv.L.nvf_max;
            const int ndof = (int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER ? 6 : 1;
            for (int k = 0; k < ndof; ++k) dcol[iv + k] = 0.0;
          }
          if (rows) {
            int roff = 0;
            for (int c = 0; c < ncon; ++c) {
              const bool on = (active >> c) & 1u;
              const int nr = (SURF && (int)scm[c * CP + C_TYPE] == RTOC_CONTACT_SURFACE) ? 6 : 3;
              if (on && (int)scm[c * CP + C_PARENT] == i && lane_on)
                for (int t = 0; t < nr; ++t) {
                  if (kind == 2 || (impact && kind == 1)) cr[a.rv.cdd_off(RTOC_CDD_DCDA) + (size_t)j * a.rv.L.dims.nf_max + roff + t] = 0.0;
                  if (kind != 2) cr[a.rv.cdd_off(RTOC_CDD_DIDCDQV) + (size_t)(kind == 1 ? nv + j : j) * a.rv.L.nvf_max + nv + roff + t] = 0.0;
                }
              roff += on ? nr : 0;
            }
          }
        }
      const double* const vblk = PRE ? (dyn ? a.vals : a.vals2) + rec * (size_t)nb * VAL_DOUBLES : nullptr;
      double pv = PRE ? vblk[lane] : 0.0;   // body 0 is in every pass
      const int* const vlist = a.rv.model->pass_visit[ps];
      const int nvisit = PRE ? sload_int(a.rv.model->pass_nvisit + ps) : nb;
      for (int t = 0; t < nvisit; ++t) {
        const int i = PRE ? sload_int(vlist + t) : t;   // the bodies a direction of this pass moves or loads, depth first
        const int d = (int)JM(i, J_DEPTH);
        while (top >= d) {
          close(top, topreg);
          topreg = false;
          --top;
        }
        // ---- visit body i at level d ----
        const int wk = sload_int(a.rv.model->walk + i);
        const bool chain = wk & 1, leaf = wk & 2;
        const int sslot = ((wk >> 4) & 15) - 1, pslot = ((wk >> 8) & 15) - 1;
        const int iq = (int)JM(i, J_IDXQ), iv = (int)JM(i, J_IDXV);
        const bool ff = (int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER;
        const bool own = lane_on && j >= iv && j < iv + (ff ? 6 : 1);
        M3 R, oR;
        V3 p, op, gi;
        SV vpar, apar, v, acc, vj;
        if constexpr (PRE) {
          // the body's block from rbd_values_kernel (requested one body ahead) into the level's value slots
          LV(d, lane) = pv;
          if (t + 1 < nvisit) pv = vblk[(size_t)sload_int(vlist + t + 1) * VAL_DOUBLES + lane];
          __builtin_amdgcn_wave_barrier();
          R = ldm3(&LV(d, V_R)), oR = ldm3(&LV(d, V_OR));
          p = ldv3(&LV(d, V_P)), op = ldv3(&LV(d, V_OP)), gi = ldv3(&LV(d, V_G));
          v = ld_sv(d, V_V), acc = ld_sv(d, V_A), vpar = ld_sv(d, V_VPAR), apar = ld_sv(d, V_APAR);
          vj = v - vpar;
        } else {
        M3 Rj;
        V3 pj = mk(0, 0, 0);
        SV aj;  // S aq (vj = S vq)
        if (ff) {
          Rj = quat_R(sq + iq + 3);
          pj = mk(sq[iq], sq[iq + 1], sq[iq + 2]);
          vj = SV{mk(sv[iv], sv[iv + 1], sv[iv + 2]), mk(sv[iv + 3], sv[iv + 4], sv[iv + 5])};
          aj = SV{mk(sa[iv], sa[iv + 1], sa[iv + 2]), mk(sa[iv + 3], sa[iv + 4], sa[iv + 5])};
          if (impact && !dyn) vj = vj + aj;  // kinematics at v + dv
        } else {
          const V3 ax = ldv3(&JM(i, J_AXIS));
          const double th = sq[iq];
          Rj = revolute_R(ax, sin(th), cos(th));
          const double vq = (impact && !dyn) ? sv[iv] + sa[iv] : sv[iv];
          vj = SV{mk(0, 0, 0), vq * ax};
          aj = SV{mk(0, 0, 0), sa[iv] * ax};
        }
        if (impact && dyn) vj = sv0();   // impact model: v = 0
        if (impact && !dyn) aj = sv0();  // velocity-level rows only
        joint_placement(&JM(i, J_R), Rj, pj, R, p);
        oR = R;
        op = p;
        vpar = sv0(), apar = sv0();
        gi = mulT(R, mk(-grav.x, -grav.y, -grav.z));
        if (d > 0) {
          const M3 oRp = ldm3(&LV(d - 1, V_OR));
          oR = mul(oRp, R);
          op = ldv3(&LV(d - 1, V_OP)) + mul(oRp, p);
          vpar = act_inv(R, p, ld_sv(d - 1, V_V));
          apar = act_inv(R, p, ld_sv(d - 1, V_A));
          gi = mulT(R, ldv3(&LV(d - 1, V_G)));
        }
        if (impact) gi = mk(0, 0, 0);  // the impact model has no gravity
        v = vpar + vj;
        acc = apar + aj + mcross(v, vj);
        }
        SV dvp = sv0(), dap = sv0();
        V3 dgp = mk(0, 0, 0);
        if (d > 0) {
          if (!chain) {   // the parent is not the body visited just before: its tangents are in its slot
            tdv = ld_ft(pslot, 0), tda = ld_ft(pslot, 6);
            tdg = mk(FT(pslot, 12), FT(pslot, 13), FT(pslot, 14));
          }
          dvp = act_inv(R, p, tdv);
          dap = act_inv(R, p, tda);
          dgp = mulT(R, tdg);
        }
        if (impact) dgp = mk(0, 0, 0);
        SV dv = dvp, da = dap;
        V3 dg = dgp;
        const bool vdir = (kind == 1 || (impact && !dyn && kind == 2)) && !(impact && dyn);   // the lane's direction moves v
        if (ff) {
          if (own) {
            const SV S = unit_twist(i, j - iv);
            if (kind == 0) {
              dv = dv - mcross(S, vpar);
              da = da - mcross(S, apar);
              dg = dg - cross(S.a, gi);
            } else if (kind == 1) {
              if (!(impact && dyn)) dv = dv + S;
            } else {
              if (!(impact && !dyn)) da = da + S;
              if (impact && !dyn) dv = dv + S;  // d(v + dv)/d(dv)
            }
          }
          da = da + mcross(dv, vj);
          if (own && vdir) da = da + mcross(v, unit_twist(i, j - iv));
        } else {
          // revolute joint: S = (0, axis), so S x m = (axis x m.l, axis x m.a) and m x S = (m.l x axis, m.a x axis)
          const V3 ax = ldv3(&JM(i, J_AXIS));
          if (own) {
            if (kind == 0) {
              dv = dv - SV{cross(ax, vpar.l), cross(ax, vpar.a)};
              da = da - SV{cross(ax, apar.l), cross(ax, apar.a)};
              dg = dg - cross(ax, gi);
            } else if (kind == 1) {
              if (!(impact && dyn)) dv.a = dv.a + ax;
            } else {
              if (!(impact && !dyn)) da.a = da.a + ax;
              if (impact && !dyn) dv.a = dv.a + ax;  // d(v + dv)/d(dv)
            }
          }
          da = da + SV{cross(dv.l, vj.a), cross(dv.a, vj.a)};   // dv x vj with vj = (0, vq axis)
          if (own && vdir) da = da + SV{cross(v.l, ax), cross(v.a, ax)};
        }
        // own force and its tangent
        const double mass = JM(i, J_MASS);
        const V3 com = ldv3(&JM(i, J_COM));
        const M3 I = ldm3(&JM(i, J_INERTIA));
        const SV h = PRE ? ld_sv(d, V_H) : inertia_mul(mass, com, I, v);
        SV f = PRE ? sv0() : inertia_mul(mass, com, I, SV{acc.l + gi, acc.a}) + fcross(v, h);   // PRE: the block holds the total force
        const SV df = inertia_mul(mass, com, I, SV{da.l + dg, da.a}) + fcross(dv, h) + fcross(v, inertia_mul(mass, com, I, dv));
        // contacts carried by this body; roff = rows of the active contacts before c (3 per point, 6 per surface contact)
        int roff = 0;
        for (int c = 0; c < ncon; ++c) {
          const bool on = (active >> c) & 1u;
          const bool surf = SURF && (int)scm[c * CP + C_TYPE] == RTOC_CONTACT_SURFACE;
          const int nr = surf ? 6 : 3;
          if (on && (int)scm[c * CP + C_PARENT] == i) {
            const M3 Rf = ldm3(&scm[c * CP + C_R]);
            const V3 pf = ldv3(&scm[c * CP + C_P]);
            // the contact force / wrench is given in the LOCAL contact frame (point_contact.cpp:55-60, surface_contact.cpp)
            const SV fc = PRE ? sv0() : SV{mk(sf[roff], sf[roff + 1], sf[roff + 2]), surf ? mk(sf[roff + 3], sf[roff + 4], sf[roff + 5]) : mk(0, 0, 0)};
            if (!PRE) f = f - act_f(Rf, pf, fc);
            if (rows) {
              const SV vf = act_inv(Rf, pf, v), dvf = act_inv(Rf, pf, dv);
              SV C, dC;  // angular parts only used by surface contacts
              if (impact) {
                C = vf;
                dC = dvf;
              } else {
                const SV af = act_inv(Rf, pf, acc), daf = act_inv(Rf, pf, da);
                const double kp = scm[c * CP + C_KP], kd = scm[c * CP + C_KD];
                const M3 oRf = mul(oR, Rf);
                const V3 pw = op + mul(oR, pf);
                const V3 pr = a.rv.positions ? ldv3(a.rv.positions + a.rv.placement(b, st, ncon, c) * 3) : mk(0, 0, 0);
                // the frame Jacobian column of dof j is the v-tangent of vf, one lane up (kind 0 lanes only use it)
                const SV jc = SV{mk(__shfl_down(dvf.l.x, 1, 64), __shfl_down(dvf.l.y, 1, 64), __shfl_down(dvf.l.z, 1, 64)),
                                 mk(__shfl_down(dvf.a.x, 1, 64), __shfl_down(dvf.a.y, 1, 64), __shfl_down(dvf.a.z, 1, 64))};
                if (!surf) {
                  // classical linear acceleration + kd v + kp (p - p_desired)   (point_contact.hxx:14-31, :33-83)
                  C.l = af.l + cross(vf.a, vf.l) + kd * vf.l + kp * (pw - pr);
                  dC.l = daf.l + cross(dvf.a, vf.l) + cross(vf.a, dvf.l) + kd * dvf.l;
                  if (kind == 0) dC.l = dC.l + kp * mul(oRf, jc.l);
                  C.a = mk(0, 0, 0), dC.a = mk(0, 0, 0);
                } else {
                  // spatial acceleration + kd v + kp Log6(X_desired^-1 X_frame)   (surface_contact.hxx:12-29, :31-68)
                  M3 Rd;
                  if (a.rv.rotations) {
                    Rd = ldm3(a.rv.rotations + a.rv.placement(b, st, ncon, c) * 9);
                  } else {
#pragma unroll
                    for (int e = 0; e < 9; ++e) Rd.m[e] = (e % 4 == 0) ? 1.0 : 0.0;
                  }
                  const M3 Rdt = transpose(Rd);
                  SV lg, dlg;
                  log6_fwd(mul(Rdt, oRf), mul(Rdt, pw - pr), jc, lg, dlg);
                  C = SV{af.l + kd * vf.l + kp * lg.l, af.a + kd * vf.a + kp * lg.a};
                  dC = SV{daf.l + kd * dvf.l, daf.a + kd * dvf.a};
                  if (kind == 0) dC = SV{dC.l + kp * dlg.l, dC.a + kp * dlg.a};
                }
              }
              const double Cv[6] = {C.l.x, C.l.y, C.l.z, C.a.x, C.a.y, C.a.z}, dCv[6] = {dC.l.x, dC.l.y, dC.l.z, dC.a.x, dC.a.y, dC.a.z};
              const int r0 = nv + roff;
              if (aug) {
                // lf -= dC/da beta (contact_dynamics.cpp:38; impact: dC/dv, impact_dynamics.cpp:21): sum over the a-lanes
                const bool al = lane_on && kind == 2;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                  if (t < nr) {
                    wsum += dCv[t] * smu[roff + t];
                    double rx = al ? dCv[t] * sbeta[j] : 0.0;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) rx += __shfl_xor(rx, off, 64);
                    if (lane == 0) slf[roff + t] += rx;
                  }
                }
              }
#pragma unroll
              for (int t = 0; t < 6; ++t) {
                if (t < nr) {
                  if (!PRE && lane == 0 && j0 == 0) cr[a.rv.cdd_off(RTOC_CDD_IDC) + r0 + t] = Cv[t];   // PRE: rbd_values_kernel wrote the values
                  if (lane_on) {
                    // impact: dC/dv = dC/d(dv) goes where the condensation reads it (the v block of DIDCDQV) and into DCDA
                    if (kind == 2 || (impact && kind == 1)) cr[a.rv.cdd_off(RTOC_CDD_DCDA) + (size_t)j * a.rv.L.dims.nf_max + (r0 - nv) + t] = dCv[t];
                    if (kind != 2) cr[a.rv.cdd_off(RTOC_CDD_DIDCDQV) + (size_t)(kind == 1 ? nv + j : j) * a.rv.L.nvf_max + r0 + t] = dCv[t];
                  }
                }
              }
            }
          }
          roff += on ? nr : 0;
        }
        // ---- store the level ----
        if constexpr (!PRE) {
#pragma unroll
          for (int k = 0; k < 9; ++k) LV(d, V_R + k) = R.m[k], LV(d, V_OR + k) = oR.m[k];
          stv3(&LV(d, V_P), p), stv3(&LV(d, V_OP), op);
          st_sv(d, V_V, v);
          st_sv(d, V_A, acc);
          stv3(&LV(d, V_G), gi);
          st_sv(d, V_F, f);
          LV(d, V_BODY) = (double)i;
        }
        tdv = dv, tda = da, tdg = dg;
        if (sslot >= 0) {
          st_ft(sslot, 0, dv);
          st_ft(sslot, 6, da);
          FT(sslot, 12) = dg.x, FT(sslot, 13) = dg.y, FT(sslot, 14) = dg.z;
        }
        if (leaf) cdf = df;
        else st_dt(d, df);
        top = d;
        topreg = leaf;
      }
      while (top >= 0) {
        close(top, topreg);
        topreg = false;
        --top;
      }
      if (aug && lane_on) {
        // lq / lv / la (ldv) += (this lane's column)^T [beta; mu]  (contact_dynamics.cpp:35-37,49-51; impact_dynamics.cpp:19-25)
        double* const kr = a.rv.kkt_at(rec);
        double* const dst = kind == 0 ? kr + a.rv.kkt_off(RTOC_KKT_LX) + j : kind == 1 ? kr + a.rv.kkt_off(RTOC_KKT_LX) + nv + j : a.unconstr ? kr + a.rv.kkt_off(RTOC_KKT_LU) + j : cr + a.rv.cdd_off(RTOC_CDD_LA) + j;
        if (!(impact && dyn && kind == 1)) *dst += a.scale * wsum;
      }
    }
  }
  if (aug) {
    __syncthreads();
    double* const kr = a.rv.kkt_at(rec);
    if (lane < g.dimf) cr[a.rv.cdd_off(RTOC_CDD_LF) + lane] -= slf[lane];
    if (a.unconstr) {
      if (lane < nv) cr[a.rv.cdd_off(RTOC_CDD_LA) + lane] -= a.scale * sbeta[lane];                         // lu -= dt beta (:63)
    } else if (!impact && lane < nu) kr[a.rv.kkt_off(RTOC_KKT_LU) + lane] -= sbeta[nv - nu + lane];           // lu -= beta (actuated part)
    if (nu < nv && lane < nv - nu) cr[a.rv.cdd_off(RTOC_CDD_LUP) + lane] = impact ? 0.0 : sr[a.rv.sol_off(RTOC_SOL_NUP) + lane] - sbeta[lane];  // lu_passive
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// UnconstrIntermediateStage / UnconstrTerminalStage::evalKKT up to the dynamics (reference src/unconstr/
// unconstr_intermediate_stage.cpp:64-78, unconstr_terminal_stage.cpp): kkt_matrix / kkt_residual.setZero(), the
// ConfigurationSpaceCost of a fixed-base robot (src/cost/configuration_space_cost.cpp:274-324 stage, :343-378 terminal:
// diagonal weights, q - q_ref Euclidean) and linearizeUnconstrForwardEuler (src/dynamics/unconstr_state_equation.cpp:8-24,
// 56-62).  rtoc_linearize in unconstrained mode then adds the dynamics terms.  Records in the convention of
// rtoc_unconstr_condense: KKT.Quu := Qaa, KKT.lu := la, CDD.Qaa := diag(Quu), CDD.la := lu.
// cost: [q_ref | v_ref | u_ref | wq | wv | wa | wu | wq_terminal | wv_terminal | impact weights x 3], nv + 1 doubles each
// (the table of contact_eval_kkt.hpp).
struct UkArgs {
  RecView rv;         // dx0: [batch][2 nv] computeInitialStateDirection: x0 - s[0].x
  const double* cost;
  const double* x0;   // [batch][2 nv] initial state of the horizon (q, v of updateSolution(t, q, v)); may be nullptr
  double dt;
  double* cost_out;   // [batch][nstages] value of the stage / terminal cost (the line search's evalOCP reads it), or nullptr
  QRefTable qtab;     // q_ref and isActive per grid point (ConfigurationSpaceRefBase), or q == nullptr: the constant q_ref
};

static __global__ __launch_bounds__(64) void unconstr_eval_kkt_kernel(UkArgs a) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / a.rv.nstages, st = blockIdx.x % a.rv.nstages;
  if (b >= a.rv.batch) return;
  const int nv = a.rv.nv(), nx = 2 * nv;
  const bool terminal = st == a.rv.nstages - 1;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  const double* const sn = s + a.rv.L.sol.stride;  // next grid point (not read on the terminal one)
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  const int M = nv + 1;
  const double *vr = a.cost + M, *ur = vr + M, *wq = ur + M, *wv = wq + M, *wa = wv + M, *wu = wa + M, *wqf = wu + M, *wvf = wqf + M;
  // the q_ref of this (instance, grid point): its row of the table if there is one.  An inactive row is not read: the q terms are
  // absent there (enable_q_cost && isCostConfigActive), i.e. they are the terms of a zero weight on the constant q_ref
  bool qon = true;
  const double* qr = a.cost;
  if (a.qtab.q) {
    const size_t row = a.qtab.row(b, a.rv.nstages, st);
    qon = a.qtab.active[row] != 0;
    if (qon) qr = a.qtab.q + row * a.qtab.nq;
  }
  const double dt = a.dt;
  // Hessian blocks: zero, then the diagonals (Qqq, Qvv; Qaa in the Quu slot)
  for (int e = lane; e < nx * nx; e += 64) {
    const int r = e % nx, c = e / nx;
    double v = 0.0;
    if (r == c) v = terminal ? (r < nv ? wqf[r] : wvf[r - nv]) : dt * (r < nv ? wq[r] : wv[r - nv]);
    if (!qon && r < nv) v = 0.0;
    kr[a.rv.kkt_off(RTOC_KKT_QXX) + e] = v;
  }
  for (int e = lane; e < nx * nv; e += 64) kr[a.rv.kkt_off(RTOC_KKT_QXU) + e] = 0.0;
  for (int e = lane; e < nv * nv; e += 64) kr[a.rv.kkt_off(RTOC_KKT_QUU) + e] = (!terminal && e % nv == e / nv) ? dt * wa[e % nv] : 0.0;
  for (int e = lane; e < nv * nv; e += 64) cr[a.rv.cdd_off(RTOC_CDD_MJTJINV) + e] = 0.0;  // off-diagonal part of Quu: a diagonal cost
  for (int i = lane; i < nv; i += 64) {
    const double q = s[a.rv.sol_off(RTOC_SOL_Q) + i], v = s[a.rv.sol_off(RTOC_SOL_V) + i], lmd = s[a.rv.sol_off(RTOC_SOL_LMD) + i], gmm = s[a.rv.sol_off(RTOC_SOL_GMM) + i];
    if (terminal) {
      kr[a.rv.kkt_off(RTOC_KKT_LX) + i] = (qon ? wqf[i] : 0.0) * (q - qr[i]) - lmd;   // evalTerminalCostDerivatives + ...ForwardEulerTerminal
      kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + i] = wvf[i] * (v - vr[i]) - gmm;
      kr[a.rv.kkt_off(RTOC_KKT_FX) + i] = 0.0, kr[a.rv.kkt_off(RTOC_KKT_FX) + nv + i] = 0.0;
      kr[a.rv.kkt_off(RTOC_KKT_LU) + i] = 0.0;
      cr[a.rv.cdd_off(RTOC_CDD_QAA) + i] = 0.0, cr[a.rv.cdd_off(RTOC_CDD_LA) + i] = 0.0;
    } else {
      const double acc = s[a.rv.sol_off(RTOC_SOL_A) + i], u = s[a.rv.sol_off(RTOC_SOL_U) + i];
      const double qn = sn[a.rv.sol_off(RTOC_SOL_Q) + i], vn = sn[a.rv.sol_off(RTOC_SOL_V) + i], lmdn = sn[a.rv.sol_off(RTOC_SOL_LMD) + i], gmmn = sn[a.rv.sol_off(RTOC_SOL_GMM) + i];
      kr[a.rv.kkt_off(RTOC_KKT_FX) + i] = q + dt * v - qn;                                            // Fq (:60)
      kr[a.rv.kkt_off(RTOC_KKT_FX) + nv + i] = v + dt * acc - vn;                                     // Fv (:61)
      kr[a.rv.kkt_off(RTOC_KKT_LX) + i] = dt * (qon ? wq[i] : 0.0) * (q - qr[i]) + (lmdn - lmd);      // lq
      kr[a.rv.kkt_off(RTOC_KKT_LX) + nv + i] = dt * wv[i] * (v - vr[i]) + (dt * lmdn + gmmn - gmm);   // lv
      kr[a.rv.kkt_off(RTOC_KKT_LU) + i] = dt * wa[i] * acc + dt * gmmn;                               // la (in the lu slot)
      cr[a.rv.cdd_off(RTOC_CDD_LA) + i] = dt * wu[i] * (u - ur[i]);                                   // lu (in CDD.la)
      cr[a.rv.cdd_off(RTOC_CDD_QAA) + i] = dt * wu[i];                                                // diag(Quu)
    }
  }
  if (a.cost_out) {
    // ConfigurationSpaceCost::evalStageCost / evalTerminalCost (configuration_space_cost.cpp:251-271, :323-338): the VALUE
    double l = 0.0;
    for (int i = lane; i < nv; i += 64) {
      const double dq = s[a.rv.sol_off(RTOC_SOL_Q) + i] - qr[i], dv = s[a.rv.sol_off(RTOC_SOL_V) + i] - vr[i];
      if (terminal) {
        l += (qon ? wqf[i] : 0.0) * dq * dq + wvf[i] * dv * dv;
      } else {
        const double acc = s[a.rv.sol_off(RTOC_SOL_A) + i], du = s[a.rv.sol_off(RTOC_SOL_U) + i] - ur[i];
        l += (qon ? wq[i] : 0.0) * dq * dq + wv[i] * dv * dv + wa[i] * acc * acc + wu[i] * du * du;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off, 64);
    if (lane == 0) a.cost_out[rec] = (terminal ? 0.5 : 0.5 * dt) * l;
  }
  if (st == 0 && a.x0 && a.rv.dx0) {
    for (int i = lane; i < nv; i += 64) {
      a.rv.dx0[(size_t)b * nx + i] = a.x0[(size_t)b * nx + i] - s[a.rv.sol_off(RTOC_SOL_Q) + i];
      a.rv.dx0[(size_t)b * nx + nv + i] = a.x0[(size_t)b * nx + nv + i] - s[a.rv.sol_off(RTOC_SOL_V) + i];
    }
  }
}

}  // namespace rbd
}  // namespace rtoc
