// contact_constraints.hpp -- the friction-cone rows of the contact path evaluated on the device.
//
// FrictionCone / ImpactFrictionCone (reference src/constraints/friction_cone.cpp:100-191, impact_friction_cone.cpp) per
// ACTIVE contact of a grid point: the local contact force turned into the world frame, f_W = R_wf(q) f, the five rows
//     g = cone_local f_W,   cone_local = cone_world R_surface^T,   cone_world = [0 0 -1; +-1 0 -mu/sqrt2; 0 +-1 -mu/sqrt2]
// (frictionConeResidual, friction_cone.hpp:102-120) and their Jacobians
//     dg/df = cone_local R_wf                                           (:180-182)
//     dg/dq = cone_local (w_j x f_W),  w_j the angular Jacobian column of the contact frame -- in the LOCAL frame as the
//             reference takes it (getJacobianTransformFromLocalToWorld over getFrameJacobian(LOCAL), robot.hxx:247-287;
//             friction_cone.cpp:170-176), or world-aligned (the derivative of R_wf f): RTOC_OPT_CONE_JACOBIAN
//   INIT       setSlack + setSlackAndDualPositive: slack = -g clipped at sqrt(barrier), dual = barrier / slack  (:100-116, pdipm.hxx:12-23)
//   LINEARIZE  evalConstraint + evalDerivatives: residual = g + slack, cmpl = slack dual - barrier, the Jacobians into the
//              RTOC_BUF_CONE record (what rtoc_condense / rtoc_expand read), lq += dg/dq^T dual, lf += dg/df^T dual
// The rows' ConstraintComponentData live where rtoc_set_friction_cones puts them (RTOC_BUF_CON, compacted by active contact).
// One wave per (instance, grid point), lane j = dof j: the lane carries its column of the bodies' Jacobians down the tree.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"

namespace rtoc {

struct CcArgs {
  RecView rv;
  ModelDims md;
  const double* mu;         // [ncontacts]
  int mode;
  int contact_dim, row0, cone_stride, dgdf_off, impact_cones;
  int exact_jacobian;   // RTOC_OPT_CONE_JACOBIAN: 0 = w_local x f_W as the reference composes it, 1 = w_world x f_W
  double barrier;
};
enum { CC_INIT = 0, CC_LINEARIZE = 1 };

// LDS: the per-level carve (rbd::LevelCarve), then q
__host__ __device__ constexpr size_t cc_lds_bytes(int nlevels, int njoints, int ncontacts) {
  return sizeof(double) * (rbd::LevelCarve(nlevels, njoints, ncontacts).doubles() + (RTOC_MAX_JOINTS + 8));
}

static __global__ __launch_bounds__(64) void contact_cone_kernel(CcArgs a) {
  using namespace rbd::slots;
  using rbd::M3;
  using rbd::V3;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int nst1 = a.rv.nstages - 1;
  const int b = blockIdx.x / nst1, st = blockIdx.x % nst1;   // the terminal grid point has no rows
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  if (g.dimf == 0 || (g.type == RTOC_GRID_IMPACT && !a.impact_cones)) return;
  const unsigned act = a.rv.active[st];
  const int nv = a.rv.nv(), nb = a.md.njoints, ncon = a.md.ncontacts, nlev = a.md.nlevels, cd = a.contact_dim;
  const rbd::LevelCarve carve(nlev, nb, ncon);
  double* const lval = smem;
  double* const ltan = lval + carve.val;
  double* const sjm = ltan + carve.tan;
  double* const scm = sjm + carve.joint;
  double* const sq = scm + carve.contact;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  double* const lx = a.rv.kkt ? a.rv.kkt_at(rec) + a.rv.kkt_off(RTOC_KKT_LX) : nullptr;
  double* const cr = a.rv.cdd ? a.rv.cdd_at(rec) : nullptr;
  double* const nr = a.rv.con_at(rec);
  double* const gr = a.rv.cone ? a.rv.cone + rec * a.cone_stride : nullptr;
  const int* const no = a.rv.L.con.off;
  {
    const double* const gj = &a.rv.model->joint[0][0];
    const double* const gc = &a.rv.model->contact[0][0];
    for (int e = lane; e < nb * JP; e += 64) sjm[e] = gj[e];
    for (int e = lane; e < ncon * CP; e += 64) scm[e] = gc[e];
    for (int e = lane; e < a.rv.model->m.nq; e += 64) sq[e] = s[a.rv.sol_off(RTOC_SOL_Q) + e];
  }
  __syncthreads();
  const int j = lane;
  const bool lane_on = j < nv;
  const bool lin = a.mode == CC_LINEARIZE;
  auto LV = [&](int lev, int k) -> double& { return lval[lev * LVL_VAL + k]; };
  auto LT = [&](int lev, int k) -> double& { return ltan[((size_t)lev * LVL_TAN + k) * LVL_LANES + lane]; };   // 0: linear, 3: angular
  auto JM = [&](int i, int k) -> const double& { return sjm[i * JP + k]; };
  double lq = 0.0;
  for (int i = 0; i < nb; ++i) {
    const int d = (int)JM(i, J_DEPTH), iq = (int)JM(i, J_IDXQ), iv = (int)JM(i, J_IDXV);
    const bool ff = (int)JM(i, J_TYPE) == RTOC_JOINT_FREE_FLYER;
    const bool own = lane_on && j >= iv && j < iv + (ff ? 6 : 1);
    M3 R;
    V3 p;
    rbd::joint_placement_at(sjm + i * JP, ff, sq + iq, R, p);
    M3 oR = R;
    V3 wj = rbd::mk(0, 0, 0);   // body-frame angular velocity of body i per unit rate of dof j
    if (d > 0) {
      oR = rbd::mul(rbd::ldm3(&LV(d - 1, V_OR)), R);
      wj = rbd::mulT(R, rbd::mk(LT(d - 1, 3), LT(d - 1, 4), LT(d - 1, 5)));
    }
    if (own) wj = wj + (ff ? rbd::unit_twist(j - iv).a : rbd::ldv3(&JM(i, J_AXIS)));
#pragma unroll
    for (int k = 0; k < 9; ++k) LV(d, V_OR + k) = oR.m[k];
    LT(d, 3) = wj.x, LT(d, 4) = wj.y, LT(d, 5) = wj.z;
    int k = 0;  // index among the active contacts
    for (int c = 0; c < ncon; ++c) {
      const bool on = (act >> c) & 1u;
      if (on && (int)scm[c * CP + C_PARENT] == i) {
        const M3 Rwf = rbd::mul(oR, rbd::ldm3(&scm[c * CP + C_R]));
        const V3 fW = rbd::mul(Rwf, rbd::ldv3(s + a.rv.sol_off(RTOC_SOL_F) + k * cd));
        M3 Rs;
#pragma unroll
        for (int e = 0; e < 9; ++e) Rs.m[e] = a.rv.rotations ? a.rv.rotations[a.rv.placement(b, st, ncon, c) * 9 + e] : ((e % 4 == 0) ? 1.0 : 0.0);
        const double m = a.mu[c] * 0.70710678118654752440;
        // rows of cone_local = cone_world R_surface^T: row r = R_surface * (row r of cone_world)
        V3 row[5];
        row[0] = rbd::mul(Rs, rbd::mk(0, 0, -1));
        row[1] = rbd::mul(Rs, rbd::mk(1, 0, -m));
        row[2] = rbd::mul(Rs, rbd::mk(-1, 0, -m));
        row[3] = rbd::mul(Rs, rbd::mk(0, 1, -m));
        row[4] = rbd::mul(Rs, rbd::mk(0, -1, -m));
        const int r0 = a.row0 + 5 * k;
        if (lane < 5) {
          double gval = 0.0;   // row `lane` by selection (no run-time index into row[])
#pragma unroll
          for (int r = 0; r < 5; ++r)
            if (lane == r) gval = rbd::dot(row[r], fW);
          if (!lin) {
            double slack = -gval;
            const double sb = sqrt(a.barrier);
            if (slack < sb) slack = sb;
            nr[no[RTOC_CON_SLACK] + r0 + lane] = slack;
            nr[no[RTOC_CON_DUAL] + r0 + lane] = a.barrier / slack;
          } else {
            const double slack = nr[no[RTOC_CON_SLACK] + r0 + lane], dual = nr[no[RTOC_CON_DUAL] + r0 + lane];
            nr[no[RTOC_CON_RESIDUAL] + r0 + lane] = gval + slack;
            nr[no[RTOC_CON_CMPL] + r0 + lane] = slack * dual - a.barrier;
          }
        }
        if (lin) {
          double dual[5];
#pragma unroll
          for (int r = 0; r < 5; ++r) dual[r] = nr[no[RTOC_CON_DUAL] + r0 + r];
          if (lane < 3) {   // column `lane` of dg/df = cone_local R_wf, and lf
            const V3 col = rbd::mk(Rwf.m[lane], Rwf.m[3 + lane], Rwf.m[6 + lane]);
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 5; ++r) {
              const double e = rbd::dot(row[r], col);
              gr[a.dgdf_off + k * 15 + r + 5 * lane] = e;
              acc += e * dual[r];
            }
            cr[a.rv.cdd_off(RTOC_CDD_LF) + k * cd + lane] += acc;
          }
          if (lane_on) {    // column j of dg/dq
            // the reference crosses the LOCAL-frame angular Jacobian column with the WORLD-frame force (robot.hxx:247-253,
            // 275-287: getFrameJacobian(..., pinocchio::LOCAL, ...)); the derivative of R_wf f is w_world x f_W
            const V3 wxf = rbd::cross(a.exact_jacobian ? rbd::mul(oR, wj) : rbd::mulT(rbd::ldm3(&scm[c * CP + C_R]), wj), fW);
#pragma unroll
            for (int r = 0; r < 5; ++r) {
              const double e = rbd::dot(row[r], wxf);
              gr[k * 5 * nv + r + 5 * j] = e;
              lq += e * dual[r];
            }
          }
        }
      }
      k += on ? 1 : 0;
    }
  }
  if (lin && lane_on) lx[j] += lq;
}

}  // namespace rtoc

namespace rtoc {

// The same rows (LINEARIZE) from the kinematics the rigid-body pre-pass has already computed (rbd_values_kernel: the world
// rotation of every body, V_OR of its value block): no tree walk.  The world-aligned angular Jacobian column of a contact
// frame for dof j is oR_body(j) axis_j if the dof lies on the path from the root to the contact's body, else zero.
// One wave per (instance, grid point), lane j = dof j.
struct CvArgs {
  CcArgs c;
  const double* vals;   // [batch * nstages][njoints][VAL_DOUBLES]
};

static __global__ __launch_bounds__(64) void contact_cone_vals_kernel(CvArgs v) {
  using namespace rbd::slots;
  using rbd::M3;
  using rbd::V3;
  const CcArgs& a = v.c;
  const int lane = threadIdx.x;
  const int nst1 = a.rv.nstages - 1;
  const int b = blockIdx.x / nst1, st = blockIdx.x % nst1;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  if (g.dimf == 0 || (g.type == RTOC_GRID_IMPACT && !a.impact_cones)) return;
  const unsigned act = a.rv.active[st];
  const int nv = a.rv.nv(), nb = a.md.njoints, ncon = a.md.ncontacts, cd = a.contact_dim;
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  double* const kr = a.rv.kkt_at(rec);
  double* const cr = a.rv.cdd_at(rec);
  double* const nr = a.rv.con_at(rec);
  double* const gr = a.rv.cone + rec * a.cone_stride;
  const double* const vb = v.vals + rec * (size_t)nb * VAL_DOUBLES;
  const int* const no = a.rv.L.con.off;
  const int j = lane;
  const bool lane_on = j < nv;
  // this dof's rotation axis in the world frame
  V3 wj = rbd::mk(0, 0, 0);
  if (lane_on) {
    const double* const blk = vb + (size_t)a.rv.model->dof_body[j] * VAL_DOUBLES;
    wj = rbd::mul(rbd::ldm3(blk + V_OR), rbd::ldv3(a.rv.model->dof_axis[j]));
  }
  double lq = 0.0;
  int k = 0;
  for (int c = 0; c < ncon; ++c) {
    if (!((act >> c) & 1u)) continue;
    const double* const cm = &a.rv.model->contact[c][0];
    const double* const blk = vb + (size_t)(int)cm[C_PARENT] * VAL_DOUBLES;
    const M3 Rwf = rbd::mul(rbd::ldm3(blk + V_OR), rbd::ldm3(cm + C_R));
    const V3 fW = rbd::mul(Rwf, rbd::ldv3(s + a.rv.sol_off(RTOC_SOL_F) + k * cd));
    M3 Rs;
#pragma unroll
    for (int e = 0; e < 9; ++e) Rs.m[e] = a.rv.rotations ? a.rv.rotations[a.rv.placement(b, st, ncon, c) * 9 + e] : ((e % 4 == 0) ? 1.0 : 0.0);
    const double m = a.mu[c] * 0.70710678118654752440;
    V3 row[5];
    row[0] = rbd::mul(Rs, rbd::mk(0, 0, -1));
    row[1] = rbd::mul(Rs, rbd::mk(1, 0, -m));
    row[2] = rbd::mul(Rs, rbd::mk(-1, 0, -m));
    row[3] = rbd::mul(Rs, rbd::mk(0, 1, -m));
    row[4] = rbd::mul(Rs, rbd::mk(0, -1, -m));
    const int r0 = a.row0 + 5 * k;
    double dual[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) dual[r] = nr[no[RTOC_CON_DUAL] + r0 + r];
    if (lane < 5) {
      double gval = 0.0, dl = 0.0;   // row `lane` by selection: a run-time index would put row[] and dual[] into scratch
#pragma unroll
      for (int r = 0; r < 5; ++r)
        if (lane == r) gval = rbd::dot(row[r], fW), dl = dual[r];
      const double slack = nr[no[RTOC_CON_SLACK] + r0 + lane];
      nr[no[RTOC_CON_RESIDUAL] + r0 + lane] = gval + slack;
      nr[no[RTOC_CON_CMPL] + r0 + lane] = slack * dl - a.barrier;
    }
    if (lane < 3) {
      const V3 col = rbd::mk(Rwf.m[lane], Rwf.m[3 + lane], Rwf.m[6 + lane]);
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const double e = rbd::dot(row[r], col);
        gr[a.dgdf_off + k * 15 + r + 5 * lane] = e;
        acc += e * dual[r];
      }
      cr[a.rv.cdd_off(RTOC_CDD_LF) + k * cd + lane] += acc;
    }
    if (lane_on) {
      const bool path = (a.rv.model->contact_dofs[c] >> j) & 1ull;
      // reference: LOCAL-frame angular Jacobian column x WORLD-frame force (see contact_cone_kernel); exact: w_world x f_W
      const V3 wxf = path ? rbd::cross(a.exact_jacobian ? wj : rbd::mulT(Rwf, wj), fW) : rbd::mk(0, 0, 0);
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const double e = rbd::dot(row[r], wxf);
        gr[k * 5 * nv + r + 5 * j] = e;
        lq += e * dual[r];
      }
    }
    ++k;
  }
  if (lane_on) kr[a.rv.kkt_off(RTOC_KKT_LX) + j] += lq;
}

}  // namespace rtoc

namespace rtoc {

// ContactWrenchCone / ImpactWrenchCone (reference src/constraints/contact_wrench_cone.cpp:114-204): 17 rows per ACTIVE surface
// contact, g = cone f with the constant 17 x 6 cone matrix of the sole (computeCone / updateCone, :282-313; the host builds
// it with rtoc_wrench_cone_matrix and hands a table over) acting on the local 6-d contact wrench -- no kinematics:
//   INIT       cone matrix into the RTOC_BUF_CONE record (what rtoc_condense / rtoc_expand read), slack = -g clipped at
//              sqrt(barrier), dual = barrier / slack
//   LINEARIZE  residual = g + slack, cmpl = slack dual - barrier, lf += cone^T dual
// One wave per (instance, grid point), lane r < 17 = row r of a contact.
struct WcArgs {
  RecView rv;
  ModelDims md;
  const double* table;   // [ncontacts][17 x 6], column-major (ld 17)
  int mode, row0, cone_stride, impact_cones;
  double barrier;
};

static __global__ __launch_bounds__(64) void wrench_cone_eval_kernel(WcArgs a) {
  __shared__ double sd[RTOC_WRENCH_ROWS];
  const int lane = threadIdx.x;
  const int nst1 = a.rv.nstages - 1;
  const int b = blockIdx.x / nst1, st = blockIdx.x % nst1;
  if (b >= a.rv.batch) return;
  const rtoc_grid g = a.rv.grid[st];
  if (g.dimf == 0 || (g.type == RTOC_GRID_IMPACT && !a.impact_cones)) return;
  const unsigned act = a.rv.active[st];
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const s = a.rv.sol_at(rec);
  double* const cr = a.rv.cdd ? a.rv.cdd_at(rec) : nullptr;
  double* const nr = a.rv.con_at(rec);
  double* const gr = a.rv.cone + rec * a.cone_stride;
  const int* const no = a.rv.L.con.off;
  int k = 0;
  for (int c = 0; c < a.md.ncontacts; ++c) {
    if (!((act >> c) & 1u)) continue;
    const double* const A = a.table + (size_t)c * RTOC_WRENCH_ROWS * 6;
    const int r0 = a.row0 + RTOC_WRENCH_ROWS * k;
    if (a.mode == CC_INIT)
      for (int e = lane; e < RTOC_WRENCH_ROWS * 6; e += 64) gr[k * RTOC_WRENCH_ROWS * 6 + e] = A[e];
    if (lane < RTOC_WRENCH_ROWS) {
      double gval = 0.0;
#pragma unroll
      for (int t = 0; t < 6; ++t) gval += A[lane + RTOC_WRENCH_ROWS * t] * s[a.rv.sol_off(RTOC_SOL_F) + 6 * k + t];
      if (a.mode == CC_INIT) {
        double slack = -gval;
        const double sb = sqrt(a.barrier);
        if (slack < sb) slack = sb;
        nr[no[RTOC_CON_SLACK] + r0 + lane] = slack;
        nr[no[RTOC_CON_DUAL] + r0 + lane] = a.barrier / slack;
      } else {
        const double slack = nr[no[RTOC_CON_SLACK] + r0 + lane], dual = nr[no[RTOC_CON_DUAL] + r0 + lane];
        nr[no[RTOC_CON_RESIDUAL] + r0 + lane] = gval + slack;
        nr[no[RTOC_CON_CMPL] + r0 + lane] = slack * dual - a.barrier;
        sd[lane] = dual;
      }
    }
    if (a.mode == CC_LINEARIZE) {
      __syncthreads();
      if (lane < 6) {
        double acc = 0.0;
        for (int r = 0; r < RTOC_WRENCH_ROWS; ++r) acc += A[r + RTOC_WRENCH_ROWS * lane] * sd[r];
        cr[a.rv.cdd_off(RTOC_CDD_LF) + 6 * k + lane] += acc;
      }
      __syncthreads();
    }
    ++k;
  }
}

}  // namespace rtoc
