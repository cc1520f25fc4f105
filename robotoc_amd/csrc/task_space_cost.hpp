// task_space_cost.hpp -- TaskSpace3DCost and CoMCost of {Intermediate,Impact,Terminal}Stage::evalKKT on the device.
//
// quadratizeStageCost / ImpactCost / TerminalCost of the two components (reference src/cost/task_space_3d_cost.cpp,
// src/cost/com_cost.cpp) with their references PeriodicSwingFootRef / PeriodicCoMRef (src/cost/periodic_swing_foot_ref.cpp,
// periodic_com_ref.cpp) or a constant one, per (instance, grid point), ADDED to what contact_cost_kernel stored:
//   diff = x(q) - x_ref(t)      lq += s J^T W diff      Qqq += s J^T W J      cost += s/2 sum W diff^2
// s = dt on intermediate / lift grids (weight), 1 on impact (weight_impact) and terminal (weight_terminal) grids; on intermediate
// / lift grids also the STO sensitivities hx += J^T W diff, h += 1/2 sum W diff^2 (intermediate_stage.cpp:103-108).
//
// Kinematics from q with the joint table of the rigid-body kernels (rbd::DevModel): every lane places its joint in its parent's
// frame (one sincos per revolute joint), then the tree is composed level by level.  Jacobians: lane j holds column j, the
// world-aligned linear velocity of the point for a unit rate of dof j, q perturbed as the contact rows perturb it (a free-flyer's
// translation and rotation local):  base linear dof k: R_0 e_k;  rotation about world axis w = R_b axis through the origin p_b of
// the dof's body b:  w x (x - p_b), if the frame hangs in the subtree of b (depth-first order: [b, end_b)).  CoM: the same
// column over the subtree's mass, (w x (S_b - m_b p_b)) / M with S_b = sum m_k c_k over the subtree.
// Layout: GP grid points per wave (two for nv <= 32), 64 / GP lanes each; the Jacobians of the active terms go to LDS and
// the Qqq read-modify-write gives neighbouring lanes the row pairs of a column (16-byte accesses, an odd nv ends on one double).
// Grid points where no term is active are not written.  No atomics: every record is owned by one lane group.
//
// TaskSpace6DCost (reference src/cost/task_space_6d_cost.cpp, include/robotoc/cost/task_space_6d_cost.hpp:184-214):
//   X = X_ref^-1 oMf   d = log6(X)  [linear; angular]   JJ = Jlog6(X) J_frame (LOCAL frame Jacobian)
//   lq += s JJ^T W d   Qqq += s JJ^T W JJ   cost += s/2 sum W d^2
// lane j holds column j of J_frame, the frame's spatial velocity for a unit rate of dof j in the frame's own axes: a rotation
// about w through p_b gives (R_f^T (w x (x - p_b)), R_f^T w), base linear dof k gives (R_f^T R_0 e_k, 0), zero outside the subtree;
// JJ(:, j) is the `der` of rbd::log6_fwd along that column, d its `val`.  Six rows of LDS per 6D term.
// The extended instantiation (EXT) carries what a context with only 3D / CoM terms and formula references never needs: the 6D
// arithmetic, references read from a per-grid-point table (RTOC_REF_TABLE), and the unconstrained path's scaling (dt from the
// call, no impact kind, hx / h untouched).  The host picks it; EXT = false is the kernel as it was.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"

namespace rtoc {

struct TaskCostArgs {
  RecView rv;
  double* cost_out;              // [batch][nstages] (evalOCP's stage costs), added to
  const rtoc_task_cost* terms;   // [nterms] or [batch][nterms]
  const double* t_fixed;         // [nstages] (fixed grids) or nullptr
  const double* t_inst;          // [batch][nstages] (switching-time optimisation) or nullptr
  int nterms, per_instance;
  // EXT only
  const rtoc_task_ref_entry* tab[RTOC_MAX_TASK_COSTS];   // per term: [nstages] / [batch][nstages] entries of its table, or nullptr
  unsigned tab_inst;             // bit k: table k is per instance
  int nrows;                     // Jacobian rows in LDS per lane group: the largest sum over a term list (3 per 3D / CoM, 6 per 6D term)
  double unconstr_dt;            // > 0: rtoc_unconstr_eval_kkt's dt; 0: the contact path
};

namespace tsc {

// PeriodicSwingFootRef::isActive / PeriodicCoMRef::isActive (periodic_swing_foot_ref.cpp, periodic_com_ref.cpp): the reference's
// loop, comparison by comparison.  The trip cap only guards a non-finite t (the reference would not return); periods are > 0.
// No fused multiply-adds here: t0 + i * period + pa rounded as the reference's host code rounds it decides boundary points.
__device__ inline bool periodic_active(double t, double t0, double pa, double period) {
#pragma clang fp contract(off)
  for (int i = 0; i < (1 << 20); ++i) {
    if (t < t0 + i * period) return false;
    if (t < t0 + i * period + pa) return true;
  }
  return false;
}

// updateRef of the two periodic references, restated literally
__device__ inline void periodic_ref(const rtoc_task_cost& T, double t, double x[3]) {
#pragma clang fp contract(off)
  const double pa = T.period_active, period = T.period_active + T.period_inactive;
  if (T.ref_kind == RTOC_REF_PERIODIC_FOOT) {
    double rate, adv;
    if (t < T.t0 + pa) {
      rate = (t - T.t0) / pa;
      for (int k = 0; k < 3; ++k) x[k] = T.x0[k] + (T.first_half ? 0.5 * rate : rate) * T.rate[k];
    } else {
      int i = 1;
      for (; i < (1 << 20); ++i)
        if (t < T.t0 + i * period + pa) break;
      rate = (t - T.t0 - i * period) / pa;
      adv = T.first_half ? (i - 0.5 + rate) : (i + rate);
      for (int k = 0; k < 3; ++k) x[k] = T.x0[k] + adv * T.rate[k];
    }
    if (rate < 0.5) x[2] += 2 * rate * T.step_height;
    else x[2] += 2 * (1 - rate) * T.step_height;
  } else {
    double tau;
    if (t < T.t0 + pa) {
      tau = T.first_half ? 0.5 * (t - T.t0) : (t - T.t0);
    } else {
      int i = 1;
      for (; i < (1 << 20); ++i)
        if (t < T.t0 + i * period + pa) break;
      const double t1 = (t - T.t0 - i * period);
      tau = T.first_half ? ((i - 0.5) * pa + t1) : (i * pa + t1);
    }
    for (int k = 0; k < 3; ++k) x[k] = T.x0[k] + tau * T.rate[k];
  }
}

// the table entry of term k at grid point (b, st); the host launches only when every RTOC_REF_TABLE term has its table
__device__ inline const rtoc_task_ref_entry& table_entry(const TaskCostArgs& a, int k, int b, int st) {
  return a.tab[k][(((a.tab_inst >> k) & 1u) ? (size_t)b * a.rv.nstages : 0) + st];
}

}  // namespace tsc

// LDS per lane group: per joint R (9), p (3), m c (3) in world coordinates; per term J (3 or 6 rows x nv, row-major) of the active terms
__host__ __device__ inline size_t task_cost_lds_doubles(int njoints, int nrows, int nv) { return (size_t)njoints * 15 + (size_t)nrows * nv; }
__host__ __device__ inline int task_cost_rows(int kind) { return kind == RTOC_TASK_FRAME_6D ? 6 : 3; }

template <int GP, bool EXT>
static __global__ __launch_bounds__(64) void task_space_cost_kernel(TaskCostArgs a) {
  constexpr int LW = 64 / GP;
  extern __shared__ double tc_lds[];
  const int lane = threadIdx.x % LW, grp = threadIdx.x / LW;
  const rbd::DevModel& md = *a.rv.model;
  const int nj = md.m.njoints, nv = a.rv.nv(), nx = 2 * nv, nt = a.nterms;
  double* const W = tc_lds + (size_t)grp * task_cost_lds_doubles(nj, EXT ? a.nrows : 3 * nt, nv);
  double* const Rw = W;             // [nj][9]
  double* const pw = W + 9 * nj;    // [nj][3]
  double* const mc = W + 12 * nj;   // [nj][3]: mass x world centre of mass
  double* const Jl = W + 15 * nj;   // [nt][3][nv]; EXT: [rows of term 0 .. nt - 1][nv]
  const long long nitems = (long long)a.rv.batch * a.rv.nstages;
  long long item = (long long)blockIdx.x * GP + grp;
  const bool real = item < nitems;   // a trailing group without a grid point computes the last one and writes nothing
  item = real ? item : nitems - 1;
  const int b = (int)(item / a.rv.nstages), st = (int)(item % a.rv.nstages);
  const rtoc_grid g = a.rv.grid[st];
  const bool unc = EXT && a.unconstr_dt > 0.0;
  const bool impact = !unc && g.type == RTOC_GRID_IMPACT, terminal = st == a.rv.nstages - 1, sto = !terminal && !impact && !unc;
  const double s = (impact || terminal) ? 1.0 : (unc ? a.unconstr_dt : grid_dt(a.rv.grid, a.rv.dt_inst, b, a.rv.nstages, st));
  const double t = a.t_inst ? a.t_inst[(size_t)b * a.rv.nstages + st] : (a.t_fixed ? a.t_fixed[st] : 0.0);
  const rtoc_task_cost* const terms = a.terms + (a.per_instance ? (size_t)b * nt : 0);
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const double* const q = a.rv.sol_at(rec) + a.rv.sol_off(RTOC_SOL_Q);
  // ---- which terms are on at this grid point (uniform over the group) ----
  unsigned on = 0;
  for (int k = 0; k < nt; ++k) {
    const rtoc_task_cost& T = terms[k];
    const double* w = terminal ? T.weight_terminal : impact ? T.weight_impact : T.weight;
    bool enabled = w[0] != 0.0 || w[1] != 0.0 || w[2] != 0.0;
    const double period = T.period_active + T.period_inactive;   // period_ = period_swing + period_stance
    bool active;
    if constexpr (EXT) {
      if (T.kind == RTOC_TASK_FRAME_6D) {   // enable_cost_ = !weight_.isZero() over all six
        const double* wa = terminal ? T.weight_angular_terminal : impact ? T.weight_angular_impact : T.weight_angular;
        enabled = enabled || wa[0] != 0.0 || wa[1] != 0.0 || wa[2] != 0.0;
      }
      if (T.ref_kind == RTOC_REF_TABLE) active = tsc::table_entry(a, k, b, st).active != 0;
      else active = T.ref_kind == RTOC_REF_CONST || tsc::periodic_active(t, T.t0, T.period_active, period);
    } else {
      active = T.ref_kind == RTOC_REF_CONST || tsc::periodic_active(t, T.t0, T.period_active, period);
    }
    if (enabled && active) on |= 1u << k;
  }
  // ---- local placements (lane per joint), then the tree level by level ----
  for (int i = lane; i < nj; i += LW) {
    const double* J = md.joint[i];
    const int type = (int)J[rbd::J_TYPE], iq = (int)J[rbd::J_IDXQ];
    rbd::M3 Rj;
    double pj[3] = {0.0, 0.0, 0.0};
    if (type == RTOC_JOINT_FREE_FLYER) {
      Rj = rbd::quat_R(q + iq + 3);
      pj[0] = q[iq], pj[1] = q[iq + 1], pj[2] = q[iq + 2];
    } else {
      double sn, cs;
      sincos(q[iq], &sn, &cs);
      Rj = rbd::revolute_R(rbd::ldv3(J + rbd::J_AXIS), sn, cs);
    }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Rw[9 * i + 3 * r + c] = J[rbd::J_R + 3 * r] * Rj.m[c] + J[rbd::J_R + 3 * r + 1] * Rj.m[3 + c] + J[rbd::J_R + 3 * r + 2] * Rj.m[6 + c];
      pw[3 * i + r] = J[rbd::J_R + 3 * r] * pj[0] + J[rbd::J_R + 3 * r + 1] * pj[1] + J[rbd::J_R + 3 * r + 2] * pj[2] + J[rbd::J_P + r];
    }
  }
  __syncthreads();
  for (int lvl = 1; lvl < md.nlevels; ++lvl) {
    for (int i = lane; i < nj; i += LW) {
      const int par = md.m.parent[i];
      if (md.depth[i] != lvl || par < 0 || par == i) continue;
      const double *Rp = Rw + 9 * par, *pp = pw + 3 * par;
      double R[9], p[3];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = Rp[3 * r] * Rw[9 * i + c] + Rp[3 * r + 1] * Rw[9 * i + 3 + c] + Rp[3 * r + 2] * Rw[9 * i + 6 + c];
        p[r] = pp[r] + Rp[3 * r] * pw[3 * i] + Rp[3 * r + 1] * pw[3 * i + 1] + Rp[3 * r + 2] * pw[3 * i + 2];
      }
      for (int e = 0; e < 9; ++e) Rw[9 * i + e] = R[e];
      for (int r = 0; r < 3; ++r) pw[3 * i + r] = p[r];
    }
    __syncthreads();
  }
  for (int i = lane; i < nj; i += LW) {
    const double* J = md.joint[i];
    const double m = J[rbd::J_MASS];
    for (int r = 0; r < 3; ++r)
      mc[3 * i + r] = m * (Rw[9 * i + 3 * r] * J[rbd::J_COM] + Rw[9 * i + 3 * r + 1] * J[rbd::J_COM + 1] + Rw[9 * i + 3 * r + 2] * J[rbd::J_COM + 2] + pw[3 * i + r]);
  }
  __syncthreads();
  // ---- per dof j (lane): its body, the end of that body's subtree, its world axis ----
  double mtot = 0.0, S[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < nj; ++k) {
    mtot += md.joint[k][rbd::J_MASS];
    for (int r = 0; r < 3; ++r) S[r] += mc[3 * k + r];
  }
  double lq[2] = {0.0, 0.0}, cost = 0.0;   // lane j's J^T W diff (lq[0]: dof lane, lq[1]: dof lane + LW), 1/2 sum W diff^2
  int row0 = 0;                            // EXT: first LDS row of term k
  for (int k = 0; k < nt; row0 += EXT ? task_cost_rows(terms[k].kind) : 3, ++k) {
    if (!((on >> k) & 1u)) continue;
    const rtoc_task_cost& T = terms[k];
    const double* w = terminal ? T.weight_terminal : impact ? T.weight_impact : T.weight;
    const bool com = T.kind == RTOC_TASK_COM;
    if constexpr (EXT) {
      if (T.kind == RTOC_TASK_FRAME_6D) {
        const double* wa = terminal ? T.weight_angular_terminal : impact ? T.weight_angular_impact : T.weight_angular;
        const int f = T.frame_parent;
        const rbd::M3 Rp = rbd::ldm3(Rw + 9 * f), Rf = rbd::mul(Rp, rbd::ldm3(T.frame_R));   // oMf = parent joint placement (frame_R, frame_p)
        const rbd::V3 xf = rbd::mul(Rp, rbd::ldv3(T.frame_p)) + rbd::ldv3(pw + 3 * f);
        const bool tab = T.ref_kind == RTOC_REF_TABLE;
        const rbd::M3 Rr = rbd::ldm3(tab ? tsc::table_entry(a, k, b, st).R : T.ref_R);
        const rbd::V3 pr = rbd::ldv3(tab ? tsc::table_entry(a, k, b, st).p : T.x0);
        // X = X_ref^-1 oMf
        rbd::M3 XR;
        rbd::V3 Xp;
        rbd::rel(Rr, pr, Rf, xf, XR, Xp);
        // one inlined log6_fwd: the loop is kept rolled, and its first trip (every lane takes it, with a zero column where the
        // lane has no dof) also yields d
        rbd::SV wd = rbd::sv0();
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          const int j = lane + h * LW;
          if (h > 0 && j >= nv) break;
          rbd::SV col = rbd::sv0();
          if (j < nv) {
            const int bj = md.dof_body[j];
            const double* Jb = md.joint[bj];
            const bool lin = (int)Jb[rbd::J_TYPE] == RTOC_JOINT_FREE_FLYER && j - (int)Jb[rbd::J_IDXV] < 3;
            int end = bj + 1;
            while (end < nj && md.depth[end] > md.depth[bj]) ++end;
            if (f >= bj && f < end) {
              if (lin) {
                const int e = j - (int)Jb[rbd::J_IDXV];
                col.l = rbd::mulT(Rf, rbd::mk(Rw[9 * bj + e], Rw[9 * bj + 3 + e], Rw[9 * bj + 6 + e]));
              } else {
                const rbd::V3 wv = rbd::mul(rbd::ldm3(Rw + 9 * bj), rbd::ldv3(md.dof_axis[j]));
                col = rbd::SV{rbd::mulT(Rf, rbd::cross(wv, xf - rbd::ldv3(pw + 3 * bj))), rbd::mulT(Rf, wv)};
              }
            }
          }
          rbd::SV d, der;
          rbd::log6_fwd(XR, Xp, col, d, der);
          if (h == 0) {
            wd = rbd::SV{rbd::mk(w[0] * d.l.x, w[1] * d.l.y, w[2] * d.l.z), rbd::mk(wa[0] * d.a.x, wa[1] * d.a.y, wa[2] * d.a.z)};
            cost += 0.5 * (rbd::dot(wd.l, d.l) + rbd::dot(wd.a, d.a));
          }
          if (j >= nv) break;
          const double jj[6] = {der.l.x, der.l.y, der.l.z, der.a.x, der.a.y, der.a.z};
          for (int r = 0; r < 6; ++r) Jl[(row0 + r) * nv + j] = jj[r];
          const double g = rbd::dot(der.l, wd.l) + rbd::dot(der.a, wd.a);
          if (h == 0) lq[0] += g;   // (no indexing of lq by the rolled loop's counter: it lives in registers)
          else lq[1] += g;
        }
        continue;
      }
    }
    const int jrow = EXT ? row0 : 3 * k;
    double x[3], xr[3];
    if (com) {
      for (int r = 0; r < 3; ++r) x[r] = S[r] / mtot;
    } else {
      const int f = T.frame_parent;
      for (int r = 0; r < 3; ++r)
        x[r] = Rw[9 * f + 3 * r] * T.frame_p[0] + Rw[9 * f + 3 * r + 1] * T.frame_p[1] + Rw[9 * f + 3 * r + 2] * T.frame_p[2] + pw[3 * f + r];
    }
    if (T.ref_kind == RTOC_REF_CONST) {
      for (int r = 0; r < 3; ++r) xr[r] = T.x0[r];
    } else if (EXT && T.ref_kind == RTOC_REF_TABLE) {
      for (int r = 0; r < 3; ++r) xr[r] = tsc::table_entry(a, k, b, st).p[r];
    } else {
      tsc::periodic_ref(T, t, xr);
    }
    double wd[3];
    for (int r = 0; r < 3; ++r) wd[r] = w[r] * (x[r] - xr[r]);
    cost += 0.5 * (wd[0] * (x[0] - xr[0]) + wd[1] * (x[1] - xr[1]) + wd[2] * (x[2] - xr[2]));
    for (int h = 0; h < 2; ++h) {
      const int j = lane + h * LW;
      if (j >= nv) break;
      const int bj = md.dof_body[j];
      const double* Jb = md.joint[bj];
      const double* Rb = Rw + 9 * bj;
      const bool lin = (int)Jb[rbd::J_TYPE] == RTOC_JOINT_FREE_FLYER && j - (int)Jb[rbd::J_IDXV] < 3;
      int end = bj + 1;
      while (end < nj && md.depth[end] > md.depth[bj]) ++end;
      double col[3] = {0.0, 0.0, 0.0};
      if (lin) {
        const int e = j - (int)Jb[rbd::J_IDXV];
        double msub = 0.0;
        if (com)
          for (int kk = bj; kk < end; ++kk) msub += md.joint[kk][rbd::J_MASS];
        const double f = com ? msub / mtot : 1.0;
        for (int r = 0; r < 3; ++r) col[r] = f * Rb[3 * r + e];
      } else {
        const double* ax = md.dof_axis[j];
        double wv[3], d[3];
        for (int r = 0; r < 3; ++r) wv[r] = Rb[3 * r] * ax[0] + Rb[3 * r + 1] * ax[1] + Rb[3 * r + 2] * ax[2];
        if (com) {
          double msub = 0.0, Ss[3] = {0.0, 0.0, 0.0};
          for (int kk = bj; kk < end; ++kk) {
            msub += md.joint[kk][rbd::J_MASS];
            for (int r = 0; r < 3; ++r) Ss[r] += mc[3 * kk + r];
          }
          for (int r = 0; r < 3; ++r) d[r] = (Ss[r] - msub * pw[3 * bj + r]) / mtot;
        } else {
          const bool moves = T.frame_parent >= bj && T.frame_parent < end;
          for (int r = 0; r < 3; ++r) d[r] = moves ? x[r] - pw[3 * bj + r] : 0.0;
        }
        col[0] = wv[1] * d[2] - wv[2] * d[1], col[1] = wv[2] * d[0] - wv[0] * d[2], col[2] = wv[0] * d[1] - wv[1] * d[0];
      }
      if (!com && lin && !(T.frame_parent >= bj && T.frame_parent < end)) col[0] = col[1] = col[2] = 0.0;
      for (int r = 0; r < 3; ++r) Jl[(jrow + r) * nv + j] = col[r];
      lq[h] += col[0] * wd[0] + col[1] * wd[1] + col[2] * wd[2];
    }
  }
  __syncthreads();
  if (!real || on == 0) return;   // nothing active: the record is left as contact_cost_kernel wrote it
  double* const kr = a.rv.kkt_at(rec);
  double* const Qxx = kr + a.rv.kkt_off(RTOC_KKT_QXX);
  for (int h = 0; h < 2; ++h) {
    const int j = lane + h * LW;
    if (j >= nv) break;
    kr[a.rv.kkt_off(RTOC_KKT_LX) + j] += s * lq[h];
    if (sto) kr[a.rv.kkt_off(RTOC_KKT_HX) + j] += lq[h];
  }
  if (lane == 0) {
    if (sto) kr[a.rv.kkt_off(RTOC_KKT_SCAL) + RTOC_KKT_SCAL_H] += cost;
    if (a.cost_out) a.cost_out[rec] += s * cost;
  }
  // ---- Qqq += s sum_k J_k^T W_k J_k: row pairs (r, r + 1) of column c to neighbouring lanes ----
  const int npair = (nv + 1) >> 1;
  for (int e = lane; e < nv * npair; e += LW) {
    const int c = e / npair, r = 2 * (e - c * npair);
    const bool two = r + 1 < nv;
    double v0 = 0.0, v1 = 0.0;
    int krow = 0;
    for (int k = 0; k < nt; krow += EXT ? task_cost_rows(terms[k].kind) : 3, ++k) {
      if (!((on >> k) & 1u)) continue;
      const double* w = terminal ? terms[k].weight_terminal : impact ? terms[k].weight_impact : terms[k].weight;
      for (int d = 0; d < 3; ++d) {
        const double* Jr = Jl + ((EXT ? krow : 3 * k) + d) * nv;
        const double wc = w[d] * Jr[c];
        v0 += Jr[r] * wc;
        if (two) v1 += Jr[r + 1] * wc;
      }
      if constexpr (EXT) {
        if (terms[k].kind == RTOC_TASK_FRAME_6D) {
          const double* wa = terminal ? terms[k].weight_angular_terminal : impact ? terms[k].weight_angular_impact : terms[k].weight_angular;
          for (int d = 0; d < 3; ++d) {
            const double* Jr = Jl + (krow + 3 + d) * nv;
            const double wc = wa[d] * Jr[c];
            v0 += Jr[r] * wc;
            if (two) v1 += Jr[r + 1] * wc;
          }
        }
      }
    }
    double* const p = Qxx + r + (size_t)c * nx;
    if (two) {
      double2* const p2 = reinterpret_cast<double2*>(p);
      double2 o = *p2;
      o.x += s * v0, o.y += s * v1;
      *p2 = o;
    } else {
      *p += s * v0;
    }
  }
}

}  // namespace rtoc
