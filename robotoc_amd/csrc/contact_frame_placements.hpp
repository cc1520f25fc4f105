// contact_frame_placements.hpp -- Robot::updateFrameKinematics + framePosition / frameRotation / CoM of every instance
// (include/robotoc/robot/robot.hxx: forward kinematics to the contact frames, pinocchio::centerOfMass), and the planners' "the feet
// on the ground stay where they are" (src/mpc/trot_foot_step_planner.cpp:94-98, :138-141) for a batch: the placements go straight
// into the per-instance table of desired contact placements (record_view.hpp: RecView::placement) and never leave the device.
//
// Mapping: the geometry of rbd_values_kernel (rigid_body.hpp) -- lanes = the bodies of one instance, one pass down the levels of
// the tree, 64 / gs instances per wave (gs: the next power of two >= njoints).  LDS: the world placement of every body (a child
// reads its parent's) and of every contact frame (the lanes of an instance then share the stores), FK_SLOTS doubles each.  The centre
// of mass is a butterfly over the gs lanes of an instance, in registers.  No atomics.
// Loads of q: the configurations lie a record (source 1) or a state (source 0) apart, so a wave touches 64 / gs separate runs
// of nq doubles.  Every body lane loads its own joint coordinate and nothing else -- the revolute lanes of an instance read one
// contiguous run, the root lane its seven -- so each double is fetched once and nothing is staged: no value is used by a second lane.
//
// Included by rt_placements.hip alone (a kernel header belongs to the unit that launches from it).
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"
#include "rigid_body_math.hpp"
#include "rigid_body_model.hpp"
#include "../../include/rtoc_robot.h"

namespace rtoc {

struct FkArgs {
  RecView rv;            // model, batch; hold form: placement() of the per-instance table (placement_stride = nstages)
  ModelDims md;
  const double* q;       // configuration of instance 0
  size_t q_stride;       // doubles between the configurations of two instances
  double* out_R;         // [batch][ncontacts][9] row-major, [batch][ncontacts][3], [batch][3]; each may be nullptr
  double* out_p;
  double* out_com;
  double* tab_pos;       // hold form: the per-instance tables [batch][nstages][ncontacts][3 | 9] (tab_rot may be nullptr), or nullptr
  double* tab_rot;
  int first, last;       // grid points [first, last) the hold form writes
  unsigned contacts;     // ... and the contacts, as a bit mask
};
// world placement of a body or a contact frame in LDS: rotation (row-major), position
enum : int { FK_R = 0, FK_P = 9, FK_SLOTS = 12 };
static_assert(FK_R == 0 && FK_P == FK_R + 9 && FK_SLOTS == FK_P + 3 && FK_SLOTS % 2 == 0, "placement slots");

static __global__ __launch_bounds__(64) void contact_frame_placements_kernel(FkArgs a) {
  using namespace rbd;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // [G][njoints + ncontacts][FK_SLOTS]
  const int lane = threadIdx.x, GS = a.md.gs, G = 64 / GS, nb = a.md.njoints, ncon = a.md.ncontacts;
  const int grp = lane / GS, i = lane % GS;
  const long long inst = (long long)blockIdx.x * G + grp;
  const bool gvalid = inst < a.rv.batch;
  const int b = gvalid ? (int)inst : 0;
  const bool on = gvalid && i < nb;
  const int ib = i < nb ? i : 0;
  double* const W = smem + (size_t)grp * (nb + ncon) * FK_SLOTS;   // bodies, then contact frames
  double* const me = W + (size_t)ib * FK_SLOTS;
  double* const F = W + (size_t)nb * FK_SLOTS;
  // ---- this body's constants and joint coordinate ----
  const double* const jm = &a.rv.model->joint[ib][0];
  const int type = (int)jm[J_TYPE], iq = (int)jm[J_IDXQ], depth = (int)jm[J_DEPTH];
  const int par = a.rv.model->m.parent[ib];
  const double* const q = a.q + (size_t)b * a.q_stride;
  M3 R;
  V3 p;
  joint_placement_at(jm, type == RTOC_JOINT_FREE_FLYER, q + iq, R, p);
  // ---- down the levels: world placements ----
  M3 oR = R;
  V3 op = p;
  for (int d = 0; d < a.md.nlevels; ++d) {
    if (on && depth == d) {
      if (d > 0) {
        const double* const pa = W + (size_t)par * FK_SLOTS;
        const M3 oRp = ldm3(pa + FK_R);
        oR = mul(oRp, R);
        op = ldv3(pa + FK_P) + mul(oRp, p);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) me[FK_R + k] = oR.m[k];
      stv3(me + FK_P, op);
    }
    __syncthreads();
  }
  // ---- centre of mass: sum of m_i (op_i + oR_i c_i) over the lanes of the instance / total mass ----
  {
    const double mass = on ? jm[J_MASS] : 0.0;
    const V3 cw = op + mul(oR, ldv3(jm + J_COM));
    double s[4] = {mass * cw.x, mass * cw.y, mass * cw.z, mass};
    for (int off = GS >> 1; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += __shfl_xor(s[k], off, 64);
    if (gvalid && a.out_com && i < 3) a.out_com[(size_t)b * 3 + i] = (i == 0 ? s[0] : (i == 1 ? s[1] : s[2])) / s[3];
  }
  // ---- the contact frames this body carries ----
  for (int c = 0; c < ncon; ++c) {
    const double* const cm = &a.rv.model->contact[c][0];
    if (on && (int)cm[C_PARENT] == ib) {
      const M3 oRf = mul(oR, ldm3(cm + C_R));
      const V3 pw = op + mul(oR, ldv3(cm + C_P));
      double* const f = F + (size_t)c * FK_SLOTS;
#pragma unroll
      for (int k = 0; k < 9; ++k) f[FK_R + k] = oRf.m[k];
      stv3(f + FK_P, pw);
    }
  }
  __syncthreads();
  if (!gvalid) return;
  // ---- out: the lanes of an instance share its entries, consecutive lanes consecutive doubles ----
  if (a.out_R)
    for (int e = i; e < ncon * 9; e += GS) a.out_R[(size_t)b * ncon * 9 + e] = F[(e / 9) * FK_SLOTS + FK_R + e % 9];
  if (a.out_p)
    for (int e = i; e < ncon * 3; e += GS) a.out_p[(size_t)b * ncon * 3 + e] = F[(e / 3) * FK_SLOTS + FK_P + e % 3];
  if (a.tab_pos) {
    const int n = (a.last - a.first) * ncon;
    for (int e = i; e < n * 3; e += GS) {
      const int st = a.first + (e / 3) / ncon, c = (e / 3) % ncon;
      if ((a.contacts >> c) & 1u) a.tab_pos[a.rv.placement(b, st, ncon, c) * 3 + e % 3] = F[c * FK_SLOTS + FK_P + e % 3];
    }
    if (a.tab_rot)
      for (int e = i; e < n * 9; e += GS) {
        const int st = a.first + (e / 9) / ncon, c = (e / 9) % ncon;
        const bool surf = (int)a.rv.model->contact[c][C_TYPE] == RTOC_CONTACT_SURFACE;
        if (surf && ((a.contacts >> c) & 1u)) a.tab_rot[a.rv.placement(b, st, ncon, c) * 9 + e % 9] = F[c * FK_SLOTS + FK_R + e % 9];
      }
  }
}

// A per-instance table from the one the batch shares: dst[b][0..per) = src[0..per), or without a source zeros (unit 3:
// positions) / identities (unit 9: rotations)
static __global__ __launch_bounds__(256) void placements_broadcast_kernel(double* dst, const double* src, size_t per, size_t total, int unit) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256)
    dst[e] = src ? src[e % per] : ((unit == 9 && (e % 9) % 4 == 0) ? 1.0 : 0.0);
}

}  // namespace rtoc
