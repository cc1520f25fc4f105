// rigid_body_model.hpp -- the host half of the rigid-body kernels (rigid_body.hpp, task_space_cost.hpp, ...): the robot model as
// the device reads it (DevModel, packed by rtoc_set_robot_model), the plan of the tangent walk over it, and the LDS a launch
// of the linearisation needs.  Plain host code and constants, no kernel: the context holds a DevModel, so rt_context.hpp
// includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtoc_robot.h"

namespace rtoc {
namespace rbd {

// The three packed records of the rigid-body kernels.  This is the one place their layouts are written down: every reader and
// writer (pack_model below, rigid_body.hpp, contact_constraints.hpp, switching_constraint_lin.hpp, contact_frame_placements.hpp,
// task_space_cost.hpp and their launchers) goes through these names, and the asserts hold what that code relies on.
//
// Joint record, DevModel::joint[i][JP], and contact record, DevModel::contact[c][CP]: the per-joint / per-contact constants as
// the kernel reads them, packed by rtoc_set_robot_model: one coalesced copy into LDS per grid point instead of ~30 dependent L2
// round trips per visited body.  Rotations are 9 doubles row-major, vectors 3; the integers are stored as doubles.
// (An inline namespace: rbd::JP as before, and a kernel outside rbd takes the slot names alone with `using namespace rbd::slots`.)
inline namespace slots {
enum : int {
  J_R = 0,         // placement in the parent's frame: rotation
  J_P = 9,         //   and offset
  J_AXIS = 12,     // axis of a revolute joint
  J_MASS = 15,
  J_COM = 16,
  J_INERTIA = 19,  // rotational inertia at the joint's origin (9)
  J_TYPE = 28,     // RTOC_JOINT_*
  J_IDXQ = 29,
  J_IDXV = 30,
  J_DEPTH = 31,    // level of the body in the tree
  JP = 32,         // doubles per joint
};
enum : int {
  C_R = 0,         // placement of the contact frame in its body's frame: rotation
  C_P = 9,         //   and offset
  C_KP = 12,       // Baumgarte gains
  C_KD = 13,
  C_PARENT = 14,   // the body that carries the frame
  C_TYPE = 15,     // RTOC_CONTACT_*
  CP = 16,         // doubles per contact
};
// Value block of a body, VAL_DOUBLES doubles: what rbd_values_kernel writes per (grid point, body), what the tangent walk copies
// lane for lane into the value slots of a tree level (and, without the pre-pass, fills itself up to V_BODY), and what
// contact_cone_vals_kernel reads the world rotations from.
enum : int {
  V_R = 0,         // placement in the parent's frame
  V_P = 9,
  V_OR = 12,       // placement in the world frame
  V_OP = 21,
  V_V = 24,        // spatial velocity, acceleration (6 each: linear, angular)
  V_A = 30,
  V_G = 36,        // gravity in body coordinates
  V_F = 39,        // TOTAL force: own + children - contact forces (6)
  V_BODY = 45,     // index of the body
  V_VPAR = 46,     // the parent's velocity and acceleration in body coordinates
  V_APAR = 52,
  V_H = 58,        // h = I v
  VAL_DOUBLES = 64,
};
// what contact_cone_kernel and switching_constraint_lin_kernel keep per tree level (LevelCarve below): the head of a value block
// through V_OP, and a twist per lane
enum : int { LVL_VAL = 32, LVL_TAN = 6, LVL_LANES = 64 };
}  // namespace slots
// Every record is contiguous and ends at its size: a slot moved, grown or added has to be carried through here.
static_assert(J_R == 0 && J_P == J_R + 9 && J_AXIS == J_P + 3 && J_MASS == J_AXIS + 3 && J_COM == J_MASS + 1 && J_INERTIA == J_COM + 3 &&
                  J_TYPE == J_INERTIA + 9 && J_IDXQ == J_TYPE + 1 && J_IDXV == J_IDXQ + 1 && J_DEPTH == J_IDXV + 1 && JP == J_DEPTH + 1,
              "joint record");
static_assert(C_R == 0 && C_P == C_R + 9 && C_KP == C_P + 3 && C_KD == C_KP + 1 && C_PARENT == C_KD + 1 && C_TYPE == C_PARENT + 1 && CP == C_TYPE + 1,
              "contact record");
static_assert(V_R == 0 && V_P == V_R + 9 && V_OR == V_P + 3 && V_OP == V_OR + 9 && V_V == V_OP + 3 && V_A == V_V + 6 && V_G == V_A + 6 &&
                  V_F == V_G + 3 && V_BODY == V_F + 6 && V_VPAR == V_BODY + 1 && V_APAR == V_VPAR + 6 && V_H == V_APAR + 6 && VAL_DOUBLES == V_H + 6,
              "value block");
// the walk's level-slot copy is one double per lane of a wave
static_assert(VAL_DOUBLES == 64, "LV(d, lane) = pv covers a value block with 64 lanes");
// records follow one another in arrays and LDS carves that start 16-byte aligned, and the compiler pairs the doubles of an ldm3 /
// ldv3 / ldsv into 16-byte accesses where it can prove the address even: an even record size and even slots for what is read most
static_assert(JP % 2 == 0 && CP % 2 == 0 && VAL_DOUBLES % 2 == 0 && J_AXIS % 2 == 0 && V_OR % 2 == 0 && V_V % 2 == 0 && V_A % 2 == 0, "16-byte alignment");
struct DevModel {
  rtoc_robot_model m;
  int depth[RTOC_MAX_JOINTS];
  int nlevels;
  // storage plan of the tangent walk, per body: bit 0 = its parent is the body visited just before it (the parent's forward
  // tangents are still in registers), bit 1 = leaf (its force tangent is closed from registers), bits 4-7 = 1 + the LDS slot
  // its own forward tangents are kept in (bodies with two or more children; 0 = none), bits 8-11 = 1 + its parent's slot.
  // Slots are numbered by the count of branching ancestors: two bodies with the same count are never open at once.
  int walk[RTOC_MAX_JOINTS];
  int nbranch;
  // passes of the tangent walk: pass p carries the dofs [p dpp, (p + 1) dpp), three lanes each; pass_bodies[p] = the bodies
  // a direction of the pass can move or load (bit i: some dof of the pass sits on the path root -> i or in the subtree of i);
  // the other bodies are skipped by the whole wave (their columns are zero)
  int dpp, npass;
  unsigned long long pass_bodies[RTOC_MAX_JOINTS + 8];
  int pass_nvisit[RTOC_MAX_JOINTS + 8];                          // the same as lists, in depth-first order
  int pass_visit[RTOC_MAX_JOINTS + 8][RTOC_MAX_JOINTS];       // (ints: read through the scalar cache)
  double joint[RTOC_MAX_JOINTS][JP];
  double contact[RTOC_MAX_CONTACTS][CP];
  // per dof: the body it moves and its angular axis in that body's frame (zero for the linear dofs of a free-flyer);
  // per contact: the dofs on the path from the root to the contact's body (bit j): everything the world-aligned angular
  // Jacobian column of a contact frame needs besides the bodies' world rotations (contact_cone_vals_kernel)
  int dof_body[RTOC_MAX_JOINTS + 8];
  double dof_axis[RTOC_MAX_JOINTS + 8][3];
  unsigned long long contact_dofs[RTOC_MAX_CONTACTS];
};
// nbranch of a model (the number of LDS slots the walk needs for forward tangents): 1 + the largest count of branching
// ancestors of a branching body, 0 for a chain
inline int walk_plan(const rtoc_robot_model& m, int* walk) {
  int nchild[RTOC_MAX_JOINTS] = {}, slot[RTOC_MAX_JOINTS], nbranch = 0;
  for (int i = 1; i < m.njoints; ++i)
    if (m.parent[i] >= 0 && m.parent[i] < i) nchild[m.parent[i]]++;
  for (int i = 0; i < m.njoints; ++i) {
    const int par = (i > 0 && m.parent[i] >= 0 && m.parent[i] < i) ? m.parent[i] : -1;
    // slot[i]: the slot a branching body i would use = the number of branching bodies above it
    slot[i] = par < 0 ? 0 : slot[par] + (nchild[par] >= 2 ? 1 : 0);
    const int own = nchild[i] >= 2 ? slot[i] + 1 : 0;
    const int pslot = (par >= 0 && nchild[par] >= 2) ? slot[par] + 1 : 0;
    if (own > nbranch) nbranch = own;
    if (walk) walk[i] = ((par >= 0 && par == i - 1) ? 1 : 0) | (nchild[i] == 0 ? 2 : 0) | (own << 4) | (pslot << 8);
  }
  return nbranch;
}
inline void plan_passes(DevModel* h, int forced_dpp = 0);
inline void pack_model(DevModel* h) {
  const rtoc_robot_model& m = h->m;
  for (int i = 0; i < RTOC_MAX_JOINTS; ++i) h->walk[i] = 0;
  h->nbranch = walk_plan(m, h->walk);
  plan_passes(h);
  for (int i = 0; i < m.njoints; ++i) {
    double* o = h->joint[i];
    for (int k = 0; k < 9; ++k) o[J_R + k] = m.placement_R[i][k], o[J_INERTIA + k] = m.inertia[i][k];
    for (int k = 0; k < 3; ++k) o[J_P + k] = m.placement_p[i][k], o[J_AXIS + k] = m.axis[i][k], o[J_COM + k] = m.com[i][k];
    o[J_MASS] = m.mass[i];
    o[J_TYPE] = m.type[i], o[J_IDXQ] = m.idx_q[i], o[J_IDXV] = m.idx_v[i], o[J_DEPTH] = h->depth[i];
  }
  for (int j = 0; j < RTOC_MAX_JOINTS + 8; ++j) h->dof_body[j] = 0, h->dof_axis[j][0] = h->dof_axis[j][1] = h->dof_axis[j][2] = 0.0;
  for (int i = 0; i < m.njoints; ++i) {
    const int ndof = m.type[i] == RTOC_JOINT_FREE_FLYER ? 6 : 1;
    for (int k = 0; k < ndof; ++k) {
      const int j = m.idx_v[i] + k;
      if (j < 0 || j >= RTOC_MAX_JOINTS + 8) continue;
      h->dof_body[j] = i;
      if (ndof == 6) {
        if (k >= 3) h->dof_axis[j][k - 3] = 1.0;
      } else {
        for (int t = 0; t < 3; ++t) h->dof_axis[j][t] = m.axis[i][t];
      }
    }
  }
  for (int c = 0; c < m.ncontacts; ++c) {
    unsigned long long mask = 0;
    for (int i = m.contact_parent[c]; i >= 0 && i < m.njoints; i = m.parent[i]) {
      const int ndof = m.type[i] == RTOC_JOINT_FREE_FLYER ? 6 : 1;
      for (int k = 0; k < ndof; ++k)
        if (m.idx_v[i] + k >= 0 && m.idx_v[i] + k < 64) mask |= 1ull << (m.idx_v[i] + k);
      if (m.parent[i] == i) break;
    }
    h->contact_dofs[c] = mask;
  }
  for (int c = 0; c < m.ncontacts; ++c) {
    double* o = h->contact[c];
    for (int k = 0; k < 9; ++k) o[C_R + k] = m.contact_R[c][k];
    for (int k = 0; k < 3; ++k) o[C_P + k] = m.contact_p[c][k];
    o[C_KP] = m.contact_kp[c], o[C_KD] = m.contact_kd[c], o[C_PARENT] = m.contact_parent[c], o[C_TYPE] = m.contact_type[c];
  }
}

// per-level storage in LDS of the tangent walk: a value block (VAL_DOUBLES) and, per lane,
constexpr int TAN_SLOTS = 21;    // dv 6, da 6, dg 3, df 6
constexpr int FWD_SLOTS = 15;    // dv, da, dg: read by the children only, so the deepest level keeps none
constexpr int DF_SLOTS = 6;
__host__ __device__ constexpr int lin_pad8(int n) { return (n + 7) & ~7; }
// lanes per tangent slot: three per dof of a pass plus a column the idle lanes share, even (quadrupeds: 54 -> 56; 21 dofs: 64)
__host__ __device__ constexpr int lin_lane_stride(int dpp) { return (3 * dpp + 2) & ~1; }
constexpr int LIN_MAX_DPP = 21;
// What decides the speed of this kernel is how many grid points a CU holds at once (the walk is one long dependent
// instruction stream per wave, issue-bound): only what the walk cannot carry in registers lives in LDS -- the forward tangents
// (dv, da, dg) of the bodies with two or more children (nbranch slots: a body whose parent was visited just before it takes
// them from registers) and the force tangents df of the open non-leaf levels (a leaf is closed from registers).  ANYmal:
// 1 slot + 3 levels = 22 KB (was 4 + 4 levels = 38 KB), iCub: 2 slots + 10 levels (was 11 + 11 = 128 KB); DESIGN.md 3.4.
// pre: the walk reads the values of the recursion from rbd_values_kernel (PRE): no q, v, a, f, u staging, and of the joint
// constants only axis .. depth (JP_PRE doubles from JP_PRE_OFF on) -- 20,000 B for ANYmal: EIGHT waves per CU (8 x 20,480 B).
constexpr int JP_PRE_OFF = J_AXIS, JP_PRE = JP - JP_PRE_OFF;
static_assert(JP_PRE_OFF == J_AXIS && J_R < J_AXIS && J_P < J_AXIS, "with the pre-pass the walk stages the joint record without its placement");
__host__ __device__ constexpr size_t lin_lds_bytes(int nlevels, int nbranch, int njoints, int ncontacts, int nv, int dpp, bool pre) {
  return sizeof(double) * ((size_t)nlevels * VAL_DOUBLES + (size_t)(nbranch * FWD_SLOTS + (nlevels > 1 ? nlevels - 1 : 0) * DF_SLOTS) * lin_lane_stride(dpp) +
                           (pre ? 0 : lin_pad8(nv + 1) + 3 * lin_pad8(nv) + lin_pad8(6 * ncontacts)) + lin_pad8(nv) + 2 * lin_pad8(6 * ncontacts) +
                           njoints * (pre ? JP_PRE : JP) + ncontacts * CP);
}

// Per-level storage of the kernels that walk the tree with one Jacobian column per lane (contact_cone_kernel,
// switching_constraint_lin_kernel): the head of a value block through V_OP, then this lane's twist (6 doubles x 64 lanes).
// The pieces of the carve in their order, in doubles: levels' values | levels' twists | joint records | contact records; what
// follows is the kernel's own.  The size functions sum them, the kernels step their pointers by them.
static_assert(V_OP + 3 <= LVL_VAL && LVL_VAL % 2 == 0, "a level keeps R, p, oR, op");
struct LevelCarve {
  size_t val, tan;
  int joint, contact;
  __host__ __device__ constexpr LevelCarve(int nlevels, int njoints, int ncontacts)
      : val((size_t)nlevels * LVL_VAL), tan((size_t)nlevels * LVL_TAN * LVL_LANES), joint(njoints * JP), contact(ncontacts * CP) {}
  __host__ __device__ constexpr size_t doubles() const { return val + tan + joint + contact; }
};

// bodies a pass with the dofs [j0, j1) has to visit
inline unsigned long long pass_body_mask(const rtoc_robot_model& m, int j0, int j1) {
  unsigned long long mask = 0;
  for (int b = 0; b < m.njoints; ++b) {
    const int ndof = m.type[b] == RTOC_JOINT_FREE_FLYER ? 6 : 1;
    if (m.idx_v[b] + ndof <= j0 || m.idx_v[b] >= j1) continue;   // no dof of body b in the pass
    for (int i = 0; i < m.njoints; ++i) {
      bool up = false, down = false;   // b above-or-at i; b below i
      for (int k = i; k >= 0; k = m.parent[k]) {
        if (k == b) up = true;
        if (m.parent[k] < 0 || m.parent[k] >= k) break;
      }
      for (int k = b; k >= 0; k = m.parent[k]) {
        if (k == i) down = true;
        if (m.parent[k] < 0 || m.parent[k] >= k) break;
      }
      if (up || down) mask |= 1ull << i;
    }
  }
  return mask;
}
// dofs per pass: what minimises (bodies visited over all passes) / (waves a CU holds).  The walk is one dependent instruction
// stream per wave, so a CU's rate is its resident waves -- set by the LDS of the per-lane tangents, i.e. by the lanes of a pass --
// over the visits per grid point: ANYmal one pass of 18 dofs (8 waves per CU), iCub 3 passes of 12 instead of 2 of 21.
// max_waves: what the registers of the kernel allow per CU (8; 4 with surface contacts: 256 VGPRs + AGPRs).
inline int choose_dofs_per_pass(const rtoc_robot_model& m, int nlevels, int nbranch, int max_waves) {
  const int dmax = m.nv < LIN_MAX_DPP ? m.nv : LIN_MAX_DPP, dmin = dmax < 6 ? dmax : 6;
  int best = dmax;
  double best_cost = 1e300;
  for (int d = dmax; d >= dmin && d >= 1; --d) {   // ties: the larger pass
    const size_t bytes = (lin_lds_bytes(nlevels, nbranch, m.njoints, m.ncontacts, m.nv, d, true) + 1279) / 1280 * 1280;
    int waves = (int)(160 * 1024 / bytes);
    waves = waves > max_waves ? max_waves : waves;
    if (waves < 1) continue;
    int visits = m.njoints;   // the first pass visits every body
    for (int j0 = d; j0 < m.nv; j0 += d) visits += __builtin_popcountll(pass_body_mask(m, j0, j0 + d < m.nv ? j0 + d : m.nv));
    const double cost = (double)visits / waves;
    if (cost < best_cost - 1e-9) best_cost = cost, best = d;
  }
  return best;
}
inline void plan_passes(DevModel* h, int forced_dpp) {
  const rtoc_robot_model& m = h->m;
  bool surf = false;
  for (int c = 0; c < m.ncontacts; ++c) surf = surf || m.contact_type[c] == RTOC_CONTACT_SURFACE;
  h->dpp = forced_dpp > 0 ? (forced_dpp < m.nv ? forced_dpp : (m.nv < LIN_MAX_DPP ? m.nv : LIN_MAX_DPP)) : choose_dofs_per_pass(m, h->nlevels, h->nbranch, surf ? 4 : 8);
  for (int p = 0; p < RTOC_MAX_JOINTS + 8; ++p) {
    h->pass_bodies[p] = 0, h->pass_nvisit[p] = 0;
    for (int i = 0; i < RTOC_MAX_JOINTS; ++i) h->pass_visit[p][i] = 0;
  }
  h->npass = (m.nv + h->dpp - 1) / h->dpp;
  for (int p = 0; p < h->npass; ++p) h->pass_bodies[p] = pass_body_mask(m, p * h->dpp, (p + 1) * h->dpp < m.nv ? (p + 1) * h->dpp : m.nv);
  h->pass_bodies[0] |= m.njoints >= 64 ? ~0ull : (1ull << m.njoints) - 1;   // the first pass writes the values of the contact rows: every body
  for (int p = 0; p < h->npass; ++p)
    for (int i = 0; i < m.njoints; ++i)
      if ((h->pass_bodies[p] >> i) & 1ull) h->pass_visit[p][h->pass_nvisit[p]++] = i;
}

}  // namespace rbd
}  // namespace rtoc
