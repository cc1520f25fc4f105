// rigid_body_math.hpp -- the one device copy of the rotation and SE(3) arithmetic of the kernels: 3-vectors, spatial motions /
// forces, rotations (transpose, relative placement A^-1 B, quaternion <-> matrix, the revolute joint's Rodrigues rotation, the
// placement of a joint from its joint record and the configuration, unit twists), log6 with its forward-mode derivative, exp6
// with its coefficients and translation part, the block-triangular 6 x 6 inverse of the SE(3) Jacobians, and the scalar-cache
// load of the device model.  Device functions only; the slot names of the joint record come from rigid_body_model.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "rigid_body_model.hpp"

namespace rtoc {
namespace rbd {

struct V3 {
  double x, y, z;
};
struct SV {  // spatial motion or force: linear, angular
  V3 l, a;
};
__device__ __forceinline__ V3 mk(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ SV operator+(SV a, SV b) { return SV{a.l + b.l, a.a + b.a}; }
__device__ __forceinline__ SV operator-(SV a, SV b) { return SV{a.l - b.l, a.a - b.a}; }
__device__ __forceinline__ SV sv0() { return SV{mk(0, 0, 0), mk(0, 0, 0)}; }

struct M3 {  // row-major
  double m[9];
};
__device__ __forceinline__ V3 mul(const M3& R, V3 v) {
  return mk(R.m[0] * v.x + R.m[1] * v.y + R.m[2] * v.z, R.m[3] * v.x + R.m[4] * v.y + R.m[5] * v.z,
            R.m[6] * v.x + R.m[7] * v.y + R.m[8] * v.z);
}
__device__ __forceinline__ V3 mulT(const M3& R, V3 v) {
  return mk(R.m[0] * v.x + R.m[3] * v.y + R.m[6] * v.z, R.m[1] * v.x + R.m[4] * v.y + R.m[7] * v.z,
            R.m[2] * v.x + R.m[5] * v.y + R.m[8] * v.z);
}
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
  M3 C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C.m[3 * i + j] = A.m[3 * i] * B.m[j] + A.m[3 * i + 1] * B.m[3 + j] + A.m[3 * i + 2] * B.m[6 + j];
  return C;
}
// child-frame coordinates of a parent-frame motion, X = (R, p)
__device__ __forceinline__ SV act_inv(const M3& R, V3 p, SV m) { return SV{mulT(R, m.l - cross(p, m.a)), mulT(R, m.a)}; }
// parent-frame coordinates of a child-frame force
__device__ __forceinline__ SV act_f(const M3& R, V3 p, SV f) {
  const V3 l = mul(R, f.l);
  return SV{l, mul(R, f.a) + cross(p, l)};
}
__device__ __forceinline__ SV mcross(SV v, SV m) { return SV{cross(v.a, m.l) + cross(v.l, m.a), cross(v.a, m.a)}; }   // v x m
__device__ __forceinline__ SV fcross(SV v, SV f) { return SV{cross(v.a, f.l), cross(v.a, f.a) + cross(v.l, f.l)}; }   // v x* f
__device__ __forceinline__ SV inertia_mul(double mass, V3 c, const M3& I, SV v) {
  const V3 l = mass * (v.l - cross(c, v.a));
  return SV{l, mul(I, v.a) + cross(c, l)};
}
__device__ __forceinline__ M3 ldm3(const double* p) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.m[i] = p[i];
  return r;
}
__device__ __forceinline__ V3 ldv3(const double* p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ void stv3(double* d, V3 x) { d[0] = x.x, d[1] = x.y, d[2] = x.z; }
__device__ __forceinline__ SV ldsv(const double* p) { return SV{ldv3(p), ldv3(p + 3)}; }
__device__ __forceinline__ void stsv(double* d, SV x) { stv3(d, x.l), stv3(d + 3, x.a); }
__device__ __forceinline__ M3 transpose(const M3& A) {
  M3 T;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T.m[3 * r + c] = A.m[3 * c + r];
  return T;
}
// X = A^-1 B for placements A = (Ra, pa), B = (Rb, pb)
__device__ __forceinline__ void rel(const M3& Ra, V3 pa, const M3& Rb, V3 pb, M3& R, V3& p) {
  R = mul(transpose(Ra), Rb);
  p = mulT(Ra, pb - pa);
}
// rotation matrix of the unit quaternion q = (x, y, z, w)
__device__ __forceinline__ M3 quat_R(const double* q) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  M3 R;
  R.m[0] = 1 - 2 * (y * y + z * z), R.m[1] = 2 * (x * y - z * w), R.m[2] = 2 * (x * z + y * w);
  R.m[3] = 2 * (x * y + z * w), R.m[4] = 1 - 2 * (x * x + z * z), R.m[5] = 2 * (y * z - x * w);
  R.m[6] = 2 * (x * z - y * w), R.m[7] = 2 * (y * z + x * w), R.m[8] = 1 - 2 * (x * x + y * y);
  return R;
}
// the normalised quaternion q = (x, y, z, w) of a rotation matrix: w > 0 where the trace is positive, else the largest diagonal
// entry leads.  Out through an array written from locals: with four reference outputs the compiler began the sum of squares
// below at another term, one ulp in the interpolated quaternion
__device__ __forceinline__ void R_quat(const M3& R, double* q) {
  double x, y, z, w;
  const double tr = R.m[0] + R.m[4] + R.m[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s, x = (R.m[7] - R.m[5]) / s, y = (R.m[2] - R.m[6]) / s, z = (R.m[3] - R.m[1]) / s;
  } else if (R.m[0] >= R.m[4] && R.m[0] >= R.m[8]) {
    const double s = sqrt(fmax(0.0, 1.0 + R.m[0] - R.m[4] - R.m[8])) * 2.0;
    x = 0.25 * s, y = (R.m[3] + R.m[1]) / s, z = (R.m[6] + R.m[2]) / s, w = (R.m[7] - R.m[5]) / s;
  } else if (R.m[4] >= R.m[8]) {
    const double s = sqrt(fmax(0.0, 1.0 + R.m[4] - R.m[8] - R.m[0])) * 2.0;
    y = 0.25 * s, z = (R.m[7] + R.m[5]) / s, x = (R.m[1] + R.m[3]) / s, w = (R.m[2] - R.m[6]) / s;
  } else {
    const double s = sqrt(fmax(0.0, 1.0 + R.m[8] - R.m[0] - R.m[4])) * 2.0;
    z = 0.25 * s, x = (R.m[2] + R.m[6]) / s, y = (R.m[5] + R.m[7]) / s, w = (R.m[3] - R.m[1]) / s;
  }
  const double n = sqrt(x * x + y * y + z * z + w * w);
  q[0] = x / n, q[1] = y / n, q[2] = z / n, q[3] = w / n;
}
// rotation of a revolute joint about its unit axis (Rodrigues), from the sine and cosine of the angle: the caller evaluates them
__device__ __forceinline__ M3 revolute_R(V3 ax, double sn, double cs) {
  const double t = 1.0 - cs;
  M3 R;
  R.m[0] = t * ax.x * ax.x + cs, R.m[1] = t * ax.x * ax.y - sn * ax.z, R.m[2] = t * ax.x * ax.z + sn * ax.y;
  R.m[3] = t * ax.x * ax.y + sn * ax.z, R.m[4] = t * ax.y * ax.y + cs, R.m[5] = t * ax.y * ax.z - sn * ax.x;
  R.m[6] = t * ax.x * ax.z - sn * ax.y, R.m[7] = t * ax.y * ax.z + sn * ax.x, R.m[8] = t * ax.z * ax.z + cs;
  return R;
}
// placement (R, p) of a joint in its parent's frame: the fixed placement of its joint record (`fixed` points at its J_R, the
// offset J_P follows) times the joint's own transform (Rj, pj)
__device__ __forceinline__ void joint_placement(const double* fixed, const M3& Rj, V3 pj, M3& R, V3& p) {
  const M3 Rp = ldm3(fixed);
  R = mul(Rp, Rj);
  p = mul(Rp, pj) + ldv3(fixed + (J_P - J_R));
}
// the same at the configuration q: `jm` the joint record, `qj` the joint's coordinates in q (at J_IDXQ) -- a free-flyer's position
// and quaternion, a revolute joint's angle about J_AXIS
__device__ __forceinline__ void joint_placement_at(const double* jm, bool free_flyer, const double* qj, M3& R, V3& p) {
  M3 Rj;
  V3 pj = mk(0, 0, 0);
  if (free_flyer) {
    Rj = quat_R(qj + 3);
    pj = ldv3(qj);
  } else {
    const double th = qj[0];
    Rj = revolute_R(ldv3(jm + J_AXIS), sin(th), cos(th));
  }
  joint_placement(jm + J_R, Rj, pj, R, p);
}
// S_k of a free-flyer joint: the k-th unit twist (linear 0..2, angular 3..5)
__device__ __forceinline__ SV unit_twist(int k) { return SV{mk(k == 0, k == 1, k == 2), mk(k == 3, k == 4, k == 5)}; }

// pinocchio::log6 of X = (R, p) and its derivative along the right perturbation X exp(twist) (what Jlog6 * twist is):
//   w = log3 R,  lin = p - w x p / 2 + beta w x (w x p),  beta(t) = 1/t^2 - cot(t/2) / (2 t)  (= the Jlog3 coefficient too)
//   dw = twist.a + w x twist.a / 2 + beta w x (w x twist.a),  dp = R twist.l,  dt = w.dw / t
__device__ __forceinline__ void log6_fwd(const M3& R, V3 p, SV twist, SV& val, SV& der) {
  const double tr = R.m[0] + R.m[4] + R.m[8];
  double c = 0.5 * (tr - 1.0);
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  const V3 as = mk(R.m[7] - R.m[5], R.m[2] - R.m[6], R.m[3] - R.m[1]);  // vee(R - R^T) = 4 q_w (q_x, q_y, q_z)
  V3 w;
  if (c < -0.99) {
    // Near pi the antisymmetric part vanishes and theta / (2 sin theta) amplifies its rounding like 1 / (pi - theta)^2; at pi it
    // is 0 / 0.  Take 4 q_i (q_x, q_y, q_z, q_w) of the quaternion of R instead, i the largest diagonal entry (q_i^2 >= 1/3 here:
    // no cancellation), and w = 2 atan2(|v|, q_w) v / |v|, in which the scale drops out.  Uniform over the lanes of a call.
    const double d0 = R.m[0], d1 = R.m[4], d2 = R.m[8];
    const double sxy = R.m[1] + R.m[3], sxz = R.m[2] + R.m[6], syz = R.m[5] + R.m[7];
    V3 v;
    double qw;
    if (d0 >= d1 && d0 >= d2) {
      v = mk(1.0 + d0 - d1 - d2, sxy, sxz), qw = as.x;
    } else if (d1 >= d2) {
      v = mk(sxy, 1.0 + d1 - d0 - d2, syz), qw = as.y;
    } else {
      v = mk(sxz, syz, 1.0 + d2 - d0 - d1), qw = as.z;
    }
    // atan2(|v|, |q_w|) = pi/2 - atan x, x = |q_w| / |v| = cot(theta / 2) < 0.071 on this branch: seven terms of the series of atan
    // (the next one is below 4e-19) instead of the library's atan2, whose registers the rigid-body kernels do not have to spare
    const double n = sqrt(dot(v, v)), x = fabs(qw) / n, x2 = x * x;
    const double at = x * (1.0 + x2 * (-1.0 / 3.0 + x2 * (1.0 / 5.0 + x2 * (-1.0 / 7.0 + x2 * (1.0 / 9.0 + x2 * (-1.0 / 11.0 + x2 * (1.0 / 13.0)))))));
    w = ((qw < 0.0 ? -2.0 : 2.0) * (1.57079632679489661923 - at) / n) * v;
  } else {
    const double th = acos(c);
    const double k = th < 1e-6 ? 0.5 + th * th / 12.0 : th / (2.0 * sin(th));
    w = mk(k * as.x, k * as.y, k * as.z);
  }
  const double t = sqrt(dot(w, w));
  double beta, dbeta;
  if (t < 1e-3) {
    beta = 1.0 / 12.0 + t * t / 720.0;
    dbeta = t / 360.0 + t * t * t / 7560.0;
  } else if (t < 0.005) {
    // the closed forms below cancel like 1e-16 / t^2 and 1e-16 / t^3, which puts Jlog6 off by about 1.5e-16 |p| / t: the series
    // above continued (truncated under 1e-22) up to where that is 3e-14 |p|, a third of the 1e-13 the derivatives are held to --
    // the margin of the near-pi switch; from there on the closed forms, as before
    const double t2 = t * t;
    beta = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0;
    dbeta = t / 360.0 + t * t2 / 7560.0 + t * t2 * t2 / 201600.0;
  } else {
    const double h = 0.5 * t, ct = cos(h) / sin(h), cs2 = 1.0 / (sin(h) * sin(h));
    beta = 1.0 / (t * t) - ct / (2.0 * t);
    dbeta = -2.0 / (t * t * t) + ct / (2.0 * t * t) + cs2 / (4.0 * t);
  }
  const V3 wxp = cross(w, p), wxwxp = cross(w, wxp);
  val = SV{p - 0.5 * wxp + beta * wxwxp, w};
  const V3 ta = twist.a;
  const V3 dw = ta + 0.5 * cross(w, ta) + beta * cross(w, cross(w, ta));
  const V3 dp = mul(R, twist.l);
  const double dt = t > 1e-12 ? dot(w, dw) / t : 0.0;
  const V3 dlin = dp - 0.5 * (cross(dw, p) + cross(w, dp)) + (dbeta * dt) * wxwxp +
                  beta * (cross(dw, wxp) + cross(w, cross(dw, p)) + cross(w, cross(w, dp)));
  der = SV{dlin, dw};
}

// The coefficients of exp3 = I + S K + C K^2 and of V = I + C K + B K^2 in exp6([v; w]) = (exp3(w), V(w) v), K = skew w:
//   S = sin t / t,  C = (1 - cos t) / t^2,  B = (t - sin t) / t^3   at t = |w|, t2 = t^2.
// 1 - cos t cancels: the quotient is off by about 1e-16 / t^2 and V(w) v by 1e-16 |v| / t -- 1e-9 |v| at t = 1e-7, the angle of
// a time step of a base that barely turns.  So below 1e-3 three terms of the series in t^2 (the next one is under 3e-22) and
// above it 2 sin^2(t/2) / t^2, which loses nothing.  t - sin t cancels the same way, B is off by about 1e-16 / t^2 (1e-10
// relative at 1e-3), but it only ever meets w x (w x v), which is t^2 |v|: 1e-16 |v| at any angle.  Against the 50-digit
// reference either side of 1e-3 stays under 0.004 of the 1e-13 max(1, |v|) the exponential is held to
// (tests/test_lie_exp_branch_points*.py).
__device__ __forceinline__ void exp_coefficients(double t2, double t, double& S, double& C, double& B) {
  if (t < 1e-3) {
    S = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
    C = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    B = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
  } else {
    const double sh = sin(0.5 * t), s = sin(t);
    S = s / t, C = 2.0 * sh * sh / t2, B = (t - s) / (t2 * t);
  }
}
// V(w) v = v + C w x v + B w x (w x v), C and B from exp_coefficients
__device__ __forceinline__ V3 exp6_translation(V3 v, V3 w, double C, double B) {
  const V3 wxv = cross(w, v);
  return v + C * wxv + B * cross(w, wxv);
}
// exp6([v; w]) = (E, p): E = I + S K + C K^2 with K^2 = w w^T - t^2 I written out (no products with the zeros of K)
__device__ __forceinline__ void exp6(V3 v, V3 w, M3& E, V3& p) {
  const double t2 = dot(w, w);
  double S, C, B;
  exp_coefficients(t2, sqrt(t2), S, C, B);
  p = exp6_translation(v, w, C, B);
  E.m[0] = 1.0 - C * (w.y * w.y + w.z * w.z), E.m[1] = C * w.x * w.y - S * w.z, E.m[2] = C * w.x * w.z + S * w.y;
  E.m[3] = C * w.x * w.y + S * w.z, E.m[4] = 1.0 - C * (w.x * w.x + w.z * w.z), E.m[5] = C * w.y * w.z - S * w.x;
  E.m[6] = C * w.x * w.z - S * w.y, E.m[7] = C * w.y * w.z + S * w.x, E.m[8] = 1.0 - C * (w.x * w.x + w.y * w.y);
}

// Inverse of a 6 x 6 block upper-triangular matrix [[A, B], [0, D]] (column-major, 3 x 3 blocks) -- the shape of Jlog6 and
// of Ad in the (linear, angular) ordering, hence of every SE(3) difference Jacobian here: [[A^-1, -A^-1 B D^-1], [0, D^-1]]
// with the 3 x 3 inverses by cofactors (what the reference's SE3JacobianInverse exploits, se3_jacobian_inverse.hxx).  All
// indices are compile-time constants: the arrays stay in registers (a general inverse pivots, i.e. indexes at run time,
// which puts its 72 doubles into scratch memory).
__device__ __forceinline__ void inv3(const double (&m)[3][3], double (&o)[3][3]) {
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double id = 1.0 / (m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02);
  o[0][0] = c00 * id, o[1][0] = c01 * id, o[2][0] = c02 * id;
  o[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id, o[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id, o[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id;
  o[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id, o[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id, o[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id;
}
__device__ __forceinline__ void inv6_block_ut(const double* J, double* out) {
  double A[3][3], B[3][3], D[3][3], Ai[3][3], Di[3][3], T[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = J[r + 6 * c], B[r][c] = J[r + 6 * (c + 3)], D[r][c] = J[r + 3 + 6 * (c + 3)];
  inv3(A, Ai);
  inv3(D, Di);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T[r][c] = Ai[r][0] * B[0][c] + Ai[r][1] * B[1][c] + Ai[r][2] * B[2][c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out[r + 6 * c] = Ai[r][c];
      out[r + 3 + 6 * c] = 0.0;
      out[r + 3 + 6 * (c + 3)] = Di[r][c];
      out[r + 6 * (c + 3)] = -(T[r][0] * Di[0][c] + T[r][1] * Di[1][c] + T[r][2] * Di[2][c]);
    }
}

// an int of the device model through the scalar cache: the model is read-only while a kernel runs, but the compiler cannot know
// (the kernel stores through other pointers) and would issue a vector load + v_readfirstlane on the walk's critical path
typedef const int __attribute__((address_space(4))) lin_const_int;
__device__ __forceinline__ int sload_int(const int* p) { return *(lin_const_int*)(unsigned long long)p; }

}  // namespace rbd
}  // namespace rtoc
