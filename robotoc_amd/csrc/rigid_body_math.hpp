// rigid_body_math.hpp -- spatial-vector arithmetic of the rigid-body kernels: 3-vectors, spatial motions / forces, rotations,
// log6 with its forward-mode derivative, and the scalar-cache load of the device model.  Device functions only.
#pragma once
#include <hip/hip_runtime.h>

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

// an int of the device model through the scalar cache: the model is read-only while a kernel runs, but the compiler cannot know
// (the kernel stores through other pointers) and would issue a vector load + v_readfirstlane on the walk's critical path
typedef const int __attribute__((address_space(4))) lin_const_int;
__device__ __forceinline__ int sload_int(const int* p) { return *(lin_const_int*)(unsigned long long)p; }

}  // namespace rbd
}  // namespace rtoc
