// parnmpc_backward_correction.hpp -- the backward correction of UnconstrParNMPC (backward Euler, fixed base, no contacts).
//
// Replaces UnconstrBackwardCorrection::coarseUpdate / backwardCorrection (reference src/parnmpc/unconstr_backward_correction.cpp:
// 154-228, without the evalKKT and the expansion inside them), UnconstrSplitBackwardCorrection (unconstr_split_backward_correction.cpp:
// 57-133, .hpp:162-182) and UnconstrKKTMatrixInverter::invert (unconstr_kkt_matrix_inverter.hxx:39-79), on CONDENSED records in the
// convention of rtoc_unconstr_condense (KKT.Quu = Qaa, KKT.lu = la, KKT.Qxu = [Qqa; Qva]).
//
// Per stage the KKT system over (lmd, gmm | a, q, v) is the saddle matrix K = [[0, F], [F^T, H]] with H (3nv x 3nv, SPD) over
// (a, q, v) and the constant backward-Euler Jacobian F = [[0, -I, dt I], [dt I, 0, -I]].  Two kernels:
//   parnmpc_coarse_kernel   one wavefront per (instance, stage), the stages independent of each other: H^-1 by the blocked Cholesky-
//       with-inverse of wave_llt.hpp (16 < 3nv <= 32, trailing update on the matrix cores), F H^-1 and S = F H^-1 F^T as row and
//       column combinations (F is +-I / dt I blocks: no product), S^-1 by the one-block Cholesky-with-inverse (2nv <= 16), the blocks
//       of K^-1 = [[-S^-1, S^-1 F H^-1], [.^T, H^-1 - (.)^T S (.)]], the coarse update s_new = s - K^-1 [Fx; la; lx].  Of K^-1 only
//       what the correction passes read goes to HBM: rows 0:2nv (all 5nv columns; its transpose serves the forward passes, its
//       first 2nv columns are the next auxiliary matrix) and the block [2nv:5nv, 3nv:5nv] -- 16 nv^2 doubles per stage instead of 25.
//   parnmpc_correct_kernel  one workgroup per instance: backwardCorrectionSerial (i = N-2 .. 0) and forwardCorrectionSerial
//       (i = 1 .. N-1) by its first wave -- a 2nv x 2nv matrix-vector product per step whose matrix does not depend on the chain and
//       is fetched one step ahead, the vector carried in registers --, backwardCorrectionParallel / forwardCorrectionParallel,
//       aux_mat[i] = -K^-1[0:2nv, 0:2nv] and computeDirection by all of its waves, workgroup barriers in between.  Every loop is
//       bounded by the horizon; no wave waits on anything another workgroup writes.
// The order of the four passes and the lag of the auxiliary matrices are the reference's: H of stage i < N-1 takes aux_mat[i+1] of
// the PREVIOUS call, and this call leaves -K^-1[0:2nv, 0:2nv] of its own H behind for the next one.
// A non-SPD H or S raises RTOC_STAT_PARNMPC_H_NOT_SPD / RTOC_STAT_PARNMPC_S_NOT_SPD on the instance; parnmpc_correct_kernel then
// zeroes that instance's direction and leaves its auxiliary matrices alone.  Other instances never read its data.
#pragma once
#include "device_utils.hpp"
#include "kernel_args.hpp"  // PbcArgs
#include "wave_llt.hpp"
#include "../../include/rtoc.h"

namespace rtoc {

template <int NV>
struct PbcCfg {
  static constexpr int N2 = 2 * NV, N3 = 3 * NV, N5 = 5 * NV;
  static constexpr bool OK = N3 > 16 && N3 <= 32 && N2 <= 16;  // the two factorisations of wave_llt.hpp that fit
  static constexpr int KINV = 16 * NV * NV;                   // doubles of K^-1 kept per stage: N2 x N5, then N3 x N2
};

// entry idx of a stage's solution in the order (lmd, gmm, a, q, v)
template <int NV>
__device__ __forceinline__ double pbc_sol(const double* sr, const rtoc_record_layout& sl, int idx) {
  const int f = idx / NV, k = idx - f * NV;
  const int field = f == 0 ? RTOC_SOL_LMD : f == 1 ? RTOC_SOL_GMM : f == 2 ? RTOC_SOL_A : f == 3 ? RTOC_SOL_Q : RTOC_SOL_V;
  return sr[sl.off[field] + k];
}

template <int NV>
__global__ __launch_bounds__(64) void parnmpc_coarse_kernel(PbcArgs a) {
  using Cfg = PbcCfg<NV>;
  constexpr int N2 = Cfg::N2, N3 = Cfg::N3, N5 = Cfg::N5, NX = 2 * NV;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / a.nstages, st = blockIdx.x % a.nstages;
  if (b >= a.batch) return;
  const size_t rec = (size_t)b * a.nstages + st;
  const double* const kr = a.kkt + rec * a.kl.stride;
  const double* const sr = a.sol + rec * a.sl.stride;
  __shared__ double Hm[N3 * N3], Lm[N3 * N3], Ym[N3 * N3], scr[256], linv[32];
  __shared__ double FH[N2 * N3], Sm[N2 * N2], Ys[N2 * N2], Si[N2 * N2], Bm[N2 * N3], Tm[N2 * N3], rv[N5];
  // ---- H (coarseUpdate_impl, .hpp:168-171; the terminal overload adds no aux matrix, .cpp:61-63) and the residual (:173-175) ----
  {
    const double* const Quu = kr + a.kl.off[RTOC_KKT_QUU];
    const double* const Qxu = kr + a.kl.off[RTOC_KKT_QXU];
    const double* const Qxx = kr + a.kl.off[RTOC_KKT_QXX];
    const bool last = st == a.nstages - 1;
    const double* const aux_next = a.aux + (rec + (last ? 0 : 1)) * (size_t)(N2 * N2);
    for (int e = lane; e < N3 * N3; e += 64) {
      const int r = e % N3, c = e / N3;
      double v;
      if (r < NV && c < NV) v = Quu[r + c * NV];
      else if (c < NV) v = Qxu[(r - NV) + c * NX];
      else if (r < NV) v = Qxu[(c - NV) + r * NX];
      else v = Qxx[(c - NV) + (r - NV) * NX] + (last ? 0.0 : aux_next[(r - NV) + (c - NV) * N2]);
      Hm[e] = v;
    }
    if (lane < N5)
      rv[lane] = lane < N2 ? kr[a.kl.off[RTOC_KKT_FX] + lane] : lane < N3 ? kr[a.kl.off[RTOC_KKT_LU] + (lane - N2)] : kr[a.kl.off[RTOC_KKT_LX] + (lane - N3)];
  }
  __syncthreads();
  // ---- H^-1 = Y^T Y, Y = L^-1 (llt_H_.solve(Identity), .hxx:46-49) ----
  const bool bad_h = wave_llt_inv_blocked<N3, N3>(Hm, Lm, linv, Ym, scr, lane);
  __syncthreads();
  for (int e = lane; e < N3 * N3; e += 64) {
    const int i = e % N3, j = e / N3;
    double acc = 0.0;
    for (int k = (i > j ? i : j); k < N3; ++k) acc += Ym[k + i * N3] * Ym[k + j * N3];
    Hm[e] = acc;
  }
  __syncthreads();
  // ---- F H^-1 (.hxx:50-55): rows of H^-1 combined ----
  const double dt = a.dt;
  for (int e = lane; e < N2 * N3; e += 64) {
    const int r = e % N2, c = e / N2;
    FH[e] = r < NV ? -Hm[(NV + r) + c * N3] + dt * Hm[(2 * NV + r) + c * N3] : dt * Hm[(r - NV) + c * N3] - Hm[(NV + r) + c * N3];
  }
  __syncthreads();
  // ---- S = F H^-1 F^T (.hxx:56-67): columns of F H^-1 combined ----
  for (int e = lane; e < N2 * N2; e += 64) {
    const int r = e % N2, c = e / N2;
    Sm[e] = c < NV ? -FH[r + (NV + c) * N2] + dt * FH[r + (2 * NV + c) * N2] : dt * FH[r + (c - NV) * N2] - FH[r + (NV + c) * N2];
  }
  __syncthreads();
  // ---- S^-1 (.hxx:68-71) ----
  const bool bad_s = wave_llt_inv<N2, N2, 16, false>(Sm, nullptr, nullptr, Ys, N2, lane);
  __syncthreads();
  for (int e = lane; e < N2 * N2; e += 64) {
    const int i = e % N2, j = e / N2;
    double acc = 0.0;
    for (int k = (i > j ? i : j); k < N2; ++k) acc += Ys[k + i * N2] * Ys[k + j * N2];
    Si[e] = acc;
  }
  __syncthreads();
  // ---- B = K^-1[0:2nv, 2nv:5nv] = S^-1 F H^-1 (.hxx:72-73) ----
  for (int e = lane; e < N2 * N3; e += 64) {
    const int r = e % N2, c = e / N2;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k) acc += Si[r + k * N2] * FH[k + c * N2];
    Bm[e] = acc;
  }
  __syncthreads();
  // ---- K^-1[2nv:5nv, 2nv:5nv] = H^-1 - B^T (S B) (.hxx:76-78), into Lm ----
  for (int e = lane; e < N2 * N3; e += 64) {
    const int r = e % N2, c = e / N2;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k) acc += Sm[r + k * N2] * Bm[k + c * N2];
    Tm[e] = acc;
  }
  __syncthreads();
  for (int e = lane; e < N3 * N3; e += 64) {
    const int i = e % N3, j = e / N3;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k) acc += Bm[k + i * N2] * Tm[k + j * N2];
    Lm[e] = Hm[e] - acc;
  }
  __syncthreads();
  // ---- d = K^-1 [Fx; la; lx], s_new = s - d (.hpp:176-181) ----
  if (lane < N5) {
    double d = 0.0;
    if (lane < N2) {
      for (int k = 0; k < N2; ++k) d -= Si[lane + k * N2] * rv[k];
      for (int k = 0; k < N3; ++k) d += Bm[lane + k * N2] * rv[N2 + k];
    } else {
      const int i = lane - N2;
      for (int k = 0; k < N2; ++k) d += Bm[k + i * N2] * rv[k];
      for (int k = 0; k < N3; ++k) d += Lm[i + k * N3] * rv[N2 + k];
    }
    a.snew[rec * N5 + lane] = pbc_sol<NV>(sr, a.sl, lane) - d;
  }
  // ---- what the correction passes read of K^-1 ----
  double* const kv = a.kinv + rec * (size_t)Cfg::KINV;
  for (int e = lane; e < N2 * N2; e += 64) kv[e] = -Si[e];
  for (int e = lane; e < N2 * N3; e += 64) kv[N2 * N2 + e] = Bm[e];
  for (int e = lane; e < N3 * N2; e += 64) kv[N2 * N5 + e] = Lm[e + NV * N3];   // columns nv .. 3nv of the (a, q, v) block
  if (lane == 0 && (bad_h || bad_s)) atomicOr(&a.status[b], (bad_h ? RTOC_STAT_PARNMPC_H_NOT_SPD : 0u) | (bad_s ? RTOC_STAT_PARNMPC_S_NOT_SPD : 0u));
}

constexpr int PBC_CORRECT_NT = 256;

template <int NV>
__global__ __launch_bounds__(PBC_CORRECT_NT) void parnmpc_correct_kernel(PbcArgs a) {
  using Cfg = PbcCfg<NV>;
  constexpr int N2 = Cfg::N2, N3 = Cfg::N3, N5 = Cfg::N5, NT = PBC_CORRECT_NT;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, N = a.nstages;
  if (b >= a.batch) return;
  const size_t rec0 = (size_t)b * N;
  const double* const sol = a.sol + rec0 * a.sl.stride;
  double* const dir = a.dir + rec0 * a.dl.stride;
  double* const snew = a.snew + rec0 * N5;
  double* const xres = a.xres + rec0 * N2;
  const double* const kinv = a.kinv + rec0 * (size_t)Cfg::KINV;
  auto write_direction = [&](bool zero) {   // computeDirection (.cpp:125-133) into the SplitDirection record
    for (int it = tid; it < N * N5; it += NT) {
      const int i = it / N5, idx = it - i * N5;
      const double d = zero ? 0.0 : snew[(size_t)i * N5 + idx] - pbc_sol<NV>(sol + (size_t)i * a.sl.stride, a.sl, idx);
      double* const dr = dir + (size_t)i * a.dl.stride;
      if (idx < N2) dr[a.dl.off[RTOC_DIR_DLMDGMM] + idx] = d;
      else if (idx < N3) dr[a.dl.off[RTOC_DIR_DU] + (idx - N2)] = d;   // da: the control of the unconstrained records
      else dr[a.dl.off[RTOC_DIR_DX] + (idx - N3)] = d;
    }
  };
  if (a.status[b] & (RTOC_STAT_PARNMPC_H_NOT_SPD | RTOC_STAT_PARNMPC_S_NOT_SPD)) {   // (uniform over the workgroup)
    write_direction(true);
    return;
  }
  // ---- backwardCorrectionSerial, i = N-2 .. 0 (unconstr_backward_correction.cpp:196-198; split .cpp:83-91) ----
  if (tid < 64 && N > 1) {
    const int l = tid < N2 ? tid : 0;
    double m[N2], mn[N2];
    // row l of K^-1[0:2nv, 3nv:5nv] of stage i
    auto fetch = [&](int i, double (&dst)[N2]) {
      const double* const p = kinv + (size_t)i * Cfg::KINV;
#pragma unroll
      for (int k = 0; k < N2; ++k) dst[k] = p[l + (N3 + k) * N2];
    };
    fetch(N - 2, mn);
    double x = snew[(size_t)(N - 1) * N5 + l] - pbc_sol<NV>(sol + (size_t)(N - 1) * a.sl.stride, a.sl, l);
    for (int i = N - 2; i >= 0; --i) {
#pragma unroll
      for (int k = 0; k < N2; ++k) m[k] = mn[k];
      if (i > 0) fetch(i - 1, mn);
      double dx = 0.0;
#pragma unroll
      for (int k = 0; k < N2; ++k) dx += m[k] * __shfl(x, k, 64);
      if (tid < N2) xres[(size_t)i * N2 + l] = x;
      const double sn = snew[(size_t)i * N5 + l] - dx;
      if (tid < N2) snew[(size_t)i * N5 + l] = sn;
      x = sn - pbc_sol<NV>(sol + (size_t)i * a.sl.stride, a.sl, l);
    }
  }
  __syncthreads();
  // ---- backwardCorrectionParallel, i < N-1 (:199-202; split .cpp:94-101) ----
  for (int it = tid; it < (N - 1) * N3; it += NT) {
    const int i = it / N3, r = it - i * N3;
    const double* const R = kinv + (size_t)i * Cfg::KINV + N2 * N5;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k) acc += R[r + k * N3] * xres[(size_t)i * N2 + k];
    snew[(size_t)i * N5 + N2 + r] -= acc;
  }
  __syncthreads();
  // ---- forwardCorrectionSerial, i = 1 .. N-1 (:203-205; split .cpp:104-112): K^-1[3nv:5nv, 0:2nv] is the transpose of the stored rows ----
  if (tid < 64 && N > 1) {
    const int l = tid < N2 ? tid : 0;
    double m[N2], mn[N2];
    auto fetch = [&](int i, double (&dst)[N2]) {
      const double* const p = kinv + (size_t)i * Cfg::KINV;
#pragma unroll
      for (int k = 0; k < N2; ++k) dst[k] = p[k + (N3 + l) * N2];
    };
    fetch(1, mn);
    double x = snew[N3 + l] - pbc_sol<NV>(sol, a.sl, N3 + l);
    for (int i = 1; i < N; ++i) {
#pragma unroll
      for (int k = 0; k < N2; ++k) m[k] = mn[k];
      if (i + 1 < N) fetch(i + 1, mn);
      double dx = 0.0;
#pragma unroll
      for (int k = 0; k < N2; ++k) dx += m[k] * __shfl(x, k, 64);
      if (tid < N2) xres[(size_t)i * N2 + l] = x;
      const double sn = snew[(size_t)i * N5 + N3 + l] - dx;
      if (tid < N2) snew[(size_t)i * N5 + N3 + l] = sn;
      x = sn - pbc_sol<NV>(sol + (size_t)i * a.sl.stride, a.sl, N3 + l);
    }
  }
  __syncthreads();
  // ---- forwardCorrectionParallel and aux_mat[i] = -K^-1[0:2nv, 0:2nv], i > 0 (:206-211; split .cpp:115-122) ----
  for (int it = tid; it < (N - 1) * N3; it += NT) {
    const int i = 1 + it / N3, r = it % N3;
    const double* const P = kinv + (size_t)i * Cfg::KINV;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k) acc += (r < N2 ? P[r + k * N2] : P[k + r * N2]) * xres[(size_t)i * N2 + k];
    snew[(size_t)i * N5 + r] -= acc;
  }
  for (int it = tid; it < (N - 1) * N2 * N2; it += NT) {
    const int i = 1 + it / (N2 * N2), e = it % (N2 * N2);
    a.aux[(rec0 + i) * (size_t)(N2 * N2) + e] = -kinv[(size_t)i * Cfg::KINV + e];
  }
  __syncthreads();
  write_direction(false);
}

}  // namespace rtoc
