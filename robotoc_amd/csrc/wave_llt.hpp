// wave_llt.hpp -- in-wave Cholesky factorisation, inverse factor and triangular solves of a small SPD matrix held in LDS: what the
// backward Riccati kernels (riccati_backward*.hpp: the control Hessian G) and the condensation (condense.hpp: the saddle
// matrices) share.  Device functions only.
#pragma once
#include "device_utils.hpp"

namespace rtoc {

// In-wave Cholesky of an n x n SPD matrix held in LDS (column-major, ld = LD).
// Lane i owns row i in registers; pivots / columns travel by wave shuffles.
// Writes the lower factor back to Ldst (ld LD) and 1/diag to linv.  Returns true on failure.
template <int NMAX, int LD>
__device__ __forceinline__ bool wave_llt(const double* __restrict__ A, double* __restrict__ Ldst,
                                         double* __restrict__ linv, int n, int lane) {
  double g[NMAX];
  const int li = lane < n ? lane : 0;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) g[k] = (k < n) ? A[li + k * LD] : 0.0;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    if (j < n) {
      // j, k are compile-time constants (fully unrolled): pivots and column entries travel through
      // the scalar unit (readlane), not the LDS crossbar
      const double d = readlane_d(g[j], j);
      if (!(d > 0.0)) bad = true;
      const double inv = rsqrt_d(d);
      const double lij = g[j] * inv;  // lane j: d / sqrt(d) = sqrt(d)
      g[j] = lij;
      if (lane == j) linv[j] = inv;
#pragma unroll
      for (int k = j + 1; k < NMAX; ++k) {
        if (k < n) {
          const double lkj = readlane_d(lij, k);
          g[k] -= lij * lkj;
        }
      }
    }
  }
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < NMAX; ++k)
      if (k < n) Ldst[lane + k * LD] = (k <= lane) ? g[k] : 0.0;
  }
  return bad;
}

// In-wave Cholesky as wave_llt, and in the same sweep Y = L^-1 by forward substitution on the
// identity.  Lanes 0..15 carry the rows of G / L, lanes 16..31 the columns of Y (lane 16+j = column
// j): the column-j step of both is "scale entry j by 1/l_jj, subtract (entry j) x L[k][j] from
// entry k", with the same broadcast scalars L[k][j], so ONE instruction stream serves both -- the
// inverse factor costs no instructions beyond the Cholesky's own.
// Writes L / 1/diag like wave_llt and Y column-major (ld NMAX) to Ydst.  Returns true on failure.
// The same in three parts, so that a wave can run the column steps in the gaps its other work leaves (the tile-split kernel gives
// the first columns to a wave that would otherwise wait at the barrier behind P+ A): the state -- row lane's entries of G / L, or
// one column of Y -- stays in registers between the calls.
template <int NMAX>
struct LltInvState {
  double g[NMAX];
  bool bad;
};
template <int NMAX, int LD, int YOFF>
__device__ __forceinline__ void llt_inv_load(LltInvState<NMAX>& s, const double* __restrict__ A, int n, int lane) {
  // rows in lanes [0, YOFF), columns of Y in lanes [YOFF, 2*YOFF): YOFF = 16 (n <= 16) or 32 (n <= 32)
  static_assert(NMAX <= YOFF && 2 * YOFF <= 64, "rows of G and columns of Y share one wave");
  const int li = lane < n ? lane : 0;
  const bool ylane = lane >= YOFF;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) {
    const double a = (k < n) ? A[li + k * LD] : 0.0;
    s.g[k] = ylane ? ((k == lane - YOFF) ? 1.0 : 0.0) : a;
  }
  s.bad = false;
}
// KEEP_L = false: a caller that reads only Y afterwards; neither 1/diag(L) nor L is stored (linv, Ldst are not touched).
template <int NMAX, int J0, int J1, bool KEEP_L = true>
__device__ __forceinline__ void llt_inv_steps(LltInvState<NMAX>& s, double* __restrict__ linv, int n, int lane) {
#pragma unroll
  for (int j = J0; j < J1; ++j) {
    if (j < n) {
      const double d = readlane_d(s.g[j], j);
      if (!(d > 0.0)) s.bad = true;
      const double inv = rsqrt_d(d);
      const double xj = s.g[j] * inv;  // L[lane][j] | Y[j][lane-YOFF]
      s.g[j] = xj;
      if (KEEP_L && lane == j) linv[j] = inv;
#pragma unroll
      for (int k = j + 1; k < NMAX; ++k) {
        if (k < n) {
          const double lkj = readlane_d(xj, k);
          s.g[k] -= xj * lkj;
        }
      }
    }
  }
}
template <int NMAX, int LD, int YOFF, bool KEEP_L = true>
__device__ __forceinline__ bool llt_inv_store(const LltInvState<NMAX>& s, double* __restrict__ Ldst, double* __restrict__ Ydst, int n,
                                              int lane) {
  const bool ylane = lane >= YOFF;
  if (KEEP_L && lane < n) {
#pragma unroll
    for (int k = 0; k < NMAX; ++k)
      if (k < n) Ldst[lane + k * LD] = (k <= lane) ? s.g[k] : 0.0;
  } else if (ylane && lane < YOFF + NMAX) {
    const int c = lane - YOFF;
#pragma unroll
    for (int k = 0; k < NMAX; ++k) Ydst[k + c * NMAX] = (c < n && k < n) ? s.g[k] : 0.0;
  }
  return s.bad;
}
template <int NMAX, int LD, int YOFF = 16, bool KEEP_L = true>
__device__ __forceinline__ bool wave_llt_inv(const double* __restrict__ A, double* __restrict__ Ldst,
                                             double* __restrict__ linv, double* __restrict__ Ydst,
                                             int n, int lane) {
  LltInvState<NMAX> s;
  llt_inv_load<NMAX, LD, YOFF>(s, A, n, lane);
  llt_inv_steps<NMAX, 0, NMAX, KEEP_L>(s, linv, n, lane);
  return llt_inv_store<NMAX, LD, YOFF, KEEP_L>(s, Ldst, Ydst, n, lane);
}

// x <- (L L^T)^-1 x for one right-hand side held in registers (x[NMAX]); L in LDS.
template <int NMAX, int LD>
__device__ __forceinline__ void llt_solve_reg(const double* __restrict__ L,
                                              const double* __restrict__ linv, double (&x)[NMAX],
                                              int n) {
#pragma unroll
  for (int i = 0; i < NMAX; ++i) {
    if (i < n) {
      double v = x[i];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= L[i + k * LD] * x[k];
      x[i] = v * linv[i];
    }
    // keep the scheduler from hoisting the (uniform) loads of the whole factor ahead of the chain:
    // the rows are serially dependent anyway, and ~80 hoisted doubles cost 160 VGPRs
    if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = NMAX - 1; i >= 0; --i) {
    if (i < n) {
      double v = x[i];
#pragma unroll
      for (int k = i + 1; k < NMAX; ++k)
        if (k < n) v -= L[k + i * LD] * x[k];
      x[i] = v * linv[i];
    }
    if ((i & 1) == 0) __builtin_amdgcn_sched_barrier(0);
  }
}

// The same factorisation and inverse factor for 16 < n <= 32, blocked 16 + (n - 16) with the trailing update and the off-diagonal
// block of the inverse on the matrix cores.  The column steps of wave_llt_inv cost (n - j) broadcasts each -- n^2 / 2 readlane
// pairs, every one of them spilled through a VGPR lane in the register-starved tile-split kernels (19k cycles at n = 29).  Here:
//   panel     columns 0..15 of ALL n rows (lanes = rows) by the column steps, 16 - j broadcasts each: L11, L21; Y11 = L11^-1 on
//             lanes 32..47 in the same stream
//   trailing  S = G22 - L21 L21^T: 4 MFMAs, both operands the same fragment of L21
//   block 2   S = L22 L22^T by the column steps (n - 16 columns), Y22 = L22^-1 beside it
//   inverse   Y21 = -Y22 (L21 Y11): two MFMA products chained through the C layout
// Same outputs as wave_llt_inv: L (lower, zeros above) at Ldst (ld LD), 1/diag(L) at linv, Y column-major (ld NMAX) at Ydst; scr: 256
// doubles of LDS scratch.  One wave; LDS hand-offs inside it are ordered by wave_lds_fence.
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
template <int NMAX, int LD>
__device__ __forceinline__ bool wave_llt_inv_blocked(const double* __restrict__ A, double* __restrict__ Ldst, double* __restrict__ linv,
                                                     double* __restrict__ Ydst, double* __restrict__ scr, int lane) {
  static_assert(NMAX > 16 && NMAX <= 32, "two blocks");
  constexpr int n = NMAX, N2 = NMAX - 16;
  const int li = lane & 15, q = lane >> 4;
  const bool ylane = lane >= 32;
  const int yc = lane - 32;            // column of Y11 / Y22 this lane carries
  const int row = lane < n ? lane : 0;
  bool bad = false;
  // ---- panel: columns 0..15 ----
  double g[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) g[k] = ylane ? ((k == yc) ? 1.0 : 0.0) : A[row + k * LD];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double d = readlane_d(g[j], j);
    if (!(d > 0.0)) bad = true;
    const double inv = rsqrt_d(d);
    const double xj = g[j] * inv;   // L[lane][j] | Y11[j][yc]
    g[j] = xj;
    if (lane == j) linv[j] = inv;
#pragma unroll
    for (int k = j + 1; k < 16; ++k) {
      const double lkj = readlane_d(xj, k);
      g[k] -= xj * lkj;
    }
  }
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < 16; ++k) Ldst[lane + k * LD] = (k <= lane) ? g[k] : 0.0;
#pragma unroll
    for (int k = 16; k < n; ++k)
      if (lane < 16) Ldst[lane + k * LD] = 0.0;   // the block above the diagonal
  } else if (ylane && yc < 16) {
#pragma unroll
    for (int k = 0; k < 16; ++k) Ydst[k + yc * NMAX] = g[k];
#pragma unroll
    for (int k = 16; k < n; ++k) Ydst[k + yc * NMAX] = 0.0;   // placeholder of Y21 (overwritten below)
  }
  wave_lds_fence();
  // ---- trailing update on the matrix cores: S = G22 - L21 L21^T (C layout: row q + 4r, column li) ----
  {
    d4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u0 = drow(q, r), u1 = li;
      acc[r] = (u0 < N2 && u1 < N2) ? A[(16 + u0) + (16 + u1) * LD] : ((u0 == u1) ? 1.0 : 0.0);   // padding: identity
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double v = (li < N2) ? Ldst[(16 + li) + (ks * 4 + q) * LD] : 0.0;   // L21[li][4 ks + q]: A and B fragment alike
      acc = mfma16(-v, v, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) scr[drow(q, r) + li * 16] = acc[r];
  }
  wave_lds_fence();
  // ---- block 2 ----
  double h[16];
  const int row2 = lane < N2 ? lane : 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) h[k] = ylane ? ((k == yc) ? 1.0 : 0.0) : scr[row2 + k * 16];
#pragma unroll
  for (int j = 0; j < N2; ++j) {
    const double d = readlane_d(h[j], j);
    if (!(d > 0.0)) bad = true;
    const double inv = rsqrt_d(d);
    const double xj = h[j] * inv;   // L22[lane][j] | Y22[j][yc]
    h[j] = xj;
    if (lane == j) linv[16 + j] = inv;
#pragma unroll
    for (int k = j + 1; k < N2; ++k) {
      const double lkj = readlane_d(xj, k);
      h[k] -= xj * lkj;
    }
  }
  if (lane < N2) {
#pragma unroll
    for (int k = 0; k < N2; ++k) Ldst[(16 + lane) + (16 + k) * LD] = (k <= lane) ? h[k] : 0.0;
  } else if (ylane && yc < N2) {
#pragma unroll
    for (int k = 0; k < 16; ++k) Ydst[k + (16 + yc) * NMAX] = 0.0;            // Y12 = 0
#pragma unroll
    for (int k = 0; k < N2; ++k) Ydst[(16 + k) + (16 + yc) * NMAX] = h[k];   // Y22
  }
  wave_lds_fence();
  // ---- Y21 = -Y22 (L21 Y11) ----
  {
    d4 t = zero4(), y = zero4();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double a_ = (li < N2) ? Ldst[(16 + li) + (ks * 4 + q) * LD] : 0.0;   // L21[i = li][k]
      const double b_ = Ydst[(ks * 4 + q) + li * NMAX];                            // Y11[k][n = li]
      t = mfma16(a_, b_, t);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {   // k = 4 ks + q < N2 (Y22 is zero-padded by the masks)
      const int k = ks * 4 + q;
      const double a_ = (li < N2 && k < N2) ? Ydst[(16 + li) + (16 + k) * NMAX] : 0.0;   // Y22[i = li][k]
      y = mfma16(-a_, t[ks], y);   // the C layout of T (row q + 4 ks, column li) is the B fragment of k-step ks
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = drow(q, r);
      if (i < N2) Ydst[(16 + i) + li * NMAX] = y[r];
    }
  }
  wave_lds_fence();
  return bad;
}

}  // namespace rtoc
