// riccati_forward.hpp -- batched forward Riccati recursion for gfx950.
//
// Replaces RiccatiRecursion::forwardRiccatiRecursion (reference
// src/riccati/riccati_recursion.cpp:83-131) and the free functions it calls
// (src/riccati/riccati_factorizer.cpp:200-277): forwardRiccatiRecursion (x2),
// computeSwitchingTimeDirection, computeCostateDirection (x2),
// computeLagrangeMultiplierDirection.
//
// The forward pass is a chain of mat-vecs (about 0.24 flop/byte): HBM-bound, and bound by the NUMBER and width of its
// load instructions more than by its bytes.  riccati_forward_kernel (2 NV + NU <= 64): one wave per instance, lanes as
// row pairs x column groups, every matrix read with 16-byte loads (864 B per instruction for ANYmal, 32 vector-memory
// reads per grid point against the former row walk's ~87), partial sums reduced through LDS in a fixed order, Fxx of
// the next grid point in flight across the serial tail of this one.  riccati_forward_mw_kernel (iCub): several waves,
// thread t < NX owns row t of Fxx and P, threads NX..NX+NU-1 a row of K.
#pragma once
#include "device_utils.hpp"
#include "kernel_args.hpp"  // FwdArgs, FillArgs
#include "../../include/rtoc.h"

namespace rtoc {

#ifndef FWD_PREFETCH
#define FWD_PREFETCH 12  // Fxx loads of grid point st + 1 requested ahead of the tail of st (all of them for ANYmal)
#endif
#ifndef FWD_WAVES_PER_SIMD
// 2: a register budget of 256 VGPRs.  ANYmal takes 218 (no scratch), so eight waves per CU; the 7:7:x and 12:6:6 shapes
// take 118-120 and still run sixteen.  Capped at 128, ANYmal spills 58-84 VGPRs whatever the prefetch depth (0, 6, 12).
#define FWD_WAVES_PER_SIMD 2
#endif

template <int NV, int NU>
struct FwdPairCfg {
  static constexpr int NX = 2 * NV;
  static constexpr int G = 64 / NV;               // column groups: lane l = c * NV + p, l < G * NV
  static constexpr int TX = (NX + G - 1) / G;     // 16-B loads per NX x NX matrix (Fxx, P): column G t + c in load t
  static constexpr int TXP = (TX + 1) & ~1;       // row of the permuted dx copy, a whole number of 16-B reads
  static constexpr int TK = (NU + G - 1) / G;     // 16-B loads of K (row u = G t + c in load t)
  static constexpr int NVP = (NV + 1) & ~1;       // row of the K partials
  static constexpr int NF = NV * NU, NFP = (NF + 1) & ~1;
  static constexpr int TF = (NFP + 127) / 128;    // 16-B loads of Fvu, a flat copy (an odd NF reads one double of padding)
};

// Hand-over of dx / du / dts between the threads of an instance goes through LDS only: one wavefront needs no barrier
// at all (its LDS operations complete in order), several need s_barrier behind their own LDS traffic -- and neither
// needs the s_waitcnt vmcnt(0) that __syncthreads() puts in front of it, which would drain the loads in flight.
template <int NWF>
__device__ __forceinline__ void fwd_sync() {
  if constexpr (NWF == 1)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One wave per instance (2 NV + NU <= 64).  Lane l = c * NV + p (l < G * NV, G = floor(64 / NV)) owns row pair p and
// column group c: in load t it reads rows 2p, 2p+1 of column G t + c -- 16 contiguous, aligned bytes, since the leading
// dimension NX = 2 NV is even and fields are 64-B aligned -- so ONE global_load_dwordx4 covers G whole columns (ANYmal:
// 3 columns = 864 B on 54 lanes).  Fxx and P take ceil(NX / G) loads each, K (row-major = K^T column-major, the same
// map with u = G t + c) ceil(NU / G), Fvu a flat copy of ceil(NV NU / 128) loads into LDS; ANYmal: 12 + 12 + 4 + 2 + 2
// vector loads per grid point against the row walk's ~87.  The lane's operands dx[G t + c] are one ds_read_b128 per two
// loads from a permuted copy of dx in LDS.  Partial sums go through LDS and are reduced in a fixed order (over c for
// Fxx dx and P dx, over p for K dx), so results repeat bit for bit.  The Fxx loads of grid point st + 1 are issued
// before the tail of st (K dx -> du -> Fvu du -> dx+): all instances reach that tail together, and without requests in
// flight across it the memory system idles once per grid point.  Lanes past G * NV repeat group 0's addresses and drop
// their sums; a column or K row past the matrix is clamped to a live one and its product is not accumulated.
// P of a grid point i < N is taken as symmetric (every backward kernel stores it so) and read from its lower triangle: the
// same 12 load instructions, but a lane whose row pair lies wholly above the diagonal makes no request (ANYmal: 342 of
// 648 pairs, 5,472 of 10,368 B), and the missing products come from the mirror terms of the live pairs (see pe below).
// The terminal P_N is a copy of the caller's Qxx_N and is read in full.
template <int NV, int NU, int NS>
__global__ __launch_bounds__(64, FWD_WAVES_PER_SIMD) void riccati_forward_kernel(FwdArgs a) {
  using C = FwdPairCfg<NV, NU>;
  constexpr int NX = C::NX, G = C::G, TX = C::TX, TXP = C::TXP, TK = C::TK, NVP = C::NVP, NF = C::NF, TF = C::TF;
  constexpr int PF = FWD_PREFETCH < TX ? FWD_PREFETCH : TX;  // Fxx loads of grid point st + 1 issued ahead of the tail of st
  static_assert(NX + NU <= 64, "one lane per row of [Fxx; K] in the reductions");
  __shared__ __attribute__((aligned(16))) double sDx[2][NX + 8];   // dx in natural order
  __shared__ __attribute__((aligned(16))) double sXp[2][G * TXP];  // dx permuted: [c][t] = dx[G t + c], 0 past NX
  // partial sums; the last row of each takes the sums that are dropped, so that every lane writes (a branch around the
  // writes lets the compiler sink the products, and with them every register the loads landed in, into it)
  __shared__ __attribute__((aligned(16))) double sPa[G + 1][NX];    // Fxx dx, partial over column group c
  __shared__ __attribute__((aligned(16))) double sPp[G + 1][NX];    // P dx, the same
  // partials over row pair p, one row per lane of the reduction: rows [0, NX) the mirror terms of P dx (below), rows
  // [NX, NX + NU) K dx, the last row what is dropped
  __shared__ __attribute__((aligned(16))) double sPk[NX + NU + 1][NVP];
  __shared__ __attribute__((aligned(16))) double sF[TF * 128];      // Fvu of the grid point, column-major
  __shared__ double sDu[NU + 8];
  __shared__ double sDt[NX];  // dtsdx of an impact grid point with sto_next, requested ahead like the other riders
  __shared__ double sRed[8];
  extern __shared__ int sGridTab[];  // [nstages] (dynamic): type | sto << 4 | sto_next << 5 | switching_constraint << 6 | dims << 8
  const int tid = threadIdx.x;
  const int b = a.first + blockIdx.x;
  if (b >= a.batch) return;
  for (int st = tid; st < a.nstages; st += 64) {
    const rtoc_grid* gp = a.grid + st;
    sGridTab[st] = (gp->type & 15) | ((gp->sto != 0) << 4) | ((gp->sto_next != 0) << 5) |
                   ((gp->switching_constraint != 0) << 6) | (gp->dims << 8);
  }
  for (int e = tid; e < 2 * G * TXP; e += 64) (&sXp[0][0])[e] = 0.0;
  const int N = a.nstages - 1;
  constexpr rtoc_layout SL = StaticLayout<NV, NU, NS>::make();
  constexpr rtoc_record_layout KL = SL.kkt, RL = SL.ric, DL = SL.dir;
  const double* kb = a.kkt + (size_t)b * a.nstages * KL.stride;
  const double* rb = a.ric + (size_t)b * a.nstages * RL.stride;
  double* db = a.dir + (size_t)b * a.nstages * DL.stride;

  // lane roles: (p, c) in the loads and partial sums; row tid < NX, row NX + u of K in the reductions and the outputs
  const bool lg = tid < G * NV;
  const int p = lg ? tid % NV : tid - G * NV;
  const int c = lg ? tid / NV : 0;
  const int cw = lg ? c : G;  // row of sPa / sPp this lane writes
  const bool xrow = tid < NX;
  const int r = xrow ? tid : NX - 1;
  const bool kl = tid >= NX && tid < NX + NU;
  const int u = kl ? tid - NX : 0;
  const int pos = (r % G) * TXP + r / G;  // place of dx[r] in the permuted copy
  __syncthreads();
  if (xrow) {
    const double v = a.dx0 ? a.dx0[(size_t)b * NX + tid] : db[DL.off[RTOC_DIR_DX] + tid];
    sDx[0][tid] = v;
    sXp[0][pos] = v;
    if (a.dx0) db[DL.off[RTOC_DIR_DX] + tid] = v;
  }
  __syncthreads();
  double dts = 0.0, dtsn = 0.0;  // d[i].dts, d[i].dts_next carried along (uniform)
  {
    const rtoc_grid g0 = a.grid[0];
    if (g0.sto) {
      // computeSwitchingTimeDirection(sto_policy_[0], d[0], false)  (riccati_recursion.cpp:91-94)
      if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < NX; ++k) acc += rb[RL.off[RTOC_RIC_DTSDX] + k] * sDx[0][k];
        sRed[0] = acc + rb[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
      }
      __syncthreads();
      dtsn = sRed[0];
      __syncthreads();
    }
  }
  // offset of the lane's 16 bytes in load t of an NX x NX matrix (Fxx, P) and of K, and whether its product counts.  Only
  // the last load of a matrix whose order G does not divide can run past it; it is clamped into the matrix, and the
  // other addresses stay lane base + t x immediate.
  const int lo = c * NX + 2 * p;
  auto moff = [&](int t) { return (NX % G == 0 || t < TX - 1 || G * t + c < NX) ? lo + t * (G * NX) : (NX - 1) * NX + 2 * p; };
  auto live = [&](int t) { return NX % G == 0 || t < TX - 1 || G * t + c < NX; };
  auto koff = [&](int t) { return (NU % G == 0 || t < TK - 1 || G * t + c < NU) ? lo + t * (G * NX) : (NU - 1) * NX + 2 * p; };
  auto klive = [&](int t) { return NU % G == 0 || t < TK - 1 || G * t + c < NU; };
  // P of a grid point i < N is symmetric as every backward kernel stores it, and only its lower triangle is requested: the
  // lane's pair in load t is live iff it reaches the diagonal, 2p + 1 >= j with j = G t + c (ANYmal: 342 of 648 pairs).  With
  // dd = j - 2p the pair gives P[2p][j] x[j] (dd <= 0) and P[2p+1][j] x[j] (dd <= 1) to its own rows and the mirror terms
  // P[2p][j] x[2p] (dd < 0) + P[2p+1][j] x[2p+1] (dd < 1) to row j, a partial over p reduced like K dx.  Every term is
  // selected, never multiplied by a mask: the upper element of a pair astride the diagonal is data this kernel does not read.
  // The loads are raw buffer loads through one descriptor over the instance's records: a silent lane's offset lies past
  // num_records, so the range check drops its request (no fetch, no branch, no wait between the loads) and returns zero.
  // Lanes past G NV are silent; a column past the matrix cannot be live (2p + 1 < NX).
  const int pe = lg ? c - 2 * p : (1 << 20);
  constexpr unsigned P_SILENT = 0x80000000u;
  const auto prsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(rb), 0, a.nstages * (int)RL.stride * 8, 0x00020000);
  // row of sPk a lane sums: its own row of P dx's mirror terms, its row of K dx, or the dropped one
  const int prow = tid < NX + NU ? tid : NX + NU;
  // Fx[r] | k[u] and s[r]: one 8-B load each
  auto vec_ptr = [&](int st) {
    return xrow ? kb + (size_t)st * KL.stride + KL.off[RTOC_KKT_FX] + tid : rb + (size_t)st * RL.stride + RL.off[RTOC_RIC_KV] + u;
  };
  auto s_ptr = [&](int st) { return rb + (size_t)st * RL.stride + RL.off[RTOC_RIC_S] + r; };
  d2 fa[TX];
  double vec, sv;
#pragma unroll
  for (int t = 0; t < PF; ++t) fa[t] = *(const d2*)(kb + KL.off[RTOC_KKT_FXX] + moff(t));
  vec = *vec_ptr(0);
  sv = *s_ptr(0);
  int cur = 0;
  struct GridBits { int type, sto, sto_next, switching_constraint, dims; };
  for (int st = 0; st < N; ++st) {
    // grid descriptor from the LDS table: a global read here waits, on gfx9's single vector-memory counter, for the
    // acknowledgement of the previous stage's stores as well -- a write round trip per stage with nothing else in flight
    const int gb = __builtin_amdgcn_readfirstlane(sGridTab[st]);
    const GridBits g = {gb & 15, (gb >> 4) & 1, (gb >> 5) & 1, (gb >> 6) & 1, gb >> 8};
    const bool impact = g.type == RTOC_GRID_IMPACT, lift = g.type == RTOC_GRID_LIFT;
    const bool sto = g.sto != 0, sto_next = g.sto_next != 0;
    const double* kr = kb + (size_t)st * KL.stride;
    const double* rr = rb + (size_t)st * RL.stride;
    double* dr = db + (size_t)st * DL.stride;
    const double* dx = sDx[cur];
    const double* xp = sXp[cur];

    if (impact || lift) {
      dts = dtsn;  // d[i].dts = d[i-1].dts_next
      dtsn = 0.0;
      if (lift && sto_next) {
        if (tid == 0) {
          double acc = 0.0;
          #pragma unroll 4
          for (int k = 0; k < NX; ++k) acc += rr[RL.off[RTOC_RIC_DTSDX] + k] * dx[k];
          acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
          if (sto) acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTSDTS] * dts;
          sRed[0] = acc;
        }
        fwd_sync<1>();
        dtsn = sRed[0];
        fwd_sync<1>();
      }
    }

    // ---- the requests of this grid point not made ahead: the rest of Fxx, K, Fvu (read on impact grid points too, and
    //      dropped), P ----
    d2 fk[TK], ff[TF], fp[TX];
#pragma unroll
    for (int t = PF; t < TX; ++t) fa[t] = *(const d2*)(kr + KL.off[RTOC_KKT_FXX] + moff(t));
#pragma unroll
    for (int t = 0; t < TK; ++t) fk[t] = *(const d2*)(rr + RL.off[RTOC_RIC_K] + koff(t));
#pragma unroll
    for (int i = 0; i < TF; ++i) {
      const int e = 2 * (64 * i + tid);
      ff[i] = *(const d2*)(kr + KL.off[RTOC_KKT_FVU] + (e < NF ? e : 0));
    }
    // the STO riders (T | Ffx, W | Psi, Phi) and the dtsdx of an impact grid point: requested here, AHEAD of the Fxx loads of
    // st + 1, since gfx9 has one vector-memory counter: a load issued behind the prefetch waits for all of it
    double rd1 = 0.0, rd2 = 0.0, rd3 = 0.0, rdt = 0.0, rs0 = 0.0, rss = 0.0;
    if (sto) {
      rd1 = xrow ? kr[KL.off[RTOC_KKT_FFX] + tid] : rr[RL.off[RTOC_RIC_T] + u];
      rd2 = xrow ? rr[RL.off[RTOC_RIC_PSI] + tid] : rr[RL.off[RTOC_RIC_W] + u];
      rd3 = rr[RL.off[RTOC_RIC_PHI] + r];
    }
    if (impact && sto_next) {
      rdt = rr[RL.off[RTOC_RIC_DTSDX] + r];
      rs0 = rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
      rss = rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTSDTS];
    }
    d2 x[TXP / 2];
#pragma unroll
    for (int i = 0; i < TXP / 2; ++i) x[i] = *(const d2*)(xp + c * TXP + 2 * i);
    const d2 xq = *(const d2*)(dx + 2 * p);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int t = 0; t < TX; ++t) {
      const double xt = x[t / 2][t % 2];
      if (live(t)) {
        a0 += fa[t].x * xt;
        a1 += fa[t].y * xt;
      }
    }
    // P is requested only once Fxx has been consumed: this bounds the registers the loads of a grid point hold at once
    // (the scheduler otherwise hoists every load of the stage to its top)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < TX; ++t) {
      const unsigned vo = (pe + G * t <= 1) ? (unsigned)(lo + t * (G * NX)) * 8u : P_SILENT;
      fp[t] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(prsrc, vo, (unsigned)(st * (int)RL.stride + (int)RL.off[RTOC_RIC_P]) * 8u, 0));
    }
    double pk[TK];
#pragma unroll
    for (int t = 0; t < TK; ++t) pk[t] = fk[t].x * xq.x + fk[t].y * xq.y;
#pragma unroll
    for (int i = 0; i < TF; ++i) *(d2*)(sF + 2 * (64 * i + tid)) = ff[i];
    double q0 = 0.0, q1 = 0.0;
#pragma unroll
    for (int t = 0; t < TX; ++t) {
      const double xt = x[t / 2][t % 2];
      const int dd = pe + G * t;
      const double o0 = q0 + fp[t].x * xt, o1 = q1 + fp[t].y * xt;
      q0 = dd <= 0 ? o0 : q0;
      q1 = dd <= 1 ? o1 : q1;
      const double m1 = fp[t].y * xq.y, m01 = m1 + fp[t].x * xq.x;
      // (every lane writes its entry, zero where it has no mirror term: each [row][p] is written once per grid point; the
      // readers of the previous grid point are past the fwd_sync that ended it)
      sPk[lg && live(t) ? G * t + c : NX + NU][p] = dd < 0 ? m01 : (dd < 1 ? m1 : 0.0);
    }
    // ---- the Fxx loads and the two vectors of grid point st + 1, in flight across the tail of this one
    //      (st + 1 <= N: the terminal records exist, what is read there is dropped) ----
    double vec_n, sv_n;
    __builtin_amdgcn_sched_barrier(0);
    {
      const double* kn = kb + (size_t)(st + 1) * KL.stride;
#pragma unroll
      for (int t = 0; t < PF; ++t) fa[t] = *(const d2*)(kn + KL.off[RTOC_KKT_FXX] + moff(t));
      vec_n = *vec_ptr(st + 1);
      sv_n = *s_ptr(st + 1);
    }
    // ---- partial sums -> LDS -> row sums, in a fixed order ----
    {
      d2 va = {a0, a1}, vp = {q0, q1};
      *(d2*)(&sPa[cw][2 * p]) = va;
      *(d2*)(&sPp[cw][2 * p]) = vp;
#pragma unroll
      for (int t = 0; t < TK; ++t) sPk[lg && klive(t) ? NX + G * t + c : NX + NU][p] = pk[t];
    }
    fwd_sync<1>();
    double acc_a = sPa[0][r], acc_p = sPp[0][r];
#pragma unroll
    for (int cc = 1; cc < G; ++cc) {
      acc_a += sPa[cc][r];
      acc_p += sPp[cc][r];
    }
    double kd = 0.0;   // lanes [NX, NX + NU): K dx; lanes [0, NX): the mirror terms of P dx
#pragma unroll 3
    for (int i = 0; i < NVP / 2; ++i) {
      const d2 w = *(const d2*)(&sPk[prow][2 * i]);
      kd += w.x;
      if (2 * i + 1 < NV) kd += w.y;
    }
    acc_p += xrow ? kd : 0.0;
    if (kl && !impact) {
      double du = kd + vec;
      if (sto) {
        du += rd1 * (dtsn - dts);
        if (sto_next) du -= rd2 * dtsn;
      }
      sDu[u] = du;
      dr[DL.off[RTOC_DIR_DU] + u] = du;
    }
    fwd_sync<1>();
    double* dxn = sDx[cur ^ 1];
    if (xrow) {
      double v = vec + acc_a;
      if (!impact) {
        if (tid >= NV) {
#pragma unroll 4
          for (int cc = 0; cc < NU; ++cc) v += sF[cc * NV + tid - NV] * sDu[cc];
        }
        if (sto) v += rd1 * (dtsn - dts);
      }
      dxn[tid] = v;
      if (impact && sto_next) sDt[tid] = rdt;
      sXp[cur ^ 1][pos] = v;
      (dr + DL.stride)[DL.off[RTOC_DIR_DX] + tid] = v;
    }
    if (impact && sto_next) {
      // riccati_recursion.cpp:101-107: dts_next of d[i+1] from sto_policy_[i] and dx[i+1]
      fwd_sync<1>();
      if (tid == 0) {
        double acc = 0.0;
        #pragma unroll 4
        for (int k = 0; k < NX; ++k) acc += sDt[k] * dxn[k];
        acc += rs0;
        if (sto) acc += rss * dts;
        sRed[0] = acc;
      }
      fwd_sync<1>();
      dtsn = sRed[0];
    }
    // ---- costate (riccati_factorizer.cpp:243-262) ----
    if (xrow) {
      double lam = acc_p - sv;
      if (sto) {
        if (impact) {
          lam -= rd3 * dtsn;
        } else {
          lam += rd2 * (dtsn - dts);
          if (sto_next) lam -= rd3 * dtsn;
        }
      }
      dr[DL.off[RTOC_DIR_DLMDGMM] + tid] = lam;
    }
    // ---- switching-constraint multiplier (:265-277): two grid points of a trot, a plain row walk (its loads, like those of
    //      the dtsdx walk of a lift grid point with sto_next, wait for the prefetch: rare grid points) ----
    if (NS > 0 && g.switching_constraint && tid < g.dims) {
      const double* M = rr + RL.off[RTOC_RIC_M] + tid;
      double acc = 0.0;
      #pragma unroll 4
      for (int j = 0; j < NX; ++j) acc += M[j * NS] * dx[j];
      acc += rr[RL.off[RTOC_RIC_MV] + tid];
      if (sto) {
        acc += rr[RL.off[RTOC_RIC_MT] + tid] * (dtsn - dts);
        if (sto_next) acc -= rr[RL.off[RTOC_RIC_MTN] + tid] * dtsn;
      }
      dr[DL.off[RTOC_DIR_DXI] + tid] = acc;
    }
    if (tid == 0) {
      dr[DL.off[RTOC_DIR_DTS] + 0] = dts;
      dr[DL.off[RTOC_DIR_DTS] + 1] = dtsn;
    }
    fwd_sync<1>();
    cur ^= 1;
    vec = vec_n;
    sv = sv_n;
  }
  // terminal costate (riccati_recursion.cpp:128-130): P dx - s with the same map (the Fxx / Fx requested ahead are dropped)
  {
    const double* rr = rb + (size_t)N * RL.stride;
    double* dr = db + (size_t)N * DL.stride;
    const double* xp = sXp[cur];
    d2 fp[TX], x[TXP / 2];
#pragma unroll
    for (int t = 0; t < TX; ++t) fp[t] = *(const d2*)(rr + RL.off[RTOC_RIC_P] + moff(t));
#pragma unroll
    for (int i = 0; i < TXP / 2; ++i) x[i] = *(const d2*)(xp + c * TXP + 2 * i);
    double q0 = 0.0, q1 = 0.0;
#pragma unroll
    for (int t = 0; t < TX; ++t) {
      const double xt = x[t / 2][t % 2];
      if (live(t)) {
        q0 += fp[t].x * xt;
        q1 += fp[t].y * xt;
      }
    }
    {
      d2 vp = {q0, q1};
      *(d2*)(&sPp[cw][2 * p]) = vp;
    }
    fwd_sync<1>();
    double acc_p = sPp[0][r];
#pragma unroll
    for (int cc = 1; cc < G; ++cc) acc_p += sPp[cc][r];
    if (xrow) dr[DL.off[RTOC_DIR_DLMDGMM] + tid] = acc_p - sv;
    if (tid == 0) {
      dr[DL.off[RTOC_DIR_DTS] + 0] = dts;
      dr[DL.off[RTOC_DIR_DTS] + 1] = dtsn;
    }
  }
}

// Instances whose rows need more than one wavefront (NX + NU > 64: iCub): the plain form -- thread t < NX owns row t of
// Fxx and P, threads NX..NX+NU-1 a row of K, hardware barriers between the phases.  The single-wave kernel above relies on
// the in-order LDS of ONE wave for its hand-overs and on its roles sharing a wave's load instructions; with two waves the
// same structure measured slower than this one (iCub nv = 32: 1.51 vs 0.77 ms per 1024 x 35 stages), so it is kept.
template <int NV, int NU, int NS, int NWF>
__global__ __launch_bounds__(64 * NWF) void riccati_forward_mw_kernel(FwdArgs a) {
  constexpr int NX = 2 * NV, NT = 64 * NWF;
  static_assert(NX + NU <= NT, "one thread per row of [Fxx;K]");
  __shared__ double sDx[2][NX + 8];
  __shared__ double sDu[NU + 8];
  __shared__ double sRed[8];
  const int tid = threadIdx.x;
  const int b = a.first + blockIdx.x;
  if (b >= a.batch) return;
  const int N = a.nstages - 1;
  constexpr rtoc_layout SL = StaticLayout<NV, NU, NS>::make();
  constexpr rtoc_record_layout KL = SL.kkt, RL = SL.ric, DL = SL.dir;
  const double* kb = a.kkt + (size_t)b * a.nstages * KL.stride;
  const double* rb = a.ric + (size_t)b * a.nstages * RL.stride;
  double* db = a.dir + (size_t)b * a.nstages * DL.stride;

  if (tid < NX) {
    const double v = a.dx0 ? a.dx0[(size_t)b * NX + tid] : db[DL.off[RTOC_DIR_DX] + tid];
    sDx[0][tid] = v;
    if (a.dx0) db[DL.off[RTOC_DIR_DX] + tid] = v;
  }
  __syncthreads();
  double dts = 0.0, dtsn = 0.0;  // d[i].dts, d[i].dts_next carried along (uniform)
  {
    const rtoc_grid g0 = a.grid[0];
    if (g0.sto) {
      // computeSwitchingTimeDirection(sto_policy_[0], d[0], false)  (riccati_recursion.cpp:91-94)
      if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < NX; ++k) acc += rb[RL.off[RTOC_RIC_DTSDX] + k] * sDx[0][k];
        sRed[0] = acc + rb[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
      }
      __syncthreads();
      dtsn = sRed[0];
      __syncthreads();
    }
  }
  int cur = 0;
  for (int st = 0; st < N; ++st) {
    const rtoc_grid g = a.grid[st];
    const bool impact = g.type == RTOC_GRID_IMPACT, lift = g.type == RTOC_GRID_LIFT;
    const bool sto = g.sto != 0, sto_next = g.sto_next != 0;
    const double* kr = kb + (size_t)st * KL.stride;
    const double* rr = rb + (size_t)st * RL.stride;
    double* dr = db + (size_t)st * DL.stride;
    const double* dx = sDx[cur];
    double* dxn = sDx[cur ^ 1];

    if (impact || lift) {
      dts = dtsn;  // d[i].dts = d[i-1].dts_next
      dtsn = 0.0;
      if (lift && sto_next) {
        if (tid == 0) {
          double acc = 0.0;
          for (int k = 0; k < NX; ++k) acc += rr[RL.off[RTOC_RIC_DTSDX] + k] * dx[k];
          acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
          if (sto) acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTSDTS] * dts;
          sRed[0] = acc;
        }
        __syncthreads();
        dtsn = sRed[0];
        __syncthreads();
      }
    }

    // ---- row products: threads < NX: Fxx dx and P dx ; threads NX..NX+NU-1: K dx ----
    double acc_a = 0.0, acc_p = 0.0;
    if (tid < NX) {
      const double* A = kr + KL.off[RTOC_KKT_FXX] + tid;
      const double* P = rr + RL.off[RTOC_RIC_P] + tid;
#pragma unroll 18
      for (int j = 0; j < NX; ++j) {
        const double x = dx[j];
        acc_a += A[j * NX] * x;
        acc_p += P[j * NX] * x;
      }
    } else if (!impact && tid < NX + NU) {
      const int u = tid - NX;
      const double* K = rr + RL.off[RTOC_RIC_K] + (size_t)u * NX;  // row u of row-major K
#pragma unroll 6
      for (int j = 0; j < NX; ++j) acc_a += K[j] * dx[j];
      double du = acc_a + rr[RL.off[RTOC_RIC_KV] + u];
      if (sto) {
        du += rr[RL.off[RTOC_RIC_T] + u] * (dtsn - dts);
        if (sto_next) du -= rr[RL.off[RTOC_RIC_W] + u] * dtsn;
      }
      sDu[u] = du;
      dr[DL.off[RTOC_DIR_DU] + u] = du;
    }
    __syncthreads();
    if (tid < NX) {
      double v = kr[KL.off[RTOC_KKT_FX] + tid] + acc_a;
      if (!impact) {
        if (tid >= NV) {
          const double* Bv = kr + KL.off[RTOC_KKT_FVU] + (tid - NV);
#pragma unroll 4
          for (int u = 0; u < NU; ++u) v += Bv[u * NV] * sDu[u];
        }
        if (sto) v += kr[KL.off[RTOC_KKT_FFX] + tid] * (dtsn - dts);
      }
      dxn[tid] = v;
      (dr + DL.stride)[DL.off[RTOC_DIR_DX] + tid] = v;
    }
    if (impact && sto_next) {
      // riccati_recursion.cpp:101-107: dts_next of d[i+1] from sto_policy_[i] and dx[i+1]
      __syncthreads();
      if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < NX; ++k) acc += rr[RL.off[RTOC_RIC_DTSDX] + k] * dxn[k];
        acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTS0];
        if (sto) acc += rr[RL.off[RTOC_RIC_SCAL] + RTOC_RIC_SCAL_DTSDTS] * dts;
        sRed[0] = acc;
      }
      __syncthreads();
      dtsn = sRed[0];
    }
    // ---- costate (riccati_factorizer.cpp:243-262) ----
    if (tid < NX) {
      double lam = acc_p - rr[RL.off[RTOC_RIC_S] + tid];
      if (sto) {
        if (impact) {
          lam -= rr[RL.off[RTOC_RIC_PHI] + tid] * dtsn;
        } else {
          lam += rr[RL.off[RTOC_RIC_PSI] + tid] * (dtsn - dts);
          if (sto_next) lam -= rr[RL.off[RTOC_RIC_PHI] + tid] * dtsn;
        }
      }
      dr[DL.off[RTOC_DIR_DLMDGMM] + tid] = lam;
    }
    // ---- switching-constraint multiplier (:265-277) ----
    if (NS > 0 && g.switching_constraint && tid < g.dims) {
      const double* M = rr + RL.off[RTOC_RIC_M] + tid;
      double acc = 0.0;
      for (int j = 0; j < NX; ++j) acc += M[j * NS] * dx[j];
      acc += rr[RL.off[RTOC_RIC_MV] + tid];
      if (sto) {
        acc += rr[RL.off[RTOC_RIC_MT] + tid] * (dtsn - dts);
        if (sto_next) acc -= rr[RL.off[RTOC_RIC_MTN] + tid] * dtsn;
      }
      dr[DL.off[RTOC_DIR_DXI] + tid] = acc;
    }
    if (tid == 0) {
      dr[DL.off[RTOC_DIR_DTS] + 0] = dts;
      dr[DL.off[RTOC_DIR_DTS] + 1] = dtsn;
    }
    __syncthreads();
    cur ^= 1;
  }
  // terminal costate (riccati_recursion.cpp:128-130)
  {
    const double* rr = rb + (size_t)N * RL.stride;
    double* dr = db + (size_t)N * DL.stride;
    const double* dx = sDx[cur];
    if (tid < NX) {
      const double* P = rr + RL.off[RTOC_RIC_P] + tid;
      double acc = 0.0;
#pragma unroll 6
      for (int j = 0; j < NX; ++j) acc += P[j * NX] * dx[j];
      dr[DL.off[RTOC_DIR_DLMDGMM] + tid] = acc - rr[RL.off[RTOC_RIC_S] + tid];
    }
    if (tid == 0) {
      dr[DL.off[RTOC_DIR_DTS] + 0] = dts;
      dr[DL.off[RTOC_DIR_DTS] + 1] = dtsn;
    }
  }
}

// Unconstrained (fixed-base, no contact) OCPs reuse the general kernels: the structured
// A = [[I, dt I],[0, I]], Bv = dt I of unconstr_backward_riccati_recursion_factorizer.cpp:27-50
// are materialised once into the Fxx / Fvu slots of every record.
template <int NV>
__global__ void unconstr_fill_kernel(FillArgs a) {
  constexpr int NX = 2 * NV;
  const int rec = blockIdx.x;  // instance*nstages + stage
  if (rec >= a.batch * a.nstages) return;
  double* r = a.kkt + (size_t)rec * a.kl.stride;
  double* A = r + a.kl.off[RTOC_KKT_FXX];
  double* Bv = r + a.kl.off[RTOC_KKT_FVU];
  for (int e = threadIdx.x; e < NX * NX; e += blockDim.x) {
    const int i = e % NX, j = e / NX;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < NV && j == i + NV) v = a.dt;
    A[e] = v;
  }
  for (int e = threadIdx.x; e < NV * NV; e += blockDim.x) {
    const int i = e % NV, j = e / NV;
    Bv[e] = (i == j) ? a.dt : 0.0;
  }
}

}  // namespace rtoc
