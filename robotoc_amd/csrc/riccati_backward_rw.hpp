// riccati_backward_rw.hpp -- register-resident backward Riccati recursion of the iCub-size shapes (nx = 64 / 70): ONE wavefront
// per OCP instance with the whole 512-entry register file of its SIMD (VGPR + AGPR, one wave per SIMD, four instances per CU).
//
// Same recursion and HBM record contract as riccati_backward.hpp (reference: src/riccati/riccati_recursion.cpp:32-80,
// riccati_factorizer.cpp:44-56,178-197, backward_riccati_recursion_factorizer.cpp:31-91); the machine mapping is the one of
// riccati_backward_rv.hpp carried to T = 4 / 5 state tiles, where the stacked operand [P+; PB^T] no longer fills its tiles and
// no state column is free for the riders:
//
//   * P+ lives in T x T accumulator tiles in the f64 MFMA C layout (lane (li, q), register r <-> row q + 4r, column li);
//     for a symmetric matrix that layout IS the A fragment (and the B fragment) of the products P+ [.]: no LDS copy of P+.
//   * Fxx is taken in its STRUCTURED form (src/dynamics/state_equation.cpp:52-55,80-82, checked on the device by
//     fxx_structure_kernel before the kernel is chosen): rows [NP, NV) are a e_k^T | c e_k^T.  Only the k groups that hold a
//     dense row -- the NP corner rows and the NV velocity rows -- are staged in LDS (21.5 of 32 KB at nv = 32: that is what
//     lets FOUR instances share a CU) and multiplied on the matrix cores; the structured rows are scaled copies of P+ / W tiles
//     in place, TS tiles and LS lanes (rows) away (NV = 16 TS + LS; nv = 32: LS = 0).
//   * PB = P+[:, v] Bv stays in accumulators: as B fragment of G = Quu + Bv^T PB[v, :] and of H = A^T PB, and its idle column NU
//     carries z = s+ - P+ Fx through both: column NU of G is Bv^T z_v (-> lu'), column NU of H is A^T z (-> s).
//   * H^T = Qxu^T + PB^T A is formed DIRECTLY in the layout Z^T = Y H^T reads (rows = controls): PB's C tiles are the A operand as they
//     stand, A's LDS fragments the B operand, the structured rows of A synthesised fragments; no transposes (riccati_rw_hrow.inc).
//   * LLT(G), Y = L^-1 by wave_llt_inv_blocked (16 + (NU - 16) columns, trailing update on the matrix cores);
//     K = -Y^T Z^T tile by tile to HBM; F = Qxx - Z Z^T + A^T (P+ A) column tile by column tile; P = sym(F).
//   * z, A^T z, lu', t = Y lu', k = -Y^T t and s = A^T z - lx + Z t are vectors in LDS / per-lane partial sums with a q-reduction
//     (no free column for riders at nx = 64).
//   * Record traffic: the dense k groups of A, the strip Fx | lx | lu, Quu and Qxx (in column panels) by LDS-DMA; Bv and Qxu^T by
//     per-lane loads straight into operand registers.
//
// Scope (plan_backward, rt_sweep.hip): grids without switching-time optimisation; switching-constraint grid points are single
// launches of the tile-split kernel (its one-stage mode), P+ / s+ handed over through the Riccati records -- the host cuts the
// horizon into segments [seg_hi .. seg_lo]; structured Fxx; RTOC_OPT_WRITEBACK_KKT = 0.  tests/rw_lane_model.py states the lane
// algebra in numpy against the oracle (tests/test_rw_lane_model.py).
//
// The two-wave form riccati_backward_rw2.hpp runs the same lane algebra, and there is ONE copy of it: the helpers of RwLanes below, and
// the blocks that work on the register tiles or issue DMA as textual fragments riccati_rw_*.inc (scope, vload, dma, z, g, hrow,
// column, end), which both kernels include; each names in its head what it expects in scope and by what the two sites differ.
#pragma once
#include "riccati_backward_rv.hpp"

namespace rtoc {

template <int NV, int NU>
struct RwCfg {
  static constexpr int NX = 2 * NV, NP = NV - NU;
  static constexpr int T = (NX + 15) / 16, TU = (NU + 15) / 16;
  static constexpr int KG = (NX + 3) / 4, KGU = (NU + 3) / 4;
  static constexpr int G0 = NV / 4;                 // first aligned k group that meets the velocity rows [NV, NX)
  static constexpr int G1 = (NP + 3) / 4;           // k groups [0, G1) meet the corner rows [0, NP)
  static constexpr int NDG = G1 + KG - G0;          // k groups with a dense row of A (staged in LDS)
  static constexpr int NUC = NU - 16 * (TU - 1);    // lane of the rider column NU in the last control tile
  static constexpr int TS = NV / 16, LS = NV % 16, QS = LS % 4, RS = LS / 4;
  static constexpr int LDA = lds_ld(4 * NDG), HL = LDA / 2;
  // T = 4 only: at T = 5 (nx = 70) P+ and F alone are 40 tiles = 320 registers and the compiler spills 540 of them -- measured 6.7 ms
  // per 1024 against the tile-split kernel's 4.8; the code below is written for general T (tests/rw_lane_model.py checks the lane
  // algebra of both shapes); T = 5 runs the two-wave form, riccati_backward_rw2.hpp
  static constexpr bool SHAPE_OK = (TU == 2) && (NU > 16) && (NU < 32) && (NP > 0) && (G1 < G0) && (NX % 2 == 0) && (NUC > 0) && (NUC < 16);
  static constexpr bool OK = (T == 4) && SHAPE_OK;    // one wave per instance (this file)
  static constexpr bool OK2 = (T == 5) && SHAPE_OK;   // two waves per instance (riccati_backward_rw2.hpp)
  static constexpr int cg(int g) { return g < G1 ? g : g - G0 + G1; }   // compact index of the dense k group g
  static constexpr int pad8(int n) { return (n + 7) & ~7; }
  static constexpr int SCR_LD = 17, SCR_TILE = pad8(16 * SCR_LD);
};

template <int NV, int NU, int NS>
struct RwLds {
  using C = RwCfg<NV, NU>;
  static constexpr rtoc_layout SL = StaticLayout<NV, NU, NS>::make();
  static constexpr int VOFF_LX = SL.kkt.off[RTOC_KKT_LX] - SL.kkt.off[RTOC_KKT_FX], VOFF_LU = SL.kkt.off[RTOC_KKT_LU] - SL.kkt.off[RTOC_KKT_FX];
  static constexpr int CV = (VOFF_LU + NU + 1) / 2, PS = (CV + 63) / 64;   // 16-byte chunks / DMA pieces of the strip Fx | lx | lu
  static constexpr int OFF_A = 0;
  static constexpr int OFF_ST = C::NX * C::LDA;
  static constexpr int OFF_S = OFF_ST + C::pad8(2 * CV);         // s+ (the last strip piece is partial: the strip takes 2 CV doubles)
  // ---- the landing zone of the Qxx panels: everything from here to the grid table is dead between the policy products and the
  //      transposes at the stage end ----
  static constexpr int OFF_G = OFF_S + C::pad8(C::NX);           // Quu (by DMA) -> G, factorised in place (L)
  static constexpr int OFF_Y = OFF_G + C::pad8(NU * NU);
  static constexpr int OFF_LINV = OFF_Y + C::pad8(NU * NU);
  static constexpr int OFF_SCR = OFF_LINV + C::pad8(NU);         // two transpose tiles; the Cholesky's 256-double scratch
  static constexpr int OFF_Z = OFF_SCR + 2 * C::SCR_TILE;
  static constexpr int OFF_W0 = OFF_Z + C::pad8(C::NX);
  static constexpr int OFF_LUP = OFF_W0 + C::pad8(C::NX);
  static constexpr int OFF_T = OFF_LUP + C::pad8(NU);
  static constexpr int OFF_GRID = OFF_T + C::pad8(NU);           // grid-point kinds of the horizon (ints)
  static constexpr int LDQ = lds_ld(C::NX), PANEL = 16 * LDQ;    // one column tile of Qxx (16 columns, padded: conflict-free both ways)
  static constexpr int OFF_Q = OFF_G;
  static_assert(OFF_Q + 2 * PANEL <= OFF_GRID, "two Qxx panels in the dead zone");
  static constexpr int DOUBLES = OFF_GRID + RV_MAX_STAGES / 2;
  static constexpr int BYTES = DOUBLES * 8;
  static_assert(2 * C::SCR_TILE >= 256, "the blocked Cholesky's scratch");
};

// ---- the lane algebra that the one-wave kernel below and the two-wave one (riccati_backward_rw2.hpp) share, by the names of
//      tests/rw_lane_model.py.  An RwLanes object carries what the helpers read the way a closure would -- the lane (lane; li =
//      lane & 15, q = lane >> 4) BY REFERENCE: the kernels re-derive it stage by stage --, and the LDS places of A's dense rows and of z;
//      the two coefficients of the structured rows, ca = A[NP][NP] and cc = A[NP][NV + NP], are arguments.  The larger shared blocks
//      are textual fragments, riccati_rw_*.inc, included by both kernels: as functions over the register tiles (P+, F, W) they cost
//      registers, and the DMA loops came out in another order ----
template <int NV, int NU>
struct RwGroups {   // compile-time predicates of the k groups (apart from RwLanes so that its static_asserts can call them)
  using C = RwCfg<NV, NU>;
  static constexpr bool group_dense(int g) { return g < C::G1 || g >= C::G0; }
  static constexpr bool group_all_dense(int g) { return 4 * g + 3 < C::NP || (4 * g >= NV && 4 * g + 3 < C::NX); }
  // the structured rows k in [NP, NV) of k group g meet column tile c (at x == k or x == NV + k)
  static constexpr bool struct_hit(int g, int c) {
    const int k0 = (4 * g > C::NP) ? 4 * g : C::NP, k1 = (4 * g + 3 < NV - 1) ? 4 * g + 3 : NV - 1;
    if (k0 > k1) return false;
    return (k0 <= 16 * c + 15 && k1 >= 16 * c) || (NV + k0 <= 16 * c + 15 && NV + k1 >= 16 * c);
  }
  static constexpr int dense_groups() {
    int n = 0;
    for (int g = 0; g < C::KG; ++g) n += group_dense(g) ? 1 : 0;
    return n;
  }
  static constexpr bool all_dense_group_hit() {
    for (int g = 0; g < C::KG; ++g)
      for (int c = 0; c < C::T; ++c)
        if (group_all_dense(g) && struct_hit(g, c)) return true;
    return false;
  }
};

template <int NV, int NU>
struct RwLanes : RwGroups<NV, NU> {
  using C = RwCfg<NV, NU>;
  using G = RwGroups<NV, NU>;
  static constexpr int NX = C::NX, NP_ = C::NP, T = C::T, TS = C::TS, QS = C::QS, RS = C::RS, LDA = C::LDA;
  static_assert(G::dense_groups() == C::NDG, "the LDS carve of A and the DMA's compact row map (cg) count the dense k groups");
  static_assert(!G::all_dense_group_hit(), "a k group without a structured row meets no synthesised fragment");
  const int &lane, &li, &q;
  const double* const sA;   // the dense rows of A, compact (RwCfg::cg), leading dimension LDA
  const double* const sZ;   // z = s+ - P+ Fx
  __device__ __forceinline__ RwLanes(const int& lane_, const int& li_, const int& q_, const double* sA_, const double* sZ_)
      : lane(lane_), li(li_), q(q_), sA(sA_), sZ(sZ_) {}

  static __device__ __forceinline__ double qsum(double v) {   // sum over the four lanes (li, 0..3)
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
  }
  __device__ __forceinline__ double zrow(int g) const {   // z in the row layout: z[4g + q] (re-read where it rides: no registers held)
    const double v = sZ[4 * g + q];
    return (4 * g + 3 < NX || 4 * g + q < NX) ? v : 0.0;
  }
  __device__ __forceinline__ double masked(int c, int t, int r, double v) const {   // element r of tile (c, t), zero outside the matrix
    const int i = 16 * c + 4 * r + q, j = 16 * t + li;
    if (16 * c + 4 * r >= NX) return 0.0;
    const bool rowok = (16 * c + 4 * r + 3 < NX) || i < NX;
    const bool colok = (16 * t + 15 < NX) || j < NX;
    return (rowok && colok) ? v : 0.0;
  }
  // A fragment of k group g, column tile c: A[4g + q][16c + li], the B operand of [.] A and the A operand of A^T [.] alike
  __device__ __forceinline__ double afrag(int g, int c) const {
    const int j = 16 * c + li;
    const double v = sA[4 * C::cg(g) + q + ((16 * c + 15 < NX || j < NX) ? j : NX - 1) * LDA];
    const int k = 4 * g + q;
    const bool rowok = G::group_all_dense(g) || (k < NP_ || (k >= NV && k < NX));
    return (rowok && (16 * c + 15 < NX || j < NX)) ? v : 0.0;
  }
  // structured rows of k group g as a B fragment of column tile c: B[k = 4g + q][x = 16c + li] = ca (x == k) + cc (x == NV + k), k in [NP, NV)
  __device__ __forceinline__ double struct_frag(int g, int c, double ca, double cc) const {
    const int k = 4 * g + q, x = 16 * c + li;
    const double v = (x == k) ? ca : (x == NV + k) ? cc : 0.0;
    return (k >= NP_ && k < NV) ? v : 0.0;
  }
  // structured rows of A^T [.] for one column of C tiles (rows = state rows): dst[k] += ca src[k], dst[NV + k] += cc src[k],
  // k in [NP, NV); NV + k lies TS tiles, RS registers and QS q-groups below k (tests/rw_lane_model.py: struct_rows_add)
  __device__ __forceinline__ void struct_rows_add(d4 (&dst)[T], const d4 (&src)[T], int cmax, double ca, double cc) const {
    d4 rot[T];
#pragma unroll
    for (int c = 0; c < T; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * c + r;
        const bool used = 4 * e + 3 >= NP_ && 4 * e < NV;   // the register holds a row of [NP, NV)
        rot[c][r] = (QS != 0 && used) ? __shfl(src[c][r], (lane + 16 * (4 - QS)) & 63, 64) : src[c][r];
      }
#pragma unroll
    for (int c = 0; c < T; ++c) {
      if (c > cmax) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * c + r, i = 4 * e + q;
        if (4 * e + 3 >= NP_ && 4 * e < NV) {
          const double coef = (i >= NP_ && i < NV) ? ca : 0.0;
          dst[c][r] = __builtin_fma(coef, src[c][r], dst[c][r]);
        }
        if (4 * e + 3 >= NV + NP_ && 4 * e < NX) {
          const int ehi = 4 * (c - TS) + r - RS, elo = ehi - 1;
          const double vhi = (ehi >= 0 && ehi < 4 * T) ? rot[(ehi >= 0 ? ehi : 0) / 4][(ehi >= 0 ? ehi : 0) % 4] : 0.0;
          const double vlo = (QS != 0 && elo >= 0 && elo < 4 * T) ? rot[(elo >= 0 ? elo : 0) / 4][(elo >= 0 ? elo : 0) % 4] : 0.0;
          const double got = (QS == 0 || q >= QS) ? vhi : vlo;
          const int k = i - NV;
          const double coef = (k >= NP_ && k < NV && i < NX) ? cc : 0.0;
          dst[c][r] = __builtin_fma(coef, got, dst[c][r]);
        }
      }
    }
  }
  // fragments of Y = L^-1 (lower triangular, in sY with leading dimension NU): Y[m = 16 tu + li][k = 4 gj + q], the A operand of
  // Z^T = Y H^T, and -Y[k][m], the A operand of K = -Y^T Z^T
  __device__ __forceinline__ double yfrag(const double* sY, int tu, int gj) const {
    const int m = 16 * tu + li, k = 4 * gj + q;
    const bool ok = m < NU && k < NU;
    const double v = sY[(ok ? m : 0) + (ok ? k : 0) * NU];
    return ok ? v : 0.0;
  }
  __device__ __forceinline__ double ytfrag(const double* sY, int tu, int gj) const {
    const int m = 16 * tu + li, k = 4 * gj + q;
    const bool ok = m < NU && k < NU;
    const double v = sY[(ok ? k : 0) + (ok ? m : 0) * NU];
    return ok ? -v : 0.0;
  }
};

template <int NV, int NU, int NS>
__global__ __launch_bounds__(64, 1) void riccati_backward_rw_kernel(BwdArgs a) {
  using C = RwCfg<NV, NU>;
  using M = RwLds<NV, NU, NS>;
  using L = RwLanes<NV, NU>;
  static_assert(C::OK, "shape outside the register-wide kernel's tiling");
  constexpr int ST_FX = M::OFF_ST, ST_LX = ST_FX + M::VOFF_LX, ST_LU = ST_FX + M::VOFF_LU;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* const sA = smem + M::OFF_A;
  double* const sG = smem + M::OFF_G;
  double* const sY = smem + M::OFF_Y;
  double* const scr = smem + M::OFF_SCR;
  double* const sS = smem + M::OFF_S;
  double* const sZ = smem + M::OFF_Z;
  double* const sW0 = smem + M::OFF_W0;
  double* const sLup = smem + M::OFF_LUP;
  double* const sT = smem + M::OFF_T;
  int* const sGrid = reinterpret_cast<int*>(smem + M::OFF_GRID);
  const int lane0 = threadIdx.x;
#include "riccati_rw_scope.inc"
  // what the shared fragments (riccati_rw_*.inc) take from this kernel: one wave that owns all of F and writes the terminal record, one
  // strip, the panels in the dead zone of its LDS; macros (each undefined by its fragment) where a variable would move instructions
  auto own = [](int) constexpr { return true; };
  auto strip_of = [](int) { return smem + M::OFF_ST; };
  auto qpanel = [](int p) { return smem + M::OFF_Q + (p & 1) * M::PANEL; };
  constexpr bool TERM_WRITER = true;
#define RW_LDS(p) ((lds_ptr_t)(p))
#define RW_QUU (smem + M::OFF_G)
#define RW_FX_OFF ST_FX
#define RW_LU(u) smem[ST_LU + (u)]
#define RW_COLUMN_MID
  d4 pp[T][T];   // P+: the value function of the grid point behind
#include "riccati_rw_vload.inc"
  d4 f[T][T];
#include "riccati_rw_dma.inc"
  // ---- operands requested one stage ahead: Bv fragments (B operand of PB, A operand of G) straight from HBM -- RAW: lanes beyond the
  //      matrix load a clamped address and are masked where the value is USED --, and Quu by DMA ----
  double bvr[KG - G0][TU];
  auto issue_bq = [&](int stage) __attribute__((always_inline)) {
    const double* kp = a.kkt + kinst + (size_t)stage * KL.stride;
    const double* bp = kp + KL.off[RTOC_KKT_FVU];
#pragma unroll
    for (int g = G0; g < KG; ++g)
#pragma unroll
      for (int tu = 0; tu < TU; ++tu) {
        const int k = 4 * g + q - NV, u = 16 * tu + li;
        const bool ok = k >= 0 && k < NV && u < NU;
        bvr[g - G0][tu] = bp[ok ? k + u * NV : (g - G0) * TU + tu];
      }
    issue_dma_quu(stage);
  };
  auto NQ_NEXT = [](int t) constexpr { return (16 * (t + 2) <= NX) ? 16 : NX - 16 * (t + 1); };   // DMA instructions of panel t + 1
  issue_dma_strip(hi);
  issue_bq(hi);
  issue_dma_A(hi);
  for (int e = lane; e < a.nstages; e += 64) sGrid[e] = a.grid[e].type | (a.grid[e].dims << 8);   // (the host keeps nstages <= RV_MAX_STAGES)
  rv_lds_sync();

  for (int st = hi; st >= lo; --st) {
    lane = lane0;
    asm volatile("" : "+v"(lane));   // opaque per stage: keeps LICM from pinning the per-lane addresses of every unrolled loop
    lane &= 63;
    li = lane & 15;
    q = lane >> 4;
    const int gword = __builtin_amdgcn_readfirstlane(sGrid[st]);
    const bool impact = (gword & 0xff) == RTOC_GRID_IMPACT;
    const double* kr = a.kkt + kinst + (size_t)st * KL.stride;
    double* rr = a.ric + rinst + (size_t)st * RL.stride;

    RV_PROF(0);
    // the strip of this grid point and its Bv / Quu registers have landed; the DMA pieces of A -- the youngest vector-memory
    // operations of the previous stage, NPC_A instructions -- may still be in flight (A is first read by the H product)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC_A) : "memory");
    __builtin_amdgcn_wave_barrier();
    RV_PROF(1);
    // ================= 1. z = s+ - P+ Fx (brrf.cpp:86): per-lane partial sums over the rows a lane holds, q-reduction =========
    {
#include "riccati_rw_z.inc"
    }
    rv_lds_sync();

    RV_PROF(2);
    // Qxu^T in the layout of H^T (row u = 16 tu + 4r + q, column x = 16c + li), RAW
    d4 hq[TU][T];
    auto issue_hq = [&]() __attribute__((always_inline)) {
      const double* hp = kr + KL.off[RTOC_KKT_QXU];
#pragma unroll
      for (int tu = 0; tu < TU; ++tu)
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u = 16 * tu + 4 * r + q, x = 16 * c + li;
            hq[tu][c][r] = hp[((x < NX) ? x : NX - 1) + ((u < NU) ? u : NU - 1) * NX];
          }
    };
    d4 acc[T][TU];   // PB = P+[:, v] Bv: rows x = 16c + .., columns u = 16 tu + li; column NU: z
#pragma unroll
    for (int c = 0; c < T; ++c)
#pragma unroll
      for (int tu = 0; tu < TU; ++tu) acc[c][tu] = zero4();
    if (!impact) {
      // ================= 2. PB, G = Quu + Bv^T PB[v, :] (rider column NU: Bv^T z_v) =================
      double bvf[KG - G0][TU];
#pragma unroll
      for (int g = G0; g < KG; ++g)
#pragma unroll
        for (int tu = 0; tu < TU; ++tu) {
          const int k = 4 * g + q - NV, u = 16 * tu + li;
          bvf[g - G0][tu] = (k >= 0 && k < NV && u < NU) ? bvr[g - G0][tu] : 0.0;
        }
#pragma unroll
      for (int g = G0; g < KG; ++g)
#pragma unroll
        for (int tu = 0; tu < TU; ++tu)
#pragma unroll
          for (int c = 0; c < T; ++c) acc[c][tu] = mfma16(pp[g / 4][c][g % 4], bvf[g - G0][tu], acc[c][tu]);
#include "riccati_rw_g.inc"
    }
    RV_PROF(3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // A has landed
    __builtin_amdgcn_wave_barrier();
    // z into the idle column NU of PB: column NU of H = A^T PB is then A^T z (on an impact grid point PB is that column alone)
#pragma unroll
    for (int g = 0; g < KG; ++g) acc[g / 4][TU - 1][g % 4] = (li == NUC) ? ln.zrow(g) : acc[g / 4][TU - 1][g % 4];

    const double ca = sA[NP_ + NP_ * LDA], cc = sA[NP_ + (NV + NP_) * LDA];   // A[NP][NP], A[NP][NV + NP] (row NP is a corner-group row: staged)

    d4 zt[TU][T];   // Z^T = Y H^T
    if (!impact) {
      issue_hq();
      // ================= 4. H^T = Qxu^T + PB^T A DIRECTLY in the layout Z^T = Y H^T reads (rows u, columns x): PB's C tiles are the
      //                      A operand as they stand, A's fragments the B operand; the structured rows k of A (ca e_k | cc e_NV+k)
      //                      are synthesised fragments that meet two or three column tiles.  Row NUC of control tile TU - 1 is the
      //                      rider (A^T z)^T.  No transposes, no rotations (tests/rw_lane_model.py: direct_ht) =================
      d4 hT[TU][T];
#pragma unroll
      for (int tu = 0; tu < TU; ++tu) {
        asm volatile("" ::: "memory");   // (A's fragments are re-read per control tile rather than held across them)
#pragma unroll
        for (int c = 0; c < T; ++c) hT[tu][c] = zero4();
        d4(&hrow)[T] = hT[tu];
#include "riccati_rw_hrow.inc"
        if (tu == TU - 1) {   // the rider: w0 = A^T z
#pragma unroll
          for (int c = 0; c < T; ++c) {
            const int x = 16 * c + li;
            if (q == NUC % 4 && x < NX) sW0[x] = hT[tu][c][NUC / 4];
          }
        }
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u = 16 * tu + 4 * r + q, x = 16 * c + li;
            hT[tu][c][r] = (u < NU && x < NX) ? hT[tu][c][r] + hq[tu][c][r] : 0.0;
          }
      }
      RV_PROF(4);
      // ================= 3. LLT(G) (riccati_factorizer.cpp:49), Y = L^-1; t = Y lu', k = -Y^T t =================
      if (wave_llt_inv_blocked<NU, NU>(sG, sG, smem + M::OFF_LINV, sY, scr, lane)) stat |= RTOC_STAT_QUU_NOT_SPD;
      rv_lds_sync();
      RV_PROF(5);
      {
        const int u = (lane < NU) ? lane : 0;
        double tv = 0.0;
#pragma unroll
        for (int j = 0; j < NU; ++j) tv = __builtin_fma(sY[u + j * NU], sLup[j], tv);
        if (lane < NU) sT[lane] = tv;
        rv_lds_sync();
        double kv = 0.0;
#pragma unroll
        for (int j = 0; j < NU; ++j) kv = __builtin_fma(sY[j + u * NU], sT[j], kv);
        if (lane < NU) rr[RL.off[RTOC_RIC_KV] + lane] = -kv;
        if (is_bad(kv)) stat |= RTOC_STAT_NAN;
      }
      RV_PROF(6);
      // ================= 6. Z^T = Y H^T (Y lower triangular: the tile above the diagonal is skipped) =================
#pragma unroll
      for (int tu = 0; tu < TU; ++tu) {
#pragma unroll
        for (int c = 0; c < T; ++c) zt[tu][c] = zero4();
#pragma unroll
        for (int gj = 0; gj < KGU; ++gj) {
          if (gj >= 4 * (tu + 1)) continue;
          const double av = ln.yfrag(sY, tu, gj);
#pragma unroll
          for (int c = 0; c < T; ++c) zt[tu][c] = mfma16(av, hT[gj / 4][c][gj % 4], zt[tu][c]);
        }
      }
      RV_PROF(7);
      // ================= 7. K = -Y^T Z^T (riccati_factorizer.cpp:55), tile by tile -> HBM (K row-major) =================
      double chk = 0.0;
#pragma unroll
      for (int tu = 0; tu < TU; ++tu) {
        double yv[KGU];
#pragma unroll
        for (int gj = 0; gj < KGU; ++gj) yv[gj] = ln.ytfrag(sY, tu, gj);
#pragma unroll
        for (int c = 0; c < T; ++c) {
          d4 kk = zero4();
#pragma unroll
          for (int gj = 0; gj < KGU; ++gj) {
            if (gj < 4 * tu) continue;
            kk = mfma16(yv[gj], zt[gj / 4][c][gj % 4], kk);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u = 16 * tu + 4 * r + q, x = 16 * c + li;
            if (u < NU && x < NX) rr[RL.off[RTOC_RIC_K] + u * NX + x] = kk[r];
            chk = __builtin_fma(kk[r], 0.0, chk);
          }
        }
      }
      if (is_bad(chk)) stat |= RTOC_STAT_NAN;
    } else {
      // impact grid point (riccati_factorizer.cpp:178-197): no controls; A^T z by the rider column alone
      constexpr int tu = TU - 1;
      d4 hrow[T];   // row NUC: (A^T z)^T
#pragma unroll
      for (int c = 0; c < T; ++c) hrow[c] = zero4();
#include "riccati_rw_hrow.inc"
#pragma unroll
      for (int c = 0; c < T; ++c) {
        const int x = 16 * c + li;
        if (q == NUC % 4 && x < NX) sW0[x] = hrow[c][NUC / 4];
      }
#pragma unroll
      for (int tz = 0; tz < TU; ++tz)
#pragma unroll
        for (int c = 0; c < T; ++c) zt[tz][c] = zero4();
    }

    RV_PROF(8);
    // ================= 8. F starts from Qxx (upper tiles; off-diagonal ones symmetrised: brrf.cpp:85 folded into the start
    //                      value), F -= Z Z^T (brrf.cpp:82-84) =================
    // F accumulates from ZERO (-Z Z^T, then A^T W column by column); G, Y and the scratch are dead: the first two panels of Qxx
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    issue_qxx_panel(kr, 0);   // (panel 1 covers A^T z and t, which the update of s below still reads: behind it)
#pragma unroll
    for (int c = 0; c < T; ++c)
#pragma unroll
      for (int t = c; t < T; ++t) f[c][t] = zero4();
    if (!impact) {
#pragma unroll
      for (int gu = 0; gu < KGU; ++gu)
#pragma unroll
        for (int c = 0; c < T; ++c)
#pragma unroll
          for (int t = c; t < T; ++t) f[c][t] = mfma16(-zt[gu / 4][c][gu % 4], zt[gu / 4][t][gu % 4], f[c][t]);
    }
    RV_PROF(9);
    // ---- s = A^T z - lx - H k = w0 - lx + Z t (brrf.cpp:86-90): column layout, per-lane partial sums + q-reduction; -> LDS (the s+
    //      of the next grid point) and HBM, with the (zero) switching-time fields of the record ----
    rv_lds_sync();
    {
      double tr_[KGU];
#pragma unroll
      for (int gu = 0; gu < KGU; ++gu) {
        const double v = sT[4 * gu + q];
        tr_[gu] = (!impact && 4 * gu + q < NU) ? v : 0.0;
      }
#pragma unroll
      for (int c = 0; c < T; ++c) {
        double part = 0.0;
#pragma unroll
        for (int gu = 0; gu < KGU; ++gu) part = __builtin_fma(zt[gu / 4][c][gu % 4], tr_[gu], part);
        part = L::qsum(part);
        const int j = 16 * c + li;
        const int jc = (j < NX) ? j : 0;
        const double sn = sW0[jc] - smem[ST_LX + jc] + part;
        if (q == 0 && j < NX) {
          sS[j] = sn;
          rr[RL.off[RTOC_RIC_S] + j] = sn;
        }
        if (q == 1 && j < NX) rr[RL.off[RTOC_RIC_PSI] + j] = 0.0;
        if (q == 2 && j < NX) rr[RL.off[RTOC_RIC_PHI] + j] = 0.0;
      }
      if (lane < 5) rr[RL.off[RTOC_RIC_SCAL] + lane] = 0.0;
    }
    // the strip (Fx, lx, lu) has been read for the last time: the one of the next grid point
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    issue_qxx_panel(kr, 1);
    if (st > lo) issue_dma_strip(st - 1);
    asm volatile("" ::: "memory");

    RV_PROF(10);
    // ================= 9. column tile by column tile: W[:, t] = P+ A[:, t], F[c][t] += A^T[c] W[:, t] =================
#pragma unroll
    for (int t = 0; t < T; ++t) {
#include "riccati_rw_column.inc"
      // ---- panel t of Qxx has landed: every vector-memory operation older than the DMA of panel t + 1 is waited for (counted
      //      conservatively: only that younger panel's instructions may still be in flight); its part of the start value of F ----
      if (t + 1 < T) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ_NEXT(t)) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      qxx_seed_panel(t);
      // ---- P of grid point st + 1 -> HBM, a T-th per column tile, from the registers that hold it as P+ until the last of these
      //      products (element (i, j) through its mirror (j, i): li along the contiguous index) ----
      if (st < hi) {
        double* pw = a.ric + rinst + (size_t)(st + 1) * RL.stride + RL.off[RTOC_RIC_P];
#pragma unroll
        for (int mt = 0; mt < T; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * t + 4 * r + q, j = 16 * mt + li;
            if (i < NX && j < NX) pw[j + i * NX] = pp[t][mt][r];
          }
      }
      if (t + 2 < T) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the panel's reads are done: its buffer takes panel t + 2
        __builtin_amdgcn_wave_barrier();
        issue_qxx_panel(kr, t + 2);
      }
    }
    RV_PROF(11);
    // ---- A has been read for the last time: the dense rows of the next grid point's ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (st > lo) {
      issue_bq(st - 1);
      issue_dma_A(st - 1);   // (the LAST vector-memory operations of the stage: the counted wait at the next stage top)
    }
    asm volatile("" ::: "memory");

    RV_PROF(12);
    // ================= 10. P <- sym(F): upper tiles as computed, diagonal tiles mirrored, lower tiles transposed =================
    {
      constexpr int NTR = T * (T + 1) / 2;
#pragma unroll
      for (int n0 = 0; n0 < NTR; n0 += 2) {
#pragma unroll
        for (int n = n0; n < n0 + 2 && n < NTR; ++n) {
          const int c = rv_tile_row(T, n), t = rv_tile_col(T, n);
          double* s_ = scr + (n - n0) * SCR_TILE;
#pragma unroll
          for (int r = 0; r < 4; ++r) s_[(q + 4 * r) * SCR_LD + li] = ln.masked(c, t, r, f[c][t][r]);
        }
        rv_lds_sync();
#pragma unroll
        for (int n = n0; n < n0 + 2 && n < NTR; ++n) {
          const int c = rv_tile_row(T, n), t = rv_tile_col(T, n);
          const double* s_ = scr + (n - n0) * SCR_TILE;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double tr = s_[li * SCR_LD + q + 4 * r];
            if (t > c) {
              pp[c][t][r] = ln.masked(c, t, r, f[c][t][r]);
              pp[t][c][r] = tr;                                  // zero outside the matrix: the tile was masked on its way in
            } else {
              pp[c][c][r] = (q + 4 * r <= li) ? ln.masked(c, c, r, f[c][c][r]) : tr;   // upper triangle mirrored (P exactly symmetric)
            }
          }
        }
        rv_lds_sync();
      }
    }
    RV_PROF(13);
  }

#include "riccati_rw_end.inc"
}

}  // namespace rtoc
