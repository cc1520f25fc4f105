// riccati_rw_dma.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): the
// LDS-DMA issue loops of a grid point's record and the start value of F that the Qxx panels bring, as lambdas of the including
// kernel.  (Textual: as members of RwLanes the strip's and the panel's loops came out in another instruction order in _rw2.)
// Expects in scope: C, M, KL, NX, NU, T, LDA, LDQ, a, kinst, smem, sA, lane, li, q and f (d4 f[T][T]: the accumulators of F).
// The sites differ by strip_of(stage): where the strip Fx | lx | lu of grid point stage lands; qpanel(p): the panel of column tile p
// of Qxx; own(t): this wave holds column tile t of F; and two macros -- RW_LDS(p): the LDS destination operand of a DMA for the generic
// pointer p (as a lambda, _rw's cast costs its kernel the host stub); RW_QUU: the LDS place of Quu and G (one name for both moves code).
  // ---- the dense k groups of A (rows [0, 4 G1) and [4 G0, 4 KG) of every column) into the padded compact layout; whole padded
  //      columns per piece, so that a piece differs from the next by a scalar ----
  constexpr int NPC_A = (NX + 64 / C::HL - 1) / (64 / C::HL);   // DMA instructions of A per grid point
  static_assert(NPC_A < 64, "counted wait");
  auto issue_dma_A = [&](int stage) __attribute__((always_inline)) {
    const double* kp = a.kkt + kinst + (size_t)stage * KL.stride + KL.off[RTOC_KKT_FXX];
    constexpr int CPP = 64 / C::HL, NPC = NPC_A;
    const unsigned col0 = (unsigned)lane / C::HL, ch0 = (unsigned)lane - col0 * C::HL;
    const unsigned rl = 2 * ch0;                                                        // compact row of the chunk
    const unsigned srow = (rl < 4 * C::G1) ? rl : ((rl < 4 * C::NDG) ? rl + 4 * (C::G0 - C::G1) : 0);   // (the padding chunk loads anything)
    const unsigned voff = col0 * NX + srow;
    if (col0 < CPP) {
#pragma unroll
      for (int p = 0; p < NPC; ++p) {
        if ((p + 1) * CPP <= NX || p * CPP + (int)col0 < NX)
          __builtin_amdgcn_global_load_lds(kp + p * CPP * NX + voff, RW_LDS(sA + p * CPP * LDA), 16, 0, 0);
      }
    }
  };
  auto issue_dma_strip = [&](int stage) __attribute__((always_inline)) {
    const double* kp = a.kkt + kinst + (size_t)stage * KL.stride + KL.off[RTOC_KKT_FX];
#pragma unroll
    for (int p = 0; p < M::PS; ++p) {
      const int n = lane + 64 * p;
      if (64 * (p + 1) <= M::CV || n < M::CV) __builtin_amdgcn_global_load_lds(kp + 2 * n, RW_LDS(strip_of(stage) + 128 * p), 16, 0, 0);
    }
  };
  // Quu -> the LDS place of G (flat: G's leading dimension is NU); the G product adds itself onto it
  auto issue_dma_quu = [&](int stage) __attribute__((always_inline)) {
    const double* kp = a.kkt + kinst + (size_t)stage * KL.stride;
    constexpr int CQ = (NU * NU + 1) / 2, PQ = (CQ + 63) / 64;
    const double* gp = kp + KL.off[RTOC_KKT_QUU];
#pragma unroll
    for (int p = 0; p < PQ; ++p) {
      const int n = lane + 64 * p;
      if (64 * (p + 1) <= CQ || n < CQ) __builtin_amdgcn_global_load_lds(gp + 2 * n, RW_LDS(RW_QUU + 128 * p), 16, 0, 0);
    }
  };
  // Qxx comes in by DMA too, one column tile (16 columns, all rows: 8 KB, contiguous in the record) at a time into one of two padded
  // panels in the zone that is dead between the policy products and the transposes; F accumulates from zero and takes its start
  // value panel by panel at the end of the column loop's iterations (the same sum in another order; the symmetrisation of
  // brrf.cpp:85 folded in): panel p holds the transposed elements of the tiles (p, t >= p) -- read with li along the contiguous
  // index -- and the direct elements of the tiles (c < p, p).  No registers wait for these 32 KB.
  auto issue_qxx_panel = [&](const double* kr_, int p) __attribute__((always_inline)) {
    const double* qb_ = kr_ + KL.off[RTOC_KKT_QXX] + (size_t)16 * p * NX;
    double* dst = qpanel(p);
#pragma unroll
    for (int col = 0; col < 16; ++col) {
      if (16 * p + col >= NX) continue;
      if (lane < NX / 2) __builtin_amdgcn_global_load_lds(qb_ + col * NX + 2 * lane, RW_LDS(dst + col * LDQ), 16, 0, 0);
    }
  };
  auto qxx_seed_panel = [&](int p) __attribute__((always_inline)) {
    const double* pan = qpanel(p);
#pragma unroll
    for (int t = p; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // tile (p, t): element (16p + 4r + q, 16t + li) <- Qxx[16t + li][16p + 4r + q], column 4r + q of the panel
        if (!own(t)) continue;
        const int i = 16 * p + 4 * r + q, j = 16 * t + li;
        if (16 * p + 4 * r >= NX) continue;
        const bool ok = ((16 * p + 4 * r + 3 < NX) || i < NX) && ((16 * t + 15 < NX) || j < NX);
        const double v = pan[(ok ? j : 0) + (ok ? 4 * r + q : 0) * LDQ];
        f[p][t][r] = __builtin_fma((t == p) ? 1.0 : 0.5, ok ? v : 0.0, f[p][t][r]);
      }
#pragma unroll
    for (int c = 0; c < p; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // tile (c, p): element (16c + 4r + q, 16p + li) <- Qxx[16c + 4r + q][16p + li], column li of the panel
        if (!own(p)) continue;
        const int j = 16 * p + li;
        const bool ok = (16 * p + 15 < NX) || j < NX;
        const double v = pan[16 * c + 4 * r + q + (ok ? li : 0) * LDQ];
        f[c][p][r] = __builtin_fma(0.5, ok ? v : 0.0, f[c][p][r]);
      }
  };
#undef RW_LDS
#undef RW_QUU
