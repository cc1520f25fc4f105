// riccati_rw_g.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp: its wave 0):
// G = Quu + Bv^T PB[v, :] onto Quu's LDS place, and by the rider column NU, Bv^T z_v, lu' = lu - Bv^T z_v (riccati_factorizer.cpp:44-49).
// Expects in scope: ln, acc (PB), bvf (Bv's fragments), sG, sLup, G0, KG, TU, NU, NUC, li, q.  The sites differ by RW_LU(u): lu[u].
      d4 gacc[TU][TU];
#pragma unroll
      for (int tr = 0; tr < TU; ++tr)
#pragma unroll
        for (int tu = 0; tu < TU; ++tu) gacc[tr][tu] = zero4();
#pragma unroll
      for (int g = G0; g < KG; ++g)
#pragma unroll
        for (int tu = 0; tu < TU; ++tu) {
          double bop = acc[g / 4][tu][g % 4];
          if (tu == TU - 1) bop = (li == NUC) ? ln.zrow(g) : bop;
#pragma unroll
          for (int tr = 0; tr < TU; ++tr) gacc[tr][tu] = mfma16(bvf[g - G0][tr], bop, gacc[tr][tu]);
        }
#pragma unroll
      for (int tr = 0; tr < TU; ++tr)
#pragma unroll
        for (int tu = 0; tu < TU; ++tu)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u0 = 16 * tr + 4 * r + q, u1 = 16 * tu + li;
            if (u0 < NU && u1 < NU) sG[u0 + u1 * NU] += gacc[tr][tu][r];
            if (tu == TU - 1 && u0 < NU && li == NUC) sLup[u0] = RW_LU(u0) - gacc[tr][tu][r];   // lu' = lu - Bv^T z_v
          }
      rv_lds_sync();
#undef RW_LU
