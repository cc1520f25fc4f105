// riccati_rw_z.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp at every stage top,
// _rw2.hpp in its prologue): z = s+ - P+ Fx (brrf.cpp:86) from the resident P+: per-lane partial sums over the rows a lane holds,
// q-reduction.  Expects in scope: L, pp, smem, sS, sZ, KG, T, NX, li, q.  The sites differ by RW_FX_OFF (a macro: as a variable it moves instructions in _rw2): where Fx lies in smem.
      double fxr[KG];
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        const double v = smem[RW_FX_OFF + 4 * g + q];
        fxr[g] = (4 * g + 3 < NX || 4 * g + q < NX) ? v : 0.0;
      }
#pragma unroll
      for (int mt = 0; mt < T; ++mt) {
        double part = 0.0;
#pragma unroll
        for (int g = 0; g < KG; ++g) part = __builtin_fma(pp[g / 4][mt][g % 4], fxr[g], part);
        part = L::qsum(part);
        const int j = 16 * mt + li;
        const double sv = sS[(j < NX) ? j : 0];
        if (q == 0 && j < NX) sZ[j] = sv - part;
      }
#undef RW_FX_OFF
