// riccati_rw_hrow.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): the rows of
// control tile tu of PB^T A onto hrow, DIRECTLY in the layout Z^T = Y H^T reads: PB's C tiles are the A operand as they stand, A's
// fragments the B operand, the structured rows k of A (ca e_k | cc e_NV+k) synthesised fragments (tests/rw_lane_model.py: direct_ht).
// Expects in scope: tu, hrow (d4 [T]: row tile tu of H^T, or on an impact grid point the rider row (A^T z)^T alone), acc (PB, z in
// its idle column NU), L, ln, ca, cc, KG, T.
#pragma unroll
        for (int g = 0; g < KG; ++g) {
          const double aop = acc[g / 4][tu][g % 4];
#pragma unroll
          for (int c = 0; c < T; ++c) {
            const bool hit = L::struct_hit(g, c);
            if (!L::group_dense(g) && !hit) continue;
            double bop = L::group_dense(g) ? ln.afrag(g, c) : 0.0;
            if (hit) bop += ln.struct_frag(g, c, ca, cc);   // (afrag is zero on the structured rows)
            hrow[c] = mfma16(aop, bop, hrow[c]);
          }
        }
