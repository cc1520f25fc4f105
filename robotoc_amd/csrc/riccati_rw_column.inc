// riccati_rw_column.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): column
// tile t of the O(n^3) part, W[:, t] = P+ A[:, t] and F[c][t] += A^T[c] W[:, t], c <= t (brrf.cpp:31-91).
// Expects in scope: t, L, ln, pp, f, ca, cc, NV, NX, NP_, T, KG, TS, LS; declares w (d4 w[T]: column tile t of W).
// The sites differ by RW_COLUMN_MID: what the kernel does between the two products.
      d4 w[T];
#pragma unroll
      for (int tm = 0; tm < T; ++tm) w[tm] = zero4();
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        if (!L::group_dense(g)) continue;
        const double bv = ln.afrag(g, t);
#pragma unroll
        for (int tm = 0; tm < T; ++tm) w[tm] = mfma16(pp[g / 4][tm][g % 4], bv, w[tm]);
      }
      {
        // structured rows k of A: W[:, k] += ca P+[:, k] (same tile / lane), W[:, NV + k] += cc P+[:, k] (TS tiles, LS lanes to the left)
        const int j = 16 * t + li, k = j - NV;
        const double ca_l = (j >= NP_ && j < NV) ? ca : 0.0;
        const double cc_l = (k >= NP_ && k < NV && j < NX) ? cc : 0.0;
#pragma unroll
        for (int tm = 0; tm < T; ++tm)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (16 * t + 15 >= NP_ && 16 * t < NV) w[tm][r] = __builtin_fma(ca_l, pp[tm][t][r], w[tm][r]);
            if (16 * t + 15 >= NV + NP_ && 16 * t < NX) {
              double src = 0.0;
              if constexpr (LS == 0) {
                if (t - TS >= 0) src = pp[tm][(t - TS >= 0) ? t - TS : 0][r];
              } else {
                if (t - TS >= 0) src = dpp_from_left<LS>(pp[tm][(t - TS >= 0) ? t - TS : 0][r]);
                if (t - TS - 1 >= 0) src += dpp_from_right<16 - LS>(pp[tm][(t - TS - 1 >= 0) ? t - TS - 1 : 0][r]);
              }
              w[tm][r] = __builtin_fma(cc_l, src, w[tm][r]);
            }
          }
      }
      RW_COLUMN_MID;
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        if (!L::group_dense(g)) continue;
        const double bw = w[g / 4][g % 4];
#pragma unroll
        for (int c = 0; c <= t; ++c) f[c][t] = mfma16(ln.afrag(g, c), bw, f[c][t]);
      }
      {
        d4 col[T];
#pragma unroll
        for (int c = 0; c < T; ++c) col[c] = (c <= t) ? f[c][t] : zero4();
        ln.struct_rows_add(col, w, t, ca, cc);
#pragma unroll
        for (int c = 0; c <= t; ++c) f[c][t] = col[c];
      }
#undef RW_COLUMN_MID
