// riccati_rw_vload.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): the
// value function of grid point hi + 1 -> registers / LDS: the terminal one (P_N = Qxx_N, s_N = -lx_N, riccati_recursion.cpp:37-38),
// which goes to the Riccati record of grid point N too, or the one a previous segment left in the Riccati records.
// Expects in scope: pp (d4 pp[T][T]), KL, RL, NX, T, a, kinst, rinst, N, hi, sS, lane, li, q.
// The sites differ by TERM_WRITER (constexpr bool): this wave writes the terminal record.
  {
    const bool term = (hi == N - 1);
    const double* psrc = term ? (a.kkt + kinst + (size_t)N * KL.stride + KL.off[RTOC_KKT_QXX])
                              : (a.ric + rinst + (size_t)(hi + 1) * RL.stride + RL.off[RTOC_RIC_P]);
    const double* ssrc = term ? (a.kkt + kinst + (size_t)N * KL.stride + KL.off[RTOC_KKT_LX])
                              : (a.ric + rinst + (size_t)(hi + 1) * RL.stride + RL.off[RTOC_RIC_S]);
#pragma unroll
    for (int kt = 0; kt < T; ++kt)
#pragma unroll
      for (int mt = 0; mt < T; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * kt + 4 * r + q, j = 16 * mt + li;
          const bool ok = i < NX && j < NX;
          const double v = psrc[ok ? j + i * NX : 0];   // (symmetric: the mirror element, li along the contiguous index)
          pp[kt][mt][r] = ok ? v : 0.0;
        }
    for (int e = lane; e < NX; e += 64) sS[e] = term ? -ssrc[e] : ssrc[e];
    if (term && TERM_WRITER) {
      double* rr = a.ric + rinst + (size_t)N * RL.stride;
      const d2* s2 = reinterpret_cast<const d2*>(psrc);
      d2* t2 = reinterpret_cast<d2*>(rr + RL.off[RTOC_RIC_P]);
      for (int e = lane; e < NX * NX / 2; e += 64) t2[e] = s2[e];
      for (int e = lane; e < NX; e += 64) rr[RL.off[RTOC_RIC_S] + e] = -ssrc[e];
    }
  }
