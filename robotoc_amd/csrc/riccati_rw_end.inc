// riccati_rw_end.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): behind the
// stage loop, P of the last grid point of the segment -> its Riccati record (element (i, j) through its mirror (j, i): li along the
// contiguous index; each wave the row tiles it owns), and the instance's status bits.
// Expects in scope: pp, own, RL, NX, T, a, rinst, lo, b, stat, li, q.
  {
    double* pw = a.ric + rinst + (size_t)lo * RL.stride + RL.off[RTOC_RIC_P];
#pragma unroll
    for (int kt = 0; kt < T; ++kt)
#pragma unroll
      for (int mt = 0; mt < T; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * kt + 4 * r + q, j = 16 * mt + li;
          if (own(kt) && i < NX && j < NX) pw[j + i * NX] = pp[kt][mt][r];
        }
  }
  if (stat) atomicOr(&a.status[b], stat);
