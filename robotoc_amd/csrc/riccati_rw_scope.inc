// riccati_rw_scope.inc -- textual fragment shared by the register-wide backward kernels (riccati_backward_rw.hpp, _rw2.hpp): the names
// both kernels and the other riccati_rw_*.inc fragments work with -- the shape's constants, the record layouts, the instance and the
// per-lane state (lane, li, q: re-derived at every stage top; ln: the lane algebra over them).
// Expects in scope: C, M, L, NV, NU, NS, a, sA, sZ and lane0 (this lane of the wave).
  constexpr int NX = C::NX, NP_ = C::NP, T = C::T, TU = C::TU, KG = C::KG, KGU = C::KGU, G0 = C::G0, NUC = C::NUC;
  constexpr int TS = C::TS, LS = C::LS, LDA = C::LDA, LDQ = M::LDQ, SCR_LD = C::SCR_LD, SCR_TILE = C::SCR_TILE;
  constexpr rtoc_layout SL = StaticLayout<NV, NU, NS>::make();
  constexpr rtoc_record_layout KL = SL.kkt, RL = SL.ric;
  static_assert(M::VOFF_LX > 0 && M::VOFF_LU > M::VOFF_LX && M::VOFF_LX % 2 == 0 && M::VOFF_LU % 2 == 0, "Fx, lx, lu lie behind one another in the record");
  static_assert(KL.off[RTOC_KKT_FXX] % 2 == 0 && KL.off[RTOC_KKT_FX] % 2 == 0 && KL.off[RTOC_KKT_QUU] % 2 == 0 && KL.off[RTOC_KKT_QXX] % 2 == 0 && KL.stride % 2 == 0 && NX % 2 == 0, "16-byte chunks");
  const int b = a.first + (int)blockIdx.x;
  if (b >= a.batch) return;
  int lane = lane0 & 63, li = lane & 15, q = lane >> 4;
  const int N = a.nstages - 1;
  const size_t kinst = (size_t)b * a.nstages * KL.stride;
  const size_t rinst = (size_t)b * a.nstages * RL.stride;
  const int hi = a.seg_hi, lo = a.seg_lo;
  unsigned stat = 0;
  const L ln(lane, li, q, sA, sZ);
