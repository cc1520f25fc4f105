// kernel_set.hpp -- the kernels of ONE robot shape <NV, NU, NS> (NF = NS: the reference sizes the switching-
// constraint blocks with max_dimf too, split_kkt_matrix.cpp:7-34) gathered behind descriptors, so that the host
// runtime (rt_shapes.hip) dispatches by dimensions at run time.  Every shape is compiled in its own translation unit
// (shape_inst.hip, once per entry of the SHAPES list in the Makefile): adding a robot = one entry + make.
// The descriptors and the table are kernel_table.hpp, which is all the host runtime sees of a shape.  Here: the kernel
// headers and make_set, which writes a kernel's launch geometry next to its entry point (the block size is the kernel's
// __launch_bounds__).  Included by shape_inst.hip alone; every header below holds templates only, so that a shape object
// carries the instantiations of its shape and nothing else.
#pragma once
#include <cstring>

#include "../../include/rtoc.h"
#include "kernel_table.hpp"
#include "condense.hpp"
#include "unconstr_dynamics.hpp"
#include "friction_cone.hpp"
#include "riccati_backward.hpp"
#include "riccati_backward_rs.hpp"
#include "riccati_backward_rv.hpp"
#include "riccati_backward_rw.hpp"
#include "riccati_backward_rw2.hpp"
#include "condense_rv.hpp"
#include "riccati_scan.hpp"
#include "riccati_forward.hpp"
#include "unconstr_riccati.hpp"
#include "parnmpc_backward_correction.hpp"

namespace rtoc {

template <int NV, int NU, int NS, int NW0, int NW1>
inline KernelSet make_set() {
  KernelSet k;
  memset(&k, 0, sizeof(k));
  k.nv = NV;
  k.nu = NU;
  k.ns = NS;
  k.nvariants = 2;
  k.kl = StaticLayout<NV, NU, NS>::make().kkt;
  k.rl = StaticLayout<NV, NU, NS>::make().ric;
  k.bwd[0] = {riccati_backward_kernel<NV, NU, NS, NW0>, 64 * NW0, BwdCfg<NV, NU, NS, NW0>::LDS_BYTES, 1};
  k.bwd[1] = {riccati_backward_kernel<NV, NU, NS, NW1>, 64 * NW1, BwdCfg<NV, NU, NS, NW1>::LDS_BYTES, 1};
  // role-split kernel: matrix wave + vector wave per instance; needs the state in 4 tiles, the control Hessian and the
  // three free-rider columns of the G product in one 16-column tile, and two spare columns in the state's last tile
  if constexpr (2 * NV + 1 <= 64 && NU + 3 <= 16 && rs_rider_columns_fit<NV>) {
    k.bwd[2] = {riccati_backward_rs_kernel<NV, NU, NS>, 128, BwdCfg<NV, NU, NS, 2>::LDS_BYTES, 1};
    k.nvariants = 3;
    // four instances per workgroup, both waves of an instance on one SIMD
    if (4 * BwdCfg<NV, NU, NS, 2>::LDS_BYTES + 64 <= 160 * 1024) {
      k.bwd[3] = {riccati_backward_rs4_kernel<NV, NU, NS>, 512, 4 * BwdCfg<NV, NU, NS, 2>::LDS_BYTES + 64, 4};
      k.nvariants = 4;
      if constexpr (NV % 4 == 2 && NV > NU) k.bwd_sa = {riccati_backward_rs4_kernel<NV, NU, NS, true>, 512, k.bwd[3].lds, 4};
    }
  }
  if constexpr (RvCfg<NV, NU>::OK) {
    k.bwd_rv = {riccati_backward_rv_kernel<NV, NU, NS, false>, 64, rv_lds_bytes<NV, NU, NS>(), 1};
    if constexpr (NV % 16 == 2 && RvCfg<NV, NU>::T == 3 && NV - NU > 0 && NV - NU <= 8 && (NV - NU) % 2 == 0)
    {
      k.bwd_rv_sa = {riccati_backward_rv_kernel<NV, NU, NS, true>, 64, k.bwd_rv.lds, 1};
      k.bwd_rv_sto = {riccati_backward_rv_kernel<NV, NU, NS, true, true>, 64, k.bwd_rv.lds, 1};
    }
  }
  if constexpr (RwCfg<NV, NU>::OK)
    k.bwd_rw = {riccati_backward_rw_kernel<NV, NU, NS>, 64, RwLds<NV, NU, NS>::BYTES, 1};
  else if constexpr (RwCfg<NV, NU>::OK2)
    k.bwd_rw = {riccati_backward_rw2_kernel<NV, NU, NS>, 128, Rw2Lds<NV, NU, NS>::BYTES, 1};
  constexpr int NWF = (2 * NV + NU + 63) / 64;
  if constexpr (NWF == 1)
    k.fwd = {riccati_forward_kernel<NV, NU, NS>, 64, 0, 1};
  else
    k.fwd = {riccati_forward_mw_kernel<NV, NU, NS, NWF>, 64 * NWF, 0, 1};
  k.dl = StaticLayout<NV, NU, NS>::make().dir;
  k.cl = StaticLayout<NV, NU, NS>::make().cdd;
  k.fill = {unconstr_fill_kernel<NV>, 128, 0, 1};
  k.ucond = {unconstr_condense_kernel<NV>, 64, 0, 1};
  k.uexp = {unconstr_expand_kernel<NV>, 64, 0, 1};
  if constexpr (NU == NV && NS == 0 && 2 * NV + 1 <= 64) {
    if constexpr (NV <= 8) k.ubwd = {unconstr_riccati_backward_kernel<NV>, 64, 0, 1};
    else k.ubwd = {unconstr_riccati_backward_lds_kernel<NV>, 64, 0, 1};
    k.ufwd = {unconstr_riccati_forward_kernel<NV>, 64, 0, 1};
  }
  if constexpr (NU == NV && NS == 0 && PbcCfg<NV>::OK) {
    k.pcoarse = {parnmpc_coarse_kernel<NV>, 64, 0, 1};
    k.pcorrect = {parnmpc_correct_kernel<NV>, PBC_CORRECT_NT, 0, 1};
  }
  k.ccond = {cone_condense_kernel<NV, NS>, 64, 0, 1};
  k.cexp = {cone_expand_kernel<NV, NS>, 64, 0, 1};
  k.wcond = {wrench_condense_kernel<NV, NS>, 64, 0, 1};
  k.wexp = {wrench_expand_kernel<NV, NS>, 64, 0, 1};
  constexpr int NF = NS;  // nf_max == ns_max for all supported robots
  k.cond = {condense_kernel<NV, NU, NF, NS>, CondCfg<NV, NU, NF, NS>::NT, CondCfg<NV, NU, NF, NS>::LDS_BYTES, 1};
  k.cond_split = {condense_kernel<NV, NU, NF, NS, true>, CondCfg<NV, NU, NF, NS>::NT, CondCfg<NV, NU, NF, NS, true>::LDS_BYTES, 1};
  k.mjt = {mjtjinv_kernel<NV, NU, NF, NS>, 64, MjCfg<NV, NF>::LDS_BYTES, 1};
  k.cond_fuses_cones = CondCfg<NV, NU, NF, NS>::FUSE ? 1 : 0;
  k.cond_fused_default = (CondCfg<NV, NU, NF, NS>::FUSE && CondCfg<NV, NU, NF, NS>::ITEMS >= 5) ? 1 : 0;
  if constexpr (CrvCfg<NV, NU, NF, NS>::OK) {
    k.cond_rv = {condense_rv_kernel<NV, NU, NF, NS>, 64, CrvCfg<NV, NU, NF, NS>::LDS_BYTES, 1};
    k.cond_rv_nc = {condense_rv_kernel<NV, NU, NF, NS, false>, 64, CrvCfg<NV, NU, NF, NS>::LDS_BYTES, 1};
    k.cond_rv_cones = CrvCfg<NV, NU, NF, NS>::CONES ? 1 : 0;
  }
  // regression guard for the occupancy the quadruped shape is sized for (condense.hpp: five / ten work items per CU)
  static_assert(!(NV == 18 && NU == 12 && NS == 12) ||
                    (CondCfg<NV, NU, NF, NS, true>::ITEMS >= 5 && CondCfg<NV, NU, NF, NS, true>::MIN_WAVES == 4 && MjCfg<NV, NF>::ITEMS >= 10),
                "LDS carve of the split condensation grew past its granule budget");
  k.expd = {expand_kernel<NV, NU, NF, NS>, 64, ExpCfg<NV, NU, NF>::LDS_BYTES, 1};
  k.scan_elt = {scan_element_kernel<NV, NU, NS>, SCAN_ELT_NT, scan::ElementCfg<NV, NU, NS>::LDS_BYTES, 1};
  k.scan_comb = {scan_combine_kernel<NV>, scan_comb_nt(NV), scan::CombineCfg<NV, scan_comb_nt(NV)>::LDS_BYTES, 1};
  k.scan_elt_stride = scan::EltLayout<NV>::STRIDE;
  k.scan_ps_stride = scan::EltLayout<NV>::PS_STRIDE;
  k.scan_ps_soff = scan::EltLayout<NV>::PS_S;
  k.scan_policy_variant = 1;  // NW1 waves share the tiles of the one stage
  k.fscan_elt = {fwd_scan_element_kernel<NV, NU, NS>, SCAN_FWD_NT, scan::FwdCfg<NV, NU>::LDS_BYTES, 1};
  k.fscan_comb = {fwd_scan_combine_kernel<NV, NU, NS>, SCAN_FWD_NT, scan::FwdCfg<NV, NU>::LDS_BYTES, 1};
  k.fscan_fin = {fwd_scan_finish_kernel<NV, NU, NS>, 64, 0, 1};
  k.sto_prep = {scan_sto_prep_kernel<NV, NU, NS>, SCAN_STO_PREP_NT, scan::StoPrepCfg<NV, NU, NS>::LDS_DOUBLES * (int)sizeof(double), 1};
  k.sto_vec = {scan_sto_vector_kernel<NV, NU, NS>, scan_sto_vec_nt(NV), scan::StoVecCfg<NV, NU, NS>::LDS_BYTES, 1};
  k.sto_scr_stride = scan::StoScratch<NV, NU, NS>::STRIDE;
  static_assert(scan::StoVecCfg<NV, NU, NS>::LDS_BYTES <= 160 * 1024, "the vector pass keeps one grid point's bundle in LDS");
  static_assert(scan::StoVecCfg<NV, NU, NS>::MAX_STAGES == SCAN_STO_MAX_STAGES, "the host's limit (kernel_args.hpp) is the kernel's grid table");
  static_assert(scan::CombineCfg<NV, scan_comb_nt(NV)>::LDS_BYTES <= 160 * 1024, "combination scratch must fit the LDS of a CU");
  return k;
}


}  // namespace rtoc
