// kernel_table.hpp -- how the host runtime sees the kernels of ONE robot shape: a table of descriptors.  A descriptor (Kern) is
// the kernel's entry point WITH its launch geometry: block size, dynamic LDS, instances per workgroup.  make_set
// (kernel_set.hpp, compiled once per shape in shape_inst.hip) writes the three next to the kernel they belong to, and the host
// launches through the descriptor alone (rt_context.hpp: launch).  No kernel is declared here: the host units see the table and
// the argument blocks (kernel_args.hpp), never a kernel body.  Adding a kernel = a Kern member of KernelSet, a line in
// for_each_kernel (the static_assert below refuses the one without the other) and a statement in make_set.
#pragma once
#include <cstddef>

#include "kernel_args.hpp"

namespace rtoc {

template <class Args>
struct Kern {
  void (*fn)(Args);  // nullptr: not in this shape's kernel set
  int threads;       // block size
  int lds;           // dynamic LDS of a launch, bytes (what the kernel's own carve asks for; a launch may add to it)
  int inst;          // OCP instances per workgroup (1 except the four-instance role-split kernels)
  constexpr explicit operator bool() const { return fn != nullptr; }
};
// what a shape plugin must agree on with the runtime that loads it: the kernel-set table and every argument block
constexpr size_t kernel_abi_stamp() {
  size_t h = 1469598103934665603ull;
  const size_t parts[] = {sizeof(BwdArgs), sizeof(FwdArgs), sizeof(FillArgs), sizeof(UdArgs), sizeof(ConeArgs), sizeof(CondArgs),
                          sizeof(ExpArgs), sizeof(ScanArgs), sizeof(FwdScanArgs), sizeof(UrArgs), sizeof(StoScanArgs),
                          sizeof(PbcArgs), sizeof(Kern<BwdArgs>)};
  for (size_t v : parts) h = (h ^ v) * 1099511628211ull;
  return h;
}

// everything of a kernel set that is not a kernel
struct alignas(8) ShapeInfo {
  int nv, nu, ns;
  int nvariants;                      // entries of bwd[] this shape has
  rtoc_record_layout kl, rl, dl, cl;  // record layouts the kernels were compiled for
  int cond_fuses_cones;    // the one-kernel condensation condenses the friction / wrench cone rows itself (CondCfg::FUSE)
  int cond_fused_default;  // ... and is the default pipeline of this shape: five of its work items fit the LDS of a CU
  int cond_rv_cones;       // cond_rv condenses friction-cone rows of point contacts itself (CrvCfg::CONES)
  int scan_elt_stride, scan_ps_stride, scan_ps_soff;  // horizon scan: doubles per element / value record, offset of s
  int scan_policy_variant;                            // tile-split backward kernel used in its one-stage mode
  int sto_scr_stride;
};
// ... and the kernels: descriptors only (for_each_kernel)
struct KernelSet : ShapeInfo {
  Kern<BwdArgs> bwd[4];      // tile-split (0, 1) and role-split (2; 3: four instances per workgroup) kernels
  Kern<BwdArgs> bwd_sa;      // structured-Fxx form of variant 3, or null
  Kern<BwdArgs> bwd_rv;      // register-resident kernel, one wave per instance (riccati_backward_rv.hpp), or null
  Kern<BwdArgs> bwd_rv_sa;   // ... its structured-Fxx form, or null
  Kern<BwdArgs> bwd_rv_sto;  // ... the structured form for grids with switching-time optimisation, or null
  Kern<BwdArgs> bwd_rw;      // register-wide kernel of the iCub-size shapes, or null: 64 threads riccati_backward_rw_kernel (T = 4, one
                             // wave per instance and SIMD), 128 riccati_backward_rw2_kernel (T = 5, two waves per instance)
  Kern<FwdArgs> fwd;         // (a launch adds the grid table of its horizon to lds)
  Kern<FillArgs> fill;
  Kern<UdArgs> ucond, uexp;  // UnconstrDynamics condense / expand
  Kern<UrArgs> ubwd, ufwd;   // structured unconstrained Riccati recursion (unconstr_riccati.hpp); null unless nu == nv, ns == 0
  Kern<ConeArgs> ccond, cexp;  // friction-cone rows
  Kern<ConeArgs> wcond, wexp;  // contact-wrench-cone rows
  Kern<CondArgs> cond;
  Kern<CondArgs> cond_split, mjt;  // split condensation: MJtJinv kernel + the rest
  Kern<CondArgs> cond_rv;     // register-chained condensation of the contact grid points, one wave per work item (condense_rv.hpp), or null
  Kern<CondArgs> cond_rv_nc;  // ... without the cone-row code (contexts without cone rows)
  Kern<ExpArgs> expd;
  Kern<ScanArgs> scan_elt, scan_comb;                  // horizon scan of the backward recursion (riccati_scan.hpp)
  Kern<FwdScanArgs> fscan_elt, fscan_comb, fscan_fin;  // forward recursion as a prefix scan
  Kern<StoScanArgs> sto_prep, sto_vec;                 // scan on grids with switching-time optimisation (riccati_scan_sto.hpp)
  Kern<PbcArgs> pcoarse, pcorrect;  // ParNMPC backward correction (parnmpc_backward_correction.hpp); null unless nu == nv, ns == 0, 16 < 3nv <= 32, 2nv <= 16
};

// f(descriptor) for every kernel of the set, null ones included
template <class Set, class F>
constexpr void for_each_kernel(Set& k, F&& f) {
  for (auto& b : k.bwd) f(b);
  f(k.bwd_sa), f(k.bwd_rv), f(k.bwd_rv_sa), f(k.bwd_rv_sto), f(k.bwd_rw);
  f(k.fwd), f(k.fill), f(k.ucond), f(k.uexp), f(k.ubwd), f(k.ufwd);
  f(k.ccond), f(k.cexp), f(k.wcond), f(k.wexp);
  f(k.cond), f(k.cond_split), f(k.mjt), f(k.cond_rv), f(k.cond_rv_nc), f(k.expd);
  f(k.scan_elt), f(k.scan_comb), f(k.fscan_elt), f(k.fscan_comb), f(k.fscan_fin), f(k.sto_prep), f(k.sto_vec);
  f(k.pcoarse), f(k.pcorrect);
}
constexpr size_t kernels_visited() {
  KernelSet k{};
  size_t n = 0;
  for_each_kernel(k, [&n](const auto&) { ++n; });
  return n;
}
static_assert(sizeof(Kern<BwdArgs>) == sizeof(Kern<StoScanArgs>) && sizeof(KernelSet) == sizeof(ShapeInfo) + kernels_visited() * sizeof(Kern<BwdArgs>),
              "for_each_kernel must visit every descriptor of KernelSet (and KernelSet hold nothing else: plain fields go into ShapeInfo)");

}  // namespace rtoc
