// fxx_structure.hpp -- the device check behind RTOC_OPT_FXX_STRUCTURE = 0 (auto).  A runtime kernel (not per shape): rt_sweep.hip
// launches it and is the one unit that includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "record_view.hpp"

namespace rtoc {

struct FxxCheckArgs {
  RecView rv;
  int* flag;
};

// Does every Fxx of the batch have the structure the SA kernels assume (see riccati_backward_rs_body)?  One wave per
// (instance, grid point); any violation sets *flag.  Reads the top NV rows of Fxx only (~1 GB per 4096 x 47 ANYmal
// records: 0.2 ms), run once per upload of the KKT records, not per sweep.
static __global__ __launch_bounds__(64) void fxx_structure_kernel(FxxCheckArgs a) {
  const int item = blockIdx.x, nst1 = a.rv.nstages - 1;
  const int b = item / nst1, st = item % nst1;
  if (b >= a.rv.batch) return;
  const int nv = a.rv.nv(), nx = 2 * nv, np = a.rv.L.dims.np;
  const double* A = a.rv.kkt_at((size_t)b * a.rv.nstages + st) + a.rv.kkt_off(RTOC_KKT_FXX);  // column-major nx x nx
  const double ca = A[np + (size_t)np * nx], cc = A[np + (size_t)(nv + np) * nx];
  bool bad = false;
  for (int e = threadIdx.x; e < nv * nx; e += 64) {
    const int i = e % nv, j = e / nv;  // rows [0, nv) of column j
    const double v = A[i + (size_t)j * nx];
    if (i < np) {
      const bool corner = j < np || (j >= nv && j < nv + np);
      if (!corner && v != 0.0) bad = true;
    } else {
      const double want = (j == i) ? ca : ((j == nv + i) ? cc : 0.0);
      if (v != want) bad = true;
    }
  }
  if (__any(bad) && threadIdx.x == 0) atomicOr(a.flag, 1);
}

}  // namespace rtoc
