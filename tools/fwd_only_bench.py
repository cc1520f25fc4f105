#!/usr/bin/env python3
"""Forward recursion of one configuration alone (after one backward recursion), min / median of 30 timings: compares builds
of riccati_forward.hpp with other FWD_PREFETCH / FWD_WAVES_PER_SIMD, or another library (RTOC_HIP_LIB=...).
usage: fwd_only_bench.py [anymal_trot | anymal_jump_sto | iiwa14 | manipulator]
  anymal_trot / anymal_jump_sto: 4096 distinct instances (18:12:12); iiwa14: 4096 x 21 on the general kernels (7:7:0,
  RTOC_OPT_UNCONSTR_DENSE, as bench.py times it); manipulator: iiwa14 + one point contact (7:7:3), 4096 x 15 grid points."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from robotoc_amd import capi, problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import BUF_KKT, BUF_RIC, BUF_DX0, BUF_DIR, Dims, Records
cfg = sys.argv[1] if len(sys.argv) > 1 else "anymal_trot"
batch = 4096
dt = None
if cfg == "anymal_trot":
    dims, grids, _ = pr.config_anymal_trot()
elif cfg == "anymal_jump_sto":
    dims, grids, _ = pr.config_anymal_jump_sto()
elif cfg == "iiwa14":
    dims, grids, info = pr.config_iiwa14()
    dt = info["dt"]
elif cfg == "manipulator":
    dims = Dims(7, 7, 0, 3, 3, 48)
    cs = ContactSequence([3, 0, 3], [Event("lift", 0.07, sto=False), Event("impact", 0.15, sto=False, impact_dimf=3)])
    grids = discretize(14, 14 * 0.02, 0.0, cs)
else:
    sys.exit("unknown configuration " + cfg)
n = len(grids)
ctx = capi.Context(dims, n, batch, 0)
L = ctx.L
ctx.set_grid(grids)
z = lambda w: torch.zeros((batch, n, getattr(L, w).stride), dtype=torch.float64, device="cuda:0")
kkt = z("kkt")
if cfg == "iiwa14":
    k1 = Records(L, "kkt").zeros(1, n)
    pr.fill_unconstr_instance(L, n, k1[0], np.random.default_rng(1))
    kkt[...] = torch.from_numpy(k1).to("cuda:0")
elif cfg == "manipulator":
    kkt[...] = torch.from_numpy(pr.make_kkt_batch(L, grids, batch, mode="factory")).to("cuda:0")
else:
    pr.make_kkt_batch_unique(L, grids, batch, seed=0, backend="torch", device="cuda:0", out=kkt)
dx0 = pr.make_dx0_unique(L, batch, seed=0, backend="torch", device="cuda:0").contiguous()
ric, d = z("ric"), z("dir")
for b_, t_ in ((BUF_KKT, kkt), (BUF_DX0, dx0), (BUF_RIC, ric), (BUF_DIR, d)):
    ctx.bind(b_, t_.data_ptr())
torch.cuda.synchronize()
if cfg == "iiwa14":
    ctx.set_unconstr_dense(True)  # the general kernels, on the structured A, B materialised once
    ctx.unconstr_backward(dt)
ctx.riccati_backward(); ctx.sync()
for _ in range(5):
    ctx.riccati_forward()
ctx.sync()
t = sorted(ctx.time_phase(1, 1) for _ in range(30))
print("%s forward ms: min %.4f median %.4f  (status != 0: %d)" % (cfg, t[0], t[15], int((ctx.status() != 0).sum())))
ctx.close()
