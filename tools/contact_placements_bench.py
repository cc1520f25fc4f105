"""Per-instance contact placements at the bench size (ANYmal trot, batch x 46 grid points), for the record:
  * rtoc_linearize_contact_dynamics with the table the batch shares and with one table per instance (the same footholds in
    both: only the addressing differs), timed alternately in one process;
  * rtoc_hold_contact_placements over the whole grid beside the host path it replaces: RobotModel.frame_placement in a Python
    loop over the instances plus the upload through rtoc_set_contact_placements.
Wall clock around `reps` asynchronous launches, synchronised once, after a warm-up; three rounds each (no conclusion from one).
Usage: contact_placements_bench.py [batch] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from robotoc_amd import capi, problems as pr, robot_model as rm
from robotoc_amd.grid import ANYMAL_Q_STANDING
from robotoc_amd.types import BUF_SOL

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
m = rm.load_named("anymal")
dims, grids, _ = pr.config_anymal_trot()
n = len(grids)
ctx = capi.Context(dims, n, batch, 0)
ctx.set_grid(grids)
ctx.set_robot_model(m)
masks, flip = [], False
for g in grids:
    masks.append(0b1111 if g.dimf == 12 else 0 if g.dimf == 0 else (0b0110 if flip else 0b1001))
    flip = flip != (g.dimf == 6)
masks = np.array(masks, dtype=np.uint32)
rng = np.random.default_rng(0)
shared = rng.uniform(-0.5, 0.5, (n, 4, 3))
o = ctx.L.sol.off
one = np.zeros((64, n, ctx.L.sol.stride))
for b in range(64):
    for i in range(n):
        q, v, a = rm.random_configuration(m, rng, 0.8)
        one[b, i, o[0]:o[0] + m.nq], one[b, i, o[1]:o[1] + m.nv], one[b, i, o[2]:o[2] + m.nv] = q, v, a
        one[b, i, o[3]:o[3] + 12] = rng.uniform(-5, 5, 12)
        one[b, i, o[4]:o[4] + 12] = rng.uniform(-20, 20, 12)
ctx.upload(BUF_SOL, np.ascontiguousarray(np.tile(one, (batch // 64 + 1, 1, 1))[:batch]))
ctx.upload(0, np.zeros(ctx.shape("kkt")))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


out = {"batch": batch, "grid_points": n, "linearize_ms": {"shared": [], "per_instance": []}, "hold_ms": [], "host_path_ms": []}
ctx.set_contact_schedule(masks, shared)
for rnd in range(3):
    for mode in ("shared", "per_instance"):
        ctx.set_contact_placements(shared if mode == "shared" else np.ascontiguousarray(np.tile(shared[None], (batch, 1, 1, 1))))
        out["linearize_ms"][mode].append(timed(lambda: ctx.linearize_contact_dynamics(1), 10))
# ---- "where are this instance's feet now; hold them there" ----
x0 = np.zeros((batch, m.nq + m.nv))
x0[:, :m.nq] = ANYMAL_Q_STANDING
x0[:, 0:2] = rng.uniform(-5, 5, (batch, 2))
yaw = rng.uniform(-3, 3, batch)
x0[:, 5], x0[:, 6] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
ctx.set_initial_state(x0)
for rnd in range(3):
    out["hold_ms"].append(timed(lambda: ctx.hold_contact_placements(0b1111), 20))
dev = ctx.contact_placements()[0]
for rnd in range(3):
    t0 = time.perf_counter()
    feet = np.array([[m.frame_placement(x0[b, :m.nq], c)[1] for c in range(4)] for b in range(batch)])
    ctx.set_contact_placements(np.ascontiguousarray(np.tile(feet[:, None], (1, n, 1, 1))))
    ctx.sync()
    out["host_path_ms"].append((time.perf_counter() - t0) * 1e3)
out["hold_vs_host_max_abs_difference"] = float(np.abs(dev - ctx.contact_placements()[0]).max())
ctx.close()
print(json.dumps(out))
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    json.dump(out, open(sys.argv[2], "w"), indent=1)
