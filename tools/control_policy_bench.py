"""The feedback law of a batch at each instance's time: rtoc_control_input and rtoc_control_policy with device pointers (asynchronous)
and with host pointers (the result on the host at return), against the route a caller had before them -- rtoc_download of
RTOC_BUF_RIC and RTOC_BUF_SOL and the blend in numpy -- on the ANYmal trot grid at N = 40 (47 grid points), for 4096 instances and
for one.  The records are seeded random numbers (the same for every instance: the times do not depend on the values), the query
times are every instance's own, drawn over the horizon.
All routes are timed in ONE process after a warm-up, alternating round by round, with a host clock around work that ends in a
stream synchronise: a device-pointer call is enqueued `--calls` times and synchronised once (its time is the mean of those: the
rate at which a control loop can issue it), a host-pointer call and the download route synchronise themselves.  The numpy blend of
the download route is vectorised over the batch (one interval search per instance by searchsorted), not a Python loop.
Reported per batch: median, min and max over the rounds, and the ratio of the download route to each call.
usage: python tools/control_policy_bench.py [--batches 4096,1] [--rounds 5] [--calls 200] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
DEVICE_PTRS = 1
GRID_IMPACT = 1


def select_batch(types, tg, N, t):
    """ControlPolicy::set's choice of records (include/rtoc_robot.h) for many times at once: (a, b, alpha) with the policy
    alpha rec[a] + (1 - alpha) rec[b]; b = a and alpha = 1 where one record is taken.  N >= 3."""
    cand = np.arange(1, N - 1)
    hit = (t[:, None] < tg[cand][None]) & (types[cand - 1] != GRID_IMPACT)[None]
    found, i = hit.any(axis=1), cand[hit.argmax(axis=1)]
    front = t < tg[0]
    blend = found & ~front & (types[i] != GRID_IMPACT)
    back = N - 2 if types[N - 1] == GRID_IMPACT else N - 1
    a = np.where(front, 0, np.where(found, i - 1, back))
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(blend, (tg[i] - t) / (tg[i] - tg[i - 1]), 1.0)
    return a, np.where(blend, i, a), alpha


def main():
    import torch
    from robotoc_amd import capi, problems as pr
    from robotoc_amd.types import BUF_RIC, BUF_SOL, Records, control_policy_offsets
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi.build()
    lib = capi.lib()
    dims, grids, _ = pr.config_anymal_trot()
    n, N = len(grids), 40
    nv, nu, nq = dims.nv, dims.nu, dims.nv + 1
    off, stride = control_policy_offsets(nu)
    types = np.array([g.type for g in grids])
    tg = np.concatenate([[0.0], np.cumsum([g.dt for g in grids[:-1]])])
    out = {"problem": "anymal trot grid, N = 40, %d grid points" % n, "rounds": args.rounds, "calls_per_round": args.calls, "cases": []}
    for batch in [int(x) for x in args.batches.split(",") if x]:
        ctx = capi.Context(dims, n, batch)
        ctx.set_grid(grids)
        S, R = Records(ctx.L, "sol"), Records(ctx.L, "ric")
        rng = np.random.default_rng(7)
        sol1, ric1 = rng.normal(size=(n, S.stride)), rng.normal(size=(n, R.stride))
        for b in range(batch):
            ctx.upload(BUF_SOL, sol1, offset=b * sol1.size)
            ctx.upload(BUF_RIC, ric1, offset=b * ric1.size)
        t = rng.uniform(0.0, tg[N - 2], batch)
        x = rng.normal(size=(batch, nq + nv))
        td, xd = torch.tensor(t, device="cuda"), torch.tensor(x, device="cuda")
        pol_d = torch.empty((batch, stride), dtype=torch.float64, device="cuda")
        u_d = torch.empty((batch, nu), dtype=torch.float64, device="cuda")
        pol_h, u_h = np.empty((batch, stride)), np.empty((batch, nu))
        torch.cuda.synchronize()

        def chk(rc):
            if rc != 0:
                raise RuntimeError("rtoc error %d" % rc)

        def input_device():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                chk(lib.rtoc_control_input(ctx._h, 0.0, td.data_ptr(), 1, N, xd.data_ptr(), u_d.data_ptr(), batch, DEVICE_PTRS))
            ctx.sync()
            return (time.perf_counter() - t0) / args.calls

        def policy_device():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                chk(lib.rtoc_control_policy(ctx._h, 0.0, td.data_ptr(), 1, N, pol_d.data_ptr(), batch, DEVICE_PTRS))
            ctx.sync()
            return (time.perf_counter() - t0) / args.calls

        def input_host():
            t0 = time.perf_counter()
            chk(lib.rtoc_control_input(ctx._h, 0.0, t.ctypes.data, 1, N, x.ctypes.data, u_h.ctypes.data, batch, 0))
            return time.perf_counter() - t0

        def policy_host():
            t0 = time.perf_counter()
            chk(lib.rtoc_control_policy(ctx._h, 0.0, t.ctypes.data, 1, N, pol_h.ctypes.data, batch, 0))
            return time.perf_counter() - t0

        def download_route():
            """what a caller did before: both buffers across the host link, then ControlPolicy::set in numpy"""
            t0 = time.perf_counter()
            ric = ctx.download(BUF_RIC, (batch, n, R.stride))
            sol = ctx.download(BUF_SOL, (batch, n, S.stride))
            t1 = time.perf_counter()
            a, b, alpha = select_batch(types, tg, N, t)
            rows = np.arange(batch)
            sa, sb, ra, rb = sol[rows, a], sol[rows, b], ric[rows, a], ric[rows, b]
            w = alpha[:, None]
            mix = lambda p, q: w * p + (1.0 - w) * q
            Ka, Kb = R.f(ra, "K"), R.f(rb, "K")   # [batch, 2nv, nu]: K transposed
            res = dict(tauJ=mix(S.f(sa, "u"), S.f(sb, "u")), qJ=mix(S.f(sa, "q")[:, nq - nu:nq], S.f(sb, "q")[:, nq - nu:nq]),
                       dqJ=mix(S.f(sa, "v")[:, nv - nu:], S.f(sb, "v")[:, nv - nu:]),
                       Kp=w[:, None] * Ka[:, nv - nu:nv] + (1.0 - w[:, None]) * Kb[:, nv - nu:nv],
                       Kd=w[:, None] * Ka[:, 2 * nv - nu:] + (1.0 - w[:, None]) * Kb[:, 2 * nv - nu:])
            t2 = time.perf_counter()
            return t2 - t0, t1 - t0, res

        for _ in range(3):   # warm-up: code objects, lazy allocations, clocks
            input_device(), policy_device(), input_host(), policy_host()
        total, dl, res = download_route()
        # the routes agree (the download route's blend is held to the calls here, not timed for it)
        chk(lib.rtoc_control_policy(ctx._h, 0.0, t.ctypes.data, 1, N, pol_h.ctypes.data, batch, 0))
        kp = pol_h[:, off["Kp"]:off["Kp"] + nu * nu].reshape(batch, nu, nu)   # [b, column, row] = K^T like the download route's
        agree = float(np.abs(kp - res["Kp"]).max()), float(np.abs(pol_h[:, :nu] - res["tauJ"]).max())
        ms = {k: [] for k in ("control_input_device_ptrs", "control_policy_device_ptrs", "control_input_host_ptrs", "control_policy_host_ptrs",
                              "download_route", "download_route_copies")}
        for _ in range(args.rounds):   # alternating
            ms["control_input_device_ptrs"].append(1e3 * input_device())
            ms["control_policy_device_ptrs"].append(1e3 * policy_device())
            ms["control_input_host_ptrs"].append(1e3 * input_host())
            ms["control_policy_host_ptrs"].append(1e3 * policy_host())
            total, dl, _ = download_route()
            ms["download_route"].append(1e3 * total), ms["download_route_copies"].append(1e3 * dl)
        case = {"batch": batch, "ric_bytes": 8 * batch * n * R.stride, "sol_bytes": 8 * batch * n * S.stride,
                "bytes_read_per_instance_at_most": 8 * 2 * (3 * nu + 2 * nu * nu), "max_abs_difference_to_download_route": {"Kp": agree[0], "tauJ": agree[1]}}
        for k, v in ms.items():
            case[k + "_ms"] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
        for k in ("control_input_device_ptrs", "control_policy_device_ptrs", "control_input_host_ptrs", "control_policy_host_ptrs"):
            case["download_route_over_" + k] = float(np.median(ms["download_route"]) / np.median(ms[k]))
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
        ctx.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
