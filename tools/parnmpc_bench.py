"""ms per iteration of rtoc_parnmpc_update_solution and of the backward correction alone (rtoc_parnmpc_backward_correction), with
rtoc_unconstr_update_solution on the same problem beside it: iiwa14, the cost of the reference's ParNMPC test, N = 20 and N = 80
(dt = 0.05), batch 1 and batch 4096.  HIP events on the launch stream, after warm-up, median of repeated runs of several
iterations each.  Every timed iteration restarts from the same iterate (the upload is outside the timed region), so that neither
solver is timed on a converged problem or a diverged one.
usage: python tools/parnmpc_bench.py [--batches 1,4096] [--horizons 20,80] [--reps 7] [--iters 5]   (prints one JSON document)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch
    import parnmpc_restatement as pn
    from robotoc_amd import capi, problems as pr, robot_model as rm
    from robotoc_amd.grid import uniform_grid
    from robotoc_amd.types import BUF_SOL, Records
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4096")
    ap.add_argument("--horizons", default="20,80")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    capi.build()
    torch.zeros(1, device="cuda:0")
    stream = torch.cuda.Stream()
    m = rm.load_named("iiwa14")
    nv, dt = m.nv, 0.05
    cost, q0, v0, _, _ = pn.reference_test_problem(nv)
    dims = pr.config_iiwa14()[0]
    out = {"dt": dt, "reps": args.reps, "iterations_per_rep": args.iters, "cases": []}

    def timed(fn, restart):
        """median over reps of (ms per call of fn), iters calls per rep"""
        ms = []
        for rep in range(args.reps + 2):   # the first two warm up (lazy allocations, clocks)
            restart()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(args.iters):
                    fn()
                e1.record(stream)
            e1.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1) / args.iters)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    for N in [int(x) for x in args.horizons.split(",")]:
        for batch in [int(x) for x in args.batches.split(",")]:
            rng = np.random.default_rng(5)
            x0 = np.concatenate([q0 + rng.uniform(-0.2, 0.2, (batch, nv)), np.tile(v0, (batch, 1))], axis=1)
            # ParNMPC: N stages
            pc = capi.Context(dims, max(N, 2), batch, 0)
            pc.set_stream(stream.cuda_stream)
            pc.parnmpc_set_horizon(N)
            pc.set_robot_model(m)
            pc.set_configuration_cost(**cost)
            pc.set_initial_state(x0)
            S = Records(pc.L, "sol")
            psol = S.zeros(batch, N)
            S.f(psol, "q")[..., :nv] = x0[:, None, :nv]

            def p_restart():
                pc.upload(BUF_SOL, psol)
                pc.parnmpc_init_backward_correction()
                pc.sync()
            t_upd = timed(lambda: pc.parnmpc_update_solution(dt, want_kkt_error=False), p_restart)
            p_restart()
            pc.parnmpc_eval_kkt(dt)
            pc.unconstr_condense()
            pc.sync()
            t_bc = timed(lambda: pc.parnmpc_backward_correction(dt), lambda: pc.sync())
            assert (pc.status() == 0).all()
            pc.close()
            # UnconstrOCPSolver's iteration on the same problem: N intervals, N + 1 grid points
            uc = capi.Context(dims, N + 1, batch, 0)
            uc.set_stream(stream.cuda_stream)
            uc.set_grid(uniform_grid(N, dt))
            uc.set_robot_model(m)
            uc.set_configuration_cost(**cost)
            uc.set_initial_state(x0)
            usol = Records(uc.L, "sol").zeros(batch, N + 1)
            Records(uc.L, "sol").f(usol, "q")[..., :nv] = x0[:, None, :nv]

            def u_restart():
                uc.upload(BUF_SOL, usol)
                uc.sync()
            t_ric = timed(lambda: uc.unconstr_update_solution(dt, want_kkt_error=False), u_restart)
            uc.close()
            keys = ("median_ms", "min_ms", "max_ms")
            out["cases"].append({"N": N, "batch": batch, "parnmpc_update_solution": dict(zip(keys, t_upd)),
                                 "parnmpc_backward_correction": dict(zip(keys, t_bc)), "unconstr_update_solution": dict(zip(keys, t_ric)),
                                 "kinv_bytes_per_stage": 16 * nv * nv * 8})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
