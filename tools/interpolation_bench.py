"""Re-gridding the warm start of a batch: the host path of OCPSolver._mesh_refinement (download of RTOC_BUF_SOL, OCPSolver._interpolate
in Python over instances and grid points, upload) against the device path (rtoc_solution_store + rtoc_solution_interpolate), on the
ANYmal jump with switching-time optimisation at N = 40.  Both paths are timed in ONE process, alternating repetition by
repetition, after a warm-up: a host clock around work that ends in a stream synchronise; the re-discretisation between the store
and the interpolation (the same for both) is outside the timed regions.  Every repetition goes from the grid of the plan's event
times to that of event times moved by 7 ms and 11 ms, so that grid points change phase and the events do not match.
Reported per batch: the median, min and max of the repetitions; for the device path the algorithmic bytes -- two stored records
read and one record written per new grid point -- and what share of the HBM peak (8 TB/s) they amount to over the interpolation
kernel's time (its launch and synchronise included, so a floor).
usage: python tools/interpolation_bench.py [--host-batches 1,64,1024] [--device-batches 1,64,1024,4096] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
HBM_PEAK = 8.0e12   # bytes / s


def main():
    from robotoc_amd import capi, problems_jump as pj
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-batches", default="1,64,1024")
    ap.add_argument("--device-batches", default="1,64,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps-large", type=int, default=1, help="repetitions of the host path at batch >= 1024 (seconds each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi.build()
    host_batches = [int(x) for x in args.host_batches.split(",") if x]
    device_batches = [int(x) for x in args.device_batches.split(",") if x]
    out = {"problem": "anymal jump with STO, N = 40", "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK, "cases": []}
    for batch in sorted(set(host_batches) | set(device_batches)):
        solver, x0, info = pj.anymal_jump_sto_solver(batch=batch, x0_noise=0.05 if batch > 1 else 0.0)
        c = solver.ctx
        events_a = solver.event_times.copy()
        events_b = events_a + np.array([0.007, 0.011])
        sol_a = solver.get_solution()
        sol_a += 0.01 * np.random.default_rng(3).normal(size=sol_a.shape) * (sol_a != 0.0)   # no two neighbours alike

        def side(events):
            solver.event_times = events.copy()
            solver.discretize(0.0)

        def start():
            side(events_a)
            solver.set_solution(sol_a)
            c.sto_correct_time_steps()
            c.sync()

        def device():
            start()
            t0 = time.perf_counter()
            c.solution_store(0.0)
            c.sync()
            t1 = time.perf_counter()
            side(events_b)
            c.sync()
            t2 = time.perf_counter()
            c.solution_interpolate(0.0)
            c.sync()
            t3 = time.perf_counter()
            return (t1 - t0) + (t3 - t2), t3 - t2

        def host():
            start()
            t0 = time.perf_counter()
            old_grids, old_masks, old_sol, old_dt = solver.grids, solver.masks, solver.get_solution(), c.sto_time_steps()
            t1 = time.perf_counter()
            side(events_b)
            c.sync()
            t2 = time.perf_counter()
            new_dt = c.sto_time_steps()
            new_sol = solver.S.zeros(batch, len(solver.grids))
            for b in range(batch):
                t_old = np.concatenate([[0.0], np.cumsum(old_dt[b, :-1])])
                t_new = np.concatenate([[0.0], np.cumsum(new_dt[b, :-1])])
                solver._interpolate(old_grids, old_masks, t_old, old_dt[b], old_sol[b], solver.grids, solver.masks, t_new, new_sol[b])
            solver.set_solution(new_sol)
            c.sync()
            t3 = time.perf_counter()
            return (t1 - t0) + (t3 - t2)

        run_host, run_device = batch in host_batches, batch in device_batches
        host_reps = args.host_reps_large if batch >= 1024 else args.reps
        for _ in range(2):   # warm-up: lazy allocations, clocks
            if run_device:
                device()
        if run_host and batch < 1024:
            host()
        d_ms, k_ms, h_ms = [], [], []
        for rep in range(args.reps):   # alternating
            if run_device:
                total, kernel = device()
                d_ms.append(1e3 * total), k_ms.append(1e3 * kernel)
            if run_host and rep < host_reps:
                h_ms.append(1e3 * host())
        n_new, stride = len(solver.grids), c.L.sol.stride
        side(events_a)
        case = {"batch": batch, "stored_grid_points": len(solver.grids), "new_grid_points": n_new, "record_doubles": stride}
        if run_device:
            nbytes = 3 * 8 * stride * n_new * batch
            case["device"] = {"store_plus_interpolate_ms": {"median": float(np.median(d_ms)), "min": min(d_ms), "max": max(d_ms)},
                              "interpolate_ms": {"median": float(np.median(k_ms)), "min": min(k_ms), "max": max(k_ms)},
                              "algorithmic_bytes": nbytes,
                              "share_of_hbm_peak": nbytes / (1e-3 * float(np.median(k_ms))) / HBM_PEAK}
        if run_host:
            case["host"] = {"download_interpolate_upload_ms": {"median": float(np.median(h_ms)), "min": min(h_ms), "max": max(h_ms)},
                            "repetitions": len(h_ms)}
        if run_host and run_device:
            case["device_not_slower"] = bool(np.median(d_ms) <= np.median(h_ms))
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
        solver.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    slow = [k["batch"] for k in out["cases"] if k.get("device_not_slower") is False and k["batch"] >= 1024]
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
