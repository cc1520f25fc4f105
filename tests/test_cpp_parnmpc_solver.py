"""robotoc::UnconstrParNMPCSolver (robotoc_amd/host/robotoc_hip_unconstr_parnmpc_solver.hpp): compiles with g++ on the CPU; on the
GPU the reference's own test scenario (test/solver/unconstr_parnmpc_solver_test.cpp: iiwa14, N = 20, T = 1) converges through the
class, getSolution has N entries, a copy continues identically, the argument checks throw -- and the trajectory equals the same
iterations issued through ctypes bit for bit."""
import subprocess

import numpy as np
import pytest

import parnmpc_restatement as pn
from test_cpp_host import _build


def test_cpp_parnmpc_solver_compiles():
    import os
    assert os.path.exists(_build("unconstr_parnmpc_solver_test"))


def _write_problem(path, m, cost, T, N, q0, v0, rows=(), bounds=()):
    from robotoc_amd.robot_model import MAX_JOINTS
    nv = m.nv
    tab = np.zeros((12, MAX_JOINTS))
    for k, name in enumerate(("q_ref", "v_ref", "u_ref", "q_weight", "v_weight", "a_weight", "u_weight", "q_weight_terminal", "v_weight_terminal")):
        tab[k, :nv] = cost[name]
    with open(path, "wb") as f:
        f.write(bytes(m))
        f.write(tab.tobytes())
        f.write(np.array([T]).tobytes())
        f.write(np.array([N], dtype=np.int32).tobytes())
        f.write(np.asarray(q0, dtype=np.float64).tobytes())
        f.write(np.asarray(v0, dtype=np.float64).tobytes())
        f.write(np.array([len(rows)], dtype=np.int32).tobytes())
        for r in rows:
            f.write(bytes(r))
        f.write(np.asarray(bounds, dtype=np.float64).tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("limits", [False, True])
def test_cpp_parnmpc_solver_solves_the_reference_test_scenario(tmp_path, limits):
    from robotoc_amd import capi, problems as pr, robot_model as rm
    from robotoc_amd.types import BUF_SOL, Dims, Records, joint_limit_rows
    from test_unconstr_closed_loop import _limits
    exe = _build("unconstr_parnmpc_solver_test")
    m = rm.load_named("iiwa14")
    nv = m.nv
    cost, q0, v0, N, T = pn.reference_test_problem(nv)
    dims, rows, bounds = pr.config_iiwa14()[0], [], []
    if limits:   # the six joint-limit components, bounds of tests/test_unconstr_closed_loop.py, from an initial state inside them
        dims = Dims(nv, nv, 0, 0, 0, 48)
        rows = joint_limit_rows(dims)
        bounds = _limits(nv, rows)
        rng = np.random.default_rng(8)
        cost = dict(cost, q_ref=rng.uniform(-0.5, 0.5, nv), u_weight=np.full(nv, 0.001))
        q0 = rng.uniform(-0.4, 0.4, nv)
    prob, out_path = str(tmp_path / "parnmpc_problem.bin"), str(tmp_path / "parnmpc_out.bin")
    _write_problem(prob, m, cost, T, N, q0, v0, rows, bounds)
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out_path)
    iters, conv, err, err0 = int(raw[0]), raw[1], raw[2], raw[3]
    assert conv == 1.0 and err < 1e-7
    traj = raw[4:4 + N * 2 * nv].reshape(N, 2 * nv)
    # the same iterations through ctypes
    dt = T / N
    ctx = capi.Context(dims, N, 1, 0)
    ctx.parnmpc_set_horizon(N)
    ctx.set_robot_model(m)
    ctx.set_configuration_cost(**cost)
    ctx.set_initial_state(np.concatenate([q0, v0])[None])
    S = Records(ctx.L, "sol")
    sol = S.zeros(1, N)
    S.f(sol, "q")[..., :nv] = q0
    ctx.upload(BUF_SOL, sol)
    if limits:
        ctx.set_constraint_rows(rows)
        ctx.set_constraint_bounds(bounds, 1.0e-3, 0.995)
        ctx.parnmpc_init_constraints()
    ctx.parnmpc_init_backward_correction()
    errs = [ctx.parnmpc_update_solution(dt)[0] for _ in range(iters)]
    assert abs(errs[0] - err0) <= 1e-12 * err0 and errs[-1] == err
    sol = ctx.download_records(BUF_SOL, "sol")
    ref = np.concatenate([S.f(sol[0], "q")[:, :nv], S.f(sol[0], "v")], axis=1)
    assert np.array_equal(traj, ref)
    ctx.close()
