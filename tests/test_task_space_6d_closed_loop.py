"""The reference's examples/iiwa14/task_space_ocp.cpp closed on the device: robotoc::UnconstrOCPSolver (C++ shell) with a
ConfigurationSpaceCost and a TaskSpace6DCost on iiwa14's end-effector frame.  Leg 1: a constant reference -- the frame's
placement at a configuration q* near q0 -- solve() under default SolverOptions converges, the terminal |log6| error is
smaller than at q0, and the trajectory equals the same iterations driven through ctypes bit for bit.  Leg 2: the example's
circular reference, a user's object on both shells (a reference table on the device), for a fixed number of iterations:
bit for bit again, no convergence claim."""
import math
import os
import subprocess

import numpy as np
import pytest

from robotoc_amd import capi, costs, robot_model as rm
from robotoc_amd.grid import uniform_grid
from robotoc_amd.robot_model import MAX_JOINTS
from robotoc_amd.types import BUF_SOL, Records, iiwa14_dims

import task_cost_6d_restatement as t6

N, T, CIRCLE_ITERS = 20, 1.0, 5


class _Circle(costs.TaskSpace6DRefBase):
    """examples/iiwa14/task_space_ocp.cpp:27-57, with the C library's sin / cos as the C++ side calls them"""

    def __init__(self, rotm, pos0, radius):
        self.rotm, self.pos0, self.radius = rotm, pos0, radius

    def update_ref(self, g):
        pos = self.pos0.copy()
        pos[1] += self.radius * math.sin(math.pi * g.t)
        pos[2] += self.radius * math.cos(math.pi * g.t)
        return self.rotm, pos

    def is_active(self, g):
        return True


def _ctypes_solver(m, cost, q0, v0, term, dt):
    dims, grids = iiwa14_dims(), uniform_grid(N, dt)
    n, nv = len(grids), m.nv
    ctx = capi.Context(dims, n, 1, 0)
    ctx.set_grid(grids)
    ctx.set_robot_model(m)
    ctx.set_configuration_cost(*[cost[k, :nv] for k in range(9)])
    ctx.set_task_costs([term])
    times = [0.0 + i * dt for i in range(n)]
    ctx.set_grid_times(times)
    ctx.set_task_ref_tables([term], costs.grid_infos(times, [g.dt for g in grids]))
    ctx.set_initial_state(np.concatenate([q0, v0])[None])
    S = Records(ctx.L, "sol")
    sol = S.zeros(1, n)
    S.f(sol, "q")[..., :nv] = q0
    S.f(sol, "v")[...] = v0
    ctx.upload(BUF_SOL, sol)
    return ctx, S


def _trajectory(ctx, S, nv):
    sol = ctx.download_records(BUF_SOL, "sol")
    return np.concatenate([S.f(sol[0], "q")[:, :nv], S.f(sol[0], "v")], axis=1)


@pytest.mark.gpu
def test_unconstr_ocp_solver_tracks_an_end_effector_pose(tmp_path):
    from test_cpp_host import _build
    exe = _build("unconstr_task_space_ocp_test")
    m = rm.load_named("iiwa14")
    nv, n, dt = m.nv, N + 1, T / N
    rng = np.random.default_rng(31)
    q0 = np.array([0.0, 0.5 * np.pi, 0.0, 0.5 * np.pi, 0.0, 0.5 * np.pi, 0.0])   # the example's initial configuration
    v0 = np.zeros(nv)
    q_star = q0 + rng.uniform(-0.3, 0.3, nv)
    cost = np.zeros((12, MAX_JOINTS))
    cost[0, :nv] = q_star
    for k, w in ((3, 0.1), (4, 1e-4), (5, 1e-4), (7, 0.1), (8, 1e-4)):   # the example's weights: q, v, a, q terminal, v terminal
        cost[k, :nv] = w
    wp, wr = np.full(3, 1000.0), np.full(3, 1000.0)
    term = costs.TaskSpace6DCost("iiwa14", "iiwa_link_ee_kuka")
    R_star, p_star = t6.frame_placement(m, q_star, term.frame_parent, term.frame_p, term.frame_R)
    term.set_const_ref(p_star, R_star)
    term.set_weight(wp, wr)
    term.set_weight_terminal(wp, wr)
    R0, p0 = t6.frame_placement(m, q0, term.frame_parent, term.frame_p, term.frame_R)
    rotm, pos0, radius = R0, p0 - np.array([0.0, 0.0, 0.05]), 0.05   # the circle starts at the frame's placement at q0
    prob = str(tmp_path / "iiwa14_task_space.bin")
    with open(prob, "wb") as f:
        f.write(bytes(m))
        f.write(cost.tobytes())
        f.write(np.array([T]).tobytes())
        f.write(np.array([N], dtype=np.int32).tobytes())
        f.write(q0.tobytes())
        f.write(v0.tobytes())
        f.write(np.array([term.frame_parent], dtype=np.int32).tobytes())
        for a in (term.frame_R, term.frame_p, R_star, p_star, wp, wr, rotm, pos0, np.array([radius])):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(np.array([CIRCLE_ITERS], dtype=np.int32).tobytes())
    out_path = str(tmp_path / "task_space_out.bin")
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out_path)
    iters, conv, err, err0 = int(raw[0]), raw[1], raw[2], raw[3]
    print("UnconstrOCPSolver::solve with a TaskSpace6DCost: %d iterations, KKT error %.3e -> %.3e" % (iters, err0, err))
    assert conv == 1.0 and err < 1e-7   # SolverOptions' default kkt_tol
    traj = raw[4:4 + n * 2 * nv].reshape(n, 2 * nv)
    traj2 = raw[4 + n * 2 * nv:].reshape(n, 2 * nv)
    # the terminal pose error shrank
    e0 = np.linalg.norm(t6.log6(*t6.diff(m, q0, term.frame_parent, term.frame_p, term.frame_R, R_star, p_star)))
    eT = np.linalg.norm(t6.log6(*t6.diff(m, traj[-1, :nv], term.frame_parent, term.frame_p, term.frame_R, R_star, p_star)))
    print("|log6| of the end-effector error: %.3e at q0, %.3e at the end of the horizon" % (e0, eT))
    assert eT < e0
    # the same iterations through ctypes
    ctx, S = _ctypes_solver(m, cost, q0, v0, term, dt)
    errs = [ctx.unconstr_update_solution(dt)[0] for _ in range(iters)]
    assert abs(errs[0] - err0) <= 1e-12 * err0
    assert np.array_equal(traj, _trajectory(ctx, S, nv))
    ctx.close()
    # the circle: a user's reference object on both sides
    term.set_ref(_Circle(rotm, pos0, radius))
    ctx, S = _ctypes_solver(m, cost, q0, v0, term, dt)
    for _ in range(CIRCLE_ITERS):
        ctx.unconstr_update_solution(dt)
    assert np.array_equal(traj2, _trajectory(ctx, S, nv))
    assert not np.array_equal(traj2, traj)
    ctx.close()
