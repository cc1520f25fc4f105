"""examples/anymal/trot.cpp closed on the device as the reference poses it: ConfigurationSpaceCost with the example's weights,
four TaskSpace3DCost foot costs with PeriodicSwingFootRef and a CoMCost with PeriodicCoMRef (weights 1e6), joint limits and
mu = 0.7 friction cones, t0 = 0.04, swing 0.5 s, double support 0.04 s, dt = 0.02 -- through solver.OCPSolver(task_costs=...).
Checks: convergence below the reference's default tolerance, the converged trajectory by the CPU restatement (inverse dynamics
with contact rows, state equation, switching constraints), swing feet at step_height near mid-swing, stance feet in place; then
the C++ shell (ConfigurationCostSource with the C++ cost classes) on the same problem reproduces the Python KKT history."""
import os
import subprocess

import numpy as np
import pytest

from robotoc_amd import costs, robot_model as rm
from robotoc_amd.grid import ANYMAL_Q_STANDING, Event
from robotoc_amd.robot_model import MAX_JOINTS
from robotoc_amd.solver import ContactPlan, OCPSolver, SolverOptions
from robotoc_amd.types import BUF_SOL, GRID_IMPACT, GRID_LIFT, Records

import task_cost_restatement as tr

STEP, HEIGHT, SWING, DS = np.array([0.15, 0.0, 0.0]), 0.1, 0.5, 0.04
T0 = DS
LIMITS = (9.42, 7.5, 80.0)   # symmetric joint limits (the model tables carry none)
MU, BARRIER = 0.7, 1.0e-3


def _trot_problem():
    m = rm.load_named("anymal")
    nv, nu = m.nv, m.nu
    qs = np.array(ANYMAL_Q_STANDING, dtype=float)
    feet = np.array([m.frame_placement(qs, c)[1] for c in range(4)])
    pos1 = feet.copy()
    pos1[[1, 2]] += 0.5 * STEP          # LH, RF
    pos2 = pos1.copy()
    pos2[[0, 3]] += STEP                # LF, RH
    plan = ContactPlan([0b1111, 0b1001, 0b1111, 0b0110, 0b1111], [feet, feet, pos1, pos1, pos2],
                       [Event("lift", T0), Event("impact", T0 + SWING), Event("lift", T0 + SWING + DS), Event("impact", T0 + 2 * SWING + DS)])
    T = T0 + 2 * DS + 2 * SWING
    N = int(T / 0.02)
    wq = np.array([0, 0, 0, 250000, 250000, 250000] + [0.0001] * 12)
    wv = np.array([100.0] * 6 + [1.0] * 12)
    wq_imp = np.array([1.0] * 6 + [100.0] * 12)
    cost = dict(q_ref=qs, v_ref=np.zeros(nv), u_ref=np.zeros(nu), q_weight=wq, v_weight=wv, a_weight=np.zeros(nv),
                u_weight=np.full(nu, 0.1), q_weight_terminal=wq, v_weight_terminal=wv, q_weight_impact=wq_imp,
                v_weight_impact=np.full(nv, 100.0), dv_weight_impact=np.zeros(nv))
    terms = []
    for k, (name, t0, half) in enumerate((("LF_FOOT", T0 + SWING + DS, False), ("LH_FOOT", T0, True), ("RF_FOOT", T0, True),
                                          ("RH_FOOT", T0 + SWING + DS, False))):
        c = costs.TaskSpace3DCost("anymal", name, costs.PeriodicSwingFootRef(feet[k], STEP, HEIGHT, t0, SWING, SWING + 2 * DS, half))
        c.set_weight(np.full(3, 1.0e6))
        terms.append(c)
    com = costs.CoMCost("anymal", costs.PeriodicCoMRef(tr.com(m, qs), 0.5 * STEP / SWING, T0, SWING, DS, True))
    com.set_weight(np.full(3, 1.0e6))
    terms.append(com)
    return m, plan, T, N, cost, terms, qs


def _solver():
    m, plan, T, N, cost, terms, qs = _trot_problem()
    nu = m.nu
    lim = (np.full(nu, -LIMITS[0]), np.full(nu, LIMITS[0]), np.full(nu, LIMITS[1]), np.full(nu, LIMITS[2]))
    solver = OCPSolver(m, plan, T, N, cost, joint_limits=lim, friction_coefficients=np.full(4, MU), barrier_param=BARRIER,
                       options=SolverOptions(), task_costs=terms)
    solver.discretize(0.0)
    S = Records(solver.ctx.L, "sol")
    sol = S.zeros(1, len(solver.grids))
    S.f(sol, "q")[..., :m.nq] = qs
    weight = 9.81 * sum(m.mass[i] for i in range(m.njoints))
    for i, g in enumerate(solver.grids):
        act = [k for k in range(4) if (int(solver.masks[i]) >> k) & 1]
        if act and g.type != GRID_IMPACT and i < len(solver.grids) - 1:
            S.f(sol, "f")[:, i, :3 * len(act)] = np.tile([0.0, 0.0, 0.25 * weight], len(act))
    solver.set_solution(sol)
    return solver, m, plan, cost, terms, qs, sol


def _positions(grids, plan):
    pos, phase = np.zeros((len(grids), 4, 3)), 0
    for i, g in enumerate(grids):
        if g.type in (GRID_IMPACT, GRID_LIFT):
            phase += 1
        pos[i] = plan.phase_positions[min(phase, len(plan.phase_positions) - 1)]
    return pos


@pytest.mark.gpu
def test_reference_trot_with_foot_and_com_costs_closes_on_the_device(oracle, tmp_path):
    solver, m, plan, cost, terms, qs, sol0 = _solver()
    nv, nq, nu = m.nv, m.nq, m.nu
    x0 = np.concatenate([qs, np.zeros(nv)])[None]
    st = solver.solve(0.0, x0)
    hist = np.array([e[0] for e in st.kkt_error])
    print("KKT error per iteration:", ["%.2e" % e for e in hist])
    assert st.convergence and hist[-1] < SolverOptions().kkt_tol and (solver.ctx.status() == 0).all()
    grids, masks = solver.grids, solver.masks
    times = solver.ctx.grid_times()[0]
    pos = _positions(grids, plan)
    S = Records(solver.ctx.L, "sol")
    sol = solver.get_solution()[0]
    n = len(grids)
    worst = dict(IDC=0.0, impact=0.0, switching=0.0, Fx=0.0)
    for i in range(n - 1):
        s, sn, g = sol[i], sol[i + 1], grids[i]
        q, v, a = S.f(s, "q")[:nq], S.f(s, "v"), S.f(s, "a")
        qn, vn = S.f(sn, "q")[:nq], S.f(sn, "v")
        r = oracle.rbd_eval(m, int(g.type == GRID_IMPACT), q, v, a, S.f(s, "f")[:12], S.f(s, "u")[:nu], int(masks[i]), pos[i].reshape(-1))
        key = "impact" if g.type == GRID_IMPACT else "IDC"
        worst[key] = max(worst[key], np.abs(r).max())
        if g.type == GRID_IMPACT:
            worst["Fx"] = max(worst["Fx"], np.abs(oracle.se3_difference(qn[:7], q[:7])).max(), np.abs(q[7:] - qn[7:]).max(), np.abs(v + a - vn).max())
        else:
            Fq = np.concatenate([oracle.se3_difference(qn[:7], q[:7]), q[7:] - qn[7:]]) + g.dt * v
            worst["Fx"] = max(worst["Fx"], np.abs(Fq).max(), np.abs(v + g.dt * a - vn).max())
        if g.switching_constraint:
            dt1, dt2 = g.dt, grids[i + 1].dt
            qp = oracle.rbd_integrate(m, q, (dt1 + dt2) * v + dt1 * dt2 * a)
            imp = [c for c in range(4) if (int(masks[i + 2]) >> c) & 1]
            worst["switching"] = max(worst["switching"], max(np.abs(oracle.rbd_contact_position(m, qp, c) - pos[i + 2, c]).max() for c in imp))
    print("converged trot with foot and CoM costs, worst residuals by the CPU restatement:", worst)
    assert worst["IDC"] < 1e-6 and worst["impact"] < 1e-6 and worst["Fx"] < 1e-7 and worst["switching"] < 1e-7
    # the swing feet follow their references: near mid-swing (the peak of PeriodicSwingFootRef) step_height above the ground
    for k, c in enumerate(terms[:4]):
        ref = c.ref
        rise = [oracle.rbd_contact_position(m, S.f(sol[i], "q")[:nq], k)[2] - ref.x3d0[2]
                for i in range(n - 1) if ref.is_active(times[i]) and abs(times[i] - (ref.t0 + 0.5 * SWING)) <= 0.021]
        assert rise and abs(max(rise) - HEIGHT) < 1e-2, (k, rise)
    for i in range(n - 1):   # the stance feet stay put
        q = S.f(sol[i], "q")[:nq]
        for c in range(4):
            if (int(masks[i]) >> c) & 1 and grids[i].type != GRID_IMPACT:
                assert np.abs(oracle.rbd_contact_position(m, q, c) - pos[i, c]).max() < 5e-3
    # ---- the C++ shell on the same problem ----
    from test_cpp_host import _build
    exe = _build("ocp_solver_trot_task_cost_test")
    cc = np.zeros((12, MAX_JOINTS))
    for k, key in enumerate(("q_ref", "v_ref", "u_ref", "q_weight", "v_weight", "a_weight", "u_weight", "q_weight_terminal", "v_weight_terminal",
                             "q_weight_impact", "v_weight_impact", "dv_weight_impact")):
        cc[k, :len(cost[key])] = cost[key]
    weight = 9.81 * sum(m.mass[i] for i in range(m.njoints))
    finit = np.zeros((n, 12))
    for i, g in enumerate(grids):
        act = [k for k in range(4) if (int(masks[i]) >> k) & 1]
        if act and g.type != GRID_IMPACT and i < n - 1:
            finit[i, :3 * len(act)] = np.tile([0.0, 0.0, 0.25 * weight], len(act))
    o = SolverOptions()
    prob = str(tmp_path / "trot_task_cost.bin")
    with open(prob, "wb") as f:
        f.write(bytes(m))
        f.write(cc.tobytes())
        f.write(np.array([n], dtype=np.int32).tobytes())
        for g in grids:
            f.write(bytes(g))
        f.write(np.ascontiguousarray(times, dtype=np.float64).tobytes())
        f.write(np.asarray(masks, dtype=np.uint32).tobytes())
        for arr in (pos, qs, np.zeros(nv), finit, np.array([LIMITS[0], LIMITS[1], LIMITS[2], MU, BARRIER, o.kkt_tol, o.max_iter])):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
        f.write(np.array([len(terms)], dtype=np.int32).tobytes())
        for t in terms:
            f.write(bytes(t.to_struct()))
    out_path = str(tmp_path / "trot_task_cost_out.bin")
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out_path)
    iters, conv, nh = int(raw[0]), raw[1], int(raw[2])
    chist = raw[3:3 + nh]
    print("C++ shell KKT error per iteration:", ["%.2e" % e for e in chist])
    assert conv == 1.0 and iters == st.iter and nh == len(hist)
    assert np.allclose(chist, hist, rtol=1e-9, atol=0.0), np.abs(chist / hist - 1).max()
    traj = raw[3 + nh:].reshape(n, nq)
    assert np.allclose(traj, S.f(sol, "q")[:, :nq], rtol=0.0, atol=1e-9)
