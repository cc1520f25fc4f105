"""UnconstrParNMPCSolver::updateSolution closed on the device (rtoc_parnmpc_eval_kkt, rtoc_parnmpc_update_solution) for iiwa14:
(i) the pre-condensation records of the first iteration against the restated reference lines (tests/parnmpc_restatement.py),
(ii) convergence without limits on the reference's own test problem, (iii) with the six joint-limit components, (iv) the
refusals, (v) rtoc_clone."""
import ctypes as C

import numpy as np
import pytest

import parnmpc_restatement as pn
from robotoc_amd import capi, problems as pr, robot_model as rm
from robotoc_amd.types import BUF_CDD, BUF_CON, BUF_KKT, BUF_SOL, BUF_STEP, Dims, Records, joint_limit_rows
from test_unconstr_closed_loop import _limits

pytestmark = pytest.mark.gpu

# calls of updateSolution until the KKT error it reports is below 1e-8, on the reference's test problem without limits: measured by
# tests/test_parnmpc_restatement.py::test_restated_iteration_converges_on_the_reference_test_problem (it prints n_ref)
N_REF = 13


def _context(batch, N, cost, x0, dims=None):
    dims0 = pr.config_iiwa14()[0]
    dims = dims or dims0
    m = rm.load_named("iiwa14")
    ctx = capi.Context(dims, max(N, 2), batch, 0)
    ctx.parnmpc_set_horizon(N)
    ctx.set_robot_model(m)
    ctx.set_configuration_cost(**cost)
    ctx.set_initial_state(x0)
    return ctx, m


def _stage_dict(S, s, nv):
    return dict(q=S.f(s, "q")[:nv], v=S.f(s, "v"), a=S.f(s, "a"), u=S.f(s, "u"), lmd=S.f(s, "lmd"), gmm=S.f(s, "gmm"), beta=S.f(s, "beta"))


def _restated_stages(oracle, m, cost, dt, x0_b, S, sol_b):
    N, nv = sol_b.shape[0], m.nv
    st = [_stage_dict(S, sol_b[i], nv) for i in range(N)]
    return [pn.eval_stage(oracle, m, cost, dt, x0_b[:nv] if i == 0 else st[i - 1]["q"], x0_b[nv:] if i == 0 else st[i - 1]["v"], st[i],
                          st[i + 1] if i < N - 1 else None) for i in range(N)]


def test_parnmpc_eval_kkt_matches_the_restated_reference_lines(oracle):
    """tolerances: those of tests/test_unconstr_closed_loop.py::test_unconstr_eval_kkt_matches_the_restated_reference_lines"""
    batch, N, dt = 2, 3, 0.05
    rng = np.random.default_rng(0)
    nv = 7
    cost = dict(q_ref=rng.uniform(-0.8, 0.8, nv), v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0),
                v_weight=np.full(nv, 0.1), a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.001),
                q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 0.1))
    x0 = np.concatenate([rng.uniform(-0.5, 0.5, (batch, nv)), rng.uniform(-0.5, 0.5, (batch, nv))], axis=1)
    ctx, m = _context(batch, N, cost, x0)
    S, K, Cd = Records(ctx.L, "sol"), Records(ctx.L, "kkt"), Records(ctx.L, "cdd")
    sol = S.zeros(batch, N)
    for f in ("q", "v", "a", "u", "lmd", "gmm", "beta"):
        S.f(sol, f)[...] = rng.uniform(-1, 1, S.f(sol, f).shape)
    ctx.upload(BUF_SOL, sol)
    ctx.parnmpc_eval_kkt(dt)
    err = ctx.kkt_error()
    kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
    worst, acc = 0.0, np.zeros(batch)
    for b in range(batch):
        for i, e in enumerate(_restated_stages(oracle, m, cost, dt, x0[b], S, sol[b])):
            J = Cd.f(cdd[b, i], "dIDCdqv")
            got = [(np.diag(K.f(kkt[b, i], "Qxx")), e["Qxx_diag"], 1e-14), (K.f(kkt[b, i], "Fx"), e["Fx"], 1e-14), (K.f(kkt[b, i], "lx"), e["lx"], 1e-7),
                   (K.f(kkt[b, i], "lu"), e["la"], 1e-7), (Cd.f(cdd[b, i], "la"), e["lu"], 1e-14),
                   (K.f(kkt[b, i], "Quu"), np.diag(e["Qaa_diag"]), 1e-14), (Cd.f(cdd[b, i], "Qaa"), e["Quu_diag"], 1e-14),
                   (Cd.f(cdd[b, i], "IDC"), e["ID"], 1e-13), (J[:, :nv], e["Dq"], 1e-7), (J[:, nv:], e["Dv"], 1e-7), (Cd.f(cdd[b, i], "dIDda"), e["Da"], 1e-7),
                   (K.f(kkt[b, i], "Qxu"), np.zeros((2 * nv, nv)), 1e-14),
                   (K.f(kkt[b, i], "Qxx") - np.diag(np.diag(K.f(kkt[b, i], "Qxx"))), np.zeros((2 * nv, 2 * nv)), 1e-14)]
            acc[b] += e["kkt_error"]
            for g, x, tol in got:
                d = np.abs(np.asarray(g).reshape(np.asarray(x).shape) - x).max() / max(1.0, np.abs(x).max())
                worst = max(worst, d / tol)
                assert d < tol, (b, i, d, tol)
    assert np.allclose(err, np.sqrt(acc), rtol=1e-7)
    print("worst deviation / tolerance:", worst)
    ctx.close()


def test_parnmpc_converges_on_the_reference_test_problem(oracle):
    batch = 4
    cost, q0, v0, N, T = pn.reference_test_problem()
    dt, nv = T / N, 7
    rng = np.random.default_rng(77)
    x0 = np.array([np.concatenate([q0 + (0.0 if b == 0 else 1.0) * rng.uniform(-0.2, 0.2, nv), v0]) for b in range(batch)])
    ctx, m = _context(batch, N, cost, x0)
    S = Records(ctx.L, "sol")
    sol = S.zeros(batch, N)
    S.f(sol, "q")[..., :nv] = x0[:, None, :nv]   # setSolution("q", q), setSolution("v", v) of the reference's test
    ctx.upload(BUF_SOL, sol)
    ctx.parnmpc_init_backward_correction()
    hist = []
    for it in range(N_REF + 2):
        hist.append(ctx.parnmpc_update_solution(dt))
        if hist[-1].max() < 1e-8:
            break
    hist = np.array(hist)
    print("KKT error per iteration (worst instance):", ["%.2e" % e for e in hist.max(axis=1)])
    assert hist[-1].max() < 1e-8, hist[-1]
    assert (ctx.status() == 0).all()
    sol = ctx.download_records(BUF_SOL, "sol")
    worst = dict(Fx=0.0, ID=0.0, lx=0.0, la=0.0, lu=0.0)
    for b in range(batch):
        for e in _restated_stages(oracle, m, cost, dt, x0[b], S, sol[b]):
            for k in worst:
                worst[k] = max(worst[k], np.abs(e[k]).max())
    print("converged iterate, worst residuals by the CPU restatement:", worst)
    assert all(v < 1e-8 for v in worst.values()), worst
    ctx.close()


def _limits_problem(batch, N):
    nv = 7
    dims = Dims(nv, nv, 0, 0, 0, 48)
    rows = joint_limit_rows(dims)
    bounds = _limits(nv, rows)
    rng = np.random.default_rng(8)
    q_ref = rng.uniform(-0.5, 0.5, nv)
    q_ref[1], q_ref[4] = 0.9, -0.85   # beyond the +-0.6 position limits
    cost = dict(q_ref=q_ref, v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0), v_weight=np.full(nv, 0.1),
                a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.001), q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 0.1))
    x0 = np.concatenate([rng.uniform(-0.4, 0.4, (batch, nv)), np.zeros((batch, nv))], axis=1)
    ctx, m = _context(batch, N, cost, x0, dims)
    ctx.set_constraint_rows(rows)
    ctx.set_constraint_bounds(bounds, 1.0e-3, 0.995)
    S = Records(ctx.L, "sol")
    sol = S.zeros(batch, N)
    S.f(sol, "q")[..., :nv] = x0[:, None, :nv]
    ctx.upload(BUF_SOL, sol)
    ctx.parnmpc_init_constraints()
    ctx.parnmpc_init_backward_correction()
    return ctx, m, rows, cost, x0


def test_parnmpc_with_joint_limits_converges_inside_them(oracle):
    batch, N, dt, nv = 4, 20, 0.05, 7
    ctx, m, rows, cost, x0 = _limits_problem(batch, N)
    S, Nr = Records(ctx.L, "sol"), Records(ctx.L, "con")
    act = np.array([[(i + 2 if i < N - 1 else N) >= w.level for w in rows] for i in range(N)])
    hist = []
    for it in range(60):
        hist.append(ctx.parnmpc_update_solution(dt))
        steps = ctx.download(BUF_STEP, (batch, 2))
        assert (steps > 0.0).all() and (steps <= 1.0).all(), steps
        con = ctx.download_records(BUF_CON, "con")
        sl, du = Nr.f(con, "slack")[..., :len(rows)], Nr.f(con, "dual")[..., :len(rows)]
        assert (sl[:, act] > 0).all() and (du[:, act] > 0).all()
        if hist[-1].max() < 1e-9:
            break
    hist = np.array(hist)
    print("KKT error per iteration (worst instance):", ["%.1e" % e for e in hist.max(axis=1)])
    assert hist[-1].max() < 1e-8
    assert (ctx.status() == 0).all()
    sol = ctx.download_records(BUF_SOL, "sol")
    q, v, u = S.f(sol, "q")[..., :nv], S.f(sol, "v"), S.f(sol, "u")
    assert np.abs(q).max() < 0.6 and np.abs(v).max() < 1.5 and np.abs(u).max() < 60.0   # on all N records, the last included
    assert np.abs(sl[:, act] * du[:, act] - 1.0e-3).max() < 1e-8                        # complementarity of the barrier problem
    z = np.zeros(0)
    worst = max(np.abs(oracle.rbd_eval(m, 0, q[b, i], v[b, i], S.f(sol[b, i], "a"), z, u[b, i], 0, z)).max() for b in range(batch) for i in range(N))
    assert worst < 1e-8
    print("dynamics residual of the converged trajectory:", worst, " min slack:", sl[:, act].min())
    ctx.close()


def _refused(ctx, code, call):
    before = ctx.download_records(BUF_SOL, "sol")
    out = np.zeros(ctx.batch)
    rc = call(out)
    assert rc == code, (rc, code)
    assert np.array_equal(before, ctx.download_records(BUF_SOL, "sol"))


def test_parnmpc_refusals_leave_the_solution_alone():
    from robotoc_amd import costs
    lib = capi.lib()
    BAD_ARG, NOT_READY = -1, -5
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    upd = lambda c, dt: (lambda out: lib.rtoc_parnmpc_update_solution(c._h, dt, dp(out), c.batch))
    ev = lambda c, dt: (lambda out: lib.rtoc_parnmpc_eval_kkt(c._h, dt))
    batch, N, dt, nv = 2, 3, 0.05, 7
    cost, q0, v0, _, _ = pn.reference_test_problem()
    x0 = np.tile(np.concatenate([q0, v0]), (batch, 1))
    m = rm.load_named("iiwa14")
    dims = pr.config_iiwa14()[0]
    ctx = capi.Context(dims, N, batch, 0)
    S = Records(ctx.L, "sol")
    sol = S.zeros(batch, N)
    S.f(sol, "q")[..., :nv] = q0
    # before the horizon, the model, the cost, the initial state: RTOC_ERR_NOT_READY
    assert lib.rtoc_parnmpc_update_solution(ctx._h, dt, None, 0) == NOT_READY
    ctx.parnmpc_set_horizon(N)
    assert lib.rtoc_parnmpc_update_solution(ctx._h, dt, None, 0) == NOT_READY   # no solution either
    ctx.upload(BUF_SOL, sol)
    for setter in (lambda: ctx.set_robot_model(m), lambda: ctx.set_configuration_cost(**cost), lambda: ctx.set_initial_state(x0)):
        _refused(ctx, NOT_READY, upd(ctx, dt))
        _refused(ctx, NOT_READY, ev(ctx, dt))
        setter()
    # dt <= 0
    for bad_dt in (0.0, -0.05, float("nan")):
        _refused(ctx, BAD_ARG, upd(ctx, bad_dt))
        _refused(ctx, BAD_ARG, ev(ctx, bad_dt))
        _refused(ctx, BAD_ARG, lambda out: lib.rtoc_parnmpc_backward_correction(ctx._h, bad_dt))
    # what this mode leaves out: the line search, a configuration-reference table, task-space costs
    ctx.set_line_search(True)
    _refused(ctx, BAD_ARG, upd(ctx, dt))
    ctx.set_line_search(False)
    ctx.set_configuration_ref_table(np.tile(cost["q_ref"], (N, 1)))
    _refused(ctx, BAD_ARG, upd(ctx, dt))
    ctx.set_configuration_ref_table(None)
    hand = costs.TaskSpace3DCost("iiwa14", (6, [0.0, 0.0, 0.1]), np.array([0.3, 0.2, 0.8]))
    hand.set_weight([10.0, 10.0, 10.0])
    ctx.set_task_costs([hand])
    _refused(ctx, BAD_ARG, upd(ctx, dt))
    _refused(ctx, BAD_ARG, ev(ctx, dt))
    ctx.set_task_costs(None)
    assert lib.rtoc_parnmpc_update_solution(ctx._h, dt, None, 0) == 0   # and with all of it gone the call goes through
    # the entry points of a grid with a terminal point refuse the horizon
    ctx.upload(BUF_SOL, sol)
    _refused(ctx, BAD_ARG, lambda out: lib.rtoc_unconstr_update_solution(ctx._h, dt, dp(out), batch))
    _refused(ctx, BAD_ARG, lambda out: lib.rtoc_unconstr_eval_kkt(ctx._h, dt))
    _refused(ctx, BAD_ARG, lambda out: lib.rtoc_unconstr_backward(ctx._h, dt))
    _refused(ctx, BAD_ARG, lambda out: lib.rtoc_riccati_sweep(ctx._h))
    _refused(ctx, BAD_ARG, lambda out: lib.rtoc_contact_eval_kkt(ctx._h))
    # a grid of rtoc_set_grid ends the mode
    ctx.set_grid(pr.config_iiwa14()[1][:N - 1] + pr.config_iiwa14()[1][-1:])
    ctx.upload(BUF_SOL, sol)
    _refused(ctx, NOT_READY, upd(ctx, dt))
    ctx.close()
    # a shape with a free-flyer base and contacts (nu != nv): no horizon, and every entry point refuses
    quad = capi.Context(Dims(18, 12, 6, 12, 12, 0), 3, 1, 0)
    assert lib.rtoc_parnmpc_set_horizon(quad._h, 3) == BAD_ARG
    assert lib.rtoc_parnmpc_update_solution(quad._h, dt, None, 0) == BAD_ARG
    assert lib.rtoc_parnmpc_eval_kkt(quad._h, dt) == BAD_ARG
    assert lib.rtoc_parnmpc_backward_correction(quad._h, dt) == BAD_ARG
    quad.close()


def _clone(ctx):
    h = C.c_void_p()
    assert capi.lib().rtoc_clone(ctx._h, C.byref(h)) == 0
    n = object.__new__(capi.Context)
    n.__dict__.update(ctx.__dict__)
    n._h = h
    return n


def test_parnmpc_clone_continues_bit_identically():
    batch, N, dt = 2, 5, 0.05
    ctx, m, rows, cost, x0 = _limits_problem(batch, N)
    for it in range(2):
        ctx.parnmpc_update_solution(dt)
    cl = _clone(ctx)
    e0, e1 = ctx.parnmpc_update_solution(dt), cl.parnmpc_update_solution(dt)
    assert np.array_equal(e0, e1)
    assert np.array_equal(ctx.download_records(BUF_SOL, "sol"), cl.download_records(BUF_SOL, "sol"))
    assert np.array_equal(ctx.download_records(BUF_CON, "con"), cl.download_records(BUF_CON, "con"))
    assert np.array_equal(ctx.parnmpc_get_aux_mat(), cl.parnmpc_get_aux_mat())
    assert np.abs(ctx.parnmpc_get_aux_mat()[:, 1:]).max() > 0.0
    cl.close()
    ctx.close()
