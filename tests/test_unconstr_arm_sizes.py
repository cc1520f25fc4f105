"""The fixed-base (UnconstrOCPSolver) path at arm sizes other than iiwa14's nv = 7, where its kernels take paths that 7 joints
never reach:

  nv =  8   the edge of the register form of the structured recursion (unconstr_riccati_backward_kernel: all 64 lanes hold an
            entry of Qaa, 17 solving lanes); a state that fills its 16-column tile, so no role-split general kernel
  nv =  9   the smallest (and an odd) size of the LDS form (unconstr_riccati_backward_lds_kernel), 81 > 64 entries of an
            nv x nv block: the second pass of every `e += 64` loop
  nv = 12   144 entries = 2.25 wavefronts, 72 joint-limit rows and 48 primal entries in unconstr_box_kernel
  nv = 16   nx = 32 is exactly two tiles, 96 rows, 64 primal entries = exactly one wavefront

The robots are tests/arm_models.py's chains (iiwa14 with copies of its own joints appended); the kernel sets are plugins
(capi.build_plugin).  Every bound is the one the iiwa14 test of the same quantity uses (named at each test)."""
import numpy as np
import pytest

from arm_models import extended_iiwa14
from helpers import check_parity, compare_direction, compare_riccati, rel_err
from robotoc_amd import problems as pr
from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import (BUF_CDD, BUF_CON, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP, Dims, Records, VAR_Q, VAR_U,
                               VAR_V, joint_limit_rows)
from test_gpu_parity import TOL
from test_unconstr_closed_loop import _limits
from test_unconstr_dynamics import _data

pytestmark = pytest.mark.gpu

SIZES = [8, 9, 12, 16]
DT = 0.05          # the iiwa14 configuration's time step (problems.config_iiwa14)
TOL_SCAN = 1e-8    # tests/test_scan_gpu.py


@pytest.fixture(scope="module")
def arm_plugins():
    from robotoc_amd import capi
    for nv in SIZES:
        capi.build_plugin(nv, nv, 0)
    return capi


# ---- a. the recursion ---------------------------------------------------------------------------------------------------------
def _recursion_case(capi, oracle, nv, steps, dense=False, scan=False, tol=TOL):
    dims, grids, batch = Dims(nv, nv, 0, 0, 0, 0), uniform_grid(steps, DT), 5
    n = len(grids)
    ctx = capi.Context(dims, n, batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_unconstr_dense(dense)
        ctx.set_backward_scan(scan)
        ctx.set_writeback(True)
        K = Records(L, "kkt")
        kkt = K.zeros(batch, n)
        for b in range(batch):
            pr.fill_unconstr_instance(L, n, kkt[b], np.random.default_rng(pr.BASE_SEED + b))
        dx0 = pr.make_dx0(L, batch)
        ctx.upload(BUF_KKT, kkt)
        ctx.upload(BUF_DX0, dx0)
        ctx.unconstr_backward(DT)
        ctx.unconstr_forward(DT)
        assert (ctx.status() == 0).all()
        ric, d, kkt_gpu = ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir"), ctx.download_records(BUF_KKT, "kkt")
        ric_ref, d_ref, kkt_ref = Records(L, "ric").zeros(batch, n), Records(L, "dir").zeros(batch, n), kkt.copy()
        oracle.unconstr_sweep_batch(L, n, DT, kkt_ref, ric_ref, d_ref, dx0=dx0)
        structured = not dense and not scan
        worst = 0.0
        for b in range(batch):
            worst = max(worst, compare_riccati(L, grids, ric[b], ric_ref[b], tol, "arm inst %d" % b))
            worst = max(worst, compare_direction(L, grids, d[b], d_ref[b], tol, "arm inst %d" % b))
            if structured:   # the mutated records as the reference leaves them in place
                for f in ("Qxx", "Qxu", "Quu", "lu"):
                    check_parity("writeback %s inst %d" % (f, b), rel_err(K.f(kkt_gpu[b, :-1], f), K.f(kkt_ref[b, :-1], f)), tol)
        print("nv = %d, %d steps (%s): worst rel err %.2e" % (nv, steps, "scan" if scan else "general kernels" if dense else "structured", worst))
        if structured:   # a Quu that is not positive definite: that instance's flag and no other
            ib, ist = 3, steps // 2
            bad = kkt.copy()
            K.f(bad[ib, ist], "Quu")[:] = -np.eye(nv)
            ctx.upload(BUF_KKT, bad)
            ctx.clear_status()
            ctx.unconstr_backward(DT)
            st = ctx.status()
            assert st[ib] != 0 and (np.delete(st, ib) == 0).all(), st
    finally:
        ctx.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("steps", [6, 1])
@pytest.mark.parametrize("nv", SIZES)
def test_arm_recursion_matches_the_oracle(arm_plugins, oracle, nv, steps, dense):
    """tests/test_gpu_parity.py::test_iiwa14_unconstr per size, horizons of 6 steps and of 1 (one backward stage next to the
    terminal copy): structured recursion (nv = 8 registers, 9 / 12 / 16 LDS) and the general kernels on materialised A, B, at 1e-9"""
    _recursion_case(arm_plugins, oracle, nv, steps, dense=dense)


def test_arm_recursion_through_the_scan_at_nine_joints(arm_plugins, oracle):
    """tests/test_scan_gpu.py::test_scan_iiwa14_unconstr_entry_points at nv = 9, the scan's 1e-8"""
    _recursion_case(arm_plugins, oracle, 9, 6, scan=True, tol=TOL_SCAN)


# ---- b. condensation / expansion ----------------------------------------------------------------------------------------------
def _oracle_direction(oracle, L, n, kkt, cdd, dx0):
    """condense -> sweep -> expand of the CPU oracle on copies of pre-condensation records"""
    kk = kkt.copy()
    oracle.unconstr_condense_batch(L, n, kk, cdd)
    condensed = kk.copy()
    ric, d = Records(L, "ric").zeros(kkt.shape[0], n), Records(L, "dir").zeros(kkt.shape[0], n)
    oracle.unconstr_sweep_batch(L, n, DT, kk, ric, d, dx0=dx0)
    oracle.unconstr_expand_batch(L, n, cdd, d, DT)
    return condensed, d


@pytest.mark.parametrize("nv", SIZES)
def test_arm_condensation_and_expansion_match_the_oracle(arm_plugins, oracle, nv):
    """tests/test_unconstr_dynamics.py::test_gpu_unconstr_iteration_matches_oracle per size: 1e-13 and 1e-9"""
    dims, grids, batch = Dims(nv, nv, 0, 0, 0, 0), uniform_grid(6, DT), 6
    n = len(grids)
    ctx = arm_plugins.Context(dims, n, batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        kkt, cdd = _data(L, n, batch)
        dx0 = pr.make_dx0(L, batch)
        for buf, arr in ((BUF_KKT, kkt), (BUF_CDD, cdd), (BUF_DX0, dx0)):
            ctx.upload(buf, arr)
        ctx.unconstr_condense()
        got = ctx.download_records(BUF_KKT, "kkt")
        ctx.unconstr_backward(DT)
        ctx.unconstr_forward(DT)
        ctx.unconstr_expand(DT)
        assert (ctx.status() == 0).all()
        d = ctx.download_records(BUF_DIR, "dir")
        kkt_ref, d_ref = _oracle_direction(oracle, L, n, kkt, cdd, dx0)
        dev = float((np.abs(got - kkt_ref) / (1e-13 + 1e-13 * np.abs(kkt_ref))).max())   # np.allclose(rtol = atol = 1e-13) as a number
        print("nv = %d: condensed records, worst deviation / allowance of allclose(1e-13): %.3f" % (nv, dev))
        assert np.allclose(got, kkt_ref, rtol=1e-13, atol=1e-13)
        D = Records(L, "dir")
        for f in ("dx", "du", "dlmdgmm", "daf", "dbetamu"):
            check_parity("iteration " + f, rel_err(D.f(d, f), D.f(d_ref, f)), 1e-9)
    finally:
        ctx.close()


# ---- c. evalKKT on the extended models ------------------------------------------------------------------------------------------
def _cost(nv, rng, lo=-0.8, hi=0.8):
    return dict(q_ref=rng.uniform(lo, hi, nv), v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0),
                v_weight=np.full(nv, 0.1), a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.001),
                q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 0.1))


def restated_eval_kkt(oracle, m, cost, dt, L, sol, x0, fd=True):
    """UnconstrOCPSolver's evalKKT up to the condensation in numpy, as tests/test_unconstr_closed_loop.py::
    test_unconstr_eval_kkt_matches_the_restated_reference_lines restates the reference's lines.  Returns per (instance, grid point)
    the list of (record, field, expected, bound) and the KKT error of every instance; the dynamics terms from the CPU rigid-body
    restatement, its Jacobians by central differences (fd) or the complex step."""
    S = Records(L, "sol")
    batch, n, nv = sol.shape[0], sol.shape[1], m.nv
    z, idx = np.zeros(0), np.arange(nv)
    out, acc = {}, np.zeros(batch)
    for b in range(batch):
        for i in range(n):
            s = sol[b, i]
            q, v, a, u = S.f(s, "q")[:nv], S.f(s, "v"), S.f(s, "a"), S.f(s, "u")
            lmd, gmm, beta = S.f(s, "lmd"), S.f(s, "gmm"), S.f(s, "beta")
            Qxx, lx = np.zeros((2 * nv, 2 * nv)), np.zeros(2 * nv)
            if i == n - 1:  # unconstr_terminal_stage.cpp: terminal cost + linearizeUnconstrForwardEulerTerminal
                lx[:nv] = cost["q_weight_terminal"] * (q - cost["q_ref"]) - lmd
                lx[nv:] = cost["v_weight_terminal"] * (v - cost["v_ref"]) - gmm
                Qxx[idx, idx] = cost["q_weight_terminal"]
                Qxx[nv + idx, nv + idx] = cost["v_weight_terminal"]
                out[b, i] = [("kkt", "Qxx", Qxx, 1e-14), ("kkt", "lx", lx, 1e-14)]
                acc[b] += lx @ lx
                continue
            sn = sol[b, i + 1]
            qn, vn, lmdn, gmmn = S.f(sn, "q")[:nv], S.f(sn, "v"), S.f(sn, "lmd"), S.f(sn, "gmm")
            ID = oracle.rbd_eval(m, 0, q, v, a, z, u, 0, z)
            Dq, Dv, Da = oracle.rbd_linearize_fd(m, 0, q, v, a, z, u, 0, z, 1e-6) if fd else oracle.rbd_linearize_cs(m, 0, q, v, a, z, u, 0, z)
            Fx = np.concatenate([q + dt * v - qn, v + dt * a - vn])                       # unconstr_state_equation.cpp:56-62
            lx[:nv] = dt * cost["q_weight"] * (q - cost["q_ref"]) + (lmdn - lmd) + dt * Dq.T @ beta   # :14, unconstr_dynamics.cpp:60
            lx[nv:] = dt * cost["v_weight"] * (v - cost["v_ref"]) + (dt * lmdn + gmmn - gmm) + dt * Dv.T @ beta
            la = dt * cost["a_weight"] * a + dt * gmmn + dt * Da.T @ beta
            lu = dt * cost["u_weight"] * (u - cost["u_ref"]) - dt * beta
            Qxx[idx, idx] = dt * cost["q_weight"]
            Qxx[nv + idx, nv + idx] = dt * cost["v_weight"]
            out[b, i] = [("kkt", "Qxx", Qxx, 1e-14), ("kkt", "Fx", Fx, 1e-14), ("kkt", "lx", lx, 1e-7), ("kkt", "lu", la, 1e-7),
                         ("cdd", "la", lu, 1e-14), ("kkt", "Quu", np.diag(dt * cost["a_weight"]), 1e-14),
                         ("cdd", "Qaa", dt * cost["u_weight"], 1e-14), ("cdd", "IDC", ID, 1e-13),
                         ("cdd", "dIDCdqv:q", Dq, 1e-7), ("cdd", "dIDCdqv:v", Dv, 1e-7), ("cdd", "dIDda", Da, 1e-7),
                         ("kkt", "Qxu", np.zeros((2 * nv, nv)), 1e-14)]
            acc[b] += Fx @ Fx + lx @ lx + la @ la + lu @ lu + ID @ ID   # split_kkt_residual.hxx:90-104 + UnconstrOCPData::KKTError
    dx0 = np.array([x0[b] - np.concatenate([S.f(sol[b, 0], "q")[:nv], S.f(sol[b, 0], "v")]) for b in range(batch)])
    return out, np.sqrt(acc), dx0


def _arm_context(capi, nv, steps, batch, seed, nc_max=0):
    m = extended_iiwa14(nv)
    dims, grids = Dims(nv, nv, 0, 0, 0, nc_max), uniform_grid(steps, DT)
    ctx = capi.Context(dims, len(grids), batch, 0)
    ctx.set_grid(grids)
    ctx.set_robot_model(m)
    rng = np.random.default_rng(seed)
    cost = _cost(nv, rng)
    ctx.set_configuration_cost(**cost)
    x0 = np.concatenate([rng.uniform(-0.5, 0.5, (batch, nv)), np.zeros((batch, nv))], axis=1)
    ctx.set_initial_state(x0)
    return ctx, m, grids, cost, x0, rng


@pytest.mark.parametrize("nv", SIZES)
def test_arm_eval_kkt_matches_the_restated_reference_lines(arm_plugins, oracle, nv):
    """tests/test_unconstr_closed_loop.py::test_unconstr_eval_kkt_matches_the_restated_reference_lines on the nv-joint chain (random
    iterate, 2 instances, 4 grid points) at its bounds -- 1e-14, 1e-13 for the inverse dynamics, 1e-7 where central differences
    enter --, then the direction of condense -> backward -> forward -> expand on those records against the oracle's at 1e-9."""
    batch = 2
    ctx, m, grids, cost, x0, rng = _arm_context(arm_plugins, nv, 3, batch, seed=nv)
    try:
        L, n = ctx.L, len(grids)
        S, K, C = Records(L, "sol"), Records(L, "kkt"), Records(L, "cdd")
        sol = S.zeros(batch, n)
        for f in ("q", "v", "a", "u", "lmd", "gmm", "beta"):
            S.f(sol, f)[...] = rng.uniform(-1, 1, S.f(sol, f).shape)
        ctx.upload(BUF_SOL, sol)
        ctx.unconstr_eval_kkt(DT)
        err = ctx.kkt_error()
        kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
        dx0 = ctx.download(BUF_DX0, (batch, 2 * nv))
        expect, err_ref, dx0_ref = restated_eval_kkt(oracle, m, cost, DT, L, sol, x0)
        assert np.allclose(dx0, dx0_ref, atol=1e-15)
        worst = {}
        for (b, i), items in expect.items():
            for which, f, e, tol in items:
                f, _, half = f.partition(":")   # dIDCdqv = [dID/dq | dID/dv]
                g = (K.f(kkt[b, i], f) if which == "kkt" else C.f(cdd[b, i], f))
                g = g[:, :nv] if half == "q" else g[:, nv:] if half == "v" else g
                dev = np.abs(np.asarray(g).reshape(np.asarray(e).shape) - e).max() / max(1.0, np.abs(e).max())
                worst[tol] = max(worst.get(tol, 0.0), dev)
                assert dev < tol, (b, i, f, dev, tol)
        for tol, w in worst.items():
            check_parity("records held to %.0e" % tol, w, tol)
        check_parity("kkt_error", float(np.abs(err / err_ref - 1.0).max()), 1e-7)
        # the Newton direction of these very records
        ctx.unconstr_condense()
        ctx.unconstr_backward(DT)
        ctx.unconstr_forward(DT)
        ctx.unconstr_expand(DT)
        assert (ctx.status() == 0).all()
        d = ctx.download_records(BUF_DIR, "dir")
        _, d_ref = _oracle_direction(oracle, L, n, kkt, cdd, dx0)
        D = Records(L, "dir")
        for f in ("dx", "du", "dlmdgmm", "daf", "dbetamu"):
            check_parity("direction " + f, rel_err(D.f(d, f), D.f(d_ref, f)), 1e-9)
    finally:
        ctx.close()


# ---- d. joint-limit rows past one wavefront -------------------------------------------------------------------------------------
def _arm_bounds(nv, rows):
    """tests/test_unconstr_closed_loop.py's symmetric limits, except the torque limits: +-1000 on the first four joints (never
    near), +-1 on the others -- with torques of the iterate in +-3 the rows that come closest to their boundary are torque rows of
    the joints 4..., i.e. rows >= 64 of the 6 nv (5 nv + 4 = 64 at nv = 12; all torque rows at nv = 16)."""
    bounds = _limits(nv, rows)
    for r, w in enumerate(rows):
        if w.var == VAR_U:
            bounds[r] = 1000.0 if w.index < 4 else 1.0
    return bounds


def _row_value(S, nv, s, w):
    return (S.f(s, "q")[:nv], S.f(s, "v"), S.f(s, "u"))[w.var][w.index]


@pytest.mark.parametrize("nv", [12, 16])
def test_arm_joint_limit_rows_past_one_wavefront(arm_plugins, oracle, nv):
    """72 and 96 joint-limit rows, 48 and 64 primal entries: unconstr_box_kernel's second pass in every mode.  INIT / LINEARIZE as
    tests/test_unconstr_closed_loop.py::test_unconstr_solver_with_joint_limits_converges_to_the_barrier_problem restates pdipm.hxx
    and joint_*_limit.cpp (1e-15 on the rows' data, 1e-12 on their share of lx and CDD.la); EXPAND and the update restated from
    the device's own direction at 1e-12, with the fraction-to-boundary step decided by a row >= 64; CONDENSE through the
    direction: the oracle's composition on records to which numpy added the rows' Hessian and gradient terms, 1e-9."""
    capi = arm_plugins
    batch, steps, barrier, tau = 3, 4, 1.0e-3, 0.995
    rows = joint_limit_rows(Dims(nv, nv, 0, 0, 0, 0))
    nr = len(rows)
    assert nr == 6 * nv and nr > 64
    bounds = _arm_bounds(nv, rows)
    ctx, m, grids, cost, x0, rng = _arm_context(capi, nv, steps, batch, seed=40 + nv, nc_max=nr)
    ctx0 = None
    try:
        L, n = ctx.L, len(grids)
        ctx.set_constraint_rows(rows)
        ctx.set_constraint_bounds(bounds, barrier, tau)
        ctx.set_line_search(False)
        S, K, C, N, D = Records(L, "sol"), Records(L, "kkt"), Records(L, "cdd"), Records(L, "con"), Records(L, "dir")
        sol = S.zeros(batch, n)
        S.f(sol, "q")[..., :nv] = x0[:, None, :nv] + rng.uniform(-0.3, 0.3, (batch, n, nv))   # some beyond the +-0.6 position limits
        for f, sc in (("v", 1.0), ("a", 1.0), ("u", 3.0), ("lmd", 0.5), ("gmm", 0.5), ("beta", 0.5)):
            S.f(sol, f)[...] = sc * rng.uniform(-1, 1, S.f(sol, f).shape)
        ctx.upload(BUF_SOL, sol)
        ctx.unconstr_init_constraints()
        ctx.unconstr_eval_kkt(DT)
        con = ctx.download_records(BUF_CON, "con")
        kkt1, cdd1 = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
        dx0 = ctx.download(BUF_DX0, (batch, 2 * nv))
        # the same iterate without rows: the difference is the rows' gradient
        ctx0 = capi.Context(Dims(nv, nv, 0, 0, 0, 0), n, batch, 0)
        ctx0.set_grid(grids)
        ctx0.set_robot_model(m)
        ctx0.set_configuration_cost(**cost)
        ctx0.set_initial_state(x0)
        L0 = ctx0.L
        sol0 = Records(L0, "sol").zeros(batch, n)
        for f in ("q", "v", "a", "u", "lmd", "gmm", "beta"):
            Records(L0, "sol").f(sol0, f)[...] = S.f(sol, f)
        ctx0.upload(BUF_SOL, sol0)
        ctx0.unconstr_eval_kkt(DT)
        kkt0, cdd0 = ctx0.download_records(BUF_KKT, "kkt"), ctx0.download_records(BUF_CDD, "cdd")
        K0, C0 = Records(L0, "kkt"), Records(L0, "cdd")
        # ---- INIT + LINEARIZE (pdipm.hxx:12-23, joint_*_limit.cpp) ----
        sb = np.sqrt(barrier)
        act = np.array([[i >= w.level for w in rows] for i in range(n - 1)])
        slack, dual = np.zeros((batch, n - 1, nr)), np.zeros((batch, n - 1, nr))
        resid, cmpl = np.zeros((batch, n - 1, nr)), np.zeros((batch, n - 1, nr))
        worst_rows = worst_share = 0.0
        clipped = 0
        for b in range(batch):
            for i in range(n - 1):
                dlx, dlu = np.zeros(2 * nv), np.zeros(nv)
                for r, w in enumerate(rows):
                    if not act[i, r]:
                        continue
                    g = w.sign * _row_value(S, nv, sol[b, i], w) - bounds[r]
                    slack[b, i, r] = max(-g, sb)
                    clipped += -g < sb
                    dual[b, i, r] = barrier / slack[b, i, r]
                    resid[b, i, r] = g + slack[b, i, r]
                    cmpl[b, i, r] = slack[b, i, r] * dual[b, i, r] - barrier
                    for f, e in (("slack", slack), ("dual", dual), ("residual", resid), ("cmpl", cmpl)):
                        worst_rows = max(worst_rows, abs(N.f(con[b, i], f)[r] - e[b, i, r]))
                    if w.var == VAR_U:
                        dlu[w.index] += w.sign * dual[b, i, r]
                    else:
                        dlx[(nv if w.var == VAR_V else 0) + w.index] += w.sign * dual[b, i, r]
                worst_share = max(worst_share, np.abs(K.f(kkt1[b, i], "lx") - K0.f(kkt0[b, i], "lx") - dlx).max(),
                                  np.abs(C.f(cdd1[b, i], "la") - C0.f(cdd0[b, i], "la") - dlu).max())
        assert clipped > 0   # rows of both kinds: inside their limit, and beyond it with the slack at sqrt(barrier)
        check_parity("slack, dual, residual, cmpl of the active rows", worst_rows, 1e-15)
        check_parity("the rows' share of lx and CDD.la", worst_share, 1e-12)
        # ---- one iteration, line search off ----
        ctx.unconstr_update_solution(DT)
        assert (ctx.status() == 0).all()
        d, con2 = ctx.download_records(BUF_DIR, "dir"), ctx.download_records(BUF_CON, "con")
        steps_gpu = ctx.download(BUF_STEP, (batch, 2))
        # EXPAND (pdipm.hxx:104-142) from the device's own direction
        dz = np.zeros((batch, n - 1, nr))
        for r, w in enumerate(rows):
            dz[:, :, r] = D.f(d, "du")[:, :n - 1, w.index] if w.var == VAR_U else D.f(d, "dx")[:, :n - 1, (nv if w.var == VAR_V else 0) + w.index]
        sign = np.array([w.sign for w in rows], dtype=float)
        dslack = np.where(act, -sign * dz - resid, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ddual = np.where(act, -(dual * dslack + cmpl) / slack, 0.0)
            fs = np.where(act, -tau * (slack / dslack), 1.0)
            fd = np.where(act, -tau * (dual / ddual), 1.0)
        fs = np.where((fs > 0.0) & (fs < 1.0), fs, 1.0).reshape(batch, -1)
        fd = np.where((fd > 0.0) & (fd < 1.0), fd, 1.0).reshape(batch, -1)
        steps_ref = np.stack([fs.min(axis=1), fd.min(axis=1)], axis=1)
        deciding = fs.argmin(axis=1) % nr, fd.argmin(axis=1) % nr
        print("nv = %d: steps %s, deciding rows primal %s dual %s" % (nv, steps_ref.tolist(), deciding[0], deciding[1]))
        assert (steps_ref[:, 0] < 1.0).all() and (deciding[0] >= 64).any()   # the second pass of r += 64 decides a step
        check_parity("fraction-to-boundary steps", float(np.abs(steps_gpu / steps_ref - 1.0).max()), 1e-12)
        a3 = act[None].repeat(batch, axis=0)
        sel = lambda rec, f: N.f(rec, f)[:, :n - 1, :nr][a3]   # noqa: E731
        check_parity("dslack", rel_err(sel(con2, "dslack"), dslack[a3]), 1e-12)
        check_parity("ddual", rel_err(sel(con2, "ddual"), ddual[a3]), 1e-12)
        check_parity("updated slack", rel_err(sel(con2, "slack"), (slack + steps_ref[:, None, None, 0] * dslack)[a3]), 1e-12)
        check_parity("updated dual", rel_err(sel(con2, "dual"), (dual + steps_ref[:, None, None, 1] * ddual)[a3]), 1e-12)
        assert (sel(con2, "slack") > 0.0).all() and (sel(con2, "dual") > 0.0).all()
        # CONDENSE (pdipm.hxx:60-75) through the direction
        kk, cc = kkt1.copy(), cdd1.copy()
        for b in range(batch):
            for i in range(n - 1):
                for r, w in enumerate(rows):
                    if not act[i, r]:
                        continue
                    hess = dual[b, i, r] / slack[b, i, r]
                    grad = w.sign * (dual[b, i, r] * resid[b, i, r] - cmpl[b, i, r]) / slack[b, i, r]
                    if w.var == VAR_U:
                        C.f(cc[b, i], "Qaa")[w.index] += hess
                        C.f(cc[b, i], "la")[w.index] += grad
                    else:
                        t = (nv if w.var == VAR_V else 0) + w.index
                        K.f(kk[b, i], "Qxx")[t, t] += hess
                        K.f(kk[b, i], "lx")[t] += grad
        _, d_ref = _oracle_direction(oracle, L, n, kk, cc, dx0)
        for f in ("dx", "du", "dlmdgmm", "daf", "dbetamu"):
            check_parity("direction with condensed rows " + f, rel_err(D.f(d, f), D.f(d_ref, f)), 1e-9)
    finally:
        ctx.close()
        if ctx0 is not None:
            ctx0.close()


# ---- e. the closed loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [9, 12])
def test_arm_solver_iterations_converge_on_the_device(arm_plugins, oracle, nv):
    """tests/test_unconstr_closed_loop.py::test_unconstr_solver_iterations_converge_on_the_device on the 9- and 12-joint chains, 8
    grid points: the reference's initial guess, at most 25 iterations to a KKT error below 1e-8, a clean status, and the
    converged trajectory's residuals by the CPU restatement below 1e-8."""
    batch = 8
    ctx, m, grids, cost, x0, rng = _arm_context(arm_plugins, nv, 7, batch, seed=3)
    try:
        L, n = ctx.L, len(grids)
        S = Records(L, "sol")
        sol = S.zeros(batch, n)
        S.f(sol, "q")[..., :nv] = x0[:, None, :nv]  # the initial state everywhere, all else zero
        ctx.upload(BUF_SOL, sol)
        hist = []
        for it in range(25):
            hist.append(ctx.unconstr_update_solution(DT))
            if hist[-1].max() < 1e-10:
                break
        hist = np.array(hist)
        print("nv = %d, KKT error per iteration (worst instance):" % nv, ["%.2e" % e for e in hist.max(axis=1)])
        assert hist[-1].max() < 1e-8 and len(hist) <= 25
        assert (ctx.status() == 0).all()
        sol = ctx.download_records(BUF_SOL, "sol")
        z = np.zeros(0)
        worst = dict(ID=0.0, Fx=0.0, x0=0.0)
        for b in range(batch):
            worst["x0"] = max(worst["x0"], np.abs(np.concatenate([S.f(sol[b, 0], "q")[:nv], S.f(sol[b, 0], "v")]) - x0[b]).max())
            for i in range(n - 1):
                s, sn = sol[b, i], sol[b, i + 1]
                q, v, a, u = S.f(s, "q")[:nv], S.f(s, "v"), S.f(s, "a"), S.f(s, "u")
                worst["ID"] = max(worst["ID"], np.abs(oracle.rbd_eval(m, 0, q, v, a, z, u, 0, z)).max())
                worst["Fx"] = max(worst["Fx"], np.abs(q + DT * v - S.f(sn, "q")[:nv]).max(), np.abs(v + DT * a - S.f(sn, "v")).max())
        print("converged trajectory, worst residuals by the CPU restatement:", worst)
        assert worst["ID"] < 1e-8 and worst["Fx"] < 1e-8 and worst["x0"] < 1e-8
    finally:
        ctx.close()
