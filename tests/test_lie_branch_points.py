"""rbd::log6_fwd (robotoc_amd/csrc/rigid_body_math.hpp) through the C ABI at the branch points of its formula, against the
committed 50-digit fixture tests/golden/lie_branch_points.npz (tests/golden/make_lie_branch_points.py): rotation angle 0,
either side of 1e-6, 1e-3, the series threshold and the near-pi switch, pi - 1e-9 and the exact half turns.  The bound is
1e-13 max(1, |p|) for log6 and Jlog6; for an inverted Jacobian that times the fixture's condition number and the 2-norm of
the inverse.  An exact half turn has the two logarithms +-pi axis: there |w| = pi and exp3(w) = R are asserted, and the
Jacobians are compared with the reference at the sign the device returned.  Nothing here needs mpmath."""
import numpy as np
import pytest

from robotoc_amd import capi
from robotoc_amd.grid import anymal_trot_sequence, discretize
from robotoc_amd.types import BUF_CDD, BUF_DX0, BUF_KKT, BUF_SE3, BUF_SOL, Records, anymal_dims

from test_lie_branch_points_host import BOUND, expected, fx, quat_R, scale  # noqa: F401  (fx: the fixture, as a pytest fixture)


def _exp3(w):
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(t) / t * K + 2.0 * (np.sin(0.5 * t) / t) ** 2 * K @ K


def _anymal_three_grid_points():
    """ANYmal, two intermediate grid points of 0.02 s and the terminal one (the first event of the trot lies beyond them)"""
    grids = discretize(2, 0.04, 0.0, anymal_trot_sequence(t0=0.11, swing=0.2, double_support=0.1, cycles=1))
    assert len(grids) == 3
    return anymal_dims(), grids


class Worst:
    """the largest error / bound of a field, with the angle it occurred at"""

    def __init__(self):
        self.w = {}

    def add(self, field, err, bound, angle):
        r = float(err) / bound
        if not r <= self.w.get(field, (-1.0, 0.0))[0]:
            self.w[field] = (r, angle)

    def report(self, title):
        print(title + ": error / bound  " + "  ".join("%s %.2e (angle %.10g)" % (k, v[0], v[1]) for k, v in self.w.items()))

    def check(self):
        bad = {k: v for k, v in self.w.items() if not v[0] <= 1.0}
        assert not bad, bad


def _state_equation_runs(fx):
    """Linearisations of 3 grid points per fixture case, everything zero but the base poses and one unit multiplier entry
    (row r = 0..5), on one context.
    layout 'A': poses (F, I, I) -- X1 = F at grid point 0, X0 = F at grid point 1; the multiplier sits at grid point 1.
    layout 'B': poses (I, F, I) with x0 = F -- X0 = F at grid point 0 (dx0) and at the terminal one; the multiplier sits there.
    Returns {(layout, r): (Fx, Fxx, lx [batch, 3, ...], se3 [batch, 3, 72], dx0 [batch, 2 nv])}."""
    dims, grids = _anymal_three_grid_points()
    n, nv, batch = 3, dims.nv, len(fx["angle"])
    ctx = capi.Context(dims, n, batch, 0)
    out = {}
    try:
        L = ctx.L
        ctx.set_grid(grids)
        S, K = Records(L, "sol"), Records(L, "kkt")
        pose = np.concatenate([fx["pos"], fx["quat"]], axis=1)
        zk, zc = np.zeros(ctx.shape("kkt")), np.zeros(ctx.shape("cdd"))
        for layout in "AB":
            for r in range(6):
                sol = np.zeros(ctx.shape("sol"))
                q = S.f(sol, "q")
                q[..., 6] = 1.0
                q[:, 0 if layout == "A" else 1, :7] = pose
                S.f(sol, "lmd")[:, 1 if layout == "A" else 2, r] = 1.0
                x0 = np.zeros((batch, 2 * nv + 1))
                x0[:, :nv + 1] = q[:, 0]
                if layout == "B":
                    x0[:, :7] = pose
                ctx.upload(BUF_SOL, sol)
                ctx.upload(BUF_KKT, zk)
                ctx.upload(BUF_CDD, zc)
                ctx.set_initial_state(x0)
                ctx.linearize_state_equation()
                ctx.sync()
                kkt = ctx.download_records(BUF_KKT, "kkt")
                out[(layout, r)] = (K.f(kkt, "Fx").copy(), K.f(kkt, "Fxx")[..., :6, :6].copy(), K.f(kkt, "lx").copy(),
                                    ctx.download(BUF_SE3, (batch, n, 72)), ctx.download(BUF_DX0, (batch, 2 * nv)))
    finally:
        ctx.close()
    return out


@pytest.mark.gpu
def test_state_equation_at_the_branch_points(fx):
    """Fq, Fqq, Fqq_prev (read row by row through lx with unit multipliers), Fqq_inv, Fqq_prev_inv, the terminal record and the
    base part of dx0 of rtoc_linearize_state_equation with the fixture's placement as X1 resp. X0 (the other pose is the
    identity, so the relative placement is the fixture's up to the rounding of the quaternion -> rotation conversion).
    Observed on the MI355X, as error / bound: Fq 0.31, Fqq 0.26, Fqq_prev 0.26, the three inverses 0.075, dx0 0.030, all at angle
    3 (2.999), the old path just below the near-pi switch, where theta / (2 sin theta) amplifies the rounding of the rotation
    matrix 50-fold; every angle from the switch up to pi stays below 0.007, the half turns at 0.0044 (|w| - pi) and 0.0057
    (exp3(w) - R).  The device's acos and sin cost nothing visible: the float64 restatement on the CPU stands at the same 0.31
    (tests/test_lie_branch_points_host.py)."""
    n = len(fx["angle"])
    worst = Worst()
    runs = _state_equation_runs(fx)
    Fx, Fxx, _, se3A, _ = runs[("A", 0)]
    _, _, _, se3B, dx0 = runs[("B", 0)]
    for i in range(n):
        ang, b = fx["angle"][i], BOUND * scale(fx, i)
        got = Fx[i, 0, :6]
        assert np.isfinite(got).all()
        l6, J, J0, J0i = expected(fx, i, got[3:], ("log6", "jlog6", "dq0", "dq0_inv"))
        bi = b * fx["dq0_cond"][i] * fx["dq0_inv_norm"][i]
        if fx["half_turn"][i]:
            w = got[3:]
            worst.add("half turn |w| - pi", abs(np.linalg.norm(w) - np.pi), BOUND, ang)
            worst.add("half turn exp3(w) - R", np.abs(_exp3(w) - quat_R(fx["quat"][i])).max(), BOUND, ang)
        worst.add("Fq", np.abs(got - l6).max(), b, ang)
        worst.add("Fqq", np.abs(Fxx[i, 0] - J).max(), b, ang)
        worst.add("Fqq_inv", np.abs(se3A[i, 0, :36].reshape(6, 6).T - J0i).max(), bi, ang)
        # X0 = F: grid point 1 of layout A, grid point 0 and the terminal one of layout B.  The sign of a half turn is a
        # property of R, the same at every call site
        Fqq_prev = np.array([runs[("A", r)][2][i, 1, :6] for r in range(6)])
        Fqq_prev_T = np.array([runs[("B", r)][2][i, 2, :6] for r in range(6)])
        worst.add("Fqq_prev", np.abs(Fqq_prev - J0).max(), b, ang)
        worst.add("Fqq_prev terminal", np.abs(Fqq_prev_T - J0).max(), b, ang)
        worst.add("Fqq_prev_inv", np.abs(se3A[i, 1, 36:].reshape(6, 6).T - J0i).max(), bi, ang)
        worst.add("Fqq_prev_inv terminal", np.abs(se3B[i, 2, 36:].reshape(6, 6).T - J0i).max(), bi, ang)
        worst.add("Fqq_prev_inv grid 0", np.abs(se3B[i, 0, 36:].reshape(6, 6).T - J0i).max(), bi, ang)
        # dx0 (base) = -Fqq_prev_inv log6(X0): |d(inv l)| <= |d inv| |l|_1 + |inv|_inf |d l| <= bi (|l|_1 + sqrt 6)
        worst.add("dx0", np.abs(dx0[i, :6] + J0i @ l6).max(), bi * (np.abs(l6).sum() + np.sqrt(6.0)), ang)
        assert np.isfinite(se3A[i]).all() and np.isfinite(se3B[i]).all() and np.isfinite(dx0[i]).all()
    worst.report("state equation")
    worst.check()


@pytest.mark.gpu
def test_state_equation_with_identical_poses_is_exact():
    """Every pose identical (and exactly representable as a rotation: the identity, the half turn about z, both with a
    position): X is exactly the identity, so Fq = dt v bit for bit, Fqq = I, Fqq_prev = -I, their inverses too, no NaN."""
    dims, grids = _anymal_three_grid_points()
    n, nv, batch = 3, dims.nv, 2
    ctx = capi.Context(dims, n, batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        S, K = Records(L, "sol"), Records(L, "kkt")
        rng = np.random.default_rng(21)
        sol = rng.uniform(-1, 1, ctx.shape("sol"))
        q = S.f(sol, "q")
        q[0, :, :7] = [0.3, -1.7, 0.45, 0, 0, 0, 1]
        q[1, :, :7] = [-2.5, 0.125, 0.5, 0, 0, 1, 0]
        x0 = np.concatenate([q[:, 0], rng.uniform(-1, 1, (batch, nv))], axis=1)
        ctx.upload(BUF_SOL, sol)
        ctx.upload(BUF_KKT, np.zeros(ctx.shape("kkt")))
        ctx.upload(BUF_CDD, np.zeros(ctx.shape("cdd")))
        ctx.set_initial_state(x0)
        ctx.linearize_state_equation()
        ctx.sync()
        kkt = ctx.download_records(BUF_KKT, "kkt")
        se3 = ctx.download(BUF_SE3, (batch, n, 72))
        dx0 = ctx.download(BUF_DX0, (batch, 2 * nv))
        assert np.isfinite(kkt).all() and np.isfinite(se3).all() and np.isfinite(dx0).all()
        for b in range(batch):
            for i in range(n - 1):
                assert np.array_equal(K.f(kkt[b, i], "Fx")[:6], grids[i].dt * S.f(sol[b, i], "v")[:6])
                assert np.array_equal(K.f(kkt[b, i], "Fxx")[:6, :6], np.eye(6))
                assert np.array_equal(se3[b, i, :36].reshape(6, 6), -np.eye(6))
                # lx[:6] = Fqq^T lmd_next + Fqq_prev^T lmd = lmd_next - lmd
                assert np.array_equal(K.f(kkt[b, i], "lx")[:6], S.f(sol[b, i + 1], "lmd")[:6] - S.f(sol[b, i], "lmd")[:6])
            for i in range(n):
                assert np.array_equal(se3[b, i, 36:].reshape(6, 6), -np.eye(6))
            assert np.array_equal(K.f(kkt[b, n - 1], "lx")[:6], -S.f(sol[b, n - 1], "lmd")[:6])
            assert np.array_equal(dx0[b, :6], np.zeros(6))
    finally:
        ctx.close()


def _rows(fx, angles=(), quats=()):
    """fixture rows of the given angles, and the half turns with the given quaternions"""
    rows = [i for i in range(len(fx["angle"])) if not fx["half_turn"][i] and any(fx["angle"][i] == a for a in angles)]
    rows += [i for i in range(len(fx["angle"])) if fx["half_turn"][i] and any((fx["quat"][i] == np.array(q)).all() for q in quats)]
    return rows


@pytest.mark.gpu
def test_configuration_cost_base_block_at_the_branch_points(fx):
    """rtoc_contact_eval_kkt on ANYmal, 3 grid points: q_ref is the identity placement, the base sits at the fixture's, every
    multiplier, velocity and force is zero, so lq[:6] = s J^T W d and Qqq[:6, :6] = s J^T W J with d = log6, J = Jlog6 of the
    fixture, W the q weights of the grid point's kind and s = dt (1 at the terminal one).  Angles 0, 1.01e-3, pi - 1e-4 and the
    half turns about x and about z (the reversed heading).  With |dd|, |dJ| <= b = 1e-13 max(1, |p|), to first order
    |d lq| <= s b (sum_k W_k |d_k| + max_c sum_k W_k |J_kc|) and |d Qqq| <= 2 s b max_c sum_k W_k |J_kc| max|J|.
    Observed on the MI355X, as error / bound: lq 1.5e-3, Qqq 2.6e-3, both at pi - 1e-4."""
    from robotoc_amd import robot_model as rm
    from test_contact_force_cost import Q_STAND, _context
    rows = _rows(fx, (0.0, 1.01e-3, float(np.pi) - 1e-4), ([1.0, 0, 0, 0], [0, 0, 1.0, 0]))
    assert len(rows) >= 3 * 6 + 2
    m = rm.load_named("anymal")
    dims, grids = _anymal_three_grid_points()
    n, nv, batch = len(grids), m.nv, len(rows)
    ctx, _, S = _context(m, dims, grids, [0b1111] * n, batch, 1, q_center=Q_STAND)
    try:
        K = Records(ctx.L, "kkt")
        q_ref = np.array(Q_STAND, dtype=float)
        q_ref[:7] = [0, 0, 0, 0, 0, 0, 1]
        wq, wqT = np.linspace(1.0, 2.0, nv), np.linspace(2.0, 3.0, nv)
        ctx.set_configuration_cost(q_ref, np.zeros(nv), np.zeros(m.nu), wq, np.full(nv, 0.1), np.full(nv, 1e-3), np.full(m.nu, 1e-3), wqT,
                                   np.full(nv, 0.2), np.full(nv, 3.0), np.full(nv, 0.3), np.full(nv, 1e-2))
        sol = S.zeros(batch, n)
        q = S.f(sol, "q")
        q[..., :m.nq] = q_ref
        for b, i in enumerate(rows):
            q[b, :, :3], q[b, :, 3:7] = fx["pos"][i], fx["quat"][i]
        ctx.upload(BUF_SOL, sol)
        ctx.set_initial_state(np.concatenate([q[:, 0, :m.nq], np.zeros((batch, nv))], axis=1))
        ctx.contact_eval_kkt()
        ctx.sync()
        kkt = ctx.download_records(BUF_KKT, "kkt")
        assert np.isfinite(kkt).all()
        worst = Worst()
        for b, i in enumerate(rows):
            bd = BOUND * scale(fx, i)
            for st in range(n):
                W, s = (wqT[:6], 1.0) if st == n - 1 else (wq[:6], grids[st].dt)
                lq, Qqq = K.f(kkt[b, st], "lx")[:6], K.f(kkt[b, st], "Qxx")[:6, :6]
                # the sign of a half turn shows in the gradient: take the reference that the device's answer is nearer to
                cands = [(fx["log6"][i], fx["jlog6"][i])]
                if fx["half_turn"][i]:
                    k = list(fx["half_turn_rows"]).index(i)
                    cands.append((fx["log6_neg"][k], fx["jlog6_neg"][k]))
                d, J = min(cands, key=lambda c: np.abs(lq - s * c[1].T @ (W * c[0])).max())
                col = (W[:, None] * np.abs(J)).sum(axis=0).max()
                worst.add("lq", np.abs(lq - s * J.T @ (W * d)).max(), s * bd * ((W * np.abs(d)).sum() + col), fx["angle"][i])
                worst.add("Qqq", np.abs(Qqq - s * J.T @ (W[:, None] * J)).max(), 2 * s * bd * col * np.abs(J).max(), fx["angle"][i])
        worst.report("configuration cost, base block")
        worst.check()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_task_space_6d_cost_at_the_branch_points(fx):
    """TaskSpace6DCost on iiwa14, the unconstrained path, one term with a per-instance reference table: at grid point i of
    instance b the reference placement is oMf(q) F^-1 for fixture case F = b n + i, so that X_ref^-1 oMf = F up to the rounding
    of the products.  What the term adds to the records against lq = s JJ^T W d, Qqq = s JJ^T W JJ with d = log6, JJ = Jlog6
    J_frame: log6 and Jlog6 from the fixture, the LOCAL frame Jacobian from tests/task_cost_6d_restatement.py.  With |dd|,
    |dJlog6| <= b = 1e-13 max(1, |p|) and c = the largest column sum of |J_frame|, to first order
    |d lq| <= s b (c sum_k W_k |d_k| + max_col sum_k W_k |JJ_k,col|) and |d Qqq| <= 2 s b c max_col sum_k W_k |JJ_k,col|.
    The existing tests of tests/test_task_space_6d_cost.py keep their [0.1, pi - 0.1] and their bound.
    Observed on the MI355X, as error / bound: lq 0.059, Qqq 0.074, both at angle 2.999 (the old path below the near-pi switch)."""
    import task_cost_6d_restatement as t6
    from robotoc_amd import costs
    from test_task_space_6d_cost import EE, _TableRef, _eval_unconstr, _iiwa
    ncase = len(fx["angle"])
    N = 3
    n = N + 1
    batch = (ncase + n - 1) // n
    m, grids, times, ctx, sol, S, q_c, rng, dt = _iiwa(batch, N, seed=11)
    try:
        assert len(grids) == n
        infos = costs.grid_infos(times, [g.dt for g in grids])
        nv = m.nv
        terms, tables, case = [], [], {}
        for b in range(batch):
            t = costs.TaskSpace6DCost("iiwa14", EE)
            Rs, ps = [], []
            for i in range(n):
                c = (b * n + i) % ncase
                case[(b, i)] = c
                Rf, x = t6.frame_placement(m, S.f(sol[b, i], "q")[:nv], t.frame_parent, t.frame_p, t.frame_R)
                R_ref = Rf @ quat_R(fx["quat"][c]).T
                Rs.append(R_ref)
                ps.append(x - R_ref @ fx["pos"][c])
            t.set_ref(_TableRef(Rs, ps, [1] * n))
            t.set_weight([10.0, 20.0, 30.0], [1.0, 2.0, 3.0])
            t.set_weight_terminal([5.0, 6.0, 7.0], [0.5, 0.25, 0.7])
            terms.append([t])
            tables.append({0: t.ref_table(infos)})
        run = _eval_unconstr(dt)
        base = run(ctx)
        ctx.set_task_costs(terms, per_instance=True)
        ctx.set_task_ref_table(0, [tb[0] for tb in tables], per_instance=True)
        kkt = run(ctx)[0]
        assert np.isfinite(kkt).all()
        K = Records(ctx.L, "kkt")
        worst = Worst()
        for (b, i), c in case.items():
            t = terms[b][0]
            s, W = (1.0, t6.weights(t.to_struct(), "terminal")) if i == n - 1 else (dt, t6.weights(t.to_struct(), "stage"))
            Jf = t6.frame_jacobian_local(m, S.f(sol[b, i], "q")[:nv], t.frame_parent, t.frame_p, t.frame_R)
            lq = K.f(kkt[b, i], "lx")[:nv] - K.f(base[0][b, i], "lx")[:nv]
            Q = K.f(kkt[b, i], "Qxx")[:nv, :nv] - K.f(base[0][b, i], "Qxx")[:nv, :nv]
            cands = [(fx["log6"][c], fx["jlog6"][c])]
            if fx["half_turn"][c]:   # the sign of a half turn: the reference that the device's answer is nearer to
                k = list(fx["half_turn_rows"]).index(c)
                cands.append((fx["log6_neg"][k], fx["jlog6_neg"][k]))
            d, J = min(cands, key=lambda cd: np.abs(lq - s * (cd[1] @ Jf).T @ (W * cd[0])).max())
            JJ = J @ Jf
            bd, cs = BOUND * scale(fx, c), np.abs(Jf).sum(axis=0).max()
            col = (W[:, None] * np.abs(JJ)).sum(axis=0).max()
            worst.add("lq", np.abs(lq - s * JJ.T @ (W * d)).max(), s * bd * (cs * (W * np.abs(d)).sum() + col), fx["angle"][c])
            worst.add("Qqq", np.abs(Q - s * JJ.T @ (W[:, None] * JJ)).max(), 2 * s * bd * cs * col, fx["angle"][c])
        worst.report("TaskSpace6DCost")
        worst.check()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_surface_contact_rows_at_the_branch_points(fx, oracle):
    """rtoc_linearize_contact_dynamics on the iCub, both soles in contact, one intermediate grid point and the terminal one, batch
    1, v = a = 0 and the Baumgarte position gain set to 1: the contact rows are log6(X_desired^-1 X_sole) itself and their
    q-derivative is Jlog6 J_sole (LOCAL).  The desired placement is the actual one times F^-1 for fixture cases F of angle 1e-9
    and 1.01e-3 on both soles and pi - 1e-4 on one sole, and the actual one itself (|xi| = 0): there the rows are below 1e-14 and
    the Jacobian rows equal the oracle's local-frame Jacobian to 1e-13.  Elsewhere |rows - log6| <= b and
    |Jacobian rows - Jlog6 J| <= b c, b = 1e-13 max(1, |p|), c the largest column sum of |J|.
    Observed on the MI355X, as error / bound: rows at xi = 0 0.017 (1.7e-16), their Jacobian 0.010 (1.0e-15), rows 0.012 at
    1.01e-3, Jacobian rows 0.0063 at pi - 1e-4."""
    from robotoc_amd import robot_model as rm
    from robotoc_amd.types import Dims, Grid, GRID_INTERMEDIATE, GRID_TERMINAL
    m = rm.load_named("icub")
    for c in range(2):
        m.contact_kp[c] = 1.0
    dims = Dims(35, 29, 6, 12, 12, 0)
    grids = [Grid(GRID_INTERMEDIATE, 0, 0, 0, 12, 0, 1, 0, 0.02), Grid(GRID_TERMINAL, 0, 0, 0, 0, 0, 1, 1, 0.0)]
    masks = np.array([0b11, 0], dtype=np.uint32)
    ctx = capi.Context(dims, 2, 1, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_robot_model(m)
        rng = np.random.default_rng(9)
        q = rm.random_configuration(m, rng, 0.6)[0]
        nv, ldv, nfm = m.nv, dims.nv + dims.nf_max, dims.nf_max
        o, co = L.sol.off, L.cdd.off
        sol = np.zeros(ctx.shape("sol"))
        sol[0, :, o[0]:o[0] + m.nq] = q
        ctx.upload(BUF_SOL, sol)
        place = [oracle.rbd_contact_placement(m, q, c) for c in range(2)]
        zero = np.zeros(12)
        Jloc = oracle.rbd_linearize_cs(m, False, q, np.zeros(nv), np.zeros(nv), zero, np.zeros(m.nu), 0b11,
                                       np.array([p for _, p in place]).reshape(-1), rref=np.array([R for R, _ in place]).reshape(2, 9))[2][nv:]
        small = _rows(fx, (1e-9, 1.01e-3))
        near_pi = _rows(fx, (float(np.pi) - 1e-4,))
        pairs = [(None, None)] + [(small[k], small[k + 1]) for k in range(0, len(small) - 1, 2)] + [(i, None) for i in near_pi]
        worst = Worst()
        for pair in pairs:
            pos, rot = np.zeros((2, 2, 3)), np.zeros((2, 2, 3, 3))
            for c, i in enumerate(pair):
                Rw, pw = place[c]
                if i is None:
                    rot[:, c], pos[:, c] = Rw, pw
                else:
                    Rd = Rw @ quat_R(fx["quat"][i]).T
                    rot[:, c], pos[:, c] = Rd, pw - Rd @ fx["pos"][i]
            ctx.set_contact_schedule(masks, pos, rot)
            ctx.upload(BUF_CDD, np.full(ctx.shape("cdd"), np.nan))
            ctx.linearize_contact_dynamics()
            ctx.sync()
            rec = ctx.download(BUF_CDD, ctx.shape("cdd"))[0, 0]
            D = rec[co[1]:co[1] + ldv * 2 * nv].reshape(2 * nv, ldv).T
            for c, i in enumerate(pair):
                rows, Jrows, J = rec[co[3] + nv + 6 * c:co[3] + nv + 6 * c + 6], D[nv + 6 * c:nv + 6 * c + 6, :nv], Jloc[6 * c:6 * c + 6]
                assert np.isfinite(rows).all() and np.isfinite(Jrows).all()
                if i is None:
                    worst.add("rows at xi = 0", np.abs(rows).max(), 1e-14, 0.0)
                    worst.add("Jacobian rows at xi = 0", np.abs(Jrows - J).max(), 1e-13, 0.0)
                else:
                    bd = BOUND * scale(fx, i)
                    worst.add("rows", np.abs(rows - fx["log6"][i]).max(), bd, fx["angle"][i])
                    worst.add("Jacobian rows", np.abs(Jrows - fx["jlog6"][i] @ J).max(), bd * np.abs(J).sum(axis=0).max(), fx["angle"][i])
        worst.report("surface contacts")
        worst.check()
    finally:
        ctx.close()
