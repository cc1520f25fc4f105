"""The SE(3) exponential of the free-flyer base on the device -- integrate_solution_kernel (M <- M exp6(step dq_b)) and
switching_constraint_lin_kernel (q+ = q (+) dq, Tq = Ad_{exp6}^-1, Jr = Jexp6) -- through the C ABI at the branch points of
its formula, against the committed 50-digit fixture tests/golden/lie_exp_branch_points.npz
(tests/golden/make_lie_exp_branch_points.py): rotation angle 0, either side of 1e-10, 1e-8 and 1e-3, the range [1e-8, 1e-4] in
which (1 - cos t) / t^2 cancels, up to pi - 1e-3, and 4.0 for the integration.  Translations are held to 1e-13 max(1, |p0|, |v|),
the integrated quaternion to QUAT_BOUND (measured on the float64 restatement of tests/test_lie_exp_branch_points_host.py, never
on the device), the transported Jacobians to 1e-13 max(1, |v|) times the largest column sum of |Pq|, and where Jlog6 is
inverted that times the fixture's condition number and the 2-norm of the inverse.  Nothing here needs mpmath."""
import numpy as np
import pytest

from robotoc_amd import capi, robot_model as rm
from robotoc_amd.grid import ContactSequence, Event, contact_masks, discretize
from robotoc_amd.types import BUF_CDD, BUF_DIR, BUF_KKT, BUF_SOL, BUF_STEP, GRID_IMPACT, Records, anymal_dims

from test_lie_branch_points import Worst, _anymal_three_grid_points
from test_lie_branch_points_host import BOUND
from test_lie_exp_branch_points_host import QUAT_BOUND, UNIT_BOUND, fxe, vscale  # noqa: F401  (fxe: the fixture, as a pytest fixture)
from test_switching_constraint_lin import Q_STAND


@pytest.mark.gpu
def test_integrate_solution_at_the_branch_points(fxe):
    """rtoc_integrate_solution on ANYmal, 3 grid points, one instance per fixture case: the base of every record is the
    placement M0 (the identity, then a random one with |p0| = 10), everything else is random, and the base direction is xi with
    a full step resp. 2 xi with a half step -- step x dx is xi bit for bit either way.  q[:3] and q[3:7] against M0 exp6(xi)
    composed at 50 digits (the same Hamilton product: no sign ambiguity), the two runs against each other, |quat| - 1, every
    Euclidean member against s + step d at 1e-15 as tests/test_integrate_solution.py holds them, and v = 0 from the identity
    leaving the position untouched.
    Observed on the MI355X, as error / bound: position 0.0036 at 1.01e-10, quaternion 0.22 (2.2e-16) and |quat| - 1 0.56
    (2.2e-16) at 1.01e-3; the half step and the full step agree bit for bit.  Before the repair of the coefficients the position
    stood at 4.08e+04 at 1.01e-8, the figure of the float64 formula on the CPU, which is over the bound at every angle from
    1.01e-8 to 1e-4 (tests/test_lie_exp_branch_points_host.py); the quaternion was never off."""
    dims, grids = _anymal_three_grid_points()
    n, nv, batch = len(grids), dims.nv, len(fxe["angle"])
    xi = fxe["xi"]
    ctx = capi.Context(dims, n, batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        S, D = Records(L, "sol"), Records(L, "dir")
        rng = np.random.default_rng(23)
        worst = Worst()
        for k in range(2):
            M0 = fxe["M0"][k]
            p0 = float(np.linalg.norm(M0[:3]))
            got = {}
            for step, mult in ((1.0, 1.0), (0.5, 2.0)):
                sol = rng.uniform(-1, 1, ctx.shape("sol"))
                d = rng.uniform(-1, 1, ctx.shape("dir"))
                S.f(sol, "q")[..., :7] = M0
                D.f(d, "dx")[..., :6] = (mult * xi)[:, None, :]
                assert np.array_equal(step * D.f(d, "dx")[..., :6], np.broadcast_to(xi[:, None, :], (batch, n, 6)))
                steps = np.stack([np.full(batch, step), rng.uniform(0.2, 1.0, batch)], axis=1)
                ctx.upload(BUF_SOL, sol)
                ctx.upload(BUF_DIR, d)
                ctx.upload(BUF_STEP, steps)
                ctx.integrate_solution()
                ctx.sync()
                new = ctx.download_records(BUF_SOL, "sol")
                assert np.isfinite(new).all()
                # the Euclidean members: s + step d (no impact grid point here)
                ref = sol.copy()
                S.f(ref, "q")[..., 7:nv + 1] += step * D.f(d, "dx")[..., 6:nv]
                S.f(ref, "v")[...] += step * D.f(d, "dx")[..., nv:]
                S.f(ref, "a")[...] += step * D.f(d, "daf")[..., :nv]
                S.f(ref, "u")[...] += step * D.f(d, "du")
                S.f(ref, "lmd")[...] += step * D.f(d, "dlmdgmm")[..., :nv]
                S.f(ref, "gmm")[...] += step * D.f(d, "dlmdgmm")[..., nv:]
                S.f(ref, "beta")[...] += step * D.f(d, "dbetamu")[..., :nv]
                S.f(ref, "nu_passive")[..., :6] += step * D.f(d, "dnu_passive")[..., :6]
                for i, g in enumerate(grids):
                    S.f(ref, "f")[:, i, :g.dimf] += step * D.f(d, "daf")[:, i, nv:nv + g.dimf]
                    S.f(ref, "mu")[:, i, :g.dimf] += step * D.f(d, "dbetamu")[:, i, nv:nv + g.dimf]
                    S.f(ref, "xi")[:, i, :g.dims] += step * D.f(d, "dxi")[:, i, :g.dims]
                q = S.f(new, "q")[..., :7].copy()
                S.f(new, "q")[..., :7] = M0
                assert np.allclose(new, ref, rtol=1e-15, atol=1e-15)
                got[step] = q
                for i in range(batch):
                    ang, bp = fxe["angle"][i], BOUND * vscale(fxe, i, p0)
                    for st in range(n):
                        worst.add("position", np.abs(q[i, st, :3] - fxe["comp_pos"][k, i]).max(), bp, ang)
                        worst.add("quaternion", np.abs(q[i, st, 3:] - fxe["comp_quat"][k, i]).max(), QUAT_BOUND, ang)
                        worst.add("|quat| - 1", abs(np.linalg.norm(q[i, st, 3:]) - 1.0), UNIT_BOUND, ang)
                        if k == 0 and not xi[i, :3].any():
                            assert np.array_equal(q[i, st, :3], M0[:3])
            for i in range(batch):
                worst.add("half step - full step, position", np.abs(got[0.5][i, :, :3] - got[1.0][i, :, :3]).max(),
                          BOUND * vscale(fxe, i, p0), fxe["angle"][i])
                worst.add("half step - full step, quaternion", np.abs(got[0.5][i, :, 3:] - got[1.0][i, :, 3:]).max(), QUAT_BOUND, fxe["angle"][i])
        worst.report("integrate_solution")
        worst.check()
    finally:
        ctx.close()


def _lift_then_impact():
    """ANYmal, LH and RF lift and touch down again, on the fewest grid points a lift followed by an impact discretises to:
    (intermediate, lift, intermediate, impact, intermediate, terminal), the switching constraint on grid point 1; the time steps
    of grid points 1 and 2 are set to 2^-6, so that dt1 + dt2 = 2^-5 and dt1 dt2 = 2^-12 exactly"""
    cs = ContactSequence([12, 6, 12], [Event("lift", 0.005), Event("impact", 0.025, impact_dimf=6)])
    grids = discretize(2, 0.04, 0.0, cs)
    sw = [i for i, g in enumerate(grids) if g.switching_constraint]
    assert len(grids) == 6 and sw == [1] and grids[3].type == GRID_IMPACT and grids[1].dims == 6
    grids[1].dt = grids[2].dt = 2.0 ** -6
    return grids, 1, contact_masks(grids, [0b1111, 0b1001, 0b1111], [0b0110]), [1, 2]


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


@pytest.mark.gpu
def test_switching_constraint_at_the_branch_points(fxe, oracle):
    """rtoc_contact_eval_kkt on ANYmal with one switching grid point, one instance per fixture case of |w| < pi: base at M0, joints
    at the standing pose, a = 0 and v = (32 xi, 0) with dt1 = dt2 = 2^-6, so that dq_b is xi bit for bit.  P against
    p_ref + R_ref r_c - desired with (R_ref, p_ref) = M0 exp6(xi) of the fixture and r_c the foot in the base frame (the oracle's
    forward kinematics at the identity base); the base columns of Phiq against Pq_b Ad_{exp6}^-1, of Phiv / Phia against
    2^-5 / 2^-12 Pq_b Jexp6, Pq_b = [R_ref, -R_ref [r_c]x] -- with the transposed transport under the reference's composition
    (the default), the plain one under RTOC_OPT_SWITCHING_TRANSPORT.  Both placements, both settings, no NaN anywhere.
    Observed on the MI355X, as error / bound: P 0.0044 at 1.5e-8, Phiq 0.0089 at pi - 1e-3, Phiv and Phia 0.073 at 1e-2.  Before
    the repair of the coefficients: P and Phiq 4.08e+04, Phiv and Phia 9.71e+03, all at 1.01e-8."""
    m = rm.load_named("anymal")
    dims = anymal_dims()
    grids, i0, masks, imp = _lift_then_impact()
    rows = np.flatnonzero(~fxe["beyond_pi"])
    n, nv, nq, nu, ncon, batch = len(grids), m.nv, m.nq, m.nv - 6, 4, len(rows)
    xi = fxe["xi"][rows]
    rng = np.random.default_rng(5)
    place = [oracle.rbd_contact_placement(m, Q_STAND, c) for c in range(ncon)]
    pos = np.tile(np.array([p for _, p in place])[None], (n, 1, 1)) + 0.01 * rng.uniform(-1, 1, (n, ncon, 3))
    q_id = Q_STAND.copy()
    q_id[:7] = [0, 0, 0, 0, 0, 0, 1]
    r_c = [oracle.rbd_contact_placement(m, q_id, c)[1] for c in range(ncon)]
    ctx = capi.Context(dims, n, batch, 0)
    try:
        ctx.set_grid(grids)
        ctx.set_robot_model(m)
        ctx.set_contact_schedule(masks, pos, None)
        wq = np.concatenate([np.full(6, 10.0), np.full(nu, 1.0)])
        ctx.set_configuration_cost(Q_STAND, np.zeros(nv), np.zeros(nu), wq, np.full(nv, 1.0), np.full(nv, 1e-3), np.full(nu, 1e-3),
                                   10.0 * wq, np.full(nv, 1.0), q_weight_impact=wq, v_weight_impact=np.full(nv, 1.0), dv_weight_impact=np.full(nv, 1e-3))
        S, K, D = Records(ctx.L, "sol"), Records(ctx.L, "kkt"), Records(ctx.L, "cdd")
        dt1, dt2 = grids[i0].dt, grids[i0 + 1].dt
        worst = Worst()
        for k in range(2):
            M0 = fxe["M0"][k]
            p0 = float(np.linalg.norm(M0[:3]))
            sol = S.zeros(batch, n)
            q = S.f(sol, "q")
            q[..., :nq] = Q_STAND
            q[..., :7] = M0
            S.f(sol, "v")[:, i0, :6] = 32.0 * xi
            assert np.array_equal((dt1 + dt2) * S.f(sol, "v")[:, i0, :6] + dt1 * dt2 * S.f(sol, "a")[:, i0, :6], xi)
            ctx.set_initial_state(np.concatenate([q[:, 0, :nq], np.zeros((batch, nv))], axis=1))
            ctx.upload(BUF_SOL, sol)
            for exact in (False, True):
                ctx.set_switching_transport(exact)
                ctx.contact_eval_kkt()
                ctx.sync()
                kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
                assert (ctx.status() == 0).all()
                for b, i in enumerate(rows):
                    ang, sv = fxe["angle"][i], vscale(fxe, i)
                    R_ref, p_ref = fxe["comp_R"][k, i], fxe["comp_pos"][k, i]
                    Pres, Phix, Phia = K.f(kkt[b, i0], "Pres")[:6], K.f(kkt[b, i0], "Phix")[:6], D.f(cdd[b, i0], "Phia")[:6]
                    assert np.isfinite(Pres).all() and np.isfinite(Phix).all() and np.isfinite(Phia).all()
                    Tq, Jr = fxe["ad_inv"][i], fxe["jexp6"][i]
                    if not exact:
                        Tq, Jr = Tq.T, Jr.T
                    amp = fxe["jexp6_cond"][i] * fxe["jexp6_inv_norm"][i]
                    for a, c in enumerate(imp):
                        r = slice(3 * a, 3 * a + 3)
                        P = p_ref + R_ref @ r_c[c] - pos[i0 + 2, c]
                        worst.add("P", np.abs(Pres[r] - P).max(), BOUND * max(sv, p0, float(np.linalg.norm(r_c[c]))), ang)
                        Pq_b = np.concatenate([R_ref, -R_ref @ _skew(r_c[c])], axis=1)
                        bj = BOUND * sv * np.abs(Pq_b).sum(axis=0).max()
                        worst.add("Phiq", np.abs(Phix[r, :6] - Pq_b @ Tq).max(), bj, ang)
                        worst.add("Phiv", np.abs(Phix[r, nv:nv + 6] - 2.0 ** -5 * (Pq_b @ Jr)).max(), 2.0 ** -5 * bj * amp, ang)
                        worst.add("Phia", np.abs(Phia[r, :6] - 2.0 ** -12 * (Pq_b @ Jr)).max(), 2.0 ** -12 * bj * amp, ang)
        worst.report("switching constraint")
        worst.check()
    finally:
        ctx.close()
