"""The numpy restatement of the reference's ParNMPC algorithm (tests/parnmpc_restatement.py) against dense linear algebra, and
its whole iteration on the reference's own test problem.  No GPU."""
import numpy as np
import pytest

import parnmpc_restatement as pn
from robotoc_amd import robot_model as rm


def random_spd(rng, n, cond=1.0e3, scale=1.0):
    """SPD with the given 2-norm condition number: random orthogonal basis, log-spaced spectrum"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return scale * (Q * np.logspace(0.0, -np.log10(cond), n)) @ Q.T


def reference_error(dt, H, r):
    """e_ref of a case: the larger of |K Kinv - I| and the coarse update's distance from numpy.linalg.solve, both max-norm"""
    K = pn.saddle_matrix(H, dt)
    Kinv = pn.invert(dt, H)
    e1 = np.abs(K @ Kinv - np.eye(K.shape[0])).max()
    x = np.linalg.solve(K, r)
    e2 = np.abs(Kinv @ r - x).max() / max(1.0, np.abs(x).max())
    return max(e1, e2), np.linalg.cond(K)


@pytest.mark.parametrize("nv", [7, 8])
@pytest.mark.parametrize("dt", [0.05, 0.5])
def test_restated_inverter_against_dense_algebra(nv, dt):
    rng = np.random.default_rng(100 * nv + int(100 * dt))
    worst = 0.0
    for k in range(5):
        H = random_spd(rng, 3 * nv, cond=10.0 ** rng.uniform(0.5, 2.5), scale=10.0 ** rng.uniform(-0.5, 0.5))
        r = rng.standard_normal(5 * nv)
        e_ref, cond = reference_error(dt, H, r)
        print("nv %d dt %.2f case %d: e_ref %.2e cond2(K) %.2e" % (nv, dt, k, e_ref, cond))
        assert cond <= 1.0e6
        assert e_ref <= 1.0e-10
        # the coarse update through the class, against the dense solve
        rec = dict(Qaa=H[:nv, :nv], Qxa=H[nv:, :nv], Qxx=H[nv:, nv:], Fx=r[:2 * nv], la=r[2 * nv:3 * nv], lx=r[3 * nv:])
        s = rng.standard_normal(5 * nv)
        s_new = pn.SplitCorrector().coarse_update(dt, rec, s)
        x = np.linalg.solve(pn.saddle_matrix(H, dt), r)
        assert np.abs(s_new - (s - x)).max() <= 1.0e-10 * max(1.0, np.abs(x).max())
        worst = max(worst, e_ref)
    print("worst e_ref:", worst)


def test_single_stage_backward_correction_is_the_dense_solve():
    """N = 1: no correction pass does anything, the direction is minus the solution of the one saddle system"""
    rng = np.random.default_rng(5)
    nv, dt = 7, 0.1
    H = random_spd(rng, 3 * nv, cond=100.0)
    r, s = rng.standard_normal(5 * nv), rng.standard_normal((1, 5 * nv))
    rec = dict(Qaa=H[:nv, :nv], Qxa=H[nv:, :nv], Qxx=H[nv:, nv:], Fx=r[:2 * nv], la=r[2 * nv:3 * nv], lx=r[3 * nv:])
    aux = np.zeros((1, 2 * nv, 2 * nv))
    d, aux_new, _ = pn.backward_correction(dt, [rec], s, aux)
    assert np.abs(d[0] + np.linalg.solve(pn.saddle_matrix(H, dt), r)).max() < 1e-10
    assert (aux_new == aux).all()


def test_restated_iteration_converges_on_the_reference_test_problem(oracle):
    """iiwa14, N = 20, T = 1, cost and initial state of test/solver/unconstr_parnmpc_solver_test.cpp without the limits: the
    restated updateSolution drives its KKT error below 1e-8.  The iteration count printed here is N_REF of
    tests/test_parnmpc_closed_loop.py."""
    m = rm.load_named("iiwa14")
    cost, q0, v0, N, T = pn.reference_test_problem(m.nv)
    dt = T / N
    z = np.zeros(m.nv)
    sol = [dict(q=q0.copy(), v=v0.copy(), a=z.copy(), u=z.copy(), lmd=z.copy(), gmm=z.copy(), beta=z.copy()) for _ in range(N)]
    aux = pn.init_aux(cost, N)
    hist = []
    for it in range(60):
        err, aux = pn.iterate(oracle, m, cost, dt, q0, v0, sol, aux)
        hist.append(err)
        if err < 1e-8:
            break
    print("restated ParNMPC KKT error per iteration:", ["%.2e" % e for e in hist])
    print("n_ref =", len(hist), "calls of updateSolution until the KKT error it reports (of the iterate it linearised at) is below 1e-8")
    assert hist[-1] < 1e-8
