"""The 50-digit SE(3) reference (tests/lie_reference.py), the committed fixture tests/golden/lie_branch_points.npz and every
host-side copy of the log6 formula, at the branch points of that formula: rotation angle 0, either side of 1e-6 / 1e-3 / the
series threshold / the near-pi switch, pi - 1e-9 and exactly pi.

(a) the reference checks itself, (b) the fixture equals its regeneration bit for bit, (c) oracle.rbd_log6 /
oracle.se3_difference, log3 / log6 / Jlog6 of tests/task_cost_6d_restatement.py, robotoc_amd.solver._log3 and the planner
header's log3 (through SolutionInterpolator::interpolateConfiguration) are held to the fixture at 1e-13 max(1, |p|).  The
device tests (tests/test_lie_branch_points.py) lean on these copies.

Before the near-pi branch and the longer series of beta, leg (c) read, as error / bound: oracle.rbd_log6, oracle.se3_difference,
the restatement's log3 / log6 and solver._log3 2.57e+20 and the restatement's Jlog6 2.30e+20, all at pi - 1e-9 (theta / (2 sin
theta) with sin theta = 1e-16), the planner header's log3 4.16e+13; every exact half turn came back as w = 0.  Angle by angle
the restatement's log6 / Jlog6 stood at 5.6e+02 / 5.7e+05 at 1.01e-3, 1.3e+02 / 7.0e+04 at 2e-3, 2.7 / 2.7e+02 at 1e-2,
6.0e+01 / 4.8e+01 at pi - 1e-2, 2.6e+05 / 2.1e+05 at pi - 1e-4 and 6.2e+09 / 5.1e+09 at pi - 1e-6; the oracle's log6, whose
series ended at 1e-4 and whose closed form went through 1 - cos t, at 4.5e+04 at 1e-4.  After them the worst is 0.31, at
angle 3, on the old path just below the near-pi switch."""
import os
import subprocess

import numpy as np
import pytest

import task_cost_6d_restatement as t6

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_branch_points.npz")
BOUND = 1e-13  # x max(1, |p|): one decade over what the formula reaches in float64, and the bound of the rigid-body derivatives


@pytest.fixture(scope="module")
def fx():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def expected(fx, i, w_got, keys=("log6", "jlog6")):
    """the fixture's values of case i; at an exact half turn those of the sign of the rotation vector `w_got`"""
    if fx["half_turn"][i] and np.dot(w_got, fx["log6"][i][3:]) < 0:
        k = list(fx["half_turn_rows"]).index(i)
        return [fx[key + "_neg"][k] for key in keys]
    return [fx[key][i] for key in keys]


def scale(fx, i):
    return max(1.0, float(np.linalg.norm(fx["pos"][i])))


def _report(name, worst):
    print("%s: worst error / bound %.2e at angle %.10g (case %d)" % (name, worst[0], worst[1], worst[2]))


def _track(worst, err, fx, i):
    r = err / (BOUND * scale(fx, i))
    return (r, fx["angle"][i], i) if r > worst[0] else worst


# ---- (a) the reference checks itself ----

def test_reference_log6_inverts_exp6_at_every_angle():
    lr = pytest.importorskip("lie_reference")
    from golden import make_lie_branch_points as gen
    mp = lr.mp
    angles = [mp.mpf(a) for a in gen.ANGLES] + [mp.pi - mp.mpf(d) for d in gen.BELOW_PI]  # at pi itself -xi is a log too
    axes = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, -0.5, 0.8], [-0.7, 0.1, 0.2]]
    worst = mp.mpf(0)
    for th in angles:
        for ax in axes:
            n = lr.norm(lr._vec(ax))
            xi = [mp.mpf("0.4"), mp.mpf("-0.9"), mp.mpf("0.25")] + [th * mp.mpf(float(c)) / n for c in ax]
            q, p = lr.exp6(xi)
            back = lr.log6(q, p)  # mpf in, mpf out: nothing is rounded to double on the way
            worst = max(worst, max(abs(a - b) for a, b in zip(back, xi)))
    print("log6(exp6(xi)) - xi: %s" % mp.nstr(worst, 3))
    assert worst < mp.mpf("1e-40")


def test_reference_jlog6_is_the_derivative_of_log6():
    lr = pytest.importorskip("lie_reference")
    from golden import make_lie_branch_points as gen
    mp = lr.mp
    eps = mp.mpf("1e-14")  # central difference: truncation ~ eps^2 = 1e-28, rounding ~ 1e-50 / eps
    worst = mp.mpf(0)
    angles = [mp.mpf(a) for a in gen.ANGLES] + [mp.pi - mp.mpf(d) for d in gen.BELOW_PI]
    for th in angles:
        for ax, p in (([0.0, 0.0, 1.0], [0.3, -0.2, 0.9]), ([0.3, -0.5, 0.8], [6.0, -5.0, 6.2])):
            n = lr.norm(lr._vec(ax))
            q = lr.exp3_quat([th * mp.mpf(c) / n for c in ax])
            p = lr._vec(p)
            J = lr.jlog6(q, p)
            for j in range(6):
                e = [eps if k == j else mp.mpf(0) for k in range(6)]
                qe, pe = lr.exp6(e)
                qm, pm = lr.exp6([-c for c in e])
                plus, minus = lr.log6(*lr.compose(q, p, qe, pe)), lr.log6(*lr.compose(q, p, qm, pm))
                for r in range(6):
                    worst = max(worst, abs((plus[r] - minus[r]) / (2 * eps) - J[r, j]))
    print("Jlog6 - central difference: %s" % mp.nstr(worst, 3))
    assert worst < mp.mpf("1e-25")


# ---- (b) the committed fixture equals a regeneration ----

def test_fixture_regenerates_bit_for_bit(fx):
    pytest.importorskip("mpmath")
    from golden import make_lie_branch_points as gen
    new = gen.generate()
    assert sorted(new) == sorted(fx)
    for k, v in new.items():
        v = np.asarray(v)
        assert v.shape == fx[k].shape and v.dtype == fx[k].dtype, k
        assert v.tobytes() == fx[k].tobytes(), k


def test_fixture_covers_the_branch_points(fx):
    ang = fx["angle"]
    T, P = float(fx["series_threshold"]), float(fx["near_pi_threshold"])
    assert T == t6.SERIES_T and P == float(np.arccos(-0.99))
    for lo, hi in ((0.0, 0.0), (9.9e-7, 1.01e-6), (9.9e-4, 1.01e-3), (0.99 * T, 1.01 * T), (P - 1e-3, P + 1e-3)):
        for a in (lo, hi):
            rows = np.flatnonzero(ang == a)
            assert len(rows) >= 4 and (np.linalg.norm(fx["pos"][rows], axis=1) > 9).any(), a
    half = np.flatnonzero(fx["half_turn"])
    assert (fx["quat"][half, 3] == 0.0).all()
    for k in range(3):
        assert any((fx["quat"][i] == np.eye(4)[k]).all() for i in half)
    assert fx["dq0_cond"].max() < 100 and len(fx["twists"]) == 6


# ---- (c) the host-side copies of the formula ----

def test_oracle_log6_and_difference(fx, oracle):
    w_log, w_diff = (0.0, 0.0, -1), (0.0, 0.0, -1)
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    for i in range(len(fx["angle"])):
        q, p = fx["quat"][i], fx["pos"][i]
        got = oracle.rbd_log6(quat_R(q), p)
        want, = expected(fx, i, got[3:], ("log6",))
        w_log = _track(w_log, np.abs(got - want).max(), fx, i)
        got = oracle.se3_difference(ident, np.concatenate([p, q]))
        want, = expected(fx, i, got[3:], ("log6",))
        w_diff = _track(w_diff, np.abs(got - want).max(), fx, i)
    _report("oracle.rbd_log6", w_log)
    _report("oracle.se3_difference", w_diff)
    assert w_log[0] <= 1.0 and w_diff[0] <= 1.0


def test_restatement_log3_log6_jlog6(fx):
    w3, w6, wj = (0.0, 0.0, -1), (0.0, 0.0, -1), (0.0, 0.0, -1)
    for i in range(len(fx["angle"])):
        R, p = quat_R(fx["quat"][i]), fx["pos"][i]
        w = t6.log3(R)
        want, Jwant = expected(fx, i, w)
        w3 = _track(w3, np.abs(w - want[3:]).max() * scale(fx, i), fx, i)  # log3 does not see p: the plain 1e-13
        w6 = _track(w6, np.abs(t6.log6(R, p) - want).max(), fx, i)
        wj = _track(wj, np.abs(t6.jlog6(R, p) - Jwant).max(), fx, i)
    _report("restatement log3", w3)
    _report("restatement log6", w6)
    _report("restatement Jlog6", wj)
    assert w3[0] <= 1.0 and w6[0] <= 1.0 and wj[0] <= 1.0


def test_half_turns_return_pi_times_the_axis(fx):
    """the two valid answers of an exact half turn: |w| = pi and exp3(w) = R"""
    from robotoc_amd import solver
    for i in np.flatnonzero(fx["half_turn"]):
        R = quat_R(fx["quat"][i])
        for log3 in (t6.log3, solver._log3):
            w = log3(R)
            assert abs(np.linalg.norm(w) - np.pi) <= BOUND
            assert np.abs(solver._exp3(w) - R).max() <= BOUND
    for k, q in enumerate(np.eye(4)[:3]):
        assert np.allclose(np.abs(t6.log3(quat_R(q))), np.pi * np.eye(3)[k], atol=BOUND)


def test_solver_log3(fx):
    from robotoc_amd import solver
    worst = (0.0, 0.0, -1)
    for i in range(len(fx["angle"])):
        w = solver._log3(quat_R(fx["quat"][i]))
        want, = expected(fx, i, w, ("log6",))
        worst = _track(worst, np.abs(w - want[3:]).max() * scale(fx, i), fx, i)
    _report("solver._log3", worst)
    assert worst[0] <= 1.0


def test_planner_header_log3(fx):
    """SolutionInterpolator::interpolateConfiguration from the identity to the fixture's placement at alpha = 1/2 is
    exp(log3(R) / 2) on the base: twice the rotation vector of the returned quaternion is the header's log3.  The quaternion's
    own rounding (exp3, R -> quaternion, normalisation) is a few 1e-16."""
    lr = pytest.importorskip("lie_reference")
    from test_cpp_host import _build
    exe = _build("planner_log3_test")
    n = len(fx["angle"])
    lines = ["0 0 0 0 0 0 1 " + " ".join(repr(float(x)) for x in np.concatenate([fx["pos"][i], fx["quat"][i]])) + " 0.5" for i in range(n)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    out = run.stdout.splitlines()
    assert run.returncode == 0 and out[-1] == "ok %d" % n, (run.returncode, run.stdout[-500:], run.stderr[-500:])
    worst = (0.0, 0.0, -1)
    for i in range(n):
        qh = [float(x) for x in out[i].split()][3:]
        w = 2.0 * np.array(lr.to_float(lr.log3_quat(qh)))
        want, = expected(fx, i, w, ("log6",))
        worst = _track(worst, np.abs(w - want[3:]).max() * scale(fx, i), fx, i)
    _report("planner header log3", worst)
    assert worst[0] <= 1.0
