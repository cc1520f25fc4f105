"""The 50-digit SE(3) reference (tests/lie_reference.py), the committed fixture tests/golden/lie_exp_branch_points.npz and every
host-side copy of the exp6 formula, at the branch points of that formula: rotation angle 0, either side of 1e-10 / 1e-8 / 1e-3
(every threshold a copy has or had), the range [1e-8, 1e-4] in which (1 - cos t) / t^2 cancels, up to pi - 1e-3, and 4.0.

(a) the reference checks itself (exp6 against mp.expm of the twist matrix, Jexp6 against a central difference of exp6, Ad^-1
against Ad), (b) the fixture equals its regeneration bit for bit and covers every threshold, (c) oracle.rbd_exp6,
oracle.se3_integrate from both base placements, robotoc_amd.solver._exp3 / _V, exp3 / V_mat of
tests/solution_interpolator_restatement.py and the planner header's exp3 / Vmat (through
SolutionInterpolator::interpolateConfiguration) are held to the fixture: translations at 1e-13 max(1, |v|) (max(1, |p0|, |v|)
on a base placement), rotation matrices at 1e-13, the integrated quaternion at QUAT_BOUND.  The device tests
(tests/test_lie_exp_branch_points.py) use the same bounds.

QUAT_BOUND: the float64 restatement below of the repaired formula (exponential quaternion, Hamilton product, normalisation)
stays within 2.3e-16 of the reference's composed quaternion over the whole fixture and both placements (worst at angle 4), so
the 1e-15 the quaternion was to be tried at first holds with a factor of 4.5 to spare and is the bound; | |quat| - 1 | reaches
2.3e-16 of the 4e-16 allowed.

Before the repair ((1 - cos t) / t^2 in every copy, constants below 1e-8 resp. 1e-10), leg (c) read, as error / bound:
oracle.rbd_exp6 translation and oracle.se3_integrate position 4.08e+04, both at 1.01e-8 (cos t rounds to 1 or to 1 - 1.1e-16: the
coefficient is 0 or 1.09 instead of 1/2), solver._V and the restatement's V_mat 4.15e+04 at 9.9e-9 (their threshold was 1e-10),
the planner header's Vmat 1.44e+04 at 1.5e-8 (at alpha = 1/2; at alpha = 1 the error of V cancels against that of V^-1).  Angle
by angle V(w) v of that formula stood at 3.5e+02 at 1.01e-10, 4.2e+04 at 9.9e-9, 4.1e+04 at 1.01e-8, 7.8e+02 at 1.5e-8, 1.7e+03
at 3e-8, 2.8e+02 at 1e-7, 4.2e+02 at 1e-6, 3.6 at 1e-5, 2.0 at 1e-4, 0.32 at 1.01e-3 and 0.012 at 1e-2.  The rotations were
never off: exp3 0.0067 (solver, restatement), 0.0033 (oracle), the integrated quaternion 0.22 of its 1e-15.
After it (rbd::exp_coefficients of robotoc_amd/csrc/rigid_body_math.hpp restated in every copy: three series terms below 1e-3,
2 sin^2(t/2) / t^2 above): oracle.rbd_exp6 translation 0.0023 at pi - 1e-3, rotation 0.0033 at 3; oracle.se3_integrate position
0.0036 at 1.01e-10, quaternion 0.22 at 4; solver / restatement V v 0.0018 at 1.01e-8, exp3 0.0044 at 3; the planner header
position 0.046 and quaternion 0.21, both at 3 (its log3 just below the near-pi switch, as tests/test_lie_branch_points_host.py
records)."""
import os
import subprocess

import numpy as np
import pytest

from test_lie_branch_points_host import BOUND, _report, quat_R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_exp_branch_points.npz")
QUAT_BOUND = 1e-15   # the integrated quaternion against the reference's product (see the module docstring)
UNIT_BOUND = 4e-16   # | |quat| - 1 |


@pytest.fixture(scope="module")
def fxe():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def vscale(fxe, i, *more):
    """max(1, |v|, ...) of case i"""
    return max(1.0, float(np.linalg.norm(fxe["xi"][i, :3])), *more)


def _track(worst, err, bound, fxe, i):
    r = float(err) / bound
    return (r, fxe["angle"][i], i) if not r <= worst[0] else worst


ZERO = (0.0, 0.0, -1)


def exp_coefficients(t2):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 the way rbd::exp_coefficients computes them"""
    t = np.sqrt(t2)
    if t < 1e-3:
        return 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    sh, s = np.sin(0.5 * t), np.sin(t)
    return s / t, 2.0 * sh * sh / t2, (t - s) / (t2 * t)


def integrate_restatement(q7, xi):
    """M exp6(xi) in float64, operation by operation what integrate_solution_kernel does on the base"""
    v, w = xi[:3], xi[3:]
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    t = np.sqrt(t2)
    _, C, B = exp_coefficients(t2)
    wv = np.cross(w, v)
    u = v + C * wv + B * np.cross(w, wv)
    x, y, z, qw = q7[3:]
    pos = q7[:3] + quat_R(q7[3:]) @ u
    sc, ew = (0.5 - t * t / 48.0 if t < 1e-8 else np.sin(0.5 * t) / t), np.cos(0.5 * t)
    e0, e1, e2 = sc * w
    r = np.array([qw * e0 + x * ew + y * e2 - z * e1, qw * e1 - x * e2 + y * ew + z * e0, qw * e2 + x * e1 - y * e0 + z * ew,
                  qw * ew - x * e0 - y * e1 - z * e2])
    return pos, r / np.sqrt(r @ r)


# ---- (a) the reference checks itself ----

def test_reference_exp6_equals_expm_of_the_twist_matrix():
    """the closed form (sin(t/2) and the series of (t - sin t) / t^3) against the matrix exponential, at every twist of the fixture"""
    lr = pytest.importorskip("lie_reference")
    from golden import make_lie_exp_branch_points as gen
    mp = lr.mp
    worst = mp.mpf(0)
    for _, xi, _ in gen.cases()[0]:
        q, p = lr.exp6(xi)
        qm, pm = lr.exp6_expm(xi)
        sign = 1 if lr.dot(q, qm) > 0 else -1
        worst = max(worst, max(abs(a - sign * b) for a, b in zip(q, qm)), max(abs(a - b) for a, b in zip(p, pm)))
    print("exp6 - expm: %s" % mp.nstr(worst, 3))
    assert worst < mp.mpf("1e-40")


def test_reference_jexp6_is_the_derivative_of_exp6_and_ad_inv_inverts_ad():
    """exp6(xi + d) = exp6(xi) exp6(Jexp6(xi) d + O(d^2)): a central difference of log6(exp6(xi)^-1 exp6(xi +- eps e_j));
    Ad_{X^-1} Ad_X = I and Ad_{exp6(xi)}^-1 xi = xi"""
    lr = pytest.importorskip("lie_reference")
    from golden import make_lie_exp_branch_points as gen
    mp = lr.mp
    eps = mp.mpf("1e-14")  # central difference: truncation ~ eps^2 = 1e-28, rounding ~ 1e-50 / eps
    worst, worst_ad = mp.mpf(0), mp.mpf(0)
    angles = [mp.mpf(a) for a in gen.ANGLES] + [mp.pi - mp.mpf(d) for d in gen.BELOW_PI]
    for th in angles:
        for ax, v in (([0.0, 0.0, 1.0], [0.3, -0.2, 0.9]), ([0.3, -0.5, 0.8], [6.0, -5.0, 6.2])):
            n = lr.norm(lr._vec(ax))
            xi = lr._vec(v) + [th * mp.mpf(c) / n for c in ax]
            q, p = lr.exp6(xi)
            qi, pi_ = lr.inverse(q, p)
            J = lr.jexp6(xi)
            for j in range(6):
                plus = lr.log6(*lr.compose(qi, pi_, *lr.exp6([c + (eps if k == j else 0) for k, c in enumerate(xi)])))
                minus = lr.log6(*lr.compose(qi, pi_, *lr.exp6([c - (eps if k == j else 0) for k, c in enumerate(xi)])))
                for r in range(6):
                    worst = max(worst, abs((plus[r] - minus[r]) / (2 * eps) - J[r, j]))
            A = lr.ad_inv_exp6(xi)
            I6 = A * lr.Ad(q, p)
            worst_ad = max(worst_ad, max(abs(I6[r, c] - (1 if r == c else 0)) for r in range(6) for c in range(6)))
            Ax = A * mp.matrix(xi)
            worst_ad = max(worst_ad, max(abs(Ax[r] - xi[r]) for r in range(6)))
    print("Jexp6 - central difference: %s; Ad^-1: %s" % (mp.nstr(worst, 3), mp.nstr(worst_ad, 3)))
    assert worst < mp.mpf("1e-25") and worst_ad < mp.mpf("1e-45")


# ---- (b) the committed fixture equals a regeneration and covers the branch points ----

def test_fixture_regenerates_bit_for_bit(fxe):
    pytest.importorskip("mpmath")
    from golden import make_lie_exp_branch_points as gen
    new = gen.generate()
    assert sorted(new) == sorted(fxe)
    for k, v in new.items():
        v = np.asarray(v)
        assert v.shape == fxe[k].shape and v.dtype == fxe[k].dtype, k
        assert v.tobytes() == fxe[k].tobytes(), k


def test_fixture_covers_every_threshold_of_every_copy(fxe):
    ang, xi = fxe["angle"], fxe["xi"]
    th = np.linalg.norm(xi[:, 3:], axis=1)
    assert (np.abs(th - ang) <= 4e-16 * ang).all()   # the doubles have the angle they are labelled with
    # 1e-10 and 1e-8: the thresholds the copies had; 1e-3: the one they have now, the device's among them
    assert list(fxe["thresholds"]) == [1e-10, 1e-8, 1e-3]
    for T in fxe["thresholds"]:
        for side in (ang[(ang > 0.98 * T) & (ang < T)], ang[(ang > T) & (ang < 1.02 * T)]):
            assert len(side) >= 8 and len(set(side)) == 1, T
    for a in sorted(set(ang)):
        rows = np.flatnonzero(ang == a)
        nv = np.linalg.norm(xi[rows, :3], axis=1)
        assert len(rows) == 8 and (nv == 0.0).sum() == 1 and (nv > 9.0).sum() == 1 and (np.abs(nv - 1.0) < 1e-15).sum() == 6, a
        if a > 0.0:
            assert any(np.linalg.norm(np.cross(xi[i, :3], xi[i, 3:])) <= 1e-15 * a for i, s in zip(rows, nv) if s > 0.5), a  # v parallel to w
            for k in range(3):
                assert any((xi[i, 3:] == a * np.eye(3)[k]).all() for i in rows), (a, k)
    assert 0.0 in ang and 1e-12 in ang and sum(1 for a in set(ang) if 1e-8 < a <= 1e-4) >= 6
    beyond = fxe["beyond_pi"]
    assert (ang[beyond] == 4.0).all() and beyond.sum() == 8 and (ang[~beyond] < np.pi).all()
    assert np.isnan(fxe["jexp6"][beyond]).all() and np.isfinite(fxe["jexp6"][~beyond]).all()
    assert np.isfinite(fxe["ad_inv"]).all() and np.nanmax(fxe["jexp6_cond"]) < 100
    # a half step of 2 xi and (dt1 + dt2) = 2^-5 times 32 xi give the twist back bit for bit
    assert np.array_equal(0.5 * (2.0 * xi), xi) and np.array_equal(2.0 ** -5 * (32.0 * xi), xi)
    M0 = fxe["M0"]
    assert np.array_equal(M0[0], [0, 0, 0, 0, 0, 0, 1]) and abs(np.linalg.norm(M0[1, :3]) - 10.0) < 1e-14
    assert abs(np.linalg.norm(M0[1, 3:]) - 1.0) < 4e-16


# ---- (c) the host-side copies of the formula ----

def test_float64_restatement_of_the_integration_stays_inside_the_quaternion_bound(fxe):
    """where QUAT_BOUND comes from: the repaired formula in float64 on the CPU, never the device"""
    wq, wp, wn = ZERO, ZERO, ZERO
    for k in range(2):
        M0 = fxe["M0"][k]
        for i in range(len(fxe["angle"])):
            pos, quat = integrate_restatement(M0, fxe["xi"][i])
            wq = _track(wq, np.abs(quat - fxe["comp_quat"][k, i]).max(), QUAT_BOUND, fxe, i)
            wp = _track(wp, np.abs(pos - fxe["comp_pos"][k, i]).max(), BOUND * vscale(fxe, i, np.linalg.norm(M0[:3])), fxe, i)
            wn = _track(wn, abs(np.linalg.norm(quat) - 1.0), UNIT_BOUND, fxe, i)
    _report("float64 restatement, quaternion (x 1e-15 = the error itself)", wq)
    _report("float64 restatement, position", wp)
    _report("float64 restatement, |quat| - 1", wn)
    assert wq[0] <= 1.0 and wp[0] <= 1.0 and wn[0] <= 1.0


def test_oracle_exp6(fxe, oracle):
    wR, wp = ZERO, ZERO
    for i in range(len(fxe["angle"])):
        R, p = oracle.rbd_exp6(fxe["xi"][i])
        wR = _track(wR, np.abs(R - fxe["exp_R"][i]).max(), BOUND, fxe, i)
        wp = _track(wp, np.abs(p - fxe["exp_pos"][i]).max(), BOUND * vscale(fxe, i), fxe, i)
    _report("oracle.rbd_exp6 rotation", wR)
    _report("oracle.rbd_exp6 translation", wp)
    assert wR[0] <= 1.0 and wp[0] <= 1.0


def test_oracle_se3_integrate_from_both_placements(fxe, oracle):
    """full step, and the half step of twice the twist (scale x v6 is the twist bit for bit)"""
    wq, wp, wn = ZERO, ZERO, ZERO
    for k in range(2):
        M0 = fxe["M0"][k]
        for i in range(len(fxe["angle"])):
            xi = fxe["xi"][i]
            for got in (oracle.se3_integrate(M0, xi), oracle.se3_integrate(M0, 2.0 * xi, 0.5)):
                wp = _track(wp, np.abs(got[:3] - fxe["comp_pos"][k, i]).max(), BOUND * vscale(fxe, i, np.linalg.norm(M0[:3])), fxe, i)
                wq = _track(wq, np.abs(got[3:] - fxe["comp_quat"][k, i]).max(), QUAT_BOUND, fxe, i)
                wn = _track(wn, abs(np.linalg.norm(got[3:]) - 1.0), UNIT_BOUND, fxe, i)
            if k == 0 and not xi[:3].any():
                assert np.array_equal(got[:3], M0[:3])
    _report("oracle.se3_integrate position", wp)
    _report("oracle.se3_integrate quaternion", wq)
    _report("oracle.se3_integrate |quat| - 1", wn)
    assert wp[0] <= 1.0 and wq[0] <= 1.0 and wn[0] <= 1.0


def _exp3_and_V(fxe, exp3, V, name):
    wR, wp = ZERO, ZERO
    for i in range(len(fxe["angle"])):
        v, w = fxe["xi"][i, :3], fxe["xi"][i, 3:]
        wR = _track(wR, np.abs(exp3(w) - fxe["exp_R"][i]).max(), BOUND, fxe, i)
        wp = _track(wp, np.abs(V(w) @ v - fxe["exp_pos"][i]).max(), BOUND * vscale(fxe, i), fxe, i)
    _report(name + " exp3", wR)
    _report(name + " V v", wp)
    assert wR[0] <= 1.0 and wp[0] <= 1.0


def test_solver_exp3_and_V(fxe):
    from robotoc_amd import solver
    _exp3_and_V(fxe, solver._exp3, solver._V, "solver")


def test_interpolator_restatement_exp3_and_V(fxe):
    import solution_interpolator_restatement as sir
    _exp3_and_V(fxe, sir.exp3, sir.V_mat, "interpolator restatement")


def test_planner_header_exp3_and_Vmat(fxe):
    """SolutionInterpolator::interpolateConfiguration from the identity to the fixture's exp6(xi) at alpha = 1 and 1/2 is
    exp6(alpha log6(exp6(xi))): at alpha = 1 V^-1 and V are the same matrix and its error cancels, at 1/2 it does not.  The
    reference is evaluated here, at the doubles of the fixture's pose (beyond pi the logarithm is the short way round, for the
    header as for the reference); the quaternion up to sign."""
    lr = pytest.importorskip("lie_reference")
    from test_cpp_host import _build
    exe = _build("planner_log3_test")
    n = len(fxe["angle"])
    alphas = (1.0, 0.5)
    lines = ["0 0 0 0 0 0 1 " + " ".join(repr(float(x)) for x in np.concatenate([fxe["exp_pos"][i], fxe["exp_quat"][i]])) + " %r" % al
             for al in alphas for i in range(n)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    out = run.stdout.splitlines()
    assert run.returncode == 0 and out[-1] == "ok %d" % (2 * n), (run.returncode, run.stdout[-500:], run.stderr[-500:])
    wq, wp = ZERO, ZERO
    for a, al in enumerate(alphas):
        for i in range(n):
            got = np.array([float(x) for x in out[a * n + i].split()])
            lg = lr.log6(fxe["exp_quat"][i], fxe["exp_pos"][i])
            q, p = lr.exp6([lr.mp.mpf(al) * c for c in lg])
            q, p = np.array(lr.to_float(q)), np.array(lr.to_float(p))
            if q @ got[3:] < 0.0:
                q = -q
            wq = _track(wq, np.abs(got[3:] - q).max(), BOUND, fxe, i)
            wp = _track(wp, np.abs(got[:3] - p).max(), BOUND * vscale(fxe, i), fxe, i)
    _report("planner header exp3 (quaternion)", wq)
    _report("planner header Vmat (position)", wp)
    assert wq[0] <= 1.0 and wp[0] <= 1.0
