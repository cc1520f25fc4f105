"""Regenerates tests/golden/lie_exp_branch_points.npz: twists at the branch points of exp6 (rotation angle 0, either side of
every threshold any copy of the formula has or had, the range [1e-8, 1e-4] where (1 - cos t) / t^2 cancels, up to pi - 1e-3 and
one angle beyond pi) with exp6, its composition onto two base placements, Jexp6 = Jlog6(exp6)^-1 and Ad_{exp6}^-1, evaluated
at 50 digits by tests/lie_reference.py and rounded to double.  The GPU tests read the fixture, so they need no mpmath.

  python tests/golden/make_lie_exp_branch_points.py        (from the repo root; needs numpy + mpmath)

Every angle comes about the three coordinate axes and about two random axes with |v| = 1, once about a random axis with v = 0,
once with v parallel to w and once with |v| = 10.  The twists are stored as the doubles the reference was evaluated at; a
multiple of a twist by a power of two (the device tests feed 2 xi with a half step, and 32 xi with dt1 + dt2 = 2^-5) is exact.
The angle beyond pi is a valid argument of the exponential but not of Jexp6 through the logarithm: `beyond_pi` flags its rows,
whose `jexp6`, `jexp6_cond` and `jexp6_inv_norm` are NaN.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# the thresholds of the copies of the formula: solver._exp3 / _V, the planner header and the interpolator restatement (1e-10,
# before their repair), integrate_solution_kernel, switching_constraint_lin_kernel, orc_rbd_exp6, orc_se3_integrate (1e-8, before
# theirs) and rbd::exp_coefficients (robotoc_amd/csrc/rigid_body_math.hpp), which all of them restate now (1e-3)
THRESHOLDS = [1e-10, 1e-8, 1e-3]

ANGLES = [0.0, 1e-12, 0.99e-10, 1.01e-10, 0.99e-8, 1.01e-8, 1.5e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 9.9e-4, 1.01e-3, 1e-2, 0.1, 1.0,
          3.0]
BELOW_PI = [1e-3]
BEYOND_PI = [4.0]
SEED = 20240911


def cases():
    """(label angle, twist [v; w] as 6 doubles, beyond-pi flag) and the two base placements [x y z qx qy qz qw]"""
    import lie_reference as lr
    mp = lr.mp
    rng = np.random.default_rng(SEED)

    def unit(n=3):
        while True:
            u = 2.0 * rng.random(n) - 1.0
            r = float(np.linalg.norm(u))
            if 0.1 < r <= 1.0:
                return u / r

    def rotvec(axis, angle):
        a = [mp.mpf(float(c)) for c in axis]
        n = lr.norm(a)
        return np.array([float(angle * c / n) for c in a])

    out = []
    angles = [(mp.mpf(a), a, False) for a in ANGLES] + [(mp.pi - mp.mpf(d), float(np.pi) - d, False) for d in BELOW_PI]
    angles += [(mp.mpf(a), a, True) for a in BEYOND_PI]
    for ang, label, beyond in angles:
        for ax in [np.eye(3)[k] for k in range(3)] + [unit(), unit()]:
            out.append((label, np.concatenate([unit(), rotvec(ax, ang)]), beyond))
        out.append((label, np.concatenate([np.zeros(3), rotvec(unit(), ang)]), beyond))
        u = unit()
        out.append((label, np.concatenate([u, rotvec(u, ang)]), beyond))
        out.append((label, np.concatenate([10.0 * unit(), rotvec(unit(), ang)]), beyond))
    M0 = np.array([[0, 0, 0, 0, 0, 0, 1.0], np.concatenate([10.0 * unit(), unit(4)])])
    return out, M0


def generate():
    """the fixture's arrays, as a dict"""
    import lie_reference as lr
    cs, M0 = cases()
    n = len(cs)
    d = dict(angle=np.array([c[0] for c in cs]), xi=np.array([c[1] for c in cs]), beyond_pi=np.array([c[2] for c in cs]), M0=M0,
             thresholds=np.array(THRESHOLDS))
    d["exp_quat"], d["exp_pos"], d["exp_R"] = np.zeros((n, 4)), np.zeros((n, 3)), np.zeros((n, 3, 3))
    d["comp_pos"], d["comp_quat"], d["comp_R"] = np.zeros((2, n, 3)), np.zeros((2, n, 4)), np.zeros((2, n, 3, 3))
    d["ad_inv"], d["jexp6"] = np.zeros((n, 6, 6)), np.full((n, 6, 6), np.nan)
    d["jexp6_cond"], d["jexp6_inv_norm"] = np.full(n, np.nan), np.full(n, np.nan)
    for i, (_, xi, beyond) in enumerate(cs):
        q, p = lr.exp6(xi)
        d["exp_quat"][i], d["exp_pos"][i], d["exp_R"][i] = lr.to_float(q), lr.to_float(p), lr.to_float(lr.quat_to_rotation(q))
        for k in range(2):
            qc, pc = lr.compose(M0[k, 3:], M0[k, :3], q, p)
            d["comp_pos"][k, i], d["comp_quat"][k, i], d["comp_R"][k, i] = lr.to_float(pc), lr.to_float(qc), lr.to_float(lr.quat_to_rotation(qc))
        d["ad_inv"][i] = lr.to_float(lr.ad_inv_exp6(xi))
        if not beyond:
            J = lr.jexp6(xi)
            d["jexp6"][i] = lr.to_float(J)
            # the device inverts Jlog6(exp6(xi)): its condition number (that of Jexp6 too) and the 2-norm of the inverse, Jexp6
            d["jexp6_cond"][i], d["jexp6_inv_norm"][i] = float(lr.cond2(J)), float(lr.norm2(J))
    return d


def main():
    d = generate()
    path = os.path.join(HERE, "lie_exp_branch_points.npz")
    np.savez_compressed(path, **d)
    print("wrote %s: %d cases, %d bytes" % (os.path.basename(path), len(d["angle"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
