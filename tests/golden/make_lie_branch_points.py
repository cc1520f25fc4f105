"""Regenerates tests/golden/lie_branch_points.npz: placements at the branch points of log6 (rotation angle 0, either side of
every threshold of the formula, up to exactly pi) with log6, Jlog6, -Jlog6 Ad_{X^-1} and its inverse, evaluated at 50 digits
by tests/lie_reference.py and rounded to double.  The GPU tests read the fixture, so they need no mpmath.

  python tests/golden/make_lie_branch_points.py        (from the repo root; needs numpy + mpmath)

Every angle comes about the three coordinate axes (R exactly structured) and about two random axes with |p| <= 1, and once
more about a random axis with |p| = 10.  At the exact half turns (q_w = 0) both +-pi axis are logarithms: `log6` / `jlog6` /
`dq0` / `dq0_inv` hold the one along +(q_x, q_y, q_z), the `*_neg` arrays (rows in the order of `half_turn_rows`) the other.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# the thresholds of the formula (robotoc_amd/csrc/rigid_body_math.hpp: log6_fwd)
SERIES_T = 0.005                     # beta / dbeta: series below, closed form above
NEAR_PI_T = float(np.arccos(-0.99))  # rotation vector: antisymmetric part below, quaternion above (3.00005...)

ANGLES = [0.0, 1e-12, 1e-9, 3e-8, 9.9e-7, 1.01e-6, 1e-4, 9.9e-4, 1.01e-3, 2e-3, 1e-2, 0.99 * SERIES_T, 1.01 * SERIES_T, 0.1, 1.0,
          3.0, NEAR_PI_T - 1e-3, NEAR_PI_T + 1e-3]
BELOW_PI = [1e-2, 1e-3, 1e-4, 1e-6, 1e-9]
SEED = 20240607


def cases():
    """(label angle, quaternion [4] double, position [3] double, half-turn flag)"""
    import lie_reference as lr
    mp = lr.mp
    rng = np.random.default_rng(SEED)

    def unit(n=3):
        while True:
            u = 2.0 * rng.random(n) - 1.0
            r = float(np.linalg.norm(u))
            if 0.1 < r <= 1.0:
                return u / r

    def quat(axis, angle):
        a = [mp.mpf(float(c)) for c in axis]
        n = lr.norm(a)
        s, c = mp.sin(angle / 2), mp.cos(angle / 2)
        return np.array([float(s * a[0] / n), float(s * a[1] / n), float(s * a[2] / n), float(c)])

    out = []
    angles = [(mp.mpf(a), a) for a in ANGLES] + [(mp.pi - mp.mpf(d), float(np.pi) - d) for d in BELOW_PI]
    for ang, label in angles:
        axes = [np.eye(3)[k] for k in range(3)] + [unit(), unit()]
        for ax in axes:
            out.append((label, quat(ax, ang), unit() * rng.random(), False))
        out.append((label, quat(unit(), ang), unit() * 10.0, False))
    # exactly pi: q_w = 0 in the doubles
    for k in range(3):
        q = np.zeros(4)
        q[k] = 1.0
        out.append((float(np.pi), q, unit() * rng.random(), True))
    g = unit()
    out.append((float(np.pi), np.array([g[0], g[1], g[2], 0.0]), unit() * rng.random(), True))
    out.append((float(np.pi), np.array([0.0, 0.0, 1.0, 0.0]), unit() * 10.0, True))
    g = unit()
    out.append((float(np.pi), np.array([g[0], g[1], g[2], 0.0]), unit() * 10.0, True))
    return out


def generate():
    """the fixture's arrays, as a dict"""
    import lie_reference as lr
    cs = cases()
    n = len(cs)
    d = dict(angle=np.array([c[0] for c in cs]), quat=np.array([c[1] for c in cs]), pos=np.array([c[2] for c in cs]),
             half_turn=np.array([c[3] for c in cs]), twists=np.eye(6), series_threshold=np.array(SERIES_T),
             near_pi_threshold=np.array(NEAR_PI_T))
    d["log6"] = np.zeros((n, 6))
    for k in ("jlog6", "dq0", "dq0_inv"):
        d[k] = np.zeros((n, 6, 6))
    d["dq0_cond"], d["dq0_inv_norm"] = np.zeros(n), np.zeros(n)
    rows = [i for i, c in enumerate(cs) if c[3]]
    d["half_turn_rows"] = np.array(rows)
    neg = {k: [] for k in ("log6", "jlog6", "dq0", "dq0_inv")}
    for i, (_, q, p, half) in enumerate(cs):
        for sign in ((1, -1) if half else (1,)):
            J0 = lr.dq0_jacobian(q, p, sign)
            J0i = J0 ** -1
            vals = dict(log6=lr.to_float(lr.log6(q, p, sign)), jlog6=lr.to_float(lr.jlog6(q, p, sign)), dq0=lr.to_float(J0),
                        dq0_inv=lr.to_float(J0i))
            if sign > 0:
                for k, v in vals.items():
                    d[k][i] = v
                d["dq0_cond"][i], d["dq0_inv_norm"][i] = float(lr.cond2(J0)), float(lr.norm2(J0i))
            else:
                for k, v in vals.items():
                    neg[k].append(v)
    for k, v in neg.items():
        d[k + "_neg"] = np.array(v)
    return d


def main():
    d = generate()
    path = os.path.join(HERE, "lie_branch_points.npz")
    np.savez_compressed(path, **d)
    print("wrote %s: %d cases, %d bytes" % (os.path.basename(path), len(d["angle"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
