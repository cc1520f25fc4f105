"""The grids, records and query times the control-policy tests share (tests/test_control_policy_restatement.py on the CPU,
tests/test_control_policy_gpu.py on the device): the ANYmal horizon of tests/solution_interpolation_cases.py with its lift and its
touch-down (the grid re-gridded onto, N = 7), three instances, with shared times or every instance's own time steps; an iCub
shape of four grid points (nv = 35: the Kd run of a row of K starts at 328 bytes); a fixed-base iiwa14 (nu = nv: Kp is the whole
left half of K); an ANYmal grid of 70 points (the interval search in chunks of 64)."""
import numpy as np

import control_policy_restatement as cpr
import solution_interpolation_cases as cases
from robotoc_amd import capi
from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import anymal_dims, icub_dims, iiwa14_dims


def anymal_side(phase_based):
    """the grid of the ANYmal horizon: dict(grids, types, masks, dt [batch or 1, n], events)"""
    return cases.anymal_grids(phase_based)[1]


def layout(dims):
    return capi.layout_for(dims)


def shapes():
    """name -> (dims, grids, batch)"""
    return {
        "icub": (icub_dims(nc_max=0), uniform_grid(3, 0.1, dimf=12), 2),
        "iiwa14": (iiwa14_dims(), uniform_grid(4, 0.1), 2),
        "anymal70": (anymal_dims(nc_max=0), uniform_grid(69, 0.01, dimf=12), 2),
    }


def random_records(L, batch, n, seed):
    """(sol, ric) [batch, n, stride]: seeded normal numbers in EVERY double, padding included (what must not be read is poisoned
    by the tests; nothing is zero by accident)"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(batch, n, L.sol.stride)), rng.normal(size=(batch, n, L.ric.stride))


def restate(shape, types, tg, N, t, sol, ric):
    """over the batch: tg [batch or 1, n], t [batch] -> ([policy], [branch], [alpha], [scale])"""
    out = [cpr.control_policy(shape, types, tg[b if len(tg) > 1 else 0], N, t[b], sol[b], ric[b]) for b in range(len(t))]
    return [list(x) for x in zip(*out)]


def compare_policy(got, want, scale, label):
    """one instance: copies bit for bit; a blended entry within 4 eps (|alpha| |a| + |1 - alpha| |b|) -- two rounded products and
    one rounded sum, with or without contraction to a fused multiply-add.  Returns the worst error over its bound."""
    worst = 0.0
    for k in ("tauJ", "qJ", "dqJ", "Kp", "Kd"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        if scale is None:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), "%s: %s is not a copy of its record" % (label, k)
            continue
        assert np.isfinite(g).all(), (label, k)
        bound = 4 * cpr.EPS * scale[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(g - w) > 0, np.abs(g - w) / bound, 0.0)
        worst = max(worst, float(ratio.max()))
    assert worst <= 1.0, (label, worst)
    return worst
