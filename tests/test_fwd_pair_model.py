"""The lane map of the one-wave forward Riccati kernel (tools/fwd_pair_model.py: 16-B row-pair loads, partial sums over
column groups and row pairs, the flat Fvu copy) against the oracle's forward recursion, without a GPU: every one-wave
shape the library and the tests build (18:12:12, 7:7:0, 7:7:3, the plugin shape 12:6:6), trot and jump-STO grids."""
import os
import sys

import numpy as np
import pytest

from robotoc_amd import capi, problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import Dims, GRID_IMPACT, Records

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fwd_pair_model as fm  # noqa: E402

TOL = 1e-9  # the parity tolerance of the suite: an index mistake shows as O(1); STO costates cancel to ~1e-11


def _manipulator():
    cs = ContactSequence([3, 0, 3], [Event("lift", 0.07, sto=False), Event("impact", 0.15, sto=False, impact_dimf=3)])
    return Dims(7, 7, 0, 3, 3, 48), discretize(14, 14 * 0.02, 0.0, cs)


def _quadruped_like(nv, nu, ns):
    """The trot's grid kinds on another shape (the plugin shape 12:6:6)."""
    _, grids, _ = pr.config_anymal_trot(N=16)
    return Dims(nv, nu, nv - nu, ns, ns, 0), grids


CASES = {
    "anymal_trot": lambda: pr.config_anymal_trot()[:2],
    "anymal_jump_sto": lambda: pr.config_anymal_jump_sto()[:2],
    "iiwa14_7_7_0": lambda: pr.config_iiwa14()[:2],
    "manipulator_7_7_3": _manipulator,
    "plugin_12_6_6": lambda: _quadruped_like(12, 6, 6),
}


def _rel(a, b):
    den = max(np.linalg.norm(a), np.linalg.norm(b), 1e-300)
    return float(np.linalg.norm(a - b) / den)


@pytest.mark.parametrize("case", sorted(CASES))
def test_lane_map_matches_the_oracle_forward_recursion(oracle, case):
    dims, grids = CASES[case]()
    L = capi.layout_for(dims)
    batch = 2
    kkt = pr.make_kkt_batch(L, grids, batch, mode="factory")
    dx0 = pr.make_dx0(L, batch)
    ric_ref = Records(L, "ric").zeros(batch, len(grids))
    d_ref = Records(L, "dir").zeros(batch, len(grids))
    oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric_ref, d_ref, dx0=dx0)
    D = Records(L, "dir")
    N = len(grids) - 1
    m = fm.LaneMap(dims.nv, dims.nu)
    assert m.G * m.TX >= m.nx and m.G * m.TK >= m.nu and 128 * m.TF >= m.NF
    for b in range(batch):
        d = fm.forward_instance(L, grids, kkt[b], ric_ref[b], dx0[b])
        for i, g in enumerate(grids):
            fields = ["dx", "dlmdgmm", "dts"]
            if i < N and g.type != GRID_IMPACT:
                fields.append("du")
            for f in fields:
                a, r = D.f(d[i], f), D.f(d_ref[b, i], f)
                if f == "dts":
                    a, r = a[:2], r[:2]
                assert _rel(a, r) <= TOL, (case, b, i, f, _rel(a, r))
            if i < N and g.switching_constraint and g.dims > 0:
                a, r = D.f(d[i], "dxi")[:g.dims], D.f(d_ref[b, i], "dxi")[:g.dims]
                assert _rel(a, r) <= TOL, (case, b, i, "dxi", _rel(a, r))


def test_anymal_lane_map_counts():
    """ANYmal: 3 columns per load on 54 lanes, 12 loads each for Fxx and P, 4 for K, 2 for Fvu."""
    m = fm.LaneMap(18, 12)
    assert (m.G, m.TX, m.TK, m.TF, int(m.lg.sum())) == (3, 12, 4, 2, 54)
    off, live = m.moff(0)
    assert live[:54].all() and sorted(off[:54].tolist()) == list(range(0, 3 * 36, 2))
