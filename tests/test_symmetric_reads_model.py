"""One triangle of Qxx and P, in the lane models, without a GPU.

The register backward kernel (riccati_backward_rv.hpp) starts its F accumulators from the LOWER tiles of Qxx alone; the one-wave
forward kernel (riccati_forward.hpp) requests, at every grid point but the last, only the row pairs of P that reach the
diagonal, and forms the rest of P dx from mirror terms.  tools/rv_model.py and tools/fwd_pair_model.py state both; here they
are held against the oracle on small grids that have every grid-point kind, at the suite's 1e-9, and their load counts
against the figures DESIGN quotes (21 Qxx loads per lane and stage, 342 of 648 pairs of P at 18:12:12)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from robotoc_amd import capi, problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import Dims, GRID_IMPACT, GRID_LIFT, Records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fwd_pair_model as fm  # noqa: E402

TOL = 1e-9


@pytest.fixture(scope="module")
def rv():
    spec = importlib.util.spec_from_file_location("rv_model", os.path.join(ROOT, "tools", "rv_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def trot_small():
    return pr.config_anymal_trot(N=10, dt=0.08)[:2]


def jump_sto_small():
    return pr.config_anymal_jump_sto(N=8, dt=0.08)[:2]


def manipulator():
    cs = ContactSequence([3, 0, 3], [Event("lift", 0.07, sto=False), Event("impact", 0.15, sto=False, impact_dimf=3)])
    return Dims(7, 7, 0, 3, 3, 48), discretize(14, 14 * 0.02, 0.0, cs)


def test_the_small_grids_have_every_grid_point_kind():
    _, g = trot_small()
    assert len(g) == 17
    assert sum(x.type == GRID_LIFT for x in g) == 2 and sum(x.type == GRID_IMPACT for x in g) == 2
    assert sum(bool(x.switching_constraint) and x.dims > 0 for x in g) == 2
    _, g = jump_sto_small()
    assert len(g) == 12
    assert any(x.type == GRID_LIFT and x.sto_next for x in g) and any(x.type == GRID_IMPACT for x in g)
    assert any(bool(x.switching_constraint) and x.dims > 0 for x in g) and any(x.sto for x in g)
    _, g = manipulator()
    assert fm.LaneMap(7, 7).G == 9 and fm.LaneMap(7, 7).nv % 2 == 1


@pytest.mark.parametrize("sa", [True, False], ids=["structured", "dense"])
def test_backward_model_from_the_lower_tiles_on_the_trot(oracle, rv, sa):
    """Every grid point of the small trot, every field."""
    errs = rv.run(stages=None, sa=sa, verbose=False, config=trot_small())
    assert len(errs) == 16
    assert rv.stage.qxx_loads == 21
    for st, e in errs.items():
        assert e["asym"] == 0.0
        for n, v in e.items():
            assert v <= TOL, (st, n, v)


def test_backward_model_from_the_lower_tiles_on_the_jump_sto_grid(oracle, rv):
    """The model carries no switching-time riders (s, k, m differ by them): the matrix half, which is where Qxx enters."""
    errs = rv.run(stages=None, verbose=False, config=jump_sto_small())
    assert len(errs) == 11
    for st, e in errs.items():
        assert e["asym"] == 0.0
        for n in ("P", "K", "M"):
            if n in e:
                assert e[n] <= TOL, (st, n, e[n])


def test_backward_model_never_reads_a_strictly_upper_tile(oracle, rv):
    """NaN in every entry with floor(row / 16) < floor(col / 16) of the Qxx the model reads: the same bits come out."""
    def poison(qxx):
        i, j = np.indices(qxx.shape)
        qxx[(i // 16) < (j // 16)] = np.nan
    clean = rv.run(stages=(3, 7), verbose=False, config=trot_small())
    dirty = rv.run(stages=(3, 7), verbose=False, config=trot_small(), mutate_qxx=poison)
    assert clean == dirty
    assert all(np.isfinite(v) for e in dirty.values() for v in e.values())


FWD_CASES = {"anymal_trot": trot_small, "anymal_jump_sto": jump_sto_small, "manipulator_7_7_3": manipulator,
             "iiwa14_7_7_0": lambda: pr.config_iiwa14()[:2]}


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b), 1e-300))


def _oracle_sweep(oracle, dims, grids, batch=2):
    L = capi.layout_for(dims)
    kkt = pr.make_kkt_batch(L, grids, batch, mode="factory")
    dx0 = pr.make_dx0(L, batch)
    ric = Records(L, "ric").zeros(batch, len(grids))
    d = Records(L, "dir").zeros(batch, len(grids))
    oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric, d, dx0=dx0)
    return L, kkt, dx0, ric, d


@pytest.mark.parametrize("case", sorted(FWD_CASES))
def test_forward_model_from_the_lower_triangle(oracle, case):
    """The directions against the oracle's; then NaN strictly above the diagonal of P at every i < N: the same bits."""
    dims, grids = FWD_CASES[case]()
    L, kkt, dx0, ric, d_ref = _oracle_sweep(oracle, dims, grids)
    D, R = Records(L, "dir"), Records(L, "ric")
    N, nx = len(grids) - 1, 2 * dims.nv
    for b in range(2):
        d = fm.forward_instance(L, grids, kkt[b], ric[b], dx0[b])
        for i, g in enumerate(grids):
            fields = ["dx", "dlmdgmm"] + (["du"] if i < N and g.type != GRID_IMPACT else [])
            for f in fields:
                assert _rel(D.f(d[i], f), D.f(d_ref[b, i], f)) <= (5e-8 if case == "anymal_jump_sto" else TOL), (case, b, i, f)
        dirty = ric[b].copy()
        for i in range(N):
            P = R.f(dirty[i], "P")   # a view of the record: P[i, j] is element (i, j)
            assert P.shape == (nx, nx)
            ri, ci = np.indices(P.shape)
            P[ri < ci] = np.nan
        d2 = fm.forward_instance(L, grids, kkt[b], dirty, dx0[b])
        assert np.isfinite(d2).all()
        assert np.array_equal(d.view(np.int64), d2.view(np.int64))


def test_forward_model_reads_the_terminal_p_in_full(oracle):
    """P_N is the caller's Qxx_N, copied: an O(1) asymmetry must show in the terminal costate as the full product."""
    dims, grids = trot_small()
    L, kkt, dx0, ric, _ = _oracle_sweep(oracle, dims, grids, batch=1)
    D, R = Records(L, "dir"), Records(L, "ric")
    N = len(grids) - 1
    R.f(ric[0, N], "P")[3, 20] += 1.0
    d = fm.forward_instance(L, grids, kkt[0], ric[0], dx0[0])
    PN = R.f(ric[0, N], "P")
    want = PN @ D.f(d[N], "dx") - R.f(ric[0, N], "s")
    assert not np.allclose(PN, PN.T)
    assert _rel(D.f(d[N], "dlmdgmm"), want) <= 1e-12


def test_pair_counts():
    """18:12:12: 342 of the 648 pairs of P are requested; still 12 load instructions."""
    m = fm.LaneMap(18, 12)
    assert fm.p_live_pairs(m) == (342, 648) and m.TX == 12
    # a live pair reaches the diagonal; a silent one lies wholly above it
    for t in range(m.TX):
        live = fm.p_pair_live(m, t)
        j = m.G * t + m.c
        assert ((2 * m.p + 1 >= j) == live)[m.lg].all() and not live[~m.lg].any()
    # 7:7:3: 9 column groups, the second load runs past the matrix
    m = fm.LaneMap(7, 7)
    live, total = fm.p_live_pairs(m)
    assert total == 98 and live == sum(1 for j in range(14) for p in range(7) if 2 * p + 1 >= j)
