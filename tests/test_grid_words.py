"""The enumerated grid structures (tests/grid_words.py) on the CPU: the enumeration is what rtoc_set_grid accepts, the oracle
solves the dense whole-horizon KKT system on every word, and it is insensitive enough to rounding-level input changes for the
GPU test's 1e-9 (tests/test_every_grid_gpu.py) to mean something.  "dynamics" data only: on factory data the oracle itself moves
by 1.3e-10 under a 1e-15 perturbation (word R C I I C), too close to 1e-9.  ANYmal words carry 6-row constraints: with
dims == nu == 12 rows twice in a horizon the recursion's elimination order is ill conditioned (word R C C: the oracle and the
dense solve agree to 3e-8 only, the dense solve is stable at 1e-12)."""
import numpy as np
import pytest

import grid_words as gw
from dense_kkt import solve_dense
from helpers import check_parity, rel_err
from robotoc_amd import problems as pr
from robotoc_amd.types import GRID_IMPACT, Records
from test_random_grids import _valid

SETS = sorted(gw.SHAPES)


def test_counts_validator_and_structure_classes():
    counts = {}
    for w in gw.words(5):
        counts[len(w)] = counts.get(len(w), 0) + 1
        assert gw.valid(w) and _valid(gw.build(w, 6)), w
    assert counts == {1: 2, 2: 8, 3: 40, 4: 200, 5: 1000}
    assert len(gw.words(4)) == 250 and len(gw.sample(5, 8)) == 125
    assert gw.sample(5, 8) == [w for w in gw.words(5) if len(w) == 5][::8]
    # nothing the library accepts is left out: every word over KINDS that `valid` refuses breaks one of rtoc_set_grid's rules
    import itertools
    for n in (1, 2, 3):
        for w in itertools.product(gw.KINDS, repeat=n):
            assert gw.valid(w) == _valid(gw.build(w, 6)), w
    short = [" " + gw.name(w) + " " for w in gw.words(4)]
    con = ("C", "Lc")

    def has(pred):
        return any(pred(w) for w in gw.words(4))

    assert has(lambda w: w[0] in con)                                   # a constraint on point 0
    assert has(lambda w: w[-1] in con)                                  # a constraint on the last control point
    assert has(lambda w: any(a in con and b in con for a, b in zip(w, w[1:])))   # two adjacent constraints
    for mid in ("R", "L", "I"):                                         # a single R, L or I between two constraints
        assert has(lambda w: any(a in con and m == mid and b in con for a, m, b in zip(w, w[1:], w[2:]))), mid
    assert has(lambda w: any(a in con and b == "I" for a, b in zip(w, w[1:])))   # an impact directly after a constraint
    assert any(" I I " in s for s in short)                             # two adjacent impacts
    assert any(" I L " in s or " I Lc " in s for s in short)            # a lift directly after an impact


def _rw_launches(grids, terminal_always=False, terminal_never=False):
    """Mirror of launch_backward_rw (robotoc_amd/csrc/rt_sweep.hip): the launches of one backward recursion in order, ("one", st) =
    the tile-split kernel on grid point st alone (st == N: the terminal record), ("seg", hi, lo) = the register-wide kernel, which
    also writes the terminal record when hi == N - 1.  The two switches break the terminal special case on purpose."""
    N = len(grids) - 1

    def constrained(st):
        return grids[st].type != GRID_IMPACT and grids[st].dims > 0
    out = []
    if not terminal_never and (terminal_always or N == 0 or constrained(N - 1)):
        out.append(("one", N))
    hi = N - 1
    while hi >= 0:
        if constrained(hi):
            out.append(("one", hi))
            hi -= 1
            continue
        lo = hi
        while lo > 0 and not constrained(lo - 1):
            lo -= 1
        out.append(("seg", hi, lo))
        hi = lo - 1
    return out


def _writers(grids, launches):
    """grid point -> how often its record is written, and whether every launch finds the value function behind it written."""
    N = len(grids) - 1
    count, ordered = [0] * (N + 1), True
    for ln in launches:
        pts = [ln[1]] if ln[0] == "one" else list(range(ln[1], ln[2] - 1, -1))
        if ln[0] == "seg" and ln[1] == N - 1:
            count[N] += 1
        elif pts[0] < N:
            ordered &= count[pts[0] + 1] > 0
        for p in pts:
            count[p] += 1
    return count, ordered


def test_register_wide_segmentation_writes_every_record_once():
    """The host segmentation of the register-wide kernels on every enumerated word: every grid point and the terminal record are
    written exactly once, in descending order, and no segment holds a constrained grid point.  What the GPU test would list if the
    terminal special case broke: without it (nobody writes the terminal record) exactly the words whose last control point carries
    a constraint; with the one-stage launch on every word the record is written twice wherever a segment ends the horizon."""
    for w in gw.words(5):
        grids = gw.build(w, 6)
        launches = _rw_launches(grids)
        count, ordered = _writers(grids, launches)
        assert count == [1] * len(grids) and ordered, (w, launches)
        for ln in launches:
            if ln[0] == "seg":
                assert ln[1] >= ln[2] and not any(grids[p].dims > 0 and grids[p].type != GRID_IMPACT for p in range(ln[2], ln[1] + 1))
        last_constrained = w[-1] in ("C", "Lc")
        assert (_writers(grids, _rw_launches(grids, terminal_never=True))[0][-1] == 0) == last_constrained, w
        assert (_writers(grids, _rw_launches(grids, terminal_always=True))[0][-1] == 2) == (not last_constrained), w
    kinds = {(ln[0], ln[1] - ln[2] if ln[0] == "seg" else 0) for w in gw.words(4) for ln in _rw_launches(gw.build(w, 6))}
    assert ("seg", 0) in kinds and ("seg", 3) in kinds and ("one", 0) in kinds   # one-stage segments, whole horizons, hand-overs


def _sweep(oracle, L, grids, kkt, dx0):
    R, D = Records(L, "ric"), Records(L, "dir")
    ric, d = R.zeros(kkt.shape[0], len(grids)), D.zeros(kkt.shape[0], len(grids))
    st = oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric, d, dx0=dx0)
    assert (st == 0).all(), st
    return ric, d


@pytest.mark.parametrize("shape", SETS)
def test_oracle_solves_the_dense_kkt_system_on_every_word(oracle, shape):
    """Worst relative error of dx, du, dlmdgmm, dxi per grid point against tests/dense_kkt.py, and status 0 on every word.
    Bound 1e-9.  Observed worst per set: ANYmal (6 rows, 1250 words up to length 5) 2.3e-11; iCub 32 (6 rows, 250 words up to
    length 4) 3.3e-12; iCub 35 (12 rows, 250 words) 4.7e-12."""
    dims, rows, max_len = gw.SHAPES[shape]
    L = oracle.layout(dims)
    D = Records(L, "dir")
    worst, at = 0.0, None
    for w in gw.words(max_len):
        grids = gw.build(w, rows)
        kkt = pr.make_kkt_batch(L, grids, 1, mode="dynamics")
        dx0 = pr.make_dx0(L, 1)
        _, d = _sweep(oracle, L, grids, kkt, dx0)
        ref = solve_dense(L, grids, kkt[0], dx0[0])
        for i, g in enumerate(grids):
            errs = [rel_err(D.f(d[0, i], "dx"), ref["dx"][i]), rel_err(D.f(d[0, i], "dlmdgmm"), ref["lam"][i])]
            if ref["du"][i] is not None:
                errs.append(rel_err(D.f(d[0, i], "du"), ref["du"][i]))
            if ref["dxi"][i] is not None:
                errs.append(rel_err(D.f(d[0, i], "dxi")[:g.dims], ref["dxi"][i]))
            if max(errs) > worst:
                worst, at = max(errs), gw.name(w)
    print("oracle vs dense KKT, %s: worst %.2e at word %s" % (shape, worst, at))
    check_parity("oracle vs dense KKT", worst, 1e-9)


@pytest.mark.parametrize("shape", SETS)
def test_oracle_is_insensitive_to_rounding_level_input_changes(oracle, shape):
    """The KKT batch perturbed by a relative 1e-15: P, s, K, k, dx, du, dlmdgmm per grid point and field, batch 2, must move by
    1e-12 at most -- the condition under which 1e-9 on the GPU is a statement about the kernels and not about the data.
    Observed worst per set: ANYmal 2.3e-14; iCub 32 (6 rows) 7.7e-15; iCub 35 (12 rows) 1.4e-14."""
    dims, rows, max_len = gw.SHAPES[shape]
    L = oracle.layout(dims)
    R, D = Records(L, "ric"), Records(L, "dir")
    rng = np.random.default_rng(1)
    worst, at = 0.0, None
    for w in gw.words(max_len):
        grids = gw.build(w, rows)
        N = len(grids) - 1
        kkt = pr.make_kkt_batch(L, grids, 2, mode="dynamics")
        dx0 = pr.make_dx0(L, 2)
        ric, d = _sweep(oracle, L, grids, kkt, dx0)
        ricp, dp = _sweep(oracle, L, grids, kkt * (1.0 + 1e-15 * rng.standard_normal(kkt.shape)), dx0)
        for b in range(2):
            for i, g in enumerate(grids):
                has_u = i < N and g.type != GRID_IMPACT
                for rec, x, y, fields in ((R, ric, ricp, ("P", "s") + (("K", "k") if has_u else ())),
                                          (D, d, dp, ("dx", "dlmdgmm") + (("du",) if has_u else ()))):
                    for f in fields:
                        e = rel_err(rec.f(x[b, i], f), rec.f(y[b, i], f))
                        if e > worst:
                            worst, at = e, (gw.name(w), i, f)
    print("oracle self-sensitivity, %s: worst %.2e at %s" % (shape, worst, at))
    check_parity("oracle sensitivity to a 1e-15 perturbation", worst, 1e-12)
