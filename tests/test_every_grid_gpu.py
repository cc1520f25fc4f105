"""Every grid structure rtoc_set_grid accepts (tests/grid_words.py: every word up to length 4 and every 8th of length 5, 375 in
all) on every backward path, through the C ABI against the CPU oracle: one parametrised test per (shape, path), the words looped
over inside it on ONE context -- rtoc_set_grid again for every word, so the re-plan on a grid change (the Fxx structure check, the
graph epoch, the scan buffers) runs 375 times as well.  The Riccati and direction records are poisoned with NaN before every
sweep: a record left over from the previous grid cannot pass.

What the words reach that the fixed configurations and the seeded random grids do not: the host segmentation of the register-wide
kernels (launch_backward_rw, rt_sweep.hip) with segments of one stage, segments that begin or end with an impact or a lift,
constraints on point 0 and on the last control point, adjacent constraints (an empty segment); the in-kernel switching-constraint
forms of the register, role-split and tile-split kernels and the scan's element / combine kernels next to every other kind;
RTOC_OPT_WRITEBACK_KKT on the contact path.

Data: "dynamics" only, ANYmal with 6 constraint rows (tests/test_grid_words.py: there the oracle moves by < 1e-13 under a 1e-15
perturbation and solves the dense KKT system to 2.3e-11, so SURVEY 8c's 1e-9 -- 1e-8 through the scan -- is a statement about
the kernels).  Comparison failures are collected over all words and reported together: the pattern of failing words is the
diagnosis.  Anything else -- a non-zero return code of the library included -- ends the test at once.

Observed worst errors over the 375 words: ANYmal 3.1e-14 (every path, scan included), iCub 35 6.5e-15, iCub 32 4.1e-15; the
written-back Qxx, Qxu, Quu, lu 2.1e-14.  What the first run found: the written-back Qxx of every switching-constraint grid point
held -K^T Phiu^T M - (its transpose) -- which the reference subtracts from P alone -- on 321 of the 375 words (every word with a C
or an Lc), in the tile-split and the role-split kernel alike."""
import hashlib

import numpy as np
import pytest

import grid_words as gw
from helpers import check_parity, compare_direction, compare_riccati, rel_err
from robotoc_amd import problems as pr
from robotoc_amd.types import BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, GRID_IMPACT, Records

pytestmark = pytest.mark.gpu

MAX_STAGES, BATCH = 6, 3
WORDS = gw.words(4) + gw.sample(5, 8)
TOL, TOL_SCAN = 1e-9, 1e-8   # SURVEY 8c; the scan as tests/test_scan_gpu.py

# RTOC_OPT_BACKWARD_REGISTER, RTOC_OPT_BACKWARD_WAVES, RTOC_OPT_FXX_STRUCTURE, RTOC_OPT_BACKWARD_SCAN, RTOC_OPT_WRITEBACK_KKT; `ran`: the
# kernel whose run the records must give evidence of ("rw": on the words where it owns a grid point)
PATHS = {
    "register":          dict(register=1, ran="all"),                   # ANYmal default: the register kernel, structured form
    "register_dense":    dict(register=1, fxx=1, ran="all"),            # ... its dense form
    "waves1":            dict(register=0, waves=1),                     # ANYmal: one-wave, role-split pair, tile-split
    "waves2":            dict(register=0, waves=2),
    "waves3":            dict(register=0, waves=3),
    "default":           dict(register=0),                              # ANYmal: structured role-split form; iCub 32: tile-split
    "default_dense":     dict(register=0, fxx=1),                       # ANYmal: the role-split form on a dense Fxx
    "waves4":            dict(register=0, waves=4),                     # iCub 35: the two tile-split variants
    "waves5":            dict(register=0, waves=5),
    "register_wide":     dict(register=2, ran="rw"),                    # iCub: riccati_backward_rw (nv = 32) / _rw2 (nv = 35)
    "scan":              dict(register=1, scan=True, ran="all"),        # backward and forward scan
    "tile_writeback":    dict(register=0, waves="tile", writeback=True),   # (the shape's tile-split variant, below)
    "default_writeback": dict(register=0, writeback=True),              # ANYmal: the role-split kernel's write-back
    "scan_writeback":    dict(register=1, scan=True, writeback=True),
}
TILE_SPLIT_WAVES = {"anymal": 3, "icub32": 4, "icub35": 4}
ROWS = {shape: gw.SHAPES[shape][1] for shape in gw.SHAPES}
CASES = [("anymal", p) for p in ("register", "register_dense", "waves1", "waves2", "waves3", "default", "default_dense", "scan",
                                 "tile_writeback", "default_writeback", "scan_writeback")] + \
        [("icub32", p) for p in ("register_wide", "default", "scan")] + \
        [("icub35", p) for p in ("register_wide", "waves4", "waves5", "scan", "tile_writeback", "scan_writeback")]

# (shape, word) -> inputs and the oracle's result, shared by the paths and left unchanged; one shape at a time (the iCub records of
# 375 words are a gigabyte)
_CASES = {}
_BASELINE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cases_with_the_module():
    yield
    _CASES.clear()


def _case(oracle, shape, word):
    if shape not in _CASES:
        _CASES.clear()
        _CASES[shape] = {}
    c = _CASES[shape].get(word)
    if c is None:
        L = oracle.layout(gw.SHAPES[shape][0])
        grids = gw.build(word, ROWS[shape])
        kkt = pr.make_kkt_batch(L, grids, BATCH, mode="dynamics")
        dx0 = pr.make_dx0(L, BATCH)
        ric_ref, d_ref = Records(L, "ric").zeros(BATCH, len(grids)), Records(L, "dir").zeros(BATCH, len(grids))
        kkt_ref = kkt.copy()   # mutated in place like the reference: what RTOC_OPT_WRITEBACK_KKT leaves in the KKT records
        st_ref = oracle.riccati_sweep_batch(L, grids, kkt_ref, ric_ref, d_ref, dx0=dx0)
        for arr in (kkt, dx0, ric_ref, d_ref, kkt_ref, st_ref):
            arr.setflags(write=False)
        c = _CASES[shape][word] = dict(grids=grids, kkt=kkt, dx0=dx0, ric_ref=ric_ref, d_ref=d_ref, kkt_ref=kkt_ref, st_ref=st_ref)
    return c


def _configure(ctx, shape, cfg):
    ctx.set_backward_register(cfg["register"])
    waves = TILE_SPLIT_WAVES[shape] if cfg.get("waves") == "tile" else cfg.get("waves", 0)
    if waves:
        ctx.set_backward_waves(waves)
    if "fxx" in cfg:
        ctx.set_fxx_structure(cfg["fxx"])
    ctx.set_backward_scan(bool(cfg.get("scan")))
    ctx.set_writeback(bool(cfg.get("writeback")))


def _sweep(ctx, c):
    """One sweep on the grid of case c, every record it must write poisoned beforehand."""
    n = len(c["grids"])
    ctx.set_grid(c["grids"])
    ctx.upload(BUF_KKT, c["kkt"])
    ctx.upload(BUF_DX0, c["dx0"])
    ctx.upload(BUF_RIC, np.full((BATCH, n, ctx.L.ric.stride), np.nan))
    ctx.upload(BUF_DIR, np.full((BATCH, n, ctx.L.dir.stride), np.nan))
    ctx.clear_status()
    ctx.riccati_backward()
    ctx.riccati_forward()
    return ctx.status(), ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")


def _fingerprint(L, grids, ric):
    """The bits of every field compare_riccati looks at (fields one kernel writes and another leaves alone do not count)."""
    R, N, h = Records(L, "ric"), len(grids) - 1, hashlib.sha1()
    for i, g in enumerate(grids):
        for f in ("P", "s") + (("K", "k") if i < N and g.type != GRID_IMPACT else ()):
            h.update(np.ascontiguousarray(R.f(ric[:, i], f)).tobytes())
    return h.digest()


def _baseline(oracle, shape):
    """Register off, default RTOC_OPT_BACKWARD_WAVES: the records every register, register-wide and scan run must differ from."""
    if shape not in _BASELINE:
        from robotoc_amd import capi
        ctx = capi.Context(gw.SHAPES[shape][0], MAX_STAGES, BATCH, 0)
        try:
            _configure(ctx, shape, PATHS["default"])
            fp = {}
            for w in WORDS:
                c = _case(oracle, shape, w)
                st, ric, _ = _sweep(ctx, c)
                assert (st == 0).all(), (gw.name(w), st)
                fp[w] = _fingerprint(ctx.L, c["grids"], ric)
            _BASELINE[shape] = fp
        finally:
            ctx.close()
    return _BASELINE[shape]


def _constrained(g):   # launch_backward_rw's test: such a grid point is a one-stage launch of the tile-split kernel
    return g.type != GRID_IMPACT and g.dims > 0


@pytest.mark.parametrize("shape,path", CASES)
def test_every_grid_structure(oracle, shape, path):
    from robotoc_amd import capi
    cfg = PATHS[path]
    tol = TOL_SCAN if cfg.get("scan") else TOL
    base = _baseline(oracle, shape) if cfg.get("ran") else None
    ctx = capi.Context(gw.SHAPES[shape][0], MAX_STAGES, BATCH, 0)
    failures = []
    try:
        L = ctx.L
        R, K = Records(L, "ric"), Records(L, "kkt")
        _configure(ctx, shape, cfg)
        for w in WORDS:
            c = _case(oracle, shape, w)
            grids, N = c["grids"], len(c["grids"]) - 1
            st, ric, d = _sweep(ctx, c)
            kkt_out = ctx.download_records(BUF_KKT, "kkt") if cfg.get("writeback") else None
            checks = []

            def status():
                assert (st == c["st_ref"]).all() and (st == 0).all(), "status %s, oracle %s" % (st, c["st_ref"])
            checks.append(status)
            for b in range(BATCH):
                checks.append(lambda b=b: compare_riccati(L, grids, ric[b], c["ric_ref"][b], tol, "enumerated grids inst %d" % b,
                                                          check_sto=False))
                checks.append(lambda b=b: compare_direction(L, grids, d[b], c["d_ref"][b], tol, "enumerated grids inst %d" % b))

            def symmetric():
                # the grid points the kernel under test writes itself: all of them, but for the register-wide kernels the
                # unconstrained ones (and the terminal record, theirs or the one-stage launch's: a copy of Qxx)
                own = [i for i, g in enumerate(grids) if not (cfg.get("ran") == "rw" and _constrained(g))]
                P = R.f(ric, "P")[:, own]
                bad = [own[i] for i in range(len(own)) if not np.array_equal(P[:, i], np.swapaxes(P[:, i], -1, -2))]
                assert not bad, "P not exactly symmetric at grid points %s" % bad
            checks.append(symmetric)
            if cfg.get("writeback"):
                def writeback():
                    # the mutated blocks against the oracle's in-place result (Qxu, Quu, lu: grid points with controls)
                    assert not np.array_equal(c["kkt_ref"], c["kkt"])   # the oracle's result differs from the input: not vacuous
                    bad = []
                    for f in ("Qxx", "Qxu", "Quu", "lu"):
                        worst = 0.0
                        for i, g in enumerate(grids[:N]):
                            if f != "Qxx" and g.type == GRID_IMPACT:
                                continue
                            assert not np.array_equal(K.f(c["kkt_ref"][:, i], f), K.f(c["kkt"][:, i], f)), (i, f)
                            e = max(rel_err(K.f(kkt_out[b, i], f), K.f(c["kkt_ref"][b, i], f)) for b in range(BATCH))
                            worst = max(worst, e)
                            if not (e <= TOL):
                                bad.append((i, f, e))
                        if not bad:
                            check_parity("writeback %s" % f, worst, TOL)
                    assert not bad, "written-back KKT blocks (stage, field, rel_err): %s" % bad[:12]
                checks.append(writeback)
            # Evidence that the kernel under test ran: its records differ from the register-off, default-waves run in at least one
            # bit.  Excluded, a genuine coincidence: the scan on the one-point words (R, C) of the iCub shapes.  The value function
            # behind the only control point is the terminal record (P_N = Qxx_N, s_N = -lx_N: copies, no arithmetic of the scan),
            # and the policies come from the tile-split kernel in its one-stage mode, which is those shapes' default kernel too.
            coincides = cfg.get("scan") and shape != "anymal" and len(w) == 1
            if cfg.get("ran") and not coincides and (cfg["ran"] == "all" or any(not _constrained(g) for g in grids[:N])):
                def ran():
                    assert _fingerprint(L, grids, ric) != base[w], "records bit-identical to the register-off default-waves run"
                checks.append(ran)
            for chk in checks:
                try:
                    chk()
                except AssertionError as e:
                    failures.append("%s: %s" % (gw.name(w), e))
    finally:
        ctx.close()
    assert not failures, "%d comparisons failed on %d words (word: what, (stage, field, error)):\n%s" % (
        len(failures), len({f.split(":")[0] for f in failures}), "\n".join(failures[:60]))
