"""Randomised event structures: contact sequences with random lift / impact times, contact dimensions
and STO flags go through TimeDiscretization (robotoc_amd/grid.py) and the resulting grids -- every
combination of Impact / Lift / switching-constraint / sto / sto_next stage the dispatch of
riccati_recursion.cpp:41-70 can produce -- are swept on the GPU and compared with the oracle.
CPU part: the generator only yields grids the library accepts (no GPU needed to check the validator)."""
import numpy as np
import pytest

from helpers import compare_direction, compare_riccati
from robotoc_amd import problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import (BUF_CDD, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, GRID_IMPACT, GRID_LIFT, GRID_TERMINAL,
                               Records, anymal_dims, icub_dims)


def random_case(seed, dims=None, nmax=22):
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(10, nmax))
    dt = 0.02
    T = N * dt
    nev = int(rng.integers(1, 5))
    # event times at least 2.3 dt apart and away from both ends
    gaps = rng.uniform(2.3, 4.0, nev + 1)
    times = np.cumsum(gaps[:-1]) * dt + rng.uniform(0.2, 0.8) * dt
    sto_on = bool(rng.integers(0, 2))
    dimf = 12
    phase_dimf = [dimf]
    events = []
    for tm in times:
        if tm + 2.5 * dt > T:
            break
        if dimf > 0 and (dimf == 12 or rng.integers(0, 2)):
            new = int(rng.choice([d for d in (0, 6) if d < dimf]))
            events.append(Event("lift", float(tm), sto=sto_on and bool(rng.integers(0, 2))))
        else:
            new = int(rng.choice([d for d in (6, 12) if d > dimf]))
            events.append(Event("impact", float(tm), sto=sto_on and bool(rng.integers(0, 2)),
                                impact_dimf=new - dimf))
        dimf = new
        phase_dimf.append(dimf)
    cs = ContactSequence(phase_dimf, events)
    any_sto = any(e.sto for e in events)
    return (dims if dims is not None else anymal_dims()), discretize(N, T, 0.0, cs, phase_based=any_sto), any_sto


def _valid(grids):
    n = len(grids)
    for i, g in enumerate(grids):
        if g.type == GRID_IMPACT and (i == 0 or i >= n - 2):
            return False
        if g.type == GRID_LIFT and i == 0:
            return False
        if g.dt < 0 or g.dimf > 12 or g.dims > 12:
            return False
    return grids[-1].type == GRID_TERMINAL


def test_generator_produces_varied_valid_grids():
    kinds = set()
    for seed in range(24):
        _, grids, any_sto = random_case(seed)
        assert _valid(grids), seed
        for g in grids:
            kinds.add((g.type, bool(g.sto), bool(g.sto_next), g.dims > 0))
    # impacts, lifts, switching constraints and STO stages all occur
    assert any(k[0] == GRID_IMPACT for k in kinds) and any(k[0] == GRID_LIFT for k in kinds)
    assert any(k[3] for k in kinds) and any(k[1] for k in kinds) and any(k[2] for k in kinds)
    assert len(kinds) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [0, 1, 2, 3])
@pytest.mark.parametrize("seed", range(24))
def test_random_event_structures_match_oracle(oracle, seed, waves):
    """waves: 0 = the default kernel (role-split, 4 instances per workgroup), 1/2/3 = the one-wave,
    role-split pair and tile-split variants (rtoc.h RTOC_OPT_BACKWARD_WAVES)."""
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed)
    batch = 2 + seed % 4    # also odd batches / partial 4-instance workgroups
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        if waves:
            ctx.set_backward_waves(waves)
        kkt = pr.make_kkt_batch(L, grids, batch, mode="dynamics", first_instance=seed)
        dx0 = pr.make_dx0(L, batch, first_instance=seed)
        ctx.upload(BUF_KKT, kkt)
        ctx.upload(BUF_DX0, dx0)
        ctx.riccati_sweep()
        st = ctx.status()
        ric_ref = Records(L, "ric").zeros(batch, len(grids))
        d_ref = Records(L, "dir").zeros(batch, len(grids))
        st_ref = oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric_ref, d_ref, dx0=dx0)
        assert (st == st_ref).all(), (st, st_ref)
        ric, d = ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")
        tol = 1e-9   # SURVEY 8c (observed over all seeds: 2.2e-11 with STO grids, 9.4e-12 without)
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], tol, "seed %d inst %d" % (seed, b))
            compare_direction(L, grids, d[b], d_ref[b], tol, "seed %d inst %d" % (seed, b))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nv,seed", [(32, 3), (32, 8), (35, 5), (35, 11)])
def test_random_event_structures_icub(oracle, nv, seed):
    """The tile-split kernel at iCub size (the only variant for nu > 16) on random event structures."""
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed, icub_dims(nv), nmax=14)
    batch = 2
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        kkt = pr.make_kkt_batch(L, grids, batch, mode="dynamics", first_instance=seed)
        dx0 = pr.make_dx0(L, batch, first_instance=seed)
        ctx.upload(BUF_KKT, kkt)
        ctx.upload(BUF_DX0, dx0)
        ctx.riccati_sweep()
        ric_ref = Records(L, "ric").zeros(batch, len(grids))
        d_ref = Records(L, "dir").zeros(batch, len(grids))
        st_ref = oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric_ref, d_ref, dx0=dx0)
        assert (ctx.status() == st_ref).all()
        ric, d = ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")
        tol = 1e-9   # SURVEY 8c (observed over all seeds: 2.2e-11 with STO grids, 9.4e-12 without)
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], tol, "nv %d seed %d inst %d" % (nv, seed, b))
            compare_direction(L, grids, d[b], d_ref[b], tol, "nv %d seed %d inst %d" % (nv, seed, b))
    finally:
        ctx.close()


STO_SEEDS = (9, 12, 17, 18, 20, 21, 23)   # the seeds whose contact sequence has an event with switching-time optimisation
TOL_SCAN = 1e-8   # SURVEY 8c for the scan (tests/test_scan_gpu.py)


def _inputs_and_reference(oracle, L, grids, batch, seed):
    """Seeded "dynamics" inputs and the oracle's sweep: (kkt, dx0, kkt mutated in place, ric, dir, status)."""
    kkt = pr.make_kkt_batch(L, grids, batch, mode="dynamics", first_instance=seed)
    dx0 = pr.make_dx0(L, batch, first_instance=seed)
    ric_ref = Records(L, "ric").zeros(batch, len(grids))
    d_ref = Records(L, "dir").zeros(batch, len(grids))
    kkt_ref = kkt.copy()
    st_ref = oracle.riccati_sweep_batch(L, grids, kkt_ref, ric_ref, d_ref, dx0=dx0)
    return kkt, dx0, kkt_ref, ric_ref, d_ref, st_ref


def _sweep(ctx, kkt, dx0):
    ctx.upload(BUF_KKT, kkt)
    ctx.upload(BUF_DX0, dx0)
    ctx.upload(BUF_RIC, np.full((kkt.shape[0], kkt.shape[1], ctx.L.ric.stride), np.nan))   # every field compared must be written
    ctx.clear_status()
    ctx.riccati_sweep()
    return ctx.status(), ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")


def test_sto_seeds_are_the_ones_named():
    assert tuple(s for s in range(24) if random_case(s)[2]) == STO_SEEDS
    # on the STO seeds: lifts with switching-time optimisation, more than two events, sto_next on a switching-constraint grid point
    grids = [g for s in STO_SEEDS for g in random_case(s)[1]]
    assert any(g.type == GRID_LIFT and g.sto for g in grids)
    assert any(sum(g.type in (GRID_LIFT, GRID_IMPACT) for g in random_case(s)[1]) > 2 for s in STO_SEEDS)
    assert any(g.dims > 0 and g.sto_next for g in grids)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_random_event_structures_through_the_scan(oracle, seed):
    """RTOC_OPT_BACKWARD_SCAN (backward and, without switching-time optimisation, forward) on every seed; on the STO seeds the
    stage-parallel preparation and the serial vector pass of riccati_scan_sto.hpp with every switching-time field compared."""
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed)
    assert any_sto == (seed in STO_SEEDS)
    batch = 2 + seed % 4
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_backward_scan(True)
        kkt, dx0, _, ric_ref, d_ref, st_ref = _inputs_and_reference(oracle, L, grids, batch, seed)
        st, ric, d = _sweep(ctx, kkt, dx0)
        assert (st == st_ref).all() and (st == 0).all(), (st, st_ref)
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], TOL_SCAN, "scan seed %d inst %d" % (seed, b), check_sto=any_sto)
            compare_direction(L, grids, d[b], d_ref[b], TOL_SCAN, "scan seed %d inst %d" % (seed, b))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", STO_SEEDS)
def test_random_sto_structures_through_the_scan_with_writeback(oracle, seed):
    """RTOC_OPT_WRITEBACK_KKT on a grid with switching-time optimisation: the scan's preparation kernel reads the Quu, lu the policy
    workgroups overwrite, so it is launched by itself ahead of them (launch_backward_scan: ride == false).  Records and the mutated
    Qxx, Qxu, Quu, lu against the oracle's in-place result; both at the scan's 1e-8: the mutated blocks are products with the
    scan's P+."""
    from helpers import check_parity, rel_err
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed)
    assert any_sto
    batch = 2 + seed % 4
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_backward_scan(True)
        ctx.set_writeback(True)
        kkt, dx0, kkt_ref, ric_ref, d_ref, st_ref = _inputs_and_reference(oracle, L, grids, batch, seed)
        st, ric, d = _sweep(ctx, kkt, dx0)
        kkt_out = ctx.download_records(BUF_KKT, "kkt")
        assert (st == st_ref).all() and (st == 0).all(), (st, st_ref)
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], TOL_SCAN, "scan writeback seed %d inst %d" % (seed, b), check_sto=True)
            compare_direction(L, grids, d[b], d_ref[b], TOL_SCAN, "scan writeback seed %d inst %d" % (seed, b))
        K = Records(L, "kkt")
        for f in ("Qxx", "Qxu", "Quu", "lu"):
            worst, bad = 0.0, []
            for i, g in enumerate(grids[:-1]):
                if f != "Qxx" and g.type == GRID_IMPACT:
                    continue
                assert not np.array_equal(K.f(kkt_ref[:, i], f), K.f(kkt[:, i], f)), (i, f)   # not vacuous
                e = max(rel_err(K.f(kkt_out[b, i], f), K.f(kkt_ref[b, i], f)) for b in range(batch))
                worst = max(worst, e)
                if not (e <= TOL_SCAN):
                    bad.append((i, e))
            assert not bad, "written-back %s (stage, rel_err): %s" % (f, bad[:12])
            check_parity("scan writeback " + f, worst, TOL_SCAN)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nv,seed", [(32, 3), (32, 8), (35, 5), (35, 11)])
def test_random_event_structures_icub_register_wide(oracle, nv, seed):
    """RTOC_OPT_BACKWARD_REGISTER = 2 on the seeds of test_random_event_structures_icub: riccati_backward_rw (nv = 32) and
    riccati_backward_rw2 (nv = 35) on random event structures; not bit-identical to the tile-split kernel: it ran."""
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed, icub_dims(nv), nmax=14)
    assert not any_sto
    batch = 2
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_backward_register(2)
        kkt, dx0, _, ric_ref, d_ref, st_ref = _inputs_and_reference(oracle, L, grids, batch, seed)
        st, ric, d = _sweep(ctx, kkt, dx0)
        assert (st == st_ref).all(), (st, st_ref)
        tol = 1e-9
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], tol, "register-wide nv %d seed %d inst %d" % (nv, seed, b))
            compare_direction(L, grids, d[b], d_ref[b], tol, "register-wide nv %d seed %d inst %d" % (nv, seed, b))
        ctx.set_backward_register(0)
        _, ric0, _ = _sweep(ctx, kkt, dx0)
        assert not np.array_equal(ric, ric0, equal_nan=True)
    finally:
        ctx.close()


ICUB_STO_CASES = [(32, 18), (35, 17)]   # lift with sto_next, a switching constraint inside the STO phases, an impact with sto


def test_icub_sto_seeds_are_well_conditioned(oracle):
    """The iCub STO seeds are chosen by the oracle's own conditioning: under a 1e-15 perturbation of the inputs every compared
    field moves by less than 1e-12 (observed 4.6e-14 / 2.9e-14), so SURVEY 8c's 1e-9 holds the kernel.  On the seeds 12 (both
    sizes), 20 and 21 (nv = 35) one instance has a Phi that is zero but for rounding, which the oracle itself moves by O(1)."""
    for nv, seed in ICUB_STO_CASES:
        dims, grids, any_sto = random_case(seed, icub_dims(nv), nmax=14)
        assert any_sto
        L = oracle.layout(dims)
        kkt, dx0, _, ric_ref, d_ref, _ = _inputs_and_reference(oracle, L, grids, 2, seed)
        ric, d = Records(L, "ric").zeros(2, len(grids)), Records(L, "dir").zeros(2, len(grids))
        oracle.riccati_sweep_batch(L, grids, kkt * (1.0 + 1e-15 * np.random.default_rng(1).standard_normal(kkt.shape)), ric, d, dx0=dx0)
        for b in range(2):
            compare_riccati(L, grids, ric[b], ric_ref[b], 1e-12, "oracle sensitivity nv %d inst %d" % (nv, b), check_sto=True)
            compare_direction(L, grids, d[b], d_ref[b], 1e-12, "oracle sensitivity nv %d inst %d" % (nv, b))


@pytest.mark.gpu
@pytest.mark.parametrize("nv,seed", ICUB_STO_CASES)
def test_random_sto_structures_icub_keep_the_tile_split_kernel(oracle, nv, seed):
    """A grid with switching-time optimisation at iCub size: the register-wide kernels do not cover it, so with
    RTOC_OPT_BACKWARD_REGISTER = 2 plan_backward keeps the tile-split kernel -- the records equal the run with 0 bit for bit --
    and the oracle is reproduced, switching-time fields included."""
    from robotoc_amd import capi
    dims, grids, any_sto = random_case(seed, icub_dims(nv), nmax=14)
    assert any_sto
    batch = 2
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_backward_register(2)
        kkt, dx0, _, ric_ref, d_ref, st_ref = _inputs_and_reference(oracle, L, grids, batch, seed)
        st, ric, d = _sweep(ctx, kkt, dx0)
        assert (st == st_ref).all(), (st, st_ref)
        tol = 1e-9
        for b in range(batch):
            compare_riccati(L, grids, ric[b], ric_ref[b], tol, "sto nv %d seed %d inst %d" % (nv, seed, b), check_sto=True)
            compare_direction(L, grids, d[b], d_ref[b], tol, "sto nv %d seed %d inst %d" % (nv, seed, b))
        ctx.set_backward_register(0)
        st0, ric0, d0 = _sweep(ctx, kkt, dx0)
        assert np.array_equal(ric, ric0, equal_nan=True) and np.array_equal(d, d0, equal_nan=True) and (st0 == st).all()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_event_structures_condense_expand(oracle, seed):
    """Contact-dynamics condensation / expansion on the same random structures: every mix of nf in
    {0, 6, 12}, impact stages and switching-constraint stages (condenseContactDynamics /
    condenseImpactDynamics / expand*) against the oracle."""
    from robotoc_amd import capi
    dims, grids, _ = random_case(seed)
    batch = 2
    ctx = capi.Context(dims, len(grids), batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        kkt, cdd = pr.make_precondense_batch(L, grids, batch, first_instance=seed)
        dx0 = pr.make_dx0(L, batch, first_instance=seed)
        for buf, arr in ((BUF_KKT, kkt), (BUF_CDD, cdd), (BUF_DX0, dx0)):
            ctx.upload(buf, arr)
        # odd seeds: RTOC_OPT_CONDENSE_KEEP_QAF (Qafqv / Qafu_full stored and compared); even seeds: the default, where
        # the condensation does not store them and the expansion must still come out right
        keep = bool(seed & 1)
        ctx.set_condense_keep_qaf(keep)
        ctx.condense()
        kkt_gpu = ctx.download_records(BUF_KKT, "kkt")
        cdd_gpu = ctx.download_records(BUF_CDD, "cdd")
        ctx.riccati_sweep()
        ctx.expand(0.995)
        d_gpu = ctx.download_records(BUF_DIR, "dir")
        assert (ctx.status() == 0).all()
        kk, cc = kkt.copy(), cdd.copy()
        assert (oracle.condense_batch(L, grids, kk, cc) == 0).all()
        K, C, D = Records(L, "kkt"), Records(L, "cdd"), Records(L, "dir")
        from helpers import rel_err
        for f in ("Qxx", "Qxu", "Quu", "lx", "lu", "Fxx", "Fvu", "Fx", "Phix", "Phiu", "Pres"):
            assert rel_err(K.f(kkt_gpu, f), K.f(kk, f)) < 1e-9, (seed, f)
        for f in ("MJtJinv", "MJtJinv_dIDCdqv", "MJtJinv_IDC", "laf") + (("Qafqv", "Qafu_full") if keep else ()):
            assert rel_err(C.f(cdd_gpu, f), C.f(cc, f)) < 1e-9, (seed, f)
        ric_ref, d_ref = Records(L, "ric").zeros(batch, len(grids)), D.zeros(batch, len(grids))
        oracle.riccati_sweep_batch(L, grids, kk, ric_ref, d_ref, dx0=dx0)
        oracle.expand_batch(L, grids, cc, d_ref)
        for f in ("dx", "du", "dlmdgmm", "daf", "dbetamu", "dnu_passive"):
            from helpers import check_parity
            check_parity("sqp directions " + f, rel_err(D.f(d_gpu, f), D.f(d_ref, f)), 1e-9)
    finally:
        ctx.close()
