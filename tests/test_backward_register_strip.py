"""The last column tile of the register backward kernel on 4x4x4 MFMAs (riccati_backward_rv.hpp, RvCfg::STRIP4: W[:, 32..36] of ANYmal's
nx = 36 in the D4 layout, converted to the C layout at the seam) on the smallest shapes at which a wrong lane shows: ANYmal 18:12:12,
five instances, a horizon of N = 6 with a regular, a lift, an impact and a switching-constraint grid point (6 rows).  Against the CPU
oracle with the tolerance of tests/test_backward_register.py (1e-9 per stage and field); the strip's own rows and columns of
P, K and the rider's vectors s, k are asserted on their own, so that an error there is not averaged away in the norm of a whole field."""
import numpy as np
import pytest

from helpers import compare_direction, compare_riccati, rel_err
from robotoc_amd import problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import (BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, GRID_IMPACT, GRID_INTERMEDIATE, GRID_LIFT, OPT_BACKWARD_REGISTER,
                               Records, anymal_dims)

pytestmark = pytest.mark.gpu
TOL = 1e-9
BATCH = 5


def _grids():
    cs = ContactSequence([12, 6, 12], [Event("lift", 0.03), Event("impact", 0.09, impact_dimf=6)])
    grids = discretize(6, 0.12, 0.0, cs)
    kinds = [g.type for g in grids[:-1]]
    assert GRID_INTERMEDIATE in kinds and GRID_LIFT in kinds and GRID_IMPACT in kinds
    assert [g.dims for g in grids if g.dims] == [6]
    return grids


def _sweep(ctx, kkt, dx0, register):
    ctx.set_backward_register(register)
    ctx.upload(BUF_KKT, kkt)
    ctx.upload(BUF_DX0, dx0)
    ctx.upload(BUF_RIC, np.full((kkt.shape[0], kkt.shape[1], ctx.L.ric.stride), np.nan))   # poison: every field compared must be WRITTEN
    ctx.clear_status()
    ctx.riccati_backward()
    ctx.riccati_forward()
    return ctx.status(), ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")


@pytest.fixture(scope="module")
def case(oracle):
    """One context, one batch, one oracle reference for every test of this file; the reference and the first sweep stay unchanged."""
    from robotoc_amd import capi
    dims, grids = anymal_dims(), _grids()
    ctx = capi.Context(dims, len(grids), BATCH, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        kkt = pr.make_kkt_batch(L, grids, BATCH, mode="dynamics")
        dx0 = pr.make_dx0(L, BATCH)
        ric_ref, d_ref = Records(L, "ric").zeros(BATCH, len(grids)), Records(L, "dir").zeros(BATCH, len(grids))
        st_ref = oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric_ref, d_ref, dx0=dx0)
        st, ric, d = _sweep(ctx, kkt, dx0, True)
        assert ctx.get_option(OPT_BACKWARD_REGISTER) == 1
        yield dict(ctx=ctx, L=L, dims=dims, grids=grids, kkt=kkt, dx0=dx0, st=st, ric=ric, d=d, st_ref=st_ref, ric_ref=ric_ref, d_ref=d_ref)
    finally:
        ctx.close()


def _strip_fields(c, ric, ric_ref, what):
    """P[:, 32:36], P[32:36, :], s, K[:, 32:36], k of every grid point that has them, each against the oracle on its own."""
    R, grids, nx = Records(c["L"], "ric"), c["grids"], 2 * c["dims"].nv
    n = len(grids) - 1
    for b in range(ric.shape[0]):
        for i, g in enumerate(grids):
            P, Pr = R.f(ric[b, i], "P"), R.f(ric_ref[b, i], "P")
            errs = {"P[:, 32:36]": rel_err(P[:, nx - 4:], Pr[:, nx - 4:]), "P[32:36, :]": rel_err(P[nx - 4:, :], Pr[nx - 4:, :]),
                    "s": rel_err(R.f(ric[b, i], "s"), R.f(ric_ref[b, i], "s"))}
            if i < n and g.type != GRID_IMPACT:
                KT, KTr = R.f(ric[b, i], "K"), R.f(ric_ref[b, i], "K")   # (exposed as K^T: nx x nu)
                errs["K[:, 32:36]"] = rel_err(KT[nx - 4:, :], KTr[nx - 4:, :])
                errs["k"] = rel_err(R.f(ric[b, i], "k"), R.f(ric_ref[b, i], "k"))
            for name, e in errs.items():
                assert e <= TOL, "%s inst %d grid point %d %s: %.3e" % (what, b, i, name, e)


def test_strip_reproduces_the_oracle(case):
    c = case
    assert (c["st"] == c["st_ref"]).all() and (c["st"] == 0).all(), (c["st"], c["st_ref"])
    worst = 0.0
    for b in range(BATCH):
        worst = max(worst, compare_riccati(c["L"], c["grids"], c["ric"][b], c["ric_ref"][b], TOL, "strip inst %d" % b, check_sto=False))
        worst = max(worst, compare_direction(c["L"], c["grids"], c["d"][b], c["d_ref"][b], TOL, "strip inst %d" % b))
    print("register kernel with the 4x4x4 strip vs oracle: worst rel err %.3e" % worst)
    _strip_fields(c, c["ric"], c["ric_ref"], "strip")
    P = Records(c["L"], "ric").f(c["ric"], "P")
    assert np.array_equal(P, np.swapaxes(P, -1, -2))   # mirrored, not recomputed


def test_three_sweeps_repeat_bit_for_bit(case):
    c = case
    first = c["ric"].view(np.int64)
    for rep in range(3):
        st, ric, _ = _sweep(c["ctx"], c["kkt"], c["dx0"], True)
        assert (st == 0).all()
        assert np.array_equal(ric.view(np.int64), first), "sweep %d: %d words differ" % (rep, int((ric.view(np.int64) != first).sum()))


def test_role_split_kernel_agrees_on_the_same_data(case):
    c = case
    st, ric, d = _sweep(c["ctx"], c["kkt"], c["dx0"], False)
    assert c["ctx"].get_option(OPT_BACKWARD_REGISTER) == 0 and (st == 0).all()
    for b in range(BATCH):
        compare_riccati(c["L"], c["grids"], c["ric"][b], ric[b], TOL, "strip vs role-split inst %d" % b, check_sto=False)
        compare_direction(c["L"], c["grids"], c["d"][b], d[b], TOL, "strip vs role-split inst %d" % b)
    _strip_fields(c, c["ric"], ric, "strip vs role-split")


def test_bound_buffers_with_the_structure_checked_in_the_kernel(case):
    """rtoc_bind + RTOC_OPT_FXX_STRUCTURE = 0: the structured form with the kernel's own check of the rows it does not multiply.  Clean
    records reproduce the oracle; one stray entry in a structured row raises RTOC_STAT_FXX_UNSTRUCTURED on that instance alone, and the
    other instances' records are those of the clean sweep, bit for bit."""
    import torch
    from robotoc_amd import capi
    from robotoc_amd.types import STAT_FXX_UNSTRUCTURED
    c = case
    L, grids, n = c["L"], c["grids"], len(c["grids"])
    ctx = capi.Context(c["dims"], n, BATCH, 0)
    try:
        ctx.set_grid(grids)
        ctx.set_backward_register(True)
        ctx.set_fxx_structure(0)
        kkt = torch.from_numpy(c["kkt"].copy()).to("cuda:0")
        ric = torch.full((BATCH, n, L.ric.stride), float("nan"), dtype=torch.float64, device="cuda:0")
        ctx.bind(BUF_KKT, kkt.data_ptr())
        ctx.bind(BUF_RIC, ric.data_ptr())
        torch.cuda.synchronize()
        ctx.riccati_backward()
        ctx.sync()
        assert (ctx.status() == 0).all() and ctx.get_option(OPT_BACKWARD_REGISTER) == 1
        clean = ric.cpu().numpy()
        for b in range(BATCH):
            compare_riccati(L, grids, clean[b], c["ric_ref"][b], TOL, "bound inst %d" % b, check_sto=False)
        _strip_fields(c, clean, c["ric_ref"], "bound")
        assert np.array_equal(clean.view(np.int64), c["ric"].view(np.int64))   # the same kernel as through rtoc_upload
        # instance 3, grid point 2: a stray entry in a structured row of Fxx (row 9, column 30)
        nx, o = 2 * c["dims"].nv, L.kkt.off[0]
        kkt[3, 2, o + 9 + 30 * nx] = 0.125
        ric.fill_(float("nan"))
        torch.cuda.synchronize()
        ctx.clear_status()
        ctx.riccati_backward()
        ctx.sync()
        st = ctx.status()
        assert st[3] & STAT_FXX_UNSTRUCTURED and not np.delete(st, 3).any(), st
        after = ric.cpu().numpy()
        keep = [b for b in range(BATCH) if b != 3]
        assert np.array_equal(after[keep].view(np.int64), clean[keep].view(np.int64))
    finally:
        ctx.close()
