"""The one-wave forward Riccati kernel (riccati_forward.hpp: row pairs x column groups, 16-B loads, partial sums reduced
through LDS) at the batches the bench runs: jump-STO at full size against the oracle in every instance, grid point and
direction field; the odd-NV iiwa14 + point contact shape (7:7:3, 8-B columns of Fvu and M) at a batch above the CU count;
and the headline batch repeated bit for bit."""
import numpy as np
import pytest

from robotoc_amd import problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, Dims, GRID_IMPACT, Records

TOL = 1e-9


def _rows_rel_err(a, b):
    """Relative Frobenius error per instance: a, b are [batch, ...]."""
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    den = np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), 1e-300)
    return np.linalg.norm(a - b, axis=1) / den


def _check_directions(L, grids, d, d_ref, tol):
    """Every instance, grid point and field of the direction records (dx, dlmdgmm, du, dxi, dts)."""
    D = Records(L, "dir")
    N = len(grids) - 1
    worst = {}
    for i, g in enumerate(grids):
        fields = [("dx", None), ("dlmdgmm", None)]
        if i < N and g.type != GRID_IMPACT:
            fields.append(("du", None))
        if i < N and g.switching_constraint and g.dims > 0:
            fields.append(("dxi", g.dims))
        for f, n in fields:
            a, b = D.f(d[:, i], f), D.f(d_ref[:, i], f)
            if n is not None:
                a, b = a[:, :n], b[:, :n]
            e = float(_rows_rel_err(a, b).max())
            worst[f] = max(worst.get(f, 0.0), e)
            assert e <= tol, (i, f, e)
        a, b = D.f(d[:, i], "dts")[:, :2], D.f(d_ref[:, i], "dts")[:, :2]
        e = float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)).max())
        worst["dts"] = max(worst.get("dts", 0.0), e)
        assert e <= tol, (i, "dts", e)
    return worst


def _sweep_against_oracle(oracle, dims, grids, batch, mode, tol=TOL):
    from robotoc_amd import capi
    ctx = capi.Context(dims, len(grids) + 2, batch, 0)  # as test_gpu_parity.py sizes it
    try:
        L = ctx.L
        ctx.set_grid(grids)
        ctx.set_max_dts0(0.1)  # the oracle's default below
        kkt = pr.make_kkt_batch(L, grids, batch, mode=mode)  # one distinct instance per index
        dx0 = pr.make_dx0(L, batch)
        ctx.upload(BUF_KKT, kkt)
        ctx.upload(BUF_DX0, dx0)
        ctx.riccati_backward()
        ctx.riccati_forward()
        st = ctx.status()
        d = ctx.download_records(BUF_DIR, "dir")
        # the oracle's forward recursion on the device's own Riccati records: what is compared is the forward kernel
        ric = ctx.download_records(BUF_RIC, "ric")
        d_ref = Records(L, "dir").zeros(batch, len(grids))
        oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric, d_ref, dx0=dx0, backward=False)
        assert (st == 0).all()
        worst = _check_directions(L, grids, d, d_ref, tol)
        print("worst rel err per field", worst)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_jump_sto_full_batch_against_oracle(oracle):
    """configs[2] (ANYmal jump with STO): 4096 distinct instances, every lift / impact / STO rider of the kernel."""
    dims, grids, _ = pr.config_anymal_jump_sto()
    # the costate and the multiplier of the STO switching grid point cancel (P dx - s + Psi (dts+ - dts) - Phi dts+,
    # M dx + m + mt (dts+ - dts)).  On these 4096 instances the former row-walk kernel is 1.35e-9 / 8.8e-9 away from the
    # oracle there, this kernel 1.7e-9 / 1.05e-8; dx, du and dts stay below 1e-11 for both
    _sweep_against_oracle(oracle, dims, grids, 4096, "dynamics", tol=5e-8)


@pytest.mark.gpu
def test_odd_nv_manipulator_above_cu_count(oracle):
    """7:7:3 (iiwa14 + one point contact): odd NV, contact -> lift -> flight -> impact -> contact, 600 instances."""
    dims = Dims(7, 7, 0, 3, 3, 48)
    cs = ContactSequence([3, 0, 3], [Event("lift", 0.07, sto=False), Event("impact", 0.15, sto=False, impact_dimf=3)])
    grids = discretize(14, 14 * 0.02, 0.0, cs)
    _sweep_against_oracle(oracle, dims, grids, 600, "factory")


def _headline_directions(torch, batch):
    from robotoc_amd import capi
    dims, grids, _ = pr.config_anymal_trot()
    n = len(grids)
    ctx = capi.Context(dims, n, batch, 0)
    try:
        L = ctx.L
        ctx.set_grid(grids)
        z = lambda w: torch.zeros((batch, n, getattr(L, w).stride), dtype=torch.float64, device="cuda:0")
        kkt = pr.make_kkt_batch_unique(L, grids, batch, seed=1, backend="torch", device="cuda:0", out=z("kkt"))
        dx0 = pr.make_dx0_unique(L, batch, seed=1, backend="torch", device="cuda:0").contiguous()
        ric, d = z("ric"), z("dir")
        for b_, t_ in ((BUF_KKT, kkt), (BUF_DX0, dx0), (BUF_RIC, ric), (BUF_DIR, d)):
            ctx.bind(b_, t_.data_ptr())
        ctx.riccati_backward()
        ctx.riccati_forward()
        ctx.sync()
        assert (ctx.status() == 0).all()
        return d
    finally:
        ctx.close()


@pytest.mark.gpu
def test_headline_forward_repeats_bit_for_bit():
    """4096 distinct ANYmal trot instances, the sweep run twice from the same inputs: bit-identical directions."""
    import torch
    first = _headline_directions(torch, 4096)
    second = _headline_directions(torch, 4096)
    assert torch.isfinite(first).all()
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
