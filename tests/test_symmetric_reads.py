"""One triangle of Qxx and P on the device.

Backward: the register kernel (riccati_backward_rv.hpp; dense, structured and switching-time instantiations) feeds its F
accumulators from the lower 16 x 16 tiles of Qxx alone -- against the oracle, with the strictly upper tiles set to NaN (never
loaded: the same bits come out), and with a Qxx whose triangles differ at round-off.
Forward: the one-wave kernel (riccati_forward.hpp) requests, at every grid point i < N, only the row pairs of P that reach the
diagonal -- against the oracle's forward recursion on the device's own Riccati records for every one-wave shape, with NaN written
strictly above the diagonal of P, with an asymmetric P_N (read in full), and twice over for bit-identical results.

Small grids (problems.config_anymal_trot(N=10, dt=0.08): 17 grid points; config_anymal_jump_sto(N=8, dt=0.08): 12; the 7:7:3
manipulator grid, odd NV and 9 column groups; iiwa14 through the general kernels), 37 distinct instances, bound torch tensors.
tests/test_symmetric_reads_model.py checks on the CPU that the small grids hold every grid-point kind.

Tolerances: the suite's 1e-9 per stage and field, and 5e-8 for the forward recursion of the switching-time grid, whose costate
and multiplier cancel (tests/test_forward_pair_kernel.py).  NaN here is data in a buffer the kernels must not read."""
import numpy as np
import pytest

from helpers import compare_direction, compare_riccati
from robotoc_amd import capi, problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.types import BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, Dims, Records

pytestmark = pytest.mark.gpu
TOL = 1e-9
BATCH = 37


def _manipulator():
    cs = ContactSequence([3, 0, 3], [Event("lift", 0.07, sto=False), Event("impact", 0.15, sto=False, impact_dimf=3)])
    return Dims(7, 7, 0, 3, 3, 48), discretize(14, 14 * 0.02, 0.0, cs)


CASES = {
    "trot": (lambda: pr.config_anymal_trot(N=10, dt=0.08)[:2], "dynamics"),
    "jump_sto": (lambda: pr.config_anymal_jump_sto(N=8, dt=0.08)[:2], "dynamics"),
    "manipulator": (_manipulator, "factory"),
}
_INPUTS = {}


def _inputs(case):
    """(dims, grids, L, kkt, dx0) of a case, generated once and never written."""
    if case not in _INPUTS:
        make, mode = CASES[case]
        dims, grids = make()
        L = capi.layout_for(dims)
        kkt = pr.make_kkt_batch(L, grids, BATCH, mode=mode)
        dx0 = pr.make_dx0(L, BATCH)
        kkt.setflags(write=False)
        dx0.setflags(write=False)
        _INPUTS[case] = (dims, grids, L, kkt, dx0)
    return _INPUTS[case]


class Bound:
    """A context on bound torch tensors (kkt, dx0, ric, dir)."""

    def __init__(self, dims, grids, kkt, dx0, sto=False):
        import torch
        self.torch = torch
        batch, n = kkt.shape[0], len(grids)
        self.ctx = capi.Context(dims, n, batch, 0)
        self.L = self.ctx.L
        self.ctx.set_grid(grids)
        if sto:
            self.ctx.set_max_dts0(0.1)   # the oracle's default
        self.ctx.set_backward_register(2)
        dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda:0").contiguous()
        self.kkt, self.dx0 = dev(kkt), dev(dx0)
        self.ric = torch.zeros((batch, n, self.L.ric.stride), dtype=torch.float64, device="cuda:0")
        self.dir = torch.zeros((batch, n, self.L.dir.stride), dtype=torch.float64, device="cuda:0")
        for b_, t_ in ((BUF_KKT, self.kkt), (BUF_DX0, self.dx0), (BUF_RIC, self.ric), (BUF_DIR, self.dir)):
            self.ctx.bind(b_, t_.data_ptr())
        torch.cuda.synchronize()

    def backward(self):
        self.torch.cuda.synchronize()   # (torch's stream, not the context's)
        self.ctx.riccati_backward()
        self.ctx.sync()
        assert (self.ctx.status() == 0).all()

    def forward(self):
        self.torch.cuda.synchronize()
        self.ctx.riccati_forward()
        self.ctx.sync()
        assert (self.ctx.status() == 0).all()

    def close(self):
        self.ctx.close()


def _bits_equal(torch, a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _poison(torch, field, mask):
    """NaN into the entries `mask` (rows x columns) of every matrix of a [..., rows, columns] view of a bound tensor."""
    m = torch.from_numpy(mask).to(field.device)
    field[..., m] = float("nan")
    assert int(torch.isnan(field).sum()) == int(mask.sum()) * int(np.prod(field.shape[:-2]))


def _oracle_backward(oracle, L, grids, kkt, dx0):
    ric_ref = Records(L, "ric").zeros(kkt.shape[0], len(grids))
    d_ref = Records(L, "dir").zeros(kkt.shape[0], len(grids))
    oracle.riccati_sweep_batch(L, grids, kkt.copy(), ric_ref, d_ref, dx0=np.array(dx0))
    return ric_ref


# ---------------------------------------------------------------- backward ----

@pytest.mark.parametrize("fxx", [0, 1], ids=["structured", "dense"])
@pytest.mark.parametrize("case", ["trot", "jump_sto"])
def test_backward_from_the_lower_tiles_against_the_oracle(oracle, case, fxx):
    dims, grids, L, kkt, dx0 = _inputs(case)
    sto = case == "jump_sto"
    ric_ref = _oracle_backward(oracle, L, grids, kkt, dx0)
    g = Bound(dims, grids, kkt, dx0, sto)
    try:
        g.ctx.set_fxx_structure(fxx)
        g.backward()
        ric = g.ric.cpu().numpy()
        worst = 0.0
        for b in range(BATCH):
            worst = max(worst, compare_riccati(L, grids, ric[b], ric_ref[b], TOL, "%s fxx %d inst %d" % (case, fxx, b), check_sto=sto))
        print("backward %s, RTOC_OPT_FXX_STRUCTURE %d: worst rel err %.3e" % (case, fxx, worst))
    finally:
        g.close()


@pytest.mark.parametrize("case,fxx", [("trot", 0), ("trot", 1), ("jump_sto", 0)], ids=["structured", "dense", "sto"])
def test_backward_never_loads_a_strictly_upper_tile_of_qxx(case, fxx):
    """NaN in every entry with floor(row / 16) < floor(col / 16) of Qxx at i < N: finite records, the same bits."""
    import torch
    dims, grids, L, kkt, dx0 = _inputs(case)
    N = len(grids) - 1
    g = Bound(dims, grids, kkt, dx0, case == "jump_sto")
    try:
        g.ctx.set_fxx_structure(fxx)
        g.backward()
        clean = g.ric.clone()
        i, j = np.indices((2 * dims.nv, 2 * dims.nv))
        _poison(torch, Records(L, "kkt").f(g.kkt[:, :N], "Qxx"), (i // 16) < (j // 16))
        g.ric.zero_()
        g.backward()
        assert torch.isfinite(g.ric).all()
        assert _bits_equal(torch, g.ric, clean)
    finally:
        g.close()


@pytest.mark.parametrize("case", ["trot", "jump_sto"])
def test_backward_with_triangles_of_qxx_that_differ_at_round_off(oracle, case):
    """The strictly lower triangle of every Qxx moved by 1e-16 of the matrix's largest entry: within 1e-9 of the oracle."""
    dims, grids, L, kkt0, dx0 = _inputs(case)
    sto = case == "jump_sto"
    kkt = np.array(kkt0)
    Q = Records(L, "kkt").f(kkt, "Qxx")
    i, j = np.indices(Q.shape[-2:])
    Q[..., i > j] += 1e-16 * np.abs(Q).max(axis=(-1, -2))[..., None]
    assert not np.array_equal(Q, np.swapaxes(Q, -1, -2))
    ric_ref = _oracle_backward(oracle, L, grids, kkt, dx0)
    g = Bound(dims, grids, kkt, dx0, sto)
    try:
        g.backward()
        ric = g.ric.cpu().numpy()
        for b in range(BATCH):
            compare_riccati(L, grids, ric[b], ric_ref[b], TOL, "%s perturbed inst %d" % (case, b), check_sto=sto)
    finally:
        g.close()


# ----------------------------------------------------------------- forward ----

def _iiwa14():
    """iiwa14 (7:7:0) through the general kernels: A, B materialised by the unconstrained backward recursion."""
    dims, grids, info = pr.config_iiwa14()
    L = capi.layout_for(dims)
    kkt = Records(L, "kkt").zeros(BATCH, len(grids))
    for b in range(BATCH):
        pr.fill_unconstr_instance(L, len(grids), kkt[b], np.random.default_rng(pr.BASE_SEED + b))
    return dims, grids, L, kkt, pr.make_dx0(L, BATCH), info["dt"]


def _forward_setup(case):
    """A Bound whose backward recursion has run; the forward call of the case."""
    if case == "iiwa14":
        dims, grids, L, kkt, dx0, dt = _iiwa14()
        g = Bound(dims, grids, kkt, dx0)
        g.ctx.set_unconstr_dense(True)
        g.torch.cuda.synchronize()
        g.ctx.unconstr_backward(dt)
        g.ctx.sync()
        assert (g.ctx.status() == 0).all()

        def fwd():
            g.torch.cuda.synchronize()
            g.ctx.unconstr_forward(dt)
            g.ctx.sync()
            assert (g.ctx.status() == 0).all()
        return g, grids, fwd
    dims, grids, L, kkt, dx0 = _inputs(case)
    g = Bound(dims, grids, kkt, dx0, case == "jump_sto")
    g.backward()
    return g, grids, g.forward


def _oracle_forward(oracle, g, grids):
    """The oracle's forward recursion on the device's own records."""
    kkt, ric, dx0 = g.kkt.cpu().numpy(), g.ric.cpu().numpy(), g.dx0.cpu().numpy()
    d_ref = Records(g.L, "dir").zeros(kkt.shape[0], len(grids))
    oracle.riccati_sweep_batch(g.L, grids, kkt, ric, d_ref, dx0=dx0, backward=False)
    return d_ref


FWD = ["trot", "jump_sto", "manipulator", "iiwa14"]


@pytest.mark.parametrize("case", FWD)
def test_forward_from_the_lower_triangle_against_the_oracle(oracle, case):
    g, grids, fwd = _forward_setup(case)
    try:
        fwd()
        d_ref = _oracle_forward(oracle, g, grids)
        d = g.dir.cpu().numpy()
        tol = 5e-8 if case == "jump_sto" else TOL
        worst = 0.0
        for b in range(BATCH):
            worst = max(worst, compare_direction(g.L, grids, d[b], d_ref[b], tol, "%s inst %d" % (case, b)))
        print("forward %s: worst rel err %.3e" % (case, worst))
    finally:
        g.close()


@pytest.mark.parametrize("case", FWD)
def test_forward_never_uses_p_above_its_diagonal(case):
    """NaN strictly above the diagonal of P at every i < N, after the backward recursion: finite directions, the same bits."""
    import torch
    g, grids, fwd = _forward_setup(case)
    try:
        N = len(grids) - 1
        fwd()
        clean = g.dir.clone()
        nx = 2 * g.L.dims.nv
        i, j = np.indices((nx, nx))
        _poison(torch, Records(g.L, "ric").f(g.ric[:, :N], "P"), i < j)
        g.dir.zero_()
        fwd()
        assert torch.isfinite(g.dir).all()
        assert _bits_equal(torch, g.dir, clean)
    finally:
        g.close()


def test_forward_reads_the_terminal_p_in_full(oracle):
    """P_N is a copy of the caller's Qxx_N and nothing symmetrises it: with an O(1) asymmetry the terminal costate is the
    oracle's full P_N dx - s."""
    g, grids, fwd = _forward_setup("trot")
    try:
        N = len(grids) - 1
        P = Records(g.L, "ric").f(g.ric[:, N], "P")
        P[:, 3, 20] += 1.0
        P[:, 30, 7] -= 0.5
        assert not g.torch.equal(P, P.transpose(-1, -2))
        fwd()
        d_ref = _oracle_forward(oracle, g, grids)
        d = g.dir.cpu().numpy()
        D = Records(g.L, "dir")
        ric = g.ric.cpu().numpy()
        R = Records(g.L, "ric")
        for b in range(BATCH):
            compare_direction(g.L, grids, d[b], d_ref[b], TOL, "asymmetric P_N inst %d" % b)
            want = R.f(ric[b, N], "P") @ D.f(d[b, N], "dx") - R.f(ric[b, N], "s")
            got = D.f(d[b, N], "dlmdgmm")
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), b
    finally:
        g.close()


def test_sweep_repeats_bit_for_bit_at_batch_300():
    import torch
    dims, grids = CASES["trot"][0]()
    out = []
    for _ in range(2):
        ctx = capi.Context(dims, len(grids), 300, 0)
        try:
            L, n = ctx.L, len(grids)
            ctx.set_grid(grids)
            z = lambda w: torch.zeros((300, n, getattr(L, w).stride), dtype=torch.float64, device="cuda:0")
            kkt = pr.make_kkt_batch_unique(L, grids, 300, seed=5, backend="torch", device="cuda:0", out=z("kkt"))
            dx0 = pr.make_dx0_unique(L, 300, seed=5, backend="torch", device="cuda:0").contiguous()
            ric, d = z("ric"), z("dir")
            for b_, t_ in ((BUF_KKT, kkt), (BUF_DX0, dx0), (BUF_RIC, ric), (BUF_DIR, d)):
                ctx.bind(b_, t_.data_ptr())
            torch.cuda.synchronize()
            ctx.riccati_backward()
            ctx.riccati_forward()
            ctx.sync()
            assert (ctx.status() == 0).all()
            out.append((ric, d))
        finally:
            ctx.close()
    assert torch.isfinite(out[0][1]).all()
    assert _bits_equal(torch, out[0][0], out[1][0]) and _bits_equal(torch, out[0][1], out[1][1])
