"""The 4x4x4 strip of the register backward kernel (riccati_backward_rv.hpp, RvCfg::STRIP4) in the lane model, on the CPU: the operand
layout of v_mfma_f64_4x4x4_4b_f64 as tools/rv_model.py states it against a plain einsum over explicitly indexed lanes, the three
identities that let the kernel feed the instruction from registers it already holds, and one stage of every grid-point kind of the trot
-- regular, impact, both switching constraints -- against the oracle with the last column tile in the D4 layout.

Bound of the stage comparison: 1e-12, the bound tests/test_lane_models.py holds the model to.  The products are sums of at most 48 terms
in binary64 (48 x 2^-53 = 5e-15 each) chained three deep, and the strip changes only their summation order; a wrong lane is an error
of order one."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("rv_model", os.path.join(ROOT, "tools", "rv_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mfma4_layout_against_an_einsum(model):
    """A lane = 16 k + 4 blk + i, B lane = 16 k + 4 blk + j, D lane = 16 i + 4 blk + j (tools/probes/mfma4_layout_probe.hip)."""
    rng = np.random.default_rng(1)
    A, B, C = rng.standard_normal((4, 4, 4)), rng.standard_normal((4, 4, 4)), rng.standard_normal((4, 4, 4))   # [blk][i][k], [blk][k][j], [blk][i][j]
    a, b, c = np.zeros(64), np.zeros(64), np.zeros(64)
    for blk in range(4):
        for x in range(4):
            for y in range(4):
                a[16 * y + 4 * blk + x] = A[blk, x, y]
                b[16 * x + 4 * blk + y] = B[blk, x, y]
                c[16 * x + 4 * blk + y] = C[blk, x, y]
    d = model.mfma4(a, b, c)
    want = np.einsum("bik,bkj->bij", A, B) + C
    for blk in range(4):
        for i in range(4):
            for j in range(4):
                assert abs(d[16 * i + 4 * blk + j] - want[blk, i, j]) < 1e-14


def test_the_three_strip_identities(model):
    for seed in range(3):
        assert model.strip_identities(np.random.default_rng(seed)) < 1e-13


def test_seam_moves_every_strip_entry_to_its_c_layout_lane(model):
    """d4_to_c: entry (row 4r + q, column 32 + 4 nb + j) of a row tile leaves lane (q, 4r + j) of block nb for lane (q, 4 nb + j) of register r."""
    LI, Q = model.LI, model.Q
    d0 = 1000.0 + 16.0 * (4 * (LI >> 2) + Q) + (LI & 3)          # 1000 + 16 row + column of the state block
    d1 = np.where((LI & 3) == 0, 2000.0 + 4 * (LI >> 2) + Q, 0.0)   # the rider: 2000 + row on the lanes j = 0
    for r in range(4):
        w = model.d4_to_c(r, d0, d1)
        want = np.where(LI < 4, 1000.0 + 16.0 * (4 * r + Q) + LI, np.where(LI == 4, 2000.0 + 4 * r + Q, 0.0))
        assert np.array_equal(w, want), r


def test_dense_form_with_the_strip_against_the_oracle(oracle, model):
    errs = model.run(stages=(45,), sa=False, strip4=True, verbose=False)
    assert model.stage.mfma4_wf == 63 and model.stage.mfma_wf == 99
    assert max(errs[45].values()) < TOL, errs


def test_every_grid_point_kind_with_the_strip_against_the_oracle(oracle, model):
    errs = model.run(stages=(45, 35, 33, 15), strip4=True, verbose=False)
    # W: 27 of the 114 16x16x4 products became 45 4x4x4 ones (9 k groups x 3 row tiles x 2 blocks less the 3 groups without a
    # state-block entry); F: the 6 the model spends on the corner tile became 6
    assert model.stage.mfma4_wf == 51 and model.stage.mfma_wf == 81
    assert sorted(errs) == [15, 33, 35, 45]
    assert "K" not in errs[35] and "M" in errs[33] and "M" in errs[15] and "M" not in errs[45]   # impact, two constraints, regular
    for st, e in errs.items():
        print("stage", st, {n: float("%.2e" % v) for n, v in e.items()})
        assert e["asym"] == 0.0
        for n, v in e.items():
            assert v < TOL, (st, n, v)
