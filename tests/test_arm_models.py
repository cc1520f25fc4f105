"""tests/arm_models.py: the iiwa14 table extended to 8, 9, 12 and 16 joints is a model the CPU rigid-body code handles like the
bundled one -- the two formulations of tests/test_rigid_body_second_formulation.py (recursive Newton-Euler in body coordinates;
articulated-body / composite-rigid-body algorithm in world coordinates) close on each other at that file's 1e-10, and the
central differences of the first agree with its complex-step (analytic to rounding) derivatives at the same bound."""
import json
import os

import numpy as np
import pytest

from arm_models import extended_iiwa14, extended_iiwa14_table
from robotoc_amd import robot_model as rm
from test_rigid_body_second_formulation import _case

SIZES = [8, 9, 12, 16]
BOUND = 1e-10   # tests/test_rigid_body_second_formulation.py, every model


def test_seven_joints_are_the_bundled_table_and_longer_chains_append_joints_3_to_7():
    bundled = json.load(open(os.path.join(rm.MODEL_DIR, "iiwa14.json")))
    assert extended_iiwa14_table(7) == bundled
    assert bytes(extended_iiwa14(7)) == bytes(rm.load_named("iiwa14"))
    d = extended_iiwa14_table(16)
    assert d["nq"] == d["nv"] == len(d["joints"]) == 16 and d["joints"][:7] == bundled["joints"]
    assert len({j["name"] for j in d["joints"]}) == 16
    for i, j in enumerate(d["joints"]):
        assert (j["parent"], j["idx_q"], j["idx_v"]) == (i - 1, i, i)
        if i >= 7:
            src = bundled["joints"][2 + (i - 7) % 5]
            assert j["name"].startswith(src["name"] + "_")
            assert all(j[k] == src[k] for k in ("type", "axis", "placement_R", "placement_p", "mass", "com", "inertia"))
    m = extended_iiwa14(12)
    assert (m.njoints, m.nq, m.nv, m.nu, m.ncontacts) == (12, 12, 12, 12, 0) and not m.floating_base


@pytest.mark.parametrize("nv", SIZES)
def test_the_two_rigid_body_formulations_agree_on_the_extended_arm(oracle, nv):
    m = extended_iiwa14(nv)
    rng = np.random.default_rng(11 + nv)
    z = np.zeros(0)
    worst = dict(closure=0.0, mass=0.0, deriv=0.0)
    for _ in range(4):
        q, v, tau, f, active, rows = _case(m, rng)
        a = oracle.aba_forward_dynamics(m, q, v, tau, f, active)
        idc = oracle.rbd_eval(m, 0, q, v, a, f, tau, active, z)[:nv]
        worst["closure"] = max(worst["closure"], np.abs(idc).max() / max(1.0, np.abs(tau).max()))
        M = oracle.aba_crba(m, q)
        Dq, Dv, Da = oracle.rbd_linearize_cs(m, 0, q, v, a, f, tau, active, z)
        assert np.abs(M - M.T).max() < 1e-13 * np.abs(M).max()
        worst["mass"] = max(worst["mass"], np.abs(M - Da[:nv]).max() / np.abs(M).max(),
                            np.abs(M - oracle.rbd_mass_matrix_world(m, q)).max() / np.abs(M).max())
        dadq, dadv = oracle.aba_linearize_cs(m, q, v, tau, f, active)
        for lhs, rhs in ((Dq[:nv], -M @ dadq), (Dv[:nv], -M @ dadv)):
            worst["deriv"] = max(worst["deriv"], np.abs(lhs - rhs).max() / max(1.0, np.abs(lhs).max()))
    print("nv = %d, first vs second formulation, worst relative deviation:" % nv, worst)
    assert worst["closure"] < BOUND and worst["deriv"] < BOUND
    assert worst["mass"] < 1e-12   # that file's bound of the mass-matrix comparison


@pytest.mark.parametrize("nv", SIZES)
def test_central_differences_agree_with_the_complex_step_on_the_extended_arm(oracle, nv):
    """rbd_linearize_fd (what the GPU tests of the larger arms compare the device's Jacobians with) against rbd_linearize_cs.  One
    central difference of step h carries h^2 f''' / 6 of truncation and eps |f| / h of rounding, together above 1e-10 for every
    h; the Richardson combination (4 D(h/2) - D(h)) / 3 (tests/golden/make_ref_golden.py) removes the h^2 term, and h = 1e-3
    keeps the rounding share at 1e-13 |f|."""
    m = extended_iiwa14(nv)
    rng = np.random.default_rng(31 + nv)
    z = np.zeros(0)
    worst, h = 0.0, 1e-3
    for _ in range(3):
        q, v, a = rm.random_configuration(m, rng, 0.8)
        u = rng.uniform(-20, 20, nv)
        cs = oracle.rbd_linearize_cs(m, 0, q, v, a, z, u, 0, z)
        d1, d2 = oracle.rbd_linearize_fd(m, 0, q, v, a, z, u, 0, z, h), oracle.rbd_linearize_fd(m, 0, q, v, a, z, u, 0, z, h / 2)
        for c, j1, j2 in zip(cs, d1, d2):
            fd = (4.0 * j2 - j1) / 3.0
            worst = max(worst, np.abs(fd - c).max() / max(1.0, np.abs(c).max()))
    print("nv = %d: central differences (Richardson) vs complex step, worst relative %.2e" % (nv, worst))
    assert worst < BOUND
