"""The yardstick of rtoc_control_policy / rtoc_control_input (tests/control_policy_restatement.py) and the query times the device
tests run (tests/control_policy_cases.py).  No GPU.

(a) Branch coverage, a condition and not a measurement: the query set of every ANYmal instance -- before t0, exactly t0, the
    interior of an interval, exactly on a grid time, inside the interval that ends at an impact, exactly the event time, just behind
    it, behind tg[N - 2], far beyond the horizon, and the fallback onto an impact -- takes every branch of ControlPolicy::set as
    restated, the two departures included, and the blend at alpha = 1 as well as strictly inside (0, 1).
(b) At alpha = 1 the blend equals record i - 1 bit for bit.
(c) What the restatement cuts out of a record is what include/rtoc_robot.h names, by plain index arithmetic on the packed doubles.
(d) The packed record of rtoc_control_policy: every field on a 64-byte boundary, none overlapping."""
import numpy as np
import pytest

import control_policy_cases as cc
import control_policy_restatement as cpr
import solution_interpolation_cases as cases
from robotoc_amd.types import control_policy_offsets

EXPECTED = {"before_t0": "front", "at_t0": "blend", "interior": "blend", "on_a_grid_time": "blend", "hold_before_impact": "hold",
            "event_time": "blend", "just_behind_event": "blend", "behind_the_last_interval": "back", "far_beyond": "back",
            "fallback_on_an_impact": "back_impact"}


def _instances(phase_based):
    side = cc.anymal_side(phase_based)
    for dt in side["dt"]:
        yield side["types"], cpr.running_times(0.0, dt)


@pytest.mark.parametrize("phase_based", [True, False], ids=["sto", "shared_times"])
def test_the_query_set_takes_every_branch(phase_based):
    for types, tg in _instances(phase_based):
        k = list(types).index(cpr.GRID_IMPACT)
        taken, alphas = set(), {}
        for label, N, t in cpr.query_cases(types, tg):
            branch, a, b, alpha = cpr.select(types, tg, N, t)
            # the interval behind the impact ends at k + 2: within 1 .. N - 2 on the grid with shared times (k = 6 of 11 points),
            # beyond it on the STO grid (k = 7), where both queries at the event fall back to record N - 1
            behind = label in ("event_time", "just_behind_event") and k + 2 > N - 2
            assert branch == ("back" if behind else EXPECTED[label]), (label, branch)
            assert not behind or phase_based
            taken.add(branch)
            alphas[label] = alpha
            if label in ("at_t0", "on_a_grid_time") or (label == "event_time" and not behind):
                assert alpha == 1.0, (label, alpha)
            if label == "event_time":
                assert (a, b) == ((N - 1, None) if behind else (k + 1, k + 2))       # the point behind the impact, never the impact
            if label == "hold_before_impact":
                assert a == k - 1
            if label == "fallback_on_an_impact":
                assert N - 1 == k and a == k - 1
            if label == "behind_the_last_interval":
                assert a == N - 1
        assert taken == set(cpr.BRANCHES)
        assert 0.0 < alphas["interior"] < 1.0 and (phase_based or 0.0 < alphas["just_behind_event"] < 1.0)


def test_no_query_of_the_set_selects_an_impact_record():
    for phase_based in (True, False):
        for types, tg in _instances(phase_based):
            for label, N, t in cpr.query_cases(types, tg):
                _, a, b, _ = cpr.select(types, tg, N, t)
                assert types[a] != cpr.GRID_IMPACT and (b is None or types[b] != cpr.GRID_IMPACT), label


def test_alpha_one_is_the_earlier_record_bit_for_bit():
    model, dims, L, _ = cases.anymal_shape()
    shape = cpr.Shape(L)
    side = cc.anymal_side(False)
    tg = cpr.running_times(0.0, side["dt"][0])
    sol, ric = cc.random_records(L, 1, len(tg), seed=31)
    for i in (0, 1, 3):
        if side["types"][i + 1] == cpr.GRID_IMPACT:
            continue
        got, branch, alpha, scale = cpr.control_policy(shape, side["types"], tg, len(tg) - 1, tg[i], sol[0], ric[0])
        assert branch == "blend" and alpha == 1.0 and scale is None   # handed to the device tests as a copy
        want, later = shape.parts(sol[0, i], ric[0, i]), shape.parts(sol[0, i + 1], ric[0, i + 1])
        for k in want:
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (i, k)
            blended = alpha * want[k] + (1.0 - alpha) * later[k]     # control_policy.cpp:43-51 as written
            assert np.array_equal(blended.view(np.uint64), want[k].view(np.uint64)), (i, k)


@pytest.mark.parametrize("name", ["anymal", "icub", "iiwa14"])
def test_what_is_cut_out_of_a_record(name):
    if name == "anymal":
        L = cases.anymal_shape()[2]
    else:
        L = cc.layout(cc.shapes()[name][0])
    d = L.dims
    nv, nu, nq = d.nv, d.nu, d.nv + (1 if d.np == 6 else 0)
    shape = cpr.Shape(L)
    sol, ric = cc.random_records(L, 1, 1, seed=32)
    p = shape.parts(sol[0, 0], ric[0, 0])
    so, ro = L.sol.off, L.ric.off
    K = ric[0, 0, ro[9]:ro[9] + nu * 2 * nv].reshape(nu, 2 * nv)    # RTOC_RIC_K = 9: nu x 2nv, row-major
    assert np.array_equal(p["tauJ"], sol[0, 0, so[3]:so[3] + nu])   # RTOC_SOL_U = 3
    assert np.array_equal(p["qJ"], sol[0, 0, so[0] + nq - nu:so[0] + nq])
    assert np.array_equal(p["dqJ"], sol[0, 0, so[1] + nv - nu:so[1] + nv])
    assert np.array_equal(p["Kp"], K[:, nv - nu:nv]) and np.array_equal(p["Kd"], K[:, 2 * nv - nu:])
    x = np.random.default_rng(33).normal(size=nq + nv)
    u, mag = cpr.control_input(shape, p, x)
    for i in range(nu):
        want = p["tauJ"][i]
        for c in range(nu):
            want -= K[i, nv - nu + c] * (p["qJ"][c] - x[nq - nu + c])
        for c in range(nu):
            want -= K[i, 2 * nv - nu + c] * (p["dqJ"][c] - x[nq + nv - nu + c])
        assert abs(u[i] - want) <= (2 * nu + 8) * cpr.EPS * mag[i]


@pytest.mark.parametrize("nu", [7, 12, 26, 29])
def test_packed_record_layout(nu):
    off, stride = control_policy_offsets(nu)
    assert all(o % 8 == 0 for o in off.values()) and stride % 8 == 0
    spans = sorted((off[k], off[k] + (nu * nu if k in ("Kp", "Kd") else nu)) for k in off)
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= stride
    rec = np.arange(stride, dtype=float)
    fields, pad = cpr.unpack(nu, rec)
    assert fields["Kp"][2, 1] == off["Kp"] + 2 + 1 * nu      # column-major, leading dimension nu
    assert pad.sum() == stride - 3 * nu - 2 * nu * nu
