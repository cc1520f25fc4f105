"""The yardstick of the crawl, pace and flying-trot planner tests (tests/gait_planner_restatement.py) held to what can be worked
out by hand; the runs of contact statuses and the grids of tests/gait_planner_cases.py held to what the device tests rely on
(every branch visited, every kind of grid point present); and the host side of the gaits: the `gait` member, the GAIT_* values,
the three Python classes' argument checks, reached without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gait_planner_restatement as gpr
from robotoc_amd import capi

Q = np.array([0.3, -0.2, 0.48, 0, 0, 0, 1.0] + [0.0] * 12)
FEET = np.array([[0.34, 0.19, 0.0], [-0.34, 0.19, 0.0], [0.34, -0.19, 0.0], [-0.34, -0.19, 0.0]]) + Q[:3] * [1, 1, 0]
COM = np.array([0.3, -0.2, 0.45])
V0 = np.zeros(18)
GAITS = ("crawl", "pace", "flying_trot")


def _planner(gait, step_length, step_yaw=0.0, stance=False):
    pl = gpr.PLANNERS[gait]()
    if gait == "flying_trot":
        pl.set_gait_pattern(step_length, step_yaw)
    else:
        pl.set_gait_pattern(step_length, step_yaw, stance)
    pl.init(Q, FEET, COM)
    return pl


def _extra(gait):
    return 3 if gait == "flying_trot" else 2


@pytest.mark.parametrize("stance", [False, True])
@pytest.mark.parametrize("gait", GAITS)
def test_zero_step_and_zero_yaw_keep_every_foothold(gait, stance):
    if gait == "flying_trot" and stance:
        stance = False   # no such option: the same planner
    for status in gpr.PLANNERS[gait].STATUSES:
        pl = _planner(gait, np.zeros(3), 0.0, stance)
        if status == 0:
            assert pl.plan(0.0, FEET, V0, 0b1001, 6)   # a flight needs a plan behind it
        assert pl.plan(0.0, FEET, V0, status, 6) and pl.size() == 6 + _extra(gait)
        for s in range(pl.size()):
            assert np.abs(pl.contact_positions(s) - FEET).max() < 1e-15
            assert np.abs(pl.com(s) - pl.com(0)).max() < 1e-15 and np.array_equal(pl.R(s), np.eye(3))


def test_straight_crawl_without_heuristic():
    L = np.array([0.2, 0.0, 0.0])
    for stance, special in ((False, (1, 2)), (True, (1, 3))):
        pl = _planner("crawl", L, 0.0, stance)
        steps = 12
        assert pl.plan(0.0, FEET, V0, 0b1111, steps) and pl.size() == steps + 2 and pl.current_step == 0
        # plan step s + 1 is what the loop leaves at step s.  The moving steps: every one without the stance phase, the odd ones with it
        moving = [s for s in range(1, steps + 1) if not stance or s % 2 == 1]
        assert np.array_equal(pl.com(1), pl.com(0))   # step == 0: nothing moves
        for s in range(1, steps + 1):
            d = pl.com(s + 1) - pl.com(s)
            want = 0.0 if s not in moving else 0.125 if s in special else 0.25
            assert np.allclose(d, want * L, atol=1e-15), (stance, s)
        # the feet in the order RH, RF, LH, LF; half a step where the move is one of the two special steps, else a whole one
        order = (3, 2, 1, 0)
        for n, s in enumerate(moving):
            k = order[n % 4]
            d = pl.contact_positions(s + 1) - pl.contact_positions(s)
            assert np.allclose(d[k], (0.5 if s in special else 1.0) * L, atol=1e-15), (stance, s)
            assert np.array_equal(np.delete(d, k, axis=0), np.zeros((3, 3)))
        # RH and RF make their first move on the special steps, LH and LF never do
        assert [order[n % 4] for n, s in enumerate(moving) if s in special] == [3, 2]
    # with the heuristic the CoM advances a quarter of a step on the two special steps as well
    rb = gpr.CrawlFootStepPlanner()
    rb.set_raibert_gait_pattern([0.4, 0.0, 0.0], 0.0, 0.25, 0.0, 1.0)
    rb.init(Q, FEET, COM)
    assert rb.plan(0.0, FEET, V0, 0b1111, 3)
    assert np.allclose(rb.step_length, [4 * 0.25 * 0.4, 0.0, 0.0])   # period 4 (swing + stance), gain 1: period x vcom_cmd
    for s in (1, 2, 3):
        assert np.allclose(rb.com(s + 1) - rb.com(s), 0.25 * rb.step_length, atol=1e-15)


def test_the_special_crawl_steps_are_tested_on_step_alone():
    """current_step_ = 1 at the first plan (a swing status): step 1 and step 2 still take the half scales (:265, :325)"""
    L = np.array([0.2, 0.0, 0.0])
    pl = _planner("crawl", L)
    assert pl.plan(0.0, FEET, V0, 0b0111, 3) and pl.current_step == 1
    assert np.allclose(pl.com(1) - pl.com(0), 0.125 * L, atol=1e-15) and np.allclose(pl.com(2) - pl.com(1), 0.125 * L, atol=1e-15)
    assert np.allclose(pl.com(3) - pl.com(2), 0.25 * L, atol=1e-15)
    # the centre of mass of a three-foot stance: the mean over the three feet
    want = sum(FEET[i] - pl.local[i] for i in range(3)) / 3.0
    assert np.allclose(pl.com(0), want, atol=1e-15)
    assert np.allclose(pl.contact_positions(0)[3], pl.com(0) + pl.local[3] - 0.5 * L, atol=1e-15)


def test_pace_moves_feet_2_3_then_0_1():
    L = np.array([0.2, 0.0, 0.0])
    pl = _planner("pace", L)
    assert pl.plan(0.0, FEET, V0, 0b1111, 6) and pl.size() == 8
    assert np.allclose(pl.com(2) - pl.com(1), 0.25 * L, atol=1e-15)   # the first step of all
    for s in range(1, 7):
        d = pl.contact_positions(s + 1) - pl.contact_positions(s)
        moved = [k for k in range(4) if np.abs(d[k]).max() > 0]
        assert moved == ([2, 3] if s % 2 == 1 else [0, 1]), s
    ps = _planner("pace", L, 0.0, True)
    assert ps.plan(0.0, FEET, V0, 0b1111, 8)
    for s in range(1, 9):
        d = ps.contact_positions(s + 1) - ps.contact_positions(s)
        moved = [k for k in range(4) if np.abs(d[k]).max() > 0]
        assert moved == ([2, 3] if s % 4 == 1 else [0, 1] if s % 4 == 3 else []), s


def test_flying_trot_is_constant_across_odd_steps_and_one_step_longer():
    L = np.array([0.2, 0.0, 0.0])
    for steps in (0, 1, 7):
        pl = _planner("flying_trot", L, 0.1)
        assert pl.plan(0.0, FEET, V0, 0b1111, steps) and pl.size() == steps + 3
        for s in range(0, steps + 1):   # plan step s + 1 is what the loop leaves at step s
            if s % 2 == 1 or s == 0:
                assert np.array_equal(pl.contact_positions(s + 1), pl.contact_positions(s)) and np.array_equal(pl.com(s + 1), pl.com(s))
                assert np.array_equal(pl.R(s + 1), pl.R(s))
        assert np.array_equal(pl.contact_positions(steps + 2), pl.contact_positions(steps + 1)) and np.array_equal(pl.com(steps + 2), pl.com(steps + 1))
    pl = _planner("flying_trot", L)
    assert pl.plan(0.0, FEET, V0, 0b1111, 8)
    assert np.allclose(pl.com(3) - pl.com(2), 0.25 * L, atol=1e-15) and np.allclose(pl.com(5) - pl.com(4), 0.5 * L, atol=1e-15)
    for s, pair in ((2, [1, 2]), (4, [0, 3]), (6, [1, 2]), (8, [0, 3])):
        d = pl.contact_positions(s + 1) - pl.contact_positions(s)
        assert [k for k in range(4) if np.abs(d[k]).max() > 0] == pair
    # a flight carries the CoM and the footholds of the previous plan's step 0, and does not turn
    pl = _planner("flying_trot", L, 0.2)
    assert pl.plan(0.0, FEET, V0, 0b1001, 2) and pl.current_step == 1
    p0, c0, R0 = pl.contact_positions(0).copy(), pl.com(0).copy(), pl.R(0).copy()
    assert pl.plan(0.1, FEET + 0.5, V0, 0b0000, 2) and pl.current_step == 2
    assert np.array_equal(pl.contact_positions(0), p0) and np.array_equal(pl.com(0), c0) and np.array_equal(pl.R(0), R0)
    # as the first plan it reads an empty vector in the reference; the device refuses it
    with pytest.raises(IndexError):
        _planner("flying_trot", L).plan(0.0, FEET, V0, 0b0000, 2)


def _walk(gait, stance, sequence):
    pl = _planner(gait, np.zeros(3), 0.0, stance)
    out = []
    for status in sequence:
        before = pl.current_step
        assert pl.plan(0.0, FEET, V0, status, 1), (gait, bin(status))
        out.append((status, before, pl.current_step))
    return out


def test_current_step_follows_each_status_sequence():
    import gait_planner_cases as gc
    want = {
        ("pace", False): [0, 1, 2, 0, 0, 1],       # 0b1100 is the even step: it advances from 1 and stays at 0; 0b0011 is the odd one
        ("pace", True): [0, 1, 2, 2, 3, 4],        # 0b1100 belongs at % 4 == 3, 0b0011 at % 4 == 1: both advance from an even step
        ("crawl", False): [0, 1, 2, 3, 4, 5, 0, 1],
        ("crawl", True): [0, 1, 2, 3, 4, 5, 6, 7],
        ("flying_trot", False): [0, 1, 2, 3, 4, 5, 0, 1],
    }
    for (gait, stance), steps in want.items():
        got = _walk(gait, stance, gc.SEQUENCE[gait])
        assert [g[2] for g in got] == steps, (gait, stance, got)
    # a status repeated stays where it is
    assert [g[2] for g in _walk("crawl", False, (0b0111, 0b0111, 0b1011, 0b1011))] == [1, 1, 2, 2]
    assert [g[2] for g in _walk("flying_trot", False, (0b1001, 0b1001, 0b0000, 0b0000, 0b0110, 0b0110))] == [1, 1, 2, 2, 3, 3]
    assert [g[2] for g in _walk("pace", True, (0b0011, 0b0011, 0b1111, 0b1111))] == [1, 1, 2, 2]


def test_the_sequences_of_the_device_test_visit_every_branch():
    """tests/test_gait_planner_gpu.py a): every status of the gait appears; over the ticks of both inits and the three plan
    lengths every residue of the step cycle is planned from, both first-step rules (current_step_ == 0 and beyond) are met, and
    every status is seen both advancing current_step_ and keeping it (the all-feet status: resetting or rounding it)"""
    import gait_planner_cases as gc
    for gait in GAITS:
        cls = gpr.PLANNERS[gait]
        assert set(gc.SEQUENCE[gait]) == set(cls.STATUSES)
        assert gc.SEQUENCE[gait][0] == 0b1111   # nothing but a standing start precedes the first flight
        for stance in ((False, True) if gc.has_stance_option(gait) else (False,)):
            cycle = {"pace": 4 if stance else 2, "crawl": 8 if stance else 4, "flying_trot": 4}[gait]
            pl = _planner(gait, np.zeros(3), 0.0, stance)
            seen, residues = set(), set()
            for status in gc.SEQUENCE[gait]:
                for steps in gc.PLANNING_STEPS:
                    before = pl.current_step
                    assert pl.plan(0.0, FEET, V0, status, steps) and pl.size() == gc.plan_size(gait, steps)
                    seen.add((status, pl.current_step != before))
                    residues.update(s % cycle for s in range(pl.current_step, pl.current_step + steps + 1))
            assert residues == set(range(cycle)), (gait, stance)
            for status in cls.STATUSES:
                if status != 0b1111:
                    assert (status, True) in seen and (status, False) in seen, (gait, stance, bin(status))
            assert (0b1111, False) in seen
            assert (0b1111, True) in seen or (gait == "pace" and stance), (gait, stance)
    assert max(gc.PLANNING_STEPS) >= 8   # every residue mod 8 of the crawl within one plan


@pytest.mark.parametrize("gait", GAITS)
def test_an_illegal_status_returns_false(gait):
    legal = gpr.PLANNERS[gait].STATUSES
    pl = _planner(gait, np.zeros(3))
    assert pl.plan(0.0, FEET, V0, 0b1111, 2)
    for status in range(0b100000):
        if status not in legal:
            assert pl.plan(0.0, FEET, V0, status, 2) is False, bin(status)
    assert pl.current_step == 0 and pl.size() == 2 + _extra(gait)
    # another gait's legal statuses among them
    others = set().union(*(gpr.PLANNERS[g].STATUSES for g in GAITS if g != gait), (0b1001, 0b0110)) - set(legal)
    assert others and all(pl.plan(0.0, FEET, V0, s, 2) is False for s in others)


def test_setters_refuse_what_the_reference_refuses():
    for gait in GAITS:
        pl = gpr.PLANNERS[gait]()
        for bad in ((0.0, 0.1, 0.7), (0.2, -0.1, 0.7), (0.2, 0.1, 0.0)):
            with pytest.raises(ValueError):
                pl.set_raibert_gait_pattern(np.zeros(3), 0.0, *bad)
    with pytest.raises(ValueError):
        gpr.FlyingTrotFootStepPlanner().set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.0, 0.7)   # stance_time <= 0 (:66)
    gpr.PaceFootStepPlanner().set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.0, 0.7)


def test_the_grids_of_the_device_test_hold_what_they_were_chosen_for():
    """tests/test_gait_planner_gpu.py b): at most 12 grid points, every contact phase of the gait on the grid, every grid point's
    mask as many rows as the grid point has, a swinging foot after swing_start_time, and a grid point in flight for the flying trot"""
    import gait_planner_cases as gc
    for gait in GAITS:
        T = gc.GaitGrid(gait)
        assert T.n <= 12 and sorted(set(T.phase)) == [0, 1, 2, 3] and len(T.masks) == T.n and len(T.t) == T.n
        for i in range(T.n - 1):
            assert 3 * bin(int(T.masks[i])).count("1") == T.grids[i].dimf, (gait, i)
        assert T.first_status in gpr.PLANNERS[gait].STATUSES
        swinging = [(i, k) for i in range(T.n) for k in range(4) if T.t[i] > T.start and not (T.phase_masks[T.phase[i]] >> k) & 1]
        assert swinging, gait
        assert max(T.phase) + T.nph < gc.plan_size(gait, 4)   # the references read phase + nph of a plan of 4 steps
        if gait == "flying_trot":
            assert any(T.phase_masks[T.phase[i]] == 0 and T.t[i] > T.start for i in range(T.n))
        if gait == "crawl":
            assert all(bin(mk).count("1") == 3 for mk in T.phase_masks) and {k for _, k in swinging} == {0, 1, 2, 3}
        assert any(T.t[i] <= T.start for i in range(T.n))   # and a grid point ahead of the swing


# ---- the host side of the feature ----
def _header():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rtoc_robot.h")) as f:
        return f.read()


def test_the_planner_struct_has_a_gait_member_where_pad_was():
    fields = dict((name, getattr(capi.FootStepPlanner, name)) for name, _ in capi.FootStepPlanner._fields_)
    assert "gait" in fields and "pad" not in fields
    assert fields["gait"].offset == 12 and fields["gait"].size == 4 and fields["swing_time"].offset == 16
    assert C.sizeof(capi.FootStepPlanner) == 16 + 8 * 11
    assert capi.FootStepPlanner().gait == capi.GAIT_TROT == 0   # a zeroed struct is a trot
    text = _header()
    body = text[text.index("typedef struct rtoc_foot_step_planner {"):text.index("} rtoc_foot_step_planner;")]
    assert re.search(r"\bint gait;", body) and not re.search(r"\bint pad;", body)


def test_the_gait_values_match_the_header():
    text = _header()
    for name in ("TROT", "CRAWL", "PACE", "FLYING_TROT"):
        found = re.search(r"#define RTOC_GAIT_%s (\d+)" % name, text)
        assert found and int(found.group(1)) == getattr(capi, "GAIT_" + name), name
    assert (capi.GAIT_TROT, capi.GAIT_CRAWL, capi.GAIT_PACE, capi.GAIT_FLYING_TROT) == (0, 1, 2, 3)
    # no new entry point: the gaits go through the six the trot has
    assert len(re.findall(r"^int rtoc_foot_step_\w+\(|^int rtoc_set_foot_step_planner\(", text, flags=re.M)) == 6


class _Ctx:
    """a context that records what reaches it"""
    batch = 3

    def __init__(self):
        self.calls = []

    def set_foot_step_planner(self, planner):
        self.calls.append(("set", planner))

    def foot_step_plan(self, t, status, steps):
        self.calls.append(("plan", status, steps))


def test_the_python_classes_check_their_arguments_before_the_library():
    from robotoc_amd import planner as P
    classes = {"crawl": P.CrawlFootStepPlanner, "pace": P.PaceFootStepPlanner, "flying_trot": P.FlyingTrotFootStepPlanner}
    for gait, cls in classes.items():
        ctx = _Ctx()
        pl = cls(ctx)
        assert cls.GAIT == getattr(capi, "GAIT_" + gait.upper()) and tuple(sorted(cls.STATUSES)) == tuple(sorted(gpr.PLANNERS[gait].STATUSES))
        fixed = (np.zeros((2, 3)), 0.0) if gait == "flying_trot" else (np.zeros((2, 3)), 0.0, False)
        with pytest.raises(ValueError):
            pl.set_gait_pattern(*fixed)                                     # neither [3] nor [batch, 3]
        with pytest.raises(ValueError):
            pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.0, 0.1, 0.7)    # the time in the air must be positive
        with pytest.raises(ValueError):
            pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, -0.1, 0.7)
        with pytest.raises(ValueError):
            pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.1, 0.0)
        with pytest.raises(ValueError):
            pl.set_raibert_gait_pattern(np.zeros(3), np.zeros(2), 0.2, 0.1, 0.7)   # yaw rates: a scalar or [batch]
        assert ctx.calls == []
        for status in range(0b100000):
            if status not in cls.STATUSES:
                assert pl.plan(0.0, status, 2) is False
        assert ctx.calls == []
        # what does reach the library carries the gait, for the batch or per instance
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.1, 0.7)
        pl.set_gait_pattern(*((np.ones((3, 3)), 0.1) if gait == "flying_trot" else (np.ones((3, 3)), 0.1, True)))
        one, many = ctx.calls[0][1], ctx.calls[1][1]
        assert isinstance(one, capi.FootStepPlanner) and one.gait == cls.GAIT and one.mode == capi.FOOT_STEP_RAIBERT and one.swing_time == 0.2
        assert len(many) == 3 and all(p.gait == cls.GAIT and p.mode == capi.FOOT_STEP_FIXED for p in many)
        assert all(p.enable_stance_phase == (0 if gait == "flying_trot" else 1) for p in many)
        assert pl.plan(0.0, cls.STATUSES[-1], 2) is True and ctx.calls[-1] == ("plan", cls.STATUSES[-1], 2)
    ctx = _Ctx()
    with pytest.raises(ValueError):
        P.FlyingTrotFootStepPlanner(ctx).set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.0, 0.7)   # stance_time must be positive
    P.PaceFootStepPlanner(ctx).set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.0, 0.7)             # the trot's rule: non-negative
    assert len(ctx.calls) == 1
    assert P.TrotFootStepPlanner.GAIT == capi.GAIT_TROT
