"""tests/biped_walk_restatement.py held to facts derived by hand from src/mpc/biped_walk_foot_step_planner.cpp, the host side of
RTOC_GAIT_BIPED_WALK without a device (the header's value, the Python class's argument checks), and the runs of contact statuses and
the grids of tests/test_biped_walk_gpu.py held to what they are chosen for."""
import os
import re

import numpy as np
import pytest

import biped_walk_cases as bc
import biped_walk_restatement as bwr
import foot_step_planner_restatement as fsr
from robotoc_amd import capi

L = 0.2
BASE = np.array([1.0, 2.0, 0.6])


def _quat_yaw(yaw):
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw)])


def _pose(yaw=0.0, tilt=0.0):
    """q (base at BASE, yawed), the feet 0.07 m to the left and to the right of the base and 0.6 m below it, the soles turned with
    the base and pitched by `tilt`, the centre of mass 0.1 m below the base"""
    q = np.concatenate([BASE, _quat_yaw(yaw)])
    R0 = fsr.yaw_matrix(yaw)
    feet = np.array([BASE + R0 @ np.array([0.0, 0.07, -0.6]), BASE + R0 @ np.array([0.0, -0.07, -0.6])])
    c, s = np.cos(tilt), np.sin(tilt)
    pitch = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    surfaces = np.array([R0 @ pitch, R0 @ pitch.T])
    return q, feet, surfaces, BASE + np.array([0.0, 0.0, -0.1])


def _planner(q, feet, com, step_length=(0, 0, 0), yaw=0.0, dsp=False):
    pl = bwr.BipedWalkFootStepPlanner(yaw_projection=True)
    pl.set_gait_pattern(step_length, yaw, dsp)
    pl.init(q, feet, com)
    return pl


def test_init_measures_the_legs_from_the_base():
    q, feet, surfaces, com = _pose(yaw=0.4)
    pl = _planner(q, feet, com)
    assert abs(pl.left_to_right_leg_distance - 0.14) < 1e-15      # :96-97: local y of the left foot minus the right one's
    assert abs(pl.foot_height_to_com_height - 0.5) < 1e-15        # :98-100: the CoM 0.1 below the base, the feet 0.6 below
    assert np.allclose(pl.R(0), fsr.yaw_matrix(0.4), atol=1e-15) and pl.current_step == 0 and pl.size() == 0


@pytest.mark.parametrize("dsp", (False, True))
def test_zero_step_and_zero_yaw_keep_every_foothold(dsp):
    # flat soles turned with the base: the kinematics' rotations ARE R, so the moving foot's `rotation = R` changes nothing either
    q, feet, surfaces, com = _pose(yaw=0.3)
    pl = _planner(q, feet, com, dsp=dsp)
    assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), 0b11, 6) and pl.size() == 8
    for s in range(8):
        assert np.array_equal(pl.contact_positions(s), feet)
        assert np.allclose(pl.contact_surfaces(s), surfaces, atol=1e-15)
        assert np.allclose(pl.com(s), 0.5 * (feet[0] + feet[1]) + [0, 0, 0.5], atol=1e-15)
    # pitched soles: a foot that has not moved keeps the kinematics' own rotation bit for bit, a foot that has takes R
    q, feet, surfaces, com = _pose(yaw=0.3, tilt=0.2)
    pl = _planner(q, feet, com, dsp=dsp)
    assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), 0b11, 6)
    assert np.array_equal(pl.contact_surfaces(0), surfaces) and np.array_equal(pl.contact_surfaces(1), surfaces)
    first_right, first_left = 2, (4 if dsp else 3)   # plan step = loop step + 1: the right foot moves on loop step 1
    assert np.array_equal(pl.contact_surfaces(first_right)[1], pl.R(first_right)) and np.array_equal(pl.contact_surfaces(first_right)[0], surfaces[0])
    assert np.array_equal(pl.contact_surfaces(first_left)[0], pl.R(first_left))


@pytest.mark.parametrize("dsp", (False, True))
def test_a_straight_walk_without_the_heuristic(dsp):
    q, feet, surfaces, com = _pose()
    pl = _planner(q, feet, com, step_length=(L, 0, 0), dsp=dsp)
    n = 9
    assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), 0b11, n)
    x = np.array([[pl.contact_positions(s)[0][0], pl.contact_positions(s)[1][0], pl.com(s)[0]] for s in range(n + 2)]) - BASE[0]
    left, right, com_x = [0.0], [0.0], [0.0]
    moves = 0
    for step in range(n + 1):   # the loop's `step`, current_step_ = 0
        moving = step > 0 and (step % 2 == 1 if dsp else True)   # with double support nothing moves on even steps
        if moving:
            moves += 1
            foot = right if (step % 4 == 1 if dsp else step % 2 == 1) else left   # the right foot first, then they alternate
            foot[0] += 0.5 * L if moves == 1 else L
            com_x[0] += 0.25 * L if moves == 1 else 0.5 * L
        assert np.allclose(x[step + 1], [left[0], right[0], com_x[0]], atol=1e-15), (step, x[step + 1])
    assert moves == (5 if dsp else 9) and right[0] > 0 and left[0] > 0
    assert np.allclose(x[0], 0.0) and np.allclose(x[1], 0.0)   # plan steps 0 and 1: where the feet stand
    # y, z and every rotation stay
    for s in range(n + 2):
        assert np.allclose(pl.contact_positions(s)[:, 1:], feet[:, 1:], atol=1e-15) and np.allclose(pl.R(s), np.eye(3), atol=1e-15)


@pytest.mark.parametrize("dsp", (False, True))
def test_pure_yaw_composes_r_yaw_once_per_moving_step(dsp):
    th = 0.1
    q, feet, surfaces, com = _pose(yaw=0.3, tilt=0.2)
    pl = _planner(q, feet, com, yaw=th, dsp=dsp)
    assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), 0b11, 8)
    moves = 0
    for step in range(9):
        moving = step > 0 and (step % 2 == 1 if dsp else True)
        moves += moving
        assert np.allclose(pl.R(step + 1), fsr.yaw_matrix(0.3 + moves * th), atol=1e-15)
        if moving:
            foot = 1 if (step % 4 == 1 if dsp else step % 2 == 1) else 0
            assert np.array_equal(pl.contact_surfaces(step + 1)[foot], pl.R(step + 1))
        assert np.array_equal(pl.contact_positions(step + 1), feet)   # a zero step length moves no foot


@pytest.mark.parametrize("status", (0b01, 0b10))
def test_the_single_support_formula_written_out(status):
    """:148-191 for one pose: the swing foot at R (local_stance - 0.5 R_yaw^T step_length -/+ distance e_y) + q.head<3>() with
    rotation R, R = R_yaw R_.front() (current_step_ = 0 is neither 1 nor, for 0b10 ... see below), the CoM the midpoint plus the height"""
    th, yaw0 = 0.15, 0.3
    sl = np.array([0.2, 0.05, 0.0])
    q, feet, surfaces, com = _pose(yaw=yaw0, tilt=0.2)
    feet = feet + np.array([[0.03, 0.0, 0.0], [-0.02, 0.01, 0.0]])   # not side by side
    pl = _planner(q, feet, com, step_length=sl, yaw=th)
    distance = (fsr.yaw_matrix(yaw0).T @ (feet[0] - feet[1]))[1]
    assert abs(pl.left_to_right_leg_distance - distance) < 1e-15
    assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), status, 0)
    R0, Ry = fsr.yaw_matrix(yaw0), fsr.yaw_matrix(th)
    if status == 0b01:   # the left foot stands: current_step_ 0 -> 1 (0 % 2 != 1), R turns, the right foot is placed
        R = Ry @ R0
        stance, swing, sign, cur = 0, 1, -1.0, 1
    else:                # the right foot stands: current_step_ % 2 == 0 already, no turn, the left foot is placed
        R = R0
        stance, swing, sign, cur = 1, 0, +1.0, 0
    local = R0.T @ (feet[stance] - BASE) - 0.5 * (Ry.T @ sl) + sign * distance * np.array([0.0, 1.0, 0.0])
    want = R @ local + BASE
    assert pl.current_step == cur
    assert np.allclose(pl.contact_positions(0)[swing], want, atol=1e-15) and np.array_equal(pl.contact_positions(0)[stance], feet[stance])
    assert np.allclose(pl.contact_surfaces(0)[swing], R, atol=1e-15) and np.array_equal(pl.contact_surfaces(0)[stance], surfaces[stance])
    assert np.allclose(pl.com(0), 0.5 * (want + feet[stance]) + [0, 0, pl.foot_height_to_com_height], atol=1e-15)
    assert np.allclose(pl.R(0), R, atol=1e-15)


def test_current_step_under_every_status():
    q, feet, surfaces, com = _pose()
    # (status, current_step_ afterwards) in a run; without double support: 0b11 resets, 0b01 wants odd, 0b10 wants even
    runs = {False: [(0b01, 1), (0b01, 1), (0b10, 2), (0b10, 2), (0b01, 3), (0b11, 0), (0b10, 0), (0b01, 1), (0b11, 0)],
            # with it: 0b11 goes to the next even number, 0b01 wants % 4 == 1, 0b10 wants % 4 == 3
            True: [(0b11, 0), (0b01, 1), (0b01, 1), (0b11, 2), (0b11, 2), (0b10, 3), (0b10, 3), (0b11, 4), (0b01, 5), (0b10, 6), (0b10, 7),
                   (0b01, 8), (0b01, 9)]}
    for dsp, run in runs.items():
        pl = _planner(q, feet, com, yaw=0.1, dsp=dsp)
        yaws = 0
        for status, want in run:
            before = pl.current_step
            assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), status, 1)
            assert pl.current_step == want, (dsp, bin(status), want)
            yaws += status != 0b11 and pl.current_step != before   # R turns exactly when a single-support status advances
            assert np.allclose(pl.R(0), fsr.yaw_matrix(0.1 * yaws), atol=1e-14)
        for status in (0b00, 0b100, 0b111, 0b1111):
            assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), status, 1) is False


def test_the_raibert_step_length_and_the_setters_checks():
    q, feet, surfaces, com = _pose()
    pl = bwr.BipedWalkFootStepPlanner(yaw_projection=True)
    for bad in ((0.0, 0.1, 0.7), (0.2, -0.1, 0.7), (0.2, 0.1, 0.0)):   # :66-74
        with pytest.raises(ValueError):
            pl.set_raibert_gait_pattern(np.zeros(3), 0.0, *bad)
    swing, dst, gain = 0.2, 0.05, 0.7
    vcmd, v = np.array([0.5, -0.2, 0.0]), np.array([0.3, 0.1, 9.0, 0, 0, 0])
    pl.set_raibert_gait_pattern(vcmd, 0.4, swing, dst, gain)
    pl.init(q, feet, com)
    assert pl.enable_double_support_phase and np.allclose(pl.R_yaw, fsr.yaw_matrix(0.4 * (swing + dst)), atol=1e-16)   # :79, :84
    assert pl.plan(0.1, q, feet, surfaces, v, 0b11, 2)
    period = 2.0 * (swing + dst)   # :75
    want = period * v[:2] + period * gain * (vcmd[:2] - v[:2])   # raibert_heuristic.cpp:50-55 on a one-sample average
    assert np.allclose(pl.step_length, [want[0], want[1], 0.0], atol=1e-16)
    # the first step of all with the heuristic: the CoM by half a step (:208-210), the right foot by half a step
    d = pl.step_length
    assert np.allclose(pl.com(2) - pl.com(1), 0.5 * (pl.R(2) @ d), atol=1e-15)
    assert np.allclose(pl.contact_positions(2)[1] - pl.contact_positions(1)[1], 0.5 * (pl.R(2) @ d), atol=1e-15)
    pl.set_raibert_gait_pattern(vcmd, 0.4, swing, 0.0, gain)
    assert not pl.enable_double_support_phase


# ---- what the runs and grids of the GPU tests are chosen for ----
def _branches(dsp):
    """the branches of plan() the run bc.SEQUENCE x bc.PLANNING_STEPS visits: (status, advanced) of the chain, and of the loop"""
    q, feet, surfaces, com = _pose()
    pl = _planner(q, feet, com, dsp=dsp)
    chain, loop = set(), set()
    for status in bc.SEQUENCE:
        for steps in bc.PLANNING_STEPS:
            before = pl.current_step
            assert pl.plan(0.0, q, feet, surfaces, np.zeros(6), status, steps)
            chain.add((status, pl.current_step != before))
            for step in range(pl.current_step, pl.current_step + steps + 1):
                if step == 0:
                    loop.add("zero")
                elif pl.current_step == 0 and step == 1:
                    loop.add("first")
                elif dsp:
                    loop.add({1: "right", 3: "left"}.get(step % 4, "nothing"))
                else:
                    loop.add("right" if step % 2 == 1 else "left")
    return chain, loop


def test_the_run_of_statuses_visits_every_branch():
    assert set(bc.SEQUENCE) == set(bwr.BipedWalkFootStepPlanner.STATUSES) and bc.PLANNING_STEPS == (0, 1, 10)
    for dsp in (False, True):
        chain, loop = _branches(dsp)
        # both single-support cases, each advancing (and turning) and holding
        assert {(0b01, True), (0b01, False), (0b10, True), (0b10, False)} <= chain, (dsp, chain)
        assert (0b11, False) in chain
        want = {"zero", "first", "right", "left"} | ({"nothing"} if dsp else set())
        assert loop == want, (dsp, loop)
    assert (0b11, True) in _branches(True)[0]   # double support: 0b11 on an odd current_step_ advances it


def test_the_grids_hold_what_the_tick_test_asserts():
    for dsp in (False, True):
        T = bc.WalkGrid(dsp)
        assert T.n <= 12 and len(T.phase_masks) == 4 and set(T.phase) == {0, 1, 2, 3}
        assert [g.dimf for g in T.grids if g.dimf] and all(g.dimf in (6, 12) for g in T.grids)
        swinging = {k for i in range(T.n) for k in range(2) if T.t[i] > T.start and not (T.phase_masks[T.phase[i]] >> k) & 1}
        assert swinging == {0, 1}   # both feet have an active swing entry
        assert any(T.t[i] <= T.start for i in range(T.n))   # and a grid point ahead of the swing
        # a grid point past the start whose mask the 0xF test of the quadrupeds would judge wrongly: both feet down is "all contacts"
        both_down = [i for i in range(T.n) if T.t[i] > T.start and T.phase_masks[T.phase[i]] == 0b11]
        assert bool(both_down) == dsp
        if dsp:
            assert T.phase_masks == [0b11, 0b01, 0b11, 0b10] and all((T.phase_masks[T.phase[i]] & 0xF) != 0xF for i in both_down)
            assert not any(bwr.has_inactive_contact(T.phase_masks[T.phase[i]]) for i in both_down)
        # every plan step the references read lies in the plan of the tick (planning_steps = 4: six steps)
        assert max(T.phase) + T.nph < 6 and max(T.phase) + 1 < 6


# ---- the host side of the feature ----
def _header():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rtoc_robot.h")) as f:
        return f.read()


def test_the_gait_value_matches_the_header():
    found = re.search(r"#define RTOC_GAIT_BIPED_WALK (\d+)", _header())
    assert found and int(found.group(1)) == capi.GAIT_BIPED_WALK == 4


class _Ctx:
    """a context that records what reaches it"""
    batch = 3

    def __init__(self):
        self.calls = []

    def set_foot_step_planner(self, planner):
        self.calls.append(("set", planner))

    def foot_step_plan(self, t, status, steps):
        self.calls.append(("plan", status, steps))


def test_the_python_class_checks_its_arguments_before_the_library():
    from robotoc_amd import planner as P
    cls = P.BipedWalkFootStepPlanner
    ctx = _Ctx()
    pl = cls(ctx)
    assert cls.GAIT == capi.GAIT_BIPED_WALK and cls.STATUSES == (0b11, 0b01, 0b10) == bwr.BipedWalkFootStepPlanner.STATUSES
    with pytest.raises(ValueError):
        pl.set_gait_pattern(np.zeros((2, 3)), 0.0, False)                   # neither [3] nor [batch, 3]
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.0, 0.1, 0.7)        # swing_time must be positive (:66)
    with pytest.raises(ValueError, match="double_support_time"):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, -0.1, 0.7)       # double_support_time non-negative (:69)
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.1, 0.0)        # gain positive (:72)
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), np.zeros(2), 0.2, 0.1, 0.7)   # yaw rates: a scalar or [batch]
    assert ctx.calls == []
    for status in range(0b100000):
        if status not in cls.STATUSES:
            assert pl.plan(0.0, status, 2) is False
    assert ctx.calls == []
    pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.0, 0.7)            # no double support: allowed
    pl.set_gait_pattern(np.ones((3, 3)), 0.1, True)
    one, many = ctx.calls[0][1], ctx.calls[1][1]
    assert isinstance(one, capi.FootStepPlanner) and one.gait == cls.GAIT and one.mode == capi.FOOT_STEP_RAIBERT and one.stance_time == 0.0
    assert len(many) == 3 and all(p.gait == cls.GAIT and p.mode == capi.FOOT_STEP_FIXED and p.enable_stance_phase == 1 for p in many)
    assert pl.plan(0.0, 0b10, 2) is True and ctx.calls[-1] == ("plan", 0b10, 2)
    # the accessors split the read-back the way the reference's do
    pl._plan = dict(positions=np.arange(3 * 4 * 6.0).reshape(3, 4, 2, 3), surfaces=np.arange(3 * 4 * 18.0).reshape(3, 4, 2, 3, 3))
    assert pl.contact_positions(1).shape == (3, 2, 3) and pl.contact_surfaces(1).shape == (3, 2, 3, 3)
    rot, trans = pl.contact_placements(2)
    assert np.array_equal(rot, pl.contact_surfaces(2)) and np.array_equal(trans, pl.contact_positions(2))
