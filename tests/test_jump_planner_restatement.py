"""tests/jump_planner_restatement.py held to facts derived by hand from src/mpc/jump_foot_step_planner.cpp and
src/mpc/mpc_jump.cpp:141-145, and the run of contact statuses and the grid of tests/test_jump_planner_gpu.py held to what they are
chosen for.

The robot of these tests is one rigid body: feet, soles and centre of mass are fixed in the base frame, so the kinematics at any q
-- at q_goal too -- are a rotation and a translation written out below."""
import numpy as np
import pytest

import foot_step_planner_restatement as fsr
import jump_planner_cases as jc
import jump_planner_restatement as jr

BASE = np.array([1.0, -2.0, 0.5])
COM_LOCAL = np.array([0.02, -0.01, -0.1])
FEET_LOCAL = {False: np.array([[0.3, 0.2, -0.5], [-0.3, 0.2, -0.5], [0.3, -0.2, -0.5], [-0.3, -0.2, -0.5]]),
              True: np.array([[0.0, 0.07, -0.6], [0.0, -0.07, -0.6]])}
ULP = 2.3e-16


def _pitch(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _kinematics(biped, q):
    """(feet, soles, com) of the rigid robot at q; the soles are pitched in the base frame, one each way"""
    Rq = fsr.rotation_from_quaternion(q[3:7])
    local = FEET_LOCAL[biped]
    soles = [_pitch(0.2 if k % 2 == 0 else -0.15) for k in range(len(local))]
    return np.array([q[:3] + Rq @ p for p in local]), np.array([Rq @ S for S in soles]), q[:3] + Rq @ COM_LOCAL


def _quat_yaw(yaw):
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw)])


def _planner(biped, q, jump_length=(0, 0, 0), yaw=0.0, yaw_projection=True):
    pl = jr.JumpFootStepPlanner(biped, yaw_projection=yaw_projection)
    pl.set_jump_pattern(jump_length, yaw)
    feet, soles, com = _kinematics(biped, q)
    pl.init(q, feet, soles, com, _kinematics(biped, pl.goal_configuration(q))[2])
    return pl


@pytest.mark.parametrize("biped", (False, True))
def test_zero_jump_and_zero_yaw_go_nowhere(biped):
    q = np.concatenate([BASE, [0.0, 0.0, 0.0, 1.0], [0.3, -0.2]])
    pl = _planner(biped, q)
    assert pl.size() == 3 and pl.current_step == 0
    for field in (pl.contact_positions, pl.contact_surfaces, pl.com, pl.R):
        assert np.array_equal(field(2), field(0)) and np.array_equal(field(1), field(0))
    assert np.array_equal(pl.q_ref(q), q)
    # a yawed base: the same up to the rounding of quaternion -> matrix -> quaternion
    q = np.concatenate([BASE, _quat_yaw(0.7), [0.3, -0.2]])
    pl = _planner(biped, q)
    assert np.abs(pl.contact_positions(2) - pl.contact_positions(0)).max() < 8 * ULP * 2.0
    assert np.abs(pl.q_ref(q) - q).max() < 8 * ULP * 2.0


@pytest.mark.parametrize("biped", (False, True))
def test_level_base_and_zero_yaw_translate_everything(biped):
    jump = np.array([0.6, -0.25, 0.05])
    q = np.concatenate([BASE, [0.0, 0.0, 0.0, 1.0], [0.1]])
    pl = _planner(biped, q, jump)
    feet = _kinematics(biped, q)[0]
    assert np.array_equal(pl.contact_positions(0), feet) and np.array_equal(pl.contact_positions(1), feet)
    assert np.abs(pl.contact_positions(2) - (feet + jump)).max() < 4 * ULP * 2.5
    assert np.abs((pl.com(2) - pl.com(0)) - jump).max() < 4 * ULP * 2.5
    assert np.abs(pl.q_ref(q)[:3] - (BASE + jump)).max() < 4 * ULP * 2.5 and np.array_equal(pl.q_ref(q)[3:], q[3:])


@pytest.mark.parametrize("biped", (False, True))
def test_a_quarter_turn_about_the_vertical_through_the_base(biped):
    jump, yaw0 = np.array([0.4, 0.1, 0.0]), 0.3
    q = np.concatenate([BASE, _quat_yaw(yaw0)])
    pl = _planner(biped, q, jump, 0.5 * np.pi)
    feet, soles, com = _kinematics(biped, q)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    hop = Rz @ jump
    tol = 16 * ULP * 2.5
    assert np.abs(pl.contact_positions(2) - (BASE + (feet - BASE) @ Rz.T + hop)).max() < tol
    assert np.abs(pl.com(2) - (BASE + Rz @ (com - BASE) + hop)).max() < tol
    R2 = pl.R(2)
    assert np.abs(R2 @ R2.T - np.eye(3)).max() < 8 * ULP and abs(np.linalg.det(R2) - 1.0) < 8 * ULP
    assert np.abs(R2 - fsr.yaw_matrix(yaw0 + 0.5 * np.pi)).max() < 8 * ULP
    q_ref = pl.q_ref(q)
    assert abs(np.linalg.norm(q_ref[3:7]) - 1.0) < 8 * ULP
    assert np.abs(q_ref[:3] - (q[:3] + (pl.com(2) - pl.com(0)))).max() == 0.0


def test_quadruped_rotations_are_identities_and_biped_goals_turn_with_the_base():
    q = np.concatenate([BASE, _quat_yaw(-0.4)])
    quad = _planner(False, q, (0.3, 0.0, 0.0), 0.6)
    for s in range(3):
        assert np.array_equal(quad.contact_surfaces(s), np.broadcast_to(np.eye(3), (4, 3, 3)))
    biped = _planner(True, q, (0.3, 0.0, 0.0), 0.6)
    _, soles, _ = _kinematics(True, q)
    assert np.array_equal(biped.contact_surfaces(0), soles) and np.array_equal(biped.contact_surfaces(1), soles)
    R, R_goal = biped.R(0), biped.R(2)
    for k in range(2):
        assert np.abs(biped.contact_surfaces(2)[k] - R_goal @ R.T @ soles[k]).max() < 8 * ULP
    assert not np.allclose(biped.contact_surfaces(2), soles, atol=1e-3)


@pytest.mark.parametrize("biped", (False, True))
def test_the_status_run_of_the_gpu_tests(biped):
    full = 0b11 if biped else 0b1111
    q = np.concatenate([BASE, _quat_yaw(0.2)])
    pl = _planner(biped, q, (0.5, 0.1, 0.0), 0.3)
    goal = [f(2).copy() for f in (pl.contact_positions, pl.contact_surfaces, pl.com, pl.R)]
    seen_steps, seen_sizes = [], []
    for tick, status in enumerate(jc.SEQUENCE):
        status = full if status == "full" else status
        qt = q.copy()
        qt[:3] += 0.01 * (tick + 1)   # the state changes between the ticks
        qt[3:7] = _quat_yaw(0.2 + 0.05 * tick)
        feet, soles, _ = _kinematics(biped, qt)
        before = [f(1).copy() for f in (pl.contact_positions, pl.contact_surfaces, pl.com, pl.R)]
        assert pl.plan(feet, soles, status)
        seen_steps.append(pl.current_step), seen_sizes.append(pl.size())
        if status:
            # steps 0 and 1 after a tick on the ground are that tick's kinematics; CoM and R are not touched
            for s in (0, 1):
                assert np.array_equal(pl.contact_positions(s), feet)
                assert np.array_equal(pl.contact_surfaces(s), soles if biped else np.broadcast_to(np.eye(3), (4, 3, 3)))
            assert np.array_equal(pl.com(1), before[2]) and np.array_equal(pl.R(1), before[3])
            if pl.size() == 3:
                assert all(np.array_equal(f(2), g) for f, g in zip((pl.contact_positions, pl.contact_surfaces, pl.com, pl.R), goal))
        elif tick == 2:
            # the first tick of the flight: step 1 is the former step 2
            assert all(np.array_equal(f(1), g) for f, g in zip((pl.contact_positions, pl.contact_surfaces, pl.com, pl.R), goal))
        else:
            assert all(np.array_equal(f(1), g) for f, g in zip((pl.contact_positions, pl.contact_surfaces, pl.com, pl.R), before))
    assert tuple(seen_steps) == jc.CURRENT_STEPS == (0, 0, 1, 1, 2, 2, 2) and tuple(seen_sizes) == jc.SIZES == (3, 3, 2, 2, 2, 2, 2)


@pytest.mark.parametrize("biped", (False, True))
def test_the_projections_coincide_on_the_identity_orientation(biped):
    q = np.concatenate([BASE, [0.0, 0.0, 0.0, 1.0]])
    a = _planner(biped, q, (0.5, 0.1, 0.02), 0.4, yaw_projection=True)
    b = _planner(biped, q, (0.5, 0.1, 0.02), 0.4, yaw_projection=False)
    for s in range(3):
        for f, g in ((a.contact_positions, b.contact_positions), (a.contact_surfaces, b.contact_surfaces), (a.com, b.com), (a.R, b.R)):
            assert np.array_equal(f(s), g(s))
    assert np.array_equal(a.q_ref(q), b.q_ref(q))


def test_a_second_init_starts_over():
    q = np.concatenate([BASE, _quat_yaw(0.1)])
    pl = _planner(False, q, (0.5, 0.0, 0.0), 0.2)
    feet, soles, _ = _kinematics(False, q)
    pl.plan(feet, soles, 0)
    assert pl.size() == 2 and pl.current_step == 1
    q2 = q.copy()
    q2[:3] += 1.0
    feet, soles, com = _kinematics(False, q2)
    pl.init(q2, feet, soles, com, _kinematics(False, pl.goal_configuration(q2))[2])
    assert pl.size() == 3 and pl.current_step == 0 and np.array_equal(pl.com(0), com)   # (the reference would answer with the first init's)


def test_which_step_serves_which_phase():
    assert jr.placement_steps(0, 3) == [1, 2, 2] and jr.placement_steps(1, 2) == [1, 1] and jr.placement_steps(2, 1) == [1]
    for size, cur in ((3, 0), (2, 1)):   # what the caller passes to rtoc_foot_step_place: min(phase, size - 2), + 1 inside
        nph = 3 if cur == 0 else 2
        assert [min(ph, size - 2) + 1 for ph in range(nph)] == jr.placement_steps(cur, nph)


@pytest.mark.parametrize("model", ("anymal", "icub32"))
def test_the_grid_of_the_gpu_tests(model):
    T = jc.JumpGrid(model)
    assert 8 <= T.n <= 12
    assert sorted(set(T.phase.tolist())) == [0, 1, 2] and T.phase[0] == 0 and T.phase[-1] == 2
    from robotoc_amd.types import GRID_IMPACT, GRID_LIFT
    assert sum(g.type == GRID_LIFT for g in T.grids) == 1 and sum(g.type == GRID_IMPACT for g in T.grids) == 1
    assert any(int(mk) == 0 for mk in T.masks) and int(T.masks[0]) == T.full
    # distinct commands; one instance stands still
    cmds = [jc.command(b) for b in range(5)]
    assert len({(tuple(j), y) for j, y in cmds}) == 5 and not cmds[2][0].any() and cmds[2][1] == 0.0
