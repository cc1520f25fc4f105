"""The yardstick of the foot-step planner tests held to what can be worked out by hand (tests/foot_step_planner_restatement.py),
and the host side of the new entry points: argument checks and refusal codes that are reached without a device."""
import ctypes as C

import numpy as np
import pytest

import foot_step_planner_restatement as fsr
from robotoc_amd import capi

Q = np.array([0.3, -0.2, 0.48, 0, 0, 0, 1.0] + [0.0] * 12)
FEET = np.array([[0.34, 0.19, 0.0], [-0.34, 0.19, 0.0], [0.34, -0.19, 0.0], [-0.34, -0.19, 0.0]]) + Q[:3] * [1, 1, 0]
COM = np.array([0.3, -0.2, 0.45])


def _planner(step_length, step_yaw=0.0, stance=False, q=Q):
    pl = fsr.TrotFootStepPlanner()
    pl.set_gait_pattern(step_length, step_yaw, stance)
    pl.init(q, FEET, COM)
    return pl


@pytest.mark.parametrize("stance", [False, True])
@pytest.mark.parametrize("status", [0b1111, 0b1001, 0b0110])
def test_zero_step_and_zero_yaw_keep_every_foothold(stance, status):
    pl = _planner(np.zeros(3), 0.0, stance)
    assert pl.plan(0.0, FEET, np.zeros(18), status, 6) and pl.size() == 8
    for s in range(1, 8):
        assert np.abs(pl.contact_positions(s) - pl.contact_positions(0)).max() < 1e-15
        assert np.abs(pl.com(s) - pl.com(0)).max() < 1e-15 and np.array_equal(pl.R(s), np.eye(3))


def test_straight_walking_without_stance():
    L = np.array([0.2, 0.0, 0.0])
    pl = _planner(L)
    assert pl.plan(0.0, FEET, np.zeros(18), 0b1111, 6)
    # the first step of all follows the 0.25 rule (:219-224) for a fixed pattern, every later one advances the CoM by half a step
    assert np.allclose(pl.com(1), pl.com(0), atol=1e-15)                     # step == 0: nothing moves
    assert np.allclose(pl.com(2) - pl.com(1), 0.25 * L, atol=1e-15)
    for s in range(3, 8):
        assert np.allclose(pl.com(s) - pl.com(s - 1), 0.5 * L, atol=1e-15)
    # feet 1, 2 step on odd steps, feet 0, 3 on even ones; a swing pair advances by the step length per two steps
    for pair, steps in (((1, 2), (4, 6)), ((0, 3), (5, 7))):
        for s in steps:
            for k in pair:
                assert np.allclose(pl.contact_positions(s)[k] - pl.contact_positions(s - 2)[k], L, atol=1e-15)
                assert np.array_equal(pl.contact_positions(s - 1)[k], pl.contact_positions(s - 2)[k])
    # with the heuristic the first step is a half step
    rb = fsr.TrotFootStepPlanner()
    rb.set_raibert_gait_pattern([0.4, 0.0, 0.0], 0.0, 0.25, 0.0, 1.0)
    rb.init(Q, FEET, COM)
    assert rb.plan(0.0, FEET, np.zeros(18), 0b1111, 2)
    assert np.allclose(rb.step_length, [0.5 * 0.4, 0.0, 0.0]) and np.allclose(rb.com(2) - rb.com(1), 0.5 * rb.step_length, atol=1e-15)


def test_current_step_follows_the_contact_status():
    pl = _planner(np.zeros(3))
    for status, want in ((0b1111, 0), (0b1001, 1), (0b1001, 1), (0b0110, 2), (0b1001, 3), (0b1111, 0)):
        assert pl.plan(0.0, FEET, np.zeros(18), status, 1) and pl.current_step == want
    assert not pl.plan(0.0, FEET, np.zeros(18), 0b0011, 1)
    ps = _planner(np.zeros(3), stance=True)
    for status, want in ((0b1111, 0), (0b1001, 1), (0b1111, 2), (0b0110, 3), (0b1111, 4), (0b1001, 5), (0b1001, 5)):
        assert ps.plan(0.0, FEET, np.zeros(18), status, 1) and ps.current_step == want


def test_yaw_composes_one_rotation_per_step():
    yaw = 0.3
    pl = _planner(np.array([0.1, 0.0, 0.0]), yaw)
    assert pl.plan(0.0, FEET, np.zeros(18), 0b1111, 5)
    Ry = fsr.yaw_matrix(yaw)
    assert np.array_equal(pl.R(0), np.eye(3)) and np.array_equal(pl.R(1), np.eye(3))
    for s in range(2, 7):
        assert np.allclose(pl.R(s), np.linalg.matrix_power(Ry, s - 1) @ pl.R(0), atol=1e-15)


def test_projection_is_the_reference_arithmetic_and_yaw_is_a_rotation():
    th = 0.2
    R = fsr.yaw_matrix(th)
    P = fsr.project_rotation_z(R)
    norm = np.cos(th) ** 2 - 2 * np.sin(th)
    assert abs(fsr.projection_norm(R) - norm) < 1e-15 and np.allclose(P[:2, :2], R[:2, :2] / norm, atol=1e-15) and P[2, 2] == 1.0
    assert abs(fsr.projection_norm(fsr.yaw_matrix(np.arcsin(np.sqrt(2.0) - 1.0)))) < 1e-15     # the zero crossing: sin(yaw) = sqrt(2) - 1, yaw = 0.427 rad
    tilt = fsr.rotation_from_quaternion(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]))
    Y = fsr.project_rotation_z(tilt, yaw_projection=True)
    assert np.allclose(Y @ Y.T, np.eye(3), atol=1e-15) and np.allclose(Y, fsr.yaw_matrix(np.arctan2(tilt[1, 0], tilt[0, 0])), atol=1e-15)


def test_the_seed_of_the_as_reference_plan_test_keeps_the_norm_away_from_zero():
    """tests/test_foot_step_planner_gpu.py runs RTOC_PROJECT_AS_REFERENCE on cases.states(3, True): |yaw| <= 0.2 rad"""
    import foot_step_planner_cases as cases
    _, x0 = cases.states(3, True)
    norms = [fsr.projection_norm(fsr.rotation_from_quaternion(x0[b, 3:7])) for b in range(cases.BATCH)]
    yaws = [np.arctan2(R[1, 0], R[0, 0]) for R in (fsr.rotation_from_quaternion(x0[b, 3:7]) for b in range(cases.BATCH))]
    assert min(norms) > 0.5 and max(abs(y) for y in yaws) <= 0.2 + 1e-12


def test_filter_drops_close_samples_and_forgets_old_ones():
    f = fsr.MovingWindowFilter()
    f.set_parameters(1.0, 0.1)
    seq = [(0.0, [1.0, 10.0]), (0.05, [100.0, 100.0]), (0.2, [3.0, 20.0]), (0.25, [100.0, 100.0]), (0.9, [5.0, 30.0]), (1.1, [7.0, 40.0]), (1.95, [9.0, 50.0])]
    want = [([1.0, 10.0], 1), ([1.0, 10.0], 1), ([2.0, 15.0], 2), ([2.0, 15.0], 2), ([3.0, 20.0], 3), ([5.0, 30.0], 3), ([8.0, 45.0], 2)]
    for (t, x), (avg, size) in zip(seq, want):
        f.push_back(t, x)
        assert np.allclose(f.average, avg, atol=1e-15) and f.size() == size, t
    f.clear()
    assert f.size() == 0 and np.array_equal(f.average, np.zeros(2))


def test_raibert_step_length():
    r = fsr.RaibertHeuristic()
    r.set_parameters(0.5, 0.7)
    r.plan_step_length([0.2, -0.1], [0.6, 0.3], 0.0)
    assert np.allclose(r.step_length, [0.5 * 0.2 + 0.35 * 0.4, 0.5 * -0.1 + 0.35 * 0.4, 0.0], atol=1e-16)
    with pytest.raises(ValueError):
        r.set_parameters(0.0, 0.7)


def test_swing_reference_by_hand():
    pos = np.zeros((4, 4, 3))
    pos[1, 2], pos[3, 2] = [1.0, 2.0, 0.1], [2.0, 4.0, 0.3]
    masks = [0b1111, 0b1011, 0b1111, 0b1111]
    args = dict(swing_height=0.08, swing_start_time=0.5, period_swing=0.2, period_stance=0.3, num_phases_in_period=2)
    assert fsr.swing_foot_ref(pos, 2, masks, 0.5, 1, **args)[1] is False           # t <= swing_start_time
    assert fsr.swing_foot_ref(pos, 2, masks, 0.6, 0, **args)[1] is False           # the foot is on the ground
    x, a = fsr.swing_foot_ref(pos, 2, masks, 0.6, 1, **args)                        # rate = 0.5: the apex above the midpoint
    assert a and np.allclose(x, [1.5, 3.0, 0.2 + 0.08], atol=1e-15)
    x, a = fsr.swing_foot_ref(pos, 2, masks, 1.15, 1, **args)                       # one cycle later, rate = 0.75
    assert a and np.allclose(x, [1.75, 3.5, 0.25 + 0.04], atol=1e-14)
    c, a = fsr.com_ref(pos[:, 2], masks, 0.6, 0, 0.5, 0.2, 0.3, 2)                  # a standing phase: the else branch
    assert not a and np.array_equal(c, pos[0, 2])


def test_eigen_quaternion_and_slerp():
    rng = np.random.default_rng(0)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        e = fsr.eigen_quaternion(fsr.rotation_from_quaternion(q))
        assert min(np.abs(e - q).max(), np.abs(e + q).max()) < 1e-14
    a, b = np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, np.sin(0.4), np.cos(0.4)])
    assert np.allclose(fsr.eigen_slerp(a, 0.25, b), [0, 0, np.sin(0.1), np.cos(0.1)], atol=1e-15)
    assert np.allclose(fsr.eigen_slerp(a, 0.25, -b), [0, 0, np.sin(0.1), np.cos(0.1)], atol=1e-15)    # the shorter arc
    assert np.allclose(fsr.eigen_slerp(a, 0.3, a), a, atol=1e-16)                                     # the near-parallel branch
    q_ref, act = fsr.configuration_ref(Q, np.array([fsr.yaw_matrix(0.0), fsr.yaw_matrix(0.8)]), [0b1001, 0b1111], 0.3, 0, 0.1, 0.4, 0.1, 1)
    assert act and np.allclose(q_ref[3:7], [0, 0, np.sin(0.2), np.cos(0.2)], atol=1e-15) and np.array_equal(np.delete(q_ref, range(3, 7)), np.delete(Q, range(3, 7)))


def test_the_library_exports_the_foot_step_entry_points_and_refuses_a_null_context():
    L = capi.lib()
    names = ("rtoc_set_foot_step_planner", "rtoc_foot_step_planner_init", "rtoc_foot_step_plan", "rtoc_foot_step_plan_get", "rtoc_foot_step_place",
             "rtoc_foot_step_refs", "rtoc_get_task_ref_table", "rtoc_get_configuration_ref_table")
    for name in names:
        assert name in capi.EXPORTS and hasattr(L, name)
    BAD = -1
    p, r = capi.FootStepPlanner(), capi.FootStepRefs()
    ph = (C.c_int * 2)(0, 0)
    mk = (C.c_uint * 1)(15)
    assert L.rtoc_set_foot_step_planner(None, C.byref(p), 0) == BAD
    assert L.rtoc_foot_step_planner_init(None) == BAD
    assert L.rtoc_foot_step_plan(None, 0.0, 15, 1) == BAD
    assert L.rtoc_foot_step_plan_get(None, None, None, None, None, None, 0, None, None) == BAD
    assert L.rtoc_foot_step_place(None, ph, 2) == BAD
    assert L.rtoc_foot_step_refs(None, C.byref(r), ph, mk, 1, 2) == BAD
    assert L.rtoc_get_task_ref_table(None, 0, None, 0, None) == BAD
    assert L.rtoc_get_configuration_ref_table(None, None, None, 0, None) == BAD
    assert capi.MAX_PLAN_STEPS == 32
    # the structs have the header's layout: sizes as a C compiler lays them out
    assert C.sizeof(capi.FootStepPlanner) == 16 + 8 * 11 and C.sizeof(capi.FootStepRefs) == 24 + 8 * 16 + 16 + 2 * (24 + 8)


def test_the_python_planner_checks_its_arguments_before_the_library():
    from robotoc_amd.planner import TrotFootStepPlanner

    class Ctx:
        batch = 3

    pl = TrotFootStepPlanner(Ctx())
    with pytest.raises(ValueError):
        pl.set_gait_pattern(np.zeros((2, 3)), 0.0, False)              # neither [3] nor [batch, 3]
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.0, 0.1, 0.7)    # swing_time must be positive
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, -0.1, 0.7)
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), 0.0, 0.2, 0.1, 0.0)
    with pytest.raises(ValueError):
        pl.set_raibert_gait_pattern(np.zeros(3), np.zeros(2), 0.2, 0.1, 0.7)   # yaw rates: a scalar or [batch]
