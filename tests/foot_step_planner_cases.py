"""The problems of tests/test_foot_step_planner_gpu.py: ANYmal, five instances (one whole group of four per wave quarter and a
partial one), each with its own base placement, velocity and command -- signs and magnitudes differ, instance 2 has an all-zero
command.  Plan tests run on a plain 8-point grid (the plan does not depend on the grid); place / refs tests on a trot grid of 11
points and 4 contact phases: stand, LH + RF swing from 0.03 s, stand from 0.07 s, LF + RH swing from 0.09 s."""
import numpy as np

import foot_step_planner_restatement as fsr
from robotoc_amd import capi, robot_model as rm
from robotoc_amd.grid import ContactSequence, Event, contact_masks, discretize, uniform_grid
from robotoc_amd.types import anymal_dims
from task_cost_restatement import com as com_restated

Q_ANYMAL = np.array([0, 0, 0.4792, 0, 0, 0, 1, -0.1, 0.7, -1.0, -0.1, -0.7, 1.0, 0.1, 0.7, -1.0, 0.1, -0.7, 1.0])
BATCH = 5
STEP_LENGTH = np.array([[0.15, 0.0, 0.0], [-0.1, 0.05, 0.0], [0.0, 0.0, 0.0], [0.3, -0.12, 0.01], [0.02, 0.2, 0.0]])
STEP_YAW = np.array([0.1, -0.25, 0.0, 0.05, 0.4])
VCOM_CMD = np.array([[0.5, 0.0, 0.0], [-0.3, 0.2, 0.0], [0.0, 0.0, 0.0], [1.2, -0.4, 0.0], [0.05, 0.6, 0.0]])
YAW_RATE = np.array([0.3, -0.8, 0.0, 0.1, 1.5])
SWING_TIME, GAIN = 0.2, 0.7
PHASE_MASKS = [0b1111, 0b1001, 0b1111, 0b0110]


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def states(seed, small_yaw):
    """x0 [BATCH, nq + nv]: random base placements and joint angles around standing; small_yaw: |yaw| <= 0.2 rad and roll, pitch
    within 0.3 rad (RTOC_PROJECT_AS_REFERENCE: the reference's `norm` must stay away from zero), else any unit quaternion"""
    m = rm.load_named("anymal")
    rng = np.random.default_rng(seed)
    x0 = np.zeros((BATCH, m.nq + m.nv))
    for b in range(BATCH):
        q = Q_ANYMAL.copy()
        q[:2] = rng.uniform(-2, 2, 2)
        q[2] += rng.uniform(-0.05, 0.05)
        q[7:] += 0.2 * rng.uniform(-1, 1, 12)
        if small_yaw:
            R = _rot(2, rng.uniform(-0.2, 0.2)) @ _rot(1, rng.uniform(-0.3, 0.3)) @ _rot(0, rng.uniform(-0.3, 0.3))
            q[3:7] = fsr.eigen_quaternion(R)
        else:
            quat = rng.normal(size=4)
            q[3:7] = quat / np.linalg.norm(quat)
        x0[b, :m.nq] = q
        x0[b, m.nq:] = 0.5 * rng.uniform(-1, 1, m.nv)
    return m, x0


def kinematics(oracle, m, x0):
    feet = np.array([[oracle.rbd_contact_placement(m, x0[b, :m.nq], c)[1] for c in range(4)] for b in range(len(x0))])
    com = np.array([com_restated(m, x0[b, :m.nq]) for b in range(len(x0))])
    return feet, com


def planner_structs(raibert, stance, projection, insts=range(BATCH)):
    out = []
    for b in insts:
        p = capi.FootStepPlanner()
        p.mode, p.projection = (capi.FOOT_STEP_RAIBERT if raibert else capi.FOOT_STEP_FIXED), projection
        p.enable_stance_phase = int(stance)
        p.swing_time, p.stance_time, p.gain = SWING_TIME, (0.05 if stance else 0.0), GAIN
        p.step_length[:], p.step_yaw = list(STEP_LENGTH[b]), float(STEP_YAW[b])
        p.vcom_cmd[:], p.yaw_rate_cmd = list(VCOM_CMD[b]), float(YAW_RATE[b])
        out.append(p)
    return out


def restated_planners(raibert, stance, projection, insts=range(BATCH)):
    out = []
    for b in insts:
        pl = fsr.TrotFootStepPlanner(yaw_projection=projection == capi.PROJECT_YAW)
        if raibert:
            pl.set_raibert_gait_pattern(VCOM_CMD[b], YAW_RATE[b], SWING_TIME, 0.05 if stance else 0.0, GAIN)
        else:
            pl.set_gait_pattern(STEP_LENGTH[b], STEP_YAW[b], stance)
        out.append(pl)
    return out


def plain_context(m, x0):
    ctx = capi.Context(anymal_dims(), 8, len(x0), 0)
    ctx.set_grid(uniform_grid(7, 0.02, dimf=12))
    ctx.set_robot_model(m)
    ctx.set_initial_state(x0)
    return ctx


class Trot:
    """the trot grid, its phases and times, and the reference parameters of the refs tests"""

    def __init__(self):
        cs = ContactSequence([12, 6, 12, 6], [Event("lift", 0.03), Event("impact", 0.07, impact_dimf=6), Event("lift", 0.09)])
        self.grids, self.t, infos = discretize(6, 0.12, 0.0, cs, times=True, infos=True)
        self.t = np.array(self.t)
        self.phase = np.array([i[1] for i in infos], dtype=np.int32)
        self.n = len(self.grids)
        self.masks = contact_masks(self.grids, PHASE_MASKS, [0b0110])
        self.nph = 2
        self.start, self.period_swing, self.period_stance, self.height = 0.025, 0.04, 0.02, 0.08

    def refs(self, foot_terms=(0, 1, 2, 3), com_term=4, configuration=True):
        r = capi.FootStepRefs()
        r.foot_term[:] = foot_terms
        r.com_term, r.configuration = com_term, int(configuration)
        for k in range(4):
            r.swing_height[k], r.swing_start_time[k] = self.height, self.start
            r.period_swing[k], r.period_stance[k], r.swing_num_phases_in_period[k] = self.period_swing, self.period_stance, self.nph
        r.com_swing_start_time, r.com_period_active, r.com_period_inactive, r.com_num_phases_in_period = self.start, self.period_swing, self.period_stance, self.nph
        r.q_swing_start_time, r.q_period_active, r.q_period_inactive, r.q_num_phases_in_period = self.start, self.period_swing, self.period_stance, self.nph
        return r


def task_terms(m):
    """four TaskSpace3DCost terms on the feet and a CoMCost term, every one with a table reference"""
    from robotoc_amd.costs import TaskCost
    out = []
    for k in range(5):
        t = TaskCost()
        t.kind, t.ref_kind = (0 if k < 4 else 1), 3   # RTOC_TASK_FRAME_3D | RTOC_TASK_COM, RTOC_REF_TABLE
        if k < 4:
            t.frame_parent = m.contact_parent[k]
            t.frame_p[:] = list(m.contact_p[k])
        w = 1.0e3 if k < 4 else 1.0e2
        t.weight[:], t.weight_terminal[:], t.weight_impact[:] = [w] * 3, [w] * 3, [w] * 3
        out.append(t)
    return out


def trot_context(T, m, x0, raibert=True, stance=False, projection=None, insts=None, shared_command=None):
    """a context on the trot grid with the schedule, the grid times, the five terms and a planner set and initialised"""
    projection = capi.PROJECT_YAW if projection is None else projection
    insts = list(range(len(x0))) if insts is None else list(insts)
    ctx = capi.Context(anymal_dims(), T.n, len(insts), 0)
    ctx.set_grid(T.grids)
    ctx.set_robot_model(m)
    ctx.set_contact_schedule(T.masks)
    ctx.set_grid_times(T.t)
    ctx.set_task_costs(task_terms(m))
    ctx.set_initial_state(x0[insts])
    if shared_command is not None:
        ctx.set_foot_step_planner(planner_structs(raibert, stance, projection, [shared_command])[0])
    else:
        ctx.set_foot_step_planner(planner_structs(raibert, stance, projection, insts))
    ctx.foot_step_planner_init()
    return ctx


def tick(ctx, T, t, status=0b1111, steps=4):
    """what MPCTrot::resetContactPlacements does: plan, place, refs"""
    ctx.foot_step_plan(t, status, steps)
    ctx.foot_step_place(T.phase)
    ctx.foot_step_refs(T.refs(), T.phase, PHASE_MASKS)


def tables(ctx):
    """every table a tick fills, as arrays"""
    out = dict(placements=ctx.contact_placements()[0])
    for k in range(5):
        R, p, act, inst = ctx.task_ref_table(k)
        assert inst is True
        out["ref%d_R" % k], out["ref%d_p" % k], out["ref%d_active" % k] = R, p, act
    q, act, inst = ctx.configuration_ref_table()
    assert inst is True
    out["q_ref"], out["q_active"] = q, act
    return out


def plan_arrays(ctx):
    g = ctx.foot_step_plan_get()
    return {k: np.asarray(v) for k, v in g.items()}
