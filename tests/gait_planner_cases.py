"""The problems of tests/test_gait_planner_*.py: the crawl, the pace and the flying trot on the ANYmal batch of
tests/foot_step_planner_cases.py (its states, commands and timing), the run of contact statuses that takes each gait's plan()
through every branch, and one small grid per gait made of that gait's own contact phases."""
import numpy as np

import foot_step_planner_cases as cases
import gait_planner_restatement as gpr
from robotoc_amd import capi
from robotoc_amd.grid import ContactSequence, Event, contact_masks, discretize
from robotoc_amd.types import anymal_dims

GAITS = ("crawl", "pace", "flying_trot")
GAIT_ID = {"trot": capi.GAIT_TROT, "crawl": capi.GAIT_CRAWL, "pace": capi.GAIT_PACE, "flying_trot": capi.GAIT_FLYING_TROT}
STANCE_TIME = 0.05   # what cases.planner_structs sets with a stance phase
# the ticks of the plan tests: every status of the gait, each both as an advance and as a repeat or a return
SEQUENCE = {
    "pace": (0b1111, 0b0011, 0b1100, 0b1111, 0b1100, 0b0011),
    "crawl": (0b1111, 0b0111, 0b1011, 0b1101, 0b1110, 0b0111, 0b1111, 0b1011),
    "flying_trot": (0b1111, 0b1001, 0b0000, 0b0110, 0b0000, 0b1001, 0b1111, 0b0110),
}
PLANNING_STEPS = (0, 1, 10)
# one grid per gait: its contact phases, what each event is, the contacts an impact adds
PHASES = {
    "pace": ([0b1111, 0b0011, 0b1111, 0b1100], ("lift", "impact", "lift")),
    "crawl": ([0b0111, 0b1011, 0b1101, 0b1110], ("impact", "impact", "impact")),
    "flying_trot": ([0b1001, 0b0000, 0b0110, 0b0000], ("lift", "impact", "lift")),
}
EVENT_TIMES = (0.03, 0.07, 0.09)


def has_stance_option(gait):
    return gait != "flying_trot"


def planner_structs(gait, raibert, stance, projection, insts=range(cases.BATCH)):
    """cases.planner_structs with the gait set; the flying trot's Raibert pattern needs a stance time"""
    out = cases.planner_structs(raibert, stance or (gait == "flying_trot" and raibert), projection, insts)
    for p in out:
        p.gait = GAIT_ID[gait]
        if gait == "flying_trot":
            p.enable_stance_phase = 0
    return out


def restated_planners(gait, raibert, stance, projection, insts=range(cases.BATCH)):
    out = []
    for b in insts:
        pl = gpr.PLANNERS[gait](yaw_projection=projection == capi.PROJECT_YAW)
        if gait == "flying_trot":
            if raibert:
                pl.set_raibert_gait_pattern(cases.VCOM_CMD[b], cases.YAW_RATE[b], cases.SWING_TIME, STANCE_TIME, cases.GAIN)
            else:
                pl.set_gait_pattern(cases.STEP_LENGTH[b], cases.STEP_YAW[b])
        elif raibert:
            pl.set_raibert_gait_pattern(cases.VCOM_CMD[b], cases.YAW_RATE[b], cases.SWING_TIME, STANCE_TIME if stance else 0.0, cases.GAIN)
        else:
            pl.set_gait_pattern(cases.STEP_LENGTH[b], cases.STEP_YAW[b], stance)
        out.append(pl)
    return out


def plan_size(gait, planning_steps):
    return planning_steps + (3 if gait == "flying_trot" else 2)


def _popcount(mask):
    return bin(mask).count("1")


class GaitGrid(cases.Trot):
    """cases.Trot for another gait: the grid of that gait's four contact phases, its phases and times, and the reference
    parameters (refs() is inherited)"""

    def __init__(self, gait):
        self.gait = gait
        self.phase_masks, kinds = PHASES[gait]
        events, impact_masks = [], []
        for k, (kind, time) in enumerate(zip(kinds, EVENT_TIMES)):
            added = self.phase_masks[k + 1] & ~self.phase_masks[k]
            events.append(Event(kind, time, impact_dimf=3 * _popcount(added) if kind == "impact" else 0))
            if kind == "impact":
                impact_masks.append(added)
        cs = ContactSequence([3 * _popcount(mk) for mk in self.phase_masks], events, phase_masks=list(self.phase_masks))
        N = 5 if gait == "crawl" else 6   # three impacts take six grid points
        self.grids, self.t, infos = discretize(N, 0.12, 0.0, cs, times=True, infos=True)
        self.t = np.array(self.t)
        self.phase = np.array([i[1] for i in infos], dtype=np.int32)
        self.n = len(self.grids)
        self.masks = contact_masks(self.grids, self.phase_masks, impact_masks)
        self.nph = 2
        # (the swing starts ahead of the second grid point, so that the first phase has a swinging foot too)
        self.start, self.period_swing, self.period_stance, self.height = 0.015, 0.04, 0.02, 0.08
        self.first_status = self.phase_masks[0]


def gait_context(T, m, x0, raibert=True, stance=False, projection=None, insts=None, shared_command=None):
    """cases.trot_context on the gait's grid with the gait's planner"""
    projection = capi.PROJECT_YAW if projection is None else projection
    insts = list(range(len(x0))) if insts is None else list(insts)
    ctx = capi.Context(anymal_dims(), T.n, len(insts), 0)
    ctx.set_grid(T.grids)
    ctx.set_robot_model(m)
    ctx.set_contact_schedule(T.masks)
    ctx.set_grid_times(T.t)
    ctx.set_task_costs(cases.task_terms(m))
    ctx.set_initial_state(x0[insts])
    if shared_command is not None:
        ctx.set_foot_step_planner(planner_structs(T.gait, raibert, stance, projection, [shared_command])[0])
    else:
        ctx.set_foot_step_planner(planner_structs(T.gait, raibert, stance, projection, insts))
    ctx.foot_step_planner_init()
    return ctx


def tick(ctx, T, t, status, steps=4):
    """what resetContactPlacements of the gait's MPC does: plan, place, refs"""
    ctx.foot_step_plan(t, status, steps)
    ctx.foot_step_place(T.phase)
    ctx.foot_step_refs(T.refs(), T.phase, T.phase_masks)
