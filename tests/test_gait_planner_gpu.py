"""The crawl, the pace and the flying trot through foot_step_plan_kernel (foot_step_planner.hpp, rt_foot_steps.hip) against the numpy
restatement of the reference's three planners (tests/gait_planner_restatement.py), their plans through the place and refs kernels,
and the project's usual isolation checks -- a batch against batch-1 contexts, shared against repeated commands, a clone -- bit for
bit.

Tolerances are those of tests/test_foot_step_planner_gpu.py, for the reason given there: every step composes one more rotation onto
R and adds one more scaled offset to the centre of mass and the feet (the crawl adds it to the foot itself, the other gaits to the
centre of mass first), so positions and CoM are held to 1e-14 x size x max(1, max|p|), rotations to 1e-14 x size, the Raibert step
length to 1e-14 x max(1, |step_length|).  The references are compared with the restatement evaluated ON THE PLAN READ BACK:
positions to 4e-16 x 4 x max(1, max|p|), quaternions to 1e-14, active flags exactly.

tests/test_gait_planner_restatement.py holds the runs of contact statuses and the grids used here to what they are chosen for."""
import numpy as np
import pytest

import foot_step_planner_cases as cases
import foot_step_planner_restatement as fsr
import gait_planner_cases as gc
from helpers import check_parity
from robotoc_amd import capi
from robotoc_amd.capi import RtocError


def _compare_plan(label, got, planners, n):
    assert got["size"] == n and got["ok"].all()
    assert all(got["current_step"] == pl.current_step and pl.size() == n for pl in planners)
    want_p = np.array([[pl.contact_positions(s) for s in range(n)] for pl in planners])
    want_c = np.array([[pl.com(s) for s in range(n)] for pl in planners])
    want_R = np.array([[pl.R(s) for s in range(n)] for pl in planners])
    scale = max(1.0, np.abs(want_p).max())
    check_parity(label + ": contact positions", np.abs(got["positions"] - want_p).max() / scale, 1e-14 * n)
    check_parity(label + ": CoM", np.abs(got["com"] - want_c).max() / scale, 1e-14 * n)
    check_parity(label + ": R", np.abs(got["R"] - want_R).max(), 1e-14 * n)


def _plan_cases():
    out = []
    for gait in gc.GAITS:
        for raibert in (False, True):
            for stance in ((False, True) if gc.has_stance_option(gait) else (False,)):
                out.append((gait, raibert, stance, capi.PROJECT_YAW))
        out.append((gait, True, False, capi.PROJECT_AS_REFERENCE))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("gait,raibert,stance,projection", _plan_cases())
def test_plan_against_the_restatement(oracle, gait, raibert, stance, projection):
    """a) per gait both modes and both stance settings (the flying trot has one); a run of ticks over every status of the gait with
    planning_steps 0, 1 and 10; a second init starts over"""
    small = projection == capi.PROJECT_AS_REFERENCE
    m, x0 = cases.states(3 if small else 4, small)
    feet, com = cases.kinematics(oracle, m, x0)
    ctx = cases.plain_context(m, x0)
    ctx.set_foot_step_planner(gc.planner_structs(gait, raibert, stance, projection))
    planners = gc.restated_planners(gait, raibert, stance, projection)
    seq = gc.SEQUENCE[gait]
    for again in range(2):   # a second init starts over: current_step_ = 0, the filter cleared
        ctx.foot_step_planner_init()
        assert ctx.foot_step_plan_get()["size"] == 0
        for b, pl in enumerate(planners):
            pl.init(x0[b, :m.nq], feet[b], com[b])
        t = 0.0
        for status in (seq if again == 0 else seq[:3]):
            for steps in gc.PLANNING_STEPS:
                t += 0.07
                ctx.foot_step_plan(t, status, steps)
                for b, pl in enumerate(planners):
                    assert pl.plan(t, feet[b], x0[b, m.nq:], status, steps)
                got = ctx.foot_step_plan_get()
                label = "%s raibert %d stance %d projection %d status %s steps %d" % (gait, raibert, stance, projection, bin(status), steps)
                _compare_plan(label, got, planners, gc.plan_size(gait, steps))
                want_sl = np.array([pl.step_length for pl in planners])
                check_parity(label + ": step length in force", np.abs(got["step_length"] - want_sl).max() / max(1.0, np.abs(want_sl).max()), 1e-14)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gait", gc.GAITS)
def test_one_tick_on_the_gaits_own_phases(gait):
    """b) plan, place, refs on a grid of the gait's own contact phases: the placement table is contactPositions(phase + 1) bit for
    bit, the three references are the restatement's on the plan read back"""
    T = gc.GaitGrid(gait)
    m, x0 = cases.states(6, False)
    ctx = gc.gait_context(T, m, x0)
    gc.tick(ctx, T, 0.0, T.first_status)
    plan, tab = cases.plan_arrays(ctx), cases.tables(ctx)
    ctx.close()
    assert T.n <= 12 and plan["size"] == gc.plan_size(gait, 4) and plan["ok"].all()
    for i in range(T.n):
        assert np.array_equal(tab["placements"][:, i], plan["positions"][:, T.phase[i] + 1])
    assert not np.array_equal(tab["placements"][0], tab["placements"][1])
    par = (T.start, T.period_swing, T.period_stance, T.nph)
    scale = max(1.0, np.abs(plan["positions"]).max())
    swing_feet, flight_points = set(), 0
    for b in range(cases.BATCH):
        for i in range(T.n):
            for k in range(4):
                x, a = fsr.swing_foot_ref(plan["positions"][b], k, T.phase_masks, T.t[i], T.phase[i], T.height, *par)
                assert tab["ref%d_active" % k][b, i] == a
                if a:
                    swing_feet.add(k)
                check_parity(gait + ": swing foot reference", np.abs(tab["ref%d_p" % k][b, i] - x).max() / scale, 4e-16 * 4)
                assert np.array_equal(tab["ref%d_R" % k][b, i], np.eye(3))
            x, a = fsr.com_ref(plan["com"][b], T.phase_masks, T.t[i], T.phase[i], *par)
            assert tab["ref4_active"][b, i] == a
            check_parity(gait + ": CoM reference", np.abs(tab["ref4_p"][b, i] - x).max() / scale, 4e-16 * 4)
            q, a = fsr.configuration_ref(x0[b, :m.nq], plan["R"][b], T.phase_masks, T.t[i], T.phase[i], *par)
            assert tab["q_active"][b, i] == a
            check_parity(gait + ": configuration reference: quaternion", np.abs(tab["q_ref"][b, i, 3:7] - q[3:7]).max(), 1e-14)
            assert np.array_equal(np.delete(tab["q_ref"][b, i], range(3, 7)), np.delete(q, range(3, 7)))
            flight_points += b == 0 and T.phase_masks[T.phase[i]] == 0 and T.t[i] > T.start
    # the grid contains what it was chosen for: an active swing entry for a foot, and the flying trot a grid point in flight
    assert swing_feet
    if gait == "flying_trot":
        assert flight_points > 0 and swing_feet == {0, 1, 2, 3}
    if gait == "crawl":
        assert swing_feet == {0, 1, 2, 3}   # the four three-foot phases


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def _plan_tables(ctx):
    p = cases.plan_arrays(ctx)
    t = cases.tables(ctx)
    t.update({"plan_" + k: v for k, v in p.items()})
    return t


# c) and d): the first two ticks (the second one a flight for the flying trot) and a third
TICKS = {"pace": (0b1111, 0b0011, 0b1100), "crawl": (0b0111, 0b1011, 0b1101), "flying_trot": (0b1001, 0b0000, 0b0110)}


@pytest.mark.gpu
@pytest.mark.parametrize("gait", gc.GAITS)
def test_isolation_shared_commands_and_clone(gait):
    """c) across two consecutive ticks: instance b of the batch = a batch-1 context with b's inputs and command; one shared command =
    five copies of it; a clone after the first tick, then the second tick on both (the flying trot: a flight, which reads step 0 of
    the plan the clone carried over)"""
    T = gc.GaitGrid(gait)
    m, x0 = cases.states(6, False)
    x1 = x0.copy()
    x1[:, m.nq:] *= -0.7
    first, second, _ = TICKS[gait]

    def two_ticks(ctx, insts, fork=False):
        out, twin = [], None
        for t, x, status in ((0.0, x0, first), (0.12, x1, second)):
            ctx.set_initial_state(x[insts])
            if twin is not None:
                twin.set_initial_state(x[insts])
                gc.tick(twin, T, t, status)
            gc.tick(ctx, T, t, status)
            out.append(_plan_tables(ctx))
            if fork and twin is None:
                twin = ctx.clone()
        return out, twin

    big = gc.gait_context(T, m, x0)
    want, twin = two_ticks(big, list(range(cases.BATCH)), fork=True)
    assert _equal(_plan_tables(twin), want[1]) and not _equal(want[0], want[1])
    twin.close()
    big.close()
    for b in range(cases.BATCH):
        one = gc.gait_context(T, m, x0, insts=[b])
        got, _ = two_ticks(one, [b])
        for w, g in zip(want, got):
            for k in w:
                if k in ("plan_size", "plan_current_step"):
                    assert w[k] == g[k]
                else:
                    assert np.array_equal(w[k][b], g[k][0]), (gait, b, k)
        one.close()
    # per_instance = 0 with one command = per_instance = 1 with five copies of it
    a = gc.gait_context(T, m, x0, shared_command=3)
    bctx = gc.gait_context(T, m, x0)
    bctx.set_foot_step_planner(gc.planner_structs(gait, True, False, capi.PROJECT_YAW, [3] * cases.BATCH))
    every = list(range(cases.BATCH))
    for w, g in zip(two_ticks(a, every)[0], two_ticks(bctx, every)[0]):
        assert _equal(w, g)
    a.close()
    bctx.close()


def _rc(fn, *a):
    try:
        fn(*a)
    except RtocError as e:
        return e.code
    return 0


@pytest.mark.gpu
def test_refusals_launch_nothing():
    """d) an unknown gait, gaits that differ across the batch, each gait's illegal statuses (another gait's legal ones among them), a
    flight as the first plan, planning_steps = RTOC_MAX_PLAN_STEPS and stance_time = 0 for the flying trot; a refused call leaves the
    plan, the tables and current_step as they were"""
    BAD = capi.ERR_BAD_ARG
    m, x0 = cases.states(6, False)
    legal = {"trot": (0b1111, 0b1001, 0b0110), "pace": gc.SEQUENCE["pace"], "crawl": gc.SEQUENCE["crawl"], "flying_trot": gc.SEQUENCE["flying_trot"]}
    for gait in gc.GAITS:
        T = gc.GaitGrid(gait)
        ctx = gc.gait_context(T, m, x0)
        good = gc.planner_structs(gait, True, False, capi.PROJECT_YAW)
        for value in (4, -1, 17):
            bad = gc.planner_structs(gait, True, False, capi.PROJECT_YAW)
            for p in bad:
                p.gait = value
            assert _rc(ctx.set_foot_step_planner, bad) == BAD and _rc(ctx.set_foot_step_planner, bad[0]) == BAD
        for other in ("trot",) + gc.GAITS:
            if other != gait:
                bad = gc.planner_structs(gait, True, gait == "flying_trot", capi.PROJECT_YAW)
                bad[3].gait = gc.GAIT_ID[other]   # structure must agree across the batch
                assert _rc(ctx.set_foot_step_planner, bad) == BAD, (gait, other)
        if gait == "flying_trot":
            assert _rc(ctx.foot_step_plan, 0.0, 0b0000, 4) == BAD          # a flight with no plan behind it
            assert ctx.foot_step_plan_get()["size"] == 0
            bad = gc.planner_structs(gait, True, False, capi.PROJECT_YAW)
            for p in bad:
                p.stance_time = 0.0
            assert _rc(ctx.set_foot_step_planner, bad) == BAD              # flying_trot_foot_step_planner.cpp:66
        ctx.set_foot_step_planner(good)
        gc.tick(ctx, T, 0.1, T.first_status)
        before = _plan_tables(ctx)
        for status in range(0b100000):
            if status not in legal[gait]:
                assert _rc(ctx.foot_step_plan, 0.2, status, 4) == BAD, (gait, bin(status))
        assert any(s not in legal[gait] for g in legal for s in legal[g])   # another gait's legal statuses were among them
        top = capi.MAX_PLAN_STEPS - (1 if gait == "flying_trot" else 0)
        assert _rc(ctx.foot_step_plan, 0.2, T.first_status, top + 1) == BAD and _rc(ctx.foot_step_plan, 0.2, T.first_status, -1) == BAD
        assert _equal(_plan_tables(ctx), before)
        # the longest plan fits the arrays of rtoc_foot_step_plan_get
        ctx.foot_step_plan(0.2, T.first_status, top)
        got = ctx.foot_step_plan_get()
        assert got["size"] == capi.MAX_PLAN_STEPS + 2 and got["ok"].all() and got["positions"].shape == (cases.BATCH, capi.MAX_PLAN_STEPS + 2, 4, 3)
        ctx.close()


@pytest.mark.gpu
def test_a_trot_named_explicitly_is_the_trot_of_a_zeroed_member():
    """e) gait = RTOC_GAIT_TROT set explicitly against the member left zero, over three ticks, bit for bit"""
    T = cases.Trot()
    m, x0 = cases.states(6, False)
    outs = []
    for explicit in (False, True):
        ctx = cases.trot_context(T, m, x0)
        structs = cases.planner_structs(True, False, capi.PROJECT_YAW)
        assert all(p.gait == 0 for p in structs)
        if explicit:
            for p in structs:
                p.gait = capi.GAIT_TROT
        ctx.set_foot_step_planner(structs)
        ticks = []
        for t, status in ((0.0, 0b1111), (0.12, 0b1001), (0.2, 0b0110)):
            cases.tick(ctx, T, t, status)
            ticks.append(_plan_tables(ctx))
        outs.append(ticks)
        ctx.close()
    for w, g in zip(*outs):
        assert _equal(w, g) and w["plan_ok"].all()
