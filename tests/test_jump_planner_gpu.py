"""RTOC_GAIT_JUMP through jump_init_kernel / jump_plan_kernel, the place kernels and jump_refs_kernel (foot_step_planner.hpp,
rt_foot_steps.hip) against the numpy restatement of the reference's JumpFootStepPlanner with the q_ref of MPCJump::init
(tests/jump_planner_restatement.py), the project's usual isolation checks -- a batch against batch-1 contexts, shared against
repeated commands, a clone -- bit for bit, the refusals, and one solver tick fed by the device planner against its twin fed through
the host tables.

Tolerances follow the rule of tests/test_gait_planner_gpu.py with the plan's size, 3: init composes one rotation onto R and adds one
rotated offset and one rotated jump to a position, so translations and CoM are held to 3e-14 x max(1, max|p|), R and the rotations
of the goal feet to 3e-14, q_ref to 3e-14 x max(1, max|q|).  The rotation of a foot the kinematics measured is the forward
kinematics' own and is held to the 1e-14 of tests/test_contact_frame_placements_gpu.py.  Under RTOC_PROJECT_AS_REFERENCE the goal
quaternion is not of unit length, CoM(2) and q_ref[0:3] pass through kinematics at it, and they are compared for bases with the
identity orientation alone, where the projection divides by exactly 1.

tests/test_jump_planner_restatement.py holds the run of contact statuses and the grids used here to what they are chosen for."""
import numpy as np
import pytest

import jump_planner_cases as jc
from helpers import check_parity
from robotoc_amd import capi
from robotoc_amd.capi import RtocError

YAW, AS_REFERENCE = capi.PROJECT_YAW, capi.PROJECT_AS_REFERENCE
STEPS_BY_PHASE = {3: np.array([1, 2, 2]), 2: np.array([1, 1])}   # mpc_jump.cpp:305-313, by the plan's size


def _surfaces(got, model):
    if jc.is_biped(model):
        return got["surfaces"]
    assert "surfaces" not in got   # point feet: every rotation is the identity, which the plan does not store
    B, n = got["positions"].shape[:2]
    return np.broadcast_to(np.eye(3), (B, n, 4, 3, 3))


def _compare_plan(label, model, got, planners, n, current_step, goal, with_goal_com):
    """goal: (surfaces, com) of step 2 as the restatement's init left them -- the steps that still hold them are the goal's"""
    assert got["size"] == n and got["current_step"] == current_step and got["ok"].all()
    assert all(pl.current_step == current_step and pl.size() == n for pl in planners)
    want_p = np.array([[pl.contact_positions(s) for s in range(n)] for pl in planners])
    want_S = np.array([[pl.contact_surfaces(s) for s in range(n)] for pl in planners])
    want_c = np.array([[pl.com(s) for s in range(n)] for pl in planners])
    want_R = np.array([[pl.R(s) for s in range(n)] for pl in planners])
    assert got["positions"].shape == want_p.shape
    scale = max(1.0, np.abs(want_p).max())
    check_parity(label + ": contact positions", np.abs(got["positions"] - want_p).max() / scale, 3e-14)
    check_parity(label + ": R", np.abs(got["R"] - want_R).max(), 3e-14)
    got_S = _surfaces(got, model)
    for s in range(n):
        at_goal = np.array_equal(want_c[:, s], goal[1])
        if with_goal_com or not at_goal:
            check_parity(label + ": CoM(%d)" % s, np.abs(got["com"][:, s] - want_c[:, s]).max() / scale, 3e-14)
        if not jc.is_biped(model):
            assert np.array_equal(got_S[:, s], want_S[:, s])
        elif np.array_equal(want_S[:, s], goal[0]):
            check_parity(label + ": rotations of the goal feet (%d)" % s, np.abs(got_S[:, s] - want_S[:, s]).max(), 3e-14)
        else:
            check_parity(label + ": rotations of the measured feet (%d)" % s, np.abs(got_S[:, s] - want_S[:, s]).max(), 1e-14)
    want_jl = np.array([pl.jump_length for pl in planners])
    assert np.array_equal(got["step_length"], want_jl)


# 17 = the four-feet mapping's 16 instances per wave and one; 33 = the two-feet mapping's 32 and one; the URDF's nv = 35 once; under
# the reference's projection the small-yaw states, and the identity orientation, where CoM(2) and q_ref[0:3] are compared too
PLAN_CASES = [("anymal", 17, YAW, "any"), ("anymal", 1, YAW, "any"), ("icub32", 33, YAW, "any"), ("icub", 5, YAW, "any"),
              ("anymal", 5, AS_REFERENCE, "small"), ("icub32", 5, AS_REFERENCE, "small"),
              ("anymal", 5, AS_REFERENCE, "level"), ("icub32", 5, AS_REFERENCE, "level")]


@pytest.mark.gpu
@pytest.mark.parametrize("model,batch,projection,orientation", PLAN_CASES)
def test_init_and_plan_against_the_restatement(oracle, model, batch, projection, orientation):
    """init, the stored q_ref, and the run of ticks full, full, 0, 0, full, full, 0 with the state changed between the ticks; a
    second init, at another state, starts over"""
    m, x0 = jc.states(model, 21, orientation, batch)
    xs = [x0, jc.moved(m, x0)]
    full = jc.full_status(model)
    with_goal_com = projection == YAW or orientation == "level"
    ctx = jc.plain_context(model, m, x0)
    ctx.set_foot_step_planner(jc.planner_structs(projection, range(batch)))
    planners = jc.restated_planners(model, projection, range(batch))
    for again in range(2):
        label = "%s batch %d projection %d %s init %d" % (model, batch, projection, orientation, again)
        ctx.set_initial_state(xs[again])
        ctx.foot_step_planner_init()
        want_q = jc.restated_init(oracle, model, m, planners, xs[again])
        goal = (np.array([pl.contact_surfaces(2) for pl in planners]), np.array([pl.com(2) for pl in planners]))
        _compare_plan(label, model, ctx.foot_step_plan_get(), planners, 3, 0, goal, with_goal_com)
        # the stored q_ref, as rtoc_foot_step_refs writes it on every row
        ctx.foot_step_refs(jc.jump_refs())
        q_tab, active, inst = ctx.configuration_ref_table()
        assert inst is True and active.all() and (q_tab == q_tab[:, :1]).all()
        keep = slice(None) if with_goal_com else slice(3, None)
        check_parity(label + ": q_ref", np.abs(q_tab[:, 0, keep] - want_q[:, keep]).max() / max(1.0, np.abs(want_q).max()), 3e-14)
        assert np.array_equal(q_tab[:, 0, 7:], xs[again][:, 7:m.nq])
        for tick, status in enumerate(jc.SEQUENCE if again == 0 else jc.SEQUENCE[:3]):
            status = full if status == "full" else status
            x = xs[(tick + again + 1) % 2]
            ctx.set_initial_state(x)
            ctx.foot_step_plan(0.1 * tick, status, tick % 3)   # t and planning_steps are not read
            feet, surfaces, _ = jc.kinematics(oracle, model, m, x[:, :m.nq])
            for b, pl in enumerate(planners):
                assert pl.plan(feet[b], surfaces[b], status)
            _compare_plan("%s tick %d status %s" % (label, tick, bin(status)), model, ctx.foot_step_plan_get(), planners,
                          jc.SIZES[tick], jc.CURRENT_STEPS[tick], goal, with_goal_com)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sto", (False, True))
@pytest.mark.parametrize("model", ("anymal", "icub32"))
def test_place_and_refs_on_the_jumps_grid(model, sto):
    """before the flight the placement table is plan step [1, 2, 2] by phase, after it [1, 1], bit for bit, the rotation table of
    the biped too; every row of the q_ref table is the stored q_ref, active; plain and with switching-time optimisation"""
    T = jc.JumpGrid(model)
    m, x0 = jc.states(model, 6, "any", jc.bc.BATCH)
    ctx = jc.jump_context(T, m, x0, sto=sto)
    stored = None
    for grid, status, x in ((T, T.full, x0), (jc.JumpGrid(model, phases=2), 0, jc.moved(m, x0))):
        grid.set_on(ctx, sto)   # (rtoc_set_grid forgets the tables, not the plan or the stored q_ref)
        ctx.set_initial_state(x)
        jc.tick(ctx, grid, 0.0, status)
        tab = jc.tables(ctx)
        n = int(tab["plan_size"])
        assert grid.n <= 12 and n == len(grid.phase_masks) and tab["plan_ok"].all() and tab["plan_current_step"] == 3 - n
        steps = STEPS_BY_PHASE[n][grid.phase]
        assert sorted(set(grid.phase.tolist())) == list(range(n))
        for i in range(grid.n):
            assert np.array_equal(tab["placements"][:, i], tab["plan_positions"][:, steps[i]])
            if jc.is_biped(model):
                assert np.array_equal(tab["rotations"][:, i], tab["plan_surfaces"][:, steps[i]])
        assert not np.array_equal(tab["placements"][0], tab["placements"][1])
        # the q_ref table: one row per instance, everywhere, active; it is q with the head moved by CoM(2) - CoM(0) of the init
        assert tab["q_active"].all() and (tab["q_ref"] == tab["q_ref"][:, :1]).all()
        assert not np.array_equal(tab["q_ref"][0], tab["q_ref"][1])
        if stored is None:
            stored = tab["q_ref"][:, 0].copy()
            assert np.array_equal(stored[:, :3], x0[:, :3] + (tab["plan_com"][:, 2] - tab["plan_com"][:, 0]))
            assert np.array_equal(stored[:, 7:], x0[:, 7:m.nq])
            assert not np.array_equal(tab["placements"][:, 0], tab["placements"][:, -1])   # the goal is somewhere else
        else:
            assert np.array_equal(tab["q_ref"][:, 0], stored)   # the state has moved on, the stored q_ref has not
    ctx.close()


def _three_ticks(T, m, ctx, xs, insts, fork=False):
    """on the ground, in the air, landed -- place and refs each time; fork: a clone taken after the init is ticked beside"""
    out, twin = [], (ctx.clone() if fork else None)
    for t, x, status in ((0.0, xs[0], T.full), (0.1, xs[1], 0), (0.2, xs[1], T.full)):
        for c in (ctx, twin) if twin is not None else (ctx,):
            c.set_initial_state(x[insts])
            jc.tick(c, T, t, status)
        out.append(jc.tables(ctx))
        if twin is not None:
            assert jc.equal(jc.tables(twin), out[-1])
    if twin is not None:
        twin.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("model", ("anymal", "icub32"))
def test_isolation_shared_commands_and_clone(model):
    """across three ticks: instance b of the batch = a batch-1 context with b's inputs and command; one shared command = five copies
    of it; a clone taken after init, ticked beside its source"""
    T = jc.JumpGrid(model)
    B = jc.bc.BATCH
    m, x0 = jc.states(model, 8, "any", B)
    xs = [x0, jc.moved(m, x0)]
    big = jc.jump_context(T, m, x0)
    want = _three_ticks(T, m, big, xs, list(range(B)), fork=True)
    big.close()
    assert not jc.equal(want[0], want[1]) and not jc.equal(want[1], want[2])
    for b in range(B):
        one = jc.jump_context(T, m, x0, insts=[b])
        got = _three_ticks(T, m, one, xs, [b])
        for w, g in zip(want, got):
            for k in w:
                if k in ("plan_size", "plan_current_step"):
                    assert w[k] == g[k]
                else:
                    assert np.array_equal(w[k][b], g[k][0]), (model, b, k)
        one.close()
    a = jc.jump_context(T, m, x0, shared_command=3)
    bctx = jc.jump_context(T, m, x0)
    bctx.set_foot_step_planner(jc.planner_structs(YAW, [3] * B))
    bctx.foot_step_planner_init()
    every = list(range(B))
    for w, g in zip(_three_ticks(T, m, a, xs, every), _three_ticks(T, m, bctx, xs, every)):
        assert jc.equal(w, g)
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
    """a refused call launches nothing and leaves the plan, the tables and current_step as they were"""
    BAD, NOT_READY = capi.ERR_BAD_ARG, capi.ERR_NOT_READY
    for model in ("anymal", "icub32"):
        T = jc.JumpGrid(model)
        B = jc.bc.BATCH
        m, x0 = jc.states(model, 6, "any", B)
        ctx = jc.jump_context(T, m, x0)
        jc.tick(ctx, T, 0.0, T.full)
        before = jc.tables(ctx)
        # Raibert mode: the reference has no such jump; structure that differs across the batch; an option outside {0, 1}
        for field, value, rows in (("mode", capi.FOOT_STEP_RAIBERT, range(B)), ("projection", AS_REFERENCE, [3]), ("gait", capi.GAIT_TROT, [3]),
                                   ("enable_stance_phase", 2, range(B))):
            bad = jc.planner_structs(YAW, range(B))
            for b in rows:
                setattr(bad[b], field, value)
                bad[b].swing_time, bad[b].stance_time, bad[b].gain = 0.2, 0.05, 0.7   # (what a Raibert pattern would need)
            assert _rc(ctx.set_foot_step_planner, bad) == BAD, field
            if len(rows) == B:
                assert _rc(ctx.set_foot_step_planner, bad[0]) == BAD, field
        # a status bit at or beyond the model's contacts
        nf = jc.feet_of(model)
        for status in (1 << nf, (1 << nf) | T.full, 1 << 5, 1 << 31):
            assert _rc(ctx.foot_step_plan, 0.1, status, 0) == BAD, bin(status)
        assert _rc(ctx.foot_step_plan, 0.1, T.full, -1) == BAD and _rc(ctx.foot_step_plan, 0.1, T.full, capi.MAX_PLAN_STEPS + 1) == BAD
        assert _rc(ctx.foot_step_place, T.phase[:-1]) == BAD and _rc(ctx.foot_step_place, T.phase) == BAD   # phase 2 > size - 2
        # the refs call: the configuration reference and nothing else
        for k in range(4):
            terms = [-1] * 4
            terms[k] = 0
            assert _rc(ctx.foot_step_refs, jc.jump_refs(foot_terms=terms)) == BAD, k
        assert _rc(ctx.foot_step_refs, jc.jump_refs(com_term=0)) == BAD
        assert _rc(ctx.foot_step_refs, jc.jump_refs(configuration=0)) == BAD
        assert _rc(ctx.foot_step_refs, jc.jump_refs(), T.phase[:-1]) == BAD   # nstages is not the grid's
        assert jc.equal(jc.tables(ctx), before)
        # rtoc_set_robot_model ends the planner
        ctx.set_robot_model(m)
        assert _rc(ctx.foot_step_plan, 0.3, T.full, 0) == NOT_READY and _rc(ctx.foot_step_refs, jc.jump_refs()) != 0
        # NOT_READY before init
        ctx.set_foot_step_planner(jc.planner_structs(YAW, range(B)))
        assert _rc(ctx.foot_step_plan, 0.0, T.full, 0) == NOT_READY and _rc(ctx.foot_step_refs, jc.jump_refs()) == NOT_READY
        assert _rc(ctx.foot_step_place, np.zeros(T.n, dtype=np.int32)) == NOT_READY and _rc(ctx.foot_step_plan_get) == NOT_READY
        ctx.close()
    # a model with three contacts; a model of mixed contact types
    good = jc.planner_structs(YAW, range(jc.bc.BATCH))
    am, ax0 = jc.states("anymal", 6, "any", jc.bc.BATCH)
    three = type(am).from_buffer_copy(am)
    three.ncontacts = 3
    im, ix0 = jc.states("icub32", 6, "any", jc.bc.BATCH)
    mixed = type(im).from_buffer_copy(im)
    mixed.contact_type[0] = 0   # RTOC_CONTACT_POINT ahead of a surface (a model lists its points first)
    for model, mm, x in (("anymal", three, ax0), ("icub32", mixed, ix0)):
        ctx = jc.plain_context(model, mm, x)
        assert _rc(ctx.set_foot_step_planner, good) == BAD and _rc(ctx.set_foot_step_planner, good[0]) == BAD
        assert _rc(ctx.foot_step_planner_init) == NOT_READY   # the refused call set no planner
        ctx.close()
    # a ParNMPC horizon is refused by every entry point
    from robotoc_amd import robot_model as rm
    from robotoc_amd.types import iiwa14_dims
    arm = capi.Context(iiwa14_dims(), 4, jc.bc.BATCH, 0)
    arm.set_robot_model(rm.load_named("iiwa14"))
    arm.parnmpc_set_horizon(4)
    for fn, args in ((arm.set_foot_step_planner, (good,)), (arm.foot_step_planner_init, ()), (arm.foot_step_plan, (0.0, 0b1111, 0)),
                     (arm.foot_step_place, (np.zeros(4, dtype=np.int32),)), (arm.foot_step_refs, (jc.jump_refs(),)),
                     (arm.foot_step_plan_get, ())):
        assert _rc(fn, *args) == BAD
    arm.close()


@pytest.mark.gpu
def test_the_other_gaits_keep_their_refusal_of_switching_times():
    """the jump's configuration reference does not depend on time and serves a grid with switching-time optimisation; going back to
    a periodic gait on the same context, the refs call is refused there as before"""
    import foot_step_planner_cases as cases
    T = jc.JumpGrid("anymal")
    m, x0 = jc.states("anymal", 6, "any", cases.BATCH)
    ctx = jc.jump_context(T, m, x0, sto=True)
    jc.tick(ctx, T, 0.0, T.full)
    ctx.set_foot_step_planner(cases.planner_structs(False, False, YAW))
    assert _rc(ctx.foot_step_plan, 0.0, 0b1111, 2) == capi.ERR_NOT_READY   # going from the jump ends the init's state
    ctx.foot_step_planner_init()
    ctx.foot_step_plan(0.0, 0b1111, 2)
    trot = cases.Trot()
    assert _rc(ctx.foot_step_refs, trot.refs(foot_terms=(-1, -1, -1, -1), com_term=-1), T.phase, T.phase_masks) == capi.ERR_BAD_ARG
    ctx.close()


@pytest.mark.gpu
def test_one_solver_tick_twin_against_twin():
    """ANYmal, N = 12, three instances with their own jumps: solver A fed by the device planner through contact_planner=, solver B
    by the host tables built from A's plan and q_ref read back.  The tables are equal, and three update_solution calls with a
    forced re-discretisation in the middle give the same KKT errors, event times and solutions, bit for bit"""
    from robotoc_amd.problems_jump import anymal_jump_mpc_solver
    from robotoc_amd.solver import ContactPlan
    B = 3
    jumps = np.array([[0.5, 0.0, 0.0], [0.3, 0.1, 0.0], [-0.2, 0.05, 0.02]])
    yaws = np.array([0.0, 0.3, -0.4])
    A, x0, info = anymal_jump_mpc_solver(jumps, yaws, batch=B, N=12, projection=YAW)
    pl = info["planner"]
    assert pl.size() == 3 and pl.current_step() == 0
    q_ref_tab, active, inst = A.ctx.configuration_ref_table()
    assert inst is True and active.all()
    positions = [pl.contact_positions(1), pl.contact_positions(2), pl.contact_positions(2)]
    assert not np.array_equal(positions[1][0], positions[1][1])
    host_plan = ContactPlan([0b1111, 0, 0b1111], positions, [])
    Bs, _, info_b = anymal_jump_mpc_solver(jumps, yaws, batch=B, N=12, projection=YAW, host_plan=host_plan, host_q_ref=q_ref_tab[:, 0])
    assert info_b["planner"] is None

    def same_tables():
        for a, b in zip(A.ctx.contact_placements(), Bs.ctx.contact_placements()):
            assert np.array_equal(a, b)
        for a, b in zip(A.ctx.configuration_ref_table(), Bs.ctx.configuration_ref_table()):
            assert np.array_equal(a, b)

    same_tables()
    for s in (A, Bs):
        s.init_constraints()
    for it in range(3):
        if it == 1:
            # a forced re-discretisation: the device planner places and sets q_ref again, the host path uploads again
            # (the solver's own mesh-refinement branch, ocp_solver.cpp:184-199, at the event times the first iteration left)
            for s in (A, Bs):
                s.event_times = s.ctx.sto_event_times()
                s._mesh_refinement(0.0)
            same_tables()
        ka, kb = A.update_solution(0.0, x0), Bs.update_solution(0.0, x0)
        assert np.isfinite(ka).all() and np.array_equal(ka, kb), it
        assert np.array_equal(A.ctx.sto_event_times(), Bs.ctx.sto_event_times())
        assert np.array_equal(A.get_solution(), Bs.get_solution())
    assert not np.array_equal(ka[0], ka[1])   # the instances do differ
    A.close()
    Bs.close()
