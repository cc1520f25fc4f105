"""TrotFootStepPlanner and the MPC references on the device (foot_step_planner.hpp, rt_foot_steps.hip) against the numpy
restatement of the reference (tests/foot_step_planner_restatement.py), and the project's usual isolation checks: a batch against
batch-1 contexts, shared against repeated commands, a clone -- all bit for bit.

Tolerances.  The plan: the kinematics bound the project already holds is 1e-14 (tests/test_contact_frame_placements_gpu.py); every
step composes one more rotation onto R (three multiply-adds per entry, the device's sin / cos within 1 to 2 ulp of numpy's) and adds
one more scaled offset to the centre of mass and the feet, so positions and CoM are held to 1e-14 x (planning_steps + 2) x
max(1, max|p|) and rotations to 1e-14 x (planning_steps + 2).  The Raibert step length is a sum of at most 11 terms and one
multiply-add: 1e-14 x max(1, |step_length|).  The references are compared with the restatement evaluated ON THE PLAN READ BACK,
so that the plan's own error does not enter: positions to 4e-16 x max(1, max|p|) x 4 (two products and a sum), quaternions to
1e-14 (acos / sin of slerp), active flags exactly."""
import numpy as np
import pytest

import foot_step_planner_cases as cases
import foot_step_planner_restatement as fsr
from helpers import check_parity
from robotoc_amd import capi
from robotoc_amd.capi import RtocError
from robotoc_amd.types import BUF_SOL, Records, joint_limit_rows, anymal_dims

STATUSES = (0b1111, 0b1001, 0b0110, 0b1111, 0b0110, 0b1001)


def _compare_plan(label, got, planners, steps):
    n = steps + 2
    assert got["size"] == n and got["ok"].all()
    assert all(got["current_step"] == pl.current_step and pl.size() == n for pl in planners)
    want_p = np.array([[pl.contact_positions(s) for s in range(n)] for pl in planners])
    want_c = np.array([[pl.com(s) for s in range(n)] for pl in planners])
    want_R = np.array([[pl.R(s) for s in range(n)] for pl in planners])
    scale = max(1.0, np.abs(want_p).max())
    check_parity(label + ": contact positions", np.abs(got["positions"] - want_p).max() / scale, 1e-14 * n)
    check_parity(label + ": CoM", np.abs(got["com"] - want_c).max() / scale, 1e-14 * n)
    check_parity(label + ": R", np.abs(got["R"] - want_R).max(), 1e-14 * n)


@pytest.mark.gpu
@pytest.mark.parametrize("raibert", [False, True])
@pytest.mark.parametrize("stance", [False, True])
@pytest.mark.parametrize("projection", [capi.PROJECT_AS_REFERENCE, capi.PROJECT_YAW])
def test_plan_against_the_restatement(oracle, raibert, stance, projection):
    """a) both modes, both stance settings, both projections; a run of ticks over the three legal contact statuses with planning_steps
    0, 1 and 6, so that current_step_ walks through every branch of :145-202 on both sides"""
    small = projection == capi.PROJECT_AS_REFERENCE
    m, x0 = cases.states(3 if small else 4, small)
    # (small: the reference's `norm` stays above 0.5 for this seed -- tests/test_foot_step_planner_restatement.py)
    feet, com = cases.kinematics(oracle, m, x0)
    ctx = cases.plain_context(m, x0)
    ctx.set_foot_step_planner(cases.planner_structs(raibert, stance, projection))
    planners = cases.restated_planners(raibert, stance, projection)
    for again in range(2):   # a second init starts over: current_step_ = 0, the filter cleared
        ctx.foot_step_planner_init()
        assert ctx.foot_step_plan_get()["size"] == 0
        for b, pl in enumerate(planners):
            pl.init(x0[b, :m.nq], feet[b], com[b])
        t = 0.0
        for k, status in enumerate(STATUSES if again == 0 else STATUSES[1:3]):
            for steps in (0, 1, 6):
                t += 0.07
                ctx.foot_step_plan(t, status, steps)
                for b, pl in enumerate(planners):
                    assert pl.plan(t, feet[b], x0[b, m.nq:], status, steps)
                got = ctx.foot_step_plan_get()
                _compare_plan("raibert %d stance %d projection %d status %s steps %d" % (raibert, stance, projection, bin(status), steps), got, planners, steps)
                want_sl = np.array([pl.step_length for pl in planners])
                check_parity("step length in force", np.abs(got["step_length"] - want_sl).max() / max(1.0, np.abs(want_sl).max()), 1e-14)
    ctx.close()


@pytest.mark.gpu
def test_filter_across_ticks(oracle):
    """b) eight ticks in Raibert mode, a new v per tick: two closer than 0.1 period to their predecessor (dropped), the last two push
    early samples out of the window"""
    m, x0 = cases.states(5, False)
    feet, com = cases.kinematics(oracle, m, x0)
    ctx = cases.plain_context(m, x0)
    ctx.set_foot_step_planner(cases.planner_structs(True, True, capi.PROJECT_YAW))
    planners = cases.restated_planners(True, True, capi.PROJECT_YAW)
    ctx.foot_step_planner_init()
    for b, pl in enumerate(planners):
        pl.init(x0[b, :m.nq], feet[b], com[b])
    period = 2.0 * (cases.SWING_TIME + 0.05)
    times = [0.0, 0.06, 0.08, 0.15, 0.17, 0.30, 0.62, 0.70]
    sizes = []
    rng = np.random.default_rng(11)
    for t in times:
        x = x0.copy()
        x[:, m.nq:] = rng.uniform(-1, 1, (cases.BATCH, m.nv))
        ctx.set_initial_state(x)
        ctx.foot_step_plan(t, 0b1111, 2)
        for b, pl in enumerate(planners):
            assert pl.plan(t, feet[b], x[b, m.nq:], 0b1111, 2)
        sizes.append(planners[0].filter.size())
        got = ctx.foot_step_plan_get()
        for b, pl in enumerate(planners):
            check_parity("step length after the tick at %.2f, instance %d" % (t, b),
                         np.abs(got["step_length"][b] - pl.step_length).max() / max(1.0, np.abs(pl.step_length).max()), 1e-14)
    # the sequence does what it was chosen for: two samples dropped, early ones pushed out by the last two
    assert sizes == [1, 2, 2, 3, 3, 4, 3, 3] and times[2] - times[1] < 0.1 * period and times[6] - times[1] > period
    ctx.close()


@pytest.fixture(scope="module")
def trot_tick(oracle):
    """one tick on the trot grid (Raibert, no stance phase, status 0b1111), its read-backs, and the context for further use"""
    T = cases.Trot()
    m, x0 = cases.states(6, False)
    ctx = cases.trot_context(T, m, x0)
    shared = np.random.default_rng(2).uniform(-1, 1, (T.n, 4, 3))
    ctx.set_contact_schedule(T.masks, shared)
    assert ctx.contact_placements()[2] is False
    cases.tick(ctx, T, 0.0)
    out = dict(T=T, m=m, x0=x0, ctx=ctx, plan=cases.plan_arrays(ctx), tables=cases.tables(ctx), rot=ctx.contact_placements()[1], shared=shared)
    yield out
    ctx.close()


@pytest.mark.gpu
def test_place_copies_the_plan_into_the_per_instance_table(trot_tick):
    """c) grid point i of instance b = contactPositions(phase_i + 1) of b's plan, bit for bit; the shared table turned per instance"""
    T, plan, ctx = trot_tick["T"], trot_tick["plan"], trot_tick["ctx"]
    assert ctx.contact_placements()[2] is True
    pos = trot_tick["tables"]["placements"]
    for i in range(T.n):
        assert np.array_equal(pos[:, i], plan["positions"][:, T.phase[i] + 1])
    assert not np.array_equal(pos[0], pos[1])
    assert np.array_equal(trot_tick["rot"], np.tile(np.eye(3), (cases.BATCH, T.n, 4, 1, 1)))   # rotations untouched


@pytest.mark.gpu
def test_references_against_the_restatement_on_the_plan(trot_tick):
    """d) the three references at every (instance, grid point)"""
    T, plan, tab, x0, m = trot_tick["T"], trot_tick["plan"], trot_tick["tables"], trot_tick["x0"], trot_tick["m"]
    # the grid contains what it was chosen for
    act = T.t > T.start
    rates = [fsr.swing_rate(t, T.start, T.period_swing, T.period_stance) for t in T.t]
    swing = [i for i in range(T.n) if act[i] and cases.PHASE_MASKS[T.phase[i]] != 0b1111]
    assert (~act).any() and any(rates[i][1] < 0.5 for i in swing) and any(rates[i][1] >= 0.5 for i in swing)
    assert any(rates[i][0] >= 1 for i in swing) and any(act[i] and cases.PHASE_MASKS[T.phase[i]] == 0b1111 for i in range(T.n))
    par = (T.start, T.period_swing, T.period_stance, T.nph)
    scale = max(1.0, np.abs(plan["positions"]).max())
    seen_active = 0
    for b in range(cases.BATCH):
        for i in range(T.n):
            for k in range(4):
                x, a = fsr.swing_foot_ref(plan["positions"][b], k, cases.PHASE_MASKS, T.t[i], T.phase[i], T.height, *par)
                assert tab["ref%d_active" % k][b, i] == a
                seen_active += a
                check_parity("swing foot reference", np.abs(tab["ref%d_p" % k][b, i] - x).max() / scale, 4e-16 * 4)
                assert np.array_equal(tab["ref%d_R" % k][b, i], np.eye(3))
            x, a = fsr.com_ref(plan["com"][b], cases.PHASE_MASKS, T.t[i], T.phase[i], *par)
            assert tab["ref4_active"][b, i] == a
            check_parity("CoM reference", np.abs(tab["ref4_p"][b, i] - x).max() / scale, 4e-16 * 4)
            q, a = fsr.configuration_ref(x0[b, :m.nq], plan["R"][b], cases.PHASE_MASKS, T.t[i], T.phase[i], *par)
            assert tab["q_active"][b, i] == a
            check_parity("configuration reference: quaternion", np.abs(tab["q_ref"][b, i, 3:7] - q[3:7]).max(), 1e-14)
            assert np.array_equal(np.delete(tab["q_ref"][b, i], range(3, 7)), np.delete(q, range(3, 7)))
    assert seen_active > 0


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def _plan_tables(ctx):
    p = cases.plan_arrays(ctx)
    t = cases.tables(ctx)
    t.update({"plan_" + k: v for k, v in p.items()})
    return t


@pytest.mark.gpu
def test_isolation_shared_commands_and_clone(trot_tick):
    """e) across two consecutive ticks (the filter state is covered): instance b of the batch = a batch-1 context with b's inputs and
    command; one shared command = five copies of it; a clone after a tick, then one more tick on both"""
    T, m, x0 = trot_tick["T"], trot_tick["m"], trot_tick["x0"]
    x1 = x0.copy()
    x1[:, m.nq:] *= -0.7

    def two_ticks(ctx, insts):
        out = []
        for t, x, status in ((0.0, x0, 0b1111), (0.12, x1, 0b1001)):
            ctx.set_initial_state(x[insts])
            cases.tick(ctx, T, t, status)
            out.append(_plan_tables(ctx))
        return out

    big = cases.trot_context(T, m, x0)
    want = two_ticks(big, list(range(cases.BATCH)))
    for b in range(cases.BATCH):
        one = cases.trot_context(T, m, x0, insts=[b])
        got = two_ticks(one, [b])
        for w, g in zip(want, got):
            for k in w:
                if k in ("plan_size", "plan_current_step"):
                    assert w[k] == g[k]
                else:
                    assert np.array_equal(w[k][b], g[k][0]), (b, k)
        one.close()
    # per_instance = 0 with one command = per_instance = 1 with five copies of it
    a = cases.trot_context(T, m, x0, shared_command=3)
    bctx = cases.trot_context(T, m, x0)
    bctx.set_foot_step_planner(cases.planner_structs(True, False, capi.PROJECT_YAW, [3] * cases.BATCH))
    every = list(range(cases.BATCH))
    for w, g in zip(two_ticks(a, every), two_ticks(bctx, every)):
        assert _equal(w, g)
    a.close()
    bctx.close()
    # a clone after the two ticks, then one more tick on both
    twin = big.clone()
    for c in (big, twin):
        cases.tick(c, T, 0.2, 0b0110)
    assert _equal(_plan_tables(big), _plan_tables(twin))
    assert not _equal(_plan_tables(big), want[1])
    twin.close()
    big.close()


@pytest.mark.gpu
def test_device_filled_tables_are_consumed_as_uploaded_ones(oracle, trot_tick):
    """f) context A fills its tables on the device; context B receives A's read-backs through the existing setters.  Three
    rtoc_contact_update_solution iterations of the trot OCP (configuration cost, four foot terms, a CoM term, friction cones): the
    iterate and the KKT errors are equal bit for bit, and no status bit is raised."""
    from robotoc_amd.costs import TaskRefEntry
    T, m, x0, tab = trot_tick["T"], trot_tick["m"], trot_tick["x0"], trot_tick["tables"]
    nv, nq = m.nv, m.nq

    def ocp(fill):
        ctx = cases.trot_context(T, m, x0)
        fill(ctx)
        dims = anymal_dims()
        ctx.set_constraint_rows(joint_limit_rows(dims))
        ctx.set_friction_cones(4, 3)
        ctx.set_constraint_bounds(np.concatenate([np.full(24, 3.0), np.full(24, 10.0), np.full(24, 80.0)]), 1.0e-3, 0.995)
        ctx.set_friction_coefficients(np.full(4, 0.7))
        wq = np.concatenate([np.full(6, 10.0), np.full(12, 0.1)])
        ctx.set_configuration_cost(cases.Q_ANYMAL, np.zeros(nv), np.zeros(12), wq, np.full(nv, 1.0), np.full(nv, 1e-3), np.full(12, 1e-3),
                                   10.0 * wq, np.full(nv, 1.0), wq, np.full(nv, 1.0), np.full(nv, 1e-3))
        S = Records(ctx.L, "sol")
        sol = S.zeros(cases.BATCH, T.n)
        mass = sum(m.mass[i] for i in range(m.njoints))
        for b in range(cases.BATCH):
            for i in range(T.n):
                S.f(sol[b, i], "q")[:nq] = x0[b, :nq]
                act = [c for c in range(4) if (int(T.masks[i]) >> c) & 1]
                for j, c in enumerate(act):   # the stack of the active contacts: the robot's weight, in every contact's own frame
                    S.f(sol[b, i], "f")[3 * j:3 * j + 3] = oracle.rbd_contact_placement(m, x0[b, :nq], c)[0].T @ np.array([0.0, 0.0, 9.81 * mass / len(act)])
        ctx.upload(BUF_SOL, sol)
        ctx.contact_init_constraints()
        errs = [ctx.contact_update_solution() for _ in range(3)]
        out = ctx.download(BUF_SOL, (ctx.buffer_count(BUF_SOL),)), np.array(errs), ctx.status()
        ctx.close()
        return out

    def on_device(ctx):
        cases.tick(ctx, T, 0.0)

    def uploaded(ctx):
        ctx.set_contact_placements(tab["placements"])
        for k in range(5):
            rows = []
            for b in range(cases.BATCH):
                arr = (TaskRefEntry * T.n)()
                for i in range(T.n):
                    arr[i].R[:] = list(tab["ref%d_R" % k][b, i].reshape(-1))
                    arr[i].p[:] = list(tab["ref%d_p" % k][b, i])
                    arr[i].active = int(tab["ref%d_active" % k][b, i])
                rows.append(arr)
            ctx.set_task_ref_table(k, rows, per_instance=True)
        ctx.set_configuration_ref_table(tab["q_ref"], tab["q_active"])

    sol_a, err_a, st_a = ocp(on_device)
    sol_b, err_b, st_b = ocp(uploaded)
    assert (st_a == 0).all() and (st_b == 0).all()
    assert np.isfinite(sol_a).all() and np.array_equal(sol_a, sol_b) and np.array_equal(err_a, err_b)


def _rc(fn, *a):
    try:
        fn(*a)
    except RtocError as e:
        return e.code
    return 0


@pytest.mark.gpu
def test_refusals_launch_nothing(oracle):
    """g) every RTOC_ERR_* named in the header is reached; a refused call leaves plan, tables and current_step as they were"""
    BAD, NOT_READY = capi.ERR_BAD_ARG, capi.ERR_NOT_READY
    T = cases.Trot()
    m, x0 = cases.states(6, False)
    ctx = capi.Context(anymal_dims(), T.n, cases.BATCH, 0)
    ctx.set_grid(T.grids)
    structs = cases.planner_structs(True, False, capi.PROJECT_YAW)
    assert _rc(ctx.set_foot_step_planner, structs) == NOT_READY          # no model
    ctx.set_robot_model(m)
    assert _rc(ctx.foot_step_planner_init) == NOT_READY                  # no planner
    for field, value in (("mode", 2), ("projection", 3), ("enable_stance_phase", 2), ("swing_time", 0.0), ("stance_time", -0.1), ("gain", 0.0)):
        bad = cases.planner_structs(True, False, capi.PROJECT_YAW)
        for p in bad:
            setattr(p, field, value)
        assert _rc(ctx.set_foot_step_planner, bad) == BAD, field
    for field, value in (("gain", 0.5), ("swing_time", 0.3), ("mode", 0), ("projection", 0)):   # structure must agree across the batch
        bad = cases.planner_structs(True, False, capi.PROJECT_YAW)
        setattr(bad[3], field, value)
        assert _rc(ctx.set_foot_step_planner, bad) == BAD, field
    ctx.set_foot_step_planner(structs)
    assert _rc(ctx.foot_step_planner_init) == NOT_READY                  # no initial state
    ctx.set_initial_state(x0)
    assert _rc(ctx.foot_step_plan, 0.0, 0b1111, 2) == NOT_READY          # no init
    ctx.foot_step_planner_init()
    assert _rc(ctx.foot_step_place, T.phase) == NOT_READY                # no plan
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS) == NOT_READY
    ctx.foot_step_plan(0.0, 0b1111, 4)
    assert _rc(ctx.foot_step_place, T.phase) == NOT_READY                # no schedule
    ctx.set_contact_schedule(T.masks)
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS) == NOT_READY   # no grid times
    ctx.set_grid_times(T.t)
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS) == BAD         # the terms are not set
    ctx.set_task_costs(cases.task_terms(m))
    cases.tick(ctx, T, 0.1)
    before = _plan_tables(ctx)
    for status in (0b0000, 0b1011, 0b0001, 0b10000):
        assert _rc(ctx.foot_step_plan, 0.2, status, 4) == BAD
    assert _rc(ctx.foot_step_plan, 0.2, 0b1001, -1) == BAD and _rc(ctx.foot_step_plan, 0.2, 0b1001, capi.MAX_PLAN_STEPS + 1) == BAD
    assert _rc(ctx.foot_step_place, T.phase[:-1]) == BAD                 # not the grid's nstages
    assert _rc(ctx.foot_step_place, T.phase + 2) == BAD                  # a phase beyond size - 2
    assert _rc(ctx.foot_step_place, T.phase - 1) == BAD
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase[:-1], cases.PHASE_MASKS) == BAD
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase + 2, cases.PHASE_MASKS + [0b1111, 0b1001]) == BAD   # phase + nph reaches past the plan
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS[:3]) == BAD                          # a phase without a mask
    assert _rc(ctx.foot_step_refs, T.refs(foot_terms=(0, 1, 2, 5)), T.phase, cases.PHASE_MASKS) == BAD       # no such term
    assert _rc(ctx.foot_step_refs, T.refs(foot_terms=(0, 1, 2, 2)), T.phase, cases.PHASE_MASKS) == BAD       # named twice
    r = T.refs()
    r.swing_height[1] = -0.01
    assert _rc(ctx.foot_step_refs, r, T.phase, cases.PHASE_MASKS) == BAD
    r = T.refs()
    r.q_num_phases_in_period = 0
    assert _rc(ctx.foot_step_refs, r, T.phase, cases.PHASE_MASKS) == BAD
    terms = cases.task_terms(m)
    terms[4].ref_kind = 0   # a constant reference: not a table
    ctx.set_task_costs(terms)
    assert _rc(ctx.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS) == BAD
    ctx.set_task_costs(cases.task_terms(m))
    assert _rc(ctx.foot_step_refs, T.refs(foot_terms=(4, 1, 2, 3), com_term=0), T.phase, cases.PHASE_MASKS) == BAD   # a CoM term as a foot, a foot as the CoM
    # the read-backs take at most `batch` instances
    L, over = capi.lib(), cases.BATCH + 1
    assert L.rtoc_foot_step_plan_get(ctx._h, None, None, None, None, None, over, None, None) == BAD
    assert L.rtoc_get_task_ref_table(ctx._h, 0, None, over, None) == BAD and L.rtoc_get_task_ref_table(ctx._h, 8, None, 1, None) == BAD
    assert L.rtoc_get_configuration_ref_table(ctx._h, None, None, over, None) == BAD
    assert L.rtoc_foot_step_plan_get(ctx._h, None, None, None, None, None, -1, None, None) == BAD
    assert _equal(_plan_tables(ctx), before)
    # a grid with switching-time optimisation: every instance has its own grid times, which the references do not take
    sto = ctx.clone()
    sto.sto_set_problem(0.0, 0.12, [0.03, 0.07, 0.09], [0.005] * 4)
    assert _equal(_plan_tables(sto), before)
    assert _rc(sto.foot_step_refs, T.refs(), T.phase, cases.PHASE_MASKS) == BAD
    assert _equal(_plan_tables(sto), before)
    sto.close()
    # the planner outlives rtoc_set_grid, the tables do not; rtoc_set_robot_model ends the planner
    ctx.set_grid(T.grids[:4] + T.grids[-1:])
    ctx.set_grid(T.grids)
    assert _rc(ctx.task_ref_table, 0) == NOT_READY and _rc(ctx.configuration_ref_table) == NOT_READY
    ctx.set_contact_schedule(T.masks)
    ctx.set_grid_times(T.t)
    ctx.foot_step_place(T.phase)
    ctx.foot_step_refs(T.refs(), T.phase, cases.PHASE_MASKS)
    assert _equal(_plan_tables(ctx), before)
    ctx.set_robot_model(m)
    assert _rc(ctx.foot_step_plan, 0.3, 0b1111, 2) == NOT_READY
    ctx.set_foot_step_planner(structs)
    ctx.set_foot_step_planner(None)
    assert _rc(ctx.foot_step_planner_init) == NOT_READY
    ctx.close()
    # a model that has not exactly four point contacts (iCub: two surface contacts), on an ordinary grid
    from robotoc_amd import robot_model as rm
    from robotoc_amd.grid import uniform_grid
    from robotoc_amd.types import icub_dims
    icub = rm.load_named("icub")
    two = capi.Context(icub_dims(icub.nv), 4, cases.BATCH, 0)
    two.set_grid(uniform_grid(3, 0.02, dimf=12))
    two.set_robot_model(icub)
    assert _rc(two.set_foot_step_planner, structs) == BAD and _rc(two.set_foot_step_planner, structs[0]) == BAD
    two.set_initial_state(np.tile(np.concatenate([[0, 0, 0.6, 0, 0, 0, 1.0], np.zeros(icub.nq - 7 + icub.nv)]), (cases.BATCH, 1)))
    assert _rc(two.foot_step_planner_init) == NOT_READY                 # the refused call set no planner
    two.close()
    # a ParNMPC horizon is refused by every entry point
    arm = rm_arm_context()
    for fn, args in ((arm.set_foot_step_planner, (structs,)), (arm.foot_step_planner_init, ()), (arm.foot_step_plan, (0.0, 0b1111, 1)),
                     (arm.foot_step_place, (np.zeros(4, dtype=np.int32),)), (arm.foot_step_refs, (T.refs(), np.zeros(4, dtype=np.int32), [15]))):
        assert _rc(fn, *args) == BAD
    arm.close()


def rm_arm_context():
    """a fixed-base arm on a ParNMPC horizon"""
    from robotoc_amd import robot_model as rm
    from robotoc_amd.types import iiwa14_dims
    ctx = capi.Context(iiwa14_dims(), 4, cases.BATCH, 0)
    ctx.set_robot_model(rm.load_named("iiwa14"))
    ctx.parnmpc_set_horizon(4)
    return ctx
