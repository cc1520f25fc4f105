"""One life cycle for every table of the context that is "one for the batch, or one per instance", through the C ABI alone:
the contact placements (positions alone; positions and rotations), the q_ref table, and the reference tables of task terms 0 and
RTOC_MAX_TASK_COSTS - 1.  Every table goes through the same steps (shared, per instance, shared again, refused sets, a new grid, a
clone, the planner writing it, graph replays); where include/rtoc_robot.h documents a difference between the tables it is that
table's expectation in its class below, in one place.

ANYmal, batch 3, max_stages 5, a grid of 3 points and then one of 4: the smallest sizes at which "shared", "per instance",
"repeated for every instance" and "strided by nstages, not by max_stages" are four different things.  Criteria are bit-for-bit:
rows that were uploaded come back as they were, and records are compared between contexts that must have read the same rows.

Behaviour these tests pin was that of the runtime before the tables had one owner type (every case passed on it unchanged), with
one exception: rtoc_set_contact_placements used to start a new graph epoch on every call, so "the same table set again leaves the
graph standing" (test_graph_replays_across_the_setters) held for the q_ref and task tables only; it holds for all five now."""
import ctypes as C

import numpy as np
import pytest

import foot_step_planner_cases as fsc
import per_instance_placement_cases as pic
from graph_twin import Twin
from robotoc_amd import capi, robot_model as rm
from robotoc_amd.costs import MAX_TASK_COSTS, TaskCost
from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import (BUF_CDD, BUF_CON, BUF_DIR, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP, Records, anymal_dims,
                               joint_limit_rows)

OK, BAD, NOT_READY = 0, capi.ERR_BAD_ARG, capi.ERR_NOT_READY
B, MAX_STAGES, N0, N1 = 3, 5, 3, 4
NC, NQ = 4, 19
TAU = 0.995
LAST = MAX_TASK_COSTS - 1
_ip = C.POINTER(C.c_int)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class Problem:
    """what every context of this file is built from"""

    def __init__(self):
        self.m, self.dims = rm.load_named("anymal"), anymal_dims()
        m = self.m
        assert m.ncontacts == NC and m.nq == NQ
        self.grids = {N0: uniform_grid(N0 - 1, 0.02, dimf=12), N1: uniform_grid(N1 - 1, 0.02, dimf=12)}
        self.t = {n: 0.02 * np.arange(n) for n in (N0, N1)}
        rng = np.random.default_rng(7)
        self.x0 = np.zeros((B, m.nq + m.nv))
        for b, (x, y, yaw) in enumerate([(0.0, 0.0, 0.0), (0.7, -0.4, 0.3), (-0.5, 0.9, -0.6)]):
            self.x0[b, :m.nq], self.x0[b, m.nq:] = pic._yaw(pic.Q_ANYMAL, x, y, yaw), 0.1 * rng.uniform(-1, 1, m.nv)
        S = Records(capi.layout_for(self.dims), "sol")
        self.sol = {}
        for n in (N0, N1):
            sol = 0.3 * rng.uniform(-1, 1, (B, n, S.stride))
            for b in range(B):
                for i in range(n):
                    q = self.x0[b, :m.nq].copy()
                    q[:3] += 0.02 * rng.uniform(-1, 1, 3)
                    q[3:7] += 0.02 * rng.uniform(-1, 1, 4)
                    q[3:7] /= np.linalg.norm(q[3:7])
                    q[7:] += 0.1 * rng.uniform(-1, 1, m.nq - 7)
                    S.f(sol[b, i], "q")[:m.nq] = q
            self.sol[n] = sol
        wq = np.concatenate([np.full(6, 10.0), np.full(12, 1.0)])
        nv = m.nv
        self.cost = dict(q_ref=pic.Q_ANYMAL, v_ref=np.zeros(nv), u_ref=np.zeros(12), q_weight=wq, v_weight=np.full(nv, 1.0),
                         a_weight=np.full(nv, 1e-3), u_weight=np.full(12, 1e-3), q_weight_terminal=10.0 * wq, v_weight_terminal=np.full(nv, 1.0),
                         q_weight_impact=wq, v_weight_impact=np.full(nv, 1.0), dv_weight_impact=np.full(nv, 1e-3))
        # where the feet stand: the device's own kinematics at x0
        c = capi.Context(self.dims, MAX_STAGES, B, 0)
        c.set_grid(self.grids[N0])
        c.set_robot_model(m)
        c.set_initial_state(self.x0)
        _, self.feet, _ = c.contact_frame_placements("x0")
        c.close()

    def terms(self):
        """term 0 (a foot) and the last term (the centre of mass) read a table; the terms between them have constant references"""
        out = []
        for k in range(MAX_TASK_COSTS):
            t = TaskCost()
            t.kind, t.ref_kind = (1 if k == LAST else 0), (3 if k in (0, LAST) else 0)   # RTOC_TASK_COM | _FRAME_3D; RTOC_REF_TABLE | constant
            if k != LAST:
                t.frame_parent = self.m.contact_parent[k % NC]
                t.frame_p[:] = list(self.m.contact_p[k % NC])
                t.x0[:] = list(self.feet[0, k % NC])
            w = 1.0e2 if k in (0, LAST) else 1.0
            t.weight[:], t.weight_terminal[:], t.weight_impact[:] = [w] * 3, [w] * 3, [w] * 3
            out.append(t)
        return out

    def context(self, n, tables=()):
        """a context on the grid of n points with everything rtoc_contact_eval_kkt reads; `tables`: set shared, with their base rows"""
        c = capi.Context(self.dims, MAX_STAGES, B, 0)
        c.set_robot_model(self.m)
        c.set_configuration_cost(**self.cost)
        c.set_task_costs(self.terms())
        c.set_initial_state(self.x0)
        self.regrid(c, n)
        for t in tables:
            assert t.set(c, t.rows(self, n, 0), n, 0) == OK
        return c

    def regrid(self, c, n):
        c.set_grid(self.grids[n])
        c.set_contact_schedule(np.full(n, 0b1111, dtype=np.uint32))
        c.set_grid_times(self.t[n])
        c.upload(BUF_SOL, self.sol[n])

    def records(self, c, n):
        c.contact_eval_kkt()
        c.sync()
        out = {w: c.download(b, (B, n, getattr(c.L, w).stride)) for b, w in ((BUF_KKT, "kkt"), (BUF_CDD, "cdd"))}
        assert all(np.isfinite(v).all() for v in out.values())
        return out


class Placements:
    """rtoc_set_contact_placements: no nstages argument (the rows are the schedule's); a table that was never given reads as zeros
    (positions) / identities (rotations); RTOC_ERR_NOT_READY comes through the schedule, which rtoc_set_grid outdates"""
    HAS_NSTAGES, REFUSES_MODE_2, UNSET_READS = False, True, OK

    def __init__(self, with_rot):
        self.with_rot = with_rot
        self.name = "placements_pos_rot" if with_rot else "placements_pos"

    def rows(self, P, n, inst, seed=0):
        rng = np.random.default_rng(100 + seed)
        lead = (B, n) if inst else (n,)
        pos = (P.feet[:, None] if inst else P.feet[0][None]) + 0.02 * rng.uniform(-1, 1, lead + (NC, 3))
        rot = np.tile(np.eye(3).reshape(-1), lead + (NC, 1)) + 0.01 * rng.uniform(-1, 1, lead + (NC, 9))
        return (np.ascontiguousarray(pos), np.ascontiguousarray(rot)) if self.with_rot else (np.ascontiguousarray(pos),)

    def poison(self, rows):
        rows[0].reshape(-1)[4] = np.inf   # contact 1 of the first grid point: active

    def set(self, c, rows, n, inst):
        return capi.lib().rtoc_set_contact_placements(c._h, _dp(rows[0]), _dp(rows[1]) if self.with_rot else None, inst)

    def get(self, c, n, count):
        pos, rot, inst = np.full((count, n, NC, 3), np.nan), np.full((count, n, NC, 9), np.nan), C.c_int(-1)
        rc = capi.lib().rtoc_get_contact_placements(c._h, _dp(pos), _dp(rot), count, C.byref(inst))
        if rc == OK and not self.with_rot:
            assert np.array_equal(rot, np.tile(np.eye(3).reshape(-1), (count, n, NC, 1)))   # never given: identities
        return rc, ((pos, rot) if self.with_rot else (pos,)), inst.value


class QRef:
    """rtoc_set_configuration_ref_table: q_ref rows and their isActive flags"""
    HAS_NSTAGES, REFUSES_MODE_2, UNSET_READS = True, True, NOT_READY
    name = "q_ref"

    def rows(self, P, n, inst, seed=0):
        rng = np.random.default_rng(200 + seed)
        lead = (B, n) if inst else (n,)
        q = np.tile(pic.Q_ANYMAL, lead + (1,))
        q[..., 7:] += 0.1 * rng.uniform(-1, 1, lead + (NQ - 7,))
        act = np.ones(lead, dtype=np.int32)
        act.reshape(-1)[1] = 0   # an inactive row comes back as such
        return np.ascontiguousarray(q), act

    def poison(self, rows):
        rows[0].reshape(-1)[8] = np.nan   # row 0: active

    def set(self, c, rows, n, inst):
        return capi.lib().rtoc_set_configuration_ref_table(c._h, _dp(rows[0]), rows[1].ctypes.data_as(_ip), n, inst)

    def get(self, c, n, count):
        q, act, inst = np.full((count, n, NQ), np.nan), np.full((count, n), -1, dtype=np.int32), C.c_int(-1)
        rc = capi.lib().rtoc_get_configuration_ref_table(c._h, _dp(q), act.ctypes.data_as(_ip), count, C.byref(inst))
        return rc, (q, act), inst.value


class TaskRef:
    """rtoc_set_task_ref_table: entries of 13 doubles (R, p, the isActive flag and padding in the last).  per_instance is a truth
    value here: the header names no refusal for it, and 2 reads as "per instance\""""
    HAS_NSTAGES, REFUSES_MODE_2, UNSET_READS = True, False, NOT_READY

    def __init__(self, term):
        self.term, self.name = term, "task_ref_%d" % term

    def rows(self, P, n, inst, seed=0):
        rng = np.random.default_rng(300 + 10 * self.term + seed)
        lead = (B, n) if inst else (n,)
        raw = np.zeros(lead + (13,))
        raw[..., :9] = np.eye(3).reshape(-1)
        where = P.feet[:, 0] if self.term == 0 else P.x0[:, :3]
        raw[..., 9:12] = (where[:, None] if inst else where[0][None]) + 0.05 * rng.uniform(-1, 1, lead + (3,))
        raw.view(np.int32).reshape(lead + (26,))[..., 24] = 1   # active
        return (np.ascontiguousarray(raw),)

    def poison(self, rows):
        rows[0].reshape(-1)[10] = np.nan

    def set(self, c, rows, n, inst):
        return capi.lib().rtoc_set_task_ref_table(c._h, self.term, rows[0].ctypes.data_as(C.c_void_p), n, inst)

    def get(self, c, n, count):
        raw, inst = np.full((count, n, 13), np.nan), C.c_int(-1)
        rc = capi.lib().rtoc_get_task_ref_table(c._h, self.term, raw.ctypes.data_as(C.c_void_p), count, C.byref(inst))
        return rc, (raw,), inst.value


TABLES = [Placements(False), Placements(True), QRef(), TaskRef(0), TaskRef(LAST)]
# the tables rtoc_contact_eval_kkt needs besides the one under test (the terms name two tables; placements and q_ref are optional)
NEEDED = [t for t in TABLES if isinstance(t, TaskRef)]


@pytest.fixture(scope="module")
def P():
    return Problem()


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _read(tab, c, n, count, want_mode):
    rc, got, mode = tab.get(c, n, count)
    assert rc == OK and mode == want_mode, (tab.name, rc, mode)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tab", TABLES, ids=[t.name for t in TABLES])
def test_life_cycle(P, tab):
    others = [t for t in NEEDED if t.name != tab.name]
    c = P.context(N0, others)
    # 0. never set
    rc, got, mode = tab.get(c, N0, B)
    assert rc == tab.UNSET_READS
    if rc == OK:
        assert mode == 0 and not got[0].any()   # zeros
    # 1. shared: the rows repeated for every instance
    shared = tab.rows(P, N0, 0)
    assert tab.set(c, shared, N0, 0) == OK
    got = _read(tab, c, N0, B, 0)
    assert _same(got, [np.stack([a] * B) for a in shared])
    # 2. per instance, distinct rows; count = batch, 1, 0
    own = tab.rows(P, N0, 1, seed=1)
    assert not np.array_equal(own[0][0], own[0][1]) and not np.array_equal(own[0][1], own[0][2])
    assert tab.set(c, own, N0, 1) == OK
    assert _same(_read(tab, c, N0, B, 1), own)
    assert _same(_read(tab, c, N0, 1, 1), [a[:1] for a in own])
    untouched = _read(tab, c, N0, 0, 1)
    assert all(a.size == 0 for a in untouched)
    per_instance_records = P.records(c, N0)
    # 3. shared again: the records are those of a context that only ever had the shared table
    assert tab.set(c, shared, N0, 0) == OK
    assert _same(_read(tab, c, N0, B, 0), [np.stack([a] * B) for a in shared])
    got = P.records(c, N0)
    fresh = P.context(N0, others + [tab])
    want = P.records(fresh, N0)
    fresh.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), (tab.name, k)
    assert any(not np.array_equal(per_instance_records[k], want[k]) for k in want), "the records do not read " + tab.name
    # 4. refused sets leave the table as it is
    before = _read(tab, c, N0, B, 0)
    refusals = []
    if tab.HAS_NSTAGES:
        refusals.append((tab.rows(P, N1, 0, seed=2), N1, 0, BAD))
    bad = tab.rows(P, N0, 1, seed=3)
    tab.poison(bad)
    refusals.append((bad, N0, 1, BAD))
    if tab.REFUSES_MODE_2:
        refusals.append((tab.rows(P, N0, 1, seed=4), N0, 2, BAD))
    for rows, n, inst, want_rc in refusals:
        assert tab.set(c, rows, n, inst) == want_rc, (tab.name, n, inst)
        assert _same(_read(tab, c, N0, B, 0), before)
    if not tab.REFUSES_MODE_2:   # a truth value: 2 is "per instance"
        rows = tab.rows(P, N0, 1, seed=4)
        assert tab.set(c, rows, N0, 2) == OK
        assert _same(_read(tab, c, N0, B, 1), rows)
        assert tab.set(c, shared, N0, 0) == OK
    # 5. a new grid: the rows are gone until they are set for it, then they come back in the new row count
    c.set_grid(P.grids[N1])
    rc, _, _ = tab.get(c, N1, B)
    assert rc == NOT_READY
    P.regrid(c, N1)
    rc, got, mode = tab.get(c, N1, B)
    assert rc == tab.UNSET_READS
    if rc == OK:
        assert mode == 0 and not got[0].any()
    own1 = tab.rows(P, N1, 1, seed=5)
    assert tab.set(c, own1, N1, 1) == OK
    assert _same(_read(tab, c, N1, B, 1), own1)   # instance b's rows start b * N1 rows in, not b * MAX_STAGES
    for t in others:
        assert t.set(c, t.rows(P, N1, 0), N1, 0) == OK
    rec1 = P.records(c, N1)
    # 6. a clone has the rows and the mode, and keeps them when the original is gone
    twin = c.clone()
    assert _same(_read(tab, twin, N1, B, 1), own1)
    c.close()
    assert _same(_read(tab, twin, N1, B, 1), own1)
    rec2 = P.records(twin, N1)
    for k in rec1:
        assert np.array_equal(rec1[k], rec2[k]), (tab.name, k)
    twin.close()


@pytest.mark.gpu
def test_the_planner_writes_the_tables_then_a_shared_set_takes_over(P):
    """7. rtoc_foot_step_place / rtoc_foot_step_refs write the placements, the tables of the terms they are given and the q_ref
    table on the device, per instance; a shared set afterwards is a shared table again"""
    c = P.context(N0)
    c.set_foot_step_planner(fsc.planner_structs(True, False, capi.PROJECT_YAW, range(B)))
    c.foot_step_planner_init()
    c.foot_step_plan(0.0, 0b1111, 4)
    T = fsc.Trot.__new__(fsc.Trot)
    T.nph, T.start, T.period_swing, T.period_stance, T.height = 2, 0.005, 0.018, 0.011, 0.08
    phase = np.zeros(N0, dtype=np.int32)
    c.foot_step_place(phase)
    c.foot_step_refs(T.refs(foot_terms=(0, -1, -1, -1), com_term=LAST), phase, np.array([0b1111], dtype=np.uint32))
    written = [t for t in TABLES if not (isinstance(t, Placements) and t.with_rot)]
    for tab in written:
        got = _read(tab, c, N0, B, 1)
        assert all(np.isfinite(a).all() for a in got), tab.name
    instances_differ = _read(TABLES[0], c, N0, B, 1)[0]
    assert not np.array_equal(instances_differ[0], instances_differ[1])
    assert np.isfinite(P.records(c, N0)["kkt"]).all()
    for tab in written:
        shared = tab.rows(P, N0, 0)
        assert tab.set(c, shared, N0, 0) == OK
        assert _same(_read(tab, c, N0, B, 0), [np.stack([a] * B) for a in shared]), tab.name
    got = P.records(c, N0)
    fresh = P.context(N0, written)
    want = P.records(fresh, N0)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    fresh.close()
    c.close()


class TableTwin(Twin):
    """8. two contexts with every table set shared, one of them graphed; rtoc_contact_update_solution = rtoc_contact_eval_kkt and
    the graphed rtoc_newton_iteration"""

    def __init__(self, P):
        self.P = P
        ctxs = []
        for graph in (False, True):
            c = P.context(N0, [TABLES[1], TABLES[2], TABLES[3], TABLES[4]])
            c.set_constraint_rows(joint_limit_rows(P.dims))
            c.set_friction_cones(4, 3)
            c.set_constraint_bounds(np.concatenate([np.full(24, 2.5), np.full(24, 15.0), np.full(24, 80.0)]), 1.0e-3, TAU)
            c.set_friction_coefficients(np.full(4, 0.7))
            c.set_graph(graph)
            ctxs.append(c)
        self.err = {}
        super().__init__(ctxs[0], ctxs[1], self.restore, self.outputs, lambda c: c.graph_replay_count())
        L = self.plain.L
        self.poison = (np.full((B, N0, L.ric.stride), np.nan), np.full((B, N0, L.dir.stride), np.nan))

    def restore(self, c):
        c.upload(BUF_SOL, self.P.sol[N0])
        c.contact_init_constraints()
        c.upload(BUF_STEP, np.ones((B, 2)))
        c.upload(BUF_RIC, self.poison[0])
        c.upload(BUF_DIR, self.poison[1])
        c.clear_status()

    def launch(self, c):
        self.err[id(c)] = c.contact_update_solution(TAU)

    def outputs(self, c):
        out = {w: c.download(b, (B, N0, getattr(c.L, w).stride)) for b, w in ((BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_KKT, "kkt"), (BUF_CDD, "cdd"),
                                                                             (BUF_CON, "con"), (BUF_SOL, "sol"))}
        out["step"], out["status"], out["kkt_error"] = c.download(BUF_STEP, (B, 2)), c.status(), self.err.get(id(c))
        return out


@pytest.fixture(scope="module")
def twin(P):
    t = TableTwin(P)
    yield t
    t.plain.close()
    t.graph.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tab", TABLES, ids=[t.name for t in TABLES])
def test_graph_replays_across_the_setters(P, twin, tab):
    shared = tab.rows(P, N0, 0)
    twin.both(lambda c: tab.set(c, shared, N0, 0))
    for k in range(2):   # the first run at this epoch, then the capture with its first launch
        twin.run(twin.launch, "run %d" % k)
    # the same table again: same data, same mode, same grid, same allocation -- the graph stands, the next iteration is a replay
    assert twin.both(lambda c: tab.set(c, shared, N0, 0)) == (OK, OK)
    n0 = twin.replay_count()
    twin.run(twin.launch, "the same table set again")
    assert twin.replay_count() == n0 + 1, "%s set again as it was: the next iteration was not a replay" % tab.name
    # a mode flip and back: a new epoch each time, and every run equal to the plain context's
    own = tab.rows(P, N0, 1, seed=1)
    twin.case(lambda c: tab.set(c, own, N0, 1), twin.launch, name=tab.name + " shared -> per instance", recapture=True)
    twin.case(lambda c: tab.set(c, shared, N0, 0), twin.launch, name=tab.name + " per instance -> shared", recapture=True)
    assert (twin.plain.status() == 0).all()
