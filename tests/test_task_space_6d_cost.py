"""TaskSpace6DCost and per-grid-point reference tables on the device (csrc/task_space_cost.hpp), on both evalKKT paths, against
the numpy restatement of tests/task_cost_6d_restatement.py (pinned on the CPU by test_task_space_6d_cost_host.py): the
measure of test_task_space_cost.py::_check_terms -- records with the terms minus records without them, relative to
max(1, |reference|, |full record|) -- every other word of the records bit for bit equal, two evaluations bit-identical.

Bound 1e-11: the 3D terms' 1e-12 times 10 for the conditioning of acos in log3 at rotation errors of 0.1 rad and more
(d theta <= 3 u / sin theta, about 30 u at 0.1 rad); the tests keep their rotation errors inside [0.1, pi - 0.1]."""
import ctypes as C

import numpy as np
import pytest

from helpers import compare_direction, compare_riccati
from robotoc_amd import capi, costs, problems as pr, robot_model as rm
from robotoc_amd.grid import ContactSequence, Event, contact_masks, discretize, jump_sto_sequence, uniform_grid
from robotoc_amd.types import BUF_CDD, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, GRID_IMPACT, Records, anymal_dims, icub_dims, iiwa14_dims

import task_cost_6d_restatement as t6
import task_cost_restatement as tr

BOUND = 1e-11
BAD_ARG, NOT_READY = -1, -5
Q_STAND = np.array([0, 0, 0.4792, 0, 0, 0, 1, -0.1, 0.7, -1.0, -0.1, -0.7, 1.0, 0.1, 0.7, -1.0, 0.1, -0.7, 1.0])


def _structs(terms):
    return [s if isinstance(s, costs.TaskCost) else s.to_struct() for s in terms]


def _kind(grids, i, unconstr):
    if i == len(grids) - 1:
        return "terminal"
    return "impact" if (not unconstr and grids[i].type == GRID_IMPACT) else "stage"


def _angles_ok(m, q, structs, entries):
    """the rotation errors of the active 6D terms stay where the bound was derived"""
    for k, s in enumerate(structs):
        if s.kind != costs.TASK_FRAME_6D:
            continue
        e = None if entries is None else entries.get(k)
        if s.ref_kind == costs.REF_TABLE and not e.active:
            continue
        R_ref, p_ref = (e.R, e.p) if s.ref_kind == costs.REF_TABLE else (s.ref_R, s.x0)
        XR, _ = t6.diff(m, q, s.frame_parent, s.frame_p[:], s.frame_R[:], np.array(R_ref[:]), np.array(p_ref[:]))
        th = np.linalg.norm(t6.log3(XR))
        assert 0.1 <= th <= np.pi - 0.1, (k, th)


def _check(m, grids, times, sol, S, ctx, evaluate, terms, tables=None, per_instance=False, unconstr_dt=None, require_inactive=False, label=""):
    """`evaluate(ctx)` -> (kkt, cdd, cost); tables = {term: entries} shared by the batch, or a list of such dicts per instance.
    Records with the terms minus records without == the restatement; everything else bit for bit."""
    unconstr = unconstr_dt is not None
    base = evaluate(ctx)
    ctx.set_task_costs(terms, per_instance=per_instance)
    if tables is not None:
        for k in (tables[0] if per_instance else tables):
            ctx.set_task_ref_table(k, [t[k] for t in tables] if per_instance else tables[k], per_instance=per_instance)
    kkt, cdd, cost = evaluate(ctx)
    again = evaluate(ctx)
    assert np.array_equal(kkt, again[0]) and np.array_equal(cdd, again[1]) and np.array_equal(cost, again[2])   # deterministic
    assert np.array_equal(cdd, base[1])
    K = Records(ctx.L, "kkt")
    nv, nq = m.nv, m.nq
    batch, n = kkt.shape[:2]
    mask = np.ones(K.stride, dtype=bool)   # the words the terms may not change
    o_l, o_h, o_q, o_s = K.offset("lx"), K.offset("hx"), K.offset("Qxx"), K.offset("scal")
    mask[o_l:o_l + nv] = False
    if not unconstr:   # the STO sensitivities hx, h: the contact path's only
        mask[o_h:o_h + nv] = False
        mask[o_s + 2] = False
    for c in range(nv):
        mask[o_q + c * 2 * nv:o_q + c * 2 * nv + nv] = False
    n_on = n_off = 0
    worst = 0.0
    for b in range(batch):
        dcost = 0.0
        structs = _structs(terms[b] if per_instance else terms)
        tab = None if tables is None else (tables[b] if per_instance else tables)
        for i in range(n):
            kind = _kind(grids, i, unconstr)
            scale = 1.0 if kind != "stage" else (unconstr_dt if unconstr else grids[i].dt)
            q = S.f(sol[b, i], "q")[:nq]
            entries = None if tab is None else {k: tab[k][i] for k in tab}
            lq, Q, hx, h, c, on = t6.stage_terms(m, q, structs, times[i], kind, scale, entries)
            assert np.array_equal(kkt[b, i][mask], base[0][b, i][mask]), (b, i)
            if not on:
                n_off += 1
                assert np.array_equal(kkt[b, i], base[0][b, i]), (b, i)
                continue
            _angles_ok(m, q, [s for s in structs], entries)
            n_on += 1
            dcost += c
            full_l, full_Q = K.f(kkt[b, i], "lx")[:nv], K.f(kkt[b, i], "Qxx")[:nv, :nv]
            pairs = [(full_l - K.f(base[0][b, i], "lx")[:nv], lq, full_l), (full_Q - K.f(base[0][b, i], "Qxx")[:nv, :nv], Q, full_Q)]
            if kind == "stage" and not unconstr:
                pairs += [(K.f(kkt[b, i], "hx")[:nv] - K.f(base[0][b, i], "hx")[:nv], hx, K.f(kkt[b, i], "hx")[:nv]),
                          (np.array([K.f(kkt[b, i], "scal")[2] - K.f(base[0][b, i], "scal")[2]]), np.array([h]), np.array([K.f(kkt[b, i], "scal")[2]]))]
            for d, r, full in pairs:
                err = np.abs(d - r).max() / max(1.0, np.abs(r).max(), np.abs(full).max())
                worst = max(worst, err)
                assert err < BOUND, (b, i, kind, err)
        err = abs((cost[b] - base[2][b]) - dcost) / max(1.0, abs(cost[b]), dcost)
        worst = max(worst, err)
        assert err < BOUND, (b, cost[b] - base[2][b], dcost)
    print("%s: grid points with active terms %d, without %d, worst relative difference %.1e (bound %.0e)" % (label, n_on, n_off, worst, BOUND))
    assert n_on > 0 and (n_off > 0 or not require_inactive)
    return base, (kkt, cdd, cost)


# ---- the unconstrained path: iiwa14 ----
EE = ("iiwa_joint_7", [0.0, 0.0, 0.045], tr._rot([0.0, 0.6, 0.8], 0.7))   # an end-effector frame with a rotation


def _iiwa_data(batch, N, seed, dt=0.05):
    """the problem without a device: model, grid, times, cost, initial states, a random iterate around q_c"""
    m = rm.load_named("iiwa14")
    dims = iiwa14_dims()
    grids = uniform_grid(N, dt)
    n, nv = len(grids), m.nv
    rng = np.random.default_rng(seed)
    cost = dict(q_ref=rng.uniform(-0.8, 0.8, nv), v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0),
                v_weight=np.full(nv, 0.1), a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.001),
                q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 0.1))
    x0 = np.concatenate([rng.uniform(-0.5, 0.5, (batch, nv)), np.zeros((batch, nv))], axis=1)
    S = Records(capi.layout_for(dims), "sol")
    sol = S.zeros(batch, n)
    q_c = rng.uniform(-0.8, 0.8, nv)
    for f in ("v", "a", "u", "lmd", "gmm", "beta"):
        S.f(sol, f)[...] = rng.uniform(-1, 1, S.f(sol, f).shape)
    S.f(sol, "q")[..., :nv] = q_c + rng.uniform(-0.3, 0.3, (batch, n, nv))
    times = 0.3 + dt * np.arange(n)
    return m, dims, grids, times, cost, x0, sol, S, q_c, rng


def _iiwa(batch, N, seed, dt=0.05, line_search=True):
    m, dims, grids, times, cost, x0, sol, S, q_c, rng = _iiwa_data(batch, N, seed, dt)
    ctx = capi.Context(dims, len(grids), batch, 0)
    ctx.set_grid(grids)
    ctx.set_robot_model(m)
    ctx.set_configuration_cost(**cost)
    ctx.set_initial_state(x0)
    ctx.upload(BUF_SOL, sol)
    ctx.set_grid_times(times)
    if line_search:
        ctx.set_line_search(True)
    return m, grids, times, ctx, sol, S, q_c, rng, dt


def _eval_unconstr(dt):
    def run(ctx):
        ctx.unconstr_eval_kkt(dt)
        kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
        cost, _ = ctx.contact_eval_ocp()   # the cost values the line search reads (cost_out)
        return kkt, cdd, cost
    return run


def _const_6d(robot, frame, m, q_c, rng, lo=0.8, hi=1.4):
    """a 6D term whose constant reference is the frame's placement at q_c moved by a rotation of [lo, hi] rad"""
    c = costs.TaskSpace6DCost(robot, frame)
    R_ref, p_ref = t6.reference_with_error(m, q_c, c.frame_parent, c.frame_p, c.frame_R, rng, lo, hi, 0.3)
    c.set_const_ref(p_ref, R_ref)
    return c


class _TableRef(costs.TaskSpace6DRefBase):
    """a user's reference object: placements and active flags given per grid point"""

    def __init__(self, R, p, active):
        self.R, self.p, self.active = R, p, active

    def update_ref(self, g):
        return self.R[g.stage], self.p[g.stage]

    def is_active(self, g):
        return bool(self.active[g.stage])


class _PointRef:
    def __init__(self, p, active):
        self.p, self.active = p, active

    def update_ref(self, g):
        return self.p[g.stage]

    def is_active(self, g):
        return bool(self.active[g.stage])


def _table_6d(m, cost, qs, rng, active):
    """a reference object for `cost` whose placement at grid point i is the frame's at qs[i] moved by a rotation of [0.1, 2.5] rad"""
    refs = [t6.reference_with_error(m, q, cost.frame_parent, cost.frame_p, cost.frame_R, rng) for q in qs]
    return _TableRef([r[0] for r in refs], [r[1] for r in refs], active)


def _iiwa_terms(m, sol, S, b, q_c, rng, infos, with_const=True):
    """the terms of instance b and their tables: a 6D term with a constant reference, a 6D term with a table reference that is
    inactive on grid points 1 and 3, a 3D term on the same frame with a table reference inactive there too"""
    n, nv = sol.shape[1], m.nv
    qs = [S.f(sol[b, i], "q")[:nv] for i in range(n)]
    active = [1, 0, 1, 0, 1][:n]
    t1 = costs.TaskSpace6DCost("iiwa14", EE)
    t1.set_ref(_table_6d(m, t1, qs, rng, active))
    t1.set_weight([10.0, 20.0, 30.0], [1.0, 2.0, 3.0])
    t1.set_weight_terminal([5.0, 6.0, 7.0], [0.5, 0.0, 0.7])
    t2 = costs.TaskSpace3DCost("iiwa14", (EE[0], EE[1]), _PointRef([tr.frame_position(m, q, 6, EE[1]) + rng.uniform(-0.2, 0.2, 3) for q in qs], active))
    t2.set_weight([100.0, 0.0, 300.0])
    t2.set_weight_terminal([40.0, 50.0, 60.0])
    terms = [t1, t2]
    if with_const:
        t0 = _const_6d("iiwa14", "iiwa_link_ee_kuka", m, q_c, rng)
        t0.set_weight([10.0, 10.0, 10.0], [0.1, 0.2, 0.3])
        t0.set_weight_terminal([20.0, 30.0, 40.0], [1.0, 1.0, 2.0])
        terms = [t0] + terms
    return terms, {k: t.ref_table(infos) for k, t in enumerate(terms) if t.uses_table()}


@pytest.mark.gpu
def test_iiwa14_unconstrained_terms_match_the_restatement():
    batch, N = 3, 4
    m, grids, times, ctx, sol, S, q_c, rng, dt = _iiwa(batch, N, seed=1)
    infos = costs.grid_infos(times, [g.dt for g in grids])
    # the table terms alone: where their references are inactive the records are untouched
    per = [_iiwa_terms(m, sol, S, b, q_c, rng, infos, with_const=False) for b in range(batch)]
    _check(m, grids, times, sol, S, ctx, _eval_unconstr(dt), [p[0] for p in per], [p[1] for p in per], per_instance=True, unconstr_dt=dt,
           require_inactive=True, label="iiwa14 unconstrained, table terms")
    ctx.set_task_costs(None)
    # all three, per instance
    per = [_iiwa_terms(m, sol, S, b, q_c, rng, infos) for b in range(batch)]
    _check(m, grids, times, sol, S, ctx, _eval_unconstr(dt), [p[0] for p in per], [p[1] for p in per], per_instance=True, unconstr_dt=dt,
           label="iiwa14 unconstrained, const + table terms")
    ctx.close()


# ---- the contact path ----
def _contact_data(m, dims, grids, batch, seed, q_center=None):
    n, nv, nq = len(grids), m.nv, m.nq
    rng = np.random.default_rng(seed)
    x0 = np.zeros((batch, nq + nv))
    S = Records(capi.layout_for(dims), "sol")
    sol = S.zeros(batch, n)
    for b in range(batch):
        x0[b, :nq] = rm.random_configuration(m, rng, 0.3)[0]
        for i in range(n):
            q, v, a = rm.random_configuration(m, rng, 0.3)
            # the base within 0.4 rad of upright: the constant references below then keep their rotation errors off 0 and pi
            axis, half = rng.normal(size=3), 0.5 * rng.uniform(-0.4, 0.4)
            q[3:7] = np.concatenate([np.sin(half) * axis / np.linalg.norm(axis), [np.cos(half)]])
            if q_center is not None:
                q[7:] += q_center[7:]
                q[2] += q_center[2]
            S.f(sol[b, i], "q")[:nq] = q
            S.f(sol[b, i], "v")[...] = v
            S.f(sol[b, i], "a")[...] = a
            S.f(sol[b, i], "u")[...] = 0.1 * rng.uniform(-1, 1, m.nu)
            S.f(sol[b, i], "f")[...] = rng.uniform(-1, 1, dims.nf_max)
            S.f(sol[b, i], "lmd")[...] = rng.uniform(-1, 1, nv)
            S.f(sol[b, i], "gmm")[...] = rng.uniform(-1, 1, nv)
    return x0, sol, S, rng


def _contact_context(m, dims, grids, masks, times, x0, sol):
    n, nv, nq = len(grids), m.nv, m.nq
    ctx = capi.Context(dims, n, len(sol), 0)
    ctx.set_grid(grids)
    ctx.set_robot_model(m)
    ctx.set_contact_schedule(np.asarray(masks, dtype=np.uint32))
    q_ref = np.zeros(nq)
    q_ref[6] = 1.0
    ctx.set_configuration_cost(q_ref, np.zeros(nv), np.zeros(m.nu), np.full(nv, 1.0), np.full(nv, 0.1), np.full(nv, 1e-3),
                               np.full(m.nu, 1e-3), np.full(nv, 2.0), np.full(nv, 0.2), np.full(nv, 3.0), np.full(nv, 0.3),
                               np.full(nv, 1e-2))
    ctx.set_initial_state(x0)
    ctx.upload(BUF_SOL, sol)
    ctx.set_grid_times(times)
    return ctx


def _eval_contact(ctx):
    ctx.contact_eval_kkt()
    kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
    cost, _ = ctx.contact_eval_ocp()
    return kkt, cdd, cost


def _anymal_case():
    m = rm.load_named("anymal")
    dims = anymal_dims()
    cs = ContactSequence([12, 6, 12], [Event("lift", 0.11), Event("impact", 0.33, impact_dimf=6)])
    grids, times = discretize(12, 0.6, 0.0, cs, times=True)
    kinds = {_kind(grids, i, False) for i in range(len(grids))}
    assert kinds == {"stage", "impact", "terminal"} and any(g.switching_constraint for g in grids) and len(grids) == 16
    masks = contact_masks(grids, [0b1111, 0b1001, 0b1111], [0b0110])
    x0, sol, S, rng = _contact_data(m, dims, grids, 2, 21, q_center=Q_STAND)
    q_c = Q_STAND.copy()
    # the base rotates by up to 0.3 rad per axis around the identity and the reference by [0.8, 1.4]: errors stay in [0.1, pi - 0.1]
    base = _const_6d("anymal", (0, [0.1, 0.0, 0.05], tr._rot([1.0, 0.0, 0.0], 0.5)), m, q_c, rng)
    base.set_weight([100.0, 200.0, 300.0], [10.0, 20.0, 30.0])
    base.set_weight_impact([1.0, 2.0, 3.0], [4.0, 5.0, 6.0])
    shank = _const_6d("anymal", ("LF_KFE", [0.02, -0.03, -0.2], tr._rot([0.0, 0.6, 0.8], 1.1)), m, q_c, rng)
    shank.set_weight([50.0, 0.0, 70.0], [0.0, 8.0, 9.0])
    shank.set_weight_terminal([11.0, 12.0, 13.0], [14.0, 15.0, 16.0])
    assert not np.any(base.weight_terminal) and not np.any(shank.weight_impact)   # off on those kinds
    return m, dims, grids, times, masks, x0, sol, S, [base, shank]


@pytest.mark.gpu
def test_anymal_contact_path_terms_match_the_restatement():
    """stage, lift, impact, switching and terminal grid points; distinct weights per kind; the shank term has no impact weight
    at all, the base term none on the terminal grid: each is off there"""
    m, dims, grids, times, masks, x0, sol, S, terms = _anymal_case()
    ctx = _contact_context(m, dims, grids, masks, times, x0, sol)
    _check(m, grids, times, sol, S, ctx, _eval_contact, terms, label="anymal contact path")
    ctx.close()


def _icub_case():
    m = rm.load_named("icub")
    dims = icub_dims(35)
    cs = jump_sto_sequence(ground_time=0.21, flying_time=0.2, nf=12)
    for e in cs.events:
        e.sto = False
    grids, times = discretize(6, 0.6, 0.0, cs, times=True)
    masks = contact_masks(grids, [0b11, 0b00, 0b11], [0b11])
    x0, sol, S, rng = _contact_data(m, dims, grids, 2, 7)
    q0 = np.zeros(m.nq)
    q0[6] = 1.0
    hand = _const_6d("icub", ("l_wrist_yaw", [0.0, 0.02, 0.08], tr._rot([0.6, 0.0, 0.8], 0.9)), m, q0, rng, 1.2, 1.5)
    hand.set_weight([50.0, 60.0, 70.0], [5.0, 6.0, 7.0])
    hand.set_weight_terminal([80.0, 0.0, 90.0], [1.0, 2.0, 0.0])
    hand.set_weight_impact([3.0, 4.0, 5.0], [0.3, 0.4, 0.5])
    return m, dims, grids, times, masks, x0, sol, S, [hand]


@pytest.mark.gpu
def test_icub_hand_term_one_grid_point_per_wave():
    """nv = 35: the one-grid-point-per-wave instantiation, an odd nv in the row-pair tail"""
    m, dims, grids, times, masks, x0, sol, S, terms = _icub_case()
    ctx = _contact_context(m, dims, grids, masks, times, x0, sol)
    _check(m, grids, times, sol, S, ctx, _eval_contact, terms, label="icub nv = 35")
    ctx.close()


def _clone(ctx):
    h = C.c_void_p()
    assert capi.lib().rtoc_clone(ctx._h, C.byref(h)) == 0
    n = object.__new__(capi.Context)
    n.__dict__.update(ctx.__dict__)
    n._h = h.value
    return n


@pytest.mark.gpu
def test_lifecycle_on_the_unconstrained_path():
    batch, N = 2, 4
    m, grids, times, ctx, sol, S, q_c, rng, dt = _iiwa(batch, N, seed=2)
    infos = costs.grid_infos(times, [g.dt for g in grids])
    terms, tables = _iiwa_terms(m, sol, S, 0, q_c, rng, infos)
    run = _eval_unconstr(dt)
    plain = run(ctx)
    ctx.set_task_costs(terms)
    # a table term without its table
    assert capi.lib().rtoc_unconstr_eval_kkt(ctx._h, dt) == NOT_READY
    ctx.set_task_ref_tables(terms, infos)
    on = run(ctx)
    assert not np.array_equal(on[0], plain[0])
    # a clone evaluates identically: it carries the terms, the grid times and the tables
    cl = _clone(ctx)
    assert all(np.array_equal(x, y) for x, y in zip(on, run(cl)))
    cl.close()
    # rtoc_set_grid forgets the tables as it forgets the grid times
    ctx.set_grid(grids)
    assert capi.lib().rtoc_unconstr_eval_kkt(ctx._h, dt) == NOT_READY
    ctx.set_grid_times(times)
    assert capi.lib().rtoc_unconstr_eval_kkt(ctx._h, dt) == NOT_READY
    ctx.set_task_ref_tables(terms, infos)
    assert all(np.array_equal(x, y) for x, y in zip(on, run(ctx)))
    # off means unchanged
    ctx.set_task_costs(None)
    assert all(np.array_equal(x, y) for x, y in zip(plain, run(ctx)))
    # iterations with RTOC_OPT_GRAPH on (what this path captures of its launch sequence must not go stale): terms set after two
    # iterations take effect on the next one
    ref_ctx, plain_ctx = _iiwa(batch, N, seed=2)[3], _iiwa(batch, N, seed=2)[3]
    ctx.set_graph(True)
    for it in range(4):
        e1, e2 = ctx.unconstr_update_solution(dt), ref_ctx.unconstr_update_solution(dt)
        plain_ctx.unconstr_update_solution(dt)
        assert np.array_equal(e1, e2), it
        if it == 1:
            for c in (ctx, ref_ctx):
                c.set_task_costs(terms)
                c.set_task_ref_tables(terms, infos)
    got = ctx.download_records(BUF_SOL, "sol")
    assert np.array_equal(got, ref_ctx.download_records(BUF_SOL, "sol"))
    assert not np.array_equal(got, plain_ctx.download_records(BUF_SOL, "sol"))
    for c in (ctx, ref_ctx, plain_ctx):
        c.close()


@pytest.mark.gpu
def test_api_errors():
    m, grids, times, ctx, sol, S, q_c, rng, dt = _iiwa(2, 4, seed=3)
    L = capi.lib()
    good = _const_6d("iiwa14", EE, m, q_c, rng)
    good.set_weight([1.0, 1.0, 1.0], [1.0, 1.0, 1.0])

    def rc(mutate):
        s = good.to_struct()
        mutate(s)
        arr = (costs.TaskCost * 1)(s)
        return L.rtoc_set_task_costs(ctx._h, C.cast(arr, C.c_void_p), 1, 0)

    assert rc(lambda s: None) == 0
    assert rc(lambda s: setattr(s, "kind", 3)) == BAD_ARG              # unknown kind
    assert rc(lambda s: setattr(s, "ref_kind", 4)) == BAD_ARG          # unknown ref_kind
    assert rc(lambda s: setattr(s, "ref_kind", costs.REF_PERIODIC_FOOT)) == BAD_ARG   # the periodic references are positions

    def neg(s):
        s.weight_angular_terminal[1] = -1e-3
    assert rc(neg) == BAD_ARG                                           # a negative weight in the new triples

    def nan(s):
        s.frame_R[4] = float("nan")
    assert rc(nan) == BAD_ARG                                           # a non-finite frame_R

    def inf(s):
        s.ref_R[0] = float("inf")
    assert rc(inf) == BAD_ARG
    assert rc(lambda s: setattr(s, "frame_parent", m.njoints)) == BAD_ARG
    # tables
    n = len(grids)
    tab = (costs.TaskRefEntry * (n + 1))()
    for e in tab:
        e.R[:] = np.eye(3).ravel()
    p = C.cast(tab, C.c_void_p)
    assert L.rtoc_set_task_ref_table(ctx._h, 0, p, n, 0) == 0
    assert L.rtoc_set_task_ref_table(ctx._h, 0, p, n - 1, 0) == BAD_ARG   # a table of the wrong length
    assert L.rtoc_set_task_ref_table(ctx._h, 0, p, n + 1, 0) == BAD_ARG
    assert L.rtoc_set_task_ref_table(ctx._h, costs.MAX_TASK_COSTS, p, n, 0) == BAD_ARG   # a term index out of range
    assert L.rtoc_set_task_ref_table(ctx._h, -1, p, n, 0) == BAD_ARG
    assert L.rtoc_set_task_ref_table(ctx._h, 0, None, n, 0) == BAD_ARG
    tab[2].p[1] = float("nan")
    assert L.rtoc_set_task_ref_table(ctx._h, 0, p, n, 0) == BAD_ARG
    assert L.rtoc_set_task_ref_table(None, 0, p, n, 0) == BAD_ARG
    # the constant-reference term still evaluates after the refused calls
    ctx.unconstr_eval_kkt(dt)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True])
def test_dense_qqq_through_the_unconstrained_recursion(oracle, dense):
    """the records of rtoc_unconstr_eval_kkt with a 6D term (a dense Qqq block) through the device's condensation and
    recursion and through the oracle's: the bound of test_gpu_parity.py::test_iiwa14_unconstr"""
    TOL = 1e-9
    batch, N = 3, 6
    m, grids, times, ctx, sol, S, q_c, rng, dt = _iiwa(batch, N, seed=4, line_search=False)
    term = _const_6d("iiwa14", EE, m, q_c, rng)
    term.set_weight([10.0, 10.0, 10.0], [1.0, 1.0, 1.0])
    term.set_weight_terminal([10.0, 10.0, 10.0], [1.0, 1.0, 1.0])
    ctx.set_unconstr_dense(dense)
    ctx.set_task_costs([term])
    ctx.unconstr_eval_kkt(dt)
    L, n, nv = ctx.L, len(grids), m.nv
    kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
    dx0 = ctx.download(BUF_DX0, (batch, 2 * nv))
    K = Records(L, "kkt")
    Qqq = K.f(kkt[0, 1], "Qxx")[:nv, :nv]
    assert np.abs(Qqq - np.diag(np.diag(Qqq))).max() > 1e-3   # the block is dense
    ctx.unconstr_condense()
    ctx.unconstr_backward(dt)
    ctx.unconstr_forward(dt)
    assert (ctx.status() == 0).all()
    ric, d = ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")
    ric_ref, d_ref = Records(L, "ric").zeros(batch, n), Records(L, "dir").zeros(batch, n)
    kkt_ref, cdd_ref = kkt.copy(), cdd.copy()
    oracle.unconstr_condense_batch(L, n, kkt_ref, cdd_ref)
    oracle.unconstr_sweep_batch(L, n, dt, kkt_ref, ric_ref, d_ref, dx0=dx0)
    worst = 0.0
    for b in range(batch):
        worst = max(worst, compare_riccati(L, grids, ric[b], ric_ref[b], TOL, "iiwa inst %d" % b))
        worst = max(worst, compare_direction(L, grids, d[b], d_ref[b], TOL, "iiwa inst %d" % b))
    print("dense Qqq through the unconstrained recursion (%s): worst rel err %.2e" % ("general kernels" if dense else "structured", worst))
    ctx.close()
