"""TaskSpace3DCost / CoMCost evaluated by rtoc_contact_eval_kkt on the device (csrc/task_space_cost.hpp), against the numpy
restatement of tests/task_cost_restatement.py (itself pinned to oracle/rtoc_oracle_rbd.c by test_task_space_cost_host.py):
the terms the kernel adds to lq, Qqq, hx, h and the cost value, on grids with lift, impact, switching and terminal points,
nothing else touched, nothing written where no term is active; off means unchanged; graphs and clones; per-instance STO times."""
import ctypes as C

import numpy as np
import pytest

from robotoc_amd import capi, costs, problems, robot_model as rm
from robotoc_amd.grid import anymal_trot_sequence, contact_masks, discretize, jump_sto_sequence
from robotoc_amd.types import BUF_CDD, BUF_KKT, BUF_SOL, GRID_IMPACT, Records, anymal_dims, icub_dims

import task_cost_restatement as tr

Q_STAND = np.array([0, 0, 0.4792, 0, 0, 0, 1, -0.1, 0.7, -1.0, -0.1, -0.7, 1.0, 0.1, 0.7, -1.0, 0.1, -0.7, 1.0])


def _context(m, dims, grids, masks, batch, seed, q_center=None):
    n, nv, nq = len(grids), m.nv, m.nq
    ctx = capi.Context(dims, n, batch, 0)
    ctx.set_grid(grids)
    ctx.set_robot_model(m)
    ctx.set_contact_schedule(np.asarray(masks, dtype=np.uint32))
    q_ref = np.zeros(nq)
    q_ref[6] = 1.0
    ctx.set_configuration_cost(q_ref, np.zeros(nv), np.zeros(m.nu), np.full(nv, 1.0), np.full(nv, 0.1), np.full(nv, 1e-3),
                               np.full(m.nu, 1e-3), np.full(nv, 2.0), np.full(nv, 0.2), np.full(nv, 3.0), np.full(nv, 0.3),
                               np.full(nv, 1e-2))
    rng = np.random.default_rng(seed)
    x0 = np.zeros((batch, nq + nv))
    S = Records(ctx.L, "sol")
    sol = S.zeros(batch, n)
    for b in range(batch):
        x0[b, :nq] = rm.random_configuration(m, rng, 0.3)[0]
        for i in range(n):
            q, v, a = rm.random_configuration(m, rng, 0.3)
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
    ctx.set_initial_state(x0)
    ctx.upload(BUF_SOL, sol)
    return ctx, sol, S


def _eval(ctx):
    ctx.contact_eval_kkt()
    kkt, cdd = ctx.download_records(BUF_KKT, "kkt"), ctx.download_records(BUF_CDD, "cdd")
    cost, _ = ctx.contact_eval_ocp()
    return kkt, cdd, cost


def _kind(grids, i):
    return "terminal" if i == len(grids) - 1 else ("impact" if grids[i].type == GRID_IMPACT else "stage")


def _check_terms(m, grids, times, sol, S, ctx, structs, per_instance=False, require_inactive=True):
    """records with the terms minus records without them == the restatement; everything else bit for bit"""
    base = _eval(ctx)
    ctx.set_task_costs(structs, per_instance=per_instance)
    kkt, cdd, cost = _eval(ctx)
    again = _eval(ctx)
    assert np.array_equal(kkt, again[0]) and np.array_equal(cdd, again[1]) and np.array_equal(cost, again[2])   # deterministic
    assert np.array_equal(cdd, base[1])
    K = Records(ctx.L, "kkt")
    nv, nq = m.nv, m.nq
    batch, n = kkt.shape[:2]
    mask = np.ones(K.stride, dtype=bool)   # the words the terms may change
    o_l, o_h, o_q, o_s = K.offset("lx"), K.offset("hx"), K.offset("Qxx"), K.offset("scal")
    mask[o_l:o_l + nv] = mask[o_h:o_h + nv] = False
    mask[o_s + 2] = False
    for c in range(nv):
        mask[o_q + c * 2 * nv:o_q + c * 2 * nv + nv] = False
    n_on = n_off = 0
    worst = 0.0
    for b in range(batch):
        dcost = 0.0
        terms = structs[b] if per_instance else structs
        for i in range(n):
            kind = _kind(grids, i)
            scale = 1.0 if kind != "stage" else grids[i].dt
            t = times[b][i] if np.ndim(times) == 2 else times[i]
            q = S.f(sol[b, i], "q")[:nq]
            lq, Q, hx, h, c, on = tr.stage_terms(m, q, [s if isinstance(s, costs.TaskCost) else s.to_struct() for s in terms], t, kind, scale)
            assert np.array_equal(kkt[b, i][mask], base[0][b, i][mask])
            if not on:
                n_off += 1
                assert np.array_equal(kkt[b, i], base[0][b, i]), (b, i)
                continue
            n_on += 1
            dcost += c
            pairs = [(K.f(kkt[b, i], "lx")[:nv] - K.f(base[0][b, i], "lx")[:nv], lq, K.f(kkt[b, i], "lx")[:nv]),
                     (K.f(kkt[b, i], "Qxx")[:nv, :nv] - K.f(base[0][b, i], "Qxx")[:nv, :nv], Q, K.f(kkt[b, i], "Qxx")[:nv, :nv])]
            if kind == "stage":
                pairs += [(K.f(kkt[b, i], "hx")[:nv] - K.f(base[0][b, i], "hx")[:nv], hx, K.f(kkt[b, i], "hx")[:nv]),
                          (np.array([K.f(kkt[b, i], "scal")[2] - K.f(base[0][b, i], "scal")[2]]), np.array([h]), np.array([K.f(kkt[b, i], "scal")[2]]))]
            for d, r, full in pairs:
                err = np.abs(d - r).max() / max(1.0, np.abs(r).max(), np.abs(full).max())
                worst = max(worst, err)
                assert err < 1e-12, (b, i, kind, err)
        assert abs((cost[b] - base[2][b]) - dcost) <= 1e-12 * max(1.0, abs(cost[b]), dcost), (b, cost[b] - base[2][b], dcost)
    print("grid points with active terms: %d, without: %d, worst relative difference %.1e" % (n_on, n_off, worst))
    assert n_on > 0 and (n_off > 0 or not require_inactive)
    return base


def _trot_setup(batch=8, seed=3):
    m = rm.load_named("anymal")
    dims = anymal_dims()
    cs = anymal_trot_sequence(t0=0.11, swing=0.2, double_support=0.1, cycles=1)
    grids, times = discretize(40, 0.8, 0.0, cs, times=True)
    assert [bytes(g) for g in grids] == [bytes(g) for g in problems.config_anymal_trot()[1]]   # BASELINE configs[1]'s grid
    masks = contact_masks(grids, [0b1111, 0b1001, 0b1111, 0b0110, 0b1111], [0b0110, 0b1001])
    ctx, sol, S = _context(m, dims, grids, masks, batch, seed, q_center=Q_STAND)
    ctx.set_grid_times(times)
    return m, grids, times, ctx, sol, S


def _trot_terms(m):
    step = np.array([0.15, 0.0, 0.0])
    terms = []
    for k, (name, t0, half) in enumerate((("LF_FOOT", 0.31, False), ("LH_FOOT", 0.11, True), ("RF_FOOT", 0.11, True), ("RH_FOOT", 0.31, False))):
        ref = costs.PeriodicSwingFootRef(tr.frame_position(m, Q_STAND, m.contact_parent[k], m.contact_p[k][:]), step, 0.1, t0, 0.2, 0.2, half)
        c = costs.TaskSpace3DCost("anymal", name, ref)
        c.set_weight([1e3 * (k + 1), 2e3, 3e3])
        c.set_weight_terminal([5e2, 0.0, 7e2 + k])
        c.set_weight_impact([11.0, 12.0 + k, 13.0])
        terms.append(c)
    cc = costs.CoMCost("anymal", costs.PeriodicCoMRef(tr.com(m, Q_STAND), 0.5 * step / 0.2, 0.11, 0.2, 0.1, True))
    cc.set_weight([1e4, 2e4, 3e4])
    cc.set_weight_terminal([1e2, 1e2, 1e2])
    cc.set_weight_impact([7.0, 8.0, 9.0])
    return terms + [cc]


@pytest.mark.gpu
def test_anymal_trot_terms_match_the_restatement():
    m, grids, times, ctx, sol, S = _trot_setup()
    _check_terms(m, grids, times, sol, S, ctx, _trot_terms(m))


@pytest.mark.gpu
def test_icub_soles_com_and_a_hand_match_the_restatement():
    m = rm.load_named("icub")
    dims = icub_dims(35)
    cs = jump_sto_sequence(ground_time=0.21, flying_time=0.2, nf=12)
    for e in cs.events:
        e.sto = False
    grids, times = discretize(30, 0.6, 0.0, cs, times=True)
    masks = contact_masks(grids, [0b11, 0b00, 0b11], [0b11])
    ctx, sol, S = _context(m, dims, grids, masks, 4, 7)
    ctx.set_grid_times(times)
    q0 = np.zeros(m.nq)
    q0[6] = 1.0
    terms = []
    for k, name in enumerate(("l_sole", "r_sole")):
        f = costs.TaskSpace3DCost("icub", name, costs.PeriodicSwingFootRef(tr.frame_position(m, q0, m.contact_parent[k], m.contact_p[k][:]),
                                                                           [0.1, 0.0, 0.0], 0.05, 0.05 + 0.1 * k, 0.15, 0.1, k == 0))
        f.set_weight([100.0, 200.0, 300.0 + k])
        f.set_weight_impact([1.0, 2.0, 3.0])
        f.set_weight_terminal([4.0, 5.0, 6.0])
        terms.append(f)
    hand = costs.TaskSpace3DCost("icub", ("l_wrist_yaw", [0.0, 0.02, 0.08]), np.array([0.2, 0.3, 0.5]))
    hand.set_weight([50.0, 60.0, 70.0])
    hand.set_weight_terminal([80.0, 0.0, 90.0])
    com = costs.CoMCost("icub", costs.PeriodicCoMRef([0.0, 0.0, 0.5], [0.2, 0.0, 0.0], 0.1, 0.2, 0.1, False))
    com.set_weight([1e3, 1e3, 2e3])
    com.set_weight_impact([10.0, 10.0, 10.0])
    # the hand's constant reference is active on every grid point with a weight (all but impact ones)
    _check_terms(m, grids, times, sol, S, ctx, terms + [hand, com], require_inactive=False)


def _clone(ctx):
    h = C.c_void_p()
    assert capi.lib().rtoc_clone(ctx._h, C.byref(h)) == 0
    n = object.__new__(capi.Context)
    n.__dict__.update(ctx.__dict__)
    n._h = h.value
    return n


@pytest.mark.gpu
def test_off_means_unchanged_graphs_and_clones():
    m, grids, times, ctx, sol, S = _trot_setup(batch=4, seed=5)
    terms = _trot_terms(m)
    plain = _eval(ctx)
    ctx.set_task_costs(terms)
    on = _eval(ctx)
    cl = _clone(ctx)
    cl_rec = _eval(cl)
    assert all(np.array_equal(x, y) for x, y in zip(on, cl_rec))
    ctx.set_task_costs(None)
    off = _eval(ctx)
    assert all(np.array_equal(x, y) for x, y in zip(plain, off))
    assert not np.array_equal(on[0], plain[0])
    cl.close()
    # graphed iterations: terms set after two replayed iterations take effect on the next one
    ref_ctx = _trot_setup(batch=4, seed=5)[3]
    for c in (ctx, ref_ctx):
        c.upload(BUF_SOL, sol)
    ctx.set_graph(True)
    for it in range(3):
        e1 = ctx.contact_update_solution()
        e2 = ref_ctx.contact_update_solution()
        assert np.array_equal(e1, e2), it
        if it == 1:
            ctx.set_task_costs(terms)
            ref_ctx.set_task_costs(terms)
    assert np.array_equal(ctx.download_records(BUF_SOL, "sol"), ref_ctx.download_records(BUF_SOL, "sol"))
    plain_ctx = _trot_setup(batch=4, seed=5)[3]
    plain_ctx.upload(BUF_SOL, sol)
    for it in range(3):
        plain_ctx.contact_update_solution()
    assert not np.array_equal(ctx.download_records(BUF_SOL, "sol"), plain_ctx.download_records(BUF_SOL, "sol"))


@pytest.mark.gpu
def test_clone_takes_more_terms_than_its_source_had():
    """rtoc_clone copies the term table with the capacity it was allocated with (RTOC_MAX_TASK_COSTS per instance), not the
    part in use when the clone is taken: a clone of a context with one shared term takes all five terms, and five terms per
    instance, and evaluates them like a fresh context that was given the same terms directly"""
    batch = 4
    m, grids, times, ctx, sol, S = _trot_setup(batch=batch, seed=5)
    ctx.set_task_costs(_trot_terms(m)[:1])
    one = _eval(ctx)
    cl = _clone(ctx)
    fresh = _trot_setup(batch=batch, seed=5)[3]
    per = []
    for b in range(batch):
        inst = _trot_terms(m)
        for k, t in enumerate(inst):
            t.set_weight([1e3 * (b + 1), 2e3 + k, 3e3])
        per.append(inst)
    seen = [one]
    for larger, per_instance in ((_trot_terms(m), False), (per, True)):
        cl.set_task_costs(larger, per_instance=per_instance)
        fresh.set_task_costs(larger, per_instance=per_instance)
        cl_rec, fresh_rec = _eval(cl), _eval(fresh)
        assert all(np.array_equal(x, y) for x, y in zip(cl_rec, fresh_rec)), per_instance
        assert all(not np.array_equal(cl_rec[0], r[0]) for r in seen)   # the larger set took effect
        seen.append(cl_rec)
    # the source keeps its one term
    assert all(np.array_equal(x, y) for x, y in zip(one, _eval(ctx)))
    for c in (cl, fresh, ctx):
        c.close()


def _correct_time_steps(grids, t, T, ts):
    """TimeDiscretization::correctTimeSteps (time_discretization.cpp:186-222), grid times only"""
    N = len(grids) - 1
    out = np.zeros(N + 1)
    prev_stage, prev_t, e, i = 0, t, 0, 0
    while i < N:
        if grids[i].type == GRID_IMPACT:
            d = (ts[e] - prev_t) / grids[i - 1].num_grids_in_phase
            for j in range(prev_stage, i):
                out[j] = prev_t + (j - prev_stage) * d
            out[i] = ts[e]
            prev_t, prev_stage, e = ts[e], i + 1, e + 1
            i += 1
        elif grids[i + 1].type == 2:   # GRID_LIFT
            d = (ts[e] - prev_t) / grids[i].num_grids_in_phase
            for j in range(prev_stage, i + 1):
                out[j] = prev_t + (j - prev_stage) * d
            prev_t, prev_stage, e = ts[e], i + 1, e + 1
        elif grids[i + 1].type == 3:   # GRID_TERMINAL
            d = (t + T - prev_t) / grids[i].num_grids_in_phase
            for j in range(prev_stage, i + 1):
                out[j] = prev_t + (j - prev_stage) * d
        i += 1
    out[N] = t + T
    return out


@pytest.mark.gpu
def test_sto_grid_times_are_per_instance():
    from robotoc_amd.types import GRID_LIFT, GRID_TERMINAL
    assert (GRID_LIFT, GRID_TERMINAL) == (2, 3)
    m = rm.load_named("anymal")
    dims = anymal_dims()
    cs = jump_sto_sequence(ground_time=0.31, flying_time=0.2, nf=12)
    grids = discretize(40, 0.8, 0.0, cs, phase_based=True)
    masks = contact_masks(grids, [0b1111, 0b0000, 0b1111], [0b1111])
    batch = 2
    ctx, sol, S = _context(m, dims, grids, masks, batch, 11, q_center=Q_STAND)
    ts = np.array([[0.31, 0.51], [0.29, 0.53]])
    ctx.sto_set_problem(0.0, 0.8, ts, [0.02, 0.02, 0.02])
    times = ctx.grid_times()
    for b in range(batch):
        want = _correct_time_steps(grids, 0.0, 0.8, ts[b])
        assert np.array_equal(times[b], want), (b, np.abs(times[b] - want).max(), times[b], want)
    assert not np.array_equal(times[0], times[1])
    per = []
    for b in range(batch):
        c = costs.CoMCost("anymal", costs.PeriodicCoMRef(tr.com(m, Q_STAND) + [0.0, 0.0, 0.01 * b], [0.3, 0.0, 0.0], 0.2, 0.15, 0.1, b == 1))
        c.set_weight([1e3, 1e3, 1e3])
        c.set_weight_impact([5.0, 5.0, 5.0])
        c.set_weight_terminal([2.0, 2.0, 2.0])
        per.append([c])
    # instance by instance with its own grid times and time steps
    dts = ctx.sto_time_steps()
    assert not np.array_equal(dts[0], dts[1])
    base = _eval(ctx)
    ctx.set_task_costs(per, per_instance=True)
    kkt, cdd, cost = _eval(ctx)
    K = Records(ctx.L, "kkt")
    nv, nq = m.nv, m.nq
    n_on = 0

    def close(f, r):
        full = K.f(kkt[b, i], f)
        d = full - K.f(base[0][b, i], f)
        if f == "Qxx":
            full, d = full[:nv, :nv], d[:nv, :nv]
        elif f == "scal":
            full, d = full[2:3], d[2:3]
        else:
            full, d = full[:nv], d[:nv]
        assert np.abs(d - r).max() <= 1e-12 * max(1.0, np.abs(r).max(), np.abs(full).max()), (f, b, i)

    for b in range(batch):
        dcost = 0.0
        for i in range(len(grids)):
            kind = _kind(grids, i)
            scale = 1.0 if kind != "stage" else dts[b][i]
            lq, Q, hx, h, cval, on = tr.stage_terms(m, S.f(sol[b, i], "q")[:nq], [per[b][0].to_struct()], times[b][i], kind, scale)
            if not on:
                assert np.array_equal(kkt[b, i], base[0][b, i])
                continue
            n_on += 1
            dcost += cval
            close("lx", lq)
            close("Qxx", Q)
            if kind == "stage":
                close("hx", hx)
                close("scal", np.array([h]))
        assert abs((cost[b] - base[2][b]) - dcost) <= 1e-12 * max(1.0, abs(cost[b]), dcost), b
    assert n_on > 0
