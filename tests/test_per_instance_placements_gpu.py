"""Per-instance contact placements (rtoc_set_contact_placements): every kernel that reads a placement reads the table of its own
instance.  The problems are those of tests/per_instance_placement_cases.py -- robots at different places, yawed differently, with
different touch-down footholds.  Two references, neither of them the code under test alone:
  * a batch-1 context per instance, given that instance's placements through rtoc_set_contact_schedule (the shared path).  Each
    record is produced by its own work item from the same values, so the criterion is bit-for-bit equality -- except for a buffer
    that differs between a batch and a batch-1 context WITHOUT per-instance placements (one shared set of footholds, measured on
    the commit before this feature): there it is the pin of tests/golden/per_instance_placements_pins.json, 10 x the largest such
    difference;
  * the CPU restatement (oracle.rbd_eval) with that instance's feet, for the [ID; C] rows, to the bound tests/test_rigid_body.py
    holds the same field to (1e-14)."""
import json
import os

import numpy as np
import pytest

import per_instance_placement_cases as cases
from helpers import check_parity
from robotoc_amd import capi
from robotoc_amd.types import GRID_IMPACT, Records

PINS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per_instance_placements_pins.json")))
IDC_BOUND = 1e-14   # tests/test_rigid_body.py: "ID, C values vs restatement"


def _assert_equal_to_singles(key, got, singles):
    worst = cases.worst_differences(got, singles)
    print(key, "largest difference to the batch-1 contexts:", worst)
    for name, w in worst.items():
        pin = PINS[key][name]["pin"]
        if pin == 0.0:
            for b, one in enumerate(singles):
                assert np.array_equal(got[name][b], one[name][0]), "%s of instance %d differs from its batch-1 context (worst %.3e)" % (name, b, w)
        else:
            check_parity("%s %s vs batch-1 contexts (pinned)" % (key, name), w, pin)


def _singles(P, fn):
    out = []
    for b in range(P.batch):
        c = cases.make_context(P, [b], shared_from=b)
        out.append(fn(P, c))
        c.close()
    return out


_SINGLES = {}


def singles_of(P, what):
    """the batch-1 reference of a case, computed once and never written"""
    if (P.name, what) not in _SINGLES:
        outs = _singles(P, cases.eval_kkt_outputs if what == "eval_kkt" else cases.iteration_outputs)
        for o in outs:
            for v in o.values():
                v.setflags(write=False)
        _SINGLES[(P.name, what)] = outs
    return _SINGLES[(P.name, what)]


def _check_idc(oracle, P, cdd_flat):
    """[ID; C] of every record against the CPU restatement with the instance's own desired placements"""
    m, n = P.m, len(P.grids)
    L = capi.layout_for(P.dims)
    S, D = Records(L, "sol"), Records(L, "cdd")
    cdd = cdd_flat.reshape(P.batch, n, L.cdd.stride)
    worst = 0.0
    for b in range(P.batch):
        for i in range(n - 1):
            g, s = P.grids[i], P.sol[b, i]
            nf = m.max_dimf
            ref = oracle.rbd_eval(m, g.type == GRID_IMPACT, S.f(s, "q")[:m.nq], S.f(s, "v"), S.f(s, "a"), S.f(s, "f")[:nf], S.f(s, "u")[:m.nu],
                                  int(P.masks[i]), P.pos[b, i].reshape(-1), rref=None if P.rot is None else P.rot[b, i])
            idc = D.f(cdd[b, i], "IDC")[:m.nv + g.dimf]
            worst = max(worst, np.abs(idc - ref).max() / max(1.0, np.abs(ref).max()))
    check_parity("%s: [ID; C] vs restatement with every instance's own placements" % P.name, worst, IDC_BOUND)


@pytest.mark.gpu
def test_eval_kkt_point_contacts_every_instance_on_its_own_footholds(oracle):
    P = cases.anymal_case(oracle)
    feet = P.pos.reshape(P.batch, -1, 3)
    for a in range(P.batch):
        for b in range(a + 1, P.batch):   # an index mix-up cannot hide inside a tolerance
            assert np.linalg.norm(feet[a][:, None] - feet[b][None], axis=-1).min() > 0.01
    ctx = cases.make_context(P, range(P.batch))
    got = cases.eval_kkt_outputs(P, ctx)
    assert ctx.contact_placements()[2] is True
    ctx.close()
    _assert_equal_to_singles("anymal/eval_kkt", got, singles_of(P, "eval_kkt"))
    _check_idc(oracle, P, got["CDD"])


@pytest.mark.gpu
def test_eval_kkt_surface_contacts_positions_and_rotations_per_instance(oracle):
    P = cases.icub_case(oracle)
    ctx = cases.make_context(P, range(P.batch))
    got = cases.eval_kkt_outputs(P, ctx)
    ctx.close()
    assert np.abs(got["CONE"]).max() > 0 and np.abs(got["CON"]).max() > 0   # the cone rows ran
    _assert_equal_to_singles("icub32/eval_kkt", got, singles_of(P, "eval_kkt"))
    _check_idc(oracle, P, got["CDD"])


@pytest.mark.gpu
def test_iteration_evaluation_and_line_search_per_instance(oracle):
    """rtoc_contact_update_solution with the filter line search (trial evaluations included), then rtoc_contact_eval_ocp of the
    new iterate and of its trial iterate: next iterate, accepted steps, KKT error, cost and violation per instance"""
    P = cases.anymal_case(oracle)
    ctx = cases.make_context(P, range(P.batch))
    got = cases.iteration_outputs(P, ctx)
    ctx.close()
    _assert_equal_to_singles("anymal/iteration", got, singles_of(P, "iteration"))


def _poisoned(P):
    """NaN in the placements of every inactive contact, positions and rotations"""
    off = np.array([[not ((int(mk) >> c) & 1) for c in range(P.m.ncontacts)] for mk in P.masks])
    pos = np.array(P.pos)
    pos[:, off] = np.nan
    rot = None
    if P.rot is not None:
        rot = np.array(P.rot)
        rot[:, off] = np.nan
    assert off.any()
    return pos, rot


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["anymal", "icub"])
def test_placements_of_inactive_contacts_are_never_read(oracle, which):
    P = (cases.anymal_case if which == "anymal" else cases.icub_case)(oracle)
    clean = cases.make_context(P, range(P.batch))
    want = cases.eval_kkt_outputs(P, clean)
    clean.close()
    pos, rot = _poisoned(P)
    ctx = cases.make_context(P, range(P.batch), pos=pos, rot=rot)   # accepted: the host check skips inactive entries too
    got = cases.eval_kkt_outputs(P, ctx)
    ctx.close()
    for k in want:
        assert np.isfinite(got[k]).all(), k
        assert np.array_equal(got[k], want[k]), k


# ---- interface ----

def _kkt(P, ctx):
    return cases.eval_kkt_outputs(P, ctx)["CDD"]


@pytest.mark.gpu
def test_refusals_leave_the_table_in_force(oracle):
    P = cases.anymal_case(oracle)
    L, dp = capi.lib(), capi.C.POINTER(capi.C.c_double)
    NOT_READY, BAD_ARG = -5, -1   # RTOC_ERR_NOT_READY, RTOC_ERR_BAD_ARG (include/rtoc.h)
    n, B = len(P.grids), P.batch
    ctx = cases.make_context(P, range(B))
    before = _kkt(P, ctx)
    pos = np.ascontiguousarray(P.pos)
    ptr = lambda a: a.ctypes.data_as(dp)
    codes = {int(L.rtoc_set_contact_placements(ctx._h, ptr(pos), None, k)) for k in (2, -1)}
    bad = pos.copy()
    i_on = int(np.argmax([int(mk) & 1 for mk in P.masks]))
    bad[1, i_on, 0, 2] = np.inf   # contact 0 is active there
    codes.add(int(L.rtoc_set_contact_placements(ctx._h, ptr(bad), None, 1)))
    assert codes == {BAD_ARG}, codes
    for args in ((0, 0, 3, 3, 1), (0, 0, -1, 2, 1), (0, 0, 0, n + 1, 1), (0, 0, 0, n, 1 << 4), (1, n, 0, n, 1), (1, -1, 0, n, 1), (2, 0, 0, n, 1)):
        assert int(L.rtoc_hold_contact_placements(ctx._h, *args)) == BAD_ARG, args
    assert np.array_equal(_kkt(P, ctx), before)
    assert ctx.contact_placements()[2] is True
    # rtoc_set_contact_schedule after a per-instance table returns to shared
    ctx.set_contact_schedule(P.masks, P.pos[1])
    p, _, inst = ctx.contact_placements()
    assert inst is False and np.array_equal(p, np.tile(P.pos[1][None], (B, 1, 1, 1)))
    shared = _kkt(P, ctx)
    one = cases.make_context(P, [0], shared_from=1)
    assert np.array_equal(shared[0], _kkt(P, one)[0])
    one.close()
    # rtoc_set_grid with another grid invalidates the placements with the schedule; the same grid again does not
    ctx.set_grid(P.grids)
    ctx.set_contact_placements(P.pos)
    other = [type(g).from_buffer_copy(g) for g in P.grids]
    other[0].dt = other[0].dt * 0.5
    ctx.set_grid(other)
    assert int(L.rtoc_set_contact_placements(ctx._h, ptr(pos), None, 1)) == NOT_READY
    assert int(L.rtoc_hold_contact_placements(ctx._h, 0, 0, 0, n, 1)) == NOT_READY
    ctx.close()
    # before any schedule, before a model, without the source, on a ParNMPC horizon
    c = capi.Context(P.dims, n, B, 0)
    c.set_grid(P.grids)
    assert int(L.rtoc_set_contact_placements(c._h, ptr(pos), None, 1)) == NOT_READY
    c.set_robot_model(P.m)
    assert int(L.rtoc_set_contact_placements(c._h, ptr(pos), None, 1)) == NOT_READY
    assert int(L.rtoc_contact_frame_placements(c._h, 0, 0, None, None, None, 0)) == NOT_READY   # no initial state
    c.set_contact_schedule(P.masks)
    assert int(L.rtoc_hold_contact_placements(c._h, 0, 0, 0, n, 1)) == NOT_READY     # no initial state
    assert int(L.rtoc_hold_contact_placements(c._h, 1, 0, 0, n, 1)) == NOT_READY     # no solution
    c.close()
    from robotoc_amd.types import iiwa14_dims
    c = capi.Context(iiwa14_dims(), 5, 2, 0)   # a ParNMPC horizon exists for the fixed-base arm alone
    assert int(L.rtoc_parnmpc_set_horizon(c._h, 4)) == 0
    assert int(L.rtoc_hold_contact_placements(c._h, 0, 0, 0, 4, 1)) == BAD_ARG
    assert int(L.rtoc_set_contact_placements(c._h, ptr(pos), None, 1)) == BAD_ARG
    c.close()


@pytest.mark.gpu
def test_clone_carries_the_table_and_its_mode(oracle):
    P = cases.anymal_case(oracle)
    ctx = cases.make_context(P, range(P.batch))
    want = _kkt(P, ctx)
    h = capi.C.c_void_p()
    assert capi.lib().rtoc_clone(ctx._h, capi.C.byref(h)) == 0
    twin = capi.Context.__new__(capi.Context)
    twin.dims, twin.batch, twin.max_stages, twin._h, twin.L, twin.nstages = ctx.dims, ctx.batch, ctx.max_stages, h, ctx.L, ctx.nstages
    twin._model_ncontacts = P.m.ncontacts
    assert twin.contact_placements()[2] is True
    assert np.array_equal(_kkt(P, twin), want)
    # changing one does not change the other
    twin.set_contact_placements(P.pos[::-1])
    assert not np.array_equal(_kkt(P, twin), want)
    assert np.array_equal(_kkt(P, ctx), want)
    ctx.set_contact_schedule(P.masks, P.pos[0])
    assert twin.contact_placements()[2] is True and np.array_equal(twin.contact_placements()[0], P.pos[::-1])
    twin.close()
    ctx.close()


@pytest.mark.gpu
def test_shared_form_of_the_new_call_equals_the_schedule_call(oracle):
    P = cases.anymal_case(oracle)
    a = cases.make_context(P, range(P.batch), shared_from=2)
    want = _kkt(P, a)
    a.set_contact_schedule(P.masks)          # placements gone: zeros
    assert not np.array_equal(_kkt(P, a), want)
    a.set_contact_placements(P.pos[2])       # per_instance = 0
    assert a.contact_placements()[2] is False
    assert np.array_equal(_kkt(P, a), want)
    a.close()


@pytest.mark.gpu
def test_solver_takes_a_per_instance_contact_plan(oracle):
    from robotoc_amd.solver import ContactPlan, OCPSolver
    from robotoc_amd.grid import Event
    P = cases.anymal_case(oracle)
    i_imp = [i for i, g in enumerate(P.grids) if g.type == GRID_IMPACT][0]
    plan = ContactPlan([0b1111, 0b1001, 0b1111], [P.pos[:, 0], P.pos[:, 0], P.pos[:, i_imp]],
                       [Event("lift", 0.03), Event("impact", 0.07)])
    s = OCPSolver(P.m, plan, 0.12, 6, P.cost, batch=P.batch)
    s.discretize(0.0)
    pos, _, inst = s.ctx.contact_placements()
    assert inst is True and np.array_equal(pos, P.pos)
    s.close()
    # the old shape: shared, as before
    plan = ContactPlan([0b1111, 0b1001, 0b1111], [P.pos[1, 0], P.pos[1, 0], P.pos[1, i_imp]], [Event("lift", 0.03), Event("impact", 0.07)])
    s = OCPSolver(P.m, plan, 0.12, 6, P.cost, batch=P.batch)
    s.discretize(0.0)
    pos, _, inst = s.ctx.contact_placements()
    assert inst is False and np.array_equal(pos, np.tile(P.pos[1][None], (P.batch, 1, 1, 1)))
    s.close()
