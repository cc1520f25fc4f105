"""Host side of LocalContactForceCost and the DiscreteTime references (no device): the numpy restatement of the force cost
pinned by finite differences and a hand-written case; the argument checks of costs.LocalContactForceCost; DiscreteTimeSwingFootRef
/ DiscreteTimeCoMRef against hand-computed values on the one-cycle ANYmal trot; GridInfo's defaults; the table-fill rule."""
import numpy as np
import pytest

from robotoc_amd import costs
from robotoc_amd.grid import ContactSequence, Event, anymal_trot_sequence, discretize, jump_sto_sequence
from robotoc_amd.types import GRID_IMPACT, GRID_INTERMEDIATE, GRID_LIFT, GRID_TERMINAL

import contact_force_cost_restatement as fr

P, S = fr.CONTACT_POINT, fr.CONTACT_SURFACE


class _Cost:
    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.f_ref, self.fi_ref = rng.uniform(-30, 30, (n, 3)), rng.uniform(-30, 30, (n, 3))
        self.f_weight, self.fi_weight = rng.uniform(0.1, 5.0, (n, 3)), rng.uniform(0.1, 5.0, (n, 3))
        self.f_weight[n - 1] = 0.0


# ---- the restatement ----
@pytest.mark.parametrize("kind,scale", [("stage", 0.02), ("impact", 1.0)])
def test_restated_gradient_and_hessian_are_the_differences_of_the_restated_value(kind, scale):
    types = [P, P, S, S]
    cost = _Cost(4, 1)
    mask = 0b1101
    offs, rows = fr.offsets(mask, types)
    assert rows == 3 + 6 + 6
    rng = np.random.default_rng(2)
    f = rng.uniform(-50, 50, rows)
    lf, qff, hf, h, val = fr.stage_terms(f, mask, types, cost, kind, scale)
    eps = 1e-3
    for k in range(rows):
        e = np.zeros(rows)
        e[k] = eps
        vp, vm = (fr.value(f + s * e, mask, types, cost, kind, scale) for s in (1.0, -1.0))
        # a quadratic: the central difference is exact up to the rounding of the three values
        bound = 8 * 2.0 ** -53 * max(abs(vp), abs(vm), abs(val)) / eps
        assert abs((vp - vm) / (2 * eps) - lf[k]) <= bound, (k, (vp - vm) / (2 * eps), lf[k], bound)
        assert abs((vp - 2 * val + vm) / eps ** 2 - qff[k]) <= 2 * bound / eps, (k, qff[k])
    if kind == "stage":
        assert np.allclose(hf * scale, lf, rtol=1e-15, atol=0) and abs(h * scale - val) <= 1e-15 * abs(val)
    else:
        assert not hf.any() and h == 0.0
    # rows 3..5 of the surface contacts carry nothing
    for i in (2, 3):
        assert not lf[offs[i] + 3:offs[i] + 6].any() and not qff[offs[i] + 3:offs[i] + 6].any()
    assert fr.stage_terms(f, mask, types, cost, "terminal", 1.0)[4] == 0.0


def test_offsets_skip_an_inactive_middle_contact_by_hand():
    """point, point (inactive), surface, point (inactive), surface: the stack is [p0 | s2 (6) | s4 (6)]"""
    types = [P, P, S, P, S]
    offs, rows = fr.offsets(0b10101, types)
    assert offs == [0, None, 3, None, 9] and rows == 15

    class C:
        f_ref = np.array([[1.0, 2.0, 3.0], [9, 9, 9], [0.5, 0.0, -1.0], [9, 9, 9], [0.0, 0.0, 10.0]])
        f_weight = np.array([[2.0, 0.0, 1.0], [7, 7, 7], [1.0, 1.0, 4.0], [7, 7, 7], [0.5, 0.25, 2.0]])
        fi_ref, fi_weight = f_ref, f_weight
    f = np.arange(15, dtype=float)
    lf, qff, hf, h, val = fr.stage_terms(f, 0b10101, types, C, "stage", 0.5)
    # contact 0 at rows 0..2: d = (0-1, 1-2, 2-3); contact 2 at rows 3..5: d = (3-.5, 4-0, 5+1); contact 4 at rows 9..11: d = (9, 10, 1)
    want_hf = np.zeros(15)
    want_hf[0:3] = [2.0 * -1.0, 0.0, 1.0 * -1.0]
    want_hf[3:6] = [2.5, 4.0, 24.0]
    want_hf[9:12] = [4.5, 2.5, 2.0]
    want_q = np.zeros(15)
    want_q[0:3], want_q[3:6], want_q[9:12] = [1.0, 0.0, 0.5], [0.5, 0.5, 2.0], [0.25, 0.125, 1.0]
    want_h = 0.5 * (2.0 + 0.0 + 1.0 + 6.25 + 16.0 + 144.0 + 40.5 + 25.0 + 2.0)
    assert np.array_equal(hf, want_hf) and np.array_equal(lf, 0.5 * want_hf) and np.array_equal(qff, want_q)
    assert h == want_h and val == 0.5 * want_h


# ---- costs.LocalContactForceCost ----
def test_local_contact_force_cost_checks_its_arguments_and_round_trips():
    c = costs.LocalContactForceCost("anymal")
    assert c.max_num_contacts == 4
    three = [[1.0, 2.0, 3.0]] * 3
    for setter in (c.set_f_ref, c.set_f_weight, c.set_fi_ref, c.set_fi_weight):
        with pytest.raises(ValueError):
            setter(three)
    for setter in (c.set_f_weight, c.set_fi_weight):
        with pytest.raises(ValueError):
            setter([[1.0, 2.0, 3.0], [1.0, -1e-9, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    for setter in (c.set_f_ref, c.set_f_weight, c.set_fi_ref, c.set_fi_weight):   # not a number, infinite: said by the setter
        for v in (float("nan"), float("inf")):
            with pytest.raises(ValueError):
                setter([[1.0, 2.0, 3.0], [1.0, v, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    rng = np.random.default_rng(0)
    vals = [rng.uniform(0.0, 9.0, (4, 3)) for _ in range(4)]
    c.set_f_ref(list(vals[0] - 4.0)), c.set_f_weight(list(vals[1])), c.set_fi_ref(list(vals[2] - 4.0)), c.set_fi_weight(list(vals[3]))
    s = c.to_struct()
    assert isinstance(s, costs.ContactForceCost)
    for name, v in zip(("f_ref", "f_weight", "fi_ref", "fi_weight"), (vals[0] - 4.0, vals[1], vals[2] - 4.0, vals[3])):
        got = np.array([list(r) for r in getattr(s, name)])
        assert got.shape == (costs.MAX_CONTACTS, 3)
        assert np.array_equal(got[:4], v) and not got[4:].any()
    # a refused call leaves what was set
    with pytest.raises(ValueError):
        c.set_f_weight(three)
    assert np.array_equal(c.f_weight, vals[1])


# ---- the DiscreteTime references on the one-cycle trot ----
STEP = np.array([0.15, 0.0, 0.0])
FEET0 = np.array([[0.35, 0.2, 0.0], [-0.35, 0.2, 0.0], [0.35, -0.2, 0.0], [-0.35, -0.2, 0.0]])   # LF, LH, RF, RH
COM2FOOT = FEET0 - np.array([0.0, 0.0, 0.48])


def _trot():
    cs = anymal_trot_sequence(t0=0.11, swing=0.2, double_support=0.1, cycles=1)
    assert cs.phase_masks == [0b1111, 0b1001, 0b1111, 0b0110, 0b1111]
    pos = [FEET0.copy()]
    for ph in range(1, 5):
        p = pos[-1].copy()
        if ph == 2:
            p[[1, 2]] += STEP     # LH, RF have landed
        if ph == 4:
            p[[0, 3]] += STEP     # LF, RH have landed
        pos.append(p)
    cs.phase_positions = pos
    grids, times, structure = discretize(40, 0.8, 0.0, cs, times=True, infos=True)
    infos = costs.grid_infos(times, [g.dt for g in grids], structure)
    return cs, grids, infos


def test_grid_info_defaults_and_structure():
    times, dts = [0.0, 0.1, 0.2], [0.1, 0.1, 0.0]
    for i, g in enumerate(costs.grid_infos(times, dts)):
        assert tuple(g)[:3] == (times[i], dts[i], i) and (g.t, g.dt, g.stage) == (times[i], dts[i], i)
        assert (g.type, g.phase, g.stage_in_phase, g.num_grids_in_phase) == (None, 0, 0, 0)
    assert costs.GridInfo(0.5, 0.1, 3) == costs.GridInfo(0.5, 0.1, 3, None, 0, 0, 0)
    cs, grids, infos = _trot()
    assert len(grids) == 47 and [g.type for g in infos] == [g.type for g in grids]
    # what discretize returned before is what it returns now
    plain = discretize(40, 0.8, 0.0, cs)
    assert [bytes(a) for a in plain] == [bytes(b) for b in grids]
    assert len(discretize(40, 0.8, 0.0, cs, times=True)) == 2
    phase = 0
    for g, gi in zip(grids, infos):
        if g.type in (GRID_IMPACT, GRID_LIFT):
            phase += 1
        assert gi.phase == phase
        if g.type in (GRID_IMPACT, GRID_TERMINAL):
            assert (gi.stage_in_phase, gi.num_grids_in_phase) == (0, 0)
        else:
            assert gi.num_grids_in_phase == g.num_grids_in_phase and 0 <= gi.stage_in_phase < gi.num_grids_in_phase
        if g.type == GRID_LIFT:
            assert gi.stage_in_phase == 0


def test_swing_foot_ref_on_the_trot_by_hand():
    cs, grids, infos = _trot()
    h = 0.1
    seen = {"first": 0, "mid": 0, "last": 0}
    for foot in range(4):
        ref = costs.DiscreteTimeSwingFootRef(foot, h)
        ref.set_swing_foot_ref(cs)
        for gi in infos:
            swings = not cs.is_contact_active(gi.phase, foot)
            assert ref.is_active(gi) == swings
            if not swings or gi.type in (GRID_IMPACT, GRID_TERMINAL):
                continue
            a, b = cs.phase_positions[gi.phase - 1][foot], cs.phase_positions[gi.phase + 1][foot]
            assert np.array_equal(b, a + STEP)
            x = ref.update_ref(gi)
            if gi.stage_in_phase == 0:
                assert np.array_equal(x, a)
                seen["first"] += 1
            elif gi.stage_in_phase in (5, 6):
                # a swing phase of this grid has 11 grid points: the two around mid-swing, one on either branch of the height
                assert gi.num_grids_in_phase == 11
                r = gi.stage_in_phase / 11.0
                want = (1.0 - r) * a + r * b
                want[2] += 2.0 * r * h if gi.stage_in_phase == 5 else 2.0 * (1.0 - r) * h
                assert np.array_equal(x, want)
                # and mid-swing itself, which no grid point of this grid hits: the mean of the two contacts, step_height up
                mid = ref.update_ref(gi._replace(stage_in_phase=5, num_grids_in_phase=10))
                assert np.array_equal(mid, 0.5 * a + 0.5 * b + [0.0, 0.0, h])
                seen["mid"] += 1
            elif gi.stage_in_phase == gi.num_grids_in_phase - 1:
                r = (gi.num_grids_in_phase - 1.0) / gi.num_grids_in_phase
                want = (1.0 - r) * a + r * b
                want[2] += 2.0 * (1.0 - r) * h
                assert np.array_equal(x, want) and 0.5 < r < 1.0
                seen["last"] += 1
    assert seen["first"] == 4 and seen["mid"] == 8 and seen["last"] == 4, seen


def test_first_and_last_rate_blend_in_a_sequence_that_starts_and_ends_in_a_swing():
    cs = ContactSequence([6, 12, 6], [Event("impact", 0.2, impact_dimf=6), Event("lift", 0.5)], phase_masks=[0b1001, 0b1111, 0b1001],
                         phase_positions=[FEET0, FEET0 + STEP, FEET0 + STEP])
    grids, times, structure = discretize(20, 0.8, 0.0, cs, times=True, infos=True)
    infos = costs.grid_infos(times, [g.dt for g in grids], structure)
    first, last = np.array([-0.5, 0.2, 0.0]), np.array([0.1, 0.2, 0.0])
    ref = costs.DiscreteTimeSwingFootRef(1, 0.08)
    ref.set_swing_foot_ref(cs, first, last, 0.3, 0.6)
    mid = (FEET0 + STEP)[1]
    n0 = n2 = 0
    for gi in infos:
        if gi.type in (GRID_IMPACT, GRID_TERMINAL) or gi.phase == 1:
            continue
        r = gi.stage_in_phase / gi.num_grids_in_phase
        if gi.phase == 0:
            r = 0.3 * (1.0 - r) + r
            want = (1.0 - r) * first + r * mid     # contact_position[0], [1]
            n0 += 1
        else:
            r = 0.6 * (1.0 - r) + r
            want = (1.0 - r) * mid + r * last      # contact_position[phase - 1], [phase + 1] = the last one
            n2 += 1
        want[2] += 2.0 * (r if r < 0.5 else 1.0 - r) * 0.08
        assert np.array_equal(ref.update_ref(gi), want), gi
    assert n0 > 1 and n2 > 1
    g0 = infos[0]
    assert np.array_equal(ref.update_ref(g0), 0.7 * first + 0.3 * mid + [0.0, 0.0, 0.6 * 0.08])   # rate 0.3 at stage 0
    # the one-argument form: both rates 1, the foot is at the next contact from the first stage on
    plain = costs.DiscreteTimeSwingFootRef(1, 0.08)
    plain.set_swing_foot_ref(cs)
    assert (plain.first_rate, plain.last_rate) == (1.0, 1.0) and np.array_equal(plain.update_ref(g0), mid)


def _com_positions(cs):
    out = []
    for ph in range(cs.num_contact_phases()):
        act = [i for i in range(4) if cs.is_contact_active(ph, i)]
        out.append(np.mean([cs.phase_positions[ph][i] - COM2FOOT[i] for i in act], axis=0) if act else None)
    return out


def test_com_ref_on_the_trot_is_constant_in_full_support_and_interpolated_elsewhere():
    cs, grids, infos = _trot()
    ref = costs.DiscreteTimeCoMRef(list(COM2FOOT))
    ref.set_com_ref(cs)
    com = _com_positions(cs)
    com.append(com[-1])
    assert abs(com[0][2] - 0.48) < 1e-15 and com[2][0] > com[0][0]
    n_const = n_interp = 0
    for gi in infos:
        assert ref.is_active(gi)
        if gi.type in (GRID_IMPACT, GRID_TERMINAL):
            assert cs.phase_masks[gi.phase] == 0b1111    # a touch-down of this trot leads into full support: the constant
        x = ref.update_ref(gi)
        if cs.phase_masks[gi.phase] == 0b1111:
            assert np.allclose(x, com[gi.phase], rtol=0, atol=1e-15)
            n_const += 1
        else:
            r = gi.stage_in_phase / gi.num_grids_in_phase
            assert np.allclose(x, (1.0 - r) * com[gi.phase] + r * com[gi.phase + 1], rtol=0, atol=1e-15)
            n_interp += 1
    assert n_const > 0 and n_interp > 0


def test_com_ref_of_a_flight_phase_is_the_mean_of_its_neighbours():
    cs = jump_sto_sequence(ground_time=0.31, flying_time=0.2, nf=12)
    cs.phase_masks = [0b1111, 0b0000, 0b1111]
    jump = np.array([0.4, 0.0, 0.0])
    cs.phase_positions = [FEET0, FEET0, FEET0 + jump]
    ref = costs.DiscreteTimeCoMRef(list(COM2FOOT))
    ref.set_com_ref(cs)
    c0, c2 = np.array([0.0, 0.0, 0.48]), np.array([0.4, 0.0, 0.48])
    assert np.allclose(ref.com_position[0], c0, atol=1e-15) and np.allclose(ref.com_position[2], c2, atol=1e-15)
    assert np.allclose(ref.com_position[1], 0.5 * (c0 + c2), atol=1e-15) and ref.has_inactive_contacts == [False, True, False]
    grids, times, structure = discretize(40, 0.8, 0.0, cs, phase_based=True, times=True, infos=True)
    n = 0
    for gi in costs.grid_infos(times, [g.dt for g in grids], structure):
        if gi.phase == 1 and gi.type != GRID_IMPACT:
            r = gi.stage_in_phase / gi.num_grids_in_phase
            assert np.allclose(ref.update_ref(gi), (1.0 - r) * 0.5 * (c0 + c2) + r * c2, rtol=0, atol=1e-15)
            n += 1
    assert n > 2
    # the five-argument form re-averages a flight phase next to a replaced end
    first = np.array([-0.2, 0.0, 0.5])
    ref.set_com_ref(cs, first, c2 + [0.1, 0.0, 0.0], 0.25, 0.5)
    assert np.allclose(ref.com_position[1], 0.5 * (first + c2), atol=1e-15) and (ref.first_rate, ref.last_rate) == (0.25, 0.5)


# ---- the table fill ----
class _Counting:
    def __init__(self, inner):
        self.inner, self.updates = inner, []

    def is_active(self, g):
        return self.inner.is_active(g)

    def update_ref(self, g):
        self.updates.append(g.stage)
        return self.inner.update_ref(g)


def test_table_fill_does_not_ask_where_the_weight_of_the_kind_is_zero():
    cs, grids, infos = _trot()
    ref = costs.DiscreteTimeCoMRef(list(COM2FOOT))
    ref.set_com_ref(cs)
    counting = _Counting(ref)
    c = costs.CoMCost("anymal", counting)
    c.set_weight([1.0, 2.0, 3.0])
    c.set_weight_terminal([1.0, 0.0, 0.0])
    tab = c.ref_table(infos)
    impacts = [i for i, g in enumerate(grids) if g.type == GRID_IMPACT]
    assert len(impacts) == 2
    for i, e in enumerate(tab):
        if i in impacts:
            assert e.active == 0 and not any(e.p) and i not in counting.updates
        else:
            assert e.active == 1 and i in counting.updates and np.array_equal(list(e.p), ref.update_ref(infos[i]))
    # a swing-foot reference: asked only where the foot swings
    foot = costs.DiscreteTimeSwingFootRef(1, 0.1)
    foot.set_swing_foot_ref(cs)
    fc = _Counting(foot)
    t = costs.TaskSpace3DCost("anymal", "LH_FOOT", fc)
    t.set_weight([1.0, 1.0, 1.0]), t.set_weight_impact([1.0, 1.0, 1.0]), t.set_weight_terminal([1.0, 1.0, 1.0])
    tab = t.ref_table(infos)
    swing = [i for i, g in enumerate(infos) if not cs.is_contact_active(g.phase, 1)]
    assert fc.updates == swing and [i for i, e in enumerate(tab) if e.active] == swing
    # grid points that do not say their kind: asked wherever active, as before
    old = _Counting(ref)
    c2 = costs.CoMCost("anymal", old)
    assert len(c2.ref_table(costs.grid_infos([g.t for g in infos if g.type not in (GRID_IMPACT, GRID_TERMINAL)]))) == len(old.updates) == 44


def test_table_fill_refuses_a_reference_that_is_not_a_number_and_names_the_grid_point():
    """On the 4-2-4-2-4 trot a touch-down leads into full support, where DiscreteTimeCoMRef is the phase's constant (see the test
    above): nothing is 0 / 0 there, in the reference either.  The rate is 0 / 0 on an impact grid point whose NEW phase still has a
    foot in the air -- a trot whose swing feet land one after the other."""
    cs = ContactSequence([12, 6, 9, 12], [Event("lift", 0.11), Event("impact", 0.31, impact_dimf=3), Event("impact", 0.35, impact_dimf=3)],
                         phase_masks=[0b1111, 0b1001, 0b1011, 0b1111],
                         phase_positions=[FEET0, FEET0, FEET0 + [[0, 0, 0], [0.15, 0, 0], [0, 0, 0], [0, 0, 0]], FEET0 + [[0, 0, 0], [0.15, 0, 0], [0.15, 0, 0], [0, 0, 0]]])
    grids, times, structure = discretize(20, 0.8, 0.0, cs, times=True, infos=True)
    infos = costs.grid_infos(times, [g.dt for g in grids], structure)
    first_impact = [i for i, g in enumerate(grids) if g.type == GRID_IMPACT][0]
    assert infos[first_impact].phase == 2 and infos[first_impact].num_grids_in_phase == 0
    ref = costs.DiscreteTimeCoMRef(list(COM2FOOT))
    ref.set_com_ref(cs)
    c = costs.CoMCost("anymal", ref)
    c.set_weight([1.0, 1.0, 1.0])
    assert c.ref_table(infos)[first_impact].active == 0   # no impact weight: not asked, nothing to refuse
    c.set_weight_impact([0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match=r"grid point %d\b" % first_impact):
        c.ref_table(infos)
