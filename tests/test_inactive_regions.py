"""The masks of tests/inactive_regions.py against the CPU oracle (no GPU).

Ignored:            every double of input_inactive poisoned (NaN; stale finite data of another instance): the oracle returns the
                    same bits outside output_inactive and the same status.
Not under-claimed:  NaN in any one (field, kind of grid point) group that is NOT in input_inactive reaches a compared output, so
                    no mask passes by claiming too little.  Where the oracle reads less than the reference the group is listed
                    in ORACLE_READS_LESS with the reference's line.
Cap:                output_inactive leaves out only doubles the oracle does not define: those that come back as whatever was
                    there before, for two different sentinels.  Its share per buffer is printed and asserted against the share
                    found that way.
Self-test:          the same checker on two leaky pure-Python consumers names the field and the grid point.

Run with -s for the shares per stage and buffer."""
import numpy as np
import pytest

import inactive_cases as ic
import inactive_regions as ir
from robotoc_amd.types import Records

CASES = {
    "anymal": dict(sto=False, constraints=False),
    "anymal-sto": dict(sto=True, constraints=False),
    "anymal-rows": dict(sto=False, constraints=True),
    "anymal-sto-rows": dict(sto=True, constraints=True),
    "icub": None,
    "iiwa14": None,
    "icub-wrench": None,
}
STAGE_CASES = [("sweep", "anymal"), ("sweep", "anymal-sto"), ("sweep", "icub"),
               ("condense", "anymal"), ("condense", "anymal-sto"),
               ("chain", "anymal-sto"), ("chain", "anymal-rows"), ("chain", "anymal-sto-rows"),
               ("update", "anymal-rows"), ("kkt_error", "anymal-rows"), ("integrate", "anymal"), ("integrate", "iiwa14"),
               ("unconstr", "iiwa14"), ("chain", "icub-wrench"), ("update", "icub-wrench"), ("kkt_error", "icub-wrench"),
               ("sto_kkt", "anymal-sto"), ("sto_steps", "anymal-sto"),
               ("linearize", "iiwa14")]
IDS = ["%s-%s" % sc for sc in STAGE_CASES]

# Groups outside input_inactive whose NaN the oracle's stage does not pass on, because the oracle reads less than the reference:
# (stage, buffer, field) -> why.  None so far: every group that failed while the masks were written turned out to be inactive
# (Qxu, Qvq going into rtoc_unconstr_condense, the diagonal of CDD.MJtJinv, the tail of Quu_passive_topRight, whose block is
# np x nu with leading dimension np) or active after all (the cone rows of an impact point: RTOC_OPT_IMPACT_CONES).
ORACLE_READS_LESS = {}


def _case(oracle, name):
    if CASES[name] is None:
        return {"icub": ic.icub_case, "iiwa14": ic.iiwa14_case, "icub-wrench": ic.icub_wrench_case}[name](oracle.layout)
    return ic.anymal_case(oracle.layout, **CASES[name])


def _setup(oracle, stage, name, fill=0.0):
    """(problem, run, inputs, input masks, output masks) of a stage on a case."""
    _, P, batch = _case(oracle, name)
    constraints = bool(P.rows)
    if stage == "sto_steps":
        inputs = dict(dir=ic.sto_direction(P, batch))
    elif stage == "linearize":
        inputs = dict(sol=ic.unconstr_iterate(P, batch))
    elif stage == "update":
        chain = ic.oracle_chain(oracle, P)(ic.inputs_of(P, batch, "chain", name))
        inputs = dict(con=chain["con"], steps=chain["steps"])
    else:
        inputs = ic.inputs_of(P, batch, "chain" if stage in ("condense", "kkt_error") else ("sweep" if stage == "sto_kkt" else stage), name)
    run = dict(sweep=lambda: ic.oracle_sweep(oracle, P, fill), condense=lambda: ic.oracle_condense(oracle, P),
               chain=lambda: ic.oracle_chain(oracle, P, fill), update=lambda: ic.oracle_update(oracle, P),
               kkt_error=lambda: ic.oracle_kkt_error(oracle, P), integrate=lambda: ic.oracle_integrate(oracle, P),
               unconstr=lambda: ic.oracle_unconstr(oracle, P, fill), sto_kkt=lambda: ic.oracle_sto_kkt(oracle, P),
               sto_steps=lambda: ic.restated_sto_steps(P), linearize=lambda: ic.restated_unconstr_linearize(oracle, P))[stage]()
    ins, outs = ic.stage_io(stage, constraints)
    in_masks = {b: ir.input_inactive(P, b, stage) for b in ins}
    out_masks = {b: ir.output_inactive(P, b, stage) for b in outs}
    return P, run, inputs, in_masks, out_masks


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("stage,name", STAGE_CASES, ids=IDS)
def test_poisoned_inactive_inputs_are_ignored(oracle, stage, name, kind):
    P, run, inputs, in_masks, out_masks = _setup(oracle, stage, name)
    for b, m in in_masks.items():
        print("%-9s %-15s %-5s: %5.1f %% of the %s stride poisoned (%d doubles over %d grid points)"
              % (stage, name, kind, 100.0 * m.mean(), b, int(m.sum()), P.n))
        assert m.any()
    clean = run(inputs)
    assert all(np.isfinite(v[~out_masks[k][None].repeat(v.shape[0], 0)]).all() for k, v in clean.items() if k in out_masks)
    leaks = ir.find_leaks(P, run, inputs, in_masks, out_masks, kind, clean=clean)
    assert not leaks, "\n".join(leaks[:20])


@pytest.mark.parametrize("stage,name", STAGE_CASES, ids=IDS)
def test_every_group_outside_the_mask_reaches_an_output(oracle, stage, name):
    """NaN in one (field, kind of grid point) group of the doubles that are NOT masked, and nowhere else: a compared output
    or the status changes."""
    P, run, inputs, in_masks, out_masks = _setup(oracle, stage, name)
    clean = run(inputs)
    silent = []
    for buf, mask in in_masks.items():
        for (field, knd), gm in sorted(ir.groups(P, buf, ~mask).items()):
            if (stage, buf, field) in ORACLE_READS_LESS:
                continue
            trial = dict(inputs)
            trial[buf] = ir.poison(P, buf, inputs[buf], gm, "nan")
            if not ir.compare_outputs(P, clean, run(trial), out_masks):
                silent.append("%s.%s on '%s' points (%d doubles)" % (buf, field, knd, int(gm.sum())))
    assert not silent, "claimed active but nothing reads them:\n" + "\n".join(silent)


@pytest.mark.parametrize("stage,name", [sc for sc in STAGE_CASES if sc[0] not in ("kkt_error", "sto_steps", "linearize")],
                         ids=[i for i in IDS if "kkt_error" not in i and "sto_steps" not in i and "linearize" not in i])
def test_output_masks_leave_out_only_what_the_oracle_does_not_define(oracle, stage, name):
    """A double the oracle does not define comes back as what was there: the pre-fill of a buffer that is only written, the
    (inactive) input of one that is read and written -- for two sentinels.  output_inactive may hold nothing else."""
    found = None
    for s in (3.25, -17.5):
        P, run, inputs, in_masks, out_masks = _setup(oracle, stage, name, fill=s)
        trial = dict(inputs)
        for b, m in in_masks.items():
            v = np.array(inputs[b])
            v[:, m] = s
            trial[b] = v
        out = run(trial)
        same = {b: (out[b] == s).all(axis=0) for b in out_masks}
        found = same if found is None else {b: found[b] & same[b] for b in same}
    for b, m in out_masks.items():
        extra = m & ~found[b]
        print("%-9s %-15s %-4s: %5.1f %% of the stride left out of comparisons, %5.1f %% not defined by the oracle"
              % (stage, name, b, 100.0 * m.mean(), 100.0 * found[b].mean()))
        assert not extra.any(), "output_inactive hides doubles the oracle defines:\n" + "\n".join(ir.describe(P, b, extra)[:12])
        assert m.mean() <= found[b].mean()


# ---------------------------------------------------------------- the checker fails when it should ----

def _leaky_kkt_error(P):
    """A KKT error that sums Pres over all ns_max rows instead of dims."""
    K = Records(P.L, "kkt")

    def run(inp):
        e = (K.f(inp["kkt"], "lx") ** 2).sum(axis=(1, 2))
        for i, g in enumerate(P.grids[:-1]):
            e = e + (K.f(inp["kkt"][:, i], "Fx") ** 2).sum(axis=1) + (K.f(inp["kkt"][:, i], "Pres") ** 2).sum(axis=1)
        return dict(kkt_error=np.sqrt(e))
    return run


def _leaky_step_size(P):
    """A primal step size over every box row, whatever its level."""
    N = Records(P.L, "con")

    def run(inp):
        nr = len(P.rows)
        s, ds = N.f(inp["con"], "slack")[..., :nr], N.f(inp["con"], "dslack")[..., :nr]
        with np.errstate(all="ignore"):
            f = -ic.TAU * s / ds
        f = np.where((f > 0) & (f < 1), f, 1.0)[:, :-1]   # (a NaN drops out of the comparison like out of fmin)
        return dict(steps=f.min(axis=(1, 2)))
    return run


def test_the_checker_names_the_planted_leaks(oracle):
    _, P, batch = ic.anymal_case(oracle.layout, sto=False, constraints=True)
    inputs = ic.inputs_of(P, batch, "chain", "anymal-rows")
    sc = [i for i, g in enumerate(P.grids) if g.dims > 0][0]
    plain = [i for i, g in enumerate(P.grids[:-1]) if g.dims == 0][0]
    # 1. Pres over 12 rows: NaN and stale data both show it, at the switching-constraint point (rows 6..11) and elsewhere (all 12)
    for kind in ir.POISONS:
        leaks = ir.find_leaks(P, _leaky_kkt_error(P), dict(kkt=inputs["kkt"]), dict(kkt=ir.input_inactive(P, "kkt", "kkt_error")), {}, kind)
        print("\n".join(leaks[:3]))
        assert leaks and all("kkt.Pres" in s for s in leaks)
        assert any("kkt.Pres[6 entries from 6] at grid point %d (" % sc in s for s in leaks)
        assert any("kkt.Pres[12 entries from 0] at grid point %d (" % plain in s for s in leaks)
    # 2. a step size that ignores rtoc_box_row::level and the grid type: the position rows (level 2) at time stages 0 and 1, the
    #    velocity rows (level 1) at stage 0, every row of the impact point.  The NaN drops out of the minimum, so only the stale
    #    finite data shows it.
    con = ic.oracle_chain(oracle, P)(inputs)["con"]
    mask = dict(con=ir.input_inactive(P, "con", "update"))
    run = _leaky_step_size(P)
    assert ir.find_leaks(P, run, dict(con=con), mask, {}, "nan") == []
    leaks = ir.find_leaks(P, run, dict(con=con), mask, {}, "stale")
    print("\n".join(leaks[:3]))
    assert leaks and any(" at grid point 0 (" in s and ("con.slack" in s or "con.dslack" in s) for s in leaks)
    impact = [i for i, g in enumerate(P.grids) if g.type == ir.GRID_IMPACT][0]      # (no box rows on an impact point either)
    assert not any(" at grid point %d (" % i in s for s in leaks for i in range(2, P.n) if i != impact)


def test_the_masks_hold_every_region_the_contract_names(oracle):
    """Spot checks of the mask module against the list of inactive regions, on the ANYmal grid."""
    _, P, _ = ic.anymal_case(oracle.layout, sto=False, constraints=True)
    K, C, N = Records(P.L, "kkt"), Records(P.L, "cdd"), Records(P.L, "con")
    kinds = [P.kind(i) for i in range(P.n)]
    assert {"terminal", "impact dimf=6", "lift dimf=6", "intermediate dimf=12", "intermediate dimf=6 dims=6"} <= set(kinds), kinds
    sw, cd, cc = ir.input_inactive(P, "kkt", "sweep"), ir.input_inactive(P, "cdd", "condense"), ir.input_inactive(P, "con", "chain")
    for i, g in enumerate(P.grids):
        if i == P.N:
            live = ~sw[i]
            assert K.f(live, "Qxx").all() and K.f(live, "lx").all() and live.sum() == K.f(live, "Qxx").size + K.f(live, "lx").size
            continue
        assert K.f(sw[i], "Phix")[g.dims:].all() and K.f(sw[i], "Pres")[g.dims:].all() and not K.f(sw[i], "Phix")[:g.dims].any()
        assert all(K.f(sw[i], f).all() for f in ("fx", "hx", "hu", "scal", "Phit"))     # no STO point on this grid
        assert C.f(cd[i], "Qff")[g.dimf:].all() and C.f(cd[i], "Qff")[:, g.dimf:].all() and C.f(cd[i], "lf")[g.dimf:].all()
        assert C.f(cd[i], "IDC")[P.L.dims.nv + g.dimf:].all() and C.f(cd[i], "dIDCdqv")[P.L.dims.nv + g.dimf:].all()
        if g.type == ir.GRID_IMPACT:
            assert all(K.f(sw[i], f).all() for f in ("Fvu", "Qxu", "Quu", "lu", "hu", "Phiu"))
            assert N.f(cc[i], "slack")[:len(P.rows)].all()      # no box rows; the cone rows of the contacts that touch down
        else:
            for r, row in enumerate(P.rows):
                assert N.f(cc[i], "slack")[r] == (g.time_stage < row.level)
        n = 5 * (g.dimf // 3)
        assert not N.f(cc[i], "slack")[P.cone_row0():P.cone_row0() + n].any() and N.f(cc[i], "slack")[P.cone_row0() + n:].all()
    # the alignment doubles between fields belong to no field and are masked everywhere
    covered = np.zeros(K.stride, dtype=bool)
    for f in K.names:
        covered[K.offset(f):K.offset(f) + int(np.prod(K.shapes[f]))] = True
    assert (~covered).any() and sw[:, ~covered].all()
