"""Every solve-side kernel path is exactly equivariant under the scale group of tests/scale_group.py: fed inputs rescaled by powers
of two (the cost by a power of four), a kernel returns the unit result times the field's factor with identical mantissas --
np.array_equal, no tolerance.  What this sees and the parity tests at unit scale cannot: an absolute threshold or floor, a
regularisation that does not scale, a pivot or "is it positive" test against a constant, low bits dropped in one branch only, an
estimate instruction whose mantissa depends on the exponent.

The unit instance and its scaled copies are different instances of ONE batch in one launch: 2 seeds x 4 group elements = 8
instances, each on its own magnitudes, so a threshold that leaks between instances shows up too.  RTOC_BUF_RIC / RTOC_BUF_DIR are
poisoned with NaN before every launch; the status words of the copies must be equal (and clean).  The CPU oracle is held to the
same equality on the same cases, seeds and elements in tests/test_scale_equivariance.py: what fails here is the kernel's.

No oracle run here: the parity tests hold the kernels to the oracle at unit scale, this file carries that statement to every
scale at the cost of one launch per case."""
import numpy as np
import pytest

import grid_words as gw
import scale_group as sg
from robotoc_amd import problems as pr
from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import BUF_CDD, BUF_CON, BUF_CONE, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP, Dims, Records
from test_every_grid_gpu import CASES, PATHS, _configure

pytestmark = pytest.mark.gpu

BATCH = sg.SEEDS * len(sg.ELEMENTS)
_INPUTS = {}


def _inputs(key, make):
    """inputs of a case, generated once, shared by the paths and left unchanged"""
    if key not in _INPUTS:
        _INPUTS[key] = make()
        for a in (_INPUTS[key].values() if isinstance(_INPUTS[key], dict) else _INPUTS[key]):
            a.setflags(write=False)
    return _INPUTS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_inputs_with_the_module():
    yield
    _INPUTS.clear()


def _poison(ctx, n):
    ctx.upload(BUF_RIC, np.full((ctx.batch, n, ctx.L.ric.stride), np.nan))
    ctx.upload(BUF_DIR, np.full((ctx.batch, n, ctx.L.dir.stride), np.nan))
    ctx.clear_status()


def _sweep(ctx, grids, kkt, dx0, backward, forward):
    ctx.upload(BUF_KKT, kkt)
    ctx.upload(BUF_DX0, dx0)
    _poison(ctx, len(grids))
    backward()
    forward()
    return ctx.status(), ctx.download_records(BUF_RIC, "ric"), ctx.download_records(BUF_DIR, "dir")


def _status_mismatches(st, elements, what):
    bad = sg.per_instance_mismatches("status", st, elements, what=what)
    if (st != 0).any():
        bad.append(("%s status %s" % (what, st), None, "status", 0.0))
    return bad


# ---- the sweep on every backward path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("shape,path", CASES)
def test_sweep_is_scale_equivariant(shape, path, mode):
    """every (shape, path) of tests/test_every_grid_gpu.py on the words of scale_group.WORDS (every grid kind) and one longer
    horizon (phase transitions, the scan's combination levels): backward and forward records, with RTOC_OPT_WRITEBACK_KKT the
    written-back Qxx, Qxu, Quu, lu under their input factors"""
    from robotoc_amd import capi
    cfg = PATHS[path]
    cases = sg.sweep_grids(shape)
    ctx = capi.Context(gw.SHAPES[shape][0], max(len(g) for _, g in cases), BATCH, 0)
    bad = []
    try:
        _configure(ctx, shape, cfg)
        for name, grids in cases:
            kkt, dx0 = _inputs((shape, mode, name), lambda: sg.sweep_inputs(ctx.L, grids, mode))
            ctx.set_grid(grids)
            st, ric, d = _sweep(ctx, grids, kkt, dx0, ctx.riccati_backward, ctx.riccati_forward)
            what = "%s %s %s [%s]" % (shape, path, mode, name)
            bad += _status_mismatches(st, sg.ELEMENTS, what)
            bad += sg.sweep_mismatches(ctx.L, grids, ric, d, what=what, check_sto=False)
            if cfg.get("writeback"):
                kkt_out = ctx.download_records(BUF_KKT, "kkt")
                assert not np.array_equal(kkt_out, kkt)
                bad += sg.writeback_mismatches(ctx.L, grids, kkt_out, what=what)
    finally:
        ctx.close()
    assert not bad, sg.report(bad)


# ---- switching-time optimisation ------------------------------------------------------------------------------------------------
STO_FORMS = {
    "register": lambda c: c.set_backward_register(1),     # the register kernel's STO instantiation (Psi+, Phi+ as rider columns)
    "role-split": lambda c: c.set_backward_register(0),
    "scan": lambda c: c.set_backward_scan(True),          # riccati_scan_sto.hpp: matrix scan + serial vector pass
}


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("form", sorted(STO_FORMS))
def test_sto_sweep_is_scale_equivariant(form, mode):
    """ANYmal jump, both events with switching-time optimisation (44 grid points), c >= 1 (scale_group.ELEMENTS_STO): every STO
    field, the STOPolicy (dtsdx, dtsdts, dts0) and the switching-time directions"""
    from robotoc_amd import capi
    dims, grids, _ = pr.config_anymal_jump_sto()
    ctx = capi.Context(dims, len(grids), BATCH, 0)
    try:
        STO_FORMS[form](ctx)
        ctx.set_max_dts0(0.1)   # the oracle's default
        ctx.set_grid(grids)
        kkt, dx0 = _inputs(("sto", mode), lambda: sg.sweep_inputs(ctx.L, grids, mode, elements=sg.ELEMENTS_STO))
        st, ric, d = _sweep(ctx, grids, kkt, dx0, ctx.riccati_backward, ctx.riccati_forward)
        what = "jump sto %s %s" % (form, mode)
        bad = _status_mismatches(st, sg.ELEMENTS_STO, what)
        bad += sg.sweep_mismatches(ctx.L, grids, ric, d, elements=sg.ELEMENTS_STO, what=what)
        bad += sg.sto_policy_mismatches(ctx.L, grids, ric, sg.ELEMENTS_STO, what=what)
    finally:
        ctx.close()
    assert not bad, sg.report(bad)


# ---- the fixed-base arm ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arm_plugin():
    from robotoc_amd import capi
    for nv in sg.UNCONSTR_SIZES:
        if (nv, nv, 0) not in [tuple(s[:3]) for s in capi.compiled_shapes()]:
            capi.build_plugin(nv, nv, 0)
    return capi


@pytest.mark.parametrize("scan", [False, True], ids=["serial", "scan"])
@pytest.mark.parametrize("dense", [False, True], ids=["structured", "dense"])
@pytest.mark.parametrize("nv", sg.UNCONSTR_SIZES)
def test_unconstr_sweep_is_scale_equivariant(arm_plugin, nv, dense, scan):
    """rtoc_unconstr_backward / rtoc_unconstr_forward: iiwa14 (the register form of the structured recursion) and the nine-joint
    chain (its LDS form), both settings of RTOC_OPT_UNCONSTR_DENSE, with and without the scan; the subgroup a = u
    (scale_group.ELEMENTS_UNCONSTR: B = dt I is built from the call's dt)"""
    dims, grids = Dims(nv, nv, 0, 0, 0, 0), uniform_grid(sg.UNCONSTR_STEPS, sg.UNCONSTR_DT)
    ctx = arm_plugin.Context(dims, len(grids), BATCH, 0)
    try:
        ctx.set_grid(grids)
        ctx.set_unconstr_dense(dense)
        ctx.set_backward_scan(scan)
        ctx.set_writeback(True)
        kkt, dx0 = _inputs(("arm", nv), lambda: sg.sweep_inputs(ctx.L, grids, None, elements=sg.ELEMENTS_UNCONSTR, filler=pr.fill_unconstr_instance))
        st, ric, d = _sweep(ctx, grids, kkt, dx0, lambda: ctx.unconstr_backward(sg.UNCONSTR_DT), lambda: ctx.unconstr_forward(sg.UNCONSTR_DT))
        what = "arm nv = %d %s %s" % (nv, "dense" if dense else "structured", "scan" if scan else "serial")
        bad = _status_mismatches(st, sg.ELEMENTS_UNCONSTR, what)
        bad += sg.sweep_mismatches(ctx.L, grids, ric, d, elements=sg.ELEMENTS_UNCONSTR, what=what, dts=False)
        if not dense and not scan:   # the structured recursion mutates the records in place like the reference
            bad += sg.writeback_mismatches(ctx.L, grids, ctx.download_records(BUF_KKT, "kkt"), elements=sg.ELEMENTS_UNCONSTR, what=what)
    finally:
        ctx.close()
    assert not bad, sg.report(bad)


@pytest.mark.parametrize("dense", [False, True], ids=["structured", "dense"])
@pytest.mark.parametrize("nv", sg.UNCONSTR_SIZES)
def test_unconstr_pipeline_is_scale_equivariant(arm_plugin, nv, dense):
    """rtoc_unconstr_condense -> _backward -> _forward -> _expand under the cost scale: the condensed records, the Riccati records
    and the expanded directions (da, du, dbeta)"""
    import inactive_regions as ir
    dims, grids = Dims(nv, nv, 0, 0, 0, 0), uniform_grid(sg.UNCONSTR_STEPS, sg.UNCONSTR_DT)
    ctx = arm_plugin.Context(dims, len(grids), BATCH, 0)
    try:
        P = ir.Problem(ctx.L, grids)
        ctx.set_grid(grids)
        ctx.set_unconstr_dense(dense)
        inp = _inputs(("arm pipeline", nv), lambda: sg.unconstr_pipeline_inputs(ctx.L, P.n))
        for buf, key in ((BUF_KKT, "kkt"), (BUF_CDD, "cdd"), (BUF_DX0, "dx0")):
            ctx.upload(buf, inp[key])
        _poison(ctx, P.n)
        ctx.unconstr_condense()
        out = dict(kkt=ctx.download_records(BUF_KKT, "kkt"))
        ctx.unconstr_backward(sg.UNCONSTR_DT)
        ctx.unconstr_forward(sg.UNCONSTR_DT)
        ctx.unconstr_expand(sg.UNCONSTR_DT)
        out.update(ric=ctx.download_records(BUF_RIC, "ric"), dir=ctx.download_records(BUF_DIR, "dir"), status=ctx.status())
    finally:
        ctx.close()
    assert (out["status"] == 0).all(), out["status"]
    bad = sg.unconstr_pipeline_mismatches(P, out, what="arm nv = %d %s" % (nv, "dense" if dense else "structured"))
    assert not bad, sg.report(bad)


# ---- condense -> sweep -> expand -> update, the cost scale ------------------------------------------------------------------------
PIPELINES = {
    # RTOC_OPT_CONDENSE_REGISTER, RTOC_OPT_CONDENSE_SPLIT, RTOC_OPT_IMPACT_CONES
    "anymal register":            dict(register=True, split=0),
    "anymal register split":      dict(register=True, split=1),
    "anymal role-split":          dict(register=False, split=0),
    "anymal two-kernel":          dict(register=False, split=1),
    "anymal no impact cones":     dict(register=True, split=0, impact_cones=False),
    "anymal keep Qaf":            dict(register=True, split=0, keep_qaf=True),
    "icub wrench cones":          dict(),
}


def _pipeline_context(name, cfg, newton=False):
    from robotoc_amd import capi
    if name.startswith("icub"):
        dims, P = sg.icub_pipeline_problem(capi.layout_for)
    else:
        dims, P = sg.anymal_pipeline_problem(capi.layout_for, impact_cones=cfg.get("impact_cones", True))
    ctx = capi.Context(dims, P.n, BATCH, 0)
    try:
        ctx.set_grid(P.grids)
        ctx.set_constraint_rows(P.rows)
        if name.startswith("icub"):
            ctx.set_wrench_cones(P.cone_contacts)
        else:
            ctx.set_friction_cones(P.cone_contacts, P.cone_dim)
        if "register" in cfg:
            ctx.set_condense_register(cfg["register"])
        if "split" in cfg:
            ctx.set_condense_split(cfg["split"])
        if "impact_cones" in cfg:
            ctx.set_impact_cones(cfg["impact_cones"])
        if cfg.get("keep_qaf"):
            ctx.set_condense_keep_qaf(True)
        inp = _inputs(("pipeline", name.split()[0]), lambda: sg.pipeline_inputs(P))
        for buf, key in ((BUF_KKT, "kkt"), (BUF_CDD, "cdd"), (BUF_CON, "con"), (BUF_CONE, "cone"), (BUF_DX0, "dx0"), (BUF_SOL, "sol")):
            ctx.upload(buf, inp[key])
        ctx.upload(BUF_STEP, np.ones((BATCH, 2)))
        _poison(ctx, P.n)
        if newton:   # SplitSolution::integrate takes every member's direction at every grid point, the terminal one included: zero
            ctx.upload(BUF_DIR, np.zeros((BATCH, P.n, ctx.L.dir.stride)))
    except Exception:
        ctx.close()
        raise
    return ctx, P


@pytest.mark.parametrize("name", list(PIPELINES))
def test_pipeline_is_equivariant_under_the_cost_scale(name):
    """rtoc_condense -> rtoc_riccati_sweep -> rtoc_expand -> rtoc_update with c = 4^9, 4^-9, 4^20: ANYmal trot with the 72
    joint-limit rows, the 24 acceleration-limit rows and the friction cones of four feet on every condensation kernel, iCub with
    its wrench cones.  The condensed KKT and CDD records and cond; the direction records, dslack / ddual of the box and the cone
    rows; RTOC_BUF_STEP identical bit for bit; slacks and duals after the update."""
    cfg = PIPELINES[name]
    ctx, P = _pipeline_context(name, cfg)
    try:
        ctx.condense()
        out = dict(kkt=ctx.download_records(BUF_KKT, "kkt"))
        ctx.riccati_backward()
        ctx.riccati_forward()
        ctx.expand(sg.PIPELINE_TAU)
        out.update(cdd=ctx.download_records(BUF_CDD, "cdd"), ric=ctx.download_records(BUF_RIC, "ric"), dir=ctx.download_records(BUF_DIR, "dir"),
                   con=ctx.download_records(BUF_CON, "con"), steps=ctx.download(BUF_STEP, (BATCH, 2)))
        ctx.update()
        out.update(con_updated=ctx.download_records(BUF_CON, "con"), status=ctx.status())
    finally:
        ctx.close()
    assert (out["status"] == 0).all(), out["status"]
    assert (out["steps"] < 1.0).any() and (out["steps"] > 0.0).all()
    bad = sg.pipeline_mismatches(P, out, what=name, keep_qaf=bool(cfg.get("keep_qaf")))
    assert not bad, sg.report(bad)


@pytest.mark.parametrize("name", ["anymal register", "anymal two-kernel", "icub wrench cones"])
def test_newton_iteration_is_equivariant_under_the_cost_scale(name):
    """One rtoc_newton_iteration(kkt_tol = 0, tau) on both condensation pipelines, the multipliers and duals of the iterate scaled
    by c: the next iterate's primal part identical, its dual part times c.  kkt_tol = 0: the convergence freeze compares a norm
    that mixes cost and feasibility terms and is not equivariant by design."""
    ctx, P = _pipeline_context(name, PIPELINES[name], newton=True)
    try:
        ctx.newton_iteration(0.0, sg.PIPELINE_TAU)
        assert ctx.converged_count() == 0
        out = dict(dir=ctx.download_records(BUF_DIR, "dir"), con_updated=ctx.download_records(BUF_CON, "con"),
                   sol=ctx.download_records(BUF_SOL, "sol"), steps=ctx.download(BUF_STEP, (BATCH, 2)), status=ctx.status())
    finally:
        ctx.close()
    assert (out["status"] == 0).all(), out["status"]
    assert (out["steps"] < 1.0).any() and (out["steps"] > 0.0).all()
    S = Records(P.L, "sol")
    assert not np.array_equal(S.f(out["sol"], "v"), S.f(_INPUTS[("pipeline", name.split()[0])]["sol"], "v"))   # the iterate moved
    bad = sg.pipeline_mismatches(P, out, what=name + " newton")
    assert not bad, sg.report(bad)
