"""No kernel reads a record's inactive entries.

Every generator of robotoc_amd/problems.py starts from zeros and fills the active part of a record, so a kernel that loads a
full 12-row tile and uses it, sums over nf_max instead of dimf, applies a box row below its level or takes a control field of
an impact point finds zeros there and passes every parity test.  In use those entries hold whatever the last contact phase, the
last grid or the caller's buffer left in them.

Per stage: clean inputs (zero padding) through the entry point on the device; the same inputs with every double of
tests/inactive_regions.py's input_inactive poisoned (NaN; stale finite data of another instance at the field's scale) through it
again on a fresh upload, output buffers zeroed; the outputs outside output_inactive, the step sizes and the status words must be
the same BITS -- no tolerance: the two runs execute the same code on the same data (tests/test_determinism.py).  On a difference
the poison is applied again group by group and grid point by grid point, and the failure names the input field and grid point
that was read and the first output that changed.  tests/test_inactive_regions.py makes the masks exact against the CPU oracle.

NaN and stale doubles in record DATA index nothing and change no launch geometry.

Shapes (tests/inactive_cases.py): ANYmal, 12 grid points with a lift 12 -> 6, an impact 6 -> 12 whose switching constraint has
dims = 6, the terminal point, with and without switching-time optimisation, batch 5 (one full 4-instance workgroup and one
partial; 2 where the robot model is evaluated); iCub nv = 35 (the register-wide / tile-split kernels; wrench cones), 10 grid points,
batch 2; iiwa14, 4 intervals, batch 3, with position / velocity / torque rows (levels 2 / 1 / 0) where the rows are exercised.

The stages that start from the iterate in RTOC_BUF_SOL (initConstraints, the linearisation on both paths, the line search's
evaluation, a whole unconstrained iteration) have no CPU oracle that runs them end to end; their masks are the reference's
SplitSolution / ConstraintComponentData semantics, every output that is only written is compared in full, and a self-check shows
that a read of the iterate is seen."""
import numpy as np
import pytest

import inactive_cases as ic
import inactive_regions as ir
from robotoc_amd.types import BUF_CDD, BUF_CON, BUF_CONE, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP

pytestmark = pytest.mark.gpu

BUFS = dict(kkt=BUF_KKT, cdd=BUF_CDD, con=BUF_CON, cone=BUF_CONE, dx0=BUF_DX0, ric=BUF_RIC, dir=BUF_DIR, steps=BUF_STEP)

SWEEPS = {
    # what rtoc_riccati_sweep runs: RTOC_OPT_BACKWARD_WAVES 0 (default: the register kernels where they apply), the same without
    # them, the one-wave, role-split pair and tile-split variants, and the scan over the horizon
    "default": lambda c: None,
    "waves0": lambda c: c.set_backward_register(False),
    "waves1": lambda c: c.set_backward_waves(1),
    "waves2": lambda c: c.set_backward_waves(2),
    "waves3": lambda c: c.set_backward_waves(3),
    "scan": lambda c: c.set_backward_scan(True),
}
CONDENSES = {
    "default": lambda c: None,
    "keep_qaf": lambda c: c.set_condense_keep_qaf(True),
    "role-split": lambda c: c.set_condense_register(False),
    "two-kernel": lambda c: c.set_condense_split(True),
    "one-kernel": lambda c: (c.set_condense_register(False), c.set_condense_split(False)),
}


class Device:
    """One context per test; run(inputs) uploads every input afresh, zeroes the buffers that are only written, and calls `body`."""

    def __init__(self, dims, P, batch, setup=None, sto=False):
        from robotoc_amd import capi
        self.P, self.batch = P, batch
        self.ctx = capi.Context(dims, P.n, batch, 0)
        self.ctx.set_grid(P.grids)
        if sto:
            self.ctx.set_max_dts0(0.1)   # the oracle's default
        if P.rows:
            self.ctx.set_constraint_rows(P.rows)
        if P.cone_contacts and P.cone_rows == ir.WRENCH_ROWS:
            self.ctx.set_wrench_cones(P.cone_contacts)
        elif P.cone_contacts:
            self.ctx.set_friction_cones(P.cone_contacts, P.cone_dim)
        if setup:
            setup(self.ctx)

    def load(self, inputs, zero=("ric", "dir")):
        c = self.ctx
        c.clear_status()
        for name, arr in inputs.items():
            c.upload(BUFS[name], arr)
        for name in zero:
            c.upload(BUFS[name], np.zeros(c.shape(name)))

    def records(self, *names):
        return {n: self.ctx.download_records(BUFS[n], n) for n in names}

    def close(self):
        self.ctx.close()


def _sweep(dev):
    def run(inp):
        dev.load(inp)
        dev.ctx.riccati_sweep()
        out = dev.records("ric", "dir")
        out["status"] = dev.ctx.status()
        return out
    return run


def _condense(dev):
    def run(inp):
        dev.load({k: v for k, v in inp.items() if k != "dx0"}, zero=())
        dev.ctx.condense()
        out = dev.records("kkt", "cdd")
        out["status"] = dev.ctx.status()
        return out
    return run


def _chain(dev):
    """rtoc_condense -> rtoc_riccati_sweep -> rtoc_expand: the sweep sees whatever the condensation left in the padding."""
    def run(inp):
        c = dev.ctx
        dev.load(inp)
        constrained = "con" in inp
        if constrained:
            c.upload(BUF_STEP, np.ones((dev.batch, 2)))
        c.condense()
        out = dev.records("kkt")
        c.riccati_sweep()
        c.expand(ic.TAU)
        out.update(dev.records("cdd", "ric", "dir"))
        if constrained:
            out.update(dev.records("con"))
            out["steps"] = c.download(BUF_STEP, (dev.batch, 2))
        out["status"] = c.status()
        return out
    return run


def _update(dev):
    def run(inp):
        dev.load(inp, zero=())
        dev.ctx.update()
        return dev.records("con")
    return run


def _kkt_error(dev):
    def run(inp):
        dev.load({k: v for k, v in inp.items() if k in ("kkt", "cdd", "con")}, zero=())
        out = dict(kkt_error=dev.ctx.kkt_error())
        out["status"] = dev.ctx.status()
        return out
    return run


def _check(P, run, inputs, stage, kind, constraints, keep_qaf=True):
    ins, outs = ic.stage_io(stage, constraints)
    in_masks = {b: ir.input_inactive(P, b, stage) for b in ins}
    out_masks = {b: ir.output_inactive(P, b, stage, keep_qaf) for b in outs}
    clean = run(inputs)
    for name, v in clean.items():      # the clean run means something: finite where it is compared, status 0
        if name in out_masks:
            assert np.isfinite(v[:, ~out_masks[name]]).all(), name
            assert np.abs(v[:, ~out_masks[name]]).sum() > 0, name
    if "status" in clean:
        assert (clean["status"] == 0).all(), clean["status"]
    leaks = ir.find_leaks(P, run, inputs, in_masks, out_masks, kind, clean=clean)
    assert not leaks, "%d inactive regions are read:\n%s" % (len(leaks), "\n".join(leaks[:16]))


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("sto", [False, True], ids=["fixed", "sto"])
@pytest.mark.parametrize("variant", sorted(SWEEPS))
def test_riccati_sweep(variant, sto, kind):
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, sto=sto)
    dev = Device(dims, P, batch, SWEEPS[variant], sto)
    try:
        _check(P, _sweep(dev), ic.inputs_of(P, batch, "sweep", "anymal-sto" if sto else "anymal"), "sweep", kind, False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("variant", ["default", "waves0"])
def test_riccati_sweep_icub(variant, kind):
    """default: the register-wide kernel (two waves per instance at nx = 70); waves0: without it, the tile-split kernel."""
    from robotoc_amd import capi
    dims, P, batch = ic.icub_case(capi.layout_for)
    dev = Device(dims, P, batch, SWEEPS[variant])
    try:
        _check(P, _sweep(dev), ic.inputs_of(P, batch, "sweep", "icub"), "sweep", kind, False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("sto", [False, True], ids=["fixed", "sto"])
@pytest.mark.parametrize("variant", sorted(CONDENSES))
def test_condense(variant, sto, kind):
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, sto=sto)
    dev = Device(dims, P, batch, CONDENSES[variant], sto)
    try:
        _check(P, _condense(dev), ic.inputs_of(P, batch, "chain", "anymal-sto" if sto else "anymal"), "condense", kind, False,
               keep_qaf=variant == "keep_qaf")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("constraints", [False, True], ids=["plain", "rows+cones"])
@pytest.mark.parametrize("sto", [False, True], ids=["fixed", "sto"])
@pytest.mark.parametrize("variant", ["default", "keep_qaf", "two-kernel"])
def test_condense_sweep_expand(variant, sto, constraints, kind):
    """With rows + cones: the joint-limit rows (position / velocity / torque: levels 2 / 1 / 0) and the friction-cone rows in their
    condense and expand modes, and the step sizes of RTOC_BUF_STEP."""
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, sto=sto, constraints=constraints)
    dev = Device(dims, P, batch, CONDENSES[variant], sto)
    try:
        name = "anymal" + ("-sto" if sto else "") + ("-rows" if constraints else "")
        _check(P, _chain(dev), ic.inputs_of(P, batch, "chain", name), "chain", kind, constraints, keep_qaf=variant == "keep_qaf")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
def test_pdipm_update(oracle, kind):
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, constraints=True)
    chain = ic.oracle_chain(oracle, P)(ic.inputs_of(P, batch, "chain", "anymal-rows"))
    dev = Device(dims, P, batch)
    try:
        _check(P, _update(dev), dict(con=chain["con"], steps=chain["steps"]), "update", kind, True)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
def test_kkt_error(kind):
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, constraints=True)
    dev = Device(dims, P, batch)
    try:
        inputs = {k: v for k, v in ic.inputs_of(P, batch, "chain", "anymal-rows").items() if k in ("kkt", "cdd", "con")}
        _check(P, _kkt_error(dev), inputs, "kkt_error", kind, True)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("stage", ["chain", "update", "kkt_error"])
def test_wrench_cones(oracle, stage, kind):
    """iCub with joint-limit rows and the 17 wrench-cone rows per foot: condensation, expansion with the step sizes, update and
    KKT error with one foot in the air (the rows, the cone matrix and the wrench of the other contact slot are stale)."""
    from robotoc_amd import capi
    dims, P, batch = ic.icub_wrench_case(capi.layout_for)
    inputs = ic.inputs_of(P, batch, "chain", "icub-wrench")
    if stage == "update":
        chain = ic.oracle_chain(oracle, P)(inputs)
        inputs = dict(con=chain["con"], steps=chain["steps"])
    elif stage == "kkt_error":
        inputs = {k: v for k, v in inputs.items() if k in ("kkt", "cdd", "con")}
    dev = Device(dims, P, batch)
    try:
        _check(P, dict(chain=_chain, update=_update, kkt_error=_kkt_error)[stage](dev), inputs, stage, kind, True, keep_qaf=False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("robot", ["anymal", "iiwa14"])
def test_integrate_solution(robot, kind):
    """The stale f / mu of a contact that is not active, the directions beyond nv + dimf and dims, an impact point's controls."""
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for) if robot == "anymal" else ic.iiwa14_case(capi.layout_for)
    dev = Device(dims, P, batch)

    def run(inp):
        c = dev.ctx
        c.clear_status()
        c.upload(BUF_SOL, inp["sol"])
        c.upload(BUF_DIR, inp["dir"])
        c.upload(BUF_STEP, inp["steps"])
        c.integrate_solution()
        return dict(sol=c.download_records(BUF_SOL, "sol"), status=c.status())
    try:
        _check(P, run, ic.inputs_of(P, batch, "integrate", robot), "integrate", kind, False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("dense", [False, True], ids=["structured", "dense"])
def test_unconstrained_path(dense, kind):
    """rtoc_unconstr_condense -> _backward -> _forward -> _expand on the fixed-base arm: the terminal point but Qxx, lx; Fxx, Fvu
    and the switching-time fields, which this path does not have; Qxu and Qvq, which the condensation writes; the diagonal of
    the full torque Hessian in the MJtJinv field (it is the Qaa field)."""
    from robotoc_amd import capi
    dims, P, batch = ic.iiwa14_case(capi.layout_for)
    dev = Device(dims, P, batch, lambda c: c.set_unconstr_dense(dense))

    def run(inp):
        c = dev.ctx
        dev.load(inp)
        c.unconstr_condense()
        out = dev.records("kkt")
        c.unconstr_backward(ic.IIWA_DT)
        c.unconstr_forward(ic.IIWA_DT)
        c.unconstr_expand(ic.IIWA_DT)
        out.update(dev.records("ric", "dir"))
        out["status"] = c.status()
        return out
    try:
        _check(P, run, ic.inputs_of(P, batch, "unconstr", "iiwa14"), "unconstr", kind, False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
def test_the_check_sees_a_read_on_the_device(kind):
    """The harness itself, on the device: a mask that wrongly calls lu of grid point 2 inactive is reported, with its name."""
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for)
    dev = Device(dims, P, batch)
    try:
        wrong = ir.input_inactive(P, "kkt", "sweep")
        P.rec("kkt").f(wrong[2], "lu")[...] = True
        out_masks = {b: ir.output_inactive(P, b, "sweep") for b in ("ric", "dir")}
        leaks = ir.find_leaks(P, _sweep(dev), ic.inputs_of(P, batch, "sweep", "anymal"), dict(kkt=wrong), out_masks, kind)
        assert len(leaks) == 1 and "kkt.lu[12 entries from 0] at grid point 2 (" in leaks[0], leaks
    finally:
        dev.close()


# ---------------------------------------------------------------- switching-time optimisation ----

@pytest.mark.parametrize("kind", ir.POISONS)
def test_sto_eval_kkt(kind):
    """rtoc_sto_eval_kkt: of the condensed records only h of every grid point but the last (an impact point's too: an input
    here) and Qtt where an event's terms are scattered."""
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, sto=True)
    dev = Device(dims, P, batch, sto=True)
    lt, qtt = ic.sto_terms(batch)

    def run(inp):
        dev.load(dict(kkt=inp["kkt"]), zero=())
        term = dev.ctx.sto_eval_kkt(lt, qtt)
        out = dev.records("kkt")
        out.update(sto_kkt_term=term, status=dev.ctx.status())
        return out
    try:
        _check(P, run, dict(kkt=ic.inputs_of(P, batch, "sweep", "anymal-sto")["kkt"]), "sto_kkt", kind, False)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ir.POISONS)
def test_sto_on_the_device(kind):
    """SwitchingTimeOptimization resident on the device: rtoc_sto_eval_kkt_device on poisoned records, then
    rtoc_sto_compute_step_sizes on direction records of which only dts counts."""
    from robotoc_amd import capi
    dims, P, batch = ic.anymal_case(capi.layout_for, sto=True)
    dev = Device(dims, P, batch, sto=True)
    rng = np.random.default_rng(29)
    c = dev.ctx
    slack, dual = rng.uniform(0.05, 0.4, (batch, 3)), rng.uniform(0.002, 0.05, (batch, 3))
    d0 = ic.sto_direction(P, batch)

    def run(inp):
        c.clear_status()
        c.sto_set_problem(0.0, 0.16, np.array([0.05, 0.11]), np.array([0.02, 0.02, 0.02]), 1.0e-3, ic.TAU)
        c.sto_set_regularization(0.05)
        c.sto_set_slack_dual(slack, dual)
        c.sto_set_cost_terms(*ic.sto_terms(batch))
        c.upload(BUF_KKT, inp["kkt"])
        c.upload(BUF_DIR, inp["dir"])
        c.upload(BUF_STEP, np.tile([0.9, 0.8], (batch, 1)))
        c.sto_eval_kkt_device()
        lt, qd, err = c.sto_kkt_terms()
        out = dev.records("kkt")
        c.sto_compute_step_sizes()
        out.update(lt=lt, qtt=qd, sto_kkt_term=err, steps=c.download(BUF_STEP, (batch, 2)), rows=c.sto_constraint_data(), status=c.status())
        return out
    try:
        inputs = dict(kkt=ic.inputs_of(P, batch, "sweep", "anymal-sto")["kkt"], dir=d0)
        in_masks = dict(kkt=ir.input_inactive(P, "kkt", "sto_kkt"), dir=ir.input_inactive(P, "dir", "sto_steps"))
        out_masks = dict(kkt=ir.output_inactive(P, "kkt", "sto_kkt"))
        clean = run(inputs)
        assert (clean["status"] == 0).all() and np.isfinite(clean["steps"]).all() and (clean["steps"][:, 0] < 0.9).any()
        leaks = ir.find_leaks(P, run, inputs, in_masks, out_masks, kind, clean=clean)
        assert not leaks, "\n".join(leaks)
    finally:
        dev.close()


# ---------------------------------------------------------------- stages that start from the iterate ----

def _iterate_check(P, run, inputs, stage, kind, in_bufs, masked_outputs):
    in_masks = {b: ir.input_inactive(P, b, stage) for b in in_bufs}
    out_masks = {b: ir.output_inactive(P, b, stage) for b in masked_outputs}     # every other output is compared in full
    clean = run(inputs)
    assert (clean["status"] == 0).all(), clean["status"]
    for name, v in clean.items():
        if name in out_masks:
            assert np.isfinite(v[:, ~out_masks[name]]).all(), name
        elif name != "status":
            assert np.isfinite(v).all() and np.abs(v).sum() > 0, name
    leaks = ir.find_leaks(P, run, inputs, in_masks, out_masks, kind, clean=clean)
    assert not leaks, "%d inactive regions are read:\n%s" % (len(leaks), "\n".join(leaks[:16]))


def _clean(P, buf, stage, arr):
    arr[:, ir.input_inactive(P, buf, stage)] = 0.0
    return arr


def _iiwa14_rows():
    """iiwa14, 4 intervals, batch 3, with position / velocity / torque rows: levels 2, 1 and 0 all occur within the grid."""
    from robotoc_amd import capi, robot_model as rm
    from robotoc_amd.grid import uniform_grid
    from robotoc_amd.types import VAR_Q, VAR_V, Dims, joint_limit_rows
    dims = Dims(7, 7, 0, 0, 0, 48)
    rows = joint_limit_rows(dims)
    P = ir.Problem(capi.layout_for(dims), uniform_grid(4, ic.IIWA_DT), rows)
    m = rm.load_named("iiwa14")
    nv, batch = 7, 3
    rng = np.random.default_rng(21)
    dev = Device(dims, P, batch)
    c = dev.ctx
    c.set_robot_model(m)
    c.set_constraint_bounds(np.array([{VAR_Q: 0.6, VAR_V: 1.5}.get(r.var, 60.0) for r in rows]), 1.0e-3, ic.TAU)
    c.set_configuration_cost(q_ref=rng.uniform(-0.5, 0.5, nv), v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0),
                             v_weight=np.full(nv, 0.1), a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.001),
                             q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 0.1))
    c.set_initial_state(np.concatenate([rng.uniform(-0.4, 0.4, (batch, nv)), np.zeros((batch, nv))], axis=1))
    sol = rng.uniform(-1, 1, c.shape("sol"))
    S = P.rec("sol")
    S.f(sol, "q")[...] *= 0.4
    S.f(sol, "u")[...] *= 20.0
    return dev, P, batch, _clean(P, "sol", "linearize", sol)


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("stage", ["init", "linearize", "iterate"])
def test_unconstrained_box_rows(stage, kind):
    """The joint-limit rows of the unconstrained path, resident on the device: rtoc_unconstr_init_constraints (every double of
    RTOC_BUF_CON stale going in), rtoc_unconstr_eval_kkt (linearizeConstraints: slack / dual of the rows below their level and
    of the terminal point stale, as all their other fields) and one whole rtoc_unconstr_update_solution (condense, expand,
    step sizes, update).  Of the iterate the terminal point's a, u, beta and the alignment doubles are stale."""
    dev, P, batch, sol = _iiwa14_rows()
    c = dev.ctx
    try:
        c.upload(BUF_SOL, sol)
        c.upload(BUF_CON, np.zeros(c.shape("con")))
        c.unconstr_init_constraints()
        con = _clean(P, "con", "linearize", c.download_records(BUF_CON, "con"))

        def run(inp):
            c.clear_status()
            c.upload(BUF_SOL, inp["sol"])
            c.upload(BUF_CON, inp["con"])
            for name in ("kkt", "cdd", "dir", "ric"):
                c.upload(BUFS[name], np.zeros(c.shape(name)))
            if stage == "init":
                c.unconstr_init_constraints()
                out = dev.records("con")
            elif stage == "linearize":
                c.unconstr_eval_kkt(ic.IIWA_DT)
                out = dev.records("con", "kkt", "cdd")
                out["dx0"] = c.download(BUF_DX0, (batch, 2 * P.L.dims.nv))
            else:
                err = c.unconstr_update_solution(ic.IIWA_DT)
                out = dev.records("con")
                out.update(sol=c.download_records(BUF_SOL, "sol"), kkt_error=err, steps=c.download(BUF_STEP, (batch, 2)))
            out["status"] = c.status()
            return out
        _iterate_check(P, run, dict(sol=sol, con=con), stage, kind, ("sol", "con"), ("con", "sol") if stage == "iterate" else ("con",))
    finally:
        dev.close()


def _anymal_contact(fused=False):
    """ANYmal on the 12-point grid with its model, the contact schedule of the lift / touch-down of LH + RF, joint-limit and
    friction-cone rows evaluated on the device."""
    from oracle import oracle
    from robotoc_amd import capi, robot_model as rm
    from robotoc_amd.grid import ANYMAL_Q_STANDING, contact_masks
    dims, P, batch = ic.anymal_case(capi.layout_for, constraints=True)
    batch = 2
    m = rm.load_named("anymal")
    q0 = np.array(ANYMAL_Q_STANDING, dtype=np.float64)
    nv, nu, n = 18, 12, P.n
    rng = np.random.default_rng(11)
    dev = Device(dims, P, batch)
    c = dev.ctx
    c.set_robot_model(m)
    feet = np.array([oracle.rbd_contact_position(m, q0, k) for k in range(4)])
    c.set_contact_schedule(contact_masks(P.grids, [0b1111, 0b1001, 0b1111], [0b0110]), np.tile(feet[None], (n, 1, 1)))
    c.set_constraint_bounds(np.concatenate([np.full(2 * nu, 2.0), np.full(2 * nu, 7.5), np.full(2 * nu, 40.0)]), 1.0e-3, ic.TAU)
    c.set_friction_coefficients(np.array([0.7, 0.6, 0.8, 0.5]))
    c.set_linearize_fused(fused)
    wq = np.concatenate([np.full(6, 10.0), np.full(12, 1.0)])
    c.set_configuration_cost(q0, np.zeros(nv), np.zeros(nu), wq, np.full(nv, 1.0), np.full(nv, 1e-3), np.full(nu, 1e-3), 10.0 * wq,
                             np.full(nv, 1.0), q_weight_impact=wq, v_weight_impact=np.full(nv, 1.0), dv_weight_impact=np.full(nv, 1e-3))
    c.set_initial_state(np.tile(np.concatenate([q0, np.zeros(nv)]), (batch, 1)))
    S = P.rec("sol")
    sol = np.zeros(c.shape("sol"))
    for b in range(batch):
        for i in range(n):
            q = q0.copy()
            q[:7] = oracle.se3_integrate(q0[:7], 0.2 * rng.uniform(-1, 1, 6))
            q[7:] += 0.3 * rng.uniform(-1, 1, 12)
            S.f(sol[b, i], "q")[:19] = q
            for f, sc in (("v", 3.0), ("a", 1.0), ("u", 30.0), ("lmd", 0.5), ("gmm", 0.5), ("beta", 0.5), ("mu", 0.5), ("nu_passive", 0.5),
                          ("xi", 0.5)):
                S.f(sol[b, i], f)[:] = sc * rng.uniform(-1, 1, S.f(sol[b, i], f).shape)
            f = rng.uniform(-1, 1, 12) * 20.0
            f[2::3] = rng.uniform(20, 80, 4)
            S.f(sol[b, i], "f")[:] = f
    return dev, P, batch, _clean(P, "sol", "linearize", sol)


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("stage", ["init", "linearize", "linearize-fused", "eval_ocp", "eval_ocp-trial"])
def test_contact_path_from_the_iterate(stage, kind):
    """rtoc_contact_init_constraints, rtoc_contact_eval_kkt on both paths (walk with pre-pass / RTOC_OPT_LINEARIZE_FUSED) with the
    joint-limit and friction-cone rows linearised on the device, and the line search's evaluation rtoc_contact_eval_ocp of the
    iterate and of a trial iterate: the f and mu a lifted foot left behind in RTOC_BUF_SOL, the controls of the impact point, the
    terminal point but q, v, lmd, gmm, the rows below their level and on the impact / terminal points, the cone rows of the
    contact slots that are not active, and the alignment doubles are stale."""
    dev, P, batch, sol = _anymal_contact(fused=stage == "linearize-fused")
    c = dev.ctx
    name = stage.split("-")[0]
    try:
        c.upload(BUF_SOL, sol)
        c.upload(BUF_CON, np.zeros(c.shape("con")))
        c.contact_init_constraints()
        con = c.download_records(BUF_CON, "con")
        inputs = dict(sol=sol, con=con)
        if stage == "eval_ocp-trial":      # a direction and the rows' dslack at the scale of a Newton step
            rng = np.random.default_rng(31)
            inputs["dir"] = _clean(P, "dir", "eval_ocp", 0.05 * rng.uniform(-1, 1, c.shape("dir")))
            P.rec("con").f(con, "dslack")[...] = 0.01 * rng.uniform(-1, 1, P.rec("con").f(con, "dslack").shape)
        inputs["con"] = _clean(P, "con", name, con)

        def run(inp):
            c.clear_status()
            c.upload(BUF_SOL, inp["sol"])
            c.upload(BUF_CON, inp["con"])
            for nm in ("kkt", "cdd"):
                c.upload(BUFS[nm], np.zeros(c.shape(nm)))
            if name == "init":
                c.contact_init_constraints()
                out = dev.records("con")
            elif name == "linearize":
                c.contact_eval_kkt()
                out = dev.records("con", "kkt", "cdd")
                stride = c.buffer_count(BUF_CONE) // (batch * P.n)
                out["cone_jacobians"] = c.download(BUF_CONE, (batch, P.n, stride))
                out["dx0"] = c.download(BUF_DX0, (batch, 36))
            else:
                c.contact_eval_kkt()
                if "dir" in inp:
                    c.upload(BUF_DIR, inp["dir"])
                    c.upload(BUF_STEP, np.tile([0.5, 0.5], (batch, 1)))
                cost, viol = c.contact_eval_ocp(trial="dir" in inp)
                out = dict(cost=cost, violation=viol)
            out["status"] = c.status()
            return out
        _iterate_check(P, run, inputs, name, kind, [b for b in ("sol", "con", "dir") if b in inputs], ("con",) if name != "eval_ocp" else ())
    finally:
        dev.close()


def _icub_wrench_contact():
    """iCub (nv = 35) on the 10-point grid: the left sole lifts and touches down again; joint-limit rows and the 17 wrench-cone rows
    of each sole evaluated on the device."""
    from oracle import oracle
    from robotoc_amd import capi, robot_model as rm
    from robotoc_amd.grid import ICUB_Q_STANDING, contact_masks
    dims, P, batch = ic.icub_wrench_case(capi.layout_for)
    m = rm.load_named("icub")
    assert m.nv == dims.nv
    nv, nq, nu, n = m.nv, m.nq, m.nv - 6, P.n
    q0 = np.array(ICUB_Q_STANDING, dtype=np.float64)
    rng = np.random.default_rng(13)
    dev = Device(dims, P, batch)
    c = dev.ctx
    c.set_robot_model(m)
    placements = [oracle.rbd_contact_placement(m, q0, k) for k in range(2)]
    pos = np.tile(np.array([p for _, p in placements])[None], (n, 1, 1))
    rot = np.tile(np.array([R.reshape(9) for R, _ in placements])[None], (n, 1, 1))
    c.set_contact_schedule(contact_masks(P.grids, [0b11, 0b01, 0b11], [0b10]), pos, rot)
    c.set_constraint_bounds(np.concatenate([np.full(2 * nu, 2.5), np.full(2 * nu, 5.0), np.full(2 * nu, 60.0)]), 1.0e-3, ic.TAU)
    c.set_wrench_cone_params(np.array(ic.WRENCH_SOLES))
    wq = np.concatenate([np.full(6, 10.0), np.full(nu, 0.1)])
    c.set_configuration_cost(q0, np.zeros(nv), np.zeros(nu), wq, np.full(nv, 0.1), np.full(nv, 1e-3), np.full(nu, 1e-4), 10.0 * wq,
                             np.full(nv, 0.1), q_weight_impact=wq, v_weight_impact=np.full(nv, 0.1), dv_weight_impact=np.full(nv, 1e-3))
    c.set_initial_state(np.tile(np.concatenate([q0, np.zeros(nv)]), (batch, 1)))
    S = P.rec("sol")
    sol = np.zeros(c.shape("sol"))
    S.f(sol, "q")[..., :nq] = q0
    S.f(sol, "q")[..., 7:nq] += 0.05 * rng.uniform(-1, 1, (batch, n, nq - 7))
    for f, sc in (("v", 0.5), ("a", 1.0), ("u", 10.0), ("lmd", 0.5), ("gmm", 0.5), ("beta", 0.5), ("mu", 0.5), ("nu_passive", 0.5), ("xi", 0.5)):
        S.f(sol, f)[...] = sc * rng.uniform(-1, 1, S.f(sol, f).shape)
    w = np.concatenate([rng.uniform(-5, 5, (batch, n, 2, 2)), rng.uniform(100, 200, (batch, n, 2, 1)), rng.uniform(-1, 1, (batch, n, 2, 3))], axis=-1)
    S.f(sol, "f")[..., :12] = w.reshape(batch, n, 12)
    return dev, P, batch, _clean(P, "sol", "linearize", sol)


@pytest.mark.parametrize("kind", ir.POISONS)
@pytest.mark.parametrize("stage", ["init", "linearize"])
def test_contact_path_from_the_iterate_with_wrench_cones(stage, kind):
    """rtoc_contact_init_constraints and rtoc_contact_eval_kkt with the wrench-cone rows of iCub's soles: the wrench, mu and the 17
    rows of the sole in the air are stale."""
    dev, P, batch, sol = _icub_wrench_contact()
    c = dev.ctx
    try:
        c.upload(BUF_SOL, sol)
        c.upload(BUF_CON, np.zeros(c.shape("con")))
        c.contact_init_constraints()
        con = _clean(P, "con", stage, c.download_records(BUF_CON, "con"))

        def run(inp):
            c.clear_status()
            c.upload(BUF_SOL, inp["sol"])
            c.upload(BUF_CON, inp["con"])
            for nm in ("kkt", "cdd"):
                c.upload(BUFS[nm], np.zeros(c.shape(nm)))
            if stage == "init":
                c.contact_init_constraints()
                out = dev.records("con")
            else:
                c.contact_eval_kkt()
                out = dev.records("con", "kkt", "cdd")
                out["dx0"] = c.download(BUF_DX0, (batch, 2 * P.L.dims.nv))
            out["status"] = c.status()
            return out
        _iterate_check(P, run, dict(sol=sol, con=con), stage, kind, ("sol", "con"), ("con",))
    finally:
        dev.close()


def test_the_check_sees_a_read_of_the_iterate():
    """The harness on the stages that start from RTOC_BUF_SOL: a mask that wrongly calls the ACTIVE forces of grid point 4 inactive
    is reported with its name by the linearisation."""
    dev, P, batch, sol = _anymal_contact()
    c = dev.ctx
    try:
        c.upload(BUF_SOL, sol)
        c.upload(BUF_CON, np.zeros(c.shape("con")))
        c.contact_init_constraints()
        con = c.download_records(BUF_CON, "con")

        def run(inp):
            c.clear_status()
            c.upload(BUF_SOL, inp["sol"])
            c.upload(BUF_CON, con)
            c.contact_eval_kkt()
            return dev.records("kkt", "cdd")
        wrong = ir.input_inactive(P, "sol", "linearize")
        P.rec("sol").f(wrong[4], "f")[...] = True
        leaks = ir.find_leaks(P, run, dict(sol=sol), dict(sol=wrong), {}, "stale")
        assert len(leaks) == 1 and "sol.f[12 entries from 0] at grid point 4 (" in leaks[0], leaks
    finally:
        dev.close()
