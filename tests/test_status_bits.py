"""Every per-instance status bit (RTOC_STAT_*, include/rtoc.h) on every kernel path that raises it, and the isolation of the instance that
raised it: tests/status_cases.py makes one instance of a small batch exactly ill-posed at one grid point.

CPU leg (no GPU): every case through the oracle entry point that matches it -- the required bit on that instance, nothing outside
required | allowed on it, status 0 on every other instance, their output records bit-identical to the oracle's clean run.  A case the
oracle does not flag unambiguously does not belong in the table.

GPU leg: for each (kernel path, case) on a fresh context: clear_status, the clean batch, its status all zero, its output records
downloaded; then the ill-posed batch through the same call -- (a) the required bit on the instance, (b) no bit outside required |
allowed on it, (c) status 0 on the others, (d) the others' records bit-identical to the clean run; then the clean batch WITHOUT
clear_status: the same status words (the bits are sticky, a clean call neither clears nor adds one) and every record of the clean run;
then (e) clear_status and the clean batch again: all zero and bit-identical to the first run (neither a stale flag nor stale scratch
may leak into the next call).  What the ill-posed instance's own records hold is unspecified.  No tolerance anywhere: bit tests and
exact equality against the same kernel's clean run (tests/test_determinism.py: the kernels repeat bit for bit).

How a path is selected (rtoc::plan_backward, rt_sweep.hip; launch_condense, rt_condense.hip) is in PATHS below.

What a dropped `stat |=` line does to these tests (each line replaced by a no-op in a scratch build of the library, this module run
against it).  Noticed line by line: riccati_sc_block.inc:52 (phiu-row on the tile-split and both role-split paths),
condense_mjtjinv.inc:80 (every dCda case of the three ANYmal pipelines), condense_mjtjinv.inc:28 (the flight cases: with contacts LLT(J
M^-1 J^T) fails after LLT(dIDda) did and raises the same bit), riccati_backward.hpp:762 (lu-nan on the tile-split path and the scan),
riccati_backward_rv.hpp:897 and :985, riccati_backward_rs.hpp:770, riccati_backward_rw.hpp:387 (lu-nan) and :427 (qxu-nan0),
riccati_backward_rw2.hpp:487, condense_mjtjinv.inc:39 (the iCub flight case), unconstr_riccati.hpp:265 and :333.  Not noticed:
riccati_backward_rv.hpp:944 (m of the switching constraint: whatever makes m NaN makes k of the same grid point NaN, which :985
reports).  Not noticed line by line, by
construction: the scans factorise every grid point twice -- in the element / preparation kernels (riccati_scan_core.hpp:372-373,
riccati_scan_sto.hpp:141, 203) and again in the policy pass of riccati_backward_kernel (its own LLT(Quu), riccati_sc_block.inc:52) --
and check k and m in the vector pass (riccati_scan_sto.hpp:609, 633) next to the policy pass's own check; an exactly ill-posed record
fails both, so either line alone still raises the bit.  With both members of a pair dropped every scan case of that bit fails.
riccati_scan_core.hpp:724 (the flag of a combination step) was not noticed either: in every case here the policy pass, which works on
the combined values, raises RTOC_STAT_NAN by itself.  riccati_backward.hpp:781 and :598 need nu > 32, which no compiled shape has."""
import numpy as np
import pytest

import status_cases as sc
from robotoc_amd.types import (BUF_CDD, BUF_CON, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP, OPT_BACKWARD_WAVES, STAT_M_NOT_SPD,
                               Records)

# ---------------------------------------------------------------- CPU leg ----


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_oracle_flags_the_instance_alone(oracle, case):
    clean = sc.clean_inputs(case, oracle.layout)[3]
    st0, out0 = sc.run_oracle(oracle, case, clean, oracle.layout)
    assert not st0.any(), st0
    for v in out0.values():
        assert np.isfinite(v).all()
    with np.errstate(all="ignore"):
        st, out = sc.run_oracle(oracle, case, sc.corrupted_inputs(case, oracle.layout), oracle.layout)
    print("%s: oracle status %s" % (case.name, [hex(int(s)) for s in st]))
    sc.check_isolated(case, st, out, out0, "oracle")


def test_every_case_is_used_by_a_kernel_path():
    used = {name for p in PATHS.values() for name in p["cases"]}
    assert used == set(sc.BY_NAME), set(sc.BY_NAME) ^ used


# ---------------------------------------------------------------- GPU leg ----

def _names(config, *kinds):
    return ["%s-%s" % (config, k) for k in kinds]


SWEEP = ("quu", "lu-nan", "qxu-nan0", "pres-nan", "phiu-row")
CONDENSE = (_names("trot8", "dIDda", "dCda-contact", "dCda-lift") + _names("trot20", "dCda-impact", "dIDda-impact")
            + ["jump_sto-dIDda-flight"])
CONDENSE_ICUB = _names("icub35", "dIDda", "dCda-contact", "dCda-impact", "dIDda-impact", "dIDda-flight")

# setup: options set on the fresh context (in this order); call: the entry points run; structured: the plan takes the intended kernel
# only if the records pass the Fxx structure check, which the test then asserts (rtoc_check_fxx_structure).
#
# ANYmal (shape 18:12:12, tile-split variants of 1 and 3 waves, role-split variant 2 = two waves, variant 3 = four instances per
# workgroup, the default): an explicit RTOC_OPT_BACKWARD_WAVES other than the default's keeps its kernel (plan_backward: `reg` needs
# bwd_variant == default), so waves = 3 can only be riccati_backward_kernel and waves = 2 only riccati_backward_rs_kernel.  The default
# plan of this shape is the register kernel (RTOC_OPT_BACKWARD_REGISTER defaults to 1): with the option 0 and the default variant the
# plan is BWD_TILE with the four-instance role-split kernel, structured or not.  With the option 1, at most RV_MAX_STAGES grid points and
# no writeback it is BWD_RV; on a grid with switching-time optimisation its STO instantiation, if the records are structured.
# iCub (35:29:12 and 32:26:12: two tile-split variants, no register-resident kernel): the default plan is the tile-split kernel while
# batch <= the number of CUs; RTOC_OPT_BACKWARD_REGISTER = 2 takes the register-wide kernel (nv = 32: riccati_backward_rw.hpp, nv = 35:
# riccati_backward_rw2.hpp) at every batch size if the records are structured, with the switching-constraint grid point as a one-stage
# launch of the tile-split kernel (launch_backward_rw).  RTOC_OPT_BACKWARD_SCAN = 1 comes first in the plan whatever else is set; on
# a grid with switching-time optimisation of at most SCAN_STO_MAX_STAGES grid points it is the scan of riccati_scan_sto.hpp.
# rtoc_riccati_sweep with RTOC_OPT_SWEEP_CHUNKS = 2 at batch 6: chunks of ((6 + 1) / 2 + 3) & ~3 = 4 and 2 instances; instance 1
# shares its chunk with 0, 2, 3, and under the four-instance kernel its workgroup too.
# iiwa14: rtoc_unconstr_backward takes unconstr_riccati.hpp unless RTOC_OPT_UNCONSTR_DENSE, then the fill kernel and the plan above;
# nv = 7 is the register kernel of that header, the 12-joint arm (a plug-in shape, tests/test_unconstr_arm_sizes.py) its LDS kernel.
# Condensation (launch_condense): RTOC_OPT_CONDENSE_SPLIT = 1 is mjtjinv_kernel + condense_kernel<split>; with it 0,
# RTOC_OPT_CONDENSE_REGISTER = 1 is condense_rv_kernel on the contact grid points and condense_kernel on the impacts (the shape's
# default), 0 is condense_kernel alone.  All with RTOC_OPT_CONTACT_INV_DAMPING = 0: the zero row gives an exactly zero pivot.
PATHS = {
    "tile-anymal": dict(setup=[("set_backward_waves", 3)], options={OPT_BACKWARD_WAVES: 3}, call="backward+forward",
                        cases=_names("trot20", *SWEEP)),
    "tile-icub32": dict(setup=[], call="backward+forward", cases=_names("icub32", *SWEEP)),
    "tile-icub35": dict(setup=[], call="backward+forward", cases=_names("icub35", *SWEEP)),
    "role-split": dict(setup=[("set_backward_waves", 2)], options={OPT_BACKWARD_WAVES: 2}, call="backward+forward",
                       cases=_names("trot20", *SWEEP)),
    "role-split-4": dict(setup=[("set_backward_register", False)], options={OPT_BACKWARD_WAVES: 8}, call="backward+forward",
                         cases=_names("trot20", *SWEEP)),
    "rv": dict(setup=[("set_backward_register", True)], call="backward+forward", cases=_names("trot20", *SWEEP)),
    "rv-sto": dict(setup=[("set_backward_register", True)], call="backward+forward", structured=True,
                   cases=_names("jump_sto", *SWEEP)),
    "rw": dict(setup=[("set_backward_register", 2)], call="backward+forward", structured=True, cases=_names("icub32", *SWEEP)),
    "rw2": dict(setup=[("set_backward_register", 2)], call="backward+forward", structured=True, cases=_names("icub35", *SWEEP)),
    "scan": dict(setup=[("set_backward_scan", True)], call="backward+forward", cases=_names("trot20", *SWEEP)),
    "scan-sto": dict(setup=[("set_backward_scan", True)], call="backward+forward", cases=_names("jump_sto", *SWEEP)),
    "chunks-rv": dict(setup=[("set_backward_register", True), ("set_sweep_chunks", 2)], call="sweep",
                      cases=[c + "-batch6" for c in _names("trot20", *SWEEP)]),
    "chunks-role-split-4": dict(setup=[("set_backward_register", False), ("set_sweep_chunks", 2)], call="sweep",
                                cases=[c + "-batch6" for c in _names("trot20", *SWEEP)]),
    "unconstr": dict(setup=[("set_unconstr_dense", False)], call="unconstr", cases=["iiwa14-quu", "iiwa14-lu-nan"]),
    "unconstr-dense": dict(setup=[("set_unconstr_dense", True)], call="unconstr", cases=["iiwa14-quu", "iiwa14-lu-nan"]),
    "unconstr-lds": dict(setup=[("set_unconstr_dense", False)], call="unconstr", plugin=(12, 12, 0), cases=["arm12-quu", "arm12-lu-nan"]),
    "condense": dict(setup=[("set_condense_register", False), ("set_condense_split", False), ("set_contact_inv_damping", 0.0)],
                     call="condense", cases=CONDENSE),
    "condense-split": dict(setup=[("set_condense_split", True), ("set_contact_inv_damping", 0.0)], call="condense",
                           cases=CONDENSE),
    "condense-register": dict(setup=[("set_condense_register", True), ("set_condense_split", False), ("set_contact_inv_damping", 0.0)],
                              call="condense", cases=CONDENSE),
    "condense-icub": dict(setup=[("set_contact_inv_damping", 0.0)], call="condense", cases=CONDENSE_ICUB),
    "condense-icub-split": dict(setup=[("set_condense_split", True), ("set_contact_inv_damping", 0.0)], call="condense",
                                cases=CONDENSE_ICUB),
}
GPU_CASES = [(p, c) for p, spec in PATHS.items() for c in spec["cases"]]


def _run(ctx, spec, inp, clear=True):
    if clear:
        ctx.clear_status()
    ctx.upload(BUF_KKT, inp["kkt"])
    ctx.upload(BUF_DX0, inp["dx0"])
    if spec["call"] == "condense":
        ctx.upload(BUF_CDD, inp["cdd"])
        ctx.condense()
        return ctx.status(), dict(kkt=ctx.download_records(BUF_KKT, "kkt"), cdd=ctx.download_records(BUF_CDD, "cdd"))
    if spec["call"] == "sweep":
        ctx.riccati_sweep()
    elif spec["call"] == "unconstr":
        ctx.unconstr_backward(sc.IIWA_DT)
        ctx.unconstr_forward(sc.IIWA_DT)
    else:
        ctx.riccati_backward()
        ctx.riccati_forward()
    return ctx.status(), dict(ric=ctx.download_records(BUF_RIC, "ric"), dir=ctx.download_records(BUF_DIR, "dir"))


def _same_bits(a, b):
    return bool((a.view(np.int64) == b.view(np.int64)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("path,name", GPU_CASES, ids=["%s:%s" % pc for pc in GPU_CASES])
def test_kernel_flags_the_instance_alone(path, name):
    from robotoc_amd import capi
    spec, case = PATHS[path], sc.BY_NAME[name]
    if "plugin" in spec:
        capi.build_plugin(*spec["plugin"])
    dims, grids, _, clean = sc.clean_inputs(case, capi.layout_for)
    bad = sc.corrupted_inputs(case, capi.layout_for)
    ctx = capi.Context(dims, len(grids), case.batch, 0)
    try:
        ctx.set_grid(grids)
        for method, value in spec["setup"]:
            getattr(ctx, method)(value)
        for option, value in spec.get("options", {}).items():
            assert ctx.get_option(option) == value, (option, ctx.get_option(option))
        st0, out0 = _run(ctx, spec, clean)
        assert not st0.any(), [hex(int(s)) for s in st0]
        if spec.get("structured"):
            assert ctx.check_fxx_structure()
        st, out = _run(ctx, spec, bad)
        print("%s %s: status %s" % (path, name, [hex(int(s)) for s in st]))
        sc.check_isolated(case, st, out, out0, path)                     # (a) - (d)
        if spec.get("structured"):
            assert ctx.check_fxx_structure()
        st1, out1 = _run(ctx, spec, clean, clear=False)                  # sticky: a clean call in between neither clears nor adds a bit
        assert (st1 == st).all(), "%s %s: status %s after a clean batch without rtoc_clear_status" % (path, name, [hex(int(s)) for s in st1])
        for k in out0:
            assert _same_bits(out1[k], out0[k]), "%s %s: %s of the clean batch differs right after the ill-posed run" % (path, name, k)
        st2, out2 = _run(ctx, spec, clean)                               # (e)
        assert not st2.any(), "%s %s: status %s after rtoc_clear_status and a clean batch" % (path, name, [hex(int(s)) for s in st2])
        for k in out0:
            assert _same_bits(out2[k], out0[k]), "%s %s: %s of the clean batch differs after the ill-posed run" % (path, name, k)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_newton_iteration_keeps_an_ill_posed_instance_to_itself():
    """rtoc_newton_iteration on the problem of tests/test_newton_iteration.py at its batch (6): instance 3's dIDda = -I at a contact
    grid point, in the linearised records the iteration starts from.  RTOC_STAT_M_NOT_SPD on instance 3 alone; every other instance's
    direction, constraint data, solution, step sizes and KKT error bit-identical to the clean iteration's; the converged count that of
    the clean iteration, which does not count instance 3 (its KKT error, taken before the condensation, is above the tolerance).  The
    step-size minimum, the converged mask and its counter are where the instances of this call meet."""
    from test_newton_iteration import _context
    batch, tau, bad_b, gp = 6, 0.995, 3, 3
    others = [b for b in range(batch) if b != bad_b]
    runs = {}
    for which in ("clean", "bad"):
        ctx, _ = _context(batch)
        try:
            L = ctx.L
            err = ctx.kkt_error()
            tol = float(np.sort(err)[batch // 2 - 1]) * (1 + 1e-12)
            assert 0 < (err < tol).sum() < batch and not err[bad_b] < tol
            if which == "bad":
                cdd = ctx.download_records(BUF_CDD, "cdd")
                Records(L, "cdd").f(cdd[bad_b, gp], "dIDda")[...] = -np.eye(L.dims.nv)
                ctx.upload(BUF_CDD, cdd)
            ctx.clear_status()
            ctx.newton_iteration(tol, tau)
            runs[which] = dict(status=ctx.status(), nconv=ctx.converged_count(), expected=int((err < tol).sum()),
                               steps=ctx.download(BUF_STEP, (batch, 2)), dir=ctx.download_records(BUF_DIR, "dir"),
                               con=ctx.download_records(BUF_CON, "con"), sol=ctx.download_records(BUF_SOL, "sol"),
                               kkt_error=ctx.kkt_error())
        finally:
            ctx.close()
    clean, bad = runs["clean"], runs["bad"]
    assert not clean["status"].any() and clean["nconv"] == clean["expected"]
    st = bad["status"]
    assert st[bad_b] & STAT_M_NOT_SPD and not st[others].any(), [hex(int(s)) for s in st]
    assert bad["nconv"] == clean["nconv"]
    for k in ("steps", "dir", "con", "sol", "kkt_error"):
        assert _same_bits(np.ascontiguousarray(bad[k][others]), np.ascontiguousarray(clean[k][others])), k
