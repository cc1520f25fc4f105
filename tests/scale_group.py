"""The group of power-of-two rescalings under which the solve-side algorithm is EXACTLY equivariant, and the cases on which
tests/test_scale_equivariance.py (the CPU oracle) and tests/test_scale_equivariance_gpu.py (every kernel path) hold it.

An element is (c, a, u, r): cost scale, state scale, control scale, constraint-row scale.  x' = a x, u' = u u, the cost times c,
every switching-constraint row times r.  Multiplying by 2^k is exact in binary floating point, and sqrt(4^k d) = 2^k sqrt(d) bit
for bit, so with c a power of FOUR and a, u, r powers of two, uniform over all components, every sum, product, quotient and
square root of the recursion sees operands whose mantissas are those of the unit problem: the result is the unit result times
the field's factor, with identical mantissas, as long as nothing over- or underflows.  (A per-component scaling would change
pivot and summation decisions and is no exact symmetry; c = 2 puts an odd exponent under the Cholesky square roots and is the
control of tests/test_scale_equivariance.py.)

The factor tables stand here once; the oracle confirms every entry (tests/test_scale_equivariance.py)."""
import collections

import numpy as np

from robotoc_amd import problems as pr
from robotoc_amd.types import GRID_IMPACT, Records

Element = collections.namedtuple("Element", "c a u r")


def element(c4=0, a2=0, u2=0, r2=0):
    """c = 4^c4, a = 2^a2, u = 2^u2, r = 2^r2 -- exact in float64"""
    return Element(float(np.ldexp(1.0, 2 * c4)), float(np.ldexp(1.0, a2)), float(np.ldexp(1.0, u2)), float(np.ldexp(1.0, r2)))


IDENTITY = element()
# the elements of the GPU tests: 2 seeds x 4 elements = 8 instances of one launch, each on its own magnitudes
ELEMENTS = (IDENTITY, element(10), element(-12, 7, -5, 9), element(20, -11, 6, 3))
# grids with switching-time optimisation: c >= 1 only.  The STOPolicy's regularisation tests sgm = xi - 2 chi + rho (factor c)
# against sqrt(DBL_EPSILON), in the reference as here; below unit cost scale a positive sgm can cross it.
ELEMENTS_STO = (IDENTITY, element(10), element(6, 3, -2, 5), element(20, -11, 6, 3))
# the fixed-base arm path: the control is the acceleration and enters the state equation as v+ = v + dt a with dt an ARGUMENT of
# the call, not a block of the record -- B = dt I cannot take the factor a/u, so the subgroup is a = u (r has nothing to act on)
ELEMENTS_UNCONSTR = (IDENTITY, element(10), element(-12, 7, 7), element(20, -11, -11))
# the pre-condensation path: the cost scale alone
ELEMENTS_COST = (IDENTITY, element(9), element(-9), element(20))
CONTROL = Element(2.0, 1.0, 1.0, 1.0)   # NOT in the group: must break the equality


def kkt_factors(e):
    c, a, u, r = e
    return dict(Fxx=1.0, Fvu=a / u, Fx=a, fx=a, Qxx=c / (a * a), Qxu=c / (a * u), Quu=c / (u * u), lx=c / a, hx=c / a, lu=c / u, hu=c / u,
                scal=c, Phix=r / a, Phiu=r / u, Phit=r, Pres=r)


def ric_factors(e):
    c, a, u, r = e
    scal = np.array([c, c, c, c, c, 1.0, 1.0, 1.0])   # xi, chi, rho, eta, iota | dtsdts, dts0, (unused)
    return dict(P=c / (a * a), s=c / a, Psi=c / a, Phi=c / a, psi_x=c / a, phi_x=c / a, psi_u=c / u, phi_u=c / u, scal=scal, K=u / a,
                k=u, T=u, W=u, M=c / (r * a), m=c / r, mt=c / r, mt_next=c / r, dtsdx=1.0 / a)


def dir_factors(e):
    c, a, u, r = e
    # daf, dbetamu, dnu_passive: the expansion's outputs, defined under the cost scale only (a = u = 1)
    return dict(dx=a, du=u, dlmdgmm=c / a, dxi=c / r, dts=1.0, daf=1.0, dbetamu=c, dnu_passive=c)


def _cost_only(e):
    assert e.a == e.u == e.r == 1.0, "the pre-condensation records are equivariant under the cost scale only"
    return e.c


def precondense_kkt_factors(e):
    c = _cost_only(e)
    return dict(Fxx=1.0, Fvu=1.0, Fx=1.0, fx=1.0, Phix=1.0, Phiu=1.0, Phit=1.0, Pres=1.0,
                Qxx=c, Qxu=c, Quu=c, lx=c, lu=c, hx=c, hu=c, scal=c)


def cdd_factors(e):
    c = _cost_only(e)
    f = dict(dIDda=1.0, dIDCdqv=1.0, dCda=1.0, IDC=1.0, Phia=1.0, MJtJinv=1.0, MJtJinv_dIDCdqv=1.0, MJtJinv_IDC=1.0)
    f.update({name: c for name in ("Qaa", "Qff", "Qqf", "la", "lf", "ha", "hf", "lu_passive", "Qafqv", "Qafu_full", "laf", "Qxu_passive",
                                   "Quu_passive_topRight", "haf")})
    return f


def con_factors(e):
    """Box, friction-cone and wrench-cone rows alike: g(x) + slack = 0 has no cost in it, the dual is a multiplier of the cost.
    cmpl = slack * dual - barrier takes c with the barrier (set_barrier_param) scaled by c as well; cond = (dual * residual - cmpl)
    / slack and ddual = -(dual * dslack + cmpl) / slack follow."""
    c = _cost_only(e)
    return dict(slack=1.0, dual=c, residual=1.0, cmpl=c, cond=c, dslack=1.0, ddual=c)


def sol_factors(e):
    c = _cost_only(e)
    return dict(q=1.0, v=1.0, a=1.0, u=1.0, f=1.0, lmd=c, gmm=c, beta=c, mu=c, nu_passive=c, xi=c)


FACTORS = dict(kkt=kkt_factors, ric=ric_factors, dir=dir_factors, cdd=cdd_factors, con=con_factors, sol=sol_factors,
               kkt_pre=precondense_kkt_factors)


RECORD_OF = dict(kkt_pre="kkt", cdd_unconstr="cdd")   # factor tables that are another reading of a record kind


def factors(which, e):
    """{field: factor} of every field of a record kind under element e ("kkt_pre": the KKT record before the condensation)"""
    return FACTORS[which](e)


def scale(L, which, arr, e):
    """A copy of the records arr ([..., stride]) with every field times its factor (padding between fields untouched)."""
    rec = Records(L, RECORD_OF.get(which, which))
    out = np.array(arr, dtype=np.float64, copy=True)
    for f, k in factors(which, e).items():
        v = rec.f(out, f)
        v[...] = v * k
    return out


def scale_dx0(dx0, e):
    return np.asarray(dx0) * e.a


def scale_cone(cone, e):
    """Friction-cone (dg_dq, dg_df) and wrench-cone records hold Jacobians of g alone: factor 1 under the cost scale."""
    _cost_only(e)
    return np.array(cone, copy=True)


def batch_of(elements, unit, scale_one):
    """unit: [seeds, ...]; returns [seeds * len(elements), ...] with instance s * len(elements) + j = scale_one(unit[s], elements[j])"""
    return np.ascontiguousarray(np.stack([scale_one(unit[s], e) for s in range(unit.shape[0]) for e in elements]))


# ---- which fields of which grid point count: exactly what helpers.compare_riccati / compare_direction look at ----
def riccati_fields(grids, i, check_sto=True):
    """[(field, leading rows or None)]"""
    g, N = grids[i], len(grids) - 1
    out = [("P", None), ("s", None)]
    if i < N and g.type != GRID_IMPACT:
        out += [("K", None), ("k", None)]
    if i < N and g.dims > 0:
        out += [("M", g.dims), ("m", g.dims)]
    if check_sto and i < N and g.sto:
        out += [("Psi", None), ("Phi", None)]
        if g.type != GRID_IMPACT:
            out += [("T", None), ("W", None), ("psi_x", None), ("psi_u", None)]
            if g.dims > 0:
                out += [("mt", g.dims), ("mt_next", g.dims)]
        out.append(("scal", 5))
    return out


def direction_fields(grids, i, dts=True):
    """dts = False: the fixed-base path, which has no switching times and leaves dts unwritten (tests/inactive_regions.py)"""
    g, N = grids[i], len(grids) - 1
    out = [("dx", None), ("dlmdgmm", None)]
    if i < N and g.type != GRID_IMPACT:
        out.append(("du", None))
    if i < N and g.switching_constraint and g.dims > 0:
        out.append(("dxi", g.dims))
    if dts:
        out.append(("dts", 2))
    return out


def sto_policy_stages(grids):
    """The records that hold an STOPolicy {dtsdx, dtsdts, dts0} (riccati_recursion.cpp:32-80 as oracle/rtoc_oracle.c restates
    it): the impact point, the lift point or point 0 of a phase transition whose next switching time is free too."""
    from robotoc_amd.types import GRID_LIFT
    N, out = len(grids) - 1, set()
    for i in range(N):
        g = grids[i]
        if g.type == GRID_IMPACT:
            if ((i > 0 and grids[i - 1].sto) or g.sto) and g.sto_next:
                out.add(i)
        elif grids[i + 1].type == GRID_LIFT and g.sto_next:
            out.add(i + 1)
    if grids[0].sto and grids[0].sto_next:
        out.add(0)
    return sorted(out)


def sto_policy_mismatches(L, grids, ric, elements, what=""):
    """dtsdx (1 / a), dtsdts and dts0 (1) of every STOPolicy"""
    stages = sto_policy_stages(grids)
    assert stages, "no phase transition with a policy on this grid"
    return batch_mismatches(Records(L, "ric"), ric[:, stages], elements, fields=["dtsdx", ("scal", slice(5, 7))], what=what + " policy (stages %s)" % stages)


def _worst_rel(x, y):
    with np.errstate(all="ignore"):
        den = np.maximum(np.abs(x), np.abs(y))
        d = np.where(den > 0, np.abs(x - y) / den, 0.0)
        d = np.where(np.isnan(x) != np.isnan(y), np.inf, np.nan_to_num(d, nan=0.0))
    return float(d.max()) if d.size else 0.0


def mismatches(records, unit, scaled, e, grids=None, fields=None, what="", check_sto=True):
    """The fields in which `scaled` is not bit for bit `unit` times the field's factor under e (NaN positions included).
    records: Records(L, kind); unit, scaled: [stages, stride] of ONE instance (or [stride] with fields given).
    grids given (kind "ric" / "dir"; check_sto = False on "dir": without dts): per grid point the fields compare_riccati / compare_direction look at; otherwise `fields`
    (names, or (name, leading rows)) on every leading index.  Returns [(what, stage, field, worst relative difference)]."""
    fac = factors(records.which, e)
    bad = []

    def one(stage, u_rec, s_rec, f, rows):
        k = fac[f]
        x, y = records.f(u_rec, f), records.f(s_rec, f)
        if rows is not None:
            sel = rows if isinstance(rows, slice) else slice(0, rows)   # one record: rows of a matrix, entries of a vector
            x, y = x[sel], y[sel]
            if np.ndim(k):
                k = k[sel]
        x = x * k
        if not np.isfinite(x).all():   # (a record nobody wrote is NaN in both: equal, and no evidence)
            bad.append((what, stage, f + " of the unit instance is not finite", np.inf))
        elif not np.array_equal(x, y, equal_nan=True):
            bad.append((what, stage, f, _worst_rel(x, y)))
    if grids is not None:
        per_stage = riccati_fields if records.which == "ric" else direction_fields
        for i in range(len(grids)):
            args = (grids, i, check_sto)
            for f, rows in per_stage(*args):
                one(i, unit[i], scaled[i], f, rows)
    else:
        for item in fields:
            f, rows = item if isinstance(item, tuple) else (item, None)
            if unit.ndim == 1:
                one(None, unit, scaled, f, rows)
            else:
                for i in range(unit.shape[0]):
                    one(i, unit[i], scaled[i], f, rows)
    return bad


def assert_equivariant(records, unit, scaled, e, grids=None, fields=None, what="", check_sto=True):
    bad = mismatches(records, unit, scaled, e, grids=grids, fields=fields, what=what, check_sto=check_sto)
    assert not bad, report(bad)


def batch_mismatches(records, arr, elements, grids=None, fields=None, what="", check_sto=True):
    """arr: the records of a batch laid out by batch_of; every scaled copy against the identity instance of its seed."""
    assert elements[0] == IDENTITY
    bad, ne = [], len(elements)
    for b in range(arr.shape[0]):
        s, j = divmod(b, ne)
        if j:
            bad += mismatches(records, arr[s * ne], arr[b], elements[j], grids=grids, fields=fields, check_sto=check_sto,
                              what="%s inst %d (seed %d, c=2^%d a=2^%d u=2^%d r=2^%d)" % ((what, b, s) + tuple(int(np.log2(v)) for v in elements[j])))
    return bad


def report(bad):
    return "%d fields are not the unit result times their factor, bit for bit (what, stage, field, worst relative difference):\n%s" % (
        len(bad), "\n".join("  %s: stage %s %s %.3e" % b for b in bad))


# ---- the cases, shared by the CPU oracle test and the GPU tests ----------------------------------------------------------------
SEEDS = 2
# the shortest words of tests/grid_words.py that between them hold every kind (R regular, C constrained, L lift, Lc constrained
# lift, I impact) in every neighbourhood a five-point horizon allows; no adjacent constraints (`R C C` has
# ||P|| ~ 1e11 at unit scale)
WORDS = (("C",), ("R", "L"), ("R", "Lc"), ("R", "I", "R"), ("C", "I", "Lc", "R"))
MODES = ("dynamics", "factory")


def long_horizon(shape):
    """(dims, grids) of the one longer horizon of a shape: the phase transitions and the scan's combination levels run"""
    import grid_words as gw
    if shape == "anymal":
        dims, grids, _ = pr.config_anymal_trot(N=12, dt=0.05)
    else:
        dims, grids, _ = pr.config_icub_jump(nv=gw.SHAPES[shape][0].nv)
        for g in grids:
            g.sto = g.sto_next = 0
    return dims, grids


def sweep_grids(shape):
    """[(name, grids)] of a shape of tests/grid_words.py: the words and the longer horizon"""
    import grid_words as gw
    return [(gw.name(w), gw.build(w, gw.SHAPES[shape][1])) for w in WORDS] + [("long", long_horizon(shape)[1])]


def sweep_inputs(L, grids, mode, elements=ELEMENTS, filler=None):
    """(kkt, dx0) of SEEDS x len(elements) instances: problems.make_kkt_batch / make_dx0 of SEEDS seeds, each under every element"""
    if filler is None:
        kkt = pr.make_kkt_batch(L, grids, SEEDS, mode=mode)
    else:
        kkt = Records(L, "kkt").zeros(SEEDS, len(grids))
        for b in range(SEEDS):
            filler(L, len(grids), kkt[b], np.random.default_rng(pr.BASE_SEED + b))
    dx0 = pr.make_dx0(L, SEEDS)
    return (batch_of(elements, kkt, lambda k, e: scale(L, "kkt", k, e)), batch_of(elements, dx0, scale_dx0))


def sweep_mismatches(L, grids, ric, d, elements=ELEMENTS, what="", check_sto=True, dts=True):
    return (batch_mismatches(Records(L, "ric"), ric, elements, grids=grids, what=what, check_sto=check_sto)
            + batch_mismatches(Records(L, "dir"), d, elements, grids=grids, what=what, check_sto=dts))


# the fixed-base arm path: iiwa14 (the register form of the structured recursion) and the nine-joint chain of tests/arm_models.py
# (the smallest and an odd size of its LDS form)
UNCONSTR_SIZES, UNCONSTR_STEPS, UNCONSTR_DT = (7, 9), 6, 0.05

def unconstr_cdd_factors(e):
    """rtoc_unconstr_condense's convention (robotoc_amd/csrc/record_view.hpp): CDD.Qaa = diag Quu and CDD.la = lu of the torque
    cost, the full torque Hessian in the MJtJinv field -- all cost; the inverse-dynamics derivatives and ID carry none"""
    f = cdd_factors(e)
    f["MJtJinv"] = _cost_only(e)
    return f


FACTORS["cdd_unconstr"] = unconstr_cdd_factors


# ---- whole records under a mask: the pipeline condense -> sweep -> expand -> update -> integrate ----
def factor_row(L, which, e):
    """[stride]: the factor of every double of a record (1 on the alignment doubles between fields)"""
    rec = Records(L, RECORD_OF.get(which, which))
    row = np.ones(rec.stride)
    for f, k in factors(which, e).items():
        v = rec.f(row, f)
        v[...] = (k if np.ndim(k) == 0 else k.reshape(v.shape))
    return row


def con_active_mask(P):
    """[n, stride]: every field of the constraint record on the rows that exist at a grid point -- the box rows from their level
    on, the cone rows of the active contacts (tests/inactive_regions.py).  The rows of a wrench-cone contact that is not active
    hold the reference's constants (cond = 0, dslack = ddual = 1), which carry no factor, and stay out."""
    N = Records(P.L, "con")
    m = np.zeros((P.n, N.stride), dtype=bool)
    for i in range(P.n):
        rows = [r for r in range(len(P.rows)) if P.box_row_active(r, i)]
        rows += list(range(P.cone_row0(), P.cone_row0() + P.cone_rows * P.active_cone_contacts(i)))
        for f in N.names:
            N.f(m[i], f)[rows] = True
    return m


def masked_mismatches(P, buf, arr, mask, elements, which=None, what=""):
    """arr [batch, n, stride] laid out by batch_of, mask [n, stride] of the doubles that count: every scaled copy against the
    identity instance of its seed times factor_row.  One entry per (instance, grid point, field)."""
    import inactive_regions as ir
    assert elements[0] == IDENTITY and mask.any()
    names = ir.column_fields(P, buf)
    bad, ne = [], len(elements)
    for b in range(arr.shape[0]):
        s, j = divmod(b, ne)
        if not j:
            continue
        x, y = arr[s * ne] * factor_row(P.L, which or buf, elements[j])[None, :], arr[b]
        ne_ = mask & ~((x == y) | (np.isnan(x) & np.isnan(y)))
        ne_ |= mask & ~np.isfinite(x)   # (a record nobody wrote is NaN in both: equal, and no evidence)
        for i in np.nonzero(ne_.any(axis=1))[0]:
            for f in dict.fromkeys(names[ne_[i]].tolist()):
                sel = ne_[i] & (names == f)
                bad.append(("%s %s inst %d (seed %d, c=2^%d)" % (what, buf, b, s, int(np.log2(elements[j].c))), int(i), f,
                            _worst_rel(x[i][sel], y[i][sel])))
    return bad


def per_instance_mismatches(name, arr, elements, what=""):
    """step sizes and status words: identical across the copies of a seed"""
    bad, ne = [], len(elements)
    for b in range(arr.shape[0]):
        s, j = divmod(b, ne)
        if j and not np.array_equal(arr[b], arr[s * ne]):
            bad.append(("%s inst %d (seed %d): %s vs %s of the unit instance" % (what, b, s, arr[b], arr[s * ne]), None, name,
                        _worst_rel(np.asarray(arr[b], dtype=float), np.asarray(arr[s * ne], dtype=float))))
    return bad


PIPELINE_TAU = 0.995
FRICTION_CONTACTS, WRENCH_CONTACTS = 4, 2


def anymal_pipeline_problem(layout_for, impact_cones=True):
    """ANYmal trot, 12 intervals: the 72 joint-limit rows, the 24 acceleration-limit rows and the friction cones of four feet"""
    import inactive_regions as ir
    from robotoc_amd.types import anymal_dims, joint_limit_rows
    dims = anymal_dims(nc_max=120)   # 96 box rows + 20 cone rows, padded
    _, grids, _ = pr.config_anymal_trot(N=12, dt=0.05)
    return dims, ir.Problem(layout_for(dims), grids, joint_limit_rows(dims, acceleration=True), FRICTION_CONTACTS, 3, impact_cones=impact_cones)


def icub_pipeline_problem(layout_for):
    """iCub (nv = 35), joint-limit rows and the 17 wrench-cone rows of each foot, one foot in the air after the lift"""
    import inactive_cases as ic
    dims, P, _ = ic.icub_wrench_case(layout_for)
    return dims, P


def pipeline_inputs(P, elements=ELEMENTS_COST):
    """Pre-condensation records, constraint rows, cone Jacobians, dx0 and an iterate of SEEDS seeds, each under every element"""
    import inactive_regions as ir
    from robotoc_amd.types import VAR_A
    L, grids = P.L, P.grids
    kkt, cdd = pr.make_precondense_batch(L, grids, SEEDS)
    con = pr.make_constraint_batch(L, grids, SEEDS)
    N = Records(L, "con")
    # acceleration rows that matter next to Qaa ~ O(1) (tests/test_acceleration_limits.py): dual / slack of the same order
    a_rows = [r for r, w in enumerate(P.rows) if w.var == VAR_A]
    N.f(con, "dual")[..., a_rows] *= 256.0
    N.f(con, "cmpl")[...] = N.f(con, "slack") * N.f(con, "dual") - 1.0e-3
    if P.cone_rows == ir.WRENCH_ROWS:
        import inactive_cases as ic
        from oracle import oracle as orc
        cone = pr.make_wrench_cone_batch(L, grids, SEEDS, P.cone_contacts, [orc.wrench_cone_matrix(*s) for s in ic.WRENCH_SOLES])
    else:
        cone = pr.make_cone_batch(L, grids, SEEDS, P.cone_contacts)
    rng = np.random.default_rng(17)
    sol = rng.uniform(-1, 1, (SEEDS, P.n, L.sol.stride))
    sol[:, ir.input_inactive(P, "sol", "integrate")] = 0.0
    o = L.sol.off[0]
    sol[..., o + 3:o + 7] /= np.linalg.norm(sol[..., o + 3:o + 7], axis=-1, keepdims=True)   # q on the manifold
    return dict(kkt=batch_of(elements, kkt, lambda k, e: scale(L, "kkt_pre", k, e)),
                cdd=batch_of(elements, cdd, lambda k, e: scale(L, "cdd", k, e)),
                con=batch_of(elements, con, lambda k, e: scale(L, "con", k, e)),
                cone=batch_of(elements, cone, scale_cone),
                dx0=batch_of(elements, pr.make_dx0(L, SEEDS), scale_dx0),
                sol=batch_of(elements, sol, lambda k, e: scale(L, "sol", k, e)))


def pipeline_mismatches(P, out, elements=ELEMENTS_COST, what="", keep_qaf=False):
    """out: {kkt (condensed), cdd, ric, dir (expanded), con (expanded), steps, con_updated, status} and, of a Newton iteration,
    {sol}: each against its table on what tests/inactive_regions.py defines of it; the step sizes bit for bit the same"""
    import inactive_regions as ir
    bad = []
    for buf in ("kkt", "cdd", "dir"):
        if buf in out:
            bad += masked_mismatches(P, buf, out[buf], ~ir.output_inactive(P, buf, "chain", keep_qaf), elements,
                                     which="kkt_pre" if buf == "kkt" else None, what=what)
    if "ric" in out:   # the fields compare_riccati reads (the STO fields of a grid without STO are nobody's output)
        bad += batch_mismatches(Records(P.L, "ric"), out["ric"], elements, grids=P.grids, what=what + " ric", check_sto=False)
    for key in ("con", "con_updated"):
        if key in out:
            bad += masked_mismatches(P, "con", out[key], con_active_mask(P), elements, what=what + (" after the update" if key != "con" else ""))
    if "sol" in out:
        bad += masked_mismatches(P, "sol", out["sol"], ~ir.output_inactive(P, "sol", "integrate"), elements, what=what)
    for key in ("steps", "status"):
        if key in out:
            bad += per_instance_mismatches(key, out[key], elements, what=what)
    return bad


def unconstr_pipeline_inputs(L, n, elements=ELEMENTS_COST):
    """the fixed-base arm before rtoc_unconstr_condense (tests/test_unconstr_dynamics.py's data) under the cost scale"""
    from test_unconstr_dynamics import _data
    kkt, cdd = _data(L, n, SEEDS)
    return dict(kkt=batch_of(elements, kkt, lambda k, e: scale(L, "kkt_pre", k, e)),
                cdd=batch_of(elements, cdd, lambda k, e: scale(L, "cdd_unconstr", k, e)),
                dx0=batch_of(elements, pr.make_dx0(L, SEEDS), scale_dx0))


def unconstr_pipeline_mismatches(P, out, elements=ELEMENTS_COST, what=""):
    import inactive_regions as ir
    bad = []
    for buf in ("kkt", "ric", "dir"):
        bad += masked_mismatches(P, buf, out[buf], ~ir.output_inactive(P, buf, "unconstr"), elements,
                                 which="kkt_pre" if buf == "kkt" else None, what=what)
    return bad + per_instance_mismatches("status", out["status"], elements, what=what)


WRITEBACK_FIELDS = ("Qxx", "Qxu", "Quu", "lu")


def writeback_mismatches(L, grids, kkt_out, elements=ELEMENTS, what=""):
    """RTOC_OPT_WRITEBACK_KKT: the mutated Qxx, Qxu, Quu, lu carry their input factors"""
    N = len(grids) - 1
    bad = []
    for f in WRITEBACK_FIELDS:
        idx = [i for i, g in enumerate(grids[:N]) if f == "Qxx" or g.type != GRID_IMPACT]
        bad += batch_mismatches(Records(L, "kkt"), kkt_out[:, idx], elements, fields=[f], what=what + " writeback")
    return bad
