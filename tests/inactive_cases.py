"""The small problems of tests/test_inactive_regions.py (CPU) and tests/test_inactive_reads_gpu.py: grids that hold every kind of
inactive region, their clean inputs (zero padding, as robotoc_amd/problems.py generates them), and the oracle's form of every stage
as a function {inputs} -> {outputs} that does not write its arguments.

ANYmal: N = 8 intervals of 0.02 s, a lift 12 -> 6 at 0.05 s and an impact 6 -> 12 at 0.11 s whose switching constraint has
dims = 6 -- 12 grid points: intermediate points with dimf 12 and 6, a point with the switching constraint, the lift, the impact
and the terminal point; once with both events' switching times free (sto / sto_next on every phase) and once without; batch 5 =
one full 4-instance workgroup and one partial.  iCub (nv = 35): the same events on 6 intervals (6 + the lift point + the impact point and the one after it + the terminal point = 10 grid points), batch 2."""
import numpy as np

from inactive_regions import Problem, input_inactive
from robotoc_amd import problems as pr
from robotoc_amd.grid import ContactSequence, Event, discretize, uniform_grid
from robotoc_amd.types import Records, anymal_dims, icub_dims, iiwa14_dims, joint_limit_rows

MC, CD, TAU = 4, 3, 0.995
IIWA_DT = 0.05


def _grids(N, dt, lift, impact, sto):
    cs = ContactSequence([12, 6, 12], [Event("lift", lift, sto=sto), Event("impact", impact, sto=sto, impact_dimf=6)])
    return discretize(N, N * dt, 0.0, cs, phase_based=sto)


def anymal_case(layout_for, sto=False, constraints=False):
    dims = anymal_dims()
    grids = _grids(8, 0.02, 0.05, 0.11, sto)
    rows = joint_limit_rows(dims) if constraints else []
    return dims, Problem(layout_for(dims), grids, rows, MC if constraints else 0, CD), 5


def icub_case(layout_for):
    dims = icub_dims(35)
    return dims, Problem(layout_for(dims), _grids(6, 0.02, 0.03, 0.07, False), [], 0, CD), 2


WRENCH_MC = 2    # iCub: two feet, sole half-extents and friction coefficient of tests/test_contact_wrench_cone.py
WRENCH_SOLES = ((0.08, 0.04, 0.7), (0.072, 0.044, 0.6))


def icub_wrench_case(layout_for):
    """iCub with its joint-limit rows and the 17 wrench-cone rows of each foot: the lift takes one foot off (dimf 12 -> 6)."""
    nv = 35
    dims = icub_dims(nv, nc_max=6 * (nv - 6) + 17 * WRENCH_MC + 2)
    return dims, Problem(layout_for(dims), _grids(6, 0.02, 0.03, 0.07, False), joint_limit_rows(dims), WRENCH_MC, 6, cone_rows=17), 2


def iiwa14_case(layout_for):
    """The fixed-base arm (no contacts, no switching constraint): 4 intervals, batch 3.  Only the terminal point, the fields the
    unconstrained path does not use and the alignment doubles are inactive."""
    dims = iiwa14_dims()
    return dims, Problem(layout_for(dims), uniform_grid(4, IIWA_DT), [], 0, CD), 3


_CACHE = {}


def inputs_of(P, batch, stage, key):
    """Clean inputs of a stage, generated once per (key, stage) and never written."""
    if (key, stage) not in _CACHE:
        L, grids = P.L, P.grids
        if stage == "sweep":
            inp = dict(kkt=pr.make_kkt_batch(L, grids, batch, mode="dynamics"), dx0=pr.make_dx0(L, batch))
        elif stage == "integrate":
            # every member of the direction and of the solution at unit scale (tests/test_integrate_solution.py), the inactive
            # part zero, q on the manifold
            rng = np.random.default_rng(17)
            sol, d = rng.uniform(-1, 1, (batch, P.n, L.sol.stride)), rng.uniform(-1, 1, (batch, P.n, L.dir.stride))
            sol[:, input_inactive(P, "sol", "integrate")] = 0.0
            d[:, input_inactive(P, "dir", "integrate")] = 0.0
            if L.dims.np == 6:
                o = L.sol.off[0]
                sol[..., o + 3:o + 7] /= np.linalg.norm(sol[..., o + 3:o + 7], axis=-1, keepdims=True)
            inp = dict(sol=sol, dir=d, steps=np.stack([rng.uniform(0.2, 1.0, batch), rng.uniform(0.2, 1.0, batch)], axis=1))
        elif stage == "unconstr":
            # tests/test_unconstr_dynamics.py: SPD [Qxx Qxu; . Qaa] and the inverse-dynamics derivatives, with the full torque
            # Hessian's off-diagonal part in the MJtJinv field and its diagonal in Qaa ALONE
            nv = L.dims.nv
            kkt = Records(L, "kkt").zeros(batch, P.n)
            for b in range(batch):
                pr.fill_unconstr_instance(L, P.n, kkt[b], np.random.default_rng(pr.BASE_SEED + b))
            Records(L, "kkt").f(kkt, "Qxu")[...] = 0.0      # (an output of the condensation)
            rng = np.random.default_rng(3)
            C = Records(L, "cdd")
            cdd = C.zeros(batch, P.n)
            C.f(cdd, "dIDCdqv")[:, :-1] = rng.uniform(-1, 1, (batch, P.N, nv, 2 * nv))
            C.f(cdd, "dIDda")[:, :-1] = rng.uniform(-1, 1, (batch, P.N, nv, nv))
            C.f(cdd, "IDC")[:, :-1] = rng.uniform(-1, 1, (batch, P.N, nv))
            C.f(cdd, "Qaa")[:, :-1] = rng.uniform(0.1, 1.0, (batch, P.N, nv))
            C.f(cdd, "la")[:, :-1] = rng.uniform(-1, 1, (batch, P.N, nv))
            Q = rng.uniform(-0.2, 0.2, (batch, P.N, nv, nv))
            Q = 0.5 * (Q + np.swapaxes(Q, -1, -2))
            Q[..., np.arange(nv), np.arange(nv)] = 0.0
            C.f(cdd, "MJtJinv")[:, :-1] = Q
            kkt[:, input_inactive(P, "kkt", "unconstr")] = 0.0
            inp = dict(kkt=kkt, cdd=cdd, dx0=pr.make_dx0(L, batch))
        else:
            kkt, cdd = pr.make_precondense_batch(L, grids, batch)
            inp = dict(kkt=kkt, cdd=cdd, dx0=pr.make_dx0(L, batch))
            if P.rows or P.cone_contacts:
                con = pr.make_constraint_batch(L, grids, batch)
                rng = np.random.default_rng(2)   # a cmpl that does not vanish (tests/test_kkt_error.py)
                Records(L, "con").f(con, "cmpl")[...] = 0.01 * rng.uniform(-1, 1, (batch, len(grids), L.dims.nc_max))
                inp["con"] = con
                if P.cone_rows == 17:
                    from oracle import oracle as orc
                    inp["cone"] = pr.make_wrench_cone_batch(L, grids, batch, P.cone_contacts, [orc.wrench_cone_matrix(*s) for s in WRENCH_SOLES])
                else:
                    inp["cone"] = pr.make_cone_batch(L, grids, batch, MC)
        for v in inp.values():
            v.setflags(write=False)
        _CACHE[(key, stage)] = inp
    return _CACHE[(key, stage)]


# ---------------------------------------------------------------- the oracle's stages ----

def _zeros(P, which, batch):
    return Records(P.L, which).zeros(batch, P.n)


def oracle_sweep(oracle, P, fill=0.0):
    def run(inp):
        b = inp["kkt"].shape[0]
        ric, d = _zeros(P, "ric", b) + fill, _zeros(P, "dir", b) + fill
        st = oracle.riccati_sweep_batch(P.L, P.grids, np.array(inp["kkt"]), ric, d, dx0=np.array(inp["dx0"]))
        return dict(ric=ric, dir=d, status=st)
    return run


def oracle_condense(oracle, P):
    def run(inp):
        kk, cc = np.array(inp["kkt"]), np.array(inp["cdd"])
        st = oracle.condense_batch(P.L, P.grids, kk, cc)
        return dict(kkt=kk, cdd=cc, status=st)
    return run


def oracle_chain(oracle, P, fill=0.0):
    """Constraints::condenseSlackAndDual (box rows, cones) -> contact dynamics -> Riccati -> expansion -> step sizes, as
    rtoc_condense, rtoc_riccati_sweep and rtoc_expand run them (tests/test_friction_cone.py)."""
    def run(inp):
        L, grids = P.L, P.grids
        kk, cc = np.array(inp["kkt"]), np.array(inp["cdd"])
        b = kk.shape[0]
        out = {}
        if "con" in inp:
            nn, cone = np.array(inp["con"]), np.array(inp["cone"])
            oracle.pdipm_condense_batch(L, grids, P.rows, kk, nn)
            if P.cone_rows == 17:
                oracle.wrench_condense_batch(L, grids, P.cone_contacts, cone, cc, nn)
            else:
                oracle.cone_condense_batch(L, grids, P.cone_contacts, P.cone_dim, cone, kk, cc, nn)
        st = oracle.condense_batch(L, grids, kk, cc)
        kkt_condensed = kk.copy()
        ric, d = _zeros(P, "ric", b) + fill, _zeros(P, "dir", b) + fill
        st = st | oracle.riccati_sweep_batch(L, grids, kk, ric, d, dx0=np.array(inp["dx0"]))
        oracle.expand_batch(L, grids, cc, d)
        if "con" in inp:
            steps = oracle.pdipm_expand_batch(L, grids, P.rows, nn, d, TAU)
            if P.cone_rows == 17:
                oracle.wrench_expand_batch(L, grids, P.cone_contacts, cone, nn, d, TAU, steps)
            else:
                oracle.cone_expand_batch(L, grids, P.cone_contacts, P.cone_dim, cone, nn, d, TAU, steps)
            out.update(con=nn, steps=steps)
        out.update(kkt=kkt_condensed, cdd=cc, ric=ric, dir=d, status=st)
        return out
    return run


def oracle_update(oracle, P):
    def run(inp):
        nn = np.array(inp["con"])
        oracle.pdipm_update_batch(P.L, P.grids, P.rows, nn, inp["steps"])
        if P.cone_rows == 17:
            oracle.wrench_update_batch(P.L, P.grids, P.cone_contacts, nn, inp["steps"])
        else:
            oracle.cone_update_batch(P.L, P.grids, P.cone_contacts, P.cone_dim, nn, inp["steps"])
        return dict(con=nn)
    return run


def oracle_kkt_error(oracle, P):
    def run(inp):
        return dict(kkt_error=oracle.kkt_error(P.L, P.grids, np.array(inp["kkt"]), np.array(inp["cdd"]), np.array(inp["con"]), P.rows,
                                               P.cone_contacts, P.cone_dim, P.cone_rows))
    return run


def oracle_integrate(oracle, P):
    def run(inp):
        sol = np.array(inp["sol"])
        oracle.integrate_solution_batch(P.L, P.grids, inp["steps"], np.array(inp["dir"]), sol)
        return dict(sol=sol)
    return run


def oracle_unconstr(oracle, P, fill=0.0):
    def run(inp):
        kk, cc = np.array(inp["kkt"]), np.array(inp["cdd"])
        b = kk.shape[0]
        oracle.unconstr_condense_batch(P.L, P.n, kk, cc)
        condensed = kk.copy()
        ric, d = _zeros(P, "ric", b) + fill, _zeros(P, "dir", b) + fill
        st = oracle.unconstr_sweep_batch(P.L, P.n, IIWA_DT, kk, ric, d, dx0=np.array(inp["dx0"]))
        oracle.unconstr_expand_batch(P.L, P.n, cc, d, IIWA_DT)
        return dict(kkt=condensed, ric=ric, dir=d, status=st)
    return run


def sto_terms(batch, nev=2):
    """lt and the diagonal of Qtt of the two events, per instance"""
    rng = np.random.default_rng(23)
    return rng.uniform(-1, 1, (batch, nev)), rng.uniform(0.1, 1, (batch, nev))


def oracle_sto_kkt(oracle, P):
    def run(inp):
        kk = np.array(inp["kkt"])
        lt, qtt = sto_terms(kk.shape[0])
        return dict(kkt=kk, sto_kkt_term=oracle.sto_eval_kkt(P.L, P.grids, kk, lt, qtt))
    return run


def sto_direction(P, batch):
    """direction records of which only the switching-time direction is filled"""
    rng = np.random.default_rng(29)
    d = _zeros(P, "dir", batch)
    Records(P.L, "dir").f(d, "dts")[..., 0] = 0.05 * rng.uniform(-1, 1, (batch, P.n))
    d[:, input_inactive(P, "dir", "sto_steps")] = 0.0
    return d


def restated_sto_steps(P):
    """SwitchingTimeOptimization::computeStepSizes as oracle/sto.py restates it (the reference of tests/test_sto_device.py), on
    dwell-time rows off their initialisation."""
    from oracle import sto as osto
    D = Records(P.L, "dir")

    def run(inp):
        rng = np.random.default_rng(31)
        steps, rows = [], []
        for b in range(inp["dir"].shape[0]):
            con = np.zeros((6, 3))
            con[0], con[1] = rng.uniform(0.05, 0.4, 3), rng.uniform(0.002, 0.05, 3)
            con[2], con[3] = 0.01 * rng.uniform(-1, 1, 3), con[0] * con[1] - 1.0e-3
            steps.append(osto.step_sizes(con, osto.event_dts(P.grids, D.f(inp["dir"][b], "dts")[:, 0]), TAU))
            rows.append(con)      # (dslack, ddual: a NaN direction drops out of the step sizes themselves)
        return dict(steps=np.array(steps), rows=np.array(rows))
    return run


def unconstr_iterate(P, batch):
    """a rough iterate of the fixed-base arm, the inactive part zero"""
    rng = np.random.default_rng(21)
    sol = rng.uniform(-1, 1, (batch, P.n, P.L.sol.stride))
    S = Records(P.L, "sol")
    S.f(sol, "q")[...] *= 0.4
    S.f(sol, "u")[...] *= 20.0
    sol[:, input_inactive(P, "sol", "linearize")] = 0.0
    return sol


def restated_unconstr_linearize(oracle, P):
    """UnconstrOCPSolver's evalKKT up to the condensation as tests/test_unconstr_arm_sizes.py restates the reference's lines in
    numpy (the reference rtoc_unconstr_eval_kkt is compared with), Jacobians by the complex step."""
    from robotoc_amd import robot_model as rm
    from test_unconstr_arm_sizes import _cost, restated_eval_kkt
    m = rm.load_named("iiwa14")
    cost = _cost(m.nv, np.random.default_rng(5))

    def run(inp):
        b = inp["sol"].shape[0]
        x0 = np.zeros((b, 2 * m.nv))
        with np.errstate(all="ignore"):
            out, err, dx0 = restated_eval_kkt(oracle, m, cost, IIWA_DT, P.L, np.array(inp["sol"]), x0, fd=False)
        res = dict(kkt_error=err, dx0=dx0)
        for (bb, i), items in out.items():
            for rec, field, val, _ in items:
                res["%s.%s at grid point %d, instance %d" % (rec, field, i, bb)] = np.atleast_1d(np.asarray(val, dtype=np.float64))
        return res
    return run


def stage_io(stage, constraints):
    if stage == "linearize":
        return ("sol",), ()
    if stage == "sto_kkt":
        return ("kkt",), ("kkt",)
    if stage == "sto_steps":
        return ("dir",), ()
    """(input buffers with a mask, output buffers with a mask) of a stage."""
    if stage == "sweep":
        return ("kkt",), ("ric", "dir")
    if stage == "condense":
        return ("kkt", "cdd"), ("kkt", "cdd")
    if stage == "chain":
        return (("kkt", "cdd", "con", "cone"), ("kkt", "cdd", "con", "ric", "dir")) if constraints else (("kkt", "cdd"), ("kkt", "cdd", "ric", "dir"))
    if stage == "update":
        return ("con",), ("con",)
    if stage == "kkt_error":
        return ("kkt", "cdd", "con"), ()
    if stage == "integrate":
        return ("dir", "sol"), ("sol",)
    if stage == "unconstr":
        return ("kkt", "cdd"), ("kkt", "ric", "dir")
    raise KeyError(stage)
