"""RTOC_OPT_GRAPH after every context mutator: a replay from a captured hipGraph gives the bits of the plain launch sequence, and
graphing resumes after the mutation (tests/graph_twin.py holds the protocol; tests/graph_mutators.py names, for every function of
the C ABI, the case here that covers it).  Every comparison is np.array_equal: there is no tolerance.

Scenario R (records): ANYmal dims, grids of at most 6 points from tests/grid_words.py with an impact, a lift and a switching
constraint, batch 3, synthetic pre-condensation records; launches rtoc_newton_iteration(0, 0.995) and rtoc_condense +
rtoc_riccati_sweep.  Its switching-time cases need the sto flags only TimeDiscretization produces (grid_words has none): they run
on the smallest phase-based jump grid, 7 points.
Scenario W (wide kernels): iCub nv = 32, 5 grid points, batch 2: the register-wide kernel against the tile kernel.
Scenario C (closed loop): the ANYmal model on 6 grid points, batch 2, rtoc_contact_update_solution -- evalKKT launched plainly, then
the captured Newton iteration.  Most of its setters feed evalKKT alone: their cases show that, with an effect guard.  The wrench
cone table needs surface contacts: that one case runs on iCub's soles (tests/per_instance_placement_cases.py, 8 grid points).
Paths that are not graphed (the unconstrained solver, ParNMPC, the line-search iteration): one plain-vs-graph run each, equal, and the
replay counter does not move.

One module-scoped twin per scenario, put back to its base configuration before every case; a case that cannot be undone (a bound
buffer, a lazily created one, the profile buffer, a clone) builds a twin of its own."""
import struct

import numpy as np
import pytest

import grid_words as gw
from graph_twin import Effect, Twin, differing
from robotoc_amd import problems as pr
from robotoc_amd.grid import ContactSequence, Event, contact_masks, discretize, jump_sto_sequence
from robotoc_amd.types import (BUF_CDD, BUF_CON, BUF_CONE, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_SOL, BUF_STEP, OPT_BACKWARD_REGISTER,
                               OPT_BACKWARD_SCAN, OPT_BACKWARD_WAVES, OPT_CONDENSE_KEEP_QAF, OPT_CONDENSE_REGISTER, OPT_CONDENSE_SPLIT,
                               OPT_CONE_JACOBIAN, OPT_CONTACT_INV_DAMPING, OPT_FXX_STRUCTURE, OPT_GRAPH, OPT_IMPACT_CONES,
                               OPT_LINEARIZE_DOFS_PER_PASS, OPT_LINEARIZE_FUSED, OPT_MAX_DTS0, OPT_SWEEP_CHUNKS, OPT_SWITCHING_TRANSPORT,
                               OPT_UNCONSTR_DENSE, OPT_WRITEBACK_KKT, Records, anymal_dims, iiwa14_dims, joint_limit_rows)

pytestmark = pytest.mark.gpu

TAU = 0.995
WRITTEN = ("dir", "ric", "step", "kkt_error")   # what a launch writes and no upload or setter does: tests/graph_twin.py, `guard`
MC, CD = 4, 3   # friction cones: four point contacts


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _set_option(option, value):
    from robotoc_amd import capi
    return lambda c: capi._chk(capi.lib().rtoc_set_option(c._h, int(option), int(value)))


def _download(ctx, buf, which):
    from robotoc_amd import capi
    try:
        return ctx.download_records(buf, which)
    except capi.RtocError:
        return None   # the buffer does not exist (yet): on both contexts or on neither


def _converged(ctx):
    from robotoc_amd import capi
    try:
        return np.array(ctx.converged_count())
    except capi.RtocError:
        return None   # no Newton iteration ran on this context


# ---- a twin on synthetic records (scenarios R and W, the switching-time cases) ---------------------------------------------------
class RecordTwin(Twin):
    """grids: {name: grid}.  st: what restore and outputs depend on and the cases change -- the grid in force, whether the
    constraint / cone / solution records are uploaded, a stray Fxx entry, the switching-time problem."""

    def __init__(self, dims, grids, base, batch, rows=(), condensed=False, sol=True):
        from robotoc_amd import capi
        self.dims, self.grids, self.base, self.batch, self.rows, self.condensed = dims, grids, base, batch, list(rows), condensed
        self.max_stages = max(len(g) for g in grids.values())
        self._inputs, self.keep = {}, []
        self.base_sol = sol
        ctxs = [capi.Context(dims, self.max_stages, batch, 0) for _ in range(2)]
        self.L = ctxs[0].L
        super().__init__(ctxs[0], ctxs[1], self.restore, self.outputs, lambda c: c.graph_replay_count())
        self.defaults = {o: self.plain.get_option(o) for o in (OPT_CONDENSE_SPLIT, OPT_CONDENSE_REGISTER, OPT_BACKWARD_REGISTER)}
        self.reset()

    def inputs(self, key):
        if key not in self._inputs:
            L, grids, B = self.L, self.grids[key], self.batch
            n = len(grids)
            inp = dict(dx0=pr.make_dx0(L, B), step=np.ones((B, 2)))
            if self.condensed:
                inp["kkt"] = pr.make_kkt_batch(L, grids, B, mode="dynamics")
            else:
                inp["kkt"], inp["cdd"] = pr.make_precondense_batch(L, grids, B)
                inp["con"] = pr.make_constraint_batch(L, grids, B)
                inp["cone"] = pr.make_cone_batch(L, grids, B, MC)
                sol = np.random.default_rng(5).uniform(-1, 1, (B, n, L.sol.stride))
                o = L.sol.off[0]
                sol[..., o + 3:o + 7] /= np.linalg.norm(sol[..., o + 3:o + 7], axis=-1, keepdims=True)   # q on the manifold
                inp["sol"] = sol
            # one entry off the [a I | c I] pattern of the top half of Fxx, in one record of one instance: below the two dense 6 x 6
            # floating-base corners (rows 0..5), off the diagonal of the velocity block
            stray = inp["kkt"].copy()
            Records(L, "kkt").f(stray[B - 1, 1], "Fxx")[8, L.dims.nv + 3] = 0.3
            inp["kkt_stray"] = stray
            inp["poison_ric"] = np.full((B, n, L.ric.stride), np.nan)
            inp["poison_dir"] = np.full((B, n, L.dir.stride), np.nan)
            for a in inp.values():
                a.setflags(write=False)
            self._inputs[key] = inp
        return self._inputs[key]

    def reset(self):
        """the base configuration, through the public setters (every one of them a new epoch)"""
        self.st = dict(grid=self.base, con=bool(self.rows), cones=False, sol=self.base_sol and not self.condensed, stray=False, sto=False)
        for c in (self.plain, self.graph):
            c.set_stream(0)   # the context's own
            c.set_grid(self.grids[self.base])
            c.set_constraint_rows(self.rows)
            c.set_friction_cones(0, CD)
            for o, v in ((OPT_WRITEBACK_KKT, 0), (OPT_MAX_DTS0, _bits(0.1)), (OPT_BACKWARD_WAVES, 0), (OPT_CONTACT_INV_DAMPING, _bits(0.0)),
                         (OPT_SWEEP_CHUNKS, 1), (OPT_BACKWARD_SCAN, 0), (OPT_CONDENSE_KEEP_QAF, 0), (OPT_FXX_STRUCTURE, 0),
                         (OPT_IMPACT_CONES, 1)) + tuple(self.defaults.items()):
                _set_option(o, v)(c)
            c.sto_set_problem(0.0, 1.0, np.zeros(0), np.zeros(1))   # num_events == 0: off
            c.set_graph(c is self.graph)
        return self

    def restore(self, ctx):
        st, inp = self.st, self.inputs(self.st["grid"])
        ctx.upload(BUF_KKT, inp["kkt_stray" if st["stray"] else "kkt"])
        ctx.upload(BUF_DX0, inp["dx0"])
        ctx.upload(BUF_STEP, inp["step"])
        if not self.condensed:
            ctx.upload(BUF_CDD, inp["cdd"])
            if st["con"]:
                ctx.upload(BUF_CON, inp["con"])
            if st["cones"]:
                ctx.upload(BUF_CONE, inp["cone"])
            if st["sol"]:
                ctx.upload(BUF_SOL, inp["sol"])
        ctx.upload(BUF_RIC, inp["poison_ric"])
        ctx.upload(BUF_DIR, inp["poison_dir"])
        if st["sto"]:
            ctx.sto_set_slack_dual(*st["sto"])
        ctx.clear_status()

    def outputs(self, ctx):
        out = {w: _download(ctx, b, w) for b, w in ((BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_KKT, "kkt"), (BUF_CDD, "cdd"),
                                                   (BUF_CON, "con"), (BUF_SOL, "sol"))}
        out["step"] = ctx.download(BUF_STEP, (self.batch, 2))
        out["status"] = ctx.status()
        out["kkt_error"] = ctx.kkt_error()
        out["converged"] = _converged(ctx)
        if self.st["sto"]:
            out["event_times"], out["time_steps"], out["sto_rows"] = ctx.sto_event_times(), ctx.sto_time_steps(), ctx.sto_constraint_data()
            out["sto_lt"], out["sto_qtt"], out["sto_err"] = ctx.sto_kkt_terms()
        return out

    def close(self):
        self.plain.close()
        self.graph.close()
        self.keep.clear()


def _newton(c):
    c.newton_iteration(0.0, TAU)


def _sweep(c):
    c.condense()
    c.riccati_sweep()


def _sweep_alone(c):
    c.riccati_sweep()


LAUNCHES = {"newton": _newton, "sweep": _sweep}
R_WORDS = {"base": ("C", "R", "I", "L", "R"), "other": ("R", "L", "C", "I", "R"), "short": ("C", "L", "I", "R")}


def _r_grids():
    rows = gw.SHAPES["anymal"][1]
    return {k: gw.build(w, rows) for k, w in R_WORDS.items()}


def _r_twin(rows=None, sol=True):
    dims = anymal_dims()
    return RecordTwin(dims, _r_grids(), "base", 3, rows=joint_limit_rows(dims)[:48] if rows is None else rows, sol=sol)


@pytest.fixture(scope="module")
def twin_r_module():
    t = _r_twin()
    yield t
    t.close()


@pytest.fixture
def R(twin_r_module):
    return twin_r_module.reset()


@pytest.fixture
def fresh_r():
    made = []

    def make(**kw):
        made.append(_r_twin(**kw))
        return made[-1]
    yield make
    for t in made:
        t.close()


def test_r_the_words_hold_an_impact_a_lift_and_a_switching_constraint():
    for w in R_WORDS.values():
        assert gw.valid(w) and len(w) + 1 <= 6 and "I" in w and "L" in w and ("C" in w or "Lc" in w), w


# ---- scenario R: every option -----------------------------------------------------------------------------------------------------
def _reads_back(option, value):
    """replacement evidence of an option step that changes the launch structure and no bit of the result"""
    return Effect("launch structure only: rtoc_get_option reads the new value on both contexts",
                  lambda tw, before, after: all(c.get_option(option) == value for c in (tw.plain, tw.graph)) and not differing(before, after))


# option -> the values it steps through, from its default and back to it; True: the step changes no bit of the result (the same
# arithmetic from another launch structure, or a value that selects the same kernel at this batch size), and rtoc_get_option is the
# evidence in place of the effect guard
R_OPTION_STEPS = {
    "writeback_kkt": (OPT_WRITEBACK_KKT, [(1, False), (0, False)]),
    "backward_waves": (OPT_BACKWARD_WAVES, [(1, False), (3, True), (0, False)]),   # the two tile-split variants: the same bits
    "contact_inv_damping": (OPT_CONTACT_INV_DAMPING, [(_bits(1.0e-3), False), (_bits(0.0), False)]),
    "sweep_chunks": (OPT_SWEEP_CHUNKS, [(2, True), (16, True), (1, True)]),
    "condense_split": (OPT_CONDENSE_SPLIT, [(1, False), (0, False)]),
    "backward_scan": (OPT_BACKWARD_SCAN, [(1, False), (2, True), (0, False)]),
    "condense_keep_qaf": (OPT_CONDENSE_KEEP_QAF, [(1, False), (0, False)]),
    "fxx_structure": (OPT_FXX_STRUCTURE, [(1, False), (2, False), (0, True)]),
    "impact_cones": (OPT_IMPACT_CONES, [(0, False), (1, False)]),
    "backward_register": (OPT_BACKWARD_REGISTER, [(0, False), (2, False), (1, True)]),
    "condense_register": (OPT_CONDENSE_REGISTER, [(0, False), (2, False), (1, True)]),
}
DOUBLE_OPTIONS = (OPT_MAX_DTS0, OPT_CONTACT_INV_DAMPING)


def _with_cones(tw):
    def on(c):
        c.set_friction_cones(MC, CD)
        tw.st["cones"] = tw.st["con"] = True
    tw.both(on)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("name", sorted(R_OPTION_STEPS))
def test_r_option(R, name, launch):
    option, steps = R_OPTION_STEPS[name]
    if name == "condense_split":   # its default is the shape's, or the environment's (RTOC_CONDENSE_SPLIT)
        d = R.defaults[OPT_CONDENSE_SPLIT]
        steps = [(1 - d, False), (d, False)]
    if name in ("impact_cones", "condense_register", "condense_split"):
        _with_cones(R)
    if name == "condense_register":   # the register-chained kernel serves the one-kernel pipeline only
        R.both(_set_option(OPT_CONDENSE_SPLIT, 0))
    R.both(_set_option(option, steps[-1][0]))   # the steps start from, and end at, the documented default
    for value, neutral in steps:
        effect = _reads_back(option, value) if neutral and option not in DOUBLE_OPTIONS else None
        R.case(_set_option(option, value), LAUNCHES[launch], effect=effect, name="%s = %d (%s)" % (name, value, launch), recapture=True)
    assert (R.plain.status() == 0).all()


def test_r_graph_option_off_on_off_on(R):
    """RTOC_OPT_GRAPH itself: off, the counter stands still and the results stay those of the plain context; on, graphing resumes"""
    def graph(v):
        return lambda c: c.set_graph(v) if c is R.graph else None
    reads = lambda v: Effect("rtoc_get_option(RTOC_OPT_GRAPH) reads %d; the results do not change" % v,
                             lambda tw, before, after: tw.graph.get_option(OPT_GRAPH) == v and not differing(before, after))
    R.case(graph(False), _newton, effect=reads(0), name="graph off", replay_after=False)
    R.case(graph(True), _newton, effect=reads(1), name="graph on", replay_before=False, recapture=True)
    R.case(graph(False), _sweep, effect=reads(0), name="graph off (sweep)", replay_after=False)
    R.case(graph(True), _sweep, effect=reads(1), name="graph on (sweep)", replay_before=False, recapture=True)


# ---- scenario R: grid, rows, cones ------------------------------------------------------------------------------------------------
def _grid(tw, key):
    def fn(c):
        c.set_grid(tw.grids[key])
        tw.st["grid"] = key
    return fn


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_r_set_grid(R, launch):
    """the same length with another structure; a shorter horizon and the long one again; the identical grid again"""
    run = LAUNCHES[launch]
    R.case(_grid(R, "other"), run, name="another structure", recapture=True)
    R.case(_grid(R, "short"), run, name="a shorter horizon", recapture=True)
    R.case(_grid(R, "base"), run, name="the long horizon again", recapture=True)
    same = Effect("the grid in force set again: the results do not change, the sequence is captured anew and replayed",
                  lambda tw, before, after: not differing(before, after))
    R.case(_grid(R, "base"), run, effect=same, name="the identical grid", recapture=True)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_r_set_constraint_rows(R, launch):
    rows, run = joint_limit_rows(R.dims), LAUNCHES[launch]
    R.case(lambda c: c.set_constraint_rows(rows), run, name="more rows", recapture=True)
    R.case(lambda c: c.set_constraint_rows(rows[:12]), run, name="fewer rows", recapture=True)
    R.case(lambda c: c.set_constraint_rows(rows[24:36]), run, name="a different row set", recapture=True)


def test_r_set_constraint_rows_from_none(fresh_r):
    """no rows at all, then rows: RTOC_BUF_CON is created by the setter, after the capture"""
    tw = fresh_r(rows=[])
    rows = joint_limit_rows(tw.dims)

    def some(c):
        c.set_constraint_rows(rows[:24])
        tw.st["con"] = True

    def none(c):
        c.set_constraint_rows([])
        tw.st["con"] = False
    tw.case(some, _newton, name="rows where there were none", recapture=True)
    tw.case(none, _newton, name="no rows again", recapture=True)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_r_set_friction_cones(R, launch):
    """from none to cones (the cone kernels join the sequence, RTOC_BUF_CONE is created) and back to none (they leave it)"""
    run = LAUNCHES[launch]

    def on(c):
        c.set_friction_cones(MC, CD)
        R.st["cones"] = True

    def off(c):
        c.set_friction_cones(0, CD)
        R.st["cones"] = False
    R.case(on, run, name="cones on", recapture=True)
    R.case(off, run, name="cones off", recapture=True)
    R.case(on, run, name="cones on again", recapture=True)


def test_r_set_wrench_cones_refused_leaves_the_sequence(R):
    """ANYmal's point contacts take no wrench cones (6 * 4 > nf_max): the refused call changes nothing of the replayed sequence"""
    from robotoc_amd import capi

    def refused(c):
        with pytest.raises(capi.RtocError):
            c.set_wrench_cones(MC)
    R.case(refused, _newton, effect=Effect("a refused call: the results do not change", lambda tw, b, a: not differing(b, a)), name="wrench cones refused", recapture=False)


# ---- scenario R: buffers created, bound and streamed after the capture --------------------------------------------------------------
def test_r_first_upload_of_the_solution(fresh_r):
    """RTOC_BUF_SOL does not exist while the sequence is captured; its first upload creates it and rtoc_integrate_solution joins"""
    tw = fresh_r(sol=False)
    assert _download(tw.plain, BUF_SOL, "sol") is None

    def upload(c):
        tw.st["sol"] = True
        c.upload(BUF_SOL, tw.inputs("base")["sol"])
    integrated = Effect("the solution records exist and moved from what was uploaded",
                        lambda tw_, before, after: before["sol"] is None and after["sol"] is not None and
                        not np.array_equal(after["sol"], tw.inputs("base")["sol"]))
    tw.case(upload, _newton, effect=integrated, name="first upload of RTOC_BUF_SOL", recapture=True)


def test_r_device_ptr_creates_and_exposes(fresh_r):
    """rtoc_device_ptr on a buffer that does not exist creates it (RTOC_BUF_SOL: the integration joins the sequence); on
    RTOC_BUF_KKT it marks the records as rewritable by the caller, which changes the backward plan's verification"""
    tw = fresh_r(sol=False)

    def expose(c):
        assert c.device_ptr(BUF_SOL) and c.device_ptr(BUF_KKT)
        tw.st["sol"] = True
    tw.case(expose, _newton, effect=Effect("the solution records exist", lambda tw_, b, a: b["sol"] is None and a["sol"] is not None),
            name="rtoc_device_ptr", recapture=True)


def _torch_buffer(ctx, buf):
    import torch
    return torch.full((ctx.buffer_count(buf),), float("nan"), dtype=torch.float64, device="cuda")


def test_r_bind_and_rebind(fresh_r):
    """KKT, DIR, RIC and SOL bound to torch tensors after the capture, then to other tensors: the results land in the storage bound
    last, and the storage bound before, filled with NaN after the re-bind, is never written again"""
    import torch
    tw = fresh_r()
    bufs = ((BUF_KKT, "kkt"), (BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_SOL, "sol"))
    bound = {}   # (context, buffer) -> the tensors bound so far
    tw.keep.append(bound)   # they outlive the contexts

    def bind(c):
        for b, _ in bufs:
            t = _torch_buffer(c, b)
            bound.setdefault((id(c), b), []).append(t)
            c.bind(b, t.data_ptr())
        torch.cuda.synchronize()
        for ts in bound.values():   # what was bound before: poison
            for t in ts[:-1]:
                t.fill_(float("nan"))
        torch.cuda.synchronize()

    def lands(tw_, before, after):
        torch.cuda.synchronize()
        for c in (tw.plain, tw.graph):
            out = tw.outputs(c)
            for b, w in bufs:
                ts = bound[(id(c), b)]
                if not np.array_equal(ts[-1].cpu().numpy()[:out[w].size], out[w].reshape(-1), equal_nan=True):
                    return False
                if not all(bool(torch.isnan(t).all()) for t in ts[:-1]):
                    return False
        return True
    for k in range(2):
        for name, run in sorted(LAUNCHES.items()):
            tw.case(bind, run, effect=Effect("the results are in the tensors bound last; those bound before are still all NaN", lands),
                    name="bind %d (%s)" % (k, name), recapture=True)


def test_r_set_stream(R):
    """a torch stream and back to the context's own"""
    import torch
    s = torch.cuda.Stream()
    same = Effect("the results do not change; the sequence is captured anew on the stream given and replayed",
                  lambda tw, before, after: not differing(before, after))
    for name, run in sorted(LAUNCHES.items()):
        R.case(lambda c: c.set_stream(s.cuda_stream), run, effect=same, name="a torch stream (%s)" % name, recapture=True)
        R.case(lambda c: c.set_stream(0), run, effect=same, name="the context's own stream (%s)" % name, recapture=True)
    torch.cuda.synchronize()


def test_r_fxx_verdict_flips(R):
    """RTOC_OPT_FXX_STRUCTURE = 0: after a capture on structured records one stray Fxx entry arrives with an upload (the dense
    kernel must run: the structured one would ignore the entry), then clean records again"""
    def stray(v):
        def fn(c):
            R.st["stray"] = v
        return fn
    for name, run in sorted(LAUNCHES.items()):
        R.case(stray(True), run, name="a stray Fxx entry (%s)" % name, recapture=True, guard=WRITTEN)
        assert (R.plain.status() == 0).all()
        R.case(stray(False), run, name="structured records again (%s)" % name, recapture=True, guard=WRITTEN)


def test_r_new_tau_and_kkt_tol(R):
    """the two scalar arguments of rtoc_newton_iteration are part of the graph's key"""
    args = dict(tol=0.0, tau=TAU)

    def run(c):
        c.newton_iteration(args["tol"], args["tau"])

    def setter(**kw):
        return lambda c: args.update(kw)
    R.case(setter(tau=0.9), run, name="a new tau")
    R.case(setter(tol=1.0e30), run, name="a new kkt_tol")
    assert R.plain.converged_count() == R.batch
    R.case(setter(tol=0.0, tau=TAU), run, name="both back")
    assert R.plain.converged_count() == 0


def test_r_debug_profile_attach(fresh_r):
    """rtoc_debug_profile attaches the stamp buffer, whose pointer the condensation, expansion and backward launches carry: the
    sequence must be captured anew -- the replay counter moves by exactly 2 in the three runs after the attach (a graph that was
    kept gives 3: what this case catches in the default build, where no kernel writes a stamp) -- and the graph context's stamps
    are non-zero exactly where the plain context's are (a build with the phase stamps compiled in, make PROF=1: 94 of them)"""
    from robotoc_amd import capi
    tw = fresh_r()

    def stamps(tw_, before, after):
        p, g = capi.debug_profile(tw.plain), capi.debug_profile(tw.graph)
        print("phase stamps: %d non-zero on the plain context, %d on the graph context" % ((p != 0).sum(), (g != 0).sum()))
        return bool((p != 0).any()) == bool((g != 0).any()) and np.array_equal(p != 0, g != 0)
    tw.case(capi.debug_profile, _newton, effect=Effect("stamps on the graph context where the plain context has them", stamps), name="profile attach", recapture=True)


def test_r_clone(fresh_r):
    """a warmed graph context cloned: the clone and the original each continue bit-equal to their plain twins; the clone
    destroyed, the original still replays"""
    tw = fresh_r()
    for k in range(3):
        tw.run(_newton, "warming %d" % k)
    assert tw.replay_count() >= 2
    clones = Twin(tw.plain.clone(), tw.graph.clone(), tw.restore, tw.outputs, lambda c: c.graph_replay_count())
    try:
        assert clones.graph.get_option(OPT_GRAPH) == 1 and clones.plain.get_option(OPT_GRAPH) == 0
        assert clones.replay_count() == 0   # a clone starts without the original's graphs
        first = clones.run(_newton, "the clones, first run")
        assert not differing(first, tw.last)   # the same records, the same configuration: the same results as the originals
        same = Effect("the clone computes what the original computes", lambda t, b, a: not differing(b, a))
        clones.case(lambda c: None, _newton, effect=same, name="the clones", recapture=False)
        tw.case(lambda c: None, _newton, effect=same, name="the originals beside their clones", recapture=False)
        # the clone is a context of its own: a mutation of it leaves the original's graph alone
        clones.case(_set_option(OPT_CONTACT_INV_DAMPING, _bits(1.0e-3)), _newton, name="the clones, damped", recapture=True)
        n0 = tw.replay_count()
        tw.run(_newton, "the originals after the clones changed")
        assert tw.replay_count() == n0 + 1 and not differing(tw.last, first)
    finally:
        clones.plain.close()
        clones.graph.close()
    n0 = tw.replay_count()
    tw.run(_newton, "the originals after the clones are gone")
    assert tw.replay_count() == n0 + 1 and not differing(tw.last, first)


def test_r_stage_dump_round_trip(fresh_r, tmp_path):
    """rtoc_load_stage_dump builds a context through rtoc_create and the public setters: a twin loaded from a dump graphs like one
    built by hand"""
    from robotoc_amd import capi
    tw = fresh_r()
    tw.both(tw.restore)
    path = str(tmp_path / "twin.dump")
    tw.plain.save_stage_dump(path, [BUF_KKT, BUF_CDD, BUF_CON, BUF_DX0, BUF_SOL])
    a, b = capi.Context.from_stage_dump(path), capi.Context.from_stage_dump(path)
    b.set_graph(True)
    loaded = Twin(a, b, tw.restore, tw.outputs, lambda c: c.graph_replay_count())
    try:
        loaded.case(_set_option(OPT_CONTACT_INV_DAMPING, _bits(1.0e-3)), _newton, name="a loaded twin", recapture=True)
    finally:
        a.close()
        b.close()


# ---- the switching-time problem (scenario R's launches on the smallest grid with sto flags) -----------------------------------------
STO_T0, STO_T = 0.0, 0.4


def _sto_grids():
    cs = jump_sto_sequence(ground_time=0.13, flying_time=0.1)
    return {"jump": discretize(3, STO_T, STO_T0, cs, phase_based=True), "flat": discretize(3, STO_T, STO_T0, ContactSequence([12]))}


@pytest.fixture(scope="module")
def twin_s_module():
    t = RecordTwin(anymal_dims(), _sto_grids(), "jump", 3, rows=joint_limit_rows(anymal_dims())[:48])
    yield t
    t.close()


@pytest.fixture
def S(twin_s_module):
    return twin_s_module.reset()


def _converged_newton(c):
    """every instance counts as converged: the step sizes are zero and nothing moves, so `restore` restores everything -- the
    switching-time state too, which only rtoc_sto_set_problem (a new epoch) could put back"""
    c.newton_iteration(1.0e30, TAU)


def _sto_problem(tw, ts, barrier=1.0e-3):
    rng = np.random.default_rng(9)
    slack, dual = rng.uniform(0.05, 0.4, (tw.batch, 3)), rng.uniform(0.002, 0.05, (tw.batch, 3))

    def fn(c):
        c.sto_set_problem(STO_T0, STO_T, ts, np.array([0.02, 0.03, 0.02]), barrier, TAU)
        tw.st["sto"] = (slack, dual)
    return fn


STO_TS = np.array([[0.13, 0.23], [0.12, 0.24], [0.14, 0.22]])


def test_s_the_grid_has_sto_flags():
    g = _sto_grids()
    assert len(g["jump"]) == 7 and any(x.sto for x in g["jump"]) and sum(x.type in (1, 2) for x in g["jump"]) == 2
    assert sum(x.type in (1, 2) for x in g["flat"]) == 0


def test_s_sto_set_problem(S):
    """on; other event times; off with num_events == 0; on again, then a grid without events, where sto_on drops inside
    rtoc_set_grid"""
    S.case(_sto_problem(S, STO_TS), _converged_newton, name="problem on", recapture=True, guard=WRITTEN)
    assert (S.plain.status() == 0).all()
    assert np.array_equal(S.last["event_times"], STO_TS) and (S.last["step"] == 0).all()   # nothing moved: what restore relies on
    S.case(_sto_problem(S, STO_TS[::-1] + 0.005), _converged_newton, name="other event times", recapture=True, guard=WRITTEN)
    S.case(_sto_problem(S, STO_TS, barrier=1.0e-2), _converged_newton, name="another barrier", recapture=True, guard=WRITTEN)

    def off(c):
        c.sto_set_problem(STO_T0, STO_T, np.zeros(0), np.zeros(1))
        S.st["sto"] = False
    S.case(off, _converged_newton, name="problem off", recapture=True, guard=WRITTEN)
    S.case(_sto_problem(S, STO_TS), _converged_newton, name="problem on again", recapture=True, guard=WRITTEN)

    def flat(c):
        c.set_grid(S.grids["flat"])
        S.st["grid"], S.st["sto"] = "flat", False
    S.case(flat, _converged_newton, name="a grid without events", recapture=True, guard=WRITTEN)


def test_s_sto_iterates(S):
    """kkt_tol = 0: the event times, the time steps and the dwell-time rows move with every iteration, on both contexts alike
    (they are not restored: the state drifts, and the drift is the evidence that the switching-time kernels ran)"""
    S.both(_sto_problem(S, STO_TS))
    moved = Effect("the event times moved", lambda tw, before, after: not np.array_equal(after["event_times"], STO_TS) and
                   not np.array_equal(after["event_times"], before["event_times"]))
    S.case(_sto_problem(S, STO_TS[::-1] + 0.005), _newton, effect=moved, name="other event times, iterating", recapture=True)
    S.case(lambda c: c.sto_correct_time_steps(), _newton, effect=moved, name="time steps corrected", recapture=False)
    S.case(lambda c: c.sto_init_constraints(), _newton, effect=moved, name="rows initialised", recapture=False)


def test_s_sto_scalars_and_cost_terms(S):
    S.both(_sto_problem(S, STO_TS))
    S.case(lambda c: c.sto_set_regularization(0.3), _converged_newton, name="regularisation set", recapture=True)
    S.case(lambda c: c.sto_set_regularization(0.0), _converged_newton, name="regularisation cleared", recapture=True)
    rng = np.random.default_rng(2)
    lt, qtt = rng.uniform(-1, 1, (S.batch, 2)), rng.uniform(0.1, 1, (S.batch, 2))
    S.case(lambda c: c.sto_set_cost_terms(lt, qtt), _converged_newton, name="cost terms set", recapture=True)
    S.case(lambda c: c.sto_set_cost_terms(-lt, 2 * qtt), _converged_newton, name="other cost terms, same buffer", recapture=False)
    S.case(lambda c: c.sto_set_cost_terms(None, None), _converged_newton, name="cost terms cleared", recapture=True)


def test_s_sto_set_slack_dual(S):
    S.both(_sto_problem(S, STO_TS))
    slack, dual = S.st["sto"]

    def warm(c):
        S.st["sto"] = (2 * slack, 0.5 * dual)
    S.case(warm, _converged_newton, name="other slacks and duals", recapture=False)


def test_s_max_dts0(S):
    """RTOC_OPT_MAX_DTS0 acts on grids with switching-time optimisation only"""
    for launch in (_newton, _sweep):
        S.case(_set_option(OPT_MAX_DTS0, _bits(0.01)), launch, name="max_dts0 = 0.01", recapture=True)
        S.case(_set_option(OPT_MAX_DTS0, _bits(0.1)), launch, name="max_dts0 = 0.1", recapture=True)


def test_s_sto_eval_kkt_from_the_host(S):
    """rtoc_sto_eval_kkt (the host-side form) grows a staging buffer of its own and scatters into the records: a launch, the
    captured sequence is untouched"""
    lt, qtt = np.full((S.batch, 2), 0.3), np.full((S.batch, 2), 0.7)
    same = Effect("the records are restored before every run: the results do not change", lambda tw, b, a: not differing(b, a))
    S.case(lambda c: c.sto_eval_kkt(lt, qtt), _newton, effect=same, name="host-side evalKKT", recapture=False)


# ---- scenario W: the register-wide kernel against the tile kernel ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_w_module():
    dims, rows, _ = gw.SHAPES["icub32"]
    t = RecordTwin(dims, {"base": gw.build(("C", "R", "I", "R"), rows)}, "base", 2, condensed=True)
    yield t
    t.close()


def test_w_backward_register(twin_w_module):
    W = twin_w_module.reset()
    W.both(_set_option(OPT_BACKWARD_REGISTER, 2))
    W.case(_set_option(OPT_BACKWARD_REGISTER, 0), _sweep_alone, name="register-wide -> tile", recapture=True)
    W.case(_set_option(OPT_BACKWARD_REGISTER, 2), _sweep_alone, name="tile -> register-wide", recapture=True)
    assert (W.plain.status() == 0).all()


# ---- scenario C: the closed loop ----------------------------------------------------------------------------------------------------
class ClosedLoopTwin(Twin):
    """ANYmal, 6 grid points (a lift, the touch-down of the two swing feet, the switching constraint two points ahead of it), two
    robots at different places on their own footholds; joint limits with bounds and friction cones with coefficients on the device."""
    BATCH = 2

    def __init__(self):
        import per_instance_placement_cases as pic
        from robotoc_amd import capi, robot_model as rm
        self.m, self.dims = rm.load_named("anymal"), anymal_dims()
        m, B = self.m, self.BATCH
        cs = ContactSequence([12, 6, 12], [Event("lift", 0.011), Event("impact", 0.029, impact_dimf=6)])
        self.grids, self.t, infos = discretize(2, 0.04, 0.0, cs, times=True, infos=True)
        self.t, self.phase = np.array(self.t), np.array([i[1] for i in infos], dtype=np.int32)
        self.n = n = len(self.grids)
        assert n == 6 and any(g.switching_constraint for g in self.grids)
        self.masks = contact_masks(self.grids, [0b1111, 0b1001, 0b1111], [0b0110])
        rng = np.random.default_rng(41)
        self.x0 = np.zeros((B, m.nq + m.nv))
        for b, (x, y, yaw) in enumerate([(0.0, 0.0, 0.0), (0.7, -0.4, 0.3)]):
            self.x0[b, :m.nq], self.x0[b, m.nq:] = pic._yaw(pic.Q_ANYMAL, x, y, yaw), 0.1 * rng.uniform(-1, 1, m.nv)
        S = Records(capi.layout_for(self.dims), "sol")
        self.sol = 0.3 * rng.uniform(-1, 1, (B, n, S.stride))
        for b in range(B):
            for i in range(n):
                q = self.x0[b, :m.nq].copy()
                q[:3] += 0.02 * rng.uniform(-1, 1, 3)
                q[3:7] += 0.02 * rng.uniform(-1, 1, 4)
                q[3:7] /= np.linalg.norm(q[3:7])
                q[7:] += 0.1 * rng.uniform(-1, 1, m.nq - 7)
                S.f(self.sol[b, i], "q")[:m.nq] = q
        wq = np.concatenate([np.full(6, 10.0), np.full(12, 1.0)])
        nv = m.nv
        self.cost = dict(q_ref=pic.Q_ANYMAL, v_ref=np.zeros(nv), u_ref=np.zeros(12), q_weight=wq, v_weight=np.full(nv, 1.0),
                         a_weight=np.full(nv, 1e-3), u_weight=np.full(12, 1e-3), q_weight_terminal=10.0 * wq, v_weight_terminal=np.full(nv, 1.0),
                         q_weight_impact=wq, v_weight_impact=np.full(nv, 1.0), dv_weight_impact=np.full(nv, 1e-3))
        self.rows = joint_limit_rows(self.dims)
        self.bounds = np.concatenate([np.full(24, 2.5), np.full(24, 15.0), np.full(24, 80.0)])
        self.mu = np.full(4, 0.7)
        ctxs = [capi.Context(self.dims, n, B, 0) for _ in range(2)]
        # where the feet stand: the device's own kinematics at x0; the swing feet touch down a step ahead
        ctxs[0].set_grid(self.grids)
        ctxs[0].set_robot_model(m)
        ctxs[0].set_initial_state(self.x0)
        _, feet, _ = ctxs[0].contact_frame_placements("x0")
        self.pos = np.repeat(feet[:, None], n, axis=1)
        i_imp = [i for i, g in enumerate(self.grids) if g.type == 1][0]
        self.pos[:, i_imp:, 1:3, 0] += np.array([0.03, 0.05])[:, None, None]
        super().__init__(ctxs[0], ctxs[1], self.restore, self.outputs, lambda c: c.graph_replay_count())
        self.poison = (np.full((B, n, self.plain.L.ric.stride), np.nan), np.full((B, n, self.plain.L.dir.stride), np.nan))
        self.reset()

    def reset(self):
        self.err = {}
        for c in (self.plain, self.graph):
            c.set_grid(self.grids)
            for o, v in ((OPT_SWITCHING_TRANSPORT, 0), (OPT_CONE_JACOBIAN, 0), (OPT_LINEARIZE_FUSED, 0), (OPT_LINEARIZE_DOFS_PER_PASS, 0),
                         (OPT_CONTACT_INV_DAMPING, _bits(0.0))):
                _set_option(o, v)(c)
            c.set_robot_model(self.m)
            c.set_contact_schedule(self.masks)
            c.set_contact_placements(self.pos)
            c.set_constraint_rows(self.rows)
            c.set_friction_cones(MC, CD)
            c.set_constraint_bounds(self.bounds, 1.0e-3, TAU)
            c.set_friction_coefficients(self.mu)
            c.set_configuration_cost(**self.cost)
            c.set_configuration_ref_table(None)
            c.set_task_costs(None)
            c.set_contact_force_cost(None)
            c.set_foot_step_planner(None)
            c.set_initial_state(self.x0)
            c.set_line_search(False)
            c.solution_forget()
            c.set_graph(c is self.graph)
        return self

    def restore(self, ctx):
        ctx.upload(BUF_SOL, self.sol)
        ctx.contact_init_constraints()
        ctx.upload(BUF_STEP, np.ones((self.BATCH, 2)))
        ctx.upload(BUF_RIC, self.poison[0])
        ctx.upload(BUF_DIR, self.poison[1])
        ctx.line_search_clear()
        ctx.clear_status()

    def launch(self, ctx):
        self.err[id(ctx)] = ctx.contact_update_solution(TAU)

    def outputs(self, ctx):
        out = {w: _download(ctx, b, w) for b, w in ((BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_KKT, "kkt"), (BUF_CDD, "cdd"),
                                                   (BUF_CON, "con"), (BUF_SOL, "sol"))}
        out["step"] = ctx.download(BUF_STEP, (self.BATCH, 2))
        out["status"] = ctx.status()
        out["kkt_error"] = self.err.get(id(ctx))
        out["converged"] = _converged(ctx)
        return out

    def close(self):
        self.plain.close()
        self.graph.close()


@pytest.fixture(scope="module")
def twin_c_module():
    t = ClosedLoopTwin()
    yield t
    t.close()


@pytest.fixture
def Cl(twin_c_module):
    return twin_c_module.reset()


def _task_terms(tw):
    import foot_step_planner_cases as fsc
    return fsc.task_terms(tw.m)


def _ref_entries(tw, shift):
    from robotoc_amd.costs import TaskRefEntry
    out = (TaskRefEntry * tw.n)()
    for i in range(tw.n):
        out[i].R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        out[i].p[:] = [0.1 + shift, -0.05, 0.3 + 0.01 * i]
        out[i].active = 1
    return out


def _tasks_on(tw, shift=0.0):
    def fn(c):
        c.set_grid_times(tw.t)
        c.set_task_costs(_task_terms(tw))
        for k in range(5):
            c.set_task_ref_table(k, _ref_entries(tw, shift + 0.02 * k))
    return fn


def _force_cost(w):
    from robotoc_amd.costs import ContactForceCost
    fc = ContactForceCost()
    for k in range(4):
        fc.f_ref[k][:], fc.f_weight[k][:] = [0.0, 0.0, 70.0], [w, w, w]
        fc.fi_ref[k][:], fc.fi_weight[k][:] = [0.0, 0.0, 10.0], [w, w, w]
    return fc


def _foot_step_tick(tw):
    """plan, place, refs: what MPCTrot::resetContactPlacements does (tests/foot_step_planner_cases.py: tick)"""
    import foot_step_planner_cases as fsc
    from robotoc_amd import capi
    T = fsc.Trot.__new__(fsc.Trot)
    T.nph, T.start, T.period_swing, T.period_stance, T.height = 2, 0.005, 0.018, 0.011, 0.08

    def fn(c):
        _tasks_on(tw)(c)
        c.set_foot_step_planner(fsc.planner_structs(True, False, capi.PROJECT_YAW, range(tw.BATCH)))
        c.foot_step_planner_init()
        c.foot_step_plan(0.0, 0b1111, 4)
        c.foot_step_place(tw.phase)
        c.foot_step_refs(T.refs(), tw.phase, np.array([0b1111, 0b1001, 0b1111], dtype=np.uint32))
    return fn


def _reads(option, value):
    return Effect("rtoc_get_option reads the new value; evalKKT's arithmetic may or may not keep its bits",
                  lambda tw, before, after: all(c.get_option(option) == value for c in (tw.plain, tw.graph)))


def _model_again(tw, dpp):
    def fn(c):
        _set_option(OPT_LINEARIZE_DOFS_PER_PASS, dpp)(c)
        c.set_robot_model(tw.m)   # ends the per-instance placement table and the planner
        c.set_contact_placements(tw.pos)
    return fn


def _c_cases(tw):
    """name -> [(mutation, effect)]: the steps of a case, each a full protocol"""
    x1 = tw.x0.copy()
    x1[:, 7:19] += 0.05
    rot = np.tile(np.eye(3).reshape(-1), (tw.n, 4, 1))
    qtab = np.tile(tw.x0[0, :tw.m.nq], (tw.n, 1))
    qtab[:, 7:] += 0.1
    rows_on = [1] * tw.n
    return {
        "set_contact_schedule": [(lambda c: c.set_contact_schedule(tw.masks, tw.pos[1]), None),
                                 (lambda c: c.set_contact_schedule(tw.masks, tw.pos[0], rot), None)],
        "set_contact_placements": [(lambda c: c.set_contact_placements(tw.pos[0]), None),          # per instance -> shared
                                   (lambda c: c.set_contact_placements(tw.pos[::-1].copy()), None),  # shared -> per instance
                                   (lambda c: c.set_contact_placements(tw.pos), None)],
        "hold_contact_placements": [(lambda c: c.set_contact_placements(tw.pos[0] + 0.01), None),   # shared
                                    (lambda c: c.hold_contact_placements(0b1111, 0, 3, "x0"), None)],
        "task_costs": [(_tasks_on(tw), None), (_tasks_on(tw, 0.05), None),
                       (lambda c: c.set_grid_times(tw.t + 0.5), Effect("table references do not read the time: the results do not change",
                                                                      lambda t, b, a: not differing(b, a))),
                       (lambda c: c.set_task_costs(None), None)],
        "set_contact_force_cost": [(lambda c: c.set_contact_force_cost(_force_cost(1.0e-2)), None),
                                   (lambda c: c.set_contact_force_cost([_force_cost(1.0e-2), _force_cost(3.0e-2)], per_instance=True), None),
                                   (lambda c: c.set_contact_force_cost(None), None)],
        "set_configuration_cost": [(lambda c: c.set_configuration_cost(**dict(tw.cost, v_weight=np.full(tw.m.nv, 2.0))), None)],
        "set_configuration_ref_table": [(lambda c: c.set_configuration_ref_table(qtab), None),
                                        (lambda c: c.set_configuration_ref_table(np.stack([qtab, qtab + 0.05])), None),
                                        (lambda c: c.set_configuration_ref_table(None), None)],
        "set_barrier_param": [(lambda c: c.set_barrier_param(1.0e-2, 0.9), None)],
        "set_constraint_bounds": [(lambda c: c.set_constraint_bounds(0.9 * tw.bounds, 5.0e-3, 0.9), None)],
        "set_friction_coefficients": [(lambda c: c.set_friction_coefficients(np.full(4, 0.5)), None)],
        "set_initial_state": [(lambda c: c.set_initial_state(x1), None)],
        "set_robot_model": [(_model_again(tw, 9), _reads(OPT_LINEARIZE_DOFS_PER_PASS, 9)),
                            (_model_again(tw, 0), _reads(OPT_LINEARIZE_DOFS_PER_PASS, 18))],
        "foot_step_tick": [(_foot_step_tick(tw), None)],
        "contact_inv_damping": [(_set_option(OPT_CONTACT_INV_DAMPING, _bits(1.0e-3)), None)],
        "switching_transport": [(_set_option(OPT_SWITCHING_TRANSPORT, 1), None), (_set_option(OPT_SWITCHING_TRANSPORT, 0), None)],
        "cone_jacobian": [(_set_option(OPT_CONE_JACOBIAN, 1), _reads(OPT_CONE_JACOBIAN, 1))],
        "linearize_fused": [(_set_option(OPT_LINEARIZE_FUSED, 1), _reads(OPT_LINEARIZE_FUSED, 1))],
        "linearize_dofs_per_pass": [(_set_option(OPT_LINEARIZE_DOFS_PER_PASS, 6), _reads(OPT_LINEARIZE_DOFS_PER_PASS, 6)),
                                    (_set_option(OPT_LINEARIZE_DOFS_PER_PASS, 0), _reads(OPT_LINEARIZE_DOFS_PER_PASS, 18))],
        "solution_store": [(lambda c: c.solution_store(0.0), Effect("a solution is stored; the iteration does not read it",
                                                                     lambda t, b, a: t.graph.solution_stored() == t.n and not differing(b, a))),
                           (lambda c: c.solution_forget(), Effect("nothing is stored any more",
                                                                  lambda t, b, a: t.graph.solution_stored() == 0 and not differing(b, a)))],
    }


C_CASES = ("set_contact_schedule", "set_contact_placements", "hold_contact_placements", "task_costs", "set_contact_force_cost",
           "set_configuration_cost", "set_configuration_ref_table", "set_barrier_param", "set_constraint_bounds",
           "set_friction_coefficients", "set_initial_state", "set_robot_model", "foot_step_tick", "contact_inv_damping",
           "switching_transport", "cone_jacobian", "linearize_fused", "linearize_dofs_per_pass", "solution_store")


@pytest.mark.parametrize("name", C_CASES)
def test_c_closed_loop(Cl, name):
    steps = _c_cases(Cl)[name]
    for k, (mutate, effect) in enumerate(steps):
        Cl.case(mutate, Cl.launch, effect=effect, name="%s, step %d" % (name, k))
    assert (Cl.plain.status() == 0).all()


def test_c_the_case_list_is_the_case_table(Cl):
    assert sorted(_c_cases(Cl)) == sorted(C_CASES)


def test_c_line_search_on_and_off(Cl):
    """with the line search the iteration synchronises with the host and is never replayed; once it is off, graphing resumes"""
    searched = Effect("rtoc_line_search_trials counts trial evaluations on both contexts",
                      lambda tw, b, a: all(c.line_search_trials() >= 1 for c in (tw.plain, tw.graph)))
    Cl.case(lambda c: c.set_line_search(True), Cl.launch, effect=searched, name="line search on", replay_after=False)
    merit = Effect("the merit terms of the last search are there, the same on both contexts",
                   lambda tw, b, a: all(np.array_equal(x, y) and np.isfinite(x).all() for x, y in zip(tw.plain.line_search_merit_terms(), tw.graph.line_search_merit_terms())))
    Cl.case(lambda c: c.set_line_search_method("merit"), Cl.launch, effect=merit, name="merit backtracking", replay_before=False, replay_after=False)
    n_off = []
    resumed = Effect("the iteration is replayed again", lambda tw, b, a: tw.replay_count() >= n_off[0] + 2)

    def off(c):
        c.set_line_search(False)
        c.set_line_search_method("filter")
        n_off[:] = [Cl.replay_count()]
    Cl.case(off, Cl.launch, effect=resumed, name="line search off", replay_before=False)
    assert (Cl.plain.status() == 0).all()


def test_c_solution_interpolate_is_a_launch(Cl):
    """store, then interpolate onto the same grid: RTOC_BUF_SOL is rewritten by a kernel outside the sequence, which is replayed on it"""
    def regrid(c):
        c.upload(BUF_SOL, Cl.sol)
        c.solution_store(0.0)
    Cl.both(regrid)

    def launch(c):
        c.solution_interpolate(0.005)
        Cl.launch(c)
    x1 = Cl.x0.copy()
    x1[:, 7:19] += 0.01
    Cl.case(lambda c: c.set_initial_state(x1), launch, name="interpolated warm start")


def test_c_wrench_cones_and_their_params(oracle):
    """iCub's soles (tests/per_instance_placement_cases.py: 8 grid points, batch 2) with contact wrench cones on the device: the cone
    table is read by rtoc_contact_init_constraints and rtoc_contact_eval_kkt, outside the captured iteration"""
    import per_instance_placement_cases as pic
    from robotoc_amd import capi
    P = pic.icub_case(oracle)
    n, nu = len(P.grids), P.m.nv - 6
    rows = joint_limit_rows(P.dims)[:4 * nu]   # position and velocity limits: room for the 2 x 17 cone rows

    def make():
        c = capi.Context(P.dims, n, P.batch, 0)
        c.set_grid(P.grids)
        c.set_robot_model(P.m)
        c.set_contact_schedule(P.masks)
        c.set_contact_placements(P.pos, P.rot)
        c.set_constraint_rows(rows)
        c.set_wrench_cones(2)
        c.set_constraint_bounds(P.bounds[:4 * nu], 1.0e-3, TAU)
        c.set_wrench_cone_params(np.array([[0.05, 0.03, 0.7], [0.05, 0.03, 0.6]]))
        c.set_configuration_cost(**P.cost)
        c.set_initial_state(P.x0)
        return c
    err = {}
    poison = (np.full((P.batch, n, capi.layout_for(P.dims).ric.stride), np.nan), np.full((P.batch, n, capi.layout_for(P.dims).dir.stride), np.nan))

    def restore(c):
        c.upload(BUF_SOL, P.sol)
        c.contact_init_constraints()
        c.upload(BUF_RIC, poison[0])
        c.upload(BUF_DIR, poison[1])
        c.clear_status()

    def launch(c):
        err[id(c)] = c.contact_update_solution(TAU)

    def outputs(c):
        out = {w: _download(c, b, w) for b, w in ((BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_KKT, "kkt"), (BUF_CDD, "cdd"), (BUF_CON, "con"),
                                                   (BUF_SOL, "sol"))}
        out.update(step=c.download(BUF_STEP, (P.batch, 2)), status=c.status(), kkt_error=err.get(id(c)), converged=_converged(c))
        out["cone"] = c.download(BUF_CONE, (c.buffer_count(BUF_CONE),))
        return out
    tw = _inert_twin(make, restore, outputs)
    try:
        tw.case(lambda c: c.set_wrench_cone_params(np.array([[0.06, 0.04, 0.5], [0.04, 0.03, 0.8]])), launch, name="other soles")
        # rtoc_set_wrench_cones accepted between replays: the cone kernels leave the captured sequence and join it again
        tw.case(lambda c: c.set_wrench_cones(0), launch, name="wrench cones off", recapture=True, guard=WRITTEN)
        tw.case(lambda c: c.set_wrench_cones(2), launch, name="wrench cones on again", recapture=True, guard=WRITTEN)
        assert (tw.plain.status() == 0).all() and np.isfinite(tw.last["kkt_error"]).all()
    finally:
        tw.plain.close()
        tw.graph.close()


# ---- paths that are not graphed: the option is inert there ---------------------------------------------------------------------------
def _inert_twin(make, restore, outputs):
    a, b = make(), make()
    b.set_graph(True)
    return Twin(a, b, restore, outputs, lambda c: c.graph_replay_count())


def _arm_contexts():
    """the fixed-base arm of tests/test_unconstr_closed_loop.py's kind: iiwa14, 5 grid points, batch 2"""
    from robotoc_amd import capi, robot_model as rm
    from robotoc_amd.grid import uniform_grid
    m, dims = rm.load_named("iiwa14"), iiwa14_dims()
    nv, n, B = m.nv, 5, 2
    rng = np.random.default_rng(3)
    S = Records(capi.layout_for(dims), "sol")
    x0 = 0.3 * rng.uniform(-1, 1, (B, 2 * nv))
    sol = S.zeros(B, n)
    S.f(sol, "q")[..., :nv], S.f(sol, "v")[...] = x0[:, None, :nv], x0[:, None, nv:]
    cost = dict(q_ref=np.zeros(nv), v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0), v_weight=np.full(nv, 1.0),
                a_weight=np.full(nv, 0.01), u_weight=np.full(nv, 0.01), q_weight_terminal=np.full(nv, 10.0), v_weight_terminal=np.full(nv, 1.0),
                q_weight_impact=np.zeros(nv), v_weight_impact=np.zeros(nv), dv_weight_impact=np.zeros(nv))

    def make(parnmpc=False):
        c = capi.Context(dims, n, B, 0)
        if parnmpc:
            c.parnmpc_set_horizon(n)
        else:
            c.set_grid(uniform_grid(n - 1, 0.05))
        c.set_robot_model(m)
        c.set_configuration_cost(**cost)
        c.set_initial_state(x0)
        return c

    def restore(c):
        c.upload(BUF_SOL, sol)
        c.clear_status()

    def outputs(c):
        out = {w: _download(c, b, w) for b, w in ((BUF_DIR, "dir"), (BUF_RIC, "ric"), (BUF_KKT, "kkt"), (BUF_SOL, "sol"))}
        out["status"] = c.status()
        return out
    return make, restore, outputs


def test_inert_unconstr_update_solution():
    """rtoc_unconstr_update_solution launches its sequence plainly whatever RTOC_OPT_GRAPH says, with both recursions
    (RTOC_OPT_UNCONSTR_DENSE) and with the line search"""
    make, restore, outputs = _arm_contexts()
    tw = _inert_twin(make, restore, outputs)
    try:
        run = lambda c: c.unconstr_update_solution(0.05)
        first = tw.inert(run, "unconstrained solver")
        assert (tw.plain.status() == 0).all()
        tw.both(_set_option(OPT_UNCONSTR_DENSE, 1))
        dense = tw.inert(run, "unconstrained solver, dense recursion")
        assert tw.plain.get_option(OPT_UNCONSTR_DENSE) == 1 and first["sol"] is not None and dense["sol"] is not None
        tw.both(lambda c: c.set_line_search(True))
        tw.inert(run, "unconstrained solver, line search")
        tw.both(lambda c: c.set_line_search(False))
        tw.both(_set_option(OPT_UNCONSTR_DENSE, 0))
        again = tw.inert(run, "unconstrained solver again")
        # (the dense recursion leaves its materialised A, B in the KKT records, which the structured one does not rewrite)
        assert [k for k in differing(first, again) if k != "kkt"] == []
    finally:
        tw.plain.close()
        tw.graph.close()


def test_inert_parnmpc():
    """the ParNMPC horizon: rtoc_parnmpc_update_solution is not graphed; the auxiliary matrices set from the host act on the next
    call of both contexts alike"""
    make, restore, outputs = _arm_contexts()
    tw = _inert_twin(lambda: make(parnmpc=True), restore, outputs)
    try:
        def run(c):
            c.parnmpc_init_backward_correction()
            c.parnmpc_update_solution(0.05)
        first = tw.inert(run, "ParNMPC")
        assert (tw.plain.status() == 0).all()
        aux = tw.plain.parnmpc_get_aux_mat()
        tw.both(lambda c: c.parnmpc_set_aux_mat(2.0 * aux))
        second = tw.inert(lambda c: c.parnmpc_update_solution(0.05), "ParNMPC, auxiliary matrices from the host")
        assert differing(first, second)
    finally:
        tw.plain.close()
        tw.graph.close()


# what tests/graph_mutators.py may name: the test functions of this module and, of the parametrised ones, their cases
CASE_IDS = {
    "test_r_option": sorted(R_OPTION_STEPS),
    "test_c_closed_loop": list(C_CASES),
}
