"""rtoc_solution_store / rtoc_solution_interpolate on the device against the numpy restatement of SolutionInterpolator
(tests/solution_interpolator_restatement.py), on the grids of tests/solution_interpolation_cases.py (their branch coverage is
checked on the CPU, tests/test_solution_interpolator_restatement.py).  Bounds, field by field: copied and zeroed entries bit for
bit; linear blends 4 eps max(|a|, |b|), eps = 2.2e-16 (the two evaluation orders of (1 - alpha) a + alpha b, with and without
contraction to fused multiply-adds, differ by at most three roundings); base position and quaternion 1e-13 max(1, |p|), the bound of
the project's SE(3) formulas.  The times on both sides are the running sum of the time steps the DEVICE holds, so alpha is
bit-identical.  Before every interpolation RTOC_BUF_SOL is filled with NaN over its whole capacity: an entry the kernel leaves
alone shows."""
import ctypes as C

import numpy as np
import pytest

import solution_interpolation_cases as cases
import solution_interpolator_restatement as sir
from robotoc_amd import capi
from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import BUF_SOL

pytestmark = pytest.mark.gpu
BAD_ARG, NOT_READY = -1, -5


def _anymal_ctx(batch, max_stages=12):
    model, dims, L, shape = cases.anymal_shape()
    ctx = capi.Context(dims, max_stages, batch)
    ctx.set_robot_model(model)
    return ctx, model, shape


def _set_side(ctx, side, phase_based):
    """the grid, the schedule and, with `phase_based`, the STO problem with every instance's own event times"""
    n = len(side["grids"])
    ctx.set_grid(side["grids"])
    ctx.set_contact_schedule(side["masks"], np.zeros((n, 4, 3)))
    if phase_based:
        ctx.sto_set_problem(0.0, cases.T, side["events"], np.zeros(3))
        return ctx.sto_time_steps()
    return np.array([[g.dt for g in side["grids"]]])


def _poison(ctx, shape):
    ctx.upload(BUF_SOL, np.full((ctx.batch, ctx.max_stages, shape.stride), np.nan))


def _records(ctx, shape):
    return ctx.download(BUF_SOL, (ctx.batch, ctx.nstages, shape.stride))


def _clone(ctx):
    h = C.c_void_p()
    assert capi.lib().rtoc_clone(ctx._h, C.byref(h)) == 0
    n = object.__new__(capi.Context)
    n.__dict__.update(ctx.__dict__)
    n._h = h
    return n


@pytest.mark.parametrize("phase_based", [True, False], ids=["sto", "shared_times"])
def test_anymal_against_the_restatement(phase_based):
    stored, new = cases.anymal_grids(phase_based)
    ctx, model, shape = _anymal_ctx(3)
    sol0 = cases.random_records(shape, 3, len(stored["grids"]), seed=21)
    dt0 = _set_side(ctx, stored, phase_based)
    ctx.upload(BUF_SOL, sol0)
    if phase_based:
        ctx.sto_correct_time_steps()
    ctx.solution_store(0.0)
    assert ctx.solution_stored() == len(stored["grids"])
    dt1 = _set_side(ctx, new, phase_based)
    assert ctx.solution_stored() == len(stored["grids"])   # the store survives rtoc_set_grid with another nstages
    _poison(ctx, shape)
    ctx.solution_interpolate(0.0)
    got = _records(ctx, shape)
    want, branches = cases.restate(shape, stored, new, sol0, 0.0, 0.0, dt0, dt1)
    kind, operand = cases.classify(shape, stored, new, sol0, 0.0, 0.0, dt0, dt1)
    taken = set().union(*[names for per_point in branches for names in per_point])
    if phase_based:   # with the device's own time steps the instances still fall into every branch
        assert taken >= set(sir.BRANCHES) - {"stepped_back", "lift_partial"}, taken
    cases.compare(shape, got, want, kind, operand, "device, anymal " + ("per-instance" if phase_based else "shared") + " times")
    ctx.close()


def _rotvec(q):
    v, w = np.asarray(q[:3]), q[3]
    n = np.linalg.norm(v)
    return np.zeros(3) if n == 0.0 else (2.0 * np.arctan2(n, w) / n) * v


def test_branch_points_of_the_logarithm():
    """stored grid: t = 0 (the identity) and t = 1 (a placement of tests/golden/lie_branch_points.npz); new grid: a point at 0.5.
    Twice the rotation vector of its quaternion is log3 of the fixture's rotation, held to the fixture as
    tests/test_lie_branch_points_host.py::test_planner_header_log3 holds the header, half-turn sign rule included."""
    from test_lie_branch_points_host import BOUND, GOLDEN, expected
    d = np.load(GOLDEN)
    fx = {k: d[k] for k in d.files}
    n = len(fx["angle"])
    ctx, model, shape = _anymal_ctx(n, max_stages=3)
    sol0 = np.zeros((n, 2, shape.stride))
    o = shape.off["q"]
    sol0[:, 0, o + 6] = 1.0
    sol0[:, 1, o:o + 3], sol0[:, 1, o + 3:o + 7] = fx["pos"], fx["quat"]
    for grids in (uniform_grid(1, 1.0, dimf=12), uniform_grid(2, 0.5, dimf=12)):
        ctx.set_grid(grids)
        ctx.set_contact_schedule(np.full(len(grids), 0b1111, dtype=np.uint32), np.zeros((len(grids), 4, 3)))
        if len(grids) == 2:
            ctx.upload(BUF_SOL, sol0)
            ctx.solution_store(0.0)
    _poison(ctx, shape)
    ctx.solution_interpolate(0.0)
    got = _records(ctx, shape)
    worst = (0.0, 0.0, -1)
    for i in range(n):
        w = 2.0 * _rotvec(got[i, 1, o + 3:o + 7])
        want, = expected(fx, i, w, ("log6",))
        r = np.abs(w - want[3:]).max() / BOUND   # the rotation vector does not see p: the plain 1e-13, as for the header
        if r > worst[0]:
            worst = (r, fx["angle"][i], i)
    print("device interpolation, log3 at the branch points: worst error / bound %.2e at angle %.10g (case %d)" % worst)
    assert worst[0] <= 1.0
    # the end points are copies
    assert np.array_equal(got[:, 0], sol0[:, 0]) and np.array_equal(got[:, 2, o:o + 7], sol0[:, 1, o:o + 7])
    ctx.close()


def test_fixed_base_without_a_schedule():
    model, dims, L, shape = cases.iiwa_shape()
    stored, new = cases.iiwa_grids()
    ctx = capi.Context(dims, 6, 2)
    sol0 = cases.random_records(shape, 2, len(stored["grids"]), seed=22)
    ctx.set_grid(stored["grids"])
    ctx.upload(BUF_SOL, sol0)
    ctx.solution_store(0.0)
    ctx.set_grid(new["grids"])
    _poison(ctx, shape)
    ctx.solution_interpolate(0.0)
    got = _records(ctx, shape)
    want, _ = cases.restate(shape, stored, new, sol0, 0.0, 0.0)
    kind, operand = cases.classify(shape, stored, new, sol0, 0.0, 0.0)
    cases.compare(shape, got, want, kind, operand, "device, iiwa14")
    ctx.close()


def test_same_grid_in_same_solution_out():
    stored, _ = cases.anymal_grids(True)
    ctx, model, shape = _anymal_ctx(3)
    n = len(stored["grids"])
    # base rotations below 120 degrees: beyond, the quaternion of a rotation matrix comes back with its largest component positive
    # (the planner header's rule), which for half of the quaternions with w > 0 is the other sign
    sol0 = cases.random_records(shape, 3, n, seed=23, max_angle=1.9, xi_everywhere=False)
    for i, g in enumerate(stored["grids"]):   # xi lives where a switching constraint does
        if g.switching_constraint:
            sol0[:, i, shape.off["xi"]:shape.off["xi"] + g.dims] = np.random.default_rng(24).normal(size=(3, g.dims))
    _set_side(ctx, stored, True)
    ctx.upload(BUF_SOL, sol0)
    ctx.sto_correct_time_steps()
    ctx.solution_store(0.0)
    _poison(ctx, shape)
    ctx.solution_interpolate(0.0)
    got = _records(ctx, shape)
    o = shape.off["q"]
    pose = np.zeros(shape.stride, dtype=bool)
    pose[o:o + 7] = True
    want = sol0.copy()
    for name in ("u", "a", "f", "beta", "mu", "nu_passive"):   # modifyTerminalSolution
        shape.f(want[:, -1].T, name)[:] = 0.0
    k = stored["types"].index(sir.GRID_IMPACT)
    for name in ("u", "a", "nu_passive"):   # the copied impact (modifyImpactSolution)
        shape.f(want[:, k].T, name)[:] = 0.0
    for i in range(n):   # behind the packed rows of a stack the interpolation leaves zeros
        rows = model.active_rows(int(stored["masks"][i]))
        for name in ("f", "mu"):
            shape.f(want[:, i].T, name)[rows:] = 0.0
    assert np.array_equal(got[:, :, ~pose].view(np.uint64), want[:, :, ~pose].view(np.uint64))
    err = np.abs(got[:, :, pose] - want[:, :, pose]).max()
    print("same grid in, same solution out: base pose off by %.2e (bound 1e-14)" % err)
    assert err <= 1e-14
    for name in ("u", "a", "f", "beta", "mu", "nu_passive"):
        assert not shape.f(got[:, -1].T, name).any()
    ctx.close()


def test_nothing_stored_forget_and_clone():
    stored, new = cases.anymal_grids(True)
    ctx, model, shape = _anymal_ctx(3)
    sol0 = cases.random_records(shape, 3, len(stored["grids"]), seed=25)
    _set_side(ctx, stored, True)
    ctx.upload(BUF_SOL, sol0)
    assert ctx.solution_stored() == 0
    ctx.solution_interpolate(0.0)   # nothing stored: RTOC_OK, nothing written
    assert np.array_equal(_records(ctx, shape).view(np.uint64), sol0.view(np.uint64))
    ctx.sto_correct_time_steps()
    ctx.solution_store(0.0)
    ctx.solution_forget()
    assert ctx.solution_stored() == 0
    ctx.solution_interpolate(0.0)
    assert np.array_equal(_records(ctx, shape).view(np.uint64), sol0.view(np.uint64))
    ctx.solution_store(0.0)
    _set_side(ctx, new, True)
    other = _clone(ctx)
    assert other.solution_stored() == len(stored["grids"])
    for c in (ctx, other):
        _poison(c, shape)
        c.solution_interpolate(0.0)
    a, b = _records(ctx, shape), _records(other, shape)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    other.close()
    ctx.close()


def test_refusals_write_nothing():
    lib = capi.lib()
    stored, new = cases.anymal_grids(False)
    model, dims, L, shape = cases.anymal_shape()
    rng = np.random.default_rng(26)

    def refused(ctx, code, stride):
        before = ctx.download(BUF_SOL, (ctx.batch, ctx.max_stages, stride))
        assert lib.rtoc_solution_store(ctx._h, 0.0) == code
        assert lib.rtoc_solution_interpolate(ctx._h, 0.0) == code
        assert np.array_equal(ctx.download(BUF_SOL, (ctx.batch, ctx.max_stages, stride)).view(np.uint64), before.view(np.uint64))
        assert ctx.solution_stored() == 0

    # no grid
    ctx = capi.Context(dims, 12, 2)
    ctx.upload(BUF_SOL, rng.normal(size=(2, 12, shape.stride)))
    refused(ctx, NOT_READY, shape.stride)
    # a grid, but contact rows without a model
    ctx.set_grid(stored["grids"])
    refused(ctx, NOT_READY, shape.stride)
    # a model, but no contact schedule
    ctx.set_robot_model(model)
    refused(ctx, NOT_READY, shape.stride)
    # a schedule, but one that was set for the grid before this one: its masks belong to another grid
    ctx.set_contact_schedule(stored["masks"], np.zeros((len(stored["grids"]), 4, 3)))
    ctx.set_grid(new["grids"])
    refused(ctx, NOT_READY, shape.stride)
    ctx.set_grid(stored["grids"])
    refused(ctx, NOT_READY, shape.stride)
    # an STO problem whose time steps date from before the last rtoc_set_grid (same events, so the problem stays set)
    ctx.set_contact_schedule(stored["masks"], np.zeros((len(stored["grids"]), 4, 3)))
    ctx.sto_set_problem(0.0, cases.T, stored["events"][0], np.zeros(3))
    ctx.set_grid(new["grids"])
    ctx.set_contact_schedule(new["masks"], np.zeros((len(new["grids"]), 4, 3)))
    refused(ctx, NOT_READY, shape.stride)
    ctx.sto_correct_time_steps()
    ctx.solution_store(0.0)
    assert ctx.solution_stored() == len(new["grids"])
    ctx.solution_forget()
    ctx.close()
    # a store whose contacts are not those of the model now set
    ctx = capi.Context(dims, 12, 2)
    ctx.upload(BUF_SOL, rng.normal(size=(2, 12, shape.stride)))
    ctx.set_grid(stored["grids"])
    ctx.set_robot_model(model)
    ctx.set_contact_schedule(stored["masks"], np.zeros((len(stored["grids"]), 4, 3)))
    ctx.solution_store(0.0)
    fewer = type(model).from_buffer_copy(model)
    fewer.ncontacts = 3
    ctx.set_robot_model(fewer)
    before = ctx.download(BUF_SOL, (2, 12, shape.stride))
    assert lib.rtoc_solution_interpolate(ctx._h, 0.0) == BAD_ARG
    assert lib.rtoc_solution_interpolate(ctx._h, float("nan")) == BAD_ARG
    assert np.array_equal(ctx.download(BUF_SOL, (2, 12, shape.stride)).view(np.uint64), before.view(np.uint64))
    ctx.close()
    # a ParNMPC horizon
    _, idims, _, ishape = cases.iiwa_shape()
    ctx = capi.Context(idims, 6, 2)
    ctx.upload(BUF_SOL, rng.normal(size=(2, 6, ishape.stride)))
    assert lib.rtoc_parnmpc_set_horizon(ctx._h, 4) == 0
    refused(ctx, BAD_ARG, ishape.stride)
    ctx.close()
