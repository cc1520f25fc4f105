"""The yardstick of rtoc_solution_interpolate (tests/solution_interpolator_restatement.py) against the two host mirrors of
SolutionInterpolator, and the branch coverage of the grids the device tests run (tests/solution_interpolation_cases.py).  No GPU.

(a) The restatement equals OCPSolver._interpolate of robotoc_amd/solver.py to 1e-15 relative, per field.  The two pick the
    quaternion of a rotation matrix differently once its trace is not positive (solver._R_quat keeps w > 0 down to w = 1e-6, the
    planner header and the restatement let the largest diagonal entry lead, so q and -q can come out): the records of this leg hold
    base rotations of at most 0.8 rad, whose blends keep a positive trace.  Every other leg runs unrestricted unit quaternions.
(b) The restatement equals the C++ SolutionInterpolator of robotoc_hip_planner.hpp through tests/cpp/solution_interpolator_test.cpp,
    within the bounds the device is held to (copies and zeros bit for bit, linear blends 4 eps max(|a|, |b|), base pose 1e-13).
(c) Branch coverage, a condition and not a measurement: front copy, back copy, matched impact with the xi transfer, matched lift,
    unmatched impact and lift blended by initEventSolution, an unmatched event in front of the stored terminal point on the partial
    path, full blend, partial blend before an event, a new grid point whose mask differs from both stored neighbours' -- each taken
    by an instance of the ANYmal case.  The step back over a stored point with dt <= 0 cannot be reached from times that are the
    running sum of non-negative time steps (such a point shares its time with its successor, and the search stops at the LAST
    stored point not after t): it is taken here by a stored grid whose times are given directly, as the C++ mirror's are, with
    the point behind an impact a rounding later than the impact; on the device the branch is kept and dead."""
import subprocess

import numpy as np

import solution_interpolation_cases as cases
import solution_interpolator_restatement as sir
from robotoc_amd.types import Records


def _mirror(model, L):
    from robotoc_amd.solver import OCPSolver
    s = object.__new__(OCPSolver)
    s.S, s.model, s.nc = Records(L, "sol"), model, model.ncontacts
    return s


def _setups():
    model, dims, L, shape = cases.anymal_shape()
    for phase_based in (True, False):
        stored, new = cases.anymal_grids(phase_based)
        yield "anymal, %s times" % ("per-instance" if phase_based else "shared"), model, dims, L, shape, stored, new, 3
    model, dims, L, shape = cases.iiwa_shape()
    stored, new = cases.iiwa_grids()
    yield "iiwa14", model, dims, L, shape, stored, new, 2


def test_grids_are_as_small_as_promised():
    stored, new = cases.anymal_grids(True)
    assert len(stored["grids"]) <= 10 and len(new["grids"]) <= 12
    assert sorted(stored["types"]).count(sir.GRID_LIFT) == 1 and stored["types"].count(sir.GRID_IMPACT) == 1
    assert new["types"].count(sir.GRID_LIFT) == 1 and new["types"].count(sir.GRID_IMPACT) == 1


def test_restatement_equals_solver_interpolate():
    worst = 0.0
    for label, model, dims, L, shape, stored, new, batch in _setups():
        sol0 = cases.random_records(shape, batch, len(stored["grids"]), seed=11, max_angle=0.8)
        want, _ = cases.restate(shape, stored, new, sol0, 0.0, 0.0)
        mirror = _mirror(model, L)
        for b in range(batch):
            d0, d1 = stored["dt"][b if len(stored["dt"]) > 1 else 0], new["dt"][b if len(new["dt"]) > 1 else 0]
            got = np.zeros_like(want[b])
            mirror._interpolate(stored["grids"], stored["masks"], sir.running_times(0.0, d0), d0, sol0[b], new["grids"], new["masks"],
                                sir.running_times(0.0, d1), got)
            for name in sir.FIELDS:
                for i in range(len(got)):
                    g, w = mirror.S.f(got[i], name), mirror.S.f(want[b][i], name)
                    ref = np.abs(w).max() if w.size else 0.0
                    err = np.abs(g - w).max() if w.size else 0.0
                    if ref == 0.0:
                        assert err == 0.0, (label, b, i, name)
                    else:
                        worst = max(worst, err / ref)
                        assert err <= 1e-15 * ref, (label, b, i, name, err / ref)
    print("restatement against OCPSolver._interpolate: worst relative error of a field %.2e (bound 1e-15)" % worst)


def _cpp(dims, shape, stored_types, t0s, dt0, masks0, sol0, types1, t1s, masks1):
    from test_cpp_host import _build
    exe = _build("solution_interpolator_test")
    lines = ["%d %d %d %d %d %d %d %s" % (dims.nv, dims.nu, dims.np, dims.nf_max, dims.ns_max, dims.nc_max, len(shape.rows),
                                          " ".join(str(r) for r in shape.rows))]
    lines.append(str(len(stored_types)))
    lines += ["%d %r %r %d" % (ty, float(t), float(d), int(m)) for ty, t, d, m in zip(stored_types, t0s, dt0, masks0)]
    lines += [" ".join(repr(float(x)) for x in rec) for rec in sol0]
    lines.append(str(len(types1)))
    lines += ["%d %r %d" % (ty, float(t), int(m)) for ty, t, m in zip(types1, t1s, masks1)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    out = run.stdout.splitlines()
    assert run.returncode == 0 and out and out[-1] == "ok %d" % len(types1), (run.returncode, run.stdout[-300:], run.stderr[-300:])
    return np.array([[float(x) for x in ln.split()] for ln in out[:-1]])


def test_restatement_equals_cpp_solution_interpolator():
    for label, model, dims, L, shape, stored, new, batch in _setups():
        sol0 = cases.random_records(shape, batch, len(stored["grids"]), seed=12)
        want, _ = cases.restate(shape, stored, new, sol0, 0.0, 0.0)
        kind, operand = cases.classify(shape, stored, new, sol0, 0.0, 0.0)
        got = np.zeros_like(want)
        for b in range(batch):
            d0, d1 = stored["dt"][b if len(stored["dt"]) > 1 else 0], new["dt"][b if len(new["dt"]) > 1 else 0]
            got[b] = _cpp(dims, shape, stored["types"], sir.running_times(0.0, d0), d0, stored["masks"], sol0[b], new["types"],
                          sir.running_times(0.0, d1), new["masks"])
        cases.compare(shape, got, want, kind, operand, "C++ SolutionInterpolator, " + label)


def _step_back_case(shape):
    """a stored grid whose times are given directly: the point behind the impact lies a rounding later than the impact itself"""
    stored, new = cases.anymal_grids(False)
    d0 = stored["dt"][0]
    t0s = sir.running_times(0.0, d0)
    k = stored["types"].index(sir.GRID_IMPACT)
    t0s[k + 1] = t0s[k] + 1e-12
    types1 = [sir.GRID_INTERMEDIATE, sir.GRID_INTERMEDIATE, sir.GRID_TERMINAL]
    t1s = np.array([0.0, t0s[k] + 5e-13, cases.T])
    return stored, t0s, d0, types1, t1s, np.array([0b1111, 0b1111, 0b1111], dtype=np.uint32), k


def test_branch_coverage():
    _, _, _, shape = cases.anymal_shape()
    taken = {}
    for phase_based in (True, False):
        stored, new = cases.anymal_grids(phase_based)
        sol0 = cases.random_records(shape, 3, len(stored["grids"]), seed=13)
        _, branches = cases.restate(shape, stored, new, sol0, 0.0, 0.0)
        for b, per_point in enumerate(branches):
            for i, names in enumerate(per_point):
                for n in names:
                    taken.setdefault((phase_based, n), []).append((b, i))
        for b, per_point in enumerate(branches):
            print("per-instance times" if phase_based else "shared times", "instance", b, [",".join(sorted(n)) for n in per_point])
    on_device = [n for n in sir.BRANCHES if n not in ("stepped_back", "lift_partial")]
    # with per-instance times (the run with an STO problem) every branch a device run can reach is taken
    missing = [n for n in on_device if (True, n) not in taken]
    assert not missing, missing
    # one unmatched event in front of the stored terminal point is asked for; this case's is the impact
    assert (True, "impact_partial") in taken
    # with shared times: the matched events and the plain blends at least (the sum of seven steps T / 7 may end a rounding short of
    # the stored horizon's end: the back copy is not asked of this run)
    for n in ("front", "impact_matched", "xi_transfer", "lift_matched", "full", "partial"):
        assert (False, n) in taken, n

    stored, t0s, d0, types1, t1s, masks1, k = _step_back_case(shape)
    sol0 = cases.random_records(shape, 1, len(stored["grids"]), seed=14)[0]
    sol1, branches = sir.interpolate(shape, stored["types"], t0s, d0, stored["masks"], sol0, types1, t1s, masks1)
    assert "stepped_back" in branches[1] and "partial" in branches[1]
    # alpha clamps at 1 in front of the impact: the velocity is that of the stored impact point
    assert np.array_equal(shape.f(sol1[1], "v"), shape.f(sol0[k], "v"))


def test_step_back_agrees_with_the_cpp_mirror():
    _, dims, _, shape = cases.anymal_shape()
    stored, t0s, d0, types1, t1s, masks1, k = _step_back_case(shape)
    sol0 = cases.random_records(shape, 1, len(stored["grids"]), seed=14)[0]
    args = (shape, stored["types"], t0s, d0, stored["masks"], sol0, types1, t1s, masks1)
    want, _ = sir.interpolate(*args)
    kind, operand = sir.classify(*args)
    got = _cpp(dims, *args)
    cases.compare(shape, got[None], want[None], kind[None], operand[None], "C++ SolutionInterpolator, step back")
