"""robotoc::BipedWalkFootStepPlanner of robotoc_amd/host/robotoc_hip_planner.hpp over the C ABI:
tests/cpp/biped_walk_foot_step_planner_test.cpp plans for five iCubs with their own step lengths and yaws through the header class
and places the plan; here the plan is held to the numpy restatement of the reference (tests/biped_walk_restatement.py) at the bounds
of tests/test_biped_walk_gpu.py, and the two placement tables to the plan, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import biped_walk_cases as bc
import foot_step_planner_cases as cases
from helpers import check_parity
from robotoc_amd import capi
from robotoc_amd.types import grid_array, icub_dims
from test_cpp_host import _build


def test_cpp_biped_walk_foot_step_planner_program_compiles():
    assert os.path.exists(_build("biped_walk_foot_step_planner_test"))


@pytest.mark.gpu
def test_cpp_biped_walk_planner_plans_and_places_like_the_restatement(tmp_path, oracle):
    exe = _build("biped_walk_foot_step_planner_test")
    T = bc.WalkGrid(True)
    m, x0 = bc.states("icub32", 8, False)
    steps, B = 4, bc.BATCH
    prob, out_path = str(tmp_path / "walk.bin"), str(tmp_path / "out.bin")
    with open(prob, "wb") as f:
        f.write(bytes(icub_dims(m.nv)))
        f.write(np.array([T.n], dtype=np.int32).tobytes())
        f.write(bytes(grid_array(T.grids)))
        f.write(bytes(m))
        f.write(np.array([B], dtype=np.int32).tobytes())
        for arr in (x0, cases.STEP_LENGTH, cases.STEP_YAW):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(T.phase, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(T.masks, dtype=np.uint32).tobytes())
        f.write(np.array([steps], dtype=np.int32).tobytes())
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    # the same calls on the restatement: with double support, at 0b11 and then at 0b01
    feet, surfaces, c0 = bc.kinematics(oracle, "icub32", m, x0)
    planners = bc.restated_planners(False, True, capi.PROJECT_YAW)
    for b, pl in enumerate(planners):
        pl.init(x0[b, :m.nq], feet[b], c0[b])
        for t, status in ((0.0, 0b11), (0.1, 0b01)):
            assert pl.plan(t, x0[b, :m.nq], feet[b], surfaces[b], x0[b, m.nq:], status, steps)
    raw = np.fromfile(out_path)
    size = int(raw[0])
    assert size == steps + 2 and raw[1] == planners[0].current_step == 1
    o = 2
    parts = {}
    for name, shape in (("pos", (B, size, 2, 3)), ("surf", (B, size, 2, 3, 3)), ("com", (B, size, 3)), ("R", (B, size, 3, 3)), ("ok", (B,)),
                        ("tab_p", (B, T.n, 2, 3)), ("tab_r", (B, T.n, 2, 3, 3)), ("inst", (1,))):
        count = int(np.prod(shape))
        parts[name] = raw[o:o + count].reshape(shape)
        o += count
    assert o == raw.size and (parts["ok"] == 1.0).all() and parts["inst"][0] == 1.0
    want_p = np.array([[pl.contact_positions(s) for s in range(size)] for pl in planners])
    want_S = np.array([[pl.contact_surfaces(s) for s in range(size)] for pl in planners])
    scale = max(1.0, np.abs(want_p).max())
    check_parity("C++ biped walk planner: contact positions", np.abs(parts["pos"] - want_p).max() / scale, 1e-14 * size)
    check_parity("C++ biped walk planner: contact surfaces", np.abs(parts["surf"] - want_S).max(), 1e-14 * size)
    check_parity("C++ biped walk planner: CoM", np.abs(parts["com"] - np.array([[pl.com(s) for s in range(size)] for pl in planners])).max() / scale, 1e-14 * size)
    check_parity("C++ biped walk planner: R", np.abs(parts["R"] - np.array([[pl.R(s) for s in range(size)] for pl in planners])).max(), 1e-14 * size)
    for i in range(T.n):
        assert np.array_equal(parts["tab_p"][:, i], parts["pos"][:, T.phase[i] + 1])
        assert np.array_equal(parts["tab_r"][:, i], parts["surf"][:, T.phase[i] + 1])
