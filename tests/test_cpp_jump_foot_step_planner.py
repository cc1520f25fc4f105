"""robotoc::JumpFootStepPlanner of robotoc_amd/host/robotoc_hip_planner.hpp over the C ABI:
tests/cpp/jump_foot_step_planner_test.cpp initialises a jump for five robots with their own jump lengths and yaws through the header
class, ticks once on the ground and once in the air (resetContactPlacements, setConfigurationRef) and reads everything back; here
the same calls go through the Python shell (robotoc_amd.planner.JumpFootStepPlanner), and the two read-backs are equal bit for bit:
both are the same device code.  tests/test_jump_planner_gpu.py holds that code to the restatement of the reference."""
import os
import subprocess

import numpy as np
import pytest

import jump_planner_cases as jc
from robotoc_amd import capi
from robotoc_amd.planner import JumpFootStepPlanner
from robotoc_amd.types import grid_array
from test_cpp_host import _build


def test_cpp_jump_foot_step_planner_program_compiles():
    assert os.path.exists(_build("jump_foot_step_planner_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("model", ("anymal", "icub32"))
def test_cpp_jump_planner_reads_back_what_the_python_shell_reads_back(tmp_path, model):
    exe = _build("jump_foot_step_planner_test")
    T = jc.JumpGrid(model)
    B, nf = jc.bc.BATCH, jc.feet_of(model)
    m, x0 = jc.states(model, 8, "any", B)
    x1 = jc.moved(m, x0)
    jumps = np.array([jc.command(b)[0] for b in range(B)])
    yaws = np.array([jc.command(b)[1] for b in range(B)])
    prob, out_path = str(tmp_path / "jump.bin"), str(tmp_path / "out.bin")
    with open(prob, "wb") as f:
        f.write(bytes(jc.dims_of(model, m)))
        f.write(np.array([T.n], dtype=np.int32).tobytes())
        f.write(bytes(grid_array(T.grids)))
        f.write(bytes(m))
        f.write(np.array([B], dtype=np.int32).tobytes())
        for arr in (x0, jumps, yaws):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(T.phase, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(T.masks, dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(x1, dtype=np.float64).tobytes())
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out_path)
    # the same calls through the Python shell
    ctx = capi.Context(jc.dims_of(model, m), T.n, B, 0)
    ctx.set_grid(T.grids)
    ctx.set_robot_model(m)
    ctx.set_contact_schedule(T.masks)
    pl = JumpFootStepPlanner(ctx, capi.PROJECT_YAW)
    pl.set_jump_pattern(jumps, yaws)
    pl.init(x0)
    o = 0
    for tick, (x, status, size, cur) in enumerate(((x0, T.full, 3, 0), (x1, 0, 2, 1))):
        assert pl.reset_contact_placements(0.1 * tick, status, T.phase, x)
        pl.set_configuration_ref()
        assert raw[o] == size == pl.size() and raw[o + 1] == cur == pl.current_step()
        o += 2
        tab_p, tab_r, inst = ctx.contact_placements()
        q_ref, active, q_inst = ctx.configuration_ref_table()
        assert inst and q_inst
        want = [np.stack([pl.contact_positions(s) for s in range(size)], axis=1), np.stack([pl.contact_surfaces(s) for s in range(size)], axis=1),
                np.stack([pl.com(s) for s in range(size)], axis=1), np.stack([pl.R(s) for s in range(size)], axis=1),
                pl.ok().astype(np.float64), pl.jump_length(), tab_p, tab_r, np.array([1.0]), q_ref, active.astype(np.float64)]
        assert want[0].shape == (B, size, nf, 3) and want[1].shape == (B, size, nf, 3, 3) and np.array_equal(want[5], jumps)
        for k, w in enumerate(want):
            got = raw[o:o + w.size].reshape(w.shape)
            o += w.size
            assert np.array_equal(got, w), (tick, k)
        assert want[4].all() and want[10].all()
    assert o == raw.size
    ctx.close()
