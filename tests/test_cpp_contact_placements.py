"""ConfigurationCostSource::setContactPlacements (robotoc_amd/host/robotoc_hip_device_source.hpp) through robotoc::OCPSolver:
tests/cpp/contact_placements_test.cpp gives the batch-shared placements WRONG (every foot at the origin) and the robot's real
footholds per instance.  The solve converges and the feet end on the real footholds only if schedule() passed the per-instance
table on to the device.  The robot stands away from the origin and yawed, so the two sets of footholds are metres apart."""
import subprocess

import numpy as np
import pytest

from per_instance_placement_cases import Q_ANYMAL, _yaw
from robotoc_amd import robot_model as rm
from robotoc_amd.robot_model import MAX_JOINTS
from test_cpp_host import _build


def test_cpp_contact_placements_program_compiles():
    import os
    assert os.path.exists(_build("contact_placements_test"))


@pytest.mark.gpu
def test_cpp_source_passes_per_instance_placements_on(tmp_path, oracle):
    exe = _build("contact_placements_test")
    m = rm.load_named("anymal")
    N, dt = 10, 0.02
    nv, nq = m.nv, m.nq
    stand = _yaw(Q_ANYMAL, 1.5, -0.8, 0.7)
    feet = np.array([oracle.rbd_contact_position(m, stand, c) for c in range(4)])
    wq = np.concatenate([np.full(6, 10.0), np.full(12, 0.1)])
    cost = np.zeros((12, MAX_JOINTS))
    for k, val in ((0, stand), (3, wq), (4, np.full(nv, 1.0)), (5, np.full(nv, 1e-3)), (6, np.full(12, 1e-3)), (7, 10.0 * wq), (8, np.full(nv, 1.0))):
        cost[k, :len(val)] = val
    q0 = stand.copy()
    q0[:7] = oracle.se3_integrate(stand[:7], np.array([0.005, -0.004, 0.003, 0.01, -0.006, 0.004]))
    v0 = np.zeros(nv)
    mass = sum(m.mass[i] for i in range(m.njoints))
    f0 = np.concatenate([oracle.rbd_contact_placement(m, q0, c)[0].T @ np.array([0.0, 0.0, 9.81 * mass / 4]) for c in range(4)])
    u0 = oracle.rbd_eval(m, 0, q0, np.zeros(nv), np.zeros(nv), f0, np.zeros(12), 0b1111, feet.reshape(-1))[6:nv]
    prob = str(tmp_path / "anymal_standing.bin")
    with open(prob, "wb") as f:
        f.write(bytes(m))
        f.write(cost.tobytes())
        f.write(np.array([N], dtype=np.int32).tobytes())
        f.write(np.array([dt]).tobytes())
        for arr in (q0, v0, feet.reshape(-1), f0, u0):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    out_path = str(tmp_path / "out.bin")
    run = subprocess.run([exe, prob, out_path], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out_path)
    assert raw[1] == 1.0 and raw[2] < 1e-8
    qT = raw[4:].reshape(N + 1, nq)[-1]
    assert max(np.abs(oracle.rbd_contact_position(m, qT, c) - feet[c]).max() for c in range(4)) < 5e-3
