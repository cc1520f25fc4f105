"""The C++ table fill of a ConfigurationSpaceRefBase (robotoc_amd/host/robotoc_hip_task_costs.hpp: configurationRefTable)
against the Python one (costs.configuration_ref_table) on the one-cycle ANYmal trot at N = 40 with the same stub reference: the
same operations in the same order, equal to 1e-15.  The program (tests/cpp/configuration_ref_test.cpp) is host code; it also holds
the fill's order of questions and its refusal of a reference that is not finite."""
import subprocess

import numpy as np

from robotoc_amd import costs, robot_model as rm

from test_configuration_ref_host import StubRef
from test_contact_force_cost_host import _trot
from test_cpp_host import _build


def test_cpp_configuration_ref_table_equals_the_python_one():
    exe = _build("configuration_ref_test")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.returncode, run.stdout[-2000:], run.stderr)
    cs, grids, infos = _trot()
    m = rm.load_named("anymal")
    nv = m.nv
    q_ref, active = costs.configuration_ref_table(StubRef(), m, infos, 1.0 + np.arange(nv), np.full(nv, 2.0), np.zeros(nv))
    lines = run.stdout.splitlines()
    assert lines[0] == "grid %d" % len(grids)
    worst, n_active = 0.0, 0
    for i in range(len(grids)):
        w = lines[1 + i].split()
        assert w[0] == "row" and int(w[1]) == i and int(w[2]) == active[i], (i, w[:3])
        d = np.abs(np.array([float(x) for x in w[3:]]) - q_ref[i]).max()
        worst = max(worst, d)
        assert d <= 1e-15, (i, d)
        n_active += int(w[2])
    print("rows compared: %d (%d active), worst difference %.1e" % (len(grids), n_active, worst))
    assert 0 < n_active < len(grids)
    assert any(l.startswith("refused: [ConfigurationSpaceCost] the reference at grid point 3 ") for l in lines)
