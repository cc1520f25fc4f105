"""Task-space cost components on the host (no GPU): the numpy restatement of tests/task_cost_restatement.py pinned to the
independent C restatement of oracle/rtoc_oracle_rbd.c (frame positions, CoM from the potential energy and the momentum,
Jacobians against central differences on the manifold), robotoc_amd.costs against the reference's loops on the trot
example's parameters (phase boundaries included), and the ctypes mirror of rtoc_task_cost against the C header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from robotoc_amd import costs, robot_model as rm

import task_cost_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [("anymal", 0), ("icub", 1), ("icub", 2)]


@pytest.mark.parametrize("name,seed", MODELS)
def test_frame_positions_and_com_match_the_c_restatement(oracle, name, seed):
    m = rm.load_named(name)
    rng = np.random.default_rng(seed)
    M = sum(m.mass[i] for i in range(m.njoints))
    for _ in range(3):
        q, _, _ = rm.random_configuration(m, rng)
        for c in range(m.ncontacts):
            x = tr.frame_position(m, q, m.contact_parent[c], m.contact_p[c][:])
            assert np.abs(x - oracle.rbd_contact_position(m, q, c)).max() < 1e-12
        _, U = oracle.rbd_energy(m, q, np.zeros(m.nv))
        assert abs(tr.com(m, q)[2] - U / (M * -m.gravity[2])) < 1e-12


@pytest.mark.parametrize("name,seed", MODELS)
def test_jacobians_match_central_differences_and_momentum(oracle, name, seed):
    m = rm.load_named(name)
    rng = np.random.default_rng(10 + seed)
    M = sum(m.mass[i] for i in range(m.njoints))
    q, _, _ = rm.random_configuration(m, rng)
    # a contact frame and a point of the last joint that is not a contact
    frames = [(m.contact_parent[0], np.array(m.contact_p[0][:])), (m.njoints - 1, np.array([0.03, -0.02, 0.1]))]
    eps = 1e-6
    for parent, off in frames:
        J = tr.frame_jacobian(m, q, parent, off)
        Jfd = np.zeros_like(J)
        for j in range(m.nv):
            e = np.zeros(m.nv)
            e[j] = eps
            Jfd[:, j] = (tr.frame_position(m, oracle.rbd_integrate(m, q, e), parent, off)
                         - tr.frame_position(m, oracle.rbd_integrate(m, q, -e), parent, off)) / (2 * eps)
        assert np.abs(J - Jfd).max() < 1e-7
    Jc = tr.com_jacobian(m, q)
    for j in range(m.nv):
        e = np.zeros(m.nv)
        e[j] = 1.0
        assert np.abs(Jc[:, j] - oracle.rbd_momentum_world(m, q, e)[:3] / M).max() < 1e-12
        e[j] = eps
        fd = (tr.com(m, oracle.rbd_integrate(m, q, e)) - tr.com(m, oracle.rbd_integrate(m, q, -e))) / (2 * eps)
        assert np.abs(Jc[:, j] - fd).max() < 1e-7


# examples/anymal/trot.cpp:42-128
STEP, HEIGHT, SWING, DS = np.array([0.15, 0.0, 0.0]), 0.1, 0.5, 0.04
T0 = DS


def _trot_refs():
    x0 = np.array([0.4, 0.2, 0.0])
    feet = [costs.PeriodicSwingFootRef(x0, STEP, HEIGHT, t0, SWING, SWING + 2 * DS, half)
            for t0, half in ((T0 + SWING + DS, False), (T0, True), (T0, True), (T0 + SWING + DS, False))]
    c = costs.PeriodicCoMRef([0.0, 0.0, 0.45], 0.5 * STEP / SWING, T0, SWING, DS, True)
    return feet, c


def test_periodic_references_reproduce_the_reference_loops():
    feet, cref = _trot_refs()
    # a fine sweep, the dt = 0.02 grid times as products and as sums, and every phase boundary exactly
    ts = list(np.linspace(-0.1, 4.0, 997)) + [0.02 * i for i in range(200)]
    acc = 0.0
    for _ in range(200):
        ts.append(acc)
        acc += 0.02
    for f in feet:
        ts += [f.t0 + i * f.period + d for i in range(5) for d in (0.0, f.period_swing)]
    ts += [cref.t0 + i * cref.period + d for i in range(5) for d in (0.0, cref.period_active)]
    n_on = n_off = 0
    for t in ts:
        for f in feet:
            a = tr.foot_is_active(t, f.t0, f.period_swing, f.period_stance)
            assert f.is_active(t) == a
            n_on, n_off = n_on + a, n_off + (not a)
            if a:
                assert np.array_equal(f.update_ref(t), tr.foot_ref(t, f.x3d0, f.step_length, f.step_height, f.t0, f.period_swing,
                                                                    f.period_stance, f.is_first_step_half))
        a = tr.com_is_active(t, cref.t0, cref.period_active, cref.period_inactive)
        assert cref.is_active(t) == a
        if a:
            assert np.array_equal(cref.update_ref(t), tr.com_ref(t, cref.com_ref0, cref.vcom_ref, cref.t0, cref.period_active,
                                                                 cref.period_inactive, cref.is_first_move_half))
    assert n_on > 100 and n_off > 100
    # on a boundary: active from t0 on, inactive from t0 + period_swing on; the peak at mid-swing
    f = feet[1]
    assert not f.is_active(f.t0 - 1e-12) and f.is_active(f.t0) and not f.is_active(f.t0 + f.period_swing)
    assert abs(f.update_ref(f.t0 + 0.5 * f.period_swing)[2] - HEIGHT) < 1e-15


def test_cost_classes_check_arguments_and_fill_the_struct():
    feet, cref = _trot_refs()
    c = costs.TaskSpace3DCost("anymal", "LH_FOOT", feet[1])
    c.set_weight([1e6, 1e6, 1e6])
    s = c.to_struct()
    assert (s.kind, s.ref_kind, s.frame_parent, s.first_half) == (costs.TASK_FRAME_3D, costs.REF_PERIODIC_FOOT, 6, 1)
    assert s.period_active == SWING and s.period_inactive == SWING + 2 * DS and list(s.rate) == list(STEP)
    with pytest.raises(ValueError):
        c.set_weight([1.0, -1.0, 0.0])
    with pytest.raises(ValueError):
        c.set_weight_terminal([-1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        c.set_weight_impact([0.0, 0.0, -1e-9])
    with pytest.raises(ValueError):
        costs.TaskSpace3DCost("anymal", "NO_SUCH_FOOT")
    h = costs.TaskSpace3DCost("icub", ("l_wrist_yaw", [0.0, 0.0, 0.1]), np.array([0.1, 0.2, 0.3]))
    assert h.frame_parent == rm.joint_names("icub").index("l_wrist_yaw")
    assert h.to_struct().ref_kind == costs.REF_CONST and list(h.to_struct().x0) == [0.1, 0.2, 0.3]
    cc = costs.CoMCost("anymal", cref).to_struct()
    assert (cc.kind, cc.ref_kind, cc.first_half) == (costs.TASK_COM, costs.REF_PERIODIC_COM, 1)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_mirror_and_its_solver_test_compile_as_cpp11():
    for src in ("robotoc_amd/host/robotoc_hip_task_costs.hpp", "tests/cpp/ocp_solver_trot_task_cost_test.cpp"):
        lang = ["-x", "c++"] if src.endswith(".hpp") else []
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only"] + lang + [os.path.join(ROOT, src)], check=True)


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="needs gcc / g++")
def test_ctypes_struct_matches_the_c_header(tmp_path):
    fields = [f[0] for f in costs.TaskCost._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtoc_robot.h"\nint main(void) {\n'
                   '  printf("%d %d\\n", (int)sizeof(rtoc_task_cost), RTOC_MAX_TASK_COSTS);\n'
                   + "".join('  printf("%%d\\n", (int)offsetof(rtoc_task_cost, %s));\n' % f for f in fields)
                   + '  printf("%d %d %d %d %d\\n", RTOC_TASK_FRAME_3D, RTOC_TASK_COM, RTOC_REF_CONST, RTOC_REF_PERIODIC_FOOT, RTOC_REF_PERIODIC_COM);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    size, nmax = map(int, out[0].split())
    assert size == C.sizeof(costs.TaskCost) and nmax == costs.MAX_TASK_COSTS
    assert [int(out[1 + k]) for k in range(len(fields))] == [getattr(costs.TaskCost, f).offset for f in fields]
    assert list(map(int, out[1 + len(fields)].split())) == [costs.TASK_FRAME_3D, costs.TASK_COM, costs.REF_CONST,
                                                           costs.REF_PERIODIC_FOOT, costs.REF_PERIODIC_COM]
