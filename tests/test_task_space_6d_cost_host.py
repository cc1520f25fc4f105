"""The numpy restatement of TaskSpace6DCost (tests/task_cost_6d_restatement.py) pinned on the CPU -- Pinocchio is absent, so
nothing compiled from the reference can pin 6D kinematics: log6 against the oracle's, JJ = Jlog6 J_frame and lq against central
differences over the configuration manifold, the linear rows against the 3D Jacobian that is already pinned -- and the host
classes of robotoc_amd.costs: the reference's argument checks and weight order, user reference objects as tables."""
import numpy as np
import pytest

from robotoc_amd import costs, robot_model as rm

import task_cost_6d_restatement as t6
import task_cost_restatement as tr

MODELS = [("iiwa14", 0), ("iiwa14", 1), ("anymal", 2), ("anymal", 3)]
EPS = 1e-6


def _frames(m, rng):
    """(parent, frame_p, frame_R) with non-trivial rotations: the last joint, a joint mid-tree, the root"""
    return [(p, rng.uniform(-0.1, 0.1, 3), t6.random_rotation(rng, 0.3, 2.0)) for p in (m.njoints - 1, m.njoints // 2, 0)]


def _cases(name, seed, n=2):
    m = rm.load_named(name)
    rng = np.random.default_rng(100 + seed)
    for _ in range(n):
        q = rm.random_configuration(m, rng)[0]
        for parent, fp, fR in _frames(m, rng):
            R_ref, p_ref = t6.reference_with_error(m, q, parent, fp, fR, rng)   # rotation-error angle in [0.1, 2.5] rad
            yield m, rng, q, parent, fp, fR, R_ref, p_ref


@pytest.mark.parametrize("name,seed", MODELS)
def test_log6_matches_the_oracle(oracle, name, seed):
    worst = 0.0
    for m, rng, q, parent, fp, fR, R_ref, p_ref in _cases(name, seed):
        XR, Xp = t6.diff(m, q, parent, fp, fR, R_ref, p_ref)
        angle = np.linalg.norm(t6.log3(XR))
        assert 0.1 - 1e-9 <= angle <= 2.5 + 1e-9
        worst = max(worst, np.abs(t6.log6(XR, Xp) - oracle.rbd_log6(XR, Xp)).max())
    print("log6 against the oracle: worst absolute difference %.1e" % worst)
    assert worst < 1e-13


def _perturbed(oracle, m, q, j, eps):
    e = np.zeros(m.nv)
    e[j] = eps
    return oracle.rbd_integrate(m, q, e)


@pytest.mark.parametrize("name,seed", MODELS)
def test_jj_matches_central_differences(oracle, name, seed):
    """JJ against central differences of log6(X_ref^-1 oMf(q (+) eps e_j)), eps = 1e-6: the differences' own error is about
    eps^2 + u / eps = 1e-10, the bound 1e-6 max(1, |JJ|) leaves four decades"""
    worst = 0.0
    for m, rng, q, parent, fp, fR, R_ref, p_ref in _cases(name, seed):
        d, JJ = t6.term6(m, q, parent, fp, fR, R_ref, p_ref)
        fd = np.zeros_like(JJ)
        for j in range(m.nv):
            fd[:, j] = (t6.log6(*t6.diff(m, _perturbed(oracle, m, q, j, EPS), parent, fp, fR, R_ref, p_ref))
                        - t6.log6(*t6.diff(m, _perturbed(oracle, m, q, j, -EPS), parent, fp, fR, R_ref, p_ref))) / (2 * EPS)
        err = np.abs(JJ - fd).max()
        worst = max(worst, err / max(1.0, np.abs(JJ).max()))
        assert err < 1e-6 * max(1.0, np.abs(JJ).max()), (parent, err)
    print("JJ against central differences: worst %.1e of the bound's scale" % worst)


@pytest.mark.parametrize("name,seed", MODELS)
def test_lq_matches_central_differences_of_the_value(oracle, name, seed):
    worst = 0.0
    for m, rng, q, parent, fp, fR, R_ref, p_ref in _cases(name, seed):
        W = rng.uniform(0.5, 10.0, 6)
        value = lambda qq: 0.5 * float(np.sum(W * t6.log6(*t6.diff(m, qq, parent, fp, fR, R_ref, p_ref)) ** 2))
        d, JJ = t6.term6(m, q, parent, fp, fR, R_ref, p_ref)
        lq = JJ.T @ (W * d)
        fd = np.array([(value(_perturbed(oracle, m, q, j, EPS)) - value(_perturbed(oracle, m, q, j, -EPS))) / (2 * EPS) for j in range(m.nv)])
        err = np.abs(lq - fd).max()
        worst = max(worst, err / max(1.0, np.abs(lq).max()))
        assert err < 1e-6 * max(1.0, np.abs(lq).max()), (parent, err)
    print("lq against central differences: worst %.1e of the bound's scale" % worst)


@pytest.mark.parametrize("name,seed", MODELS)
def test_zero_error_gives_the_local_frame_jacobian(name, seed):
    """X_ref = oMf: d = 0, Jlog6 = identity, and the linear rows turned into world axes are the 3D term's Jacobian"""
    for m, rng, q, parent, fp, fR, _, _ in _cases(name, seed):
        Rf, x = t6.frame_placement(m, q, parent, fp, fR)
        d, JJ = t6.term6(m, q, parent, fp, fR, Rf, x)
        assert np.abs(d).max() < 1e-12
        assert np.abs(Rf @ JJ[:3] - tr.frame_jacobian(m, q, parent, fp)).max() < 1e-12


# ---- host classes ----
class _Circle(costs.TaskSpace6DRefBase):
    """examples/iiwa14/task_space_ocp.cpp's reference: a circle in t, active from t0 on"""

    def __init__(self, t0=0.1):
        self.t0, self.R = t0, tr._rot([0.0, 1.0, 0.0], 0.4)

    def update_ref(self, g):
        return self.R, np.array([0.0, 0.1 * np.sin(np.pi * g.t), 0.8 + 0.1 * np.cos(np.pi * g.t)])

    def is_active(self, g):
        return g.t >= self.t0


def test_set_weight_checks_raise_the_reference_messages():
    c = costs.TaskSpace6DCost("iiwa14", "iiwa_link_ee_kuka")
    for setter, suffix in ((c.set_weight, ""), (c.set_weight_terminal, "_terminal"), (c.set_weight_impact, "_impact")):
        with pytest.raises(ValueError) as e:
            setter([1.0, -1.0, 1.0], [1.0, 1.0, 1.0])
        assert str(e.value) == "[TaskSpace6DCost] invalid argument: elements of 'weight_position%s' must be non-negative!" % suffix
        with pytest.raises(ValueError) as e:
            setter([1.0, 1.0, 1.0], [1.0, 1.0, -1e-9])
        assert str(e.value) == "[TaskSpace6DCost] invalid argument: elements of 'weight_rotation%s' must be non-negative!" % suffix
    with pytest.raises(ValueError):
        costs.TaskSpace6DCost("iiwa14", "no_such_frame")
    with pytest.raises(ValueError):
        costs.TaskSpace6DCost("iiwa14", ("no_such_joint", [0, 0, 0]))


def test_to_struct_puts_weight_rotation_first():
    """the reference as written (task_space_6d_cost.cpp:124-125): weight_.head<3>() = weight_rotation multiplies the LINEAR
    components of Log6Map"""
    R_ref = tr._rot([1.0, 0.0, 0.0], 0.3)
    c = costs.TaskSpace6DCost("iiwa14", "iiwa_link_ee_kuka", ([0.1, 0.2, 0.3], R_ref))
    c.set_weight([1.0, 2.0, 3.0], [4.0, 5.0, 6.0])
    c.set_weight_terminal([7.0, 8.0, 9.0], [10.0, 11.0, 12.0])
    c.set_weight_impact([13.0, 14.0, 15.0], [16.0, 17.0, 18.0])
    s = c.to_struct()
    assert (s.kind, s.ref_kind, s.frame_parent) == (costs.TASK_FRAME_6D, costs.REF_CONST, 6)
    assert list(s.weight) == [4.0, 5.0, 6.0] and list(s.weight_angular) == [1.0, 2.0, 3.0]
    assert list(s.weight_terminal) == [10.0, 11.0, 12.0] and list(s.weight_angular_terminal) == [7.0, 8.0, 9.0]
    assert list(s.weight_impact) == [16.0, 17.0, 18.0] and list(s.weight_angular_impact) == [13.0, 14.0, 15.0]
    assert list(s.x0) == [0.1, 0.2, 0.3] and np.array_equal(np.array(s.ref_R[:]).reshape(3, 3), R_ref)
    assert list(t6.weights(s, "stage")) == [4.0, 5.0, 6.0, 1.0, 2.0, 3.0]
    # the end-effector frame of the URDF: Rz(y) Ry(p) Rx(r) of the printed numbers -- near, not exactly, the identity
    fR = np.array(s.frame_R[:]).reshape(3, 3)
    assert list(s.frame_p) == [0.0, 0.0, 0.045]
    assert np.abs(fR - np.eye(3)).max() < 1e-11 and not np.array_equal(fR, np.eye(3))
    assert np.abs(fR @ fR.T - np.eye(3)).max() < 1e-15
    # a frame with an explicit rotation, by joint index
    c2 = costs.TaskSpace6DCost("iiwa14", (3, [0.0, 0.1, 0.0], R_ref))
    s2 = c2.to_struct()
    assert s2.frame_parent == 3 and np.array_equal(np.array(s2.frame_R[:]).reshape(3, 3), R_ref)
    assert list(s2.ref_R) == list(np.eye(3).ravel())   # default constant reference: the identity placement


def test_a_user_reference_fills_a_table_with_inactive_entries():
    ref = _Circle(t0=0.1)
    c = costs.TaskSpace6DCost("iiwa14", "iiwa_link_ee_kuka", ref)
    assert c.to_struct().ref_kind == costs.REF_TABLE and c.uses_table()
    times = 0.05 * np.arange(6)
    infos = costs.grid_infos(times, np.full(6, 0.05))
    assert [g.stage for g in infos] == list(range(6)) and infos[3].t == times[3] and infos[3].dt == 0.05
    tab = c.ref_table(infos)
    assert len(tab) == 6 and [e.active for e in tab] == [0, 0, 1, 1, 1, 1]
    for e, g in zip(tab, infos):
        if e.active:
            R, p = ref.update_ref(g)
            assert np.array_equal(np.array(e.R[:]).reshape(3, 3), R) and np.array_equal(np.array(e.p[:]), p)
        else:   # update_ref is not called where the reference is inactive: a valid placement all the same
            assert list(e.R) == list(np.eye(3).ravel()) and list(e.p) == [0.0, 0.0, 0.0]
    c.set_const_ref([0.0, 0.0, 1.0], np.eye(3))
    assert c.ref_table(infos) is None and c.to_struct().ref_kind == costs.REF_CONST

    class Point:   # a user's TaskSpace3DRefBase
        def update_ref(self, g):
            return [g.t, 0.0, 1.0]

        def is_active(self, g):
            return g.stage != 1

    c3 = costs.TaskSpace3DCost("iiwa14", (6, [0.0, 0.0, 0.045]), Point())
    assert c3.to_struct().ref_kind == costs.REF_TABLE
    tab3 = c3.ref_table(infos)
    assert [e.active for e in tab3] == [1, 0, 1, 1, 1, 1] and list(tab3[2].p) == [0.1, 0.0, 1.0]
    # the periodic references stay formulas evaluated on the device
    foot = costs.TaskSpace3DCost("anymal", "LF_FOOT", costs.PeriodicSwingFootRef([0, 0, 0], [0.1, 0, 0], 0.1, 0.0, 0.2, 0.2, False))
    assert foot.to_struct().ref_kind == costs.REF_PERIODIC_FOOT and foot.ref_table(infos) is None
