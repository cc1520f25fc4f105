"""A time-varying q_ref in the closed solver loops.  (i) iiwa14 through rtoc_unconstr_update_solution with the reference
q0 + t v -- the reference's test helper ConfigurationSpaceRef (test/test_helper/cost_factory.hpp), restated here as a subclass
of costs.ConfigurationSpaceRefBase -- to the tolerance and within the iteration cap of tests/test_unconstr_closed_loop.py.
(ii) The ANYmal jump with switching-time optimisation through solver.OCPSolver(configuration_ref=...): the table is rebuilt at
the mesh refinement, after rtoc_set_grid has forgotten its rows."""
import numpy as np
import pytest

from robotoc_amd import costs
from robotoc_amd.types import BUF_SOL, Records

from test_unconstr_closed_loop import _setup


class ConfigurationSpaceRef(costs.ConfigurationSpaceRefBase):
    """integrateConfiguration(q0_ref, v_ref, t): q0 + t v on a fixed base; always active"""

    def __init__(self, q0_ref, v_ref):
        self.q0_ref, self.v_ref = np.asarray(q0_ref, dtype=float), np.asarray(v_ref, dtype=float)
        self.asked = []

    def update_ref(self, model, grid_info):
        self.asked.append(grid_info.t)
        return self.q0_ref + grid_info.t * self.v_ref

    def is_active(self, grid_info):
        return True


def _converge(ctx, dt):
    """the loop of tests/test_unconstr_closed_loop.py: at most 20 iterations to 1e-8 (it stops early below 1e-10)"""
    hist = []
    for it in range(20):
        hist.append(ctx.unconstr_update_solution(dt))
        if hist[-1].max() < 1e-10:
            break
    return np.array(hist)


@pytest.mark.gpu
def test_iiwa14_tracks_a_moving_reference_to_a_stationary_point():
    batch = 2
    ctx, m, grids, dt, cost, x0, rng = _setup(batch, seed=3)
    n, nv = len(grids), m.nv
    assert n == 21
    S = Records(ctx.L, "sol")
    guess = S.zeros(batch, n)
    S.f(guess, "q")[..., :nv] = x0[:, None, :nv]
    # the constant reference q0 first
    ctx.upload(BUF_SOL, guess)
    hist_const = _converge(ctx, dt)
    q_const = S.f(ctx.download_records(BUF_SOL, "sol"), "q")[..., :nv].copy()
    # ... then q0 + t v
    ref = ConfigurationSpaceRef(cost["q_ref"], np.linspace(-0.6, 0.6, nv))
    infos = costs.grid_infos(dt * np.arange(n), [g.dt for g in grids])
    q_ref, active = costs.configuration_ref_table(ref, m, infos, cost["q_weight"], cost["q_weight_terminal"])
    assert q_ref.shape == (n, nv) and active.all() and len(ref.asked) == n
    ctx.set_configuration_ref_table(q_ref, active)
    ctx.upload(BUF_SOL, guess)
    hist = _converge(ctx, dt)
    print("iterations: %d with the moving reference (KKT %s), %d with the constant one" % (len(hist), ["%.1e" % e for e in hist.max(axis=1)], len(hist_const)))
    assert hist[-1].max() < 1e-8 and len(hist) <= 20 and hist_const[-1].max() < 1e-8
    assert (ctx.status() == 0).all()
    q_moving = S.f(ctx.download_records(BUF_SOL, "sol"), "q")[..., :nv].copy()
    assert np.abs(q_moving - q_const).max() > 1e-2            # the table was used
    # towards the end of the horizon the trajectory follows the moving reference, not the constant one
    moved = ref.v_ref != 0.0   # (the middle joint's reference stands still)
    assert moved.sum() == nv - 1
    assert (np.abs(q_moving[:, -1] - q_ref[-1]) < np.abs(q_moving[:, -1] - cost["q_ref"]))[:, moved].all()
    # stationary: one further iteration is still below the tolerance
    again = ctx.unconstr_update_solution(dt)
    print("KKT error of one further iteration:", again)
    assert again.max() < 1e-8
    ctx.close()


class BaseRamp(costs.ConfigurationSpaceRefBase):
    """the standing posture with the base moving forward over the horizon; no q cost at the very first grid point"""

    def __init__(self, q_stand, length, T):
        self.q, self.length, self.T = np.asarray(q_stand, dtype=float), float(length), float(T)
        self.calls_at_t0 = 0

    def update_ref(self, model, grid_info):
        q = self.q.copy()
        q[0] += self.length * min(1.0, max(0.0, grid_info.t / self.T))
        return q

    def is_active(self, grid_info):
        if grid_info.stage == 0:
            self.calls_at_t0 += 1   # once per (re-)discretisation
            return False
        return True


@pytest.mark.gpu
def test_anymal_jump_with_a_moving_posture_reference_survives_the_mesh_refinement():
    from robotoc_amd import problems_jump as pj
    from robotoc_amd.problems_jump import ANYMAL_Q_STANDING
    ref = BaseRamp(ANYMAL_Q_STANDING, 0.25, 0.8)
    solver, x0, info = pj.anymal_jump_sto_solver(batch=1, configuration_ref=ref)
    try:
        st = solver.solve(0.0, x0)   # a table whose rows rtoc_set_grid forgot would end this with RTOC_ERR_NOT_READY
        hist = np.array([e.max() for e in st.kkt_error])
        print("jump with a moving q_ref: %d iterations (max_iter %d), mesh refinement at %s, KKT %s ... %s, reference asked at %d discretisations"
              % (st.iter, solver.options.max_iter, st.mesh_refinement_iter, ["%.1e" % e for e in hist[:3]], ["%.1e" % e for e in hist[-3:]],
                 ref.calls_at_t0))
        assert st.convergence and st.iter <= solver.options.max_iter and hist[-1] < solver.options.kkt_tol
        assert (solver.ctx.status() == 0).all()
        assert len(st.mesh_refinement_iter) >= 1
        # asked again at every (re-)discretisation: the factory's, solve()'s and one per mesh refinement
        assert ref.calls_at_t0 >= 2 + len(st.mesh_refinement_iter)
        r = st.mesh_refinement_iter[0]   # iter + 1 of the refinement: hist[r] is the first error on the refined mesh
        assert r < len(hist) and hist[-1] < hist[r]
        # the base follows the ramp: half way along the horizon it is between the two ends
        S = Records(solver.ctx.L, "sol")
        q = S.f(solver.get_solution()[0], "q")
        assert q[len(solver.grids) - 1, 0] > x0[0, 0] + 0.1
    finally:
        solver.close()


@pytest.mark.gpu
def test_cpp_unconstr_solver_takes_a_configuration_ref(tmp_path):
    """robotoc::UnconstrOCPSolver::setConfigurationRef / UnconstrOCP::setConfigurationRef (tests/cpp/unconstr_configuration_ref_test.cpp)"""
    import subprocess
    from robotoc_amd import problems as pr, robot_model as rm
    from robotoc_amd.robot_model import MAX_JOINTS
    from test_cpp_host import _build
    exe = _build("unconstr_configuration_ref_test")
    dims, grids, meta = pr.config_iiwa14()
    m = rm.load_named("iiwa14")
    n, nv, dt = len(grids), m.nv, meta["dt"]
    rng = np.random.default_rng(21)
    cost = np.zeros((12, MAX_JOINTS))
    cost[0, :nv] = rng.uniform(-0.8, 0.8, nv)
    for k, w in ((3, 10.0), (4, 0.1), (5, 0.01), (6, 0.001), (7, 10.0), (8, 0.1)):
        cost[k, :nv] = w
    prob = str(tmp_path / "iiwa14_problem.bin")
    with open(prob, "wb") as f:
        f.write(bytes(m))
        f.write(cost.tobytes())
        f.write(np.array([dt * (n - 1)]).tobytes())
        f.write(np.array([n - 1], dtype=np.int32).tobytes())
        f.write(rng.uniform(-0.5, 0.5, nv).tobytes())
        f.write(np.zeros(nv).tobytes())
    run = subprocess.run([exe, prob], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.returncode, run.stdout, run.stderr)
