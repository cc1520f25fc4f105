"""The ANYmal jump with switching-time optimisation of the reference's examples/anymal/python/jump_sto.py (BASELINE configs[2]),
scaled to the N = 40 horizon BASELINE.json names: stand -> flight -> stand, lift-off and touch-down times optimised
(ContactSequence::push_back(..., sto=True), :96-103), ConfigurationSpaceCost with the example's weights (:25-57), its Constraints
object (six joint-limit components + FrictionCone, :60-74), STOConstraints with minimum dwell times (:107-109), the example's
solver options (kkt_tol_mesh = 1, max_dt_mesh = T / N, :117-122).  Everything the example sets up with Pinocchio on the host
(foot positions at the standing pose, total weight) comes from robotoc_amd.robot_model."""
import numpy as np

from . import robot_model as rm
from .grid import ANYMAL_Q_STANDING, Event
from .solver import ContactPlan, OCPSolver, SolverOptions, STOConstraints
from .types import Records


def anymal_jump_sto_solver(batch=1, device=0, N=40, dt=0.02, jump_length=0.25, ground_time=0.31, flying_time=0.2,
                           min_dwell=(0.1, 0.1, 0.2), with_limits=True, with_cones=True, max_iter=200, seed=7, x0_noise=0.0,
                           horizon_scan="off", configuration_ref=None):
    m = rm.load_named("anymal")
    nv, nq, nu = m.nv, m.nq, m.nu
    qs = np.array(ANYMAL_Q_STANDING, dtype=float)
    T = N * dt
    feet = np.array([m.frame_placement(qs, c)[1] for c in range(4)])
    landed = feet + np.array([jump_length, 0.0, 0.0])
    plan = ContactPlan([0b1111, 0, 0b1111], [feet, feet, landed],
                       [Event("lift", ground_time, sto=True), Event("impact", ground_time + flying_time, sto=True)])
    q_ref = qs.copy()
    q_ref[0] += jump_length
    wq = np.concatenate([[1.0, 0.0, 0.0, 1.0, 1.0, 1.0], np.full(12, 0.001)])
    wq_imp = np.concatenate([[0.0, 0.0, 0.0, 100.0, 100.0, 100.0], np.full(12, 0.1)])
    cost = dict(q_ref=q_ref, v_ref=np.zeros(nv), u_ref=np.zeros(nu), q_weight=wq, v_weight=np.full(nv, 1.0), a_weight=np.full(nv, 1e-6),
                u_weight=np.zeros(nu), q_weight_terminal=wq, v_weight_terminal=np.full(nv, 1.0), q_weight_impact=wq_imp,
                v_weight_impact=np.full(nv, 1.0), dv_weight_impact=np.full(nv, 1e-6))
    # joint limits of the ANYmal URDF (anymal_b_simple_description): position +-9.42 (continuous joints), velocity 7.5 rad/s, effort 80 N m
    limits = (np.full(nu, -9.42), np.full(nu, 9.42), np.full(nu, 7.5), np.full(nu, 80.0)) if with_limits else None
    opts = SolverOptions(max_iter=max_iter, kkt_tol=1e-7, kkt_tol_mesh=1.0, max_dt_mesh=T / N, horizon_scan=horizon_scan)
    solver = OCPSolver(m, plan, T, N, cost, joint_limits=limits, friction_coefficients=np.full(4, 0.7) if with_cones else None,
                       sto_constraints=STOConstraints(list(min_dwell)), options=opts, batch=batch, device=device,
                       configuration_ref=configuration_ref)
    rng = np.random.default_rng(seed)
    x0 = np.tile(np.concatenate([qs, np.zeros(nv)]), (batch, 1))
    if x0_noise > 0.0:
        x0[:, 7:nq] += x0_noise * rng.uniform(-1, 1, (batch, nq - 7))
        x0[:, nq:] = x0_noise * rng.uniform(-1, 1, (batch, nv))
    solver.discretize(0.0)
    # initial guess like the example: q, v = the initial state on every grid point, f = a quarter of the weight per foot (:133-137)
    S = Records(solver.ctx.L, "sol")
    sol = S.zeros(batch, len(solver.grids))
    S.f(sol, "q")[..., :nq] = x0[:, None, :nq]
    S.f(sol, "v")[...] = x0[:, None, nq:]
    weight = 9.81 * sum(m.mass[i] for i in range(m.njoints))
    for i, g in enumerate(solver.grids):
        act = [k for k in range(4) if (int(solver.masks[i]) >> k) & 1]
        if act and g.type != 1 and i < len(solver.grids) - 1:
            S.f(sol, "f")[:, i, :3 * len(act)] = np.tile([0.0, 0.0, 0.25 * weight], len(act))
    solver.set_solution(sol)
    return solver, x0, dict(T=T, N=N, model=m, cost=cost, min_dwell=list(min_dwell),
                            limits=[9.42, 7.5, 80.0, 0.7])


# joint limits of the example's iCub URDF (examples/icub/icub_description/urdf/icub.urdf: <limit lower upper velocity effort>), in the
# order of the actuated joints of robotoc_amd/models/icub.json (legs, torso, arms)
ICUB_Q_MIN = [-0.767945, -2.07694, -1.37881, -2.18166, -0.733038, -0.418879, -0.767945, -2.07694, -1.37881, -2.18166, -0.733038, -0.418879,
              -0.383972, -0.680678, -1.02974, -1.65806, 0.0, -0.645772, 0.0959931, -0.872665, -1.13446, -0.436332, -1.65806, 0.0, -0.645772,
              0.0959931, -0.872665, -1.13446, -0.436332]
ICUB_Q_MAX = [2.30383, 0.296706, 1.37881, 0.401426, 0.366519, 0.418879, 2.30383, 0.296706, 1.37881, 0.401426, 0.366519, 0.418879, 1.46608,
              0.680678, 1.02974, 0.0872665, 2.80649, 1.74533, 1.85005, 0.872665, 0.174533, 0.436332, 0.0872665, 2.80649, 1.74533, 1.85005,
              0.872665, 0.174533, 0.436332]
ICUB_V_MAX = [100.0] * 29
ICUB_U_MAX = [84.0, 84.0, 40.0, 30.0, 24.0, 11.0, 84.0, 84.0, 40.0, 30.0, 24.0, 11.0, 36.0, 80.0, 80.0, 84.0, 84.0, 34.0, 20.0, 0.45, 0.65, 0.65,
              84.0, 84.0, 34.0, 20.0, 0.45, 0.65, 0.65]


def icub_jump_sto_solver(batch=1, device=0, dt=0.02, jump_length=0.5, ground_time=0.7, flying_time=0.25,
                         min_dwell=(0.6, 0.2, 0.6, 0.2, 0.6), max_iter=350, initial_sto_reg_iter=10, with_limits=True, with_cones=True,
                         jumps=2, horizon_scan="off", x0_noise=0.0, seed=11):
    """BASELINE configs[3] as the reference poses it (examples/icub/python/jump_sto.py): iCub (nv = 35, the example's URDF) on its two
    soles -- SURFACE contacts --, two jumps of 0.5 m (four discrete events, all with switching-time optimisation), ConfigurationSpaceCost
    with the example's weights (:30-50), its Constraints object (six joint-limit components + FrictionCone on the soles, mu = 0.6,
    :53-70), STOConstraints with the example's minimum dwell times (:104-106), T = 2.6 s, N = 130, kkt_tol_mesh = 0.1,
    max_dt_mesh = T / N, initial_sto_reg_iter = 10, max_iter = 350 (:108-121).  jumps = 1: the first jump only (two events, T = 1.65 s)."""
    from .grid import ICUB_Q_STANDING
    m = rm.load_named("icub")
    nv, nq, nu = m.nv, m.nq, m.nu
    qs = np.array(ICUB_Q_STANDING, dtype=float)
    place = [m.frame_placement(qs, c) for c in range(2)]
    pos0 = np.array([p for _, p in place])
    rot0 = np.array([R for R, _ in place])
    step = np.array([jump_length, 0.0, 0.0])
    masks, positions, events, t = [0b11], [pos0], [], 0.0
    for j in range(jumps):
        t += ground_time
        events.append(Event("lift", t, sto=True))
        masks.append(0)
        positions.append(pos0 + j * step)
        t += flying_time
        events.append(Event("impact", t, sto=True))
        masks.append(0b11)
        positions.append(pos0 + (j + 1) * step)
    T = t + ground_time
    N = int(np.floor(T / dt + 1e-9))
    plan = ContactPlan(masks, positions, events, phase_rotations=[rot0] * len(masks))
    wq = np.concatenate([[0, 1, 1, 100, 100, 100], np.full(12, 0.001), [0.001, 1, 1], np.full(14, 0.001)])
    cost = dict(q_ref=qs, v_ref=np.zeros(nv), u_ref=np.zeros(nu), q_weight=wq, v_weight=np.full(nv, 1e-3), a_weight=np.full(nv, 1e-5),
                u_weight=np.zeros(nu), q_weight_terminal=wq, v_weight_terminal=np.full(nv, 1e-3), q_weight_impact=wq,
                v_weight_impact=np.full(nv, 1e-3), dv_weight_impact=np.zeros(nv))
    limits = (np.array(ICUB_Q_MIN), np.array(ICUB_Q_MAX), np.array(ICUB_V_MAX), np.array(ICUB_U_MAX)) if with_limits else None
    opts = SolverOptions(max_iter=max_iter, kkt_tol=1e-7, kkt_tol_mesh=0.1, max_dt_mesh=T / N, initial_sto_reg_iter=initial_sto_reg_iter,
                         horizon_scan=horizon_scan)
    solver = OCPSolver(m, plan, T, N, cost, joint_limits=limits, friction_coefficients=np.full(2, 0.6) if with_cones else None,
                       sto_constraints=STOConstraints(list(min_dwell[:len(events) + 1])), options=opts, batch=batch, device=device)
    x0 = np.tile(np.concatenate([qs, np.zeros(nv)]), (batch, 1))
    if x0_noise > 0.0:   # a distinct initial state per instance (batched runs)
        rng = np.random.default_rng(seed)
        x0[:, 7:nq] += x0_noise * rng.uniform(-1, 1, (batch, nq - 7))
        x0[:, nq:] = x0_noise * rng.uniform(-1, 1, (batch, nv))
    solver.discretize(0.0)
    # the example's initial guess: q, v = the initial state on every grid point (:127-130), forces left at zero
    S = Records(solver.ctx.L, "sol")
    sol = S.zeros(batch, len(solver.grids))
    S.f(sol, "q")[..., :nq] = x0[:, None, :nq]
    solver.set_solution(sol)
    return solver, x0, dict(T=T, N=N, model=m, cost=cost, min_dwell=list(min_dwell))


class _ConstantConfigurationRef:
    """a ConfigurationSpaceRefBase that answers with one q_ref everywhere: config_cost_->set_q_ref of one instance"""

    def __init__(self, q_ref):
        self.q_ref = np.array(q_ref, dtype=float)

    def update_ref(self, model, grid_info):
        return self.q_ref

    def is_active(self, grid_info):
        return True


def anymal_jump_mpc_solver(jump_length, step_yaw, batch=1, device=0, T=0.8, N=18, flying_time=0.3, min_flying_time=0.2, ground_time=0.3,
                           min_ground_time=0.2, projection=None, x0=None, max_iter=200, host_plan=None, host_q_ref=None):
    """The batch MPCJump poses (src/mpc/mpc_jump.cpp) on ANYmal, every instance with its own jump: jump_length [3] or [batch, 3],
    step_yaw a scalar or [batch].  ConfigurationSpaceCost with the weights of :39-52, the six joint-limit components (:54-65),
    FrictionCone with mu = 0.5 (:66-68, :86-87), STOConstraints with the minimum dwell times of resetMinimumDwellTimes case 0 at
    t = t_mpc_start (:284-288: T / N, min_flying_time, min_ground_time), lift-off at T - ground_time - flying_time and touch-down at
    T - ground_time, both with switching-time optimisation (:134-138).  What MPCJump::init does next (:140-146) runs on the device:
    a robotoc_amd.planner.JumpFootStepPlanner is initialised at x0, plans once, and -- handed to the solver as contact_planner --
    writes every instance's placements and q_ref onto each grid the solver sets.  Returns (solver, x0, info); info["planner"] is
    the planner.  The receding horizon of MPCJump::updateSolution (:206-222) stays with the caller.

    host_plan / host_q_ref: the same problem fed through the host tables instead -- a per-instance ContactPlan and q_ref
    [batch, nq]; no planner is made (info["planner"] is None)."""
    from . import capi
    from .planner import JumpFootStepPlanner
    m = rm.load_named("anymal")
    nv, nq, nu = m.nv, m.nq, m.nu
    qs = np.array(ANYMAL_Q_STANDING, dtype=float)
    if x0 is None:
        x0 = np.tile(np.concatenate([qs, np.zeros(nv)]), (batch, 1))
    x0 = np.ascontiguousarray(x0, dtype=float)
    if (host_plan is None) != (host_q_ref is None):
        raise ValueError("the host path needs both host_plan and host_q_ref")
    events = [Event("lift", T - ground_time - flying_time, sto=True), Event("impact", T - ground_time, sto=True)]
    on_device = host_plan is None
    if on_device:
        # shared placements the planner overwrites on every grid: where the standing feet are
        feet = np.array([m.frame_placement(qs, c)[1] for c in range(4)])
        plan = ContactPlan([0b1111, 0, 0b1111], [feet, feet, feet], events)
    else:
        plan = ContactPlan(list(host_plan.phase_masks), list(host_plan.phase_positions), events, phase_rotations=host_plan.phase_rotations)
    wq = np.concatenate([[0.0, 100.0, 100.0, 100.0, 100.0, 100.0], np.full(nv - 6, 0.01)])
    wq_imp = np.concatenate([[0.0, 1000.0, 1000.0, 1000.0, 1000.0, 1000.0], np.full(nv - 6, 10.0)])
    cost = dict(q_ref=qs, v_ref=np.zeros(nv), u_ref=np.zeros(nu), q_weight=wq, v_weight=np.full(nv, 1.0), a_weight=np.full(nv, 1e-3),
                u_weight=np.zeros(nu), q_weight_terminal=wq, v_weight_terminal=np.full(nv, 1.0), q_weight_impact=wq_imp,
                v_weight_impact=np.full(nv, 10.0), dv_weight_impact=np.full(nv, 1e-3))
    limits = (np.full(nu, -9.42), np.full(nu, 9.42), np.full(nu, 7.5), np.full(nu, 80.0))
    opts = SolverOptions(max_iter=max_iter)
    refs = None if on_device else [_ConstantConfigurationRef(q) for q in np.asarray(host_q_ref, dtype=float).reshape(batch, nq)]
    solver = OCPSolver(m, plan, T, N, cost, joint_limits=limits, friction_coefficients=np.full(4, 0.5),
                       sto_constraints=STOConstraints([T / N, min_flying_time, min_ground_time]), options=opts, batch=batch, device=device,
                       configuration_ref=refs)
    solver.ctx.set_initial_state(x0)
    solver.discretize(0.0)
    planner = None
    if on_device:
        planner = JumpFootStepPlanner(solver.ctx, capi.PROJECT_AS_REFERENCE if projection is None else projection)
        planner.set_jump_pattern(jump_length, step_yaw)
        planner.init()                    # foot_step_planner_->init(q) and the q_ref of :141-145
        planner.plan(0.0, 0b1111)         # resetContactPlacements (:303): cs_ground_ is the first contact status
        solver.set_contact_planner(planner)   # places and sets q_ref now, and again on every later grid
    # setSolution("q", q), setSolution("v", v) (:147-148)
    S = Records(solver.ctx.L, "sol")
    sol = S.zeros(batch, len(solver.grids))
    S.f(sol, "q")[..., :nq] = x0[:, None, :nq]
    S.f(sol, "v")[...] = x0[:, None, nq:]
    solver.set_solution(sol)
    return solver, x0, dict(T=T, N=N, model=m, cost=cost, planner=planner, min_dwell=[T / N, min_flying_time, min_ground_time])
