"""Host-side mirror of robotoc::OCPSolver (include/robotoc/solver/ocp_solver.hpp:41-241, src/solver/ocp_solver.cpp:96-225) for
OCPs whose whole iteration is resident on the device (ConfigurationSpaceCost, joint limits, friction cones, contact sequence
with lifts / touch-downs, optionally switching-time optimisation): what stays on the host is what the reference keeps outside
updateSolution's kernels -- the contact sequence, the (re-)discretisation, the STO regularisation schedule, the mesh-refinement
branch with its solution interpolation, the convergence test.  One `OCPSolver` drives a BATCH of instances that share the
contact-sequence structure (initial states, and with STO the event times, are per instance); batch = 1 is the reference's solver.

The C++ mirror with the reference's signatures is robotoc_amd/host/robotoc_hip_solver.hpp; this one is what tests / bench use.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import capi
from .costs import configuration_ref_table, grid_infos
from .grid import ContactSequence, Event, contact_masks, discretize, discretize_structure_preserving, max_time_step
from .types import BUF_SOL, GRID_IMPACT, GRID_LIFT, GRID_TERMINAL, Dims, Records, joint_limit_rows


@dataclass
class SolverOptions:
    """include/robotoc/solver/solver_options.hpp:17-130 (the members this path reads)"""
    max_iter: int = 100
    kkt_tol: float = 1.0e-7
    initial_sto_reg_iter: int = 0
    initial_sto_reg: float = 1.0e30
    kkt_tol_mesh: float = 0.1
    max_dt_mesh: float = 0.0
    max_dts_riccati: float = 0.1
    enable_solution_interpolation: bool = True
    enable_line_search: bool = False
    # not in the reference: how the Riccati recursion runs on the device -- "off" (default, as the C API): the serial kernels;
    # "auto": the horizon scans for batches of at most 8 OCPs (RTOC_OPT_BACKWARD_SCAN = 2: latency of one MPC problem); "on": always
    horizon_scan: str = "off"
    # not in the reference: where SolutionInterpolator runs.  False (default): on the host, in the mesh-refinement branch alone
    # (download, OCPSolver._interpolate, upload), and a later solve() starts from the records as they are.  True: on the device
    # (rtoc_solution_store / rtoc_solution_interpolate, no record leaves it), in the mesh-refinement branch and for the
    # receding-horizon warm start of ocp_solver.cpp:159-163, :215-220 -- every solve() stores its solution at the end, and every
    # solve(init_solver=True) interpolates the stored one onto the grid it has just discretised.  Both uses are gated by
    # enable_solution_interpolation, as in the reference.
    solution_interpolation_on_device: bool = False
    # LineSearchSettings (include/robotoc/line_search/line_search_settings.hpp), filter method
    step_size_reduction_rate: float = 0.75
    min_step_size: float = 0.05
    filter_cost_reduction_rate: float = 0.005
    filter_constraint_violation_reduction_rate: float = 0.005
    line_search_method: str = "filter"   # LineSearchMethod::Filter | "merit": MeritBacktracking (line_search.cpp:87-128)
    armijo_control_rate: float = 0.001
    margin_rate: float = 0.05
    eps: float = 1.0e-8


@dataclass
class ContactPlan:
    """The ContactSequence of the OCP (src/planner/contact_sequence.cpp) as the device needs it: per contact phase the
    active-contact mask and the contact positions [ncontacts, 3]; per discrete event its kind, time and STO flag."""
    phase_masks: List[int]
    phase_positions: List[np.ndarray]
    events: List[Event] = field(default_factory=list)
    phase_rotations: Optional[List[np.ndarray]] = None   # surface contacts: per phase [ncontacts, 3, 3] (ContactStatus::setContactPlacements)

    # what the DiscreteTime* references of robotoc_amd.costs ask a contact sequence
    def num_contact_phases(self):
        return len(self.phase_masks)

    def is_contact_active(self, phase, contact):
        return bool((int(self.phase_masks[phase]) >> contact) & 1)

    def contact_position(self, phase, contact):
        return self.phase_positions[phase][contact]

    def impact_masks(self):
        out, p = [], 0
        for e in self.events:
            if e.kind == "impact":
                out.append(self.phase_masks[p + 1] & ~self.phase_masks[p])
            p += 1
        return out


def placement_tables(plan, grids, ncontacts, batch):
    """The contact placements of a plan per GRID POINT, as the device takes them: (positions, rotations or None, per_instance).
    A plan whose phase_positions[p] are [ncontacts, 3] (phase_rotations[p] [ncontacts, 3, 3]) is shared by the batch and gives
    [nstages, ncontacts, 3] ([nstages, ncontacts, 3, 3]); one whose entries are [batch, ncontacts, 3] ([batch, ncontacts, 3, 3])
    puts every instance on its own footholds and gives the same with a leading [batch].  A plan that mixes the two raises
    ValueError.  Phases advance at lift and impact grid points."""
    if ncontacts == 0:   # nothing to place
        return np.zeros((len(grids), 0, 3)), None, False

    def shapes(entries, tail):
        lead = set()
        for e in entries:
            s = np.shape(e)
            if s == (ncontacts,) + tail:
                lead.add(False)
            elif s == (batch, ncontacts) + tail:
                lead.add(True)
            else:
                raise ValueError("a phase's placements must be %s or %s, not %s" % ((ncontacts,) + tail, (batch, ncontacts) + tail, s))
        return lead
    lead = shapes(plan.phase_positions, (3,))
    if plan.phase_rotations is not None:
        lead |= shapes(plan.phase_rotations, (3, 3))
    if len(lead) > 1:
        raise ValueError("a ContactPlan is shared by the batch or per instance: its phases mix [ncontacts, ...] and [batch, ncontacts, ...]")
    per_instance = bool(lead and lead.pop())

    def table(entries, tail):
        out, phase = np.zeros((len(grids), batch if per_instance else 1, ncontacts) + tail), 0
        for i, g in enumerate(grids):
            if g.type in (GRID_IMPACT, GRID_LIFT):
                phase += 1
            out[i] = entries[min(phase, len(entries) - 1)]
        return np.ascontiguousarray(out.swapaxes(0, 1)) if per_instance else out[:, 0]
    pos = table(plan.phase_positions, (3,))
    rot = table(plan.phase_rotations, (3, 3)) if plan.phase_rotations is not None else None
    return pos, rot, per_instance


@dataclass
class STOConstraints:
    """src/sto/sto_constraints.cpp:12-59"""
    minimum_dwell_times: List[float]
    barrier_param: float = 1.0e-3
    fraction_to_boundary_rule: float = 0.995


@dataclass
class SolverStatistics:
    convergence: bool = False
    iter: int = 0
    kkt_error: List[np.ndarray] = field(default_factory=list)        # OCPSolver::KKTError() per iteration, [batch]
    ts: List[np.ndarray] = field(default_factory=list)               # event times per iteration, [batch, nev]
    mesh_refinement_iter: List[int] = field(default_factory=list)


# ---- SE(3) helpers for the solution interpolation (Robot::interpolateConfiguration = pinocchio::interpolate) ----
def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _R_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
    q = np.zeros(4)
    q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def _log3(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    if c < -0.99:
        # near pi the antisymmetric part vanishes (0 / 0 at pi): 4 q_i (q_x, q_y, q_z, q_w) of the quaternion of R, i the largest
        # diagonal entry, and w = 2 atan2(|v|, q_w) v / |v| (the scale drops out)
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        v = np.zeros(3)
        v[i], v[j], v[k] = 1.0 + R[i, i] - R[j, j] - R[k, k], R[i, j] + R[j, i], R[i, k] + R[k, i]
        qw = R[k, j] - R[j, k]
        if qw < 0.0:
            v, qw = -v, -qw
        n = np.linalg.norm(v)
        return (2.0 * np.arctan2(n, qw) / n) * v
    th = np.arccos(c)
    if th < 1e-10:
        return 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return th / (2.0 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def _exp_coefficients(w):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 at t = |w| as the device computes them (rbd::exp_coefficients,
    csrc/rigid_body_math.hpp): (1 - cos t) / t^2 cancels like 1e-16 / t^2, so the series below 1e-3 and 2 sin^2(t/2) / t^2 above"""
    t2 = float(np.dot(w, w))
    t = np.sqrt(t2)
    if t < 1e-3:
        return 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    sh, s = np.sin(0.5 * t), np.sin(t)
    return s / t, 2.0 * sh * sh / t2, (t - s) / (t2 * t)


def _exp3(w):
    K = _skew(w)
    S, C, _ = _exp_coefficients(w)
    return np.eye(3) + S * K + C * K @ K


def _V(w):   # exp6: p = V(w) v
    K = _skew(w)
    _, C, B = _exp_coefficients(w)
    return np.eye(3) + C * K + B * K @ K


def interpolate_configuration(q1, q2, alpha, floating):
    """q1 (+) alpha (q2 (-) q1): joints linearly, a free-flyer base along the screw motion between the two placements"""
    q = (1.0 - alpha) * q1 + alpha * q2
    if floating:
        R1, R2 = _quat_R(q1[3:7]), _quat_R(q2[3:7])
        Rr, pr = R1.T @ R2, R1.T @ (q2[:3] - q1[:3])
        w = _log3(Rr)
        v = np.linalg.solve(_V(w), pr)
        Ra, pa = _exp3(alpha * w), _V(alpha * w) @ (alpha * v)
        q[:3] = q1[:3] + R1 @ pa
        quat = _R_quat(R1 @ Ra)
        q[3:7] = quat / np.linalg.norm(quat)
    return q


class OCPSolver:
    def __init__(self, model, plan: ContactPlan, T, N, cost, joint_limits=None, friction_coefficients=None, barrier_param=1.0e-3,
                 fraction_to_boundary_rule=0.995, sto_constraints: Optional[STOConstraints] = None, options: Optional[SolverOptions] = None,
                 batch=1, device=0, impact_cones=False, task_costs=None, force_cost=None, configuration_ref=None, contact_planner=None):
        """cost: keyword arguments of capi.Context.set_configuration_cost; joint_limits: (q_min, q_max, v_max, u_max) over the
        actuated joints or None; friction_coefficients: per contact or None; task_costs: robotoc_amd.costs.TaskSpace3DCost /
        CoMCost / TaskSpace6DCost components added to the configuration cost (a list shared by the batch) or None; force_cost: a
        robotoc_amd.costs.LocalContactForceCost (shared by the batch) or None; configuration_ref: a
        robotoc_amd.costs.ConfigurationSpaceRefBase -- a time-varying q_ref in place of the cost's constant one
        (ConfigurationSpaceCost::set_ref) -- shared by the batch, a list of `batch` of them (every instance its own), or None.  The
        object is asked once per grid point at every (re-)discretisation, mesh refinements included; with switching-time
        optimisation at the times of the structure the batch shares (those of the mean event times), not at every instance's own
        -- the rule the task costs' user-object references follow.  contact_planner: a robotoc_amd.planner.JumpFootStepPlanner (any
        object with place(phase_of_grid_point) and set_configuration_ref()) or None.  With one, every (re-)discretisation, mesh
        refinements included, ends with the planner writing every instance's placements and q_ref from its plan on the device onto
        the grid just set, in place of the plan's shared placements and the cost's constant q_ref; a planner made without a context
        is given this solver's.  The planner's init needs a grid on the context, so a planner that is not initialised yet is handed
        over after the first discretize instead, through set_contact_planner."""
        self.model, self.plan, self.T, self.N = model, plan, float(T), int(N)
        self.options = options or SolverOptions()
        self.sto = sto_constraints
        self.batch = batch
        nu = model.nu
        self.nc = model.ncontacts
        rows = joint_limit_rows_for(model) if joint_limits is not None else []
        nc_max = (len(rows) + (5 * self.nc if friction_coefficients is not None else 0) + 7) & ~7
        self.cone_dim = model.contact_rows(0) if self.nc else 3   # FrictionCone acts on the force part of a surface contact's wrench
        self.dims = Dims(model.nv, nu, model.nv - nu, model.max_dimf, model.max_dimf, nc_max)
        nlift = sum(1 for e in plan.events if e.kind == "lift")
        nimp = len(plan.events) - nlift
        self.max_stages = self.N + 1 + nlift + 2 * nimp
        self.ctx = capi.Context(self.dims, self.max_stages, batch, device)
        c = self.ctx
        c.set_robot_model(model)
        c.set_configuration_cost(**cost)
        self.cost, self.configuration_ref = cost, configuration_ref
        self.contact_planner = contact_planner
        if contact_planner is not None and getattr(contact_planner, "ctx", None) is None:
            contact_planner.ctx = c
        self._phase = None
        if isinstance(configuration_ref, (list, tuple)) and len(configuration_ref) != batch:
            raise ValueError("a per-instance configuration_ref needs one object per instance")
        self.task_costs = list(task_costs) if task_costs else None
        if self.task_costs:
            c.set_task_costs(self.task_costs)
        self.force_cost = force_cost
        if force_cost is not None:
            c.set_contact_force_cost(force_cost)
        c.set_max_dts0(self.options.max_dts_riccati)
        c.set_backward_scan({"auto": "auto", "on": True, "off": False}[self.options.horizon_scan])
        self.tau = fraction_to_boundary_rule
        if rows:
            q_min, q_max, v_max, u_max = (np.asarray(x, dtype=float) for x in joint_limits)
            c.set_constraint_rows(rows)
            c.set_constraint_bounds(np.concatenate([-q_min, q_max, v_max, v_max, u_max, u_max]), barrier_param, fraction_to_boundary_rule)
        if friction_coefficients is not None:
            c.set_friction_cones(self.nc, self.cone_dim)
            c.set_impact_cones(impact_cones)
            c.set_barrier_param(barrier_param, fraction_to_boundary_rule)
            c.set_friction_coefficients(np.asarray(friction_coefficients, dtype=float))
        self.has_rows = bool(rows) or friction_coefficients is not None
        if self.options.enable_line_search:
            o = self.options
            c.set_line_search(True, o.step_size_reduction_rate, o.min_step_size, o.filter_cost_reduction_rate,
                              o.filter_constraint_violation_reduction_rate)
            c.set_line_search_method(o.line_search_method, o.armijo_control_rate, o.margin_rate, o.eps)
        self.event_times = np.tile(np.array([e.time for e in plan.events], dtype=float), (batch, 1))   # per instance
        self.grids, self.masks, self.t_grid = None, None, None
        self.S = Records(c.L, "sol")
        self.stats = SolverStatistics()
        self._sol_guess = None

    # ---- discretisation (ocp_solver.cpp:96-102) ----
    def _sequence(self, ts):
        return ContactSequence([self.model.active_rows(m) for m in self.plan.phase_masks],
                               [Event(e.kind, float(t), e.sto, self.model.active_rows(self.plan.phase_masks[p + 1] & ~self.plan.phase_masks[p])
                                      if e.kind == "impact" else 0) for p, (e, t) in enumerate(zip(self.plan.events, ts))])

    def discretize(self, t):
        """TimeDiscretization::discretize (+ correctTimeSteps with an STO problem).  The batch shares the structure: it is that
        of the mean event times; every instance gets its own time steps from its own event times (rtoc_sto_set_problem)."""
        self.t0 = float(t)
        cs = self._sequence(self.event_times.mean(axis=0))
        self._phase = None
        if self.task_costs or self.configuration_ref is not None or self.contact_planner is not None:
            grids, times, structure = discretize(self.N, self.T, t, cs, phase_based=self.sto is not None, times=True, infos=True)
            self._phase = [s[1] for s in structure]   # GridInfo::phase of every grid point
        else:
            grids = discretize(self.N, self.T, t, cs, phase_based=self.sto is not None)
        nev = sum(1 for g in grids if g.type in (GRID_IMPACT, GRID_LIFT))
        if len(grids) > self.max_stages or nev != len(self.plan.events):
            raise RuntimeError("the discretisation has %d grid points with %d events, the context was sized for %d with %d (an event left the horizon?)"
                               % (len(grids), nev, self.max_stages, len(self.plan.events)))
        self.grids = grids
        c = self.ctx
        c.set_grid(grids)
        if self.task_costs:
            c.set_grid_times(times)   # the periodic references' GridInfo::t (with STO the device keeps its own per instance)
            # references that are the user's objects: asked once per grid point (rtoc_set_grid has just forgotten the tables); the
            # DiscreteTime* references read the grid point's place in its phase, which the switching times do not move
            c.set_task_ref_tables(self.task_costs, grid_infos(times, [g.dt for g in grids], structure))
        if self.configuration_ref is not None:
            # rtoc_set_grid has just forgotten the rows: until they are set again evalKKT refuses to run
            wqi = self.cost.get("q_weight_impact")   # not given: zero (capi.Context.set_configuration_cost)
            c.set_configuration_ref_table(*configuration_ref_table(
                self.configuration_ref, self.model, grid_infos(times, [g.dt for g in grids], structure), self.cost.get("q_weight"),
                self.cost.get("q_weight_terminal"), np.zeros(self.model.nv) if wqi is None else wqi))
        self.masks = contact_masks(grids, self.plan.phase_masks, self.plan.impact_masks())
        pos, rot, per_instance = placement_tables(self.plan, grids, self.nc, self.batch)
        if per_instance:
            # every instance on its own footholds: the schedule's masks first, then the placements of the batch
            c.set_contact_schedule(self.masks)
            c.set_contact_placements(pos, rot)
        else:
            c.set_contact_schedule(self.masks, pos, rot)
        if self.sto is not None and len(self.plan.events) > 0:
            c.sto_set_problem(self.t0, self.T, self.event_times, self.sto.minimum_dwell_times, self.sto.barrier_param,
                              self.sto.fraction_to_boundary_rule)
        if self.contact_planner is not None:
            # rtoc_set_grid has just forgotten the tables; the plan and the stored q_ref are still on the device
            self._plan_onto_grid()

    def _plan_onto_grid(self):
        if self._phase is None:   # the grid in force was made without a planner: its structure once more
            cs = self._sequence(self.event_times.mean(axis=0))
            structure = discretize(self.N, self.T, self.t0, cs, phase_based=self.sto is not None, times=True, infos=True)[2]
            self._phase = [s[1] for s in structure]
        self.contact_planner.place(self._phase)
        self.contact_planner.set_configuration_ref()

    def set_contact_planner(self, contact_planner):
        """the contact_planner of the constructor, handed over later: an initialised planner on this solver's context (one made
        without a context is given it).  With a grid in force it places and sets q_ref at once; None takes the planner away (the
        tables it wrote stay until the next discretize)."""
        self.contact_planner = contact_planner
        if contact_planner is None:
            return
        if getattr(contact_planner, "ctx", None) is None:
            contact_planner.ctx = self.ctx
        if self.grids is not None:
            self._plan_onto_grid()

    def grid_times(self, b=0):
        """t of every grid point of instance b (TimeDiscretization::grid(i).t)"""
        dt = self.ctx.sto_time_steps()[b] if self.sto is not None and self.plan.events else np.array([g.dt for g in self.grids])
        return self.t0 + np.concatenate([[0.0], np.cumsum(dt[:-1])]), dt

    # ---- solution access ----
    def set_solution(self, sol):
        """sol: [batch, nstages, stride] SplitSolution records (Records(ctx.L, "sol"))"""
        self.ctx.upload(BUF_SOL, np.ascontiguousarray(sol))

    def get_solution(self):
        return self.ctx.download_records(BUF_SOL, "sol")

    # ---- what the MPC hands to the controller (src/mpc/control_policy.cpp:24-60; every gait MPC's getControlPolicy(t)) ----
    def get_control_policy(self, t):
        """ControlPolicy(ocp_solver, t) of every instance, evaluated on the device (rtoc_control_policy): `t` a scalar or one time
        per instance; returns {"tauJ", "qJ", "dqJ": [batch, nu], "Kp", "Kd": [batch, nu, nu]}.  The grid times run from the t of the
        last discretisation, with switching-time optimisation over every instance's own time steps."""
        return self.ctx.control_policy(self.t0, self._policy_t(t), self.N)

    def get_control_input(self, t, q, v):
        """u [batch, nu] = tauJ - Kp (qJ - q) - Kd (dqJ - v) of that policy at the measured q [batch, nq], v [batch, nv]
        (bindings/python/robotoc_sim/mpc_simulation.py:6-11; rtoc_control_input: the gains are never written anywhere)"""
        x = np.concatenate([np.asarray(q, dtype=float).reshape(self.batch, -1), np.asarray(v, dtype=float).reshape(self.batch, -1)], axis=1)
        return self.ctx.control_input(self.t0, self._policy_t(t), self.N, x)

    def _policy_t(self, t):
        t = np.asarray(t, dtype=float)
        if t.ndim == 1 and t.size != self.batch:
            raise ValueError("t must be a scalar or one time per instance (%d), not %d values" % (self.batch, t.size))
        return t

    def init_constraints(self):
        """OCPSolver::initConstraints (ocp_solver.cpp:105-108)"""
        if self.has_rows:
            self.ctx.contact_init_constraints()
        self.ctx.sto_init_constraints()

    # ---- iteration ----
    def update_solution(self, t, x0=None):
        """OCPSolver::updateSolution (ocp_solver.cpp:111-145) of every instance; returns KKTError() of the iterate it linearised at"""
        if x0 is not None:
            self.ctx.set_initial_state(x0)
        return self.ctx.contact_update_solution(self.tau)

    def solve(self, t, x0, init_solver=True):
        """OCPSolver::solve (ocp_solver.cpp:148-225).  Convergence / mesh-refinement decisions are taken for the batch as a whole
        (every instance below the tolerance); with batch = 1 that is the reference's loop."""
        o = self.options
        c = self.ctx
        c.set_initial_state(x0)
        warm = o.solution_interpolation_on_device and o.enable_solution_interpolation
        if init_solver:
            self.discretize(t)
            if warm:
                c.solution_interpolate(self.t0)                                                        # :159-163
            self.init_constraints()
            c.line_search_clear()
        st = self.stats = SolverStatistics()
        sto_on = self.sto is not None and len(self.plan.events) > 0

        def set_reg(reg):                                                                              # :169-176
            c.sto_set_regularization(reg)
            st.ts.append(c.sto_event_times())

        def update():
            err = self.update_solution(t)
            st.kkt_error.append(err)
            return float(np.max(err))

        def max_dt():                                                                                  # :181-182
            self.event_times = c.sto_event_times()
            return self._max_time_step()
        # the schedule itself -- regularisation of the first iterations, mesh-refinement branch, convergence -- is rtoc_solve_loop's
        # (include/rtoc_robot.h): the same function the C++ shell runs
        st.convergence, st.iter, st.mesh_refinement_iter = capi.solve_loop(
            o.max_iter, o.kkt_tol, update, sto_enabled=sto_on, initial_sto_reg_iter=o.initial_sto_reg_iter, initial_sto_reg=o.initial_sto_reg,
            kkt_tol_mesh=o.kkt_tol_mesh, max_dt_mesh=o.max_dt_mesh, set_sto_regularization=set_reg if sto_on else None,
            max_time_step=max_dt if sto_on else None, mesh_refinement=(lambda: self._mesh_refinement(t)) if sto_on else None)
        if sto_on:
            self.event_times = c.sto_event_times()
        if warm:                                                                                       # :215-220
            c.sto_correct_time_steps()
            c.solution_store(self.t0)
        return st

    def kkt_error(self):
        """OCPSolver::KKTError(t, q, v) (ocp_solver.cpp:414-426) at the current iterate, without moving it"""
        c = self.ctx
        c.contact_eval_kkt()
        err = c.kkt_error()
        if self.sto is not None and self.plan.events:
            c.condense()
            c.sto_eval_kkt_device()
            err = np.sqrt(err ** 2 + c.sto_kkt_terms()[2])
        return err

    # ---- mesh refinement (ocp_solver.cpp:184-199) ----
    def _max_time_step(self):
        dt = self.ctx.sto_time_steps()
        return float(dt[:, :-1].max())

    def _mesh_refinement(self, t):
        if self.options.solution_interpolation_on_device:
            # store, discretize, interpolate (ocp_solver.cpp:185-192) without a record leaving the device
            self.ctx.sto_correct_time_steps()
            if self.options.enable_solution_interpolation:
                self.ctx.solution_store(self.t0)
            self.discretize(t)
            if self.options.enable_solution_interpolation:
                self.ctx.solution_interpolate(self.t0)
            self.init_constraints()
            self.ctx.line_search_clear()
            return
        old_grids, old_masks = self.grids, self.masks
        old_sol = self.get_solution()
        # correctTimeSteps(contact_sequence_, t) ahead of solution_interpolator_.store (ocp_solver.cpp:186-189): the device's time
        # steps date from the last evalKKT, before integrateSolution moved the event times
        self.ctx.sto_correct_time_steps()
        old_dt = self.ctx.sto_time_steps()
        self.discretize(t)   # new structure at the current event times, per-instance time steps on the device
        new_dt = self.ctx.sto_time_steps()
        if self.options.enable_solution_interpolation:
            new_sol = self.S.zeros(self.batch, len(self.grids))
            for b in range(self.batch):
                t_old = self.t0 + np.concatenate([[0.0], np.cumsum(old_dt[b, :-1])])
                t_new = self.t0 + np.concatenate([[0.0], np.cumsum(new_dt[b, :-1])])
                self._interpolate(old_grids, old_masks, t_old, old_dt[b], old_sol[b], self.grids, self.masks, t_new, new_sol[b])
            self.set_solution(new_sol)
        self.init_constraints()
        self.ctx.line_search_clear()

    def _expand(self, rec, mask, name):
        """contact-indexed [ncontacts, 6] view (3 or 6 rows used per contact: point / surface) of the compacted f / mu stack"""
        out, k = np.zeros((self.nc, 6)), 0
        x = self.S.f(rec, name)
        for cidx in range(self.nc):
            if (int(mask) >> cidx) & 1:
                r = self.model.contact_rows(cidx)
                out[cidx, :r] = x[k:k + r]
                k += r
        return out

    def _interpolate(self, g0, m0, t0s, dt0, s0, g1, m1, t1s, s1):
        """SolutionInterpolator::interpolate (src/solver/solution_interpolator.cpp:33-116) on the packed records"""
        S, nq, fl = self.S, self.model.nq, self.model.floating_base
        n0 = len(g0)

        def field(rec, name):
            return S.f(rec, name)

        def put_stack(rec, mask, name, by_contact):
            k = 0
            x = field(rec, name)
            x[:] = 0.0
            for cidx in range(self.nc):
                if (int(mask) >> cidx) & 1:
                    r = self.model.contact_rows(cidx)
                    x[k:k + r] = by_contact[cidx, :r]
                    k += r

        def blend(i, a, b, alpha, mode):
            """mode: full (interpolate :119-146), partial (:149-172), event (initEventSolution :175-198)"""
            ra, rb, out = s0[a], s0[b], s1[i]
            field(out, "q")[:nq] = interpolate_configuration(field(ra, "q")[:nq], field(rb, "q")[:nq], alpha, fl)
            for name in ("v", "lmd", "gmm"):
                field(out, name)[:] = (1 - alpha) * field(ra, name) + alpha * field(rb, name)
            fa, fb = self._expand(ra, m0[a], "f"), self._expand(rb, m0[b], "f")
            ma, mb = self._expand(ra, m0[a], "mu"), self._expand(rb, m0[b], "mu")
            if mode == "full":
                for name in ("u", "a", "beta", "nu_passive"):
                    field(out, name)[:] = (1 - alpha) * field(ra, name) + alpha * field(rb, name)
                act_b = np.array([(int(m0[b]) >> cidx) & 1 for cidx in range(self.nc)], dtype=bool)[:, None]
                f_, mu_ = np.where(act_b, (1 - alpha) * fa + alpha * fb, fa), np.where(act_b, (1 - alpha) * ma + alpha * mb, ma)
            elif mode == "partial":
                for name in ("u", "a", "beta", "nu_passive"):
                    field(out, name)[:] = field(ra, name)
                f_, mu_ = fa, ma
            else:
                field(out, "a")[:] = (1 - alpha) * field(ra, "a") + alpha * field(rb, "a")
                for name in ("u", "beta", "nu_passive"):
                    field(out, name)[:] = field(rb, name)
                f_, mu_ = fb, mb
            put_stack(out, m1[i], "f", f_)
            put_stack(out, m1[i], "mu", mu_)

        def copy(i, a):
            s1[i][:] = s0[a]
            # the stacks are compacted by the active contacts of the grid point: re-pack for the new grid point's mask
            put_stack(s1[i], m1[i], "f", self._expand(s0[a], m0[a], "f"))
            put_stack(s1[i], m1[i], "mu", self._expand(s0[a], m0[a], "mu"))

        def before(tt):   # findStoredGridIndexBeforeTime
            k = int(np.searchsorted(t0s, tt, side="right") - 1)
            k = min(max(k, 0), n0 - 2)
            while k > 0 and dt0[k] <= 0.0:   # an impact grid point has no extent in time
                k -= 1
            return k

        def stored_event(tt, kind):
            for k in range(n0 - 1):
                if g0[k].type == kind and abs(t0s[k] - tt) < 1e-9:
                    return k
            return -1
        N1 = len(g1) - 1
        for i, g in enumerate(g1):
            tt = t1s[i]
            if tt <= t0s[0]:
                copy(i, 0)
                continue
            if tt >= t0s[-1]:
                copy(i, n0 - 1)
                continue
            if g.type in (GRID_IMPACT, GRID_LIFT):
                k = stored_event(tt, g.type)
                if k >= 0:
                    copy(i, k)
                    if g.type == GRID_IMPACT:
                        for name in ("u", "a", "nu_passive"):
                            field(s1[i], name)[:] = 0.0
                        if i >= 2 and k >= 2:
                            field(s1[i - 2], "xi")[:] = field(s0[k - 2], "xi")
                    continue
                a = before(tt)
                alpha = min(max((tt - t0s[a]) / dt0[a], 0.0), 1.0)
                if g0[a + 1].type == GRID_TERMINAL:
                    blend(i, a, a + 1, alpha, "partial")
                    if g.type == GRID_IMPACT:
                        for name in ("u", "a", "nu_passive"):
                            field(s1[i], name)[:] = 0.0
                else:
                    blend(i, a, a + 1, alpha, "event")
                continue
            a = before(tt)
            alpha = min(max((tt - t0s[a]) / dt0[a], 0.0), 1.0)
            blend(i, a, a + 1, alpha, "full" if g0[a + 1].type == 0 else "partial")
        for name in ("u", "a", "f", "beta", "mu", "nu_passive"):   # modifyTerminalSolution
            field(s1[N1], name)[:] = 0.0

    def close(self):
        self.ctx.close()


def joint_limit_rows_for(model):
    """the six joint-limit components over the actuated joints, in the order examples/anymal/trot.cpp:134-146 adds them"""
    return joint_limit_rows(Dims(model.nv, model.nu, model.nv - model.nu, model.max_dimf, model.max_dimf, 0))
