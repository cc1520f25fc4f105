"""TrotFootStepPlanner, CrawlFootStepPlanner, PaceFootStepPlanner, FlyingTrotFootStepPlanner, BipedWalkFootStepPlanner and
JumpFootStepPlanner over a
capi.Context: the surface of the reference's classes (src/mpc/{trot,crawl,pace,flying_trot,biped_walk,jump}_foot_step_planner.cpp) for a
batch, every instance with its own command.  The planning runs on the device (rtoc_foot_step_*, include/rtoc_robot.h); these shells
hold no state of their own beyond the commands they were given.  The five periodic gaits share one body; a class names its gait, its legal contact statuses and what its setters
check.  The jump has its own setter, plans without a step count, and places by MPCJump's mapping."""
import numpy as np

from . import capi


class TrotFootStepPlanner:
    GAIT = capi.GAIT_TROT
    STATUSES = (0b1111, 0b1001, 0b0110)   # the contact statuses plan() accepts; the reference returns false for any other

    def __init__(self, ctx, projection=capi.PROJECT_AS_REFERENCE):
        """`ctx`: a capi.Context with a robot model of four point contacts (LF, LH, RF, RH).  `projection`: how init projects the
        base rotation onto the z axis -- PROJECT_AS_REFERENCE repeats the reference's arithmetic, which divides by
        R00^2 + 2 R01 and fails near a yaw of 0.427 rad (include/rtoc_robot.h); PROJECT_YAW is the rotation about z"""
        self.ctx, self.projection = ctx, projection
        self._plan = None

    def _per_instance(self, name, a, width):
        a = np.asarray(a, dtype=np.float64)
        shape = (width,) if width else ()
        if a.shape == shape:
            return np.broadcast_to(a, (self.ctx.batch,) + shape), False
        if a.shape == (self.ctx.batch,) + shape:
            return a, True
        raise ValueError("%s must have the shape %s or %s, not %s" % (name, shape, (self.ctx.batch,) + shape, a.shape))

    def _set(self, structs, per_instance):
        self.ctx.set_foot_step_planner(structs if per_instance else structs[0])
        self._plan = None

    def set_gait_pattern(self, step_length, step_yaw, enable_stance_phase):
        """setGaitPattern: step_length [3] or [batch, 3], step_yaw a scalar or [batch]"""
        sl, inst_l = self._per_instance("step_length", step_length, 3)
        yaw, inst_y = self._per_instance("step_yaw", step_yaw, 0)
        structs = []
        for b in range(self.ctx.batch):
            p = capi.FootStepPlanner()
            p.gait, p.mode, p.projection, p.enable_stance_phase = self.GAIT, capi.FOOT_STEP_FIXED, self.projection, int(bool(enable_stance_phase))
            p.step_length[:], p.step_yaw = [float(x) for x in sl[b]], float(yaw[b])
            structs.append(p)
        self._set(structs, inst_l or inst_y)

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, swing_time, stance_time, gain):
        """setRaibertGaitPattern: vcom_cmd [3] or [batch, 3], yaw_rate_cmd a scalar or [batch]; the gait timing and the gain are
        shared by the batch"""
        self._check_timing(swing_time, stance_time, gain)
        vc, inst_v = self._per_instance("vcom_cmd", vcom_cmd, 3)
        yr, inst_y = self._per_instance("yaw_rate_cmd", yaw_rate_cmd, 0)
        structs = []
        for b in range(self.ctx.batch):
            p = capi.FootStepPlanner()
            p.gait, p.mode, p.projection = self.GAIT, capi.FOOT_STEP_RAIBERT, self.projection
            p.swing_time, p.stance_time, p.gain = float(swing_time), float(stance_time), float(gain)
            p.vcom_cmd[:], p.yaw_rate_cmd = [float(x) for x in vc[b]], float(yr[b])
            structs.append(p)
        self._set(structs, inst_v or inst_y)

    @staticmethod
    def _check_timing(swing_time, stance_time, gain):
        if swing_time <= 0.0:
            raise ValueError("'swing_time' must be positive")
        if stance_time < 0.0:
            raise ValueError("'stance_time' must be non-negative")
        if gain <= 0.0:
            raise ValueError("'gain' must be positive")

    def init(self, x0=None):
        """init(q) of every instance; x0 [batch, nq + nv]: set as the context's initial state first (None: as it stands)"""
        if x0 is not None:
            self.ctx.set_initial_state(x0)
        self.ctx.foot_step_planner_init()
        self._plan = None

    def plan(self, t, contact_status, planning_steps, x0=None):
        """plan(t, q, v, contact_status, planning_steps) of every instance; contact_status: the bit mask of the active contacts of
        the first contact phase.  False where the reference returns false (a status outside the gait's STATUSES)."""
        if x0 is not None:
            self.ctx.set_initial_state(x0)
        if int(contact_status) not in self.STATUSES:
            return False
        self.ctx.foot_step_plan(t, contact_status, planning_steps)
        self._plan = None
        return True

    def _get(self):
        if self._plan is None:
            self._plan = self.ctx.foot_step_plan_get()
        return self._plan

    def size(self):
        return self._get()["size"]

    def contact_positions(self, step):
        """[batch, 4, 3]"""
        return self._get()["positions"][:, step]

    def com(self, step):
        """[batch, 3]"""
        return self._get()["com"][:, step]

    def R(self, step):
        """[batch, 3, 3]"""
        return self._get()["R"][:, step]

    def step_length(self):
        """[batch, 3]: the step length in force (with the heuristic: what it planned at the last plan)"""
        return self._get()["step_length"]

    def ok(self):
        """[batch] bool: every number of the instance's plan is finite"""
        return self._get()["ok"]

    def reset_contact_placements(self, t, contact_status, phase_of_grid_point, phase_masks, refs, x0=None):
        """What MPCTrot::resetContactPlacements does per control tick (src/mpc/mpc_trot.cpp:357-372; MPCCrawl, MPCPace and
        MPCFlyingTrot repeat it line for line): plan with planning_steps =
        the number of contact phases, the placements of every phase into the per-instance table, the three references into their
        tables.  phase_of_grid_point: GridInfo::phase of every grid point relative to the first; phase_masks: the active contacts
        of every phase; refs: a capi.FootStepRefs.  Returns what plan returns."""
        if not self.plan(t, contact_status, len(phase_masks), x0):
            return False
        self.ctx.foot_step_place(phase_of_grid_point)
        self.ctx.foot_step_refs(refs, phase_of_grid_point, phase_masks)
        return True


class CrawlFootStepPlanner(TrotFootStepPlanner):
    """src/mpc/crawl_foot_step_planner.cpp: three feet stand while RH, RF, LH, LF swing in turn; the setters are the trot's"""
    GAIT = capi.GAIT_CRAWL
    STATUSES = (0b1111, 0b0111, 0b1011, 0b1101, 0b1110)


class PaceFootStepPlanner(TrotFootStepPlanner):
    """src/mpc/pace_foot_step_planner.cpp: the trot with the pairs (LF, LH) and (RF, RH); the setters are the trot's"""
    GAIT = capi.GAIT_PACE
    STATUSES = (0b1111, 0b0011, 0b1100)


class BipedWalkFootStepPlanner(TrotFootStepPlanner):
    """src/mpc/biped_walk_foot_step_planner.cpp on a robot model of two contact surfaces (left = contact 0, right = contact 1):
    one foot stands while the other swings, the right one first; every foot of the plan carries a rotation, which
    reset_contact_placements writes into the per-instance rotation table beside the translations
    (MPCBipedWalk::resetContactPlacements, src/mpc/mpc_biped_walk.cpp:347-359).  refs.foot_term[2:] must be negative and the
    phase masks have two bits."""
    GAIT = capi.GAIT_BIPED_WALK
    STATUSES = (0b11, 0b01, 0b10)   # both feet, the left foot alone (the right one swings), the right foot alone

    def set_gait_pattern(self, step_length, step_yaw, enable_double_support_phase):
        """setGaitPattern (:49-58): step_length [3] or [batch, 3], step_yaw a scalar or [batch]"""
        super().set_gait_pattern(step_length, step_yaw, enable_double_support_phase)

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, swing_time, double_support_time, gain):
        """setRaibertGaitPattern (:61-86): as the trot's, with double_support_time where that has stance_time"""
        super().set_raibert_gait_pattern(vcom_cmd, yaw_rate_cmd, swing_time, double_support_time, gain)

    @staticmethod
    def _check_timing(swing_time, double_support_time, gain):   # :66-74
        if swing_time <= 0.0:
            raise ValueError("'swing_time' must be positive")
        if double_support_time < 0.0:
            raise ValueError("'double_support_time' must be non-negative")
        if gain <= 0.0:
            raise ValueError("'gain' must be positive")

    def contact_positions(self, step):
        """[batch, 2, 3]"""
        return self._get()["positions"][:, step]

    def contact_surfaces(self, step):
        """[batch, 2, 3, 3]"""
        return self._get()["surfaces"][:, step]

    def contact_placements(self, step):
        """(rotations [batch, 2, 3, 3], translations [batch, 2, 3]): contactPlacements(step) as SE3's two parts"""
        return self.contact_surfaces(step), self.contact_positions(step)


class FlyingTrotFootStepPlanner(TrotFootStepPlanner):
    """src/mpc/flying_trot_foot_step_planner.cpp: a trot with a flight (contact status 0) between the pairs; the plan is
    planning_steps + 3 steps long, planning_steps at most capi.MAX_PLAN_STEPS - 1, and there is no stance-phase option"""
    GAIT = capi.GAIT_FLYING_TROT
    STATUSES = (0b1111, 0b1001, 0b0110, 0b0000)

    def set_gait_pattern(self, step_length, step_yaw):
        """setGaitPattern: step_length [3] or [batch, 3], step_yaw a scalar or [batch]"""
        super().set_gait_pattern(step_length, step_yaw, False)

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, flying_time, stance_time, gain):
        """setRaibertGaitPattern: as the trot's, with flying_time where that has swing_time"""
        super().set_raibert_gait_pattern(vcom_cmd, yaw_rate_cmd, flying_time, stance_time, gain)

    @staticmethod
    def _check_timing(flying_time, stance_time, gain):
        if flying_time <= 0.0:
            raise ValueError("'flying_time' must be positive")
        if stance_time <= 0.0:
            raise ValueError("'stance_time' must be positive")
        if gain <= 0.0:
            raise ValueError("'gain' must be positive")


class JumpFootStepPlanner(TrotFootStepPlanner):
    """src/mpc/jump_foot_step_planner.cpp on a robot model of four point contacts or of two contact surfaces: one jump of
    jump_length and step_yaw, each instance's own.  init measures the feet, sets the goal placements, the goal centre of mass and
    the q_ref of MPCJump::init (src/mpc/mpc_jump.cpp:141-145); the plan has three steps until the feet leave the ground and two
    from then on.  The receding horizon of MPCJump::updateSolution stays with the caller."""
    GAIT = capi.GAIT_JUMP

    def set_jump_pattern(self, jump_length, step_yaw):
        """setJumpPattern (:43-49): jump_length [3] or [batch, 3], step_yaw a scalar or [batch]"""
        super().set_gait_pattern(jump_length, step_yaw, False)

    def set_gait_pattern(self, *args):
        raise TypeError("a jump has no gait pattern: set_jump_pattern")

    def set_raibert_gait_pattern(self, *args):
        raise TypeError("the reference has no Raibert form of a jump: set_jump_pattern")

    def _feet(self):
        return self.ctx._model_ncontacts

    def plan(self, t, contact_status, planning_steps=0, x0=None):
        """plan(t, q, v, contact_status, planning_steps) (:127-170); t and planning_steps are not read.  Any contact status of the
        model's contacts is accepted, as in the reference; a bit beyond them raises."""
        if x0 is not None:
            self.ctx.set_initial_state(x0)
        self.ctx.foot_step_plan(t, contact_status, planning_steps)
        self._plan = None
        return True

    def current_step(self):
        return self._get()["current_step"]

    def contact_positions(self, step):
        """[batch, feet, 3]: the translations of contactPlacements(step), every foot"""
        return self._get()["positions"][:, step]

    def contact_surfaces(self, step):
        """[batch, feet, 3, 3]: the rotations of contactPlacements(step); identities for a quadruped (:99-105)"""
        g = self._get()
        if "surfaces" in g:
            return g["surfaces"][:, step]
        return np.broadcast_to(np.eye(3), (self.ctx.batch, self._feet(), 3, 3)).copy()

    def contact_placements(self, step):
        """(rotations [batch, feet, 3, 3], translations [batch, feet, 3]): contactPlacements(step) as SE3's two parts"""
        return self.contact_surfaces(step), self.contact_positions(step)

    def jump_length(self):
        """[batch, 3]"""
        return self._get()["step_length"]

    def set_configuration_ref(self):
        """config_cost_->set_q_ref(q_ref) of MPCJump::init for every instance: the q_ref stored by init onto every row of the
        per-instance configuration reference of the grid in force"""
        r = capi.FootStepRefs()
        r.foot_term[:] = [-1] * 4
        r.com_term, r.configuration = -1, 1
        self.ctx.foot_step_refs(r)

    def reset_contact_placements(self, t, contact_status, phase_of_grid_point, x0=None):
        """MPCJump::resetContactPlacements (src/mpc/mpc_jump.cpp:301-317): plan, then contact phase 0 <- contactPlacements(1) and,
        before the flight, phases 1 and 2 <- contactPlacements(2); after it every phase <- contactPlacements(1).
        phase_of_grid_point: GridInfo::phase of every grid point relative to the first."""
        self.plan(t, contact_status, 0, x0)
        self.place(phase_of_grid_point)
        return True

    def place(self, phase_of_grid_point):
        """the placing half of reset_contact_placements, from the plan as it stands: what a re-discretisation repeats"""
        self._plan = None   # (the plan may have moved on through the context)
        ph = np.minimum(np.asarray(phase_of_grid_point, dtype=np.int32), self.size() - 2)
        self.ctx.foot_step_place(ph)
