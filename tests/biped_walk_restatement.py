"""numpy restatement, line by line, of the reference's BipedWalkFootStepPlanner -- the yardstick of tests/test_biped_walk_*.py and
tests/test_cpp_biped_walk_foot_step_planner.py.  Line numbers are the reference's.

  BipedWalkFootStepPlanner  src/mpc/biped_walk_foot_step_planner.cpp:49-277 (setGaitPattern, setRaibertGaitPattern, init, plan)

MovingWindowFilter, RaibertHeuristic, project_rotation_z and yaw_matrix are those of tests/foot_step_planner_restatement.py, and so are
the three MPC references, which take the number of contacts' full mask as an argument here (com_ref, configuration_ref below).

As with the quadrupeds, the reference's Robot is Pinocchio: the planner takes the kinematics (the two frame placements, the centre of
mass) as arguments, and the tests get them from oracle.rbd_contact_placement and task_cost_restatement.com.  Parity of the planner
with the reference is therefore by restatement and unpinned.

One thing is NOT the reference's: a contact status is matched exactly against STATUSES, as the device does (include/rtoc_robot.h);
the reference reads bits 0 and 1 alone.  Every status of the set takes the branch the reference takes for it."""
import numpy as np

import foot_step_planner_restatement as fsr
from foot_step_planner_restatement import (MovingWindowFilter, RaibertHeuristic, project_rotation_z, rotation_from_quaternion,
                                           yaw_matrix)


class BipedWalkFootStepPlanner:
    STATUSES = (0b11, 0b01, 0b10)   # bit 0: the left foot (surfaceContactFrames()[0], :17), bit 1: the right foot (:18)

    def __init__(self, yaw_projection=False):
        self.yaw_projection = yaw_projection
        self.raibert_heuristic, self.filter = RaibertHeuristic(), MovingWindowFilter()
        self.enable_raibert_heuristic, self.enable_double_support_phase = False, False
        self.current_step = 0
        self.left_to_right_leg_distance, self.foot_height_to_com_height = 0.0, 0.0
        self.contact_position_ref, self.contact_surface_ref, self.com_ref, self.R_ = [], [], [], []
        self.vcom_cmd, self.step_length = np.zeros(3), np.zeros(3)
        self.R_yaw, self.yaw_rate_cmd = np.eye(3), 0.0
        self.planning_size = 0

    def set_gait_pattern(self, step_length, step_yaw, enable_double_support_phase):   # :49-58
        self.step_length = np.array(step_length, dtype=np.float64)
        self.R_yaw = yaw_matrix(step_yaw)
        self.enable_double_support_phase = bool(enable_double_support_phase)
        self.enable_raibert_heuristic = False

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, swing_time, double_support_time, gain):   # :61-86
        if swing_time <= 0.0 or double_support_time < 0.0 or gain <= 0.0:   # :66-74
            raise ValueError("swing_time and gain must be positive, double_support_time non-negative")
        period = 2.0 * (swing_time + double_support_time)   # :75
        self.raibert_heuristic.set_parameters(period, gain)
        self.filter.set_parameters(period, 0.1 * period)
        self.vcom_cmd = np.array(vcom_cmd, dtype=np.float64)
        self.R_yaw = yaw_matrix(yaw_rate_cmd * (swing_time + double_support_time))   # :79-82
        self.yaw_rate_cmd = yaw_rate_cmd
        self.enable_double_support_phase = double_support_time > 0.0
        self.enable_raibert_heuristic = True

    def init(self, q, feet, com):   # :89-108; feet [2, 3] (left, right) and com at q
        R = project_rotation_z(rotation_from_quaternion(q[3:7]), self.yaw_projection)
        feet, com = np.asarray(feet, dtype=np.float64), np.asarray(com, dtype=np.float64)
        local = [R.T @ (feet[i] - q[:3]) for i in range(2)]   # :93-95: relative to the base
        self.left_to_right_leg_distance = local[0][1] - local[1][1]   # :96-97
        foot_height = 0.5 * (feet[0][2] + feet[1][2])   # :98-99
        self.foot_height_to_com_height = com[2] - foot_height   # :100
        self.contact_position_ref, self.contact_surface_ref, self.com_ref = [], [], []
        self.R_ = [R]
        self.filter.clear()
        self.current_step = 0

    def _push(self, com, p, S, R):
        self.com_ref.append(com.copy())
        self.contact_position_ref.append([x.copy() for x in p])
        self.contact_surface_ref.append([x.copy() for x in S])
        self.R_.append(R.copy())

    def plan(self, t, q, feet, surfaces, v, contact_status, planning_steps):
        """:111-277; feet [2, 3] and surfaces [2, 3, 3]: the two frame placements at q; contact_status: bit k = contact k active"""
        assert planning_steps >= 0
        if contact_status not in self.STATUSES:
            return False
        if self.enable_raibert_heuristic:   # :116-123
            vcom = np.asarray(v, dtype=np.float64)[:3]
            self.filter.push_back(t, vcom[:2])
            self.raibert_heuristic.plan_step_length(self.filter.average, self.vcom_cmd[:2], self.yaw_rate_cmd)
            self.step_length = self.raibert_heuristic.step_length.copy()
        base = np.asarray(q, dtype=np.float64)[:3]
        p = [np.array(feet[i], dtype=np.float64) for i in range(2)]       # :125-128
        S = [np.array(surfaces[i], dtype=np.float64) for i in range(2)]
        R = self.R_[0]                                                     # :130
        local = [R.T @ (p[i] - base) for i in range(2)]                    # :131-135
        sl, dsp = self.step_length, self.enable_double_support_phase
        left, right = bool(contact_status & 1), bool(contact_status & 2)
        if left and right:   # :136-147
            if dsp:
                if self.current_step % 2 != 0:
                    self.current_step += 1
            else:
                self.current_step = 0
        elif left:   # :148-169
            if (self.current_step % 4 != 1) if dsp else (self.current_step % 2 != 1):
                self.current_step += 1
                R = self.R_yaw @ R
            local[1] = local[0] - 0.5 * (self.R_yaw.T @ sl)
            local[1][1] -= self.left_to_right_leg_distance
            p[1] = R @ local[1] + base
            S[1] = R.copy()
        else:   # :170-191
            if (self.current_step % 4 != 3) if dsp else (self.current_step % 2 != 0):
                self.current_step += 1
                R = self.R_yaw @ R
            local[0] = local[1] - 0.5 * (self.R_yaw.T @ sl)
            local[0][1] += self.left_to_right_leg_distance
            p[0] = R @ local[0] + base
            S[0] = R.copy()
        com = 0.5 * (p[0] + p[1])   # :145-146, :167-168, :189-190
        com[2] += self.foot_height_to_com_height
        self.com_ref, self.contact_position_ref, self.contact_surface_ref, self.R_ = [], [], [], []   # :195-200
        self._push(com, p, S, R)
        first = 0.5 if self.enable_raibert_heuristic else 0.25
        for step in range(self.current_step, planning_steps + self.current_step + 1):   # :201-266
            if step == 0:
                pass
            elif self.current_step == 0 and step == 1:   # :206-216, :239-249
                R = self.R_yaw @ R
                com = com + first * (R @ sl)
                p[1] = p[1] + 0.5 * (R @ sl)
                S[1] = R.copy()
            elif dsp:   # :217-228
                if step % 4 == 1:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    p[1] = p[1] + R @ sl
                    S[1] = R.copy()
                elif step % 4 == 3:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    p[0] = p[0] + R @ sl
                    S[0] = R.copy()
            elif step % 2 == 1:   # :250-255
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                p[1] = p[1] + R @ sl
                S[1] = R.copy()
            else:   # :256-261
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                p[0] = p[0] + R @ sl
                S[0] = R.copy()
            self._push(com, p, S, R)
        self.planning_size = len(self.com_ref)   # :275
        return True

    def size(self):
        return self.planning_size

    def contact_positions(self, step):
        return np.array(self.contact_position_ref[step])

    def contact_surfaces(self, step):
        return np.array(self.contact_surface_ref[step])

    def com(self, step):
        return self.com_ref[step]

    def R(self, step):
        return self.R_[step]


# ---- the MPC references on two contacts.  The swing-foot reference does not look at the other contacts and is fsr's as it is;
# "some contact is inactive" (mpc_periodic_com_ref.cpp:69-79, mpc_periodic_configuration_ref.cpp alike) is judged per contact of the
# MODEL, so fsr's `& 0xF` forms are restated with the two-contact mask ----
FULL = 0b11
swing_foot_ref = fsr.swing_foot_ref


def has_inactive_contact(mask):
    return (mask & FULL) != FULL


def com_ref(com, masks, t, phase, swing_start_time, period_active, period_inactive, num_phases_in_period):
    """(com_ref, isActive): mpc_periodic_com_ref.cpp:90-110"""
    if not (t > swing_start_time and has_inactive_contact(masks[phase])):
        return np.array(com[phase]), False
    _, rate = fsr.swing_rate(t, swing_start_time, period_active, period_inactive)
    return (1.0 - rate) * com[phase] + rate * com[phase + num_phases_in_period], True


def configuration_ref(q, R, masks, t, phase, swing_start_time, period_active, period_inactive, num_phases_in_period):
    """(q_ref, isActive = True): mpc_periodic_configuration_ref.cpp:92-115"""
    q_ref = np.array(q, dtype=np.float64)
    if t > swing_start_time and has_inactive_contact(masks[phase]):
        _, rate = fsr.swing_rate(t, swing_start_time, period_active, period_inactive)
        q_ref[3:7] = fsr.eigen_slerp(fsr.eigen_quaternion(R[phase]), rate, fsr.eigen_quaternion(R[phase + num_phases_in_period]))
    else:
        q_ref[3:7] = fsr.eigen_quaternion(R[phase])
    return q_ref, True
