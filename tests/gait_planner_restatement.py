"""numpy restatement, line by line, of the reference's crawl, pace and flying-trot foot-step planners -- the yardstick of
tests/test_gait_planner_*.py and tests/test_cpp_gait_foot_step_planner.py.  Line numbers are the reference's.

  CrawlFootStepPlanner       src/mpc/crawl_foot_step_planner.cpp:51-366 (setGaitPattern, setRaibertGaitPattern, init, plan)
  PaceFootStepPlanner        src/mpc/pace_foot_step_planner.cpp:51-283
  FlyingTrotFootStepPlanner  src/mpc/flying_trot_foot_step_planner.cpp:50-240

MovingWindowFilter, RaibertHeuristic, project_rotation_z and yaw_matrix are those of tests/foot_step_planner_restatement.py.

As with the trot, the reference's Robot is Pinocchio: the planners take the kinematics (foot positions, centre of mass) as arguments,
and the tests get them from oracle.rbd_contact_placement and task_cost_restatement.com.  Parity of the planners with the reference is
therefore by restatement and unpinned.

One thing is NOT the reference's: a contact status is matched exactly against the gait's own set (STATUSES), as the device does
(include/rtoc_robot.h).  The reference's chains test pairs or triples of contacts and would take, say, 0b1011 for a pace or flying
trot's 0b0011 / 0b1001; its flying trot treats every status that is none of the others as a flight.  Every status of a gait's set
takes the branch the reference takes for it."""
import numpy as np

from foot_step_planner_restatement import (MovingWindowFilter, RaibertHeuristic, project_rotation_z, rotation_from_quaternion,
                                           yaw_matrix)


class _Planner:
    """what the three classes share word for word: members, setGaitPattern, the accessors"""
    STATUSES = ()
    PERIODS = 2.0   # the Raibert period in units of swing_time + stance_time

    def __init__(self, yaw_projection=False):
        self.yaw_projection = yaw_projection
        self.raibert_heuristic, self.filter = RaibertHeuristic(), MovingWindowFilter()
        self.enable_raibert_heuristic, self.enable_stance_phase = False, False
        self.current_step = 0
        self.contact_position_ref, self.com_ref, self.R_ = [], [], []
        self.local = None
        self.vcom_cmd, self.step_length = np.zeros(3), np.zeros(3)
        self.R_yaw, self.yaw_rate_cmd = np.eye(3), 0.0
        self.planning_size = 0

    def set_gait_pattern(self, step_length, step_yaw, enable_stance_phase):   # crawl :51-60, pace :51-60
        self.step_length = np.array(step_length, dtype=np.float64)
        self.R_yaw = yaw_matrix(step_yaw)
        self.enable_stance_phase = bool(enable_stance_phase)
        self.enable_raibert_heuristic = False

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, swing_time, stance_time, gain):   # crawl :63-88, pace :63-88
        if swing_time <= 0.0 or stance_time < 0.0 or gain <= 0.0:
            raise ValueError("swing_time and gain must be positive, stance_time non-negative")
        period = self.PERIODS * (swing_time + stance_time)
        self.raibert_heuristic.set_parameters(period, gain)
        self.filter.set_parameters(period, 0.1 * period)
        self.vcom_cmd = np.array(vcom_cmd, dtype=np.float64)
        self.R_yaw = yaw_matrix(yaw_rate_cmd * (swing_time + stance_time))
        self.yaw_rate_cmd = yaw_rate_cmd
        self.enable_stance_phase = stance_time > 0.0
        self.enable_raibert_heuristic = True

    def init(self, q, feet, com):   # crawl :107-120 (com_ref_ stays empty), pace :91-105, flying trot :101-115; feet [4, 3] and com at q
        R = project_rotation_z(rotation_from_quaternion(q[3:7]), self.yaw_projection)
        feet, com = np.asarray(feet, dtype=np.float64), np.asarray(com, dtype=np.float64)
        self.local = [R.T @ (feet[i] - com) for i in range(4)]
        self.contact_position_ref = []
        self.com_ref = [com.copy()]
        self.R_ = [R]
        self.filter.clear()
        self.current_step = 0

    def _heuristic(self, t, v):   # the head of every plan(): crawl :128-135, pace :129-136, flying trot :123-130
        if self.enable_raibert_heuristic:
            vcom = np.asarray(v, dtype=np.float64)[:3]
            self.filter.push_back(t, vcom[:2])
            self.raibert_heuristic.plan_step_length(self.filter.average, self.vcom_cmd[:2], self.yaw_rate_cmd)
            self.step_length = self.raibert_heuristic.step_length.copy()

    def _push(self, com, cp, R):
        self.com_ref.append(com.copy())
        self.contact_position_ref.append([p.copy() for p in cp])
        self.R_.append(R.copy())

    def size(self):
        return self.planning_size

    def contact_positions(self, step):
        return np.array(self.contact_position_ref[step])

    def com(self, step):
        return self.com_ref[step]

    def R(self, step):
        return self.R_[step]


class CrawlFootStepPlanner(_Planner):
    STATUSES = (0b1111, 0b0111, 0b1011, 0b1101, 0b1110)
    PERIODS = 4.0   # :77

    def plan(self, t, feet, v, contact_status, planning_steps):   # :123-366; contact_status: bit k = contact k active
        assert planning_steps >= 0
        if contact_status not in self.STATUSES:
            return False
        self._heuristic(t, v)
        cp = [np.array(feet[i], dtype=np.float64) for i in range(4)]   # :136-140
        act = [bool((contact_status >> i) & 1) for i in range(4)]
        com = np.zeros(3)
        R = self.R_[0]
        L, sl = self.local, self.step_length
        if all(act):   # :143-158
            if self.enable_stance_phase:
                if self.current_step % 2 != 0:
                    self.current_step += 1
            else:
                self.current_step = 0
            for i in range(4):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 4.0
        else:
            # :159-250: the four branches differ in the three stance feet, the residues and the swing foot
            if act[0] and act[1] and act[2]:
                stand, res8, res4, swing = (0, 1, 2), 1, 1, 3
            elif act[0] and act[1] and act[3]:
                stand, res8, res4, swing = (0, 1, 3), 3, 2, 2
            elif act[0] and act[2] and act[3]:
                stand, res8, res4, swing = (0, 2, 3), 5, 3, 1
            elif act[1] and act[2] and act[3]:
                stand, res8, res4, swing = (1, 2, 3), 7, 0, 0
            else:
                return False
            if (self.current_step % 8 != res8) if self.enable_stance_phase else (self.current_step % 4 != res4):
                self.current_step += 1
                R = self.R_yaw @ R
            for i in stand:
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 3.0
            cp[swing] = com + R @ (L[swing] - 0.5 * sl)
        self.com_ref, self.contact_position_ref, self.R_ = [], [], []   # :254-259
        self._push(com, cp, R)
        first = 0.25 if self.enable_raibert_heuristic else 0.125
        for step in range(self.current_step, planning_steps + self.current_step + 1):   # :260-359
            if self.enable_stance_phase:   # :261-308
                if step == 0:
                    pass
                elif step == 1:
                    R = self.R_yaw @ R
                    com = com + first * (R @ sl)
                    cp[3] = cp[3] + 0.5 * (R @ sl)
                elif step == 3:
                    R = self.R_yaw @ R
                    com = com + first * (R @ sl)
                    cp[2] = cp[2] + 0.5 * (R @ sl)
                elif step % 8 == 1:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[3] = cp[3] + R @ sl
                elif step % 8 == 3:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[2] = cp[2] + R @ sl
                elif step % 8 == 5:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[1] = cp[1] + R @ sl
                elif step % 8 == 7:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[0] = cp[0] + R @ sl
            else:   # :311-358
                if step == 0:
                    pass
                elif step == 1:
                    R = self.R_yaw @ R
                    com = com + first * (R @ sl)
                    cp[3] = cp[3] + 0.5 * (R @ sl)
                elif step == 2:
                    R = self.R_yaw @ R
                    com = com + first * (R @ sl)
                    cp[2] = cp[2] + 0.5 * (R @ sl)
                elif step % 4 == 1:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[3] = cp[3] + R @ sl
                elif step % 4 == 2:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[2] = cp[2] + R @ sl
                elif step % 4 == 3:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[1] = cp[1] + R @ sl
                else:
                    R = self.R_yaw @ R
                    com = com + 0.25 * (R @ sl)
                    cp[0] = cp[0] + R @ sl
            self._push(com, cp, R)
        self.planning_size = len(self.com_ref)
        return True


class PaceFootStepPlanner(_Planner):
    STATUSES = (0b1111, 0b0011, 0b1100)

    def plan(self, t, feet, v, contact_status, planning_steps):   # :124-283
        assert planning_steps >= 0
        if contact_status not in self.STATUSES:
            return False
        self._heuristic(t, v)
        cp = [np.array(feet[i], dtype=np.float64) for i in range(4)]   # :137-141
        act = [bool((contact_status >> i) & 1) for i in range(4)]
        com = np.zeros(3)
        R = self.R_[0]
        L, sl = self.local, self.step_length
        if all(act):   # :144-159
            if self.enable_stance_phase:
                if self.current_step % 2 != 0:
                    self.current_step += 1
            else:
                self.current_step = 0
            for i in range(4):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 4.0
        elif act[0] and act[1]:   # :160-180
            if (self.current_step % 4 != 1) if self.enable_stance_phase else (self.current_step % 2 != 1):
                self.current_step += 1
                R = self.R_yaw @ R
            for i in (0, 1):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[2] = com + R @ (L[2] - 0.5 * sl)
            cp[3] = com + R @ (L[3] - 0.5 * sl)
        elif act[2] and act[3]:   # :181-201
            if (self.current_step % 4 != 3) if self.enable_stance_phase else (self.current_step % 2 != 0):
                self.current_step += 1
                R = self.R_yaw @ R
            for i in (2, 3):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[0] = com + R @ (L[0] - 0.5 * sl)
            cp[1] = com + R @ (L[1] - 0.5 * sl)
        else:
            return False
        self.com_ref, self.contact_position_ref, self.R_ = [], [], []   # :205-210
        self._push(com, cp, R)
        for step in range(self.current_step, planning_steps + self.current_step + 1):   # :211-276
            if step == 0:
                pass
            elif self.current_step == 0 and step == 1:   # :216-226, :249-259
                R = self.R_yaw @ R
                com = com + (0.5 if self.enable_raibert_heuristic else 0.25) * (R @ sl)
                cp[2], cp[3] = com + R @ L[2], com + R @ L[3]
            elif self.enable_stance_phase:   # :227-238
                if step % 4 == 1:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    cp[2], cp[3] = com + R @ L[2], com + R @ L[3]
                elif step % 4 == 3:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    cp[0], cp[1] = com + R @ L[0], com + R @ L[1]
            elif step % 2 == 1:   # :260-265
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[2], cp[3] = com + R @ L[2], com + R @ L[3]
            else:   # :266-271
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[0], cp[1] = com + R @ L[0], com + R @ L[1]
            self._push(com, cp, R)
        self.planning_size = len(self.com_ref)
        return True


class FlyingTrotFootStepPlanner(_Planner):
    STATUSES = (0b1111, 0b1001, 0b0110, 0b0000)

    def set_gait_pattern(self, step_length, step_yaw):   # :50-57
        super().set_gait_pattern(step_length, step_yaw, False)

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, flying_time, stance_time, gain):   # :60-82
        if flying_time <= 0.0 or stance_time <= 0.0 or gain <= 0.0:
            raise ValueError("flying_time, stance_time and gain must be positive")
        super().set_raibert_gait_pattern(vcom_cmd, yaw_rate_cmd, flying_time, stance_time, gain)
        self.enable_stance_phase = False   # no such member

    def plan(self, t, feet, v, contact_status, planning_steps):   # :118-240
        assert planning_steps >= 0
        if contact_status not in self.STATUSES:
            return False
        self._heuristic(t, v)
        cp = [np.array(feet[i], dtype=np.float64) for i in range(4)]   # :131-135
        act = [bool((contact_status >> i) & 1) for i in range(4)]
        com = self.com_ref[0].copy()   # :136
        R = self.R_[0]
        L, sl = self.local, self.step_length
        if all(act):   # :138-147
            self.current_step = 0
            com = np.zeros(3)
            for i in range(4):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 4.0
        elif act[0] and act[3]:   # :148-161
            if self.current_step % 4 != 1:
                self.current_step += 1
                R = self.R_yaw @ R
            com = np.zeros(3)
            for i in (0, 3):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[1] = com + R @ (L[1] - 0.5 * sl)
            cp[2] = com + R @ (L[2] - 0.5 * sl)
        elif act[1] and act[2]:   # :162-175
            if self.current_step % 4 != 3:
                self.current_step += 1
                R = self.R_yaw @ R
            com = np.zeros(3)
            for i in (1, 2):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[0] = com + R @ (L[0] - 0.5 * sl)
            cp[3] = com + R @ (L[3] - 0.5 * sl)
        else:   # :176-183: the flight.  contact_position_ref_[0] of a planner that has not planned is an empty vector: IndexError here
            previous = self.contact_position_ref[0]
            if self.current_step % 2 != 0:
                self.current_step += 1
            for i in range(4):
                cp[i] = previous[i].copy()
        self.com_ref, self.contact_position_ref, self.R_ = [], [], []   # :184-189
        self._push(com, cp, R)
        for step in range(self.current_step, planning_steps + self.current_step + 1):   # :190-230
            if step == 0:
                pass
            elif self.current_step == 0 and step == 1:
                pass
            elif self.current_step == 0 and step == 2:   # :197-207
                R = self.R_yaw @ R
                com = com + (0.5 if self.enable_raibert_heuristic else 0.25) * (R @ sl)
                cp[1], cp[2] = com + R @ L[1], com + R @ L[2]
            elif step % 4 == 1:
                pass
            elif step % 4 == 2:   # :211-216
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[1], cp[2] = com + R @ L[1], com + R @ L[2]
            elif step % 4 == 3:
                pass
            else:   # :220-225
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[0], cp[3] = com + R @ L[0], com + R @ L[3]
            self._push(com, cp, R)
        self._push(com, cp, R)   # :231-233
        self.planning_size = len(self.com_ref)
        return True


PLANNERS = {"crawl": CrawlFootStepPlanner, "pace": PaceFootStepPlanner, "flying_trot": FlyingTrotFootStepPlanner}
