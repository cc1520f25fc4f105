"""numpy restatement, line by line, of the reference's trot foot-step planning and the MPC references built on it -- the yardstick
of tests/test_foot_step_planner_*.py.  Line numbers are the reference's.

  MovingWindowFilter   include/robotoc/mpc/moving_window_filter.hpp:101-135
  RaibertHeuristic     src/mpc/raibert_heuristic.cpp:38-55
  TrotFootStepPlanner  src/mpc/trot_foot_step_planner.cpp:51-284 (setGaitPattern, setRaibertGaitPattern, init, plan)
  project_rotation_z   include/robotoc/utils/rotation.hpp:103-111, as it stands (NOT the norm of the row)
  swing_foot_ref       src/mpc/mpc_periodic_swing_foot_ref.cpp:90-110
  com_ref              src/mpc/mpc_periodic_com_ref.cpp:90-110
  configuration_ref    src/mpc/mpc_periodic_configuration_ref.cpp:92-115, with Eigen's Quaterniond(Matrix3d) and slerp

The reference's Robot is Pinocchio: the planner takes the kinematics (foot positions, centre of mass) as arguments, and the tests
get them from oracle.rbd_contact_placement and task_cost_restatement.com.  Parity of the planner with the reference is therefore by
restatement and unpinned; MovingWindowFilter and RaibertHeuristic depend on Eigen alone."""
import collections

import numpy as np


class MovingWindowFilter:
    def __init__(self, time_length=0.0, min_sampling_period=0.0):
        self.time_length, self.min_sampling_period = time_length, min_sampling_period
        self.clear()

    def set_parameters(self, time_length, min_sampling_period=0.0):   # :86-96
        if time_length <= 0.0 or min_sampling_period < 0:
            raise ValueError("time_length must be positive, min_sampling_period non-negative")
        self.time_length, self.min_sampling_period = time_length, min_sampling_period

    def clear(self):   # :101-106
        self.last_sampling_time = 0.0
        self.time, self.data = collections.deque(), collections.deque()
        self.average = np.zeros(2)

    def push_back(self, t, data):   # :113-135
        data = np.array(data, dtype=np.float64)
        if not self.time:
            self.time.append(t)
            self.data.append(data)
            self.average = data.copy()
            self.last_sampling_time = t
        elif t - self.last_sampling_time >= self.min_sampling_period:
            self.time.append(t)
            self.data.append(data)
            while t - self.time[0] > self.time_length:
                self.time.popleft()
                self.data.popleft()
            avg = np.zeros(2)
            for e in self.data:   # front to back
                avg = avg + e
            self.average = avg / len(self.data)
            self.last_sampling_time = t

    def size(self):
        return len(self.data)


class RaibertHeuristic:
    def __init__(self):
        self.period, self.gain, self.step_length = 0.0, 0.0, np.zeros(3)

    def set_parameters(self, period, gain):   # :38-47
        if period <= 0.0 or gain <= 0.0:
            raise ValueError("period and gain must be positive")
        self.period, self.gain = period, gain

    def plan_step_length(self, vcom, vcom_cmd, yaw_rate_cmd):   # :50-55
        vcom, vcom_cmd = np.asarray(vcom, dtype=np.float64), np.asarray(vcom_cmd, dtype=np.float64)
        self.step_length[:2] = self.period * vcom + (self.period * self.gain) * (vcom_cmd - vcom)


def rotation_from_quaternion(q):
    """Eigen::Quaterniond(w, x, y, z).toRotationMatrix() for q = (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def projection_norm(R):
    """what rotation.hpp:104 calls `norm`"""
    return R[0, 0] * R[0, 0] + R[0, 1] + R[0, 1]


def project_rotation_z(R, yaw_projection=False):
    R = np.array(R, dtype=np.float64)
    if yaw_projection:   # RTOC_PROJECT_YAW: the rotation about z by atan2(R10, R00)
        th = np.arctan2(R[1, 0], R[0, 0])
        R[0, 0], R[0, 1], R[1, 0], R[1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    else:   # rotation.hpp:103-111
        R = R / projection_norm(R)
    R[0, 2] = R[1, 2] = R[2, 0] = R[2, 1] = 0.0
    R[2, 2] = 1.0
    return R


def yaw_matrix(step_yaw):
    c, s = np.cos(step_yaw), np.sin(step_yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


class TrotFootStepPlanner:
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

    def set_gait_pattern(self, step_length, step_yaw, enable_stance_phase):   # :51-60
        self.step_length = np.array(step_length, dtype=np.float64)
        self.R_yaw = yaw_matrix(step_yaw)
        self.enable_stance_phase = bool(enable_stance_phase)
        self.enable_raibert_heuristic = False

    def set_raibert_gait_pattern(self, vcom_cmd, yaw_rate_cmd, swing_time, stance_time, gain):   # :63-88
        if swing_time <= 0.0 or stance_time < 0.0 or gain <= 0.0:
            raise ValueError("swing_time and gain must be positive, stance_time non-negative")
        period = 2.0 * (swing_time + stance_time)
        self.raibert_heuristic.set_parameters(period, gain)
        self.filter.set_parameters(period, 0.1 * period)
        self.vcom_cmd = np.array(vcom_cmd, dtype=np.float64)
        self.R_yaw = yaw_matrix(yaw_rate_cmd * (swing_time + stance_time))
        self.yaw_rate_cmd = yaw_rate_cmd
        self.enable_stance_phase = stance_time > 0.0
        self.enable_raibert_heuristic = True

    def init(self, q, feet, com):   # :91-106; feet [4, 3] and com at q
        R = project_rotation_z(rotation_from_quaternion(q[3:7]), self.yaw_projection)
        feet, com = np.asarray(feet, dtype=np.float64), np.asarray(com, dtype=np.float64)
        self.local = [R.T @ (feet[i] - com) for i in range(4)]
        self.contact_position_ref = []
        self.com_ref = [com.copy()]
        self.R_ = [R]
        self.filter.clear()
        self.current_step = 0

    def plan(self, t, feet, v, contact_status, planning_steps):   # :125-284; contact_status: bit k = contact k active
        assert planning_steps >= 0
        if self.enable_raibert_heuristic:   # :130-137
            vcom = np.asarray(v, dtype=np.float64)[:3]
            self.filter.push_back(t, vcom[:2])
            self.raibert_heuristic.plan_step_length(self.filter.average, self.vcom_cmd[:2], self.yaw_rate_cmd)
            self.step_length = self.raibert_heuristic.step_length.copy()
        cp = [np.array(feet[i], dtype=np.float64) for i in range(4)]   # :138-142
        act = [bool((contact_status >> i) & 1) for i in range(4)]
        com = np.zeros(3)
        R = self.R_[0]
        L, sl = self.local, self.step_length
        if all(act):   # :145-160
            if self.enable_stance_phase:
                if self.current_step % 2 != 0:
                    self.current_step += 1
            else:
                self.current_step = 0
            for i in range(4):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 4.0
        elif act[0] and act[3]:   # :161-181
            if (self.current_step % 4 != 1) if self.enable_stance_phase else (self.current_step % 2 != 1):
                self.current_step += 1
                R = self.R_yaw @ R
            for i in (0, 3):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[1] = com + R @ (L[1] - 0.5 * sl)
            cp[2] = com + R @ (L[2] - 0.5 * sl)
        elif act[1] and act[2]:   # :182-202
            if (self.current_step % 4 != 3) if self.enable_stance_phase else (self.current_step % 2 != 0):
                self.current_step += 1
                R = self.R_yaw @ R
            for i in (1, 2):
                com = com + cp[i]
                com = com - R @ L[i]
            com = com / 2.0
            cp[0] = com + R @ (L[0] - 0.5 * sl)
            cp[3] = com + R @ (L[3] - 0.5 * sl)
        else:
            return False
        self.com_ref = [com.copy()]   # :206-211
        self.contact_position_ref = [[p.copy() for p in cp]]
        self.R_ = [R.copy()]
        for step in range(self.current_step, planning_steps + self.current_step + 1):   # :212-277
            if step == 0:
                pass
            elif self.current_step == 0 and step == 1:   # :217-227, :250-260
                R = self.R_yaw @ R
                com = com + (0.5 if self.enable_raibert_heuristic else 0.25) * (R @ sl)
                cp[1], cp[2] = com + R @ L[1], com + R @ L[2]
            elif self.enable_stance_phase:   # :228-239
                if step % 4 == 1:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    cp[1], cp[2] = com + R @ L[1], com + R @ L[2]
                elif step % 4 == 3:
                    R = self.R_yaw @ R
                    com = com + 0.5 * (R @ sl)
                    cp[0], cp[3] = com + R @ L[0], com + R @ L[3]
            elif step % 2 == 1:   # :261-266
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[1], cp[2] = com + R @ L[1], com + R @ L[2]
            else:   # :267-272
                R = self.R_yaw @ R
                com = com + 0.5 * (R @ sl)
                cp[0], cp[3] = com + R @ L[0], com + R @ L[3]
            self.com_ref.append(com.copy())
            self.contact_position_ref.append([p.copy() for p in cp])
            self.R_.append(R.copy())
        self.planning_size = len(self.com_ref)
        return True

    def size(self):
        return self.planning_size

    def contact_positions(self, step):
        return np.array(self.contact_position_ref[step])

    def com(self, step):
        return self.com_ref[step]

    def R(self, step):
        return self.R_[step]


# ---- the MPC references.  positions [size, 4, 3], com [size, 3], R [size, 3, 3]: the plan; masks[phase]: the active contacts ----
def swing_foot_ref(positions, contact, masks, t, phase, swing_height, swing_start_time, period_swing, period_stance, num_phases_in_period):
    """(x3d_ref, isActive).  The reference leaves x3d_ref untouched where the reference is inactive (:92); the device writes
    contactPositions(phase) there, and so does this."""
    active = bool(t > swing_start_time and not (masks[phase] >> contact) & 1)   # :107-110
    if not active:
        return np.array(positions[phase][contact]), False
    period = period_swing + period_stance
    cycle = int(np.floor((t - swing_start_time) / period))   # :93
    rate = (t - swing_start_time - cycle * period) / period_swing   # :94
    x = (1.0 - rate) * positions[phase][contact] + rate * positions[phase + num_phases_in_period][contact]   # :95-96
    x[2] += 2 * rate * swing_height if rate < 0.5 else 2 * (1 - rate) * swing_height   # :97-102
    return x, True


def swing_rate(t, swing_start_time, period_swing, period_stance):
    period = period_swing + period_stance
    cycle = int(np.floor((t - swing_start_time) / period))
    return cycle, (t - swing_start_time - cycle * period) / period_swing


def com_ref(com, masks, t, phase, swing_start_time, period_active, period_inactive, num_phases_in_period):
    """(com_ref, isActive): updateRef's else branch where isActive is false (:100-102)"""
    active = bool(t > swing_start_time and (masks[phase] & 0xF) != 0xF)   # :106-108
    if not active:
        return np.array(com[phase]), False
    period = period_active + period_inactive
    cycle = int(np.floor((t - swing_start_time) / period))
    rate = (t - swing_start_time - cycle * period) / period_active
    return (1.0 - rate) * com[phase] + rate * com[phase + num_phases_in_period], True


def eigen_quaternion(m):
    """Eigen::Quaterniond(Matrix3d): Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>; (x, y, z, w)"""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def eigen_slerp(qa, t, qb):
    """QuaternionBase::slerp: the near-parallel branch and the sign flip of the shorter arc"""
    one = 1.0 - np.finfo(np.float64).eps
    d = float(qa @ qb)
    ad = abs(d)
    if ad >= one:
        s0, s1 = 1.0 - t, t
    else:
        theta = np.arccos(ad)
        s0, s1 = np.sin((1.0 - t) * theta) / np.sin(theta), np.sin(t * theta) / np.sin(theta)
    if d < 0:
        s1 = -s1
    return s0 * qa + s1 * qb


def configuration_ref(q, R, masks, t, phase, swing_start_time, period_active, period_inactive, num_phases_in_period):
    """(q_ref, isActive = True) (:92-115)"""
    q_ref = np.array(q, dtype=np.float64)
    if t > swing_start_time and (masks[phase] & 0xF) != 0xF:
        period = period_active + period_inactive
        cycle = int(np.floor((t - swing_start_time) / period))
        rate = (t - swing_start_time - cycle * period) / period_active
        q_ref[3:7] = eigen_slerp(eigen_quaternion(R[phase]), rate, eigen_quaternion(R[phase + num_phases_in_period]))
    else:
        q_ref[3:7] = eigen_quaternion(R[phase])
    return q_ref, True
