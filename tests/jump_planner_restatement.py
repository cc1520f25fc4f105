"""numpy restatement, line by line, of the reference's JumpFootStepPlanner and of the q_ref MPCJump::init makes of it -- the yardstick
of tests/test_jump_planner_*.py and tests/test_cpp_jump_foot_step_planner.py.  Line numbers are the reference's.

  JumpFootStepPlanner  src/mpc/jump_foot_step_planner.cpp:11-195 (constructor, setJumpPattern, init, plan, the getters)
  MPCJump::init        src/mpc/mpc_jump.cpp:141-145 (q_ref), :301-317 (resetContactPlacements: which step serves which phase)

project_rotation_z, rotation_from_quaternion, yaw_matrix and eigen_quaternion are those of tests/foot_step_planner_restatement.py.

The reference's Robot is Pinocchio: the planner takes the kinematics as arguments -- the frame placements and the centre of mass at
q, and the centre of mass at q_goal, which goal_configuration(q) returns so that the caller can evaluate it.  Parity of the planner
with the reference is therefore by restatement and unpinned.

Three things are NOT the reference's, as include/rtoc_robot.h (THE JUMP) states them: init starts com_ref_ over (the reference
pushes onto whatever a previous init left, :115-118); contact_positions / contact_surfaces are the two parts of contact_placements
for every foot (the reference keeps feet 0 and 1 alone, :110-113, :163-166); the model has exactly four point feet or exactly two
surfaces."""
import numpy as np

from foot_step_planner_restatement import eigen_quaternion, project_rotation_z, rotation_from_quaternion, yaw_matrix


class JumpFootStepPlanner:
    def __init__(self, is_biped, yaw_projection=False):
        self.is_biped = bool(is_biped)   # :25-31: fewer than four point contacts and at least two surfaces
        self.nfeet = 2 if is_biped else 4
        self.yaw_projection = yaw_projection
        self.current_step = 0
        self.placement_R, self.placement_p, self.com_ref, self.R_ = [], [], [], []
        self.jump_length, self.R_yaw = np.zeros(3), np.eye(3)

    def set_jump_pattern(self, jump_length, step_yaw):   # :43-49
        self.jump_length = np.array(jump_length, dtype=np.float64)
        self.R_yaw = yaw_matrix(step_yaw)

    def _rotations(self, q):
        R = project_rotation_z(rotation_from_quaternion(q[3:7]), self.yaw_projection)   # :69-70
        return R, self.R_yaw @ R   # :82

    def goal_configuration(self, q):   # :82-86
        q = np.asarray(q, dtype=np.float64)
        _, R_goal = self._rotations(q)
        q_goal = q.copy()
        q_goal[:3] += self.R_yaw @ self.jump_length
        q_goal[3:7] = eigen_quaternion(R_goal)   # Quaterniond(R_goal).coeffs(): not normalised
        return q_goal

    def init(self, q, feet, surfaces, com, com_goal):
        """:68-124; feet [nfeet, 3] and surfaces [nfeet, 3, 3]: the frame placements at q; com at q, com_goal at goal_configuration(q)"""
        q = np.asarray(q, dtype=np.float64)
        feet, surfaces = np.asarray(feet, dtype=np.float64), np.asarray(surfaces, dtype=np.float64)
        assert feet.shape == (self.nfeet, 3) and surfaces.shape == (self.nfeet, 3, 3)
        R, R_goal = self._rotations(q)
        local_R = [R.T @ surfaces[i] for i in range(self.nfeet)]            # :79
        local_p = [R.T @ (feet[i] - q[:3]) for i in range(self.nfeet)]      # :80
        hop = self.R_yaw @ self.jump_length
        goal_R = [R_goal @ local_R[i] for i in range(self.nfeet)]           # :91
        goal_p = [(q[:3] + R_goal @ local_p[i]) + hop for i in range(self.nfeet)]   # :92-93
        here_R = [surfaces[i].copy() for i in range(self.nfeet)]
        if not self.is_biped:   # :99-105
            here_R = [np.eye(3) for _ in range(self.nfeet)]
            goal_R = [np.eye(3) for _ in range(self.nfeet)]
        self.placement_R = [np.array(here_R), np.array(here_R), np.array(goal_R)]   # :95-98
        self.placement_p = [feet.copy(), feet.copy(), np.array(goal_p)]
        com, com_goal = np.array(com, dtype=np.float64), np.array(com_goal, dtype=np.float64)
        self.com_ref = [com.copy(), com.copy(), com_goal]   # :114-118, started over
        self.R_ = [R.copy(), R.copy(), R_goal]              # :119-122
        self.current_step = 0

    def q_ref(self, q):   # mpc_jump.cpp:141-145, between init and the first plan
        out = np.array(q, dtype=np.float64)
        out[:3] += self.com(2) - self.com(0)
        out[3:7] = eigen_quaternion(self.R(2))
        return out

    def plan(self, feet, surfaces, contact_status):
        """:127-170; feet, surfaces: the frame placements at this tick's q; contact_status: bit k = contact k active.  t, v and
        planning_steps are not read"""
        assert 0 <= contact_status < (1 << self.nfeet)
        if contact_status != 0:   # hasActiveContacts
            if self.current_step == 1:
                self.current_step = 2
            feet = np.asarray(feet, dtype=np.float64)
            if self.is_biped:   # :138-141
                self.placement_R[1] = np.array(surfaces, dtype=np.float64)
            self.placement_p[1] = feet.copy()   # :143-144
            self.placement_R[0], self.placement_p[0] = self.placement_R[1].copy(), self.placement_p[1].copy()   # :147
        elif self.current_step == 0:   # :150-158
            self.current_step = 1
            for seq in (self.placement_R, self.placement_p, self.com_ref, self.R_):
                seq[1] = seq[2]
                seq.pop()
        return True

    def size(self):
        return len(self.com_ref)   # :168

    def contact_positions(self, step):
        return self.placement_p[step]

    def contact_surfaces(self, step):
        return self.placement_R[step]

    def com(self, step):
        return self.com_ref[step]

    def R(self, step):
        return self.R_[step]


def placement_steps(current_step, nphases):
    """MPCJump::resetContactPlacements (mpc_jump.cpp:301-317): the plan step of every contact phase"""
    if current_step == 0:
        return [1, 2, 2][:nphases]
    if current_step == 1:
        return [1, 1][:nphases]
    return [1][:nphases]
