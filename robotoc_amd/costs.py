"""TaskSpace3DCost and CoMCost with their periodic references, as a robotoc OCP declares them (reference
src/cost/task_space_3d_cost.cpp, com_cost.cpp, periodic_swing_foot_ref.cpp, periodic_com_ref.cpp): constructor argument
order, setters and argument checks of the reference.  The costs themselves are evaluated on the device by
rtoc_contact_eval_kkt (csrc/task_space_cost.hpp); these classes describe them (`to_struct`: one `rtoc_task_cost`) and
restate isActive / updateRef on the host for set-up and checks.

`robot` is a robotoc_amd.robot_model.RobotModel or the name of a bundled table ("anymal", "icub", ...).  A frame is a contact
frame name of the table (models/*.json contacts[].frame), a joint name with an offset in that joint's frame
(`("l_wrist_yaw", [0, 0, 0.1])`), or a (parent joint index, offset) pair.
"""
import ctypes as C
import json
import os

import numpy as np

from . import robot_model as rm

TASK_FRAME_3D, TASK_COM = 0, 1                          # RTOC_TASK_*
REF_CONST, REF_PERIODIC_FOOT, REF_PERIODIC_COM = 0, 1, 2  # RTOC_REF_*
MAX_TASK_COSTS = 8


class TaskCost(C.Structure):
    """include/rtoc_robot.h rtoc_task_cost"""
    _fields_ = [("kind", C.c_int), ("ref_kind", C.c_int), ("frame_parent", C.c_int), ("first_half", C.c_int),
                ("frame_p", C.c_double * 3), ("weight", C.c_double * 3), ("weight_terminal", C.c_double * 3),
                ("weight_impact", C.c_double * 3), ("x0", C.c_double * 3), ("rate", C.c_double * 3),
                ("step_height", C.c_double), ("t0", C.c_double), ("period_active", C.c_double), ("period_inactive", C.c_double)]


def resolve_frame(model_name, frame):
    """(parent joint index, origin in that joint's frame) of `frame` in the bundled table `model_name`"""
    d = json.load(open(os.path.join(rm.MODEL_DIR, model_name + ".json")))
    if isinstance(frame, str):
        for c in d["contacts"]:
            if c.get("frame") == frame:
                return int(c["parent"]), np.asarray(c["p"], dtype=float)
        raise ValueError("no contact frame named %r in %s" % (frame, model_name))
    name, offset = frame
    names = [j["name"] for j in d["joints"]]
    if name not in names:
        raise ValueError("no joint named %r in %s" % (name, model_name))
    return names.index(name), np.asarray(offset, dtype=float).reshape(3)


class PeriodicSwingFootRef:
    """src/cost/periodic_swing_foot_ref.cpp"""

    def __init__(self, x3d0, step_length, step_height, t0, period_swing, period_stance, is_first_step_half):
        self.set_foot_track_ref(x3d0, step_length, step_height, t0, period_swing, period_stance, is_first_step_half)

    def set_foot_track_ref(self, x3d0, step_length, step_height, t0, period_swing, period_stance, is_first_step_half):
        # no checks here, as in the reference; rtoc_set_task_costs refuses period_swing <= 0 or period_stance < 0
        self.x3d0 = np.asarray(x3d0, dtype=float).reshape(3).copy()
        self.step_length = np.asarray(step_length, dtype=float).reshape(3).copy()
        self.step_height, self.t0 = float(step_height), float(t0)
        self.period_swing, self.period_stance = float(period_swing), float(period_stance)
        self.period = self.period_swing + self.period_stance
        self.is_first_step_half = bool(is_first_step_half)

    def update_ref(self, t):
        if t < self.t0 + self.period_swing:
            rate = (t - self.t0) / self.period_swing
            x = self.x3d0 + ((0.5 * rate) if self.is_first_step_half else rate) * self.step_length
        else:
            i = 1
            while not t < self.t0 + i * self.period + self.period_swing:
                i += 1
            rate = (t - self.t0 - i * self.period) / self.period_swing
            x = self.x3d0 + ((i - 0.5 + rate) if self.is_first_step_half else (i + rate)) * self.step_length
        x[2] += (2 * rate if rate < 0.5 else 2 * (1 - rate)) * self.step_height
        return x

    def is_active(self, t):
        i = 0
        while True:
            if t < self.t0 + i * self.period:
                return False
            if t < self.t0 + i * self.period + self.period_swing:
                return True
            i += 1

    def _fill(self, s):
        s.ref_kind, s.first_half = REF_PERIODIC_FOOT, int(self.is_first_step_half)
        s.x0[:], s.rate[:] = self.x3d0, self.step_length
        s.step_height, s.t0, s.period_active, s.period_inactive = self.step_height, self.t0, self.period_swing, self.period_stance


class PeriodicCoMRef:
    """src/cost/periodic_com_ref.cpp"""

    def __init__(self, com_ref0, vcom_ref, t0, period_active, period_inactive, is_first_move_half):
        self.set_com_ref(com_ref0, vcom_ref, t0, period_active, period_inactive, is_first_move_half)

    def set_com_ref(self, com_ref0, vcom_ref, t0, period_active, period_inactive, is_first_move_half):
        # no checks here, as in the reference; rtoc_set_task_costs refuses period_active <= 0 or period_inactive < 0
        self.com_ref0 = np.asarray(com_ref0, dtype=float).reshape(3).copy()
        self.vcom_ref = np.asarray(vcom_ref, dtype=float).reshape(3).copy()
        self.t0, self.period_active, self.period_inactive = float(t0), float(period_active), float(period_inactive)
        self.period = self.period_active + self.period_inactive
        self.is_first_move_half = bool(is_first_move_half)

    def update_ref(self, t):
        if t < self.t0 + self.period_active:
            tau = 0.5 * (t - self.t0) if self.is_first_move_half else (t - self.t0)
        else:
            i = 1
            while not t < self.t0 + i * self.period + self.period_active:
                i += 1
            t1 = t - self.t0 - i * self.period
            tau = ((i - 0.5) * self.period_active + t1) if self.is_first_move_half else (i * self.period_active + t1)
        return self.com_ref0 + tau * self.vcom_ref

    def is_active(self, t):
        i = 0
        while True:
            if t < self.t0 + i * self.period:
                return False
            if t < self.t0 + i * self.period + self.period_active:
                return True
            i += 1

    def _fill(self, s):
        s.ref_kind, s.first_half = REF_PERIODIC_COM, int(self.is_first_move_half)
        s.x0[:], s.rate[:] = self.com_ref0, self.vcom_ref
        s.step_height, s.t0, s.period_active, s.period_inactive = 0.0, self.t0, self.period_active, self.period_inactive


class _Cost3D:
    _name = ""

    def __init__(self, ref=None):
        self.weight, self.weight_terminal, self.weight_impact = np.zeros(3), np.zeros(3), np.zeros(3)
        self.const_ref, self.ref = np.zeros(3), None
        if ref is None:
            pass
        elif isinstance(ref, (PeriodicSwingFootRef, PeriodicCoMRef)):
            self.set_ref(ref)
        else:
            self.set_const_ref(ref)

    def _check(self, w, what):
        w = np.asarray(w, dtype=float).reshape(3)
        if w.min() < 0.0:
            raise ValueError("[%s] invalid argument: elements of '%s' must be non-negative!" % (self._name, what))
        return w.copy()

    def set_weight(self, weight):
        self.weight = self._check(weight, "weight")

    def set_weight_terminal(self, weight_terminal):
        self.weight_terminal = self._check(weight_terminal, "weight_terminal")

    def set_weight_impact(self, weight_impact):
        self.weight_impact = self._check(weight_impact, "weight_impact")

    def set_ref(self, ref):
        self.ref = ref

    def set_const_ref(self, const_ref):
        self.const_ref, self.ref = np.asarray(const_ref, dtype=float).reshape(3).copy(), None

    def is_cost_active(self, t):
        return True if self.ref is None else self.ref.is_active(t)

    def reference(self, t):
        """x_ref at grid time t (only meaningful where is_cost_active)"""
        return self.const_ref.copy() if self.ref is None else self.ref.update_ref(t)

    def to_struct(self):
        s = TaskCost()
        s.weight[:], s.weight_terminal[:], s.weight_impact[:] = self.weight, self.weight_terminal, self.weight_impact
        if self.ref is None:
            s.ref_kind, s.x0[:] = REF_CONST, self.const_ref
        else:
            self.ref._fill(s)
        return s


class TaskSpace3DCost(_Cost3D):
    """src/cost/task_space_3d_cost.cpp: TaskSpace3DCost(robot, frame[, ref | const_ref])"""
    _name = "TaskSpace3DCost"

    def __init__(self, robot, frame, ref=None):
        if isinstance(frame, tuple) and len(frame) == 2 and isinstance(frame[0], (int, np.integer)):
            parent, p = int(frame[0]), np.asarray(frame[1], dtype=float).reshape(3)
        else:
            if not isinstance(robot, str):
                raise ValueError("[TaskSpace3DCost] a frame given by name needs the name of a bundled model table")
            parent, p = resolve_frame(robot, frame)
        self.frame_parent, self.frame_p = parent, p
        super().__init__(ref)

    def to_struct(self):
        s = super().to_struct()
        s.kind, s.frame_parent, s.frame_p[:] = TASK_FRAME_3D, self.frame_parent, self.frame_p
        return s


class CoMCost(_Cost3D):
    """src/cost/com_cost.cpp: CoMCost(robot[, ref | const_ref])"""
    _name = "CoMCost"

    def __init__(self, robot, ref=None):
        super().__init__(ref)

    def to_struct(self):
        s = super().to_struct()
        s.kind = TASK_COM
        return s
