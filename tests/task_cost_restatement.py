"""Numpy restatement of the task-space cost components (TaskSpace3DCost, CoMCost; reference src/cost/task_space_3d_cost.cpp,
com_cost.cpp) and of their periodic references (periodic_swing_foot_ref.cpp, periodic_com_ref.cpp, the loops written out as
the reference writes them) -- what tests/test_task_space_cost*.py hold the device kernel and robotoc_amd.costs against.
Kinematics: the joint table of robotoc_amd.robot_model, body placements composed from the root; Jacobians from the tangent
convention of the contact rows (a free-flyer's translation and rotation local)."""
import numpy as np

from robotoc_amd import robot_model as rm


def _rot(axis, th):
    a = np.asarray(axis, dtype=float)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * np.outer(a, a)


def _quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def placements(m, q):
    """world (R, p) of every joint frame"""
    R, p = [None] * m.njoints, [None] * m.njoints
    for i in range(m.njoints):
        Rp, pp = np.array(m.placement_R[i]).reshape(3, 3), np.array(m.placement_p[i])
        iq = m.idx_q[i]
        if m.type[i] == rm.JOINT_FREE_FLYER:
            Rj, pj = _quat(q[iq + 3:iq + 7]), np.array(q[iq:iq + 3])
        else:
            Rj, pj = _rot(m.axis[i], q[iq]), np.zeros(3)
        Rl, pl = Rp @ Rj, Rp @ pj + pp
        par = m.parent[i]
        if par >= 0 and par != i:
            R[i], p[i] = R[par] @ Rl, p[par] + R[par] @ pl
        else:
            R[i], p[i] = Rl, pl
    return R, p


def _subtree(m, i):
    out = [i]
    for k in range(i + 1, m.njoints):
        a = m.parent[k]
        while a > i:
            a = m.parent[a]
        if a == i:
            out.append(k)
    return out


def _dofs(m):
    """per dof: (body, kind, axis in the body frame): kind 'lin' for a free-flyer translation, 'rot' otherwise"""
    out = []
    for i in range(m.njoints):
        if m.type[i] == rm.JOINT_FREE_FLYER:
            out += [(i, "lin", np.eye(3)[k]) for k in range(3)] + [(i, "rot", np.eye(3)[k]) for k in range(3)]
        else:
            out.append((i, "rot", np.array(m.axis[i])))
    return out


def frame_position(m, q, parent, offset):
    R, p = placements(m, q)
    return R[parent] @ np.asarray(offset, dtype=float) + p[parent]


def frame_jacobian(m, q, parent, offset):
    """3 x nv world-aligned linear Jacobian of the point `offset` of joint `parent`'s frame"""
    R, p = placements(m, q)
    x = R[parent] @ np.asarray(offset, dtype=float) + p[parent]
    J = np.zeros((3, m.nv))
    for j, (b, kind, ax) in enumerate(_dofs(m)):
        if parent not in _subtree(m, b):
            continue
        J[:, j] = R[b] @ ax if kind == "lin" else np.cross(R[b] @ ax, x - p[b])
    return J


def com(m, q):
    R, p = placements(m, q)
    M = sum(m.mass[i] for i in range(m.njoints))
    return sum(m.mass[i] * (R[i] @ np.array(m.com[i]) + p[i]) for i in range(m.njoints)) / M


def com_jacobian(m, q):
    R, p = placements(m, q)
    M = sum(m.mass[i] for i in range(m.njoints))
    c = [R[i] @ np.array(m.com[i]) + p[i] for i in range(m.njoints)]
    J = np.zeros((3, m.nv))
    for j, (b, kind, ax) in enumerate(_dofs(m)):
        sub = _subtree(m, b)
        msub = sum(m.mass[k] for k in sub)
        if kind == "lin":
            J[:, j] = msub / M * (R[b] @ ax)
        else:
            S = sum(m.mass[k] * c[k] for k in sub)
            J[:, j] = np.cross(R[b] @ ax, S - msub * p[b]) / M
    return J


# ---- the references, loop by loop ----
def foot_is_active(t, t0, period_swing, period_stance):
    period = period_swing + period_stance
    i = 0
    while True:
        if t < t0 + i * period:
            return False
        if t < t0 + i * period + period_swing:
            return True
        i += 1


def foot_ref(t, x3d0, step_length, step_height, t0, period_swing, period_stance, first_half):
    period = period_swing + period_stance
    x3d0, step_length = np.asarray(x3d0, dtype=float), np.asarray(step_length, dtype=float)
    if t < t0 + period_swing:
        rate = (t - t0) / period_swing
        x = x3d0 + (0.5 * rate if first_half else rate) * step_length
    else:
        i = 1
        while True:
            if t < t0 + i * period + period_swing:
                rate = (t - t0 - i * period) / period_swing
                x = x3d0 + ((i - 0.5 + rate) if first_half else (i + rate)) * step_length
                break
            i += 1
    x = x.copy()
    x[2] += (2 * rate if rate < 0.5 else 2 * (1 - rate)) * step_height
    return x


def com_is_active(t, t0, period_active, period_inactive):
    return foot_is_active(t, t0, period_active, period_inactive)


def com_ref(t, com_ref0, vcom_ref, t0, period_active, period_inactive, first_half):
    period = period_active + period_inactive
    com_ref0, vcom_ref = np.asarray(com_ref0, dtype=float), np.asarray(vcom_ref, dtype=float)
    if t < t0 + period_active:
        return com_ref0 + (0.5 * (t - t0) if first_half else (t - t0)) * vcom_ref
    i = 1
    while True:
        if t < t0 + i * period + period_active:
            t1 = t - t0 - i * period
            return com_ref0 + (((i - 0.5) * period_active + t1) if first_half else (i * period_active + t1)) * vcom_ref
        i += 1


def term_value(m, q, s, t, kind):
    """(active, x, x_ref, J, W) of one rtoc_task_cost struct `s` at configuration q, grid time t, grid kind
    'stage' | 'impact' | 'terminal'"""
    W = np.array({"stage": s.weight, "impact": s.weight_impact, "terminal": s.weight_terminal}[kind][:])
    if not W.any():
        return False, None, None, None, W
    if s.ref_kind == 1:
        if not foot_is_active(t, s.t0, s.period_active, s.period_inactive):
            return False, None, None, None, W
        xr = foot_ref(t, s.x0[:], s.rate[:], s.step_height, s.t0, s.period_active, s.period_inactive, s.first_half)
    elif s.ref_kind == 2:
        if not com_is_active(t, s.t0, s.period_active, s.period_inactive):
            return False, None, None, None, W
        xr = com_ref(t, s.x0[:], s.rate[:], s.t0, s.period_active, s.period_inactive, s.first_half)
    else:
        xr = np.array(s.x0[:])
    if s.kind == 1:
        x, J = com(m, q), com_jacobian(m, q)
    else:
        x, J = frame_position(m, q, s.frame_parent, s.frame_p[:]), frame_jacobian(m, q, s.frame_parent, s.frame_p[:])
    return True, x, xr, J, W


def stage_terms(m, q, structs, t, kind, scale):
    """what the task-space terms add at one grid point: dlq [nv], dQqq [nv, nv], dhx [nv], dh, dcost, any_active"""
    nv = m.nv
    lq, Q, hx, h, cost, any_on = np.zeros(nv), np.zeros((nv, nv)), np.zeros(nv), 0.0, 0.0, False
    for s in structs:
        on, x, xr, J, W = term_value(m, q, s, t, kind)
        if not on:
            continue
        any_on = True
        d = x - xr
        l = 0.5 * float(np.sum(W * d * d))
        g = J.T @ (W * d)
        lq += scale * g
        Q += scale * J.T @ (W[:, None] * J)
        cost += scale * l
        if kind == "stage":
            hx += g
            h += l
    return lq, Q, hx, h, cost, any_on
