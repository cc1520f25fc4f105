"""Numpy restatement of TaskSpace6DCost (reference src/cost/task_space_6d_cost.cpp, include/robotoc/cost/task_space_6d_cost.hpp:
184-214) and of the per-grid-point reference tables, on the kinematics of tests/task_cost_restatement.py -- what
tests/test_task_space_6d_cost*.py hold the device kernel and robotoc_amd.costs against.

    X = X_ref^-1 oMf      d = log6(X)  [linear; angular]      JJ = Jlog6(X) J_frame (LOCAL)
    lq += s JJ^T W d      Qqq += s JJ^T W JJ                  cost += s/2 sum W d^2

Pinocchio is absent, so nothing compiled from the reference pins log6 / Jlog6 / getFrameJacobian: this file is pinned on the
CPU instead (test_task_space_6d_cost_host.py) -- log6 against oracle.rbd_log6, JJ and lq against central differences, the
linear rows against the 3D Jacobian.  log6 and Jlog6 are written in their closed forms (pinocchio/spatial/log.hxx), not in the
forward mode the device uses, so that the two share no arithmetic."""
import numpy as np

import task_cost_restatement as tr


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def log3(R):
    c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    if c < -0.99:
        # near pi the antisymmetric part vanishes: 4 q_i (q_x, q_y, q_z, q_w) of the quaternion of R, i the largest diagonal
        # entry, and w = 2 atan2(|v|, q_w) v / |v| (the scale drops out)
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
    k = 0.5 + th * th / 12.0 if th < 1e-6 else th / (2.0 * np.sin(th))
    return k * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


SERIES_T = 0.005  # below: the series of beta and beta' / t (truncated under 1e-22); above: their closed forms, which cancel like 1e-16 / t^3


def _beta(t):
    if t < 1e-3:
        return 1.0 / 12.0 + t * t / 720.0
    if t < SERIES_T:
        t2 = t * t
        return 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0
    return 1.0 / (t * t) - 1.0 / (2.0 * t * np.tan(0.5 * t))


def _bdot_t(t):
    """beta'(t) / t"""
    if t < 1e-3:
        return 1.0 / 360.0
    if t < SERIES_T:
        t2 = t * t
        return 1.0 / 360.0 + t2 / 7560.0 + t2 * t2 / 201600.0
    h = 0.5 * t
    return (-2.0 / t ** 3 + 1.0 / (2.0 * t * t * np.tan(h)) + 1.0 / (4.0 * t * np.sin(h) ** 2)) / t


def log6(R, p):
    """[linear; angular] of pinocchio::log6"""
    w = log3(R)
    t = np.linalg.norm(w)
    beta = _beta(t)
    alpha = 1.0 - beta * t * t
    return np.concatenate([alpha * p - 0.5 * np.cross(w, p) + beta * np.dot(w, p) * w, w])


def jlog3(w):
    t = np.linalg.norm(w)
    alpha = _beta(t)
    return alpha * np.outer(w, w) + (1.0 - t * t * alpha) * np.eye(3) + 0.5 * skew(w)


def jlog6(R, p):
    """d log6(X exp(xi)) / d xi at xi = 0 (pinocchio::Jlog6), 6 x 6 in [linear; angular] order"""
    w = log3(R)
    t = np.linalg.norm(w)
    A = jlog3(w)
    beta = _beta(t)
    bdot_t = _bdot_t(t)
    wp = np.dot(w, p)
    v = (bdot_t * wp) * w - (t * t * bdot_t + 2.0 * beta) * p
    Cm = np.outer(v, w) + beta * np.outer(w, p) + wp * beta * np.eye(3) + 0.5 * skew(p)
    J = np.zeros((6, 6))
    J[:3, :3] = J[3:, 3:] = A
    J[:3, 3:] = Cm @ A
    return J


def frame_placement(m, q, parent, frame_p, frame_R):
    """oMf = parent joint placement . (frame_R, frame_p)"""
    R, p = tr.placements(m, q)
    return R[parent] @ np.asarray(frame_R, dtype=float).reshape(3, 3), R[parent] @ np.asarray(frame_p, dtype=float) + p[parent]


def frame_jacobian_local(m, q, parent, frame_p, frame_R):
    """6 x nv: pinocchio::getFrameJacobian(..., LOCAL) -- column j = the frame's spatial velocity for a unit rate of dof j in the
    frame's own axes"""
    R, p = tr.placements(m, q)
    Rf, x = frame_placement(m, q, parent, frame_p, frame_R)
    J = np.zeros((6, m.nv))
    for j, (b, kind, ax) in enumerate(tr._dofs(m)):
        if parent not in tr._subtree(m, b):
            continue
        if kind == "lin":
            J[:3, j] = Rf.T @ (R[b] @ ax)
        else:
            w = R[b] @ ax
            J[:3, j], J[3:, j] = Rf.T @ np.cross(w, x - p[b]), Rf.T @ w
    return J


def diff(m, q, parent, frame_p, frame_R, R_ref, p_ref):
    """X = X_ref^-1 oMf as (R, p)"""
    Rf, x = frame_placement(m, q, parent, frame_p, frame_R)
    R_ref = np.asarray(R_ref, dtype=float).reshape(3, 3)
    return R_ref.T @ Rf, R_ref.T @ (x - np.asarray(p_ref, dtype=float))


def term6(m, q, parent, frame_p, frame_R, R_ref, p_ref):
    """(d [6], JJ [6, nv])"""
    XR, Xp = diff(m, q, parent, frame_p, frame_R, R_ref, p_ref)
    return log6(XR, Xp), jlog6(XR, Xp) @ frame_jacobian_local(m, q, parent, frame_p, frame_R)


def weights(s, kind):
    """the weights of grid kind 'stage' | 'impact' | 'terminal' in the order they multiply d: 3 of a 3D / CoM term, 6 of a 6D one"""
    lo = {"stage": s.weight, "impact": s.weight_impact, "terminal": s.weight_terminal}[kind][:]
    if s.kind != 2:
        return np.array(lo)
    hi = {"stage": s.weight_angular, "impact": s.weight_angular_impact, "terminal": s.weight_angular_terminal}[kind][:]
    return np.array(list(lo) + list(hi))


def term_value(m, q, s, t, kind, entry=None):
    """(active, d, JJ, W) of one rtoc_task_cost struct at configuration q; `entry` = the rtoc_task_ref_entry of this grid point for a
    RTOC_REF_TABLE term"""
    W = weights(s, kind)
    if not W.any():
        return False, None, None, W
    if s.ref_kind == 3:
        if not entry.active:
            return False, None, None, W
        R_ref, p_ref = np.array(entry.R[:]).reshape(3, 3), np.array(entry.p[:])
    else:
        R_ref, p_ref = np.array(s.ref_R[:]).reshape(3, 3), np.array(s.x0[:])
    if s.kind == 2:
        d, JJ = term6(m, q, s.frame_parent, s.frame_p[:], s.frame_R[:], R_ref, p_ref)
        return True, d, JJ, W
    if s.ref_kind == 3:
        if s.kind == 1:
            x, J = tr.com(m, q), tr.com_jacobian(m, q)
        else:
            x, J = tr.frame_position(m, q, s.frame_parent, s.frame_p[:]), tr.frame_jacobian(m, q, s.frame_parent, s.frame_p[:])
        return True, x - p_ref, J, W
    on, x, xr, J, W = tr.term_value(m, q, s, t, kind)
    return (True, x - xr, J, W) if on else (False, None, None, W)


def stage_terms(m, q, structs, t, kind, scale, entries=None):
    """what the terms add at one grid point: dlq [nv], dQqq [nv, nv], dhx [nv], dh, dcost, any_active; entries[k] = the table entry
    of term k at this grid point (terms with a table reference only).  hx / h are the contact path's STO sensitivities: the
    unconstrained path does not have them."""
    nv = m.nv
    lq, Q, hx, h, cost, any_on = np.zeros(nv), np.zeros((nv, nv)), np.zeros(nv), 0.0, 0.0, False
    for k, s in enumerate(structs):
        on, d, JJ, W = term_value(m, q, s, t, kind, None if entries is None else entries.get(k))
        if not on:
            continue
        any_on = True
        l = 0.5 * float(np.sum(W * d * d))
        g = JJ.T @ (W * d)
        lq += scale * g
        Q += scale * JJ.T @ (W[:, None] * JJ)
        cost += scale * l
        if kind == "stage":
            hx += g
            h += l
    return lq, Q, hx, h, cost, any_on


def random_rotation(rng, lo=0.0, hi=np.pi):
    """a rotation about a random axis by an angle drawn from [lo, hi]"""
    u = rng.normal(size=3)
    return tr._rot(u / np.linalg.norm(u), rng.uniform(lo, hi))


def reference_with_error(m, q, parent, frame_p, frame_R, rng, lo=0.1, hi=2.5, reach=0.5):
    """(R_ref, p_ref) such that X_ref^-1 oMf has a rotation angle drawn from [lo, hi] and a translation within `reach`"""
    Rf, x = frame_placement(m, q, parent, frame_p, frame_R)
    XR, Xp = random_rotation(rng, lo, hi), rng.uniform(-reach, reach, 3)
    R_ref = Rf @ XR.T
    return R_ref, x - R_ref @ Xp
