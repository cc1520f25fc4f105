"""numpy restatement of SolutionInterpolator::interpolate (reference src/solver/solution_interpolator.cpp:30-113 with interpolate
:119-146, interpolatePartial :149-172, initEventSolution :175-198, modifyImpactSolution :201-208, modifyTerminalSolution :211-224) on
the packed SplitSolution records of RTOC_BUF_SOL -- the yardstick of rtoc_solution_interpolate.

Conventions of the packed records (those of robotoc_amd/host/robotoc_hip_planner.hpp: SolutionInterpolator, which wins where it
differs from the reference's text):
  * the f / mu stacks are compacted by the active contacts of their own grid point: each is expanded by the stored mask and
    re-packed by the new grid point's, 3 or 6 rows per contact; entries beyond the packed rows are zero
  * findStoredGridIndexBeforeTime steps back over stored points with dt <= 0; alpha is clamped to [0, 1]
  * a record is blended into a zeroed one: xi of a blended point and its padding are zero; a copy copies the whole record
  * at a copied impact the a | dv slot is zeroed as well (the reference keeps dv there)
  * q: joints linearly, a free-flyer base along the screw motion q1 (+) alpha (q2 (-) q1); the quaternion is that of the rotation
    matrix, w > 0 where the trace is positive (else the largest diagonal entry leads), normalised
Besides the records it returns, per new grid point, the set of branches taken (`BRANCHES`)."""
import numpy as np

GRID_INTERMEDIATE, GRID_IMPACT, GRID_LIFT, GRID_TERMINAL = 0, 1, 2, 3
FIELDS = ("q", "v", "a", "u", "f", "lmd", "gmm", "beta", "mu", "nu_passive", "xi")   # RTOC_SOL_*
BRANCHES = ("front", "back", "impact_matched", "xi_transfer", "lift_matched", "impact_event", "lift_event", "impact_partial",
            "lift_partial", "full", "partial", "stepped_back", "mask_differs")


def running_times(t0, dt):
    """t[0] = t0, t[i + 1] = t[i] + dt[i], summed in this order (what rtoc_solution_store / _interpolate form on the device)"""
    t = np.empty(len(dt))
    acc = float(t0)
    for i, d in enumerate(dt):
        t[i] = acc
        acc = acc + float(d)
    return t


def quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_quat(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0.0:
        s = np.sqrt(tr + 1.0) * 2.0
        q[:] = (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def log3(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    vee = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if c < -0.99:   # near pi: from the quaternion of R, the largest diagonal entry leading (the repaired log6)
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
    return (0.5 if th < 1e-10 else th / (2.0 * np.sin(th))) * vee


def exp_coefficients(w):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3 at t = |w|: the series below 1e-3, 2 sin^2(t/2) / t^2 above, where
    (1 - cos t) / t^2 would cancel like 1e-16 / t^2 (held to 50 digits by tests/test_lie_exp_branch_points_host.py)"""
    t2 = float(np.dot(w, w))
    t = np.sqrt(t2)
    if t < 1e-3:
        return 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    sh, s = np.sin(0.5 * t), np.sin(t)
    return s / t, 2.0 * sh * sh / t2, (t - s) / (t2 * t)


def exp3(w):
    K = skew(w)
    S, C, _ = exp_coefficients(w)
    return np.eye(3) + S * K + C * K @ K


def V_mat(w):   # exp6: p = V(w) v
    K = skew(w)
    _, C, B = exp_coefficients(w)
    return np.eye(3) + C * K + B * K @ K


def linear(a, b, alpha):
    return (1.0 - alpha) * a + alpha * b


def interpolate_configuration(q1, q2, alpha, floating, lerp=linear):
    """Robot::interpolateConfiguration = pinocchio::interpolate"""
    q = lerp(q1, q2, alpha)
    if floating:
        R1, R2 = quat_R(q1[3:7]), quat_R(q2[3:7])
        w = log3(R1.T @ R2)
        v = np.linalg.solve(V_mat(w), R1.T @ (q2[:3] - q1[:3]))
        q[:3] = q1[:3] + R1 @ (V_mat(alpha * w) @ (alpha * v))
        q[3:7] = R_quat(R1 @ exp3(alpha * w))
    return q


class Shape:
    """what of the problem the interpolation reads: the record layout (robotoc_amd.types.Layout) and the contacts' stack rows"""

    def __init__(self, L, contact_rows):
        d = L.dims
        self.nv, self.nu, self.np_, self.nf, self.ns = d.nv, d.nu, d.np, d.nf_max, d.ns_max
        self.floating = d.np == 6
        self.nq = d.nv + (1 if self.floating else 0)
        self.rows = [int(r) for r in contact_rows]
        self.off = {n: L.sol.off[i] for i, n in enumerate(FIELDS)}
        self.stride = L.sol.stride
        self.size = dict(q=self.nq, v=d.nv, a=d.nv, u=d.nu, f=d.nf_max, lmd=d.nv, gmm=d.nv, beta=d.nv, mu=d.nf_max, nu_passive=d.np,
                         xi=d.ns_max)

    def f(self, rec, name):
        return rec[self.off[name]:self.off[name] + self.size[name]]

    def expand(self, rec, mask, name):
        out, k, x = np.zeros((len(self.rows), 6)), 0, self.f(rec, name)
        for c, r in enumerate(self.rows):
            if (int(mask) >> c) & 1:
                out[c, :r] = x[k:k + r]
                k += r
        return out

    def put_stack(self, rec, mask, name, by_contact):
        x, k = self.f(rec, name), 0
        x[:] = 0.0
        for c, r in enumerate(self.rows):
            if (int(mask) >> c) & 1:
                x[k:k + r] = by_contact[c, :r]
                k += r


def interpolate(shape, types0, t0s, dt0, masks0, sol0, types1, t1s, masks1, blend_fn=linear):
    """types0 / t0s / dt0 / masks0 / sol0 [n0, stride]: the stored grid and solution; types1 / t1s / masks1: the grid to interpolate
    onto.  Returns (sol1 [n1, stride], branches: a set of BRANCHES names per new grid point).
    blend_fn(a, b, alpha) stands in for every linear blend (1 - alpha) a + alpha b: `classify` runs the same control flow with
    other functions to learn which entries are blends and what their operands were."""
    S, n0, n1 = shape, len(types0), len(types1)
    sol1 = np.zeros((n1, S.stride))
    branches = [set() for _ in range(n1)]

    def lerp(out, ra, rb, names, alpha):
        for name in names:
            S.f(out, name)[:] = blend_fn(S.f(ra, name), S.f(rb, name), alpha)

    def take(out, r, names):
        for name in names:
            S.f(out, name)[:] = S.f(r, name)

    def modify_impact(r):
        for name in ("u", "a", "nu_passive"):
            S.f(r, name)[:] = 0.0

    def blend(i, a, alpha, mode):
        b = a + 1
        ra, rb, out = sol0[a], sol0[b], sol1[i]
        S.f(out, "q")[:] = interpolate_configuration(S.f(ra, "q"), S.f(rb, "q"), alpha, S.floating, blend_fn)
        lerp(out, ra, rb, ("v", "lmd", "gmm"), alpha)
        fa, fb = S.expand(ra, masks0[a], "f"), S.expand(rb, masks0[b], "f")
        ma, mb = S.expand(ra, masks0[a], "mu"), S.expand(rb, masks0[b], "mu")
        if mode == "full":
            lerp(out, ra, rb, ("u", "a", "beta", "nu_passive"), alpha)
            act_b = np.array([(int(masks0[b]) >> c) & 1 for c in range(len(S.rows))], dtype=bool)[:, None]
            f_, mu_ = np.where(act_b, blend_fn(fa, fb, alpha), fa), np.where(act_b, blend_fn(ma, mb, alpha), ma)
        elif mode == "partial":
            take(out, ra, ("u", "a", "beta", "nu_passive"))
            f_, mu_ = fa, ma
        else:
            lerp(out, ra, rb, ("a",), alpha)
            take(out, rb, ("u", "beta", "nu_passive"))
            f_, mu_ = fb, mb
        S.put_stack(out, masks1[i], "f", f_)
        S.put_stack(out, masks1[i], "mu", mu_)
        if len(S.rows) and int(masks1[i]) != int(masks0[a]) and int(masks1[i]) != int(masks0[b]):
            branches[i].add("mask_differs")

    def copy(i, a):
        sol1[i][:] = sol0[a]
        S.put_stack(sol1[i], masks1[i], "f", S.expand(sol0[a], masks0[a], "f"))
        S.put_stack(sol1[i], masks1[i], "mu", S.expand(sol0[a], masks0[a], "mu"))

    def before(i, tt):
        k = 0
        while k + 1 < n0 and t0s[k + 1] <= tt:
            k += 1
        k = min(max(k, 0), n0 - 2)
        while k > 0 and dt0[k] <= 0.0:
            k -= 1
            branches[i].add("stepped_back")
        return k

    def stored_event(tt, kind):
        for k in range(n0 - 1):
            if types0[k] == kind and abs(t0s[k] - tt) < 1e-9:
                return k
        return -1

    def alpha_of(a, tt):
        return min(max((tt - t0s[a]) / dt0[a], 0.0), 1.0)

    for i in range(n1):
        tt, kind = t1s[i], types1[i]
        if tt <= t0s[0]:
            copy(i, 0)
            branches[i].add("front")
            continue
        if tt >= t0s[n0 - 1]:
            copy(i, n0 - 1)
            branches[i].add("back")
            continue
        if kind in (GRID_IMPACT, GRID_LIFT):
            name = "impact" if kind == GRID_IMPACT else "lift"
            k = stored_event(tt, kind)
            if k >= 0:
                copy(i, k)
                branches[i].add(name + "_matched")
                if kind == GRID_IMPACT:
                    modify_impact(sol1[i])
                    if i >= 2 and k >= 2:
                        S.f(sol1[i - 2], "xi")[:] = S.f(sol0[k - 2], "xi")
                        branches[i].add("xi_transfer")
                continue
            a = before(i, tt)
            if types0[a + 1] == GRID_TERMINAL:
                blend(i, a, alpha_of(a, tt), "partial")
                if kind == GRID_IMPACT:
                    modify_impact(sol1[i])
                branches[i].add(name + "_partial")
            else:
                blend(i, a, alpha_of(a, tt), "event")
                branches[i].add(name + "_event")
            continue
        a = before(i, tt)
        mode = "full" if types0[a + 1] == GRID_INTERMEDIATE else "partial"
        blend(i, a, alpha_of(a, tt), mode)
        branches[i].add(mode)
    for name in ("u", "a", "f", "beta", "mu", "nu_passive"):   # modifyTerminalSolution
        S.f(sol1[n1 - 1], name)[:] = 0.0
    return sol1, branches


LINEAR, POSE, EXACT = 1, 2, 0


def classify(shape, types0, t0s, dt0, masks0, sol0, types1, t1s, masks1):
    """(kind, operand) [n1, stride] of every entry interpolate writes: kind LINEAR for a linear blend with operand = max(|a|, |b|)
    of its two operands, POSE for the base position and quaternion of a blended record (operand 0), EXACT for what is copied or
    zeroed (operand 0)"""
    args = (shape, types0, t0s, dt0, masks0, sol0, types1, t1s, masks1)
    with np.errstate(invalid="ignore"):
        marked, _ = interpolate(*args, blend_fn=lambda a, b, alpha: np.full(np.shape(a), np.nan))
    operand, _ = interpolate(*args, blend_fn=lambda a, b, alpha: np.maximum(np.abs(a), np.abs(b)))
    kind = np.where(np.isnan(marked), LINEAR, EXACT)
    if shape.floating:
        o = shape.off["q"]
        for i in range(len(types1)):
            if kind[i, shape.off["v"]] == LINEAR:   # a blended record
                kind[i, o:o + 7] = POSE
    return kind, np.where(kind == LINEAR, operand, 0.0)
