"""SE(3) exponential, logarithm and their Jacobians at 50 digits (mpmath) -- the reference the committed fixtures
tests/golden/lie_branch_points.npz and tests/golden/lie_exp_branch_points.npz are generated from, and what every
double-precision copy of the log6 and of the exp6 formula in this repository (device, oracle, restatements, solver, planner
header) is held to.

Conventions are pinocchio's: a twist is [linear; angular], a placement X = (R, p), and Jlog6(X) is the derivative of
log6(X exp6(xi)) with respect to xi at 0.  A placement enters as a double quaternion (x, y, z, w) and a double position; the
log is that of the exact content of those doubles, the quaternion normalised at working precision.  The rotation vector is
w = 2 atan2(|v|, q_w) v / |v|, which is well conditioned on all of [0, pi]; the rotation matrix is never inverted."""
import mpmath as mp

mp.mp.dps = 50

PI = mp.pi


def _vec(x):
    return [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in x]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def norm(a):
    return mp.sqrt(dot(a, a))


def skew(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def quat_normalised(q):
    q = _vec(q)
    n = norm(q)
    return [c / n for c in q]


def quat_to_rotation(q):
    """rotation matrix of the (normalised) quaternion (x, y, z, w)"""
    x, y, z, w = quat_normalised(q)
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def exp3_quat(w):
    """unit quaternion (x, y, z, w) of exp3(w)"""
    w = _vec(w)
    t = norm(w)
    s = mp.mpf(1) / 2 if t == 0 else mp.sin(t / 2) / t
    return [s * w[0], s * w[1], s * w[2], mp.cos(t / 2)]


def exp3(w):
    return quat_to_rotation(exp3_quat(w))


def _AB(t):
    """(1 - cos t) / t^2 and (t - sin t) / t^3, through sin(t/2) and the series where the closed form cancels"""
    if t == 0:
        return mp.mpf(1) / 2, mp.mpf(1) / 6
    A = 2 * (mp.sin(t / 2) / t) ** 2
    if t < mp.mpf("1e-3"):
        B = sum((-1) ** k * t ** (2 * k) / mp.factorial(2 * k + 3) for k in range(12))
    else:
        B = (t - mp.sin(t)) / t ** 3
    return A, B


def exp6(xi):
    """(quaternion, position) of exp6([v; w]): rotation exp3(w), translation V(w) v"""
    xi = _vec(xi)
    v, w = xi[:3], xi[3:]
    A, B = _AB(norm(w))
    wxv = cross(w, v)
    wxwxv = cross(w, wxv)
    return exp3_quat(w), [v[k] + A * wxv[k] + B * wxwxv[k] for k in range(3)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def compose(qa, pa, qb, pb):
    """(qa, pa) (qb, pb)"""
    qa = quat_normalised(qa)
    Rp = quat_to_rotation(qa) * mp.matrix(_vec(pb))
    return quat_mul(qa, quat_normalised(qb)), [_vec(pa)[k] + Rp[k] for k in range(3)]


def log3_quat(q, sign=1):
    """rotation vector of the quaternion, angle in [0, pi]; at exactly pi both +-pi axis are logs: `sign` picks one"""
    x, y, z, w = quat_normalised(q)
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    v = [x, y, z]
    n = norm(v)
    if n == 0:
        return [mp.mpf(0)] * 3
    k = 2 * mp.atan2(n, w) / n
    if w == 0 and sign < 0:
        k = -k
    return [k * c for c in v]


def beta(t):
    """1/t^2 - cot(t/2) / (2 t), with its limit 1/12 at 0; the series below 1e-3 keeps the 50 digits the difference would lose"""
    if t == 0:
        return mp.mpf(1) / 12
    if t < mp.mpf("1e-3"):
        # -sum_{k>=1} B_2k t^(2k-2) / (2k)!  ... = 1/12 + t^2/720 + t^4/30240 + ...
        return sum(abs(mp.bernoulli(2 * k)) * t ** (2 * k - 2) / mp.factorial(2 * k) for k in range(1, 14))
    return 1 / t ** 2 - mp.cot(t / 2) / (2 * t)


def dbeta_over_t(t):
    """beta'(t) / t, limit 1/360"""
    if t < mp.mpf("1e-3"):
        return sum((2 * k - 2) * abs(mp.bernoulli(2 * k)) * t ** (2 * k - 4) / mp.factorial(2 * k) for k in range(2, 15))
    return (-2 / t ** 3 + mp.cot(t / 2) / (2 * t * t) + 1 / (4 * t * mp.sin(t / 2) ** 2)) / t


def log6(q, p, sign=1):
    """[V^-1 p; w] of the placement (quaternion, position)"""
    w = log3_quat(q, sign)
    p = _vec(p)
    b = beta(norm(w))
    wxp = cross(w, p)
    wxwxp = cross(w, wxp)
    return [p[k] - wxp[k] / 2 + b * wxwxp[k] for k in range(3)] + w


def jlog3(w):
    t = norm(w)
    b = beta(t)
    W = mp.matrix(w)
    return b * (W * W.T) + (1 - t * t * b) * mp.eye(3) + skew(w) / 2


def jlog6(q, p, sign=1):
    """6 x 6, [linear; angular] order: [[A, C A], [0, A]] with A = Jlog3(w) (pinocchio/spatial/log.hxx)"""
    w = log3_quat(q, sign)
    p = _vec(p)
    t = norm(w)
    b, bt = beta(t), dbeta_over_t(t)
    A = jlog3(w)
    wp = dot(w, p)
    W, P = mp.matrix(w), mp.matrix(p)
    v = (bt * wp) * W - (t * t * bt + 2 * b) * P
    Cm = v * W.T + b * (W * P.T) + wp * b * mp.eye(3) + skew(p) / 2
    J = mp.zeros(6, 6)
    CA = Cm * A
    for r in range(3):
        for c in range(3):
            J[r, c] = J[3 + r, 3 + c] = A[r, c]
            J[r, 3 + c] = CA[r, c]
    return J


def Ad(q, p):
    """action matrix of the placement on twists: [[R, [p]x R], [0, R]]"""
    R = quat_to_rotation(q)
    pR = skew(_vec(p)) * R
    M = mp.zeros(6, 6)
    for r in range(3):
        for c in range(3):
            M[r, c] = M[3 + r, 3 + c] = R[r, c]
            M[r, 3 + c] = pR[r, c]
    return M


def inverse(q, p):
    x, y, z, w = quat_normalised(q)
    qi = [-x, -y, -z, w]
    Rp = quat_to_rotation(qi) * mp.matrix(_vec(p))
    return qi, [-Rp[k] for k in range(3)]


def dq0_jacobian(q, p, sign=1):
    """-Jlog6(X) Ad_{X^-1}: the derivative of log6(M0^-1 M1) with respect to M0 (X = M0^-1 M1)"""
    qi, pi_ = inverse(q, p)
    return -jlog6(q, p, sign) * Ad(qi, pi_)


def jexp6(xi):
    """Jexp6(xi) = Jlog6(exp6(xi))^-1 (pinocchio's dIntegrate_dv on a free-flyer), for |w| < pi"""
    q, p = exp6(xi)
    return jlog6(q, p) ** -1


def ad_inv_exp6(xi):
    """Ad_{exp6(xi)}^-1 (pinocchio's dIntegrate_dq on a free-flyer)"""
    q, p = exp6(xi)
    return Ad(*inverse(q, p))


def rotation_to_quat(R):
    """unit quaternion (x, y, z, w) of a rotation matrix, the largest of the four components leading; q_w >= 0 up to that choice"""
    d = [R[0, 0], R[1, 1], R[2, 2]]
    tr = d[0] + d[1] + d[2]
    if tr > 0:
        s = 2 * mp.sqrt(1 + tr)
        return [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    i = max(range(3), key=lambda k: d[k])
    j, k = (i + 1) % 3, (i + 2) % 3
    s = 2 * mp.sqrt(1 + d[i] - d[j] - d[k])
    q = [mp.mpf(0)] * 4
    q[i], q[j], q[k], q[3] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q


def exp6_expm(xi):
    """(quaternion, position) of exp6([v; w]) by another road: mp.expm of the 4 x 4 twist matrix [[skew w, v], [0, 0]], ten
    digits over the working precision, its rotation block turned into a quaternion (sign as rotation_to_quat leaves it)"""
    xi = _vec(xi)
    with mp.workdps(mp.mp.dps + 10):
        T = mp.zeros(4, 4)
        K = skew(xi[3:])
        for r in range(3):
            for c in range(3):
                T[r, c] = K[r, c]
            T[r, 3] = xi[r]
        E = mp.expm(T)
        return rotation_to_quat(E), [E[r, 3] for r in range(3)]


def cond2(M):
    s = mp.svd_r(M, compute_uv=False)
    return max(s) / min(s)


def norm2(M):
    return max(mp.svd_r(M, compute_uv=False))


def to_float(x):
    """round to double: a list -> list of floats, a matrix -> nested lists"""
    if isinstance(x, mp.matrix):
        return [[float(x[r, c]) for c in range(x.cols)] for r in range(x.rows)]
    return [float(v) for v in x]
