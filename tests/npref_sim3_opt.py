"""Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091) restated in numpy / float64 from the reference's and g2o's text: g2o::Sim3
(ThirdParty/g2o/g2o/types/sim3.h), VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69), the two Sim3 edges
(include/g2o_cubemap_vertices_edges.h:137-209, multipinhole_project src/g2o_cubemap_vertices_edges.cpp:279-287), the numeric linearizeOplus and
the robust quadratic form of core/base_binary_edge.hpp, RobustKernelHuber, and OptimizationAlgorithmLevenberg::solve
(core/optimization_algorithm_levenberg.cpp:61-164).  Eigen's small fixed-size expressions are written out in the order Eigen evaluates them.

Where the project had to choose (DESIGN.md "OptimizeSim3") this file states the choice again on its own: the sums of a pass go through
CMS_SIM3_OPT_SLOTS slots and one pairwise tree, the 7 x 7 system is solved by an unpivoted LDL^T, pow(2 rho - 1, 3) is the cube.  exp / sin / cos
are injectable: libm's by default, the core's own through the probes for the bit-for-bit comparisons.  Edge passes are vectorised over the
pairs (every pair sees the same operations in the same order as one after the other)."""
import math

import numpy as np

SLOTS = 256
f64 = np.float64
LIBM = dict(exp=math.exp, sin=math.sin, cos=math.cos)


# ---- Eigen pieces
def quat_from_R(m):
    """Eigen::Quaterniond(Matrix3d) -> x y z w"""
    m = np.asarray(m, f64).reshape(3, 3)
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
        return q
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j = (i + 1) % 3; k = (j + 1) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[k, j] - m[j, k]) * t
    q[j] = (m[j, i] + m[i, j]) * t
    q[k] = (m[k, i] + m[i, k]) * t
    return q


def rotate(q, v):
    """Quaternion * Vector3 (Eigen's _transformVector): uv = vec x v; uv += uv; v + w uv + vec x uv.  v: (..., 3)"""
    x, y, z, w = q
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0 = y * v2 - z * v1; u1 = z * v0 - x * v2; u2 = x * v1 - y * v0
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2
    c0 = y * u2 - z * u1; c1 = z * u0 - x * u2; c2 = x * u1 - y * u0
    return np.stack([(v0 + w * u0) + c0, (v1 + w * u1) + c1, (v2 + w * u2) + c2], -1)


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_to_R(q):
    """Eigen's toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


# ---- g2o::Sim3 as (q xyzw, t, s)
def sim3_from_Rts(R, t, s):
    return quat_from_R(R), np.array(t, f64).copy(), f64(s)


def sim3_exp(update, fn=LIBM):
    """Sim3(const Vector7d& update), sim3.h:70-142"""
    u = np.asarray(update, f64)
    omega = u[0:3]; upsilon = u[3:6]; sigma = u[6]
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Omega = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]], f64)
    s = f64(fn["exp"](float(sigma)))
    Omega2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            Omega2[i, j] = Omega[i, 0] * Omega[0, j] + Omega[i, 1] * Omega[1, j] + Omega[i, 2] * Omega[2, j]
    I = np.eye(3)
    eps = 0.00001
    with np.errstate(all="ignore"):
        if abs(sigma) < eps:
            C = f64(1)
            if theta < eps:
                A = f64(1. / 2.); B = f64(1. / 6.)
                R = (I + Omega) + Omega2
            else:
                sn = f64(fn["sin"](float(theta))); cs = f64(fn["cos"](float(theta)))
                theta2 = theta * theta
                A = (1 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
                R = (I + sn / theta * Omega) + (1 - cs) / (theta * theta) * Omega2
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = (I + Omega) + Omega2
            else:
                sn = f64(fn["sin"](float(theta))); cs = f64(fn["cos"](float(theta)))
                R = (I + sn / theta * Omega) + (1 - cs) / (theta * theta) * Omega2
                a = s * sn; b = s * cs
                theta2 = theta * theta; sigma2 = sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        W = (A * Omega + B * Omega2) + C * I
        t = np.array([W[i, 0] * upsilon[0] + W[i, 1] * upsilon[1] + W[i, 2] * upsilon[2] for i in range(3)])
    return quat_from_R(R), t, s


def sim3_map(S, xyz):
    q, t, s = S
    return s * rotate(q, np.asarray(xyz, f64)) + t


def sim3_inverse(S):
    q, t, s = S
    qc = np.array([-q[0], -q[1], -q[2], q[3]])
    return qc, rotate(qc, (-1. / s) * t), 1. / s


def sim3_times(a, b):
    """operator*: ret.r = r * other.r; ret.t = s * (r * other.t) + t; ret.s = s * other.s (no renormalisation)"""
    return quat_mul(a[0], b[0]), a[2] * rotate(a[0], b[1]) + a[1], a[2] * b[2]


def oplus(S, update, fix_scale, fn=LIBM):
    """VertexSim3Expmap::oplusImpl: update[6] is zeroed IN the caller's array under _fix_scale"""
    if fix_scale:
        update[6] = 0
    return sim3_times(sim3_exp(update, fn), S)


# ---- the camera
def face_in_cubemap(F, x, y):
    """FaceInCubemap(cv::Point2f): double i = pixel.x / mWCubeFace with a float quotient.  0 front, 1 left, 2 right, 3 upper, 4 lower, -1 unknown"""
    i = (np.asarray(x, np.float32) / np.float32(F)).astype(f64); j = (np.asarray(y, np.float32) / np.float32(F)).astype(f64)
    face = np.full(i.shape, -1, np.int32)
    for f, (a, b) in ((2, (2, 1)), (4, (1, 2)), (0, (1, 1)), (3, (1, 0)), (1, (0, 1))):      # later entries win: written in reverse of the if / else chain
        face[(i >= a) & (i < a + 1) & (j >= b) & (j < b + 1)] = f
    return face


def pos_in_face(F, uc):
    """GetPosInFace<double>: u - floor(u / F) * F"""
    u = np.asarray(uc, np.float32).astype(f64)
    return u - np.floor(u / F).astype(np.int64) * F


def face_local(face, X):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    l = np.zeros(X.shape)
    for f, (a, b, c) in enumerate(((x, y, z), (z, y, -x), (-z, y, x), (x, z, -y), (x, -z, y))):
        m = face == f
        l[m, 0] = a[m]; l[m, 1] = b[m]; l[m, 2] = c[m]
    return l


def project(F, face, y, narrow=True):
    """multipinhole_project: cv::Vec3f of the point, `_x * fx / _z + cx` in double, float u, v.  narrow=False: the double projection"""
    f = F / 2.0
    with np.errstate(all="ignore"):
        if narrow:
            y = y.astype(np.float32).astype(f64)
        l = face_local(face, y)
        u = l[:, 0] * f / l[:, 2] + f; v = l[:, 1] * f / l[:, 2] + f
        if narrow:
            u = u.astype(np.float32).astype(f64); v = v.astype(np.float32).astype(f64)
    return np.stack([u, v], 1)


def make_pairs(F, prob):
    """The graph of :939-1028 over the kept correspondences"""
    kp1 = np.asarray(prob["kp1"], np.float32).reshape(-1, 2); kp2 = np.asarray(prob["kp2"], np.float32).reshape(-1, 2)
    return dict(X1=np.asarray(prob["x3dc1"], np.float32).reshape(-1, 3).astype(f64), X2=np.asarray(prob["x3dc2"], np.float32).reshape(-1, 3).astype(f64),
                face1=face_in_cubemap(F, kp1[:, 0], kp1[:, 1]), face2=face_in_cubemap(F, kp2[:, 0], kp2[:, 1]),
                m1=np.stack([pos_in_face(F, kp1[:, 0]), pos_in_face(F, kp1[:, 1])], 1), m2=np.stack([pos_in_face(F, kp2[:, 0]), pos_in_face(F, kp2[:, 1])], 1),
                om1=np.asarray(prob["inv_sigma2_1"], np.float32).astype(f64), om2=np.asarray(prob["inv_sigma2_2"], np.float32).astype(f64))


def errors(F, P, S, narrow=True):
    """computeError of both edge kinds -> (e12, e21), N x 2 each"""
    e12 = P["m1"] - project(F, P["face1"], sim3_map(S, P["X2"]), narrow)
    e21 = P["m2"] - project(F, P["face2"], sim3_map(sim3_inverse(S), P["X1"]), narrow)
    return e12, e21


def numeric_jacobians(F, P, S, fix_scale, fn=LIBM, delta=1e-9, narrow=True):
    """BaseBinaryEdge::linearizeOplus for the Sim3 vertex (the point vertex is fixed) -> (J12, J21), N x 2 x 7"""
    scalar = 1.0 / (2 * delta)
    n = len(P["X1"])
    J12 = np.zeros((n, 2, 7)); J21 = np.zeros((n, 2, 7))
    add = np.zeros(7)
    for d in range(7):
        add[d] = delta
        ep = errors(F, P, oplus(S, add, fix_scale, fn), narrow)
        add[d] = -delta
        em = errors(F, P, oplus(S, add, fix_scale, fn), narrow)
        add[d] = 0.0
        J12[:, :, d] = scalar * (ep[0] - em[0]); J21[:, :, d] = scalar * (ep[1] - em[1])
    return J12, J21


def _jpi(F, face, y):
    """2 x 3 derivative of the double face projection in the camera frame"""
    f = F / 2.0
    l = face_local(face, y)
    g0 = f / l[:, 2]; g02 = -(f * l[:, 0]) / (l[:, 2] * l[:, 2]); g12 = -(f * l[:, 1]) / (l[:, 2] * l[:, 2])
    z = np.zeros(len(y))
    Jc = np.zeros((len(y), 2, 3))
    rows = {0: ((g0, z, g02), (z, g0, g12)), 1: ((-g02, z, g0), (-g12, g0, z)), 2: ((g02, z, -g0), (g12, g0, z)),
            3: ((g0, -g02, z), (z, -g12, g0)), 4: ((g0, g02, z), (z, g12, -g0))}
    for fc, r in rows.items():
        m = face == fc
        for i in range(2):
            for j in range(3):
                Jc[m, i, j] = r[i][j][m]
    return Jc


def _jac_rows(M, p, sgn):
    """sgn * M [ -[p]x | I | p ], per pair"""
    J = np.zeros((len(p), 2, 7))
    for i in range(2):
        m0, m1, m2 = M[:, i, 0], M[:, i, 1], M[:, i, 2]
        J[:, i, 0] = sgn * (m2 * p[:, 1] - m1 * p[:, 2])
        J[:, i, 1] = sgn * (m0 * p[:, 2] - m2 * p[:, 0])
        J[:, i, 2] = sgn * (m1 * p[:, 0] - m0 * p[:, 1])
        J[:, i, 3] = sgn * m0; J[:, i, 4] = sgn * m1; J[:, i, 5] = sgn * m2
        J[:, i, 6] = sgn * ((m0 * p[:, 0] + m1 * p[:, 1]) + m2 * p[:, 2])
    return J


def analytic_jacobians(F, P, S, fix_scale):
    """For S <- exp(u) S: de12/du = -Jpi(S X2) [ -[y]x | I | y ], de21/du = +Jpi(S^-1 X1) (1/s) R^T [ -[X1]x | I | X1 ]"""
    with np.errstate(all="ignore"):
        y = sim3_map(S, P["X2"])
        J12 = _jac_rows(_jpi(F, P["face1"], y), y, -1.0)
        y = sim3_map(sim3_inverse(S), P["X1"])
        Jc = _jpi(F, P["face2"], y)
        R = quat_to_R(S[0]); inv_s = 1.0 / S[2]
        M = np.zeros((len(y), 2, 3))
        for i in range(2):
            for j in range(3):
                M[:, i, j] = (Jc[:, i, 0] * (inv_s * R[j, 0]) + Jc[:, i, 1] * (inv_s * R[j, 1])) + Jc[:, i, 2] * (inv_s * R[j, 2])
        J21 = _jac_rows(M, P["X1"], 1.0)
    if fix_scale:
        J12[:, :, 6] = 0; J21[:, :, 6] = 0
    return J12, J21


# ---- the quadratic form
def chi2(om, e):
    """_error.dot(information() * _error), information = om * I"""
    return e[:, 0] * (om * e[:, 0]) + e[:, 1] * (om * e[:, 1])


def huber(e2, delta):
    """RobustKernelHuber::robustify -> rho[0], rho[1]"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        big = ~(e2 <= dsqr)
        return np.where(big, 2 * sq * delta - dsqr, e2), np.where(big, delta / sq, 1.0)


def tree(s):
    """The fold of the slots (s: SLOTS x W): inside every group of 64, s[i] += s[i + o] for o = 32 ... 1; then (g0 + g1) + (g2 + g3)"""
    s = np.array(s, f64).reshape(SLOTS, -1).copy()
    for g in range(0, SLOTS, 64):
        o = 32
        while o > 0:
            s[g:g + o] = s[g:g + o] + s[g + o:g + 2 * o]
            o >>= 1
    return (s[0] + s[64]) + (s[128] + s[192])


def slot_sum(terms, active):
    """terms: list of N x W arrays, one per edge kind in the order the edges of a pair are visited; pair k adds into slot k mod SLOTS, ascending k"""
    n = len(active); W = terms[0].shape[1]
    slots = np.zeros((SLOTS, W))
    with np.errstate(all="ignore"):
        for c in range(0, n, SLOTS):
            sel = np.nonzero(active[c:c + SLOTS])[0]
            for t in terms:
                slots[sel] = slots[sel] + t[c + sel]
    return tree(slots)


def edge_terms(J, e, om, delta):
    """constructQuadraticForm with the Huber kernel: [28 H upper triangle row by row | 7 b | rho0] per edge"""
    with np.errstate(all="ignore"):
        rho0, w = huber(chi2(om, e), delta)
        ow = w * om
        r0 = -(om * e[:, 0]) * w; r1 = -(om * e[:, 1]) * w
        out = np.zeros((len(om), 36))
        k = 0
        for i in range(7):
            for j in range(i, 7):
                out[:, k] = (J[:, 0, i] * ow) * J[:, 0, j] + (J[:, 1, i] * ow) * J[:, 1, j]
                k += 1
        for i in range(7):
            out[:, 28 + i] = J[:, 0, i] * r0 + J[:, 1, i] * r1
        out[:, 35] = rho0
    return out


def solve7(H, b, lam):
    """Unpivoted dense LDL^T of (H + lam I) x = b -> (ok, x); ok False on a zero or non-finite pivot"""
    A = np.array(H, f64).reshape(7, 7).copy()
    for i in range(7):
        A[i, i] += lam
    D = np.zeros(7); RD = np.zeros(7)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(7):
            d = A[j, j]
            for k in range(j):
                d -= A[j, k] * A[j, k] * D[k]
            if not np.isfinite(d) or d == 0.0:
                ok = False
            D[j] = d
            rd = 1.0 / d
            RD[j] = rd
            for i in range(j + 1, 7):
                s = A[i, j]
                for k in range(j):
                    s -= A[i, k] * A[j, k] * D[k]
                A[i, j] = s * rd
        x = np.array(b, f64).copy()
        for i in range(7):
            for k in range(i):
                x[i] -= A[i, k] * x[k]
        for i in range(7):
            x[i] *= RD[i]
        for i in range(6, -1, -1):
            for k in range(i + 1, 7):
                x[i] -= A[k, i] * x[k]
    return ok, x


class Graph:
    def __init__(self, F, prob, th2, fix_scale, jacobian, fn):
        self.F = F; self.P = make_pairs(F, prob); self.n = len(self.P["X1"])
        self.fix_scale = bool(fix_scale); self.jacobian = int(jacobian); self.fn = fn
        self.delta = f64(np.float32(np.sqrt(f64(np.float32(th2)))))      # const float deltaHuber = sqrt(th2)
        self.active = np.ones(self.n, bool)
        self.e12 = np.zeros((self.n, 2)); self.e21 = np.zeros((self.n, 2))      # the edges' persistent _error
        self.S = None
        self.lam = 0.0; self.ni = 2.0; self.n_bad_it = 0

    def compute_errors(self, S):
        self.e12, self.e21 = errors(self.F, self.P, S)

    def robust_chi2(self):
        a, _ = huber(chi2(self.P["om1"], self.e12), self.delta); b, _ = huber(chi2(self.P["om2"], self.e21), self.delta)
        return slot_sum([a[:, None], b[:, None]], self.active)[0]

    def build_system(self):
        if self.jacobian == 0:
            J12, J21 = numeric_jacobians(self.F, self.P, self.S, self.fix_scale, self.fn)      # _error is restored afterwards
        else:
            J12, J21 = analytic_jacobians(self.F, self.P, self.S, self.fix_scale)
        self.J12, self.J21 = J12, J21
        return slot_sum([edge_terms(J12, self.e12, self.P["om1"], self.delta), edge_terms(J21, self.e21, self.P["om2"], self.delta)], self.active)

    def solve(self, iteration):
        """OptimizationAlgorithmLevenberg::solve -> True = OK, False = Terminate"""
        self.compute_errors(self.S)
        sums = self.build_system()
        currentChi = sums[35]      # activeRobustChi2 of the same errors through the same slots and tree
        iniChi = currentChi
        H = np.zeros((7, 7)); k = 0
        for i in range(7):
            for j in range(i, 7):
                H[i, j] = sums[k]; H[j, i] = sums[k]; k += 1
        b = sums[28:35].copy()
        if iteration == 0:
            self.lam = _lambda_init(H)
            self.ni = 2.0; self.n_bad_it = 0
        rho = 0.0; qmax = 0
        with np.errstate(all="ignore"):
            while True:
                backup = self.S
                ok2, x = solve7(H, b, self.lam)
                if not ok2:
                    x = np.zeros(7)
                self.S = oplus(backup, x, self.fix_scale, self.fn)
                self.compute_errors(self.S)
                tempChi = self.robust_chi2()
                if not ok2:
                    tempChi = f64(np.finfo(f64).max)
                scale = f64(0.0)
                for j in range(7):
                    scale += x[j] * (self.lam * x[j] + b[j])
                rho = (currentChi - tempChi) / (scale + 1e-3)
                if rho > 0 and np.isfinite(tempChi):
                    t21 = 2 * rho - 1
                    alpha = 1. - t21 * t21 * t21
                    alpha = min(alpha, 2. / 3.)
                    self.lam *= max(1. / 3., alpha)
                    self.ni = 2.0
                    currentChi = tempChi
                else:
                    self.lam *= self.ni
                    self.ni *= 2
                    self.S = backup
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                return False
            if (iniChi - currentChi) * 1e3 < iniChi:
                self.n_bad_it += 1
            else:
                self.n_bad_it = 0
        return self.n_bad_it < 3

    def optimize(self, iterations):
        if not self.active.any():
            return 0
        done = 0
        for it in range(iterations):
            ok = self.solve(it)
            done += 1
            if not ok:
                break
        return done

    def classify(self, th2):
        with np.errstate(all="ignore"):
            bad = self.active & ((chi2(self.P["om1"], self.e12) > f64(np.float32(th2))) | (chi2(self.P["om2"], self.e21) > f64(np.float32(th2))))
        self.active &= ~bad
        return int(bad.sum())


def _lambda_init(H):
    """computeLambdaInit: tau = 1e-5 times the largest |diagonal entry| (a NaN entry is skipped)"""
    md = 0.0
    for j in range(7):
        a = abs(H[j, j])
        md = a if a > md else md
    return 1e-5 * md


def canon(v):
    v = np.array(v, f64).copy().reshape(-1)
    v[np.isnan(v)] = np.nan      # numpy's nan is the quiet NaN 0x7FF8000000000000
    return v


def optimize_sim3(F, prob, th2=10.0, fix_scale=False, jacobian=0, fn=LIBM):
    """-> the dict api.sim3_opt_results() makes of a job"""
    g = Graph(F, prob, th2, fix_scale, jacobian, fn)
    S0 = sim3_from_Rts(np.asarray(prob["R12"], f64).reshape(3, 3), prob["t12"], prob["s12"])
    g.S = S0
    its = [0, 0]
    its[0] = g.optimize(5)
    n_bad = g.classify(th2)
    n = g.n

    def result(S, n_in):
        return dict(n_inliers=n_in, n_correspondences=n, n_bad=n_bad, iterations=np.array(its, np.int32), keep=g.active.astype(np.uint8),
                    q12=canon(S[0]), t12=canon(S[1]), s12=canon([S[2]]))
    if n - n_bad < 10:
        return result(S0, 0)
    its[1] = g.optimize(10 if n_bad > 0 else 5)
    bad2 = g.classify(th2)
    return result(g.S, n - n_bad - bad2)
