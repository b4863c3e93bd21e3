"""An independent restatement of Sim3Solver::ComputeSim3 (src/Sim3Solver.cpp:239-361) written from the reference's text: numpy in a working
precision of the caller's (float64 for the comparison with the core, float32 for measuring what single precision alone costs), np.linalg.eigh
for cv::eigen, and atan2 -> angle-axis -> Rodrigues for the rotation.  Each stage is a function of the previous stage's output, so that a test
can feed it the core's own previous stage.  check_inliers() restates CheckInliers (:364-394) in the core's float32 / float64 steps, bit for bit."""
import numpy as np

from npref_pnp import rays_to_cubemap

f32 = np.float32


def centroid(P, dt=np.float64):
    """ComputeCentroid: P is 3 x 3 with one point per column -> (Pr, O)"""
    P = np.asarray(P, dt)
    O = P.sum(1) / dt(3)
    return (P - O[:, None]).astype(dt), O.astype(dt)


def m_matrix(Pr1, Pr2, dt=np.float64):
    return (np.asarray(Pr2, dt) @ np.asarray(Pr1, dt).T).astype(dt)


def n_matrix(M, dt=np.float64):
    M = np.asarray(M, np.float64)
    N11 = M[0, 0] + M[1, 1] + M[2, 2]; N12 = M[1, 2] - M[2, 1]; N13 = M[2, 0] - M[0, 2]; N14 = M[0, 1] - M[1, 0]
    N22 = M[0, 0] - M[1, 1] - M[2, 2]; N23 = M[0, 1] + M[1, 0]; N24 = M[2, 0] + M[0, 2]
    N33 = -M[0, 0] + M[1, 1] - M[2, 2]; N34 = M[1, 2] + M[2, 1]; N44 = -M[0, 0] - M[1, 1] + M[2, 2]
    return np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], dt)


def top_eigenvector(N, dt=np.float64):
    """cv::eigen's first row: the eigenvector of the largest eigenvalue -> (vector, eigenvalues descending)"""
    w, V = np.linalg.eigh(np.asarray(N, dt))
    return V[:, -1].astype(dt), w[::-1].astype(dt)


def relative_gap(evals_desc):
    """(lambda1 - lambda2) / |lambda1|: what conditions the top eigenvector"""
    w = np.asarray(evals_desc, np.float64)
    return (w[0] - w[1]) / abs(w[0]) if w[0] != 0 else 0.0


def rotation(evec, dt=np.float64):
    """:298-308: the imaginary part, atan2 of its norm and the real part, angle-axis, Rodrigues"""
    e = np.asarray(evec, dt)
    vec = e[1:4]
    nrm = np.sqrt((vec.astype(np.float64) ** 2).sum())
    ang = np.arctan2(nrm, float(e[0]))
    r = (2 * ang * vec.astype(np.float64) / nrm).astype(dt)
    theta = np.sqrt((r.astype(np.float64) ** 2).sum())
    k = r.astype(np.float64) / theta
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * K
    return R.astype(dt)


def scale(Pr1, Pr2, R, dt=np.float64):
    P3 = (np.asarray(R, dt) @ np.asarray(Pr2, dt)).astype(dt)
    nom = (np.asarray(Pr1, dt).astype(np.float64) * P3.astype(np.float64)).sum()
    den = ((P3 * P3).astype(dt).astype(np.float64)).sum()
    with np.errstate(all="ignore"):
        return dt(nom / den), P3, nom, den


def translation(O1, O2, R, s, dt=np.float64):
    return (np.asarray(O1, dt) - (dt(s) * np.asarray(R, dt) @ np.asarray(O2, dt)).astype(dt)).astype(dt)


def transforms(R, t, s, dt=np.float64):
    """T12 = [sR | t], T21 = [(1/s) R^T | -(1/s) R^T t] as 3 x 4"""
    R = np.asarray(R, dt); t = np.asarray(t, dt)
    sR = (dt(s) * R).astype(dt)
    sRinv = ((1.0 / float(s)) * R.T.astype(np.float64)).astype(dt)
    tinv = (-(sRinv @ t)).astype(dt)
    return np.hstack([sR, t[:, None]]).astype(dt), np.hstack([sRinv, tinv[:, None]]).astype(dt)


def compute_sim3(P1, P2, fix_scale=False, dt=np.float64):
    """The whole of ComputeSim3 on P1, P2 (3 points x 3 coordinates, one point per ROW) in precision dt"""
    Pr1, O1 = centroid(np.asarray(P1).T, dt); Pr2, O2 = centroid(np.asarray(P2).T, dt)
    M = m_matrix(Pr1, Pr2, dt); N = n_matrix(M, dt)
    e, w = top_eigenvector(N, dt)
    R = rotation(e, dt)
    s, P3, nom, den = scale(Pr1, Pr2, R, dt)
    if fix_scale:
        s = dt(1)
    t = translation(O1, O2, R, s, dt)
    T12, T21 = transforms(R, t, s, dt)
    return dict(O1=O1, O2=O2, Pr1=Pr1, Pr2=Pr2, M=M, N=N, evec=e, evals=w, gap=relative_gap(w), R=R, s=s, t=t, T12=T12, T21=T21, P3=P3, nom=nom, den=den)


def _project(F, T, X):
    T = np.asarray(T, f32).reshape(3, 4).astype(np.float64); X = np.asarray(X, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        c = [((((T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1]) + T[k, 2] * X[:, 2]) + T[k, 3])).astype(f32) for k in range(3)]
    _, u, v = rays_to_cubemap(F, c[0], c[1], c[2])
    return u, v


def check_inliers(F, T12, T21, x1, x2, me1, me2):
    """CheckInliers bit for bit: T12 / T21 3 x 4 float32 -> bool mask"""
    x1 = np.asarray(x1, f32); x2 = np.asarray(x2, f32)
    with np.errstate(all="ignore"):
        _, p1u, p1v = rays_to_cubemap(F, x1[:, 0], x1[:, 1], x1[:, 2])
        _, p2u, p2v = rays_to_cubemap(F, x2[:, 0], x2[:, 1], x2[:, 2])
        au, av = _project(F, T12, x2)
        bu, bv = _project(F, T21, x1)
        d = lambda a, b: (a - b).astype(f32).astype(np.float64)
        e1 = (d(p1u, au) ** 2 + d(p1v, av) ** 2).astype(f32)
        e2 = (d(bu, p2u) ** 2 + d(bv, p2v) ** 2).astype(f32)
        return (e1 < np.asarray(me1, f32)) & (e2 < np.asarray(me2, f32))


def ransac_parameters(N, probability, min_inliers, max_iterations):
    """SetRansacParameters (:138-162) with x86's conversion of a double no int holds"""
    with np.errstate(all="ignore"):
        eps = f32(min_inliers) / f32(N) if N != 0 else (f32(np.inf) if min_inliers > 0 else (f32(np.nan) if min_inliers == 0 else f32(-np.inf)))
        if min_inliers == N:
            n_it = 1
        else:
            v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(eps) ** 3))
            n_it = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2 ** 31
    return max(1, min(n_it, max_iterations))
