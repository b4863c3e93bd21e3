"""numpy restatement of PnPsolver (src/PnPsolver.cpp:312-343, :385-961) for the tests of cubemapslam_amd/csrc/cms_pnp_core.h.

Every stage is a function of the previous stage's outputs, so a test can feed it what the core produced (the result of a four-point EPnP is defined by the
SVD that picks a basis of MtM's null space: two correct SVDs give different hypotheses, and only stage by stage can the core be pinned from outside).
compute_pose() is the whole solve with numpy's LAPACK SVD or with the plain Jacobi below; check_inliers() is CheckInliers bit for bit in float32.
rays_to_cubemap() here keeps the in-face values for a point that falls in a face branch but outside [0, F) -- CheckInliers does not look at the face --;
npref_reloc.rays_to_cubemap writes -1 there and is not to be used for this."""
import numpy as np

f32 = np.float32


def svd_lapack(A):
    """-> (U, w, Vt), w descending"""
    return np.linalg.svd(np.asarray(A, np.float64))


def svd_jacobi(A, sweeps=60):
    """Plain one-sided Jacobi (Hestenes) on the columns of A, independent of the core's in order and formulae: rotation angle from atan2."""
    A = np.array(A, np.float64)
    m, n = A.shape
    V = np.eye(n)
    for _ in range(sweeps):
        off = 0.0
        for p in range(n - 1):
            for q in range(p + 1, n):
                a = A[:, p] @ A[:, p]; b = A[:, q] @ A[:, q]; c = A[:, p] @ A[:, q]
                if abs(c) <= 1e-17 * np.sqrt(a * b) or c == 0.0:
                    continue
                off = max(off, abs(c) / np.sqrt(a * b))
                th = 0.5 * np.arctan2(2 * c, a - b)
                cs, sn = np.cos(th), np.sin(th)
                Ap, Aq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = cs * Ap + sn * Aq; A[:, q] = cs * Aq - sn * Ap
                Vp, Vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = cs * Vp + sn * Vq; V[:, q] = cs * Vq - sn * Vp
        if off < 1e-15:
            break
    w = np.linalg.norm(A, axis=0)
    o = np.argsort(-w, kind="stable")
    w, A, V = w[o], A[:, o], V[:, o]
    U = np.zeros_like(A)
    nz = w > 1e-300
    U[:, nz] = A[:, nz] / w[nz]
    return U, w, V.T


def sym_vectors(A, svd):
    """(w, rows): singular values and right singular vectors (rows) of a symmetric matrix"""
    _, w, Vt = svd(A)
    return w, Vt


def lstsq(A, b):
    return np.linalg.lstsq(A, b, rcond=None)[0]


def control_points(pws, dc, uct):
    n = len(pws)
    c0 = pws.sum(0) / n
    cws = np.zeros((4, 3)); cws[0] = c0
    for i in range(1, 4):
        cws[i] = c0 + np.sqrt(dc[i - 1] / n) * uct[i - 1]
    return cws


def pca(pws):
    P0 = pws - pws.sum(0) / len(pws)
    return P0.T @ P0


def barycentric(pws, cws):
    CC = (cws[1:] - cws[0]).T
    ci = np.linalg.inv(CC)
    a = np.zeros((len(pws), 4))
    a[:, 1:] = (pws - cws[0]) @ ci.T
    a[:, 0] = 1.0 - a[:, 1] - a[:, 2] - a[:, 3]
    return a


def build_M(alphas, bearings):
    n = len(alphas)
    M = np.zeros((2 * n, 12))
    r, s, t = bearings[:, 0], bearings[:, 1], bearings[:, 2]
    for i in range(4):
        a = alphas[:, i]
        M[0::2, 3 * i] = a * (s + t); M[0::2, 3 * i + 1] = -a * r; M[0::2, 3 * i + 2] = -a * r
        M[1::2, 3 * i] = -a * s; M[1::2, 3 * i + 1] = a * (r + t); M[1::2, 3 * i + 2] = -a * s
    return M


PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def L_6x10(ut):
    v = [ut[11].reshape(4, 3), ut[10].reshape(4, 3), ut[9].reshape(4, 3), ut[8].reshape(4, 3)]
    dv = [[vi[a] - vi[b] for a, b in PAIRS] for vi in v]
    L = np.zeros((6, 10))
    for i in range(6):
        d = [dv[k][i] for k in range(4)]
        L[i] = [d[0] @ d[0], 2 * d[0] @ d[1], d[1] @ d[1], 2 * d[0] @ d[2], 2 * d[1] @ d[2], d[2] @ d[2], 2 * d[0] @ d[3], 2 * d[1] @ d[3], 2 * d[2] @ d[3], d[3] @ d[3]]
    return L


def rho(cws):
    return np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in PAIRS])


def betas_approx(which, L, rh, solve=lstsq):
    """-> (betas, A): the least-squares matrix is handed back for the condition-number rule of the stage test"""
    with np.errstate(all="ignore"):
        if which == 1:
            A = L[:, [0, 1, 3, 6]]; b = solve(A, rh)
            s = -1.0 if b[0] < 0 else 1.0
            b0 = np.sqrt(s * b[0])
            return np.array([b0, s * b[1] / b0, s * b[2] / b0, s * b[3] / b0]), A
        if which == 2:
            A = L[:, [0, 1, 2]]; b = solve(A, rh)
        else:
            A = L[:, [0, 1, 2, 3, 4]]; b = solve(A, rh)
        if b[0] < 0:
            b0 = np.sqrt(-b[0]); b1 = np.sqrt(-b[2]) if b[2] < 0 else 0.0
        else:
            b0 = np.sqrt(b[0]); b1 = np.sqrt(b[2]) if b[2] > 0 else 0.0
        if b[1] < 0:
            b0 = -b0
        return np.array([b0, b1, (b[3] / b0) if which == 3 else 0.0, 0.0]), A


def gn_system(L, rh, be):
    B = np.array([be[0] * be[0], be[0] * be[1], be[1] * be[1], be[0] * be[2], be[1] * be[2], be[2] * be[2], be[0] * be[3], be[1] * be[3], be[2] * be[3], be[3] * be[3]])
    A = np.stack([2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3],
                  L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3],
                  L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3],
                  L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]], 1)
    return A, rh - L @ B


def gauss_newton(L, rh, betas, solve=lstsq):
    """-> (betas, worst condition number of the five systems)"""
    be = np.array(betas, np.float64)
    worst = 0.0
    for _ in range(5):
        A, b = gn_system(L, rh, be)
        worst = max(worst, np.linalg.cond(A) if np.isfinite(A).all() else np.inf)
        be = be + solve(A, b)
    return be, worst


def rays_to_cubemap(F, x, y, z):
    """CamModelGeneral::TransformRaysToCubemap on float32 arrays, bit for bit: (face, u, v); a point in a branch but outside the face keeps the in-face
    u, v with face -1; a point in no branch has (-1, -1)"""
    x = np.asarray(x, f32); y = np.asarray(y, f32); z = np.asarray(z, f32)
    n = x.shape[0]
    face = np.full(n, -1, np.int32); up = np.full(n, -1, f32); vp = np.full(n, -1, f32)
    f = F / 2.0
    todo = np.ones(n, bool)
    with np.errstate(all="ignore"):
        br = [(0, z > 0, (x, y), z, (x, y, z), (F, F)), (2, x > 0, (y, z), x, (-z, y, x), (2 * F, F)), (1, x < 0, (y, z), -x, (z, y, -x), (0, F)),
              (4, y > 0, (x, z), y, (x, -z, y), (F, 2 * F)), (3, y < 0, (x, z), -y, (x, z, -y), (F, 0))]
        for fid, pos, (p, q), den, (lx, ly, lz), (ox, oy) in br:
            c = pos & (p / den <= 1) & (p / den >= -1) & (q / den <= 1) & (q / den >= -1) & todo
            u = (lx.astype(np.float64) * f / lz.astype(np.float64) + f).astype(f32)
            v = (ly.astype(np.float64) * f / lz.astype(np.float64) + f).astype(f32)
            inside = c & ~((u < 0) | (u >= F) | (v < 0) | (v >= F))
            up[c] = u[c]; vp[c] = v[c]
            if ox:
                up[inside] = (u[inside] + f32(ox)).astype(f32)
            if oy:
                vp[inside] = (v[inside] + f32(oy)).astype(f32)
            face[inside] = fid
            todo &= ~c
    return face, up, vp


def check_inliers(F, R, t, p3d, p2d, max_error):
    """CheckInliers (:312-343) bit for bit: R (3x3) and t double, the rest float32 -> bool mask"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64)
    P = np.asarray(p3d, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        c = [(((R[k, 0] * P[:, 0] + R[k, 1] * P[:, 1]) + R[k, 2] * P[:, 2]) + t[k]).astype(f32) for k in range(3)]
        _, ue, ve = rays_to_cubemap(F, c[0], c[1], c[2])
        dx = (np.asarray(p2d, f32)[:, 0] - ue).astype(f32); dy = (np.asarray(p2d, f32)[:, 1] - ve).astype(f32)
        e2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
        return e2 < np.asarray(max_error, f32)


def reprojection_error(F, pws, us, R, t):
    Xc = pws @ R.T + t
    _, ue, ve = rays_to_cubemap(F, Xc[:, 0].astype(f32), Xc[:, 1].astype(f32), Xc[:, 2].astype(f32))
    return np.sqrt((us[:, 0] - ue.astype(np.float64)) ** 2 + (us[:, 1] - ve.astype(np.float64)) ** 2).sum() / len(pws)


def R_and_t(F, pws, us, alphas, ut, betas, svd=svd_lapack):
    ccs = sum(betas[i] * ut[11 - i].reshape(4, 3) for i in range(4))
    pcs = alphas @ ccs
    if pcs[0, 2] < 0:
        ccs, pcs = -ccs, -pcs
    n = len(pws)
    pc0 = pcs.sum(0) / n; pw0 = pws.sum(0) / n
    ABt = (pcs - pc0).T @ (pws - pw0)
    U, _, Vt = svd(ABt)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    t = pc0 - R @ pw0
    return R, t, reprojection_error(F, pws, us, R, t)


def compute_pose(F, pws, us, bearings, svd=svd_lapack, solve=lstsq):
    """The whole EPnP solve (:488-536) -> (R, t, rep_error)"""
    dc, uct = sym_vectors(pca(pws), svd)
    cws = control_points(pws, dc, uct)
    al = barycentric(pws, cws)
    M = build_M(al, bearings)
    _, ut = sym_vectors(M.T @ M, svd)
    L = L_6x10(ut); rh = rho(cws)
    best = None
    for which in (1, 2, 3):
        b0, _ = betas_approx(which, L, rh, solve)
        be, _ = gauss_newton(L, rh, b0, solve)
        R, t, e = R_and_t(F, pws, us, al, ut, be, svd)
        if best is None or e < best[2]:
            best = (R, t, e)
    return best
