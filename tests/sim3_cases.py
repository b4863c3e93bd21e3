"""Synthetic and hand-built problems for the Sim3 tests (numpy only, so the GPU tests can build them where they run).

problem(): points X1 in the frame of key frame 1 on the five faces of the cubemap (1.5 - 8 m away), a true similarity S21 (s in [0.7, 1.4], a
rotation <= 0.5 rad, |t| <= 1), X2 = S21 X1 with relative Gaussian noise 0.002, a share of outliers with a random X2, the constructor's filter
(both points project into a face), trimmed to N exactly, mvnMaxError from a 1.2 pyramid.  Everything a Sim3Solver holds is float32, as in the
reference.  draws(): what DUtils::Random::RandomInt(0, size - 1) would return, three per iteration."""
import numpy as np

from cubemapslam_amd import synth
from npref_pnp import rays_to_cubemap

F = 550
f32 = np.float32


def in_a_face(X, F_=F):
    """The constructor's test (:94-98): TransformRaysToCubemap leaves u >= 0 and v >= 0"""
    X = np.asarray(X, f32)
    _, u, v = rays_to_cubemap(F_, X[:, 0], X[:, 1], X[:, 2])
    return ~((u < 0) | (v < 0))


def face_points(rng, n, F_=F, margin=4.0):
    origin = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)], np.float64)
    f = rng.integers(0, 5, n)
    uv = rng.uniform(margin, F_ - margin, (n, 2)) + origin[f] * F_
    _, ray = synth.pixel_to_ray(F_, uv[:, 0], uv[:, 1])
    return ray / np.linalg.norm(ray, axis=1, keepdims=True) * rng.uniform(1.5, 8.0, (n, 1))


def true_sim3(rng):
    """S21: X2 = s R X1 + t"""
    R = synth._rot(rng.normal(size=3), rng.uniform(-0.5, 0.5))
    t = rng.uniform(-1, 1, 3); t *= rng.uniform(0, 1.0) / max(np.linalg.norm(t), 1e-9)
    return rng.uniform(0.7, 1.4), R, t


def max_error(sigma2):
    """mvnMaxError (:117-118): the double product 9.210 * sigma2 narrowed to float"""
    return (9.210 * np.asarray(sigma2, f32).astype(np.float64)).astype(f32)


def problem(seed, N=60, outliers=0.3, noise=0.002, fix_scale=0, min_inliers=20, max_its=300, F_=F):
    rng = np.random.default_rng(seed)
    s, R, t = true_sim3(rng)
    if fix_scale:
        s = 1.0
    x1, x2, out = [], [], []
    have = 0
    while have < N:
        n = 2 * N + 16
        X1 = face_points(rng, n, F_)
        X2 = s * X1 @ R.T + t
        if noise > 0:
            X2 += rng.normal(0, noise, (n, 3)) * np.linalg.norm(X2, axis=1, keepdims=True)
        o = rng.uniform(size=n) < outliers
        X2[o] = face_points(rng, int(o.sum()), F_)
        X1 = X1.astype(f32); X2 = X2.astype(f32)
        keep = in_a_face(X1, F_) & in_a_face(X2, F_)
        x1.append(X1[keep]); x2.append(X2[keep]); out.append(o[keep])
        have += int(keep.sum())
    x1 = np.concatenate(x1)[:N]; x2 = np.concatenate(x2)[:N]; out = np.concatenate(out)[:N]
    sig1 = (f32(1.2) ** (2 * rng.integers(0, 8, N))).astype(f32); sig2 = (f32(1.2) ** (2 * rng.integers(0, 8, N))).astype(f32)
    # S12 = S21^-1: X1 = (1/s) R^T (X2 - t)
    return dict(F=F_, s21=s, R21=R, t21=t, s12=1.0 / s, R12=R.T.copy(), t12=-(R.T @ t) / s, x3dc1=x1, x3dc2=x2, outlier=out, max_err1=max_error(sig1),
                max_err2=max_error(sig2), fix_scale=int(fix_scale), min_inliers=int(min_inliers), max_its=int(max_its))


def exact_problem(seed, n_in, n_out, F_=F):
    """n_in noise-free correspondences first, then n_out far outliers: a triple of inliers gives the motion and (up to float rounding, far from the
    9.21-pixel^2 bar) exactly the n_in inliers, a triple with an outlier next to nothing"""
    pr = problem(seed, N=n_in + n_out, outliers=0.0, noise=0.0, F_=F_)
    rng = np.random.default_rng(seed + 1000)
    for i in range(n_in, n_in + n_out):
        while True:
            X = face_points(rng, 1, F_).astype(f32)
            if np.linalg.norm(X[0] - pr["x3dc2"][i]) > 3.0 and in_a_face(X, F_)[0]:
                break
        pr["x3dc2"][i] = X[0]
    pr["outlier"][n_in:] = True
    pr["max_err1"][:] = max_error([1.0])[0]; pr["max_err2"][:] = max_error([1.0])[0]
    return pr


def draws(seed, N, iterations):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N - k, iterations) for k in range(3)], 1).astype(np.int32)


def draws_for(sets, N):
    """The draws that make swap-and-pop pick the listed index triples (one row per iteration)"""
    out = []
    for s in sets:
        avail = list(range(N)); row = []
        for idx in s:
            r = avail.index(idx); row.append(r)
            avail[r] = avail[-1]; avail.pop()
        out.append(row)
    return np.array(out, np.int32).reshape(-1, 3)


def swap_and_pop(N, row):
    avail = list(range(N)); idx = []
    for r in row:
        idx.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    return idx
