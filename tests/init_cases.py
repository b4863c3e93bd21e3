"""Synthetic two-view problems for the Initializer tests (numpy only, so the GPU tests can build them where they run).

problem(): points in the frame of camera 1 (mostly in front of both cameras: CheckRT drops what lies outside the field of view), the pose of
camera 2 (X2 = R X1 + t), cubemap key points through synth.rays_to_cubemap with pixel noise, unit key rays through the noisy pixels, a share of
outliers (the key point of frame 2 somewhere else on the canvas), and a matches12 vector with holes over n1 != n2 != N key points.  Everything an
Initializer holds is float32, as in the reference.  draws(): what DUtils::Random::RandomInt(0, size - 1) would return, eight per iteration."""
import numpy as np

from cubemapslam_amd import synth

F = 550


def pose(rng, angle=0.12, baseline=0.4):
    R = synth._rot(rng.normal(size=3), rng.uniform(0.3, 1.0) * angle) if angle > 0 else np.eye(3)
    t = rng.normal(size=3); t *= baseline / np.linalg.norm(t)
    return R, t


def unit_rays(Fc, px):
    _, r = synth.pixel_to_ray(Fc, px[:, 0].astype(np.float64), px[:, 1].astype(np.float64))
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)


def canvas_pixels(rng, n, Fc, margin=4.0):
    origin = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)], np.float64)
    return rng.uniform(margin, Fc - margin, (n, 2)) + origin[rng.integers(0, 5, n)] * Fc


def problem(seed, N=120, extra1=17, extra2=29, noise=0.0, outliers=0.0, angle=0.12, baseline=0.4, depth=(2.0, 8.0), Fc=F):
    rng = np.random.default_rng(seed)
    R, t = pose(rng, angle, baseline)
    X1 = np.zeros((0, 3)); p1 = np.zeros((0, 2)); p2 = np.zeros((0, 2))
    while len(X1) < N:
        d = rng.normal(size=(4 * N, 3)); d[:, 2] = np.abs(d[:, 2]) + 0.35
        X = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(depth[0], depth[1], (4 * N, 1))
        X2 = X @ R.T + t
        f1, u1, v1 = synth.rays_to_cubemap(Fc, X); f2, u2, v2 = synth.rays_to_cubemap(Fc, X2)
        inside = lambda u, v: (np.mod(u, Fc) > 5) & (np.mod(u, Fc) < Fc - 5) & (np.mod(v, Fc) > 5) & (np.mod(v, Fc) < Fc - 5)
        ok = (f1 >= 0) & (f2 >= 0) & inside(u1, v1) & inside(u2, v2) & (X2[:, 2] / np.linalg.norm(X2, axis=1) > 0.2)
        X1 = np.concatenate([X1, X[ok]]); p1 = np.concatenate([p1, np.stack([u1, v1], 1)[ok]]); p2 = np.concatenate([p2, np.stack([u2, v2], 1)[ok]])
    X1, p1, p2 = X1[:N], p1[:N], p2[:N]
    if noise > 0:
        p1 = p1 + rng.normal(0, noise, p1.shape); p2 = p2 + rng.normal(0, noise, p2.shape)
    out = np.zeros(N, bool)
    n_out = int(round(outliers * N))
    if n_out:
        out[rng.choice(N, n_out, replace=False)] = True
        p2[out] = canvas_pixels(rng, n_out, Fc)
    n1, n2 = N + extra1, N + extra2
    at1 = np.sort(rng.choice(n1, N, replace=False)); at2 = rng.permutation(n2)[:N]
    keys1 = canvas_pixels(rng, n1, Fc); keys2 = canvas_pixels(rng, n2, Fc)
    keys1[at1] = p1; keys2[at2] = p2
    keys1 = keys1.astype(np.float32); keys2 = keys2.astype(np.float32)
    matches12 = np.full(n1, -1, np.int32); matches12[at1] = at2
    truth = np.zeros((n1, 3)); truth[at1] = X1
    is_out = np.zeros(n1, bool); is_out[at1] = out
    return dict(F=Fc, R=R, t=t, keys1=keys1, rays1=unit_rays(Fc, keys1), keys2=keys2, rays2=unit_rays(Fc, keys2), matches12=matches12, truth=truth,
                outlier=is_out, N=N)


def draws(seed, N, iterations):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N - k, iterations) for k in range(8)], 1).astype(np.int32)


def draws_for(sets, N):
    """The draws that make swap-and-pop pick the listed index octuples (one row per iteration)"""
    out = []
    for s in sets:
        avail = list(range(N)); row = []
        for idx in s:
            r = avail.index(idx); row.append(r)
            avail[r] = avail[-1]; avail.pop()
        out.append(row)
    return np.array(out, np.int32)


def swap_and_pop(N, row):
    avail = list(range(N)); idx = []
    for r in row:
        idx.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    return idx


def trim(prob, keep):
    """The problem with only the first `keep` matches (in index order) left in matches12"""
    m = prob["matches12"].copy()
    at = np.flatnonzero(m >= 0)
    m[at[keep:]] = -1
    return dict(prob, matches12=m, N=min(keep, len(at)))
