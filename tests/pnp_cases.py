"""Synthetic and hand-built problems for the PnP tests (numpy only, so the GPU tests can build them where they run).

problem(): a camera pose, map points seen on the five faces of the cubemap (1.5 - 8 m away, |t| <= 3), their pixels (synth.rays_to_cubemap's layout),
unit key rays through those pixels, a share of outliers (a pixel elsewhere on the canvas), per-point sigma2 of a 1.2 pyramid.  Everything a
PnPsolver holds is float32, as in the reference.  draws(): what DUtils::Random::RandomInt(0, size - 1) would return, four per iteration."""
import numpy as np

from cubemapslam_amd import synth

F = 550


def random_pose(rng, max_angle=0.6, max_t=3.0):
    ax = rng.normal(size=3)
    R = synth._rot(ax, rng.uniform(-max_angle, max_angle))
    t = rng.uniform(-1, 1, 3); t *= rng.uniform(0, max_t) / max(np.linalg.norm(t), 1e-9)
    return R, t


def canvas_pixels(rng, n, margin=4.0, front_first=False):
    """n pixels inside the five faces of the 3F x 3F canvas"""
    origin = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)], np.float64)      # faces 0..4: column, row of the face on the canvas
    f = rng.integers(0, 5, n)
    if front_first:
        f[0] = 0
    uv = rng.uniform(margin, F - margin, (n, 2)) + origin[f] * F
    return uv


def problem(seed, N=60, outliers=0.3, noise=0.0, F_=F, front_first=False):
    """front_first: the first point is seen on the front face.  solve_for_sign (:647-660) makes the FIRST point's camera z positive, so an EPnP solve
    whose first correspondence lies behind the image plane of the front face comes out mirrored -- the reference's behaviour, kept by the core."""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng)
    uv = canvas_pixels(rng, N, front_first=front_first)
    _, ray = synth.pixel_to_ray(F_, uv[:, 0], uv[:, 1])
    Xc = ray / np.linalg.norm(ray, axis=1, keepdims=True) * rng.uniform(1.5, 8.0, (N, 1))
    Xw = (Xc - t) @ R                                  # Xc = R Xw + t
    p2d = uv + rng.normal(0, noise, uv.shape) if noise > 0 else uv.copy()
    n_out = int(round(outliers * N))
    out = np.zeros(N, bool)
    if n_out:
        out[rng.choice(N, n_out, replace=False)] = True
        p2d[out] = canvas_pixels(rng, n_out)
    p2d = p2d.astype(np.float32)
    _, kray = synth.pixel_to_ray(F_, p2d[:, 0].astype(np.float64), p2d[:, 1].astype(np.float64))
    bearing = (kray / np.linalg.norm(kray, axis=1, keepdims=True)).astype(np.float32)
    sigma2 = (1.2 ** (2 * rng.integers(0, 8, N))).astype(np.float32)
    return dict(F=F_, R=R, t=t, zc=Xc[:, 2].copy(), p3d=Xw.astype(np.float32), p2d=p2d, bearing=bearing, sigma2=sigma2, outlier=out, min_inliers=max(8, int(0.4 * N)), max_its=35)


def draws(seed, N, iterations):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N - k, iterations) for k in range(4)], 1).astype(np.int32)


def draws_for(sets, N):
    """The draws that make swap-and-pop pick the listed index quadruples (one row per iteration)"""
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


def exact_problem(seed, n_in, n_out, F_=F):
    """n_in exact correspondences first, then n_out far outliers (their pixel is that of a different, distant direction): a quadruple of inliers
    gives the pose and exactly the n_in inliers, any quadruple with an outlier gives next to nothing"""
    pr = problem(seed, N=n_in + n_out, outliers=0.0, F_=F_)
    rng = np.random.default_rng(seed + 1000)
    for i in range(n_in, n_in + n_out):
        while True:
            uv = canvas_pixels(rng, 1)[0]
            if np.hypot(*(uv - pr["p2d"][i])) > 200:
                break
        pr["p2d"][i] = uv.astype(np.float32)
        _, kray = synth.pixel_to_ray(F_, np.array([float(pr["p2d"][i, 0])]), np.array([float(pr["p2d"][i, 1])]))
        pr["bearing"][i] = (kray[0] / np.linalg.norm(kray[0])).astype(np.float32)
    pr["outlier"][n_in:] = True
    pr["sigma2"][:] = 1.0
    return pr
