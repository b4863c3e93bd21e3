"""Inputs of the SearchBySim3 tests (tests/test_sim3_search_cpu.py, tests/test_gpu_search_by_sim3.py): hand-built cases with the answers written
out, and seeded pairs of key frames.  Everything is deterministic.

A case is a dict: camd, sf, kf1 / kf2 = dict(kx, ky, koct, kdesc, pose12 = Rcw | tcw), s12, R12, t12, mp1 / mp2 = per key point of that key frame
dict(skip, pos, min_dist, max_dist (the raw members mfMinDistance / mfMaxDistance), desc), th.  run(case, z_as_written) is the restatement.

Geometry of a "track": one physical point X, given in key frame 1's camera coordinates.  Key frame 1's map point sits at X (through the frame's
pose), key frame 2's map point at Y = sR21 X + t21, the same physical point as key frame 2's drifted map has it.  Key frame 2 sees it at the
projection of Y; key frame 1's key point is placed where direction 2 -> 1 lands: the projection of X, or, for z_as_written, of (x, y, y) -- line
:1507 as the reference has it.  With |x| > |y| and x > 0 that ray falls on the right face whatever y's sign, so such tracks match in both modes."""
import numpy as np

import npref_sim3_search as ref
from cubemapslam_amd import synth
from reloc_cases import _least_float_with, desc_at, flip_bits

F = 550
CAMD = synth.camera("lafida", F)
SF = ref.scale_factors(1.2, 8)
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
EYE = np.eye(3, dtype=np.float32)
TH = 7.5
f32 = np.float32


def run(c, z_as_written=True, info=None, bounds_scaled=0):
    """the restatement on a case -> (idx2, nFound)"""
    mp1, mp2 = c["mp1"], c["mp2"]
    if bounds_scaled:
        sc = lambda m: dict(m, min_dist=(f32(0.8) * m["min_dist"]).astype(np.float32), max_dist=(f32(1.2) * m["max_dist"]).astype(np.float32))
        mp1, mp2 = sc(mp1), sc(mp2)
    return ref.search_by_sim3(c["camd"], c["sf"], c["kf1"], c["kf2"], c["s12"], c["R12"], c["t12"], mp1, mp2, th=c["th"], z_as_written=z_as_written,
                              bounds_scaled=bounds_scaled, info=info)


def _pix(x, y, z):
    _, u, v = ref.rays_to_cubemap(F, np.array([x], np.float32), np.array([y], np.float32), np.array([z], np.float32))
    return float(u[0]), float(v[0])


def _norm(p):
    return float(np.sqrt((np.asarray(p, np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------------------------------------- hand-built cases
# nine directions with x > |y| and x < z: the true projection is on the front face, the one of (x, y, y) on the right face; both sets of sites
# are at least 35 px apart (hand_sites_apart)
_RATIO = [0.05, 0.25, 0.45, 0.65, 0.85, -0.2, -0.4, -0.6, -0.8]
DIRS = [np.array([xz * 5.0, xz * 5.0 * r, 5.0]) for r, xz in zip(_RATIO, [0.3, 0.6, 0.9, 0.3, 0.6, 0.9, 0.3, 0.6, 0.9])]


def K(at, oct=4, ham=10, d=(2.0, 1.0), mp="own", level=3.5, min_dist=0.1, max_dist=None, skip=0, px=None):
    """a key point near the site of physical point `at` (key frame 1 coordinates), its descriptor `ham` bits from zero, holding the map point of
    physical point `mp` ("own": at; None: no map point) whose distance members predict ceil(level) unless max_dist is given.  px: the pixel itself."""
    return dict(at=np.asarray(at, np.float64), oct=oct, ham=ham, d=d, mp=(np.asarray(at, np.float64) if isinstance(mp, str) else mp), level=level, min_dist=min_dist,
                max_dist=max_dist, skip=skip, px=px)


def hand(k1, k2, zw, s12=1.0, R12=EYE, t12=(0, 0, 0), th=TH):
    """both key frames at the identity pose; k1 / k2: K() entries.  All map-point descriptors are zero, so a pair's distance is the key point's number."""
    assert len(k1) <= 16 and len(k2) <= 16
    m = ref.compose(s12, R12, t12)
    to2 = lambda X: m["sR21"].astype(np.float64) @ X + m["t21"].astype(np.float64)

    def side(ks, second):
        n = len(ks)
        kx = np.zeros(n, np.float32); ky = np.zeros(n, np.float32)
        pos = np.full((n, 3), np.nan, np.float32); mn = np.zeros(n, np.float32); mx = np.zeros(n, np.float32); skip = np.ones(n, np.uint8)
        for i, k in enumerate(ks):
            X = k["at"]; Y = to2(X)
            u, v = k["px"] if k["px"] is not None else (_pix(*Y) if second else _pix(X[0], X[1], X[1] if zw else X[2]))
            kx[i] = u + k["d"][0]; ky[i] = v + k["d"][1]
            if k["mp"] is None:
                continue
            Xm = np.asarray(k["mp"], np.float64); Ym = to2(Xm)
            pos[i] = Ym if second else Xm
            dist = _norm(Xm) if second else _norm(Ym)               # dist3D is taken in the OTHER camera
            mn[i] = k["min_dist"]; mx[i] = dist * 1.2 ** k["level"] if k["max_dist"] is None else k["max_dist"]
            skip[i] = k["skip"]
        kf = dict(kx=kx, ky=ky, koct=np.array([k["oct"] for k in ks], np.int32).reshape(n),
                  kdesc=(np.stack([desc_at(int(k["ham"]), 7 * i) for i, k in enumerate(ks)]) if n else np.zeros((0, 32), np.uint8)), pose12=IDENT.copy())
        return kf, dict(skip=skip, pos=pos, min_dist=mn, max_dist=mx, desc=np.zeros((n, 32), np.uint8))
    kf1, mp1 = side(k1, False)
    kf2, mp2 = side(k2, True)
    return dict(camd=CAMD, sf=SF, kf1=kf1, kf2=kf2, s12=f32(s12), R12=np.asarray(R12, np.float32).reshape(3, 3), t12=np.asarray(t12, np.float32), mp1=mp1, mp2=mp2, th=th)


def _dist_of(X):
    """dist3D as the chain computes it for a point at the identity pose and the identity similarity"""
    p = ref.transform(IDENT[:9], IDENT[9:], ref.transform(IDENT[:9], IDENT[9:], np.asarray(X, np.float32)[None, :]))[0]
    return f32(np.sqrt((p.astype(np.float64) ** 2).sum()))


def hand_cases(zw):
    """[(name, case, expected idx2)] for z_as_written = zw -- the expectations are written down here, not computed.  Key frame 1's key points sit
    where direction 2 -> 1 lands in that mode, so the lists are the same in both modes except in the last case."""
    A, B, C, D = DIRS[0], DIRS[1], DIRS[2], DIRS[3]
    out = []
    add = lambda name, k1, k2, want, **kw: out.append((name, hand(k1, k2, zw, **kw), want))
    add("one track matches", [K(A)], [K(A)], [0])
    add("two tracks, key points in another order", [K(A), K(B)], [K(B), K(A)], [1, 0])
    # --- z < 0: (3, 1, -0.5) projects onto the right face, where a key point waits; the depth test drops it in both directions
    behind = np.array([3.0, 1.0, -0.5])
    add("point behind", [K(behind), K(A)], [K(behind), K(A)], [-1, 1])
    # --- unknown face: x / z == 1 puts the pixel on the far edge of the front face (up == F); the camera centre has no face at all
    edge = np.array([5.0, 1.0, 5.0])
    add("unknown face: far edge of the face", [K(edge, px=(F + F - 1.0, 880.0)), K(A)], [K(edge, px=(F + F - 1.0, 880.0)), K(A)], [-1, 1])
    add("unknown face: the camera centre", [K(np.zeros(3), px=(825.0, 825.0), max_dist=1.0), K(A)], [K(np.zeros(3), px=(825.0, 825.0), max_dist=1.0), K(A)], [-1, 1])
    # --- dist3D against the bounds: just outside and just inside each
    dA = _dist_of(A)
    mn_out = _least_float_with(lambda m: dA < f32(0.8) * m, dA, dA * f32(1.5))                 # least mfMinDistance with dist < 0.8f * it
    mn_in = np.nextafter(mn_out, f32(0))
    mx_in = _least_float_with(lambda m: not (dA > f32(1.2) * m), dA * f32(0.5), dA)            # least mfMaxDistance with !(dist > 1.2f * it)
    mx_out = np.nextafter(mx_in, f32(0))
    add("dist3D below the lower bound (key frame 1's point)", [K(A, min_dist=mn_out)], [K(A)], [-1])
    add("dist3D on the lower bound", [K(A, min_dist=mn_in)], [K(A, min_dist=mn_in)], [0])
    add("dist3D below the lower bound (key frame 2's point)", [K(A)], [K(A, min_dist=mn_out)], [-1])
    add("dist3D above the upper bound", [K(A, oct=0, max_dist=mx_out)], [K(A, oct=0, max_dist=mx_in)], [-1])      # ratio < 1: level 0
    add("dist3D on the upper bound", [K(A, oct=0, max_dist=mx_in)], [K(A, oct=0, max_dist=mx_in)], [0])
    # --- the predicted level is clamped.  Below: the upper bound keeps dist <= 1.2f * mfMaxDistance, so the exponent reaches -1 only on the bound
    # itself (the case above); any ratio below 1 gives level 0.  Above: 1.2^12 gives nlevels - 1
    add("level 0 from a ratio below 1", [K(A, oct=0, max_dist=dA / f32(1.1))], [K(A, oct=0, max_dist=dA / f32(1.1))], [0])
    add("level 0: octave 1 is out", [K(A, oct=0, max_dist=dA / f32(1.1))], [K(A, oct=1, max_dist=dA / f32(1.1))], [-1])
    add("level clamped at nlevels - 1", [K(A, oct=7, level=12.0)], [K(A, oct=6, level=12.0)], [0])
    # --- octaves level - 1 and level are candidates, level + 1 and level - 2 are not (level 4)
    for o, want in ((2, -1), (3, 0), (4, 0), (5, -1)):
        add("octave %d in key frame 2" % o, [K(A)], [K(A, oct=o)], [want])
        add("octave %d in key frame 1" % o, [K(A, oct=o)], [K(A)], [want])
    # --- no key point in the window (radius 7.5 * 1.2^4 = 15.6 px)
    add("empty window in key frame 2", [K(A)], [K(A, d=(30.0, 1.0))], [-1])
    add("empty window in key frame 1", [K(A, d=(1.0, -30.0))], [K(A)], [-1])
    # --- bestDist <= TH_HIGH
    add("bestDist 100 is accepted", [K(A)], [K(A, ham=100)], [0])
    add("bestDist 101 is not", [K(A)], [K(A, ham=101)], [-1])
    add("bestDist 101 in key frame 1 is not", [K(A, ham=101)], [K(A)], [-1])
    # --- two candidates at the same distance: the first in GetFeaturesInArea's order wins (two key points of one grid cell come in index order).
    # The winner holds the map point in the first case and the loser in the second, where vnMatch2 therefore never answers
    add("tie: the first candidate, which holds the point", [K(A)], [K(A, ham=20, d=(1.0, 1.0)), K(A, ham=20, d=(2.5, 2.0), mp=None)], [0])
    add("tie: the first candidate, which holds none", [K(A)], [K(A, ham=20, d=(1.0, 1.0), mp=None), K(A, ham=20, d=(2.5, 2.0))], [-1])
    add("no tie: the nearer descriptor", [K(A)], [K(A, ham=21, d=(1.0, 1.0), mp=None), K(A, ham=20, d=(2.5, 2.0))], [1])
    # --- 1 -> 2 and 2 -> 1 disagree: both key points of key frame 1 choose key point 0 of key frame 2, which chooses the nearer descriptor
    add("directions disagree", [K(A, ham=30), K(A, ham=10, d=(-3.0, 2.0))], [K(A)], [-1, 0])
    # --- vbAlreadyMatched1 / 2, a key point without a map point, a bad point: all arrive as skip
    add("already matched in key frame 1", [K(A, skip=1), K(B)], [K(A), K(B)], [-1, 1])
    add("already matched in key frame 2", [K(A), K(B)], [K(A, skip=1), K(B)], [-1, 1])
    add("no map point and a bad one", [K(A, mp=None), K(B), K(C, skip=1), K(D)], [K(A), K(B), K(C), K(D, mp=None)], [-1, 1, -1, -1])
    # --- a window over the edge between the front and the right face: x / z = 0.99 projects 2.75 px in front of u = 2F, key frame 2's key point
    # lies 3 px behind it, on the right face
    near = np.array([4.95, 1.0, 5.0])
    add("window across a face edge", [K(near)], [K(near, d=(5.75, 1.0))], [0])
    # --- s12 != 1 and a translation: key frame 2 holds the point at (X - t) / s
    add("s12 = 2 with a translation", [K(A), K(B)], [K(A), K(B)], [0, 1], s12=2.0, t12=(0.25, -0.125, 0.5))
    add("s12 = 0.75, rotated", [K(A), K(C)], [K(C), K(A)], [1, 0], s12=0.75, R12=synth._rot([0.2, 1.0, 0.1], 0.12), t12=(-0.125, 0.0, 0.25))
    # --- a side without key points
    add("n1 = 0", [], [K(A)], [])
    add("n2 = 0", [K(A), K(B)], [], [-1, -1])
    # --- only z_as_written decides: y > |x| on the front face.  Key frame 1's key point sits at the true projection; as written the ray (x, y, y)
    # reaches the far edge of the front face (vp == F) and is dropped
    up = np.array([0.5, 2.0, 5.0])
    c = hand([K(up, px=_pix(*up))], [K(up)], zw)
    out.append(("only z_as_written decides", c, [-1] if zw else [0]))
    return out


def hand_sites_apart():
    """the sites the hand-built tracks use are far enough apart that no window of a case with several tracks (level 4: radius 15.6 px, key points
    within 3 px of their site) holds key points of two of them"""
    for zw in (False, True):
        for second in (False, True):
            s = np.array([_pix(*X) if second else _pix(X[0], X[1], X[1] if zw else X[2]) for X in DIRS])
            d = np.abs(s[:, None, :] - s[None, :, :]).max(-1) + 1e9 * np.eye(len(s))
            if not (s >= 0).all() or d.min() < 35:
                return False
    return True


# ------------------------------------------------------------------------------------------------------------------------- seeded cases
def _random_pose(rng, rad, trans):
    w = rng.normal(0, 1, 3)
    R = synth._rot(w, rng.uniform(0.3, 1.0) * rad)
    return np.concatenate([R.reshape(-1), rng.uniform(-trans, trans, 3)]).astype(np.float32)


def _directions(rng, n, written, cone=None):
    """n rays with z > 0 over the front and the side faces; written: most of them with |x| > |y| or y < 0, where line :1507's ray finds a face"""
    if cone is not None:
        a = rng.uniform(-cone, cone, (n, 2))
        return np.stack([0.62 + a[:, 0], -0.31 + a[:, 1], np.ones(n)], 1)
    x = rng.uniform(-2.5, 2.5, n); y = rng.uniform(-2.5, 2.5, n)
    if written:
        bad = (np.abs(x) <= np.abs(y)) & (y > 0)
        flip = bad & (rng.random(n) < 0.85)
        y = np.where(flip, -y, y)
    return np.stack([x, y, np.ones(n)], 1)


def seeded(n_kp, seed, written, n2_extra=5, cone=None, th=TH):
    """Two key frames over n physical points (two thirds of n_kp): key frame 1 with n_kp key points, key frame 2 with n_kp + n2_extra; the rest are
    distractors.  written: key frame 1's key points sit where line :1507 lands; else where component 2 does.  cone: all rays inside a narrow
    cone (the dense case)."""
    rng = np.random.default_rng(seed)
    n = (2 * n_kp) // 3
    pose1 = _random_pose(rng, 0.5, 1.0); pose2 = _random_pose(rng, 0.5, 1.0)
    s12 = f32(rng.uniform(0.7, 1.4))
    R12 = synth._rot(rng.normal(0, 1, 3), rng.uniform(0.05, 0.25)).astype(np.float32)
    t12 = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    m = ref.compose(s12, R12, t12)
    X = _directions(rng, n, written, cone) * rng.uniform(2.0, 9.0, (n, 1))                    # physical points, key frame 1's camera coordinates
    Y = X @ m["sR21"].astype(np.float64).T + m["t21"].astype(np.float64)
    inv = lambda pose, P: (P - pose[9:].astype(np.float64)) @ pose[:9].reshape(3, 3).astype(np.float64)      # R^T (P - t)
    pos1 = inv(pose1, X).astype(np.float32); pos2 = inv(pose2, Y).astype(np.float32)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    level = rng.integers(0, 8, n)

    def members(dist, k):
        mx = dist * 1.2 ** (level - rng.uniform(0.1, 0.9, k))
        mn = mx / 1.2 ** 7
        out = rng.random(k) < 0.06
        sd = rng.random(k) < 0.5
        mx = np.where(out & sd, dist / 1.2 * 0.995, mx); mn = np.where(out & ~sd, dist / 0.8 * 1.005, mn)
        return mn.astype(np.float32), mx.astype(np.float32)
    mn1, mx1 = members(np.linalg.norm(Y, axis=1), n)                                          # key frame 1's points are measured in camera 2
    mn2, mx2 = members(np.linalg.norm(X, axis=1), n)
    # the restatement's own projections: where each direction lands
    big = np.full(n, 1e9, np.float32); zero = np.zeros(n, np.float32)
    p12 = ref.project(F, pose1, m["sR21"], m["t21"], pos1, zero, big)
    p21 = ref.project(F, pose2, m["sR12"], m["t12"], pos2, zero, big, second_as_depth=written)

    def keyframe(pr, pose, nk, mp_pos, mn, mx, salt):
        """nk key points: the tracks whose projection exists, then distractors; shuffled"""
        r = np.random.default_rng(seed * 7 + salt)
        ok = np.flatnonzero(pr["drop"] == 0)[:nk]
        t = len(ok)
        kx = np.zeros(nk, np.float32); ky = np.zeros(nk, np.float32); koct = r.integers(0, 8, nk).astype(np.int32)
        kdesc = r.integers(0, 256, (nk, 32), dtype=np.uint8)
        skip = np.ones(nk, np.uint8); pos = np.zeros((nk, 3), np.float32); mnd = np.zeros(nk, np.float32); mxd = np.ones(nk, np.float32)
        mdesc = r.integers(0, 256, (nk, 32), dtype=np.uint8)
        track = np.full(nk, -1, np.int64)
        kx[:t] = pr["u"][ok] + r.uniform(-2, 2, t).astype(np.float32); ky[:t] = pr["v"][ok] + r.uniform(-2, 2, t).astype(np.float32)
        shift = r.choice([0, 0, 0, -1, -1, 1], t)                                             # octave = level or level - 1; a sixth at level + 1 (rejected)
        koct[:t] = np.clip(level[ok] + shift, 0, 7)
        kdesc[:t] = flip_bits(base[ok], r, 6)
        track[:t] = ok
        # distractors: random pixels on the faces; half of them hold a map point of their own with a random descriptor
        d = _directions(r, nk - t, False)
        _, du, dv = ref.rays_to_cubemap(F, d[:, 0].astype(np.float32), d[:, 1].astype(np.float32), d[:, 2].astype(np.float32))
        du = np.where(du < 0, f32(F + 10), du); dv = np.where(dv < 0, f32(F + 10), dv)
        kx[t:] = du; ky[t:] = dv
        # every key point of a track holds its map point; 5 % of them count as matched already or bad
        skip[:t] = r.random(t) < 0.05
        pos[:t] = mp_pos[ok]; mnd[:t] = mn[ok]; mxd[:t] = mx[ok]; mdesc[:t] = flip_bits(base[ok], r, 6)
        own = np.arange(t, nk)[r.random(nk - t) < 0.5]
        skip[own] = 0
        far = _directions(r, len(own), False) * r.uniform(2.0, 9.0, (len(own), 1))
        far[::3, 2] *= -1.0                                                                     # a third of them behind the cameras
        pos[own] = inv(pose, far).astype(np.float32)
        dd = np.linalg.norm(far, axis=1)
        mxd[own] = (dd * 1.2 ** r.uniform(0, 7, len(own))).astype(np.float32); mnd[own] = mxd[own] / f32(1.2 ** 7)
        order = r.permutation(nk)
        kf = dict(kx=kx[order], ky=ky[order], koct=koct[order], kdesc=np.ascontiguousarray(kdesc[order]), pose12=pose)
        mp = dict(skip=skip[order], pos=np.ascontiguousarray(pos[order]), min_dist=mnd[order], max_dist=mxd[order], desc=np.ascontiguousarray(mdesc[order]))
        return kf, mp, track[order]
    kf1, mp1, tr1 = keyframe(p21, pose1, n_kp, pos1, mn1, mx1, 1)
    kf2, mp2, tr2 = keyframe(p12, pose2, n_kp + n2_extra, pos2, mn2, mx2, 2)
    return dict(camd=CAMD, sf=SF, kf1=kf1, kf2=kf2, s12=s12, R12=R12, t12=t12, mp1=mp1, mp2=mp2, th=th, track1=tr1, track2=tr2)


SIZES = (61, 257, 1031)


def family(written):
    """the seeded cases of one family, smallest first"""
    return [seeded(n, 100 + 10 * k + (5 if written else 0), written) for k, n in enumerate(SIZES)]


def dense_case():
    """1031 key points per side inside a cone of a few degrees: every window holds a few hundred candidates, far beyond the 64 per entry the first
    attempt reserves"""
    return seeded(1031, 77, False, cone=0.06)


def self_case(c):
    """key frame 1 of a case against itself under the identity similarity (slot1 == slot2)"""
    return dict(c, kf2=c["kf1"], mp2=c["mp1"], s12=f32(1.0), R12=EYE.copy(), t12=np.zeros(3, np.float32))


def empty_side_case(c, first):
    """the case with a key frame without key points on one side"""
    ekf = dict(kx=np.zeros(0, np.float32), ky=np.zeros(0, np.float32), koct=np.zeros(0, np.int32), kdesc=np.zeros((0, 32), np.uint8), pose12=IDENT.copy())
    emp = dict(skip=np.zeros(0, np.uint8), pos=np.zeros((0, 3), np.float32), min_dist=np.zeros(0, np.float32), max_dist=np.zeros(0, np.float32), desc=np.zeros((0, 32), np.uint8))
    return dict(c, kf1=ekf, mp1=emp) if first else dict(c, kf2=ekf, mp2=emp)
