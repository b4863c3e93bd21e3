"""LoopClosing as ONE composite: a synthetic map with a known similarity drift, and a chain that runs DetectLoop -> ComputeSim3 -> CorrectLoop ->
RunGlobalBundleAdjustment over it through a backend, each stage fed by the previous stage's OUTPUT, with the arguments INTEGRATION.md items 22-27
prescribe.  The pattern is covis_cases.run(case, backend) / kfdb_cases.run(ops, backend): HostBackend answers every step from the CPU reference that
stage's own GPU test compares against, DeviceBackend from api.* on two contexts and one KeyframeStore.  The glue (this file's Python) is shared by
both backends on purpose: it is judged by the truth and by tests/npref_loop_closing.py, not by the backend comparison.

The scene (scene(seed)): camera synth.camera("lafida", 550), 8 levels, factor 1.2; 12 key frames of at most 400 key points, 520 + 420 physical points
0.5 to 1.2 m away on all five faces, key frames up to T_MAX = 0.4 m per axis and 10 degrees from the origin (the points are near and the baselines
wide because the truth bars below are bounded by the depth a few views of +-0.5 px can give).  An old side A0..A4 and a current side C0..C4 see the
same NS points; the old side is a covisibility chain (A_k sees the points [k, k + 2) * A_WINDOW: neighbours share points, others none), the current
side sees all of them, C0 only a few under many distractors (the covisible that sets DetectLoop's minScore).  E0 and E1 see a disjoint set.  The
old side's map points sit at the truth X with ids p; the current side has its own points, ids CUR_ID + p, at D(X) = sD RD X + tD (sD = 1.08,
4 degrees, 0.15 m), and its poses are drifted consistently (Rcw' = Rcw RD^T, tcw' = sD tcw - Rcw' tD: the same pixels, camera coordinates scaled by
sD), so each side is self-consistent and only the loop reveals D.  Key points: the truth's projection + uniform +-0.5 px; a view's descriptor: the
point's base descriptor with at most 6 bits flipped; the octave follows from the distance; a third of the key points are distractors, and a key
point that would be a point's only observation holds none either.  A fifth of the shared points look like the point three windows on (the same
base descriptor): SearchByBoW's outliers, so that the solver's inlier mask is not all ones.  E0 carries COPY_E0 descriptors (and angles) of shared
points on key points whose map points lie elsewhere: >= 20 SearchByBoW matches with C4 on 3-D points that fit no similarity, so its solver walks
all its iterations (bNoMore); E1 carries COPY_E1 of them, and LOOKALIKE_E1 more on key points WITHOUT a map point (the database sees them: E0's
accumulated score; SearchByBoW does not: E1 stays below 20).  Map points carry min_dist / max_dist / normal / desc from
orc.update_normal_and_depth / orc.distinctive_descriptors.  Vocabulary: vocab_cases.case_tree("k10_L3") with LEVELSUP = 1 (FeatureVector nodes at
level 2: up to 100 nodes, a few features each); the base descriptors are drawn near its leaves (vocab_cases.descriptors).

What the chain does where LoopClosing's text leaves a choice or the scene needs one, and why:
  * DetectLoop runs for C1, C2, C3, C4: with mnCovisibilityConsistencyTh = 3 (LoopClosing.cpp:43) a group's counter reaches 3 at the FOURTH
    consecutive detection (:185-197 start from 0); three calls can never fill mvpEnoughConsistentCandidates.
  * The accepted chain never takes E0 to bNoMore (the true candidate wins the first pass, :337); run_rejected, with [E0, E1] as its candidates, does.
  * SearchBySim3 as the bridge passes it (z_as_written) finds next to nothing on honest key points: line :1507 takes y for the depth.  The same jobs
    run once more with component 2, recorded and not consumed; and the whole chain runs a second time with zw = False ("fixed" in the tests), where
    the matcher's answers ARE written into the match list (14 and 9 key points) and everything behind it consumes them.
  * Nothing is fetched from the store between an entry that writes it and an entry that reads it, unless probe asks for it: ComputeBoW's vectors are
    read back at the end of a chain, rows and poses once behind the last search.
  * UpdateNormalAndDepth runs once behind the point loop of :470-500, not inside it (the reference reads a mix of corrected and uncorrected poses
    there); KeyFrameAndPose is walked by mnId (the reference walks it by pointer).
  * Two spanning trees (PARENTS): "jump" is the one a run would have and gives the pose graph work; "split" is the one that can end on the truth.
  * No covisibility weight of the OLD side reaches 100 at this size; the current side's do (up to 162), and its covisibility edges are in the graph.
  * tD's direction was chosen among 60 seeded ones, like the seed: one for which every optimiser's iteration count is the same in the chain and in
    the float64 restatement and the truth bars keep their margin (17 of the 60; for the others a stop rule decides on a difference of 1e-6 m),
    and among those the one with the most essential-graph work.

Counts the reference chain (HostBackend) reached on SEED = 157, against LoopClosing's thresholds (tests/test_loop_closing_cpu.py prints and asserts):
  DetectLoop: C4's consistent candidates A2, E0, A4 (candidates of C1..C4: [A0 E0] [A0 E0] [A2 E0 A0] [A2 E0 A4]).  SearchByBoW: 42, 38, 27 (>= 20).
  Sim3Solver pass 1: hypotheses for A2 (33 of 42 correspondences) and A4 (21 of 27), none for E0.  SearchBySim3 as written 0 and 0, with component 2
  14 and 9.  OptimizeSim3: 33 and 21 inliers (>= 20): A2 is matched ("fixed": 47 and 30).  SearchByProjection(Scw): 84 more, 117 matches over 273
  loop points (>= 40).  Loop fusion: 106 replaced, 11 added.  SearchAndFuse: 97 replaced, 37 added.  C1..C4 gain links to A0..A4, C0 none.
  Essential graph: 12 vertices, 15 edges, 5 iterations ("jump": chi2 0.0203 -> 0.0037).  Global BA: 566 points, 1778 edges, 6 iterations.  Rejected
  pass: SearchByBoW 38 and 10; E0 walks its 30 iterations in 6 passes; false at :343-349.

Measured on the CPU (tests/test_loop_closing_cpu.py prints them); every bar is twice the measured value:
  host chain against the float64 restatement of the glue, largest absolute difference ("jump" / "split" where they differ): Scw 1.49e-8; corrected
  points 1.19e-7 m; corrected poses 2.98e-8; points behind the essential graph 8.34e-7 / 1.19e-7 m, poses 6.97e-7 / 7.45e-9; final points 6.42e-5 /
  1.25e-4 m, final centres 5.29e-7 / 3.15e-6 m.  "fixed": 1.1e-4 to 2.1e-4 everywhere (Scw 1.33e-4): with SearchBySim3's noisy key points among
  the correspondences OptimizeSim3 moves, and its numeric Jacobian carries the float rounding of its inputs into the result.  Every discrete output
  is equal, the optimisers' iteration counts included; one count is not compared, the essential graph's on "split", where Levenberg starts at
  chi2 ~ 1e-14 and the count is noise by construction (the test says so).
  truth, RMS metres, nothing removed ("split"; all twelve key frames, all points): Scw X against sD (R X + t) over the shared points 3.16e-5
  (identity: 0.403); centres before 0.102, restatement 3.94e-4, host 3.94e-4; points before 0.149, restatement 2.94e-3, host 2.94e-3.  With "jump"
  the host chain ends at centres 4.5e-3 and points 1.07e-2 (old and current side): the graph spreads one edge's drift, and a BA that fixes key
  frame 0 alone does not give the scale back.
"""
import numpy as np

import covis_hostlib
import ess_graph_hostlib
import gba_hostlib
import kfdb_cases as kc
import kfdb_hostlib
import npref_bow_kf
import npref_essential_graph as ne
import npref_global_ba
import npref_reloc
import npref_sim3_opt as ns
import npref_sim3_projection
import npref_sim3_search
import orc
import sim3_cases
import sim3_hostlib
import sim3_opt_hostlib
import vocab_cases as vc
import vocab_hostlib
from cubemapslam_amd import api, harness, synth
from reloc_cases import flip_bits

F = 550
CAMD = synth.camera("lafida", F)
SF = npref_reloc.scale_factors(1.2, 8)
SIGMA2 = (SF * SF).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)
SEED = 157
NS, NE = 520, 420                      # shared physical points, points only E0 / E1 see
CUR_ID, E_ID = 100000, 200000          # ids of the current side's and of the elsewhere map points
A_WINDOW = NS // 6                     # A_k sees the points [k, k + 2) * A_WINDOW
COPY_E0, COPY_E1, LOOKALIKE_E1 = 230, 12, 25
LEVELSUP = 1
K_SLOTS, MAXF, MAX_NODES = 16, 512, 256
NAMES = ["A0", "A1", "A2", "A3", "A4", "E0", "E1", "C0", "C1", "C2", "C3", "C4"]
MN_ID = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13]      # C0 is younger than mLastLoopKFid + 10 (LoopClosing.cpp:113), C1..C4 are not
SLOTS = [(3 + 5 * m) % K_SLOTS for m in range(12)]    # slot != member position
CURRENT = 11                           # C4
DETECT = [8, 9, 10, 11]                # C1..C4
S_D, ANG_D, T_D = 1.08, np.deg2rad(4.0), np.array([0.048, -0.067, 0.125])
RANSAC = (0.99, 20, 300)
D_MIN, D_MAX, D_REF, T_MAX = 0.5, 1.2, 0.85, 0.4      # point distances, the distance of octave 3, the key frames' largest offset per axis (metres)
CONSISTENCY_TH = 3                     # mnCovisibilityConsistencyTh (LoopClosing.cpp:43)
f32 = np.float32
# The bars (twice what tests/test_loop_closing_cpu.py measures on the float64 restatement; the header above has the measurements)
SCW_BAR, CENTRE_BAR, POINT_BAR = 6.4e-5, 7.9e-4, 5.9e-3      # metres RMS: the recovered Scw over the shared points; key-frame centres and map points at the end ("split")
GLUE_BARS = dict(jump=dict(Scw=3.0e-8, corrected_pos=2.4e-7, corrected_poses=6.0e-8, eg_pos=1.7e-6, eg_poses=1.4e-6, final_pos=1.3e-4, final_centres=1.1e-6),
                 split=dict(Scw=3.0e-8, corrected_pos=2.4e-7, corrected_poses=6.0e-8, eg_pos=2.4e-7, eg_poses=1.5e-8, final_pos=2.5e-4, final_centres=6.3e-6),
                 fixed=dict(Scw=2.7e-4, corrected_pos=4.3e-4, corrected_poses=2.5e-4, eg_pos=3.2e-4, eg_poses=2.3e-4, final_pos=2.2e-4, final_centres=1.5e-4))


# ------------------------------------------------------------------------------------------------------------------------------- the scene
def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = np.where(d[:, 2] < 0.3, 0.6 - d[:, 2], d[:, 2])       # in front of the key frames and on the four side faces, inside the field of view
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(D_MIN, D_MAX, (n, 1))


def _pose(rng, first=False):
    if first:
        return np.eye(3), np.zeros(3)
    return synth._rot(rng.normal(size=3), rng.uniform(0.0, np.deg2rad(10.0))), rng.uniform(-T_MAX, T_MAX, 3)


def scene(seed=SEED, perturb=0.0):
    """deterministic; perturb: every physical point moved by that many metres in a seeded direction before anything is derived (the tameness test)"""
    rng = np.random.default_rng(seed)
    tree = vc.case_tree("k10_L3")
    base = vc.descriptors(seed + 1, tree, NS + NE, near=1.0, flips=6)
    pang = rng.uniform(0, 360, NS + NE)
    twin = rng.choice(NS, NS // 5, replace=False)                  # repeated texture: a fifth of the shared points look like the point 3 windows on,
    other = (twin + 3 * A_WINDOW) % NS                             # which no old key frame sees together with them: SearchByBoW's outliers
    fresh = ~np.isin(other, twin)
    base[other[fresh]] = base[twin[fresh]]; pang[other[fresh]] = pang[twin[fresh]]
    X = np.concatenate([_directions(rng, NS), _directions(rng, NE)])
    if perturb:
        X = X + np.random.default_rng(seed + 99).normal(size=X.shape) * perturb
    RD = synth._rot([0.3, 1.0, -0.2], ANG_D)
    drift = lambda P: S_D * P @ RD.T + T_D
    kfs, true_poses = [], []
    for m, name in enumerate(NAMES):
        R, t = _pose(rng, first=(m == 0))
        true_poses.append((R, t))
        side = name[0]
        if side == "A":                                            # a chain: A_k shares points with A_k-1 and A_k+1 only
            pts, p_vis = np.arange(m * A_WINDOW, (m + 2) * A_WINDOW), 0.9
        elif name == "C0":                                         # few shared points under many distractors: the covisible that sets DetectLoop's minScore
            pts, p_vis = np.arange(NS // 8), 0.9
        else:
            pts, p_vis = (np.arange(NS) if side == "C" else np.arange(NS, NS + NE)), 0.55
        Xc = X[pts] @ R.T + t
        face, up, vp = synth.rays_to_cubemap(F, Xc)
        vis = np.flatnonzero((face >= 0) & (rng.random(len(pts)) < p_vis))
        u = (up[vis] + rng.uniform(-0.5, 0.5, len(vis))).astype(f32); v = (vp[vis] + rng.uniform(-0.5, 0.5, len(vis))).astype(f32)
        ok = synth.face_of_pixel(F, u.astype(np.float64), v.astype(np.float64)) == face[vis]
        vis, u, v = vis[ok][:266], u[ok][:266], v[ok][:266]
        n = len(vis)
        depth = np.linalg.norm(Xc[vis], axis=1)
        octave = np.clip(np.round(np.log(D_REF / depth) / np.log(1.2) + 3), 0, 7).astype(np.int32)
        phys = pts[vis]
        desc = flip_bits(base[phys], rng, 6)
        angle = (pang[phys] + rng.uniform(-3, 3, n)) % 360.0
        mp = {"A": phys, "C": CUR_ID + phys, "E": E_ID + (phys - NS)}[side].astype(np.int32)
        if side == "E":                                            # descriptors and angles of shared points on key points whose map points lie elsewhere
            c = min(COPY_E0 if name == "E0" else COPY_E1, n)
            src = rng.choice(NS, c, replace=False)
            desc[:c] = flip_bits(base[src], rng, 6); angle[:c] = (pang[src] + rng.uniform(-3, 3, c)) % 360.0
        nd = 399 - n if name in ("C0", "E1") else n // 2           # distractors: a third of the key points
        origin = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)], np.float64)[rng.integers(0, 5, nd)] * F
        duv = origin + rng.uniform(4, F - 4, (nd, 2))
        x = np.concatenate([u, duv[:, 0].astype(f32)]); y = np.concatenate([v, duv[:, 1].astype(f32)])
        octave = np.concatenate([octave, rng.integers(0, 8, nd).astype(np.int32)])
        ddesc = rng.integers(0, 256, (nd, 32)).astype(np.uint8)
        if name == "E1":                                           # E1 looks like the shared scene to the database (E0's accumulated score) but its look-alikes hold no map point
            ddesc[:LOOKALIKE_E1] = flip_bits(base[rng.choice(NS, LOOKALIKE_E1, replace=False)], rng, 6)
        desc = np.concatenate([desc, ddesc])
        angle = np.concatenate([angle, rng.uniform(0, 360, nd)]).astype(f32)
        mp = np.concatenate([mp, np.full(nd, -1, np.int32)])
        order = rng.permutation(n + nd)
        if side == "C":                                            # the drifted pose: the same pixels, camera coordinates scaled by sD
            Rm = R @ RD.T; tm = S_D * t - Rm @ T_D
        else:
            Rm, tm = R, t
        Rm = Rm.astype(f32); tm = tm.astype(f32)
        Ow = (-(Rm.astype(np.float64).T @ tm.astype(np.float64))).astype(f32)
        assert n + nd <= 400
        kfs.append(dict(name=name, mn_id=MN_ID[m], slot=SLOTS[m], x=x[order], y=y[order], octave=octave[order], angle=angle[order], desc=np.ascontiguousarray(desc[order]),
                        mp=mp[order], R=Rm, t=tm, Ow=Ow, pose12=np.concatenate([Rm.reshape(-1), tm]).astype(f32)))
    # ---- the map points: id -> position, observations in key-frame order; the attributes UpdateNormalAndDepth / ComputeDistinctiveDescriptors give
    seen = {}
    for kf in kfs:
        for pid in kf["mp"][kf["mp"] >= 0]:
            seen[int(pid)] = seen.get(int(pid), 0) + 1
    for kf in kfs:                                                 # a map point has two observations at least; a key point that would be its only one holds none
        kf["mp"] = np.array([pid if pid >= 0 and seen[int(pid)] >= 2 else -1 for pid in kf["mp"]], np.int32)
    obs = {}
    for m, kf in enumerate(kfs):
        for f_, pid in enumerate(kf["mp"]):
            if pid >= 0:
                obs.setdefault(int(pid), []).append((m, f_))
    ids = np.array(sorted(obs), np.int64)
    phys = np.where(ids >= E_ID, ids - E_ID + NS, ids % CUR_ID)
    pos = np.where(((ids >= CUR_ID) & (ids < E_ID))[:, None], drift(X[phys]), X[phys]).astype(f32)
    obs_off = np.concatenate([[0], np.cumsum([len(obs[int(i)]) for i in ids])]).astype(np.int32)
    odesc = np.concatenate([np.stack([kfs[k]["desc"][f_] for k, f_ in obs[int(i)]]) for i in ids])
    oOw = np.concatenate([np.stack([kfs[k]["Ow"] for k, f_ in obs[int(i)]]) for i in ids]).astype(f32)
    refOw = np.stack([kfs[obs[int(i)][0][0]]["Ow"] for i in ids]).astype(f32)
    reflev = np.array([kfs[obs[int(i)][0][0]]["octave"][obs[int(i)][0][1]] for i in ids], np.int32)
    best = orc.distinctive_descriptors(obs_off, odesc)
    normal, dmin, dmax = orc.update_normal_and_depth(obs_off, pos, oOw, refOw, reflev, SF)
    points = dict(ids=ids, row={int(i): r for r, i in enumerate(ids)}, pos=pos, normal=normal, min_dist=dmin, max_dist=dmax,
                  desc=np.ascontiguousarray(np.stack([odesc[obs_off[r] + best[r]] for r in range(len(ids))])), obs=obs)
    draws = {m: sim3_cases.draws(seed + 1000 + m, 400, RANSAC[2] + 5) for m in range(12)}      # uniform numbers; a solver of N takes them modulo N - k (below)
    return dict(seed=seed, tree=tree, kfs=kfs, points=points, X=X, true_poses=true_poses, drift=(S_D, RD, T_D), draws=draws)


def true_scw(sc, m=CURRENT):
    """the similarity that takes the old map's world into key frame m's (drifted, hence scaled) camera: [sD R | sD t] of its true pose"""
    R, t = sc["true_poses"][m]
    return np.hstack([S_D * R, (S_D * t)[:, None]])


def scw_error(sc, Scw, m=CURRENT):
    """RMS distance, over the shared physical points, between Scw X and the truth's sD (R X + t): metres in the current key frame's camera"""
    S = np.asarray(Scw, np.float64).reshape(-1)[:12].reshape(3, 4); T = true_scw(sc, m)
    X = sc["X"][:NS]
    d = (X @ S[:, :3].T + S[:, 3]) - (X @ T[:, :3].T + T[:, 3])
    return float(np.sqrt((d * d).sum(1).mean()))


def solver_draws(sc, m, N):
    """the recorded draws of candidate m for a solver of N correspondences: DUtils::Random::RandomInt(0, size - 1), three per iteration"""
    d = sc["draws"][m].astype(np.int64)
    return np.stack([d[:, k] % (N - k) for k in range(3)], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------- glue helpers
def gather(points, ids):
    r = np.array([points["row"][int(i)] for i in ids], np.int64)
    return {k: points[k][r] for k in ("pos", "normal", "min_dist", "max_dist", "desc")}


def per_keypoint(points, kf, extra_skip=None):
    """what cms_kfstore_search_by_sim3 wants per key point of a key frame: skip, pos, min_dist, max_dist, desc"""
    n = len(kf["mp"])
    has = kf["mp"] >= 0
    r = np.array([points["row"][int(i)] if i >= 0 else 0 for i in kf["mp"]], np.int64)
    skip = (~has).astype(np.uint8)
    if extra_skip is not None:
        skip |= np.asarray(extra_skip, np.uint8)
    return dict(skip=skip, pos=points["pos"][r], min_dist=points["min_dist"][r], max_dist=points["max_dist"][r], desc=points["desc"][r]), n


def index_in_keyframe(points, pid, m):
    """MapPoint::GetIndexInKeyFrame"""
    for k, f_ in points["obs"][int(pid)]:
        if k == m:
            return f_
    return -1


def tcw(kf):
    return np.hstack([kf["R"].reshape(3, 3), kf["t"].reshape(3, 1)]).astype(f32)


def solver_problem(sc, m1, m2, idx2):
    """Sim3Solver's constructor (Sim3Solver.cpp:66-127) on SearchByBoW's answer idx2 (key points of key frame m2 per key point of m1): the kept key
    points of key frame 1 in order (mvnIndices1) and the job arrays"""
    k1, k2, P = sc["kfs"][m1], sc["kfs"][m2], sc["points"]
    keep = [i1 for i1 in range(len(idx2)) if idx2[i1] >= 0 and k1["mp"][i1] >= 0 and k2["mp"][idx2[i1]] >= 0]
    r1 = np.array([P["row"][int(k1["mp"][i])] for i in keep], np.int64); r2 = np.array([P["row"][int(k2["mp"][idx2[i]])] for i in keep], np.int64)
    x1 = sim3_hostlib.camera_points(tcw(k1), P["pos"][r1]); x2 = sim3_hostlib.camera_points(tcw(k2), P["pos"][r2])
    ok = sim3_cases.in_a_face(x1) & sim3_cases.in_a_face(x2) if len(keep) else np.zeros(0, bool)
    keep = np.array(keep, np.int64)[ok]
    i2 = np.asarray(idx2)[keep]
    return keep, dict(x3dc1=x1[ok], x3dc2=x2[ok], max_err1=sim3_cases.max_error(SIGMA2[k1["octave"][keep]]), max_err2=sim3_cases.max_error(SIGMA2[k2["octave"][i2]]))


def opt_problem(sc, m1, m2, match_id, R, t, s):
    """the graph of Optimizer.cpp:941-978 over vpMatches1 = match_id (map-point ids of key frame m2 per key point of m1, -1 = NULL)"""
    k1, k2, P = sc["kfs"][m1], sc["kfs"][m2], sc["points"]
    idx = [i for i in range(len(match_id)) if match_id[i] >= 0 and k1["mp"][i] >= 0 and index_in_keyframe(P, match_id[i], m2) >= 0]
    i2 = np.array([index_in_keyframe(P, match_id[i], m2) for i in idx], np.int64); idx = np.array(idx, np.int64)
    r1 = np.array([P["row"][int(k1["mp"][i])] for i in idx], np.int64); r2 = np.array([P["row"][int(match_id[i])] for i in idx], np.int64)
    return idx, dict(x3dc1=sim3_hostlib.camera_points(tcw(k1), P["pos"][r1]), x3dc2=sim3_hostlib.camera_points(tcw(k2), P["pos"][r2]),
                     kp1=np.stack([k1["x"][idx], k1["y"][idx]], 1), kp2=np.stack([k2["x"][i2], k2["y"][i2]], 1), inv_sigma2_1=INV_SIGMA2[k1["octave"][idx]],
                     inv_sigma2_2=INV_SIGMA2[k2["octave"][i2]], R12=np.asarray(R, np.float64).reshape(3, 3), t12=np.asarray(t, np.float64), s12=float(s), fix_scale=0)


def quat_to_R(q):
    """Eigen::Quaterniond(w, x, y, z).toRotationMatrix() of q = (x y z w), in double"""
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def compose_scw(q12, t12, s12, kf_m):
    """mg2oScw = gScm * gSmw with gSmw = (Rmw, tmw, 1.0) (LoopClosing.cpp:332-334), mScw = toCvMat: [s R | t] narrowed to float"""
    Rcm = quat_to_R(q12); Rmw = kf_m["R"].astype(np.float64).reshape(3, 3); tmw = kf_m["t"].astype(np.float64)
    R = Rcm @ Rmw
    t = float(s12) * (Rcm @ tmw) + np.asarray(t12, np.float64)
    return np.hstack([float(s12) * R, t[:, None]]).astype(f32), (R, t, float(s12))


# ------------------------------------------------------------------------------------------------------------------------------- the chain
def detect_loop(sc, be, conn, out):
    """DetectLoop for C1..C4 in turn (LoopClosing.cpp:102-228) -> mvpEnoughConsistentCandidates of the last one, as members"""
    slot_of = SLOTS; member_of = {s: m for m, s in enumerate(SLOTS)}
    groups = []                                                    # mvConsistentGroups: (set of members, counter)
    enough = []
    for cur in DETECT:
        assert sc["kfs"][cur]["mn_id"] >= 0 + 10                   # :113 (mLastLoopKFid = 0)
        connected = conn[cur]                                      # GetVectorCovisibleKeyFrames
        scores = be.bow_score([slot_of[cur]] * len(connected), [slot_of[c] for c in connected])
        min_score = f32(1.0)
        for s in scores:                                           # :126-137
            s = f32(s)
            if s < min_score:
                min_score = s
        res = be.detect([kc.job(kc.LOOP, ("slot", slot_of[cur]), min_score=min_score, connected=[slot_of[c] for c in connected])])[0]
        cands = [member_of[s] for s in res[0]]
        out.append(("DetectLoop %s" % sc["kfs"][cur]["name"], dict(score_bits=np.asarray(scores, np.float64), min_score=min_score, candidates=cands,
                                                                  common_words=np.asarray(res[1]), score=np.asarray(res[2]))))
        enough = []
        if not cands:                                              # :143-149
            be.db_add([slot_of[cur]]); groups = []
            continue
        current, seen = [], [False] * len(groups)
        for c in cands:                                            # :159-207
            group = set(conn[c]) | {c}
            is_enough = some = False
            for g, (prev, n_prev) in enumerate(groups):
                if group & prev:
                    some = True
                    if not seen[g]:
                        current.append((group, n_prev + 1)); seen[g] = True
                    if n_prev + 1 >= CONSISTENCY_TH and not is_enough:
                        enough.append(c); is_enough = True
            if not some:
                current.append((group, 0))
        groups = current
        be.db_add([slot_of[cur]])                                  # :214
        out[-1][1].update(enough=list(enough), group_counters=[n for _, n in groups])
    return enough


def compute_sim3(sc, be, conn, candidates, out, cur=CURRENT, zw=True):
    """ComputeSim3 (LoopClosing.cpp:230-399) -> dict(accepted, matched member, Scw (float 3 x 4), g = mg2oScw (R, t, s in double), matches =
    mvpCurrentMatchedPoints as ids per key point, loop_ids = mvpLoopMapPoints).  zw: SearchBySim3's z_as_written"""
    kfs, P = sc["kfs"], sc["points"]
    k1 = kfs[cur]; n1 = len(k1["mp"])
    # ---- :251-279 SearchByBoW(mpCurrentKF, pKF) for every candidate in one call, then the solvers
    res = be.search_by_bow([(SLOTS[cur], n1, SLOTS[c], len(kfs[c]["mp"]), None, None) for c in candidates])
    out.append(("SearchByBoW", dict(idx2=[r[0] for r in res], n=[r[1] for r in res])))
    solvers = {}
    for c, (idx2, nm) in zip(candidates, res):
        if nm < 20:
            continue
        keep, prob = solver_problem(sc, cur, c, idx2)
        N = len(keep)
        prob.update(fix_scale=0, min_inliers=RANSAC[1], max_its=api.sim3_ransac_parameters(N, *RANSAC) if N else 0)
        solvers[c] = dict(keep=keep, prob=prob, idx2=np.asarray(idx2), carried={}, draws=solver_draws(sc, c, N) if N > 2 else np.zeros((0, 3), np.int32))
    live = [c for c in candidates if c in solvers]
    out.append(("Sim3Solver set-up", dict(live=list(live), N=[len(solvers[c]["keep"]) for c in live], max_its=[solvers[c]["prob"]["max_its"] for c in live],
                                          indices1=[solvers[c]["keep"] for c in live])))
    n_pass = 0
    while live:                                                    # :285-341
        n_pass += 1
        states = []
        for c in live:
            s = solvers[c]
            it = s["carried"].get("iterations", 0)
            states.append(api.sim3_job_state(dict(s["prob"], **s["carried"]), 5, s["draws"][it:]))
        rs = be.sim3_iterate(states)
        rec = dict(live=list(live), status=[r["status"] for r in rs], no_more=[r["no_more"] for r in rs], n_inliers=[r["n_inliers"] for r in rs],
                   iterations=[r["iterations"] for r in rs], inliers=[r["inliers"] for r in rs], best_R=[r["best_R"] for r in rs], best_t=[r["best_t"] for r in rs],
                   best_s=[r["best_s"] for r in rs], T12=[r["T12"] for r in rs])
        out.append(("Sim3Solver pass %d" % n_pass, rec))
        hyps = []
        for c, r in zip(list(live), rs):
            s = solvers[c]
            s["carried"] = dict(iterations=r["iterations"], best_inliers=r["best_inliers"], best_mask=r["best_mask"].copy(), best_s=float(r["best_s"][0]),
                                best_R=r["best_R"].copy(), best_t=r["best_t"].copy(), best_T12=r["best_T12"].copy())
            if r["no_more"]:                                       # :303-307
                live.remove(c)
            if r["status"] == 1:                                   # :310-317: the inlier matches, as map-point ids of the candidate
                match_id = np.full(n1, -1, np.int64)
                inl = s["keep"][r["inliers"][:len(s["keep"])] != 0]
                match_id[inl] = kfs[c]["mp"][s["idx2"][inl]]
                hyps.append((c, match_id, r["best_R"].reshape(3, 3).copy(), r["best_t"].copy(), f32(r["best_s"][0])))
        if not hyps:
            continue
        # ---- :322 SearchBySim3 for every hypothesis of the pass in one call; vbAlreadyMatched1 / 2 as :1390-1400
        jobs = []
        for c, match_id, R, t, s_ in hyps:
            am1 = (match_id >= 0).astype(np.uint8)
            am2 = np.zeros(len(kfs[c]["mp"]), np.uint8)
            for pid in match_id[match_id >= 0]:
                i2 = index_in_keyframe(P, pid, c)
                if i2 >= 0:
                    am2[i2] = 1
            mp1, _ = per_keypoint(P, k1, am1); mp2, _ = per_keypoint(P, kfs[c], am2)
            jobs.append(dict(slot1=SLOTS[cur], slot2=SLOTS[c], s12=s_, R12=R, t12=t, mp1=mp1, mp2=mp2, member2=c))
        found = be.search_by_sim3(jobs, z_as_written=zw)
        for (c, match_id, R, t, s_), (idx2, nf) in zip(hyps, found):
            new = np.flatnonzero(np.asarray(idx2) >= 0)
            assert (match_id[new] < 0).all()                       # a key point already matched is skipped
            match_id[new] = kfs[c]["mp"][np.asarray(idx2)[new]]
        out.append(("SearchBySim3 pass %d" % n_pass, dict(candidates=[h[0] for h in hyps], idx2=[f[0] for f in found], n_found=[f[1] for f in found],
                                                          matches=[h[1].copy() for h in hyps])))
        if zw:
            # (as written, line :1507 takes y for the depth of direction 2 -> 1 and next to nothing is mutual on honest key points; the same jobs
            # with component 2 show that the solver's s12 / R12 / t12 mean to the matcher what they mean to the solver.  Recorded, not consumed:
            # the chain with zw = False is the one that consumes them.)
            fixed = be.search_by_sim3(jobs, z_as_written=False)
            out.append(("SearchBySim3 pass %d, component 2" % n_pass, dict(idx2=[f[0] for f in fixed], n_found=[f[1] for f in fixed])))
        # ---- :324-326 OptimizeSim3 (th2 = 10) for every hypothesis of the pass in one call
        probs = [opt_problem(sc, cur, c, match_id, R, t, s_) for c, match_id, R, t, s_ in hyps]
        ro = be.sim3_optimize([api.sim3_opt_job_state(p, th2=10.0) for _, p in probs])
        out.append(("OptimizeSim3 pass %d" % n_pass, dict(candidates=[h[0] for h in hyps], n_inliers=[r["n_inliers"] for r in ro], n_correspondences=[r["n_correspondences"] for r in ro],
                                                          iterations=[r["iterations"] for r in ro], keep=[r["keep"] for r in ro], q12=[r["q12"] for r in ro],
                                                          t12=[r["t12"] for r in ro], s12=[r["s12"] for r in ro])))
        for (c, match_id, R, t, s_), (idx, _), r in zip(hyps, probs, ro):
            match_id[idx[r["keep"][:len(idx)] == 0]] = -1          # vpMatches1[idx] = NULL (Optimizer.cpp:1046 and the second round's)
        out[-1][1]["matches"] = [h[1].copy() for h in hyps]
        for (c, match_id, R, t, s_), r in zip(hyps, ro):
            if r["n_inliers"] >= 20:                               # :328-338: the first in candidate order
                Scw, g = compose_scw(r["q12"], r["t12"], r["s12"][0], kfs[c])
                out.append(("Scw", dict(matched=c, Scw=Scw, matches=match_id.copy(), passes=n_pass)))
                return finish_sim3(sc, be, conn, c, Scw, g, match_id, out, cur)
    out.append(("ComputeSim3", dict(accepted=False, passes=n_pass, at=":343-349")))
    return dict(accepted=False)


def finish_sim3(sc, be, conn, matched, Scw, g, match_id, out, cur=CURRENT):
    """:351-397: the loop map points of the matched key frame and its covisibles, SearchByProjection(Scw, th = 10), accept at >= 40"""
    kfs, P = sc["kfs"], sc["points"]
    members = list(conn[matched]) + [matched]
    rc, n_out, lists = be.local_points([members], cap=K_SLOTS * MAXF)
    assert rc == 0
    loop_ids = np.array(lists[0], np.int64)                        # first-occurrence order over the key frames' rows (:355-371)
    pts = gather(P, loop_ids)
    found_already = set(int(i) for i in match_id[match_id >= 0])
    skip = np.array([int(i) in found_already for i in loop_ids], np.uint8)      # spAlreadyFound (ORBMatcher.cpp:805-806, :817)
    job = dict(slot=SLOTS[cur], n=len(kfs[cur]["mp"]), Scw=Scw, set=0, skip=skip, taken=(match_id >= 0).astype(np.uint8), member=cur)
    match_kp, nm = be.search_by_projection_sim3([pts], [job])[0]
    for j in np.flatnonzero(np.asarray(match_kp) >= 0):
        assert match_id[match_kp[j]] < 0
        match_id[match_kp[j]] = loop_ids[j]
    total = int((match_id >= 0).sum())
    out.append(("SearchByProjection(Scw)", dict(members=members, loop_ids=loop_ids, match_kp=np.asarray(match_kp), n_matches=nm, total=total, accepted=total >= 40,
                                                matches=match_id.copy())))
    return dict(accepted=total >= 40, matched=matched, Scw=Scw, g=g, matches=match_id, loop_ids=loop_ids)


def read_bow(be):
    return dict(bow=[be.fetch_bow(SLOTS[m]) for m in range(12)])


def setup(sc, be, out, probe=False):
    """ComputeBoW of all key frames, the database (everything older than C1), the covisibility index, the covisibles -> connections per member.  The
    vectors ComputeBoW made are read back at the END of a chain (a fetch waits for the store's stream, which the database and the searches on the
    other context must do by themselves); probe: at once as well"""
    be.load(sc)
    if probe:
        out.append(("ComputeBoW, read at once", read_bow(be)))
    be.db_add([SLOTS[m] for m in range(12) if m not in DETECT])
    be.covis_build(SLOTS)
    w, order, nc = be.connections(list(range(12)), 15)
    conn = [[int(x) for x in order[m, :nc[m]]] for m in range(12)]
    neigh = np.full((12, 10), -1, np.int32)
    for m in range(12):
        best = conn[m][:10]
        neigh[m, :len(best)] = [SLOTS[c] for c in best]
    be.db_set_covisibles(SLOTS, neigh)
    out.append(("Covisibility", dict(weights=np.asarray(w), order=np.asarray(order), n_connected=np.asarray(nc))))
    return conn


def run(sc, be, upto_sim3=False, tree="jump", probe=False, zw=True):
    """the accepted chain -> [(stage name, outputs)]; upto_sim3: stop behind ComputeSim3; tree: the spanning tree (PARENTS).  probe: read the store's
    rows and poses back after every rewrite.  A read-back waits for the store's stream, which a search on another context's stream must do by itself:
    the chain that is compared runs WITHOUT it (the store is read once, behind the last search), a second run with it shows where a row went wrong.
    zw: SearchBySim3's z_as_written; False is the chain of a maintainer who fixes line :1507, in which SearchBySim3's matches are consumed."""
    out = []
    conn = setup(sc, be, out, probe)
    enough = detect_loop(sc, be, conn, out)
    res = compute_sim3(sc, be, conn, enough, out, zw=zw)
    out.append(("ComputeSim3", dict(accepted=bool(res["accepted"]), matched=res.get("matched", -1))))
    if res["accepted"] and upto_sim3 is False:
        st = MapState(sc, probe)
        loop = correct_loop(sc, be, st, conn, res, out)
        search_and_fuse(sc, be, st, res, loop, out)
        loop_connections(sc, be, st, conn, loop, out)
        essential_graph(sc, be, st, res, loop, out, tree)
        global_ba(sc, be, st, out)
    out.append(("ComputeBoW", read_bow(be)))
    return out


def run_rejected(sc, be, before=None):
    """only E0 and E1 as candidates: E1 is discarded at :266, E0's solver walks all its iterations (bNoMore), the pass ends false at :343-349.
    before: called between the set-up and ComputeSim3 (the GPU test takes its snapshot of the store there)"""
    out = []
    conn = setup(sc, be, out)
    if before is not None:
        before()
    res = compute_sim3(sc, be, conn, [NAMES.index("E0"), NAMES.index("E1")], out)
    assert not res["accepted"]
    out.append(("ComputeBoW", read_bow(be)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------- CorrectLoop
# The spanning tree, scene data, in two variants.  "jump": every key frame hangs under the one created before it (A0..A4, E0, E1, C0..C4), so the
# edge E1 - C0 carries the whole drift and the pose graph has something to spread: the optimisation is not trivial, which is what the comparison of
# device and host wants.  It cannot end on the truth: the drift sits in ONE edge, the graph spreads it over all of them, and the global BA that
# follows fixes key frame 0 alone, so the scale the graph left is nobody's to restore.  "split": C0 has no parent; the current side joins the old one
# through the loop edges only, every edge agrees with the corrected poses, and the chain can be held to the ground truth.
PARENTS = dict(jump=[-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], split=[-1, 0, 1, 2, 3, 4, 5, -1, 7, 8, 9, 10])


class MapState:
    """what CorrectLoop changes: the key frames' map-point rows and poses, the points' positions, attributes and observations"""

    def __init__(self, sc, probe=False):
        P = sc["points"]
        self.probe = probe                                          # read the store back after every rewrite (see run())
        self.row = P["row"]
        self.rows = [kf["mp"].copy() for kf in sc["kfs"]]
        self.R = [kf["R"].reshape(3, 3).copy() for kf in sc["kfs"]]; self.t = [kf["t"].copy() for kf in sc["kfs"]]
        self.pos, self.normal, self.min_dist, self.max_dist, self.desc = (P[k].copy() for k in ("pos", "normal", "min_dist", "max_dist", "desc"))
        self.obs = {i: list(v) for i, v in P["obs"].items()}
        self.ref_kf = {i: v[0][0] for i, v in P["obs"].items()}      # GetReferenceKeyFrame: the key frame that made the point
        self.bad = set()
        self.corrected_ref = {}                                     # mnCorrectedByKF == mpCurrentKF->mnId: id -> mnCorrectedReference (a member)

    def Ow(self, m):
        return (-(self.R[m].astype(np.float64).T @ self.t[m].astype(np.float64))).astype(f32)

    def T(self, m):
        T = np.eye(4, dtype=f32); T[:3, :3] = self.R[m]; T[:3, 3] = self.t[m]
        return T

    def live(self):
        return [int(i) for i in sorted(self.obs) if self.obs[i] and i not in self.bad]

    def gather(self, ids):
        r = np.array([self.row[int(i)] for i in ids], np.int64)
        return dict(pos=self.pos[r], normal=self.normal[r], min_dist=self.min_dist[r], max_dist=self.max_dist[r], desc=self.desc[r])


def replace(st, old, new, updates):
    """MapPoint::Replace (MapPoint.cpp:198-241): `old`'s observations move to `new` unless `new` is seen by that key frame already; `old` is bad"""
    if old == new:
        return
    seen = set(k for k, _ in st.obs[new])
    for k, f_ in st.obs[old]:
        if k not in seen:
            st.rows[k][f_] = new; st.obs[new].append((k, f_)); seen.add(k); updates.append((k, f_, new))
        else:
            st.rows[k][f_] = -1; updates.append((k, f_, -1))
    st.obs[old] = []; st.bad.add(old)


def write_rows(be, updates):
    """cms_kfstore_update_map_points: sparse (slot, feature, id) triples, the last value of a feature"""
    last = {}
    for k, f_, v in updates:
        last[(k, f_)] = v
    be.update_map_points([SLOTS[k] for k, _ in last], [f_ for _, f_ in last], list(last.values()))


def refresh_attributes(sc, be, st, ids):
    """MapPoint::UpdateNormalAndDepth of the listed points on the poses as they are now.  (The reference calls it inside the point loop of :470-500,
    while some key frames carry the corrected pose and others do not yet; here it runs once behind the loop.)"""
    ids = [i for i in ids if st.obs[int(i)]]
    if not ids:
        return
    kfs = sc["kfs"]
    obs_off = np.concatenate([[0], np.cumsum([len(st.obs[int(i)]) for i in ids])]).astype(np.int32)
    oOw = np.concatenate([np.stack([st.Ow(k) for k, _ in st.obs[int(i)]]) for i in ids]).astype(f32)
    ref = []
    for i in ids:
        o = st.obs[int(i)]
        ref.append(next(((k, f_) for k, f_ in o if k == st.ref_kf[int(i)]), o[0]))
    refOw = np.stack([st.Ow(k) for k, _ in ref]).astype(f32)
    reflev = np.array([kfs[k]["octave"][f_] for k, f_ in ref], np.int32)
    r = np.array([st.row[int(i)] for i in ids], np.int64)
    st.normal[r], st.min_dist[r], st.max_dist[r] = be.normal_and_depth(obs_off, st.pos[r], oOw, refOw, reflev)


def refresh_descriptors(sc, be, st, ids):
    """MapPoint::ComputeDistinctiveDescriptors of the listed points"""
    ids = [i for i in ids if st.obs[int(i)]]
    if not ids:
        return
    obs_off = np.concatenate([[0], np.cumsum([len(st.obs[int(i)]) for i in ids])]).astype(np.int32)
    odesc = np.concatenate([np.stack([sc["kfs"][k]["desc"][f_] for k, f_ in st.obs[int(i)]]) for i in ids])
    best = be.distinctive(obs_off, odesc)
    for n, i in enumerate(ids):
        st.desc[st.row[int(i)]] = odesc[obs_off[n] + best[n]]


def s8(S):
    return np.concatenate([np.asarray(S[0], np.float64), np.asarray(S[1], np.float64), [np.float64(S[2])]])


def se3_of(S):
    """[R | t / s] narrowed to float (LoopClosing.cpp:503-509)"""
    q, t, s = S
    return ns.quat_to_R(q).astype(f32), (np.asarray(t, np.float64) * (1. / s)).astype(f32)


def read_rows(be, st):
    rows = [be.fetch_mp(SLOTS[m], len(st.rows[m])) for m in range(12)]
    for m in range(12):
        assert np.array_equal(rows[m], st.rows[m]), m              # the store holds what the map holds
    return rows


def push_poses(be, st, members):
    be.update_poses([SLOTS[m] for m in members], np.stack([st.R[m].reshape(9) for m in members]), np.stack([st.t[m] for m in members]), np.stack([st.Ow(m) for m in members]))
    return [be.fetch_pose(SLOTS[m]) for m in members] if st.probe else []


def correct_loop(sc, be, st, conn, res, out, cur=CURRENT):
    """CorrectLoop's first half (LoopClosing.cpp:431-534)"""
    kfs = sc["kfs"]
    be.covis_build(SLOTS)                                          # :431 mpCurrentKF->UpdateConnections()
    w, order, nc = be.connections([cur], 15)
    connected = [int(x) for x in order[0, :nc[0]]] + [cur]         # mvpCurrentConnectedKFs
    gScw = ns.sim3_from_Rts(*res["g"])
    Twc = np.eye(4, dtype=f32); Twc[:3, :3] = st.R[cur].T; Twc[:3, 3] = st.Ow(cur)      # GetPoseInverse
    corrected, non_corrected = {}, {}
    for i in connected:                                            # :446-468
        Tiw = st.T(i)
        if i != cur:
            Tic = Tiw @ Twc
            corrected[i] = ns.sim3_times(ns.sim3_from_Rts(Tic[:3, :3], Tic[:3, 3], 1.0), gScw)
        else:
            corrected[i] = gScw
        non_corrected[i] = ns.sim3_from_Rts(Tiw[:3, :3], Tiw[:3, 3], 1.0)
    order_kf = sorted(corrected, key=lambda m: kfs[m]["mn_id"])    # KeyFrameAndPose is ordered by pointer; here by mnId
    S_old = np.stack([s8(non_corrected[i]) for i in order_kf]); S_new = np.stack([s8(corrected[i]) for i in order_kf])
    ids, ref = [], []
    for j, i in enumerate(order_kf):                               # :471-500: a point is corrected by the first key frame that holds it
        for pid in st.rows[i]:
            pid = int(pid)
            if pid < 0 or pid in st.bad or pid in st.corrected_ref:
                continue
            st.corrected_ref[pid] = i; ids.append(pid); ref.append(j)
    r = np.array([st.row[i] for i in ids], np.int64)
    st.pos[r] = be.correct_points(st.pos[r], ref, S_old, S_new)
    for i in order_kf:                                             # :502-511
        st.R[i], st.t[i] = se3_of(corrected[i])
    stored = push_poses(be, st, order_kf)
    refresh_attributes(sc, be, st, ids)
    out.append(("CorrectLoop: Sim3 propagation", dict(connected=connected, order=order_kf, S_old=S_old, S_new=S_new, ids=np.array(ids, np.int64), ref=np.array(ref, np.int32),
                                                      pos=st.pos[r].copy(), stored_poses=stored, normal=st.normal[r].copy(), min_dist=st.min_dist[r].copy(),
                                                      max_dist=st.max_dist[r].copy())))
    updates, replaced, added = [], [], []
    for i, L in enumerate(res["matches"]):                         # :519-534 loop fusion
        L = int(L)
        if L < 0:
            continue
        held = int(st.rows[cur][i])
        if held >= 0:
            replace(st, held, L, updates); replaced.append((held, L))
        else:
            st.rows[cur][i] = L; st.obs[L].append((cur, i)); updates.append((cur, i, L)); added.append((i, L))
    write_rows(be, updates)
    refresh_descriptors(sc, be, st, sorted(set(int(L) for L in res["matches"] if L >= 0)))
    out.append(("CorrectLoop: loop fusion", dict(replaced=np.array(replaced, np.int64).reshape(-1, 2), added=np.array(added, np.int64).reshape(-1, 2),
                                                 rows=read_rows(be, st) if st.probe else [], n_bad=len(st.bad))))
    return dict(connected=connected, order=order_kf, corrected=corrected, non_corrected=non_corrected)


def search_and_fuse(sc, be, st, res, loop, out):
    """SearchAndFuse (LoopClosing.cpp:586-612): one search call over every corrected key frame, then the surgery per key frame in list order"""
    loop_ids = [int(i) for i in res["loop_ids"]]
    pts = st.gather(loop_ids)
    jobs = []
    for i in loop["order"]:
        q, t, s = loop["corrected"][i]
        Scw = np.hstack([s * ns.quat_to_R(q), np.asarray(t, np.float64)[:, None]]).astype(f32)      # Converter::toCvMat(g2oScw)
        held = set(int(v) for v in st.rows[i] if v >= 0)
        skip = np.array([(pid in st.bad) or (pid in held) for pid in loop_ids], np.uint8)           # ORBMatcher.cpp:1255, :1268
        jobs.append(dict(slot=SLOTS[i], n=len(st.rows[i]), Scw=Scw, set=0, skip=skip, member=i))
    found = be.fuse_search_sim3([pts], jobs)
    updates, replaced, added = [], [], []
    for i, (bi, bd) in zip(loop["order"], found):
        reps = []
        for j, pid in enumerate(loop_ids):
            if bi[j] < 0 or pid in st.bad or any(k == i for k, _ in st.obs[pid]):      # :1268, as of this key frame's turn
                continue
            held = int(st.rows[i][bi[j]])
            if held >= 0:                                          # :1347-1358
                if held not in st.bad:
                    reps.append((held, pid))
            else:
                st.rows[i][bi[j]] = pid; st.obs[pid].append((i, int(bi[j]))); updates.append((i, int(bi[j]), pid)); added.append((i, int(bi[j]), pid))
        for held, pid in reps:                                     # LoopClosing.cpp:603-610
            if st.obs[held]:
                replaced.append((i, held, pid))
            replace(st, held, pid, updates)
    write_rows(be, updates)
    out.append(("SearchAndFuse", dict(best_idx=[f[0] for f in found], best_dist=[f[1] for f in found], replaced=np.array(replaced, np.int64).reshape(-1, 3),
                                      added=np.array(added, np.int64).reshape(-1, 3), rows=read_rows(be, st) if st.probe else [], n_bad=len(st.bad))))


def loop_connections(sc, be, st, conn, loop, out):
    """:545-563: the covisibility index rebuilt on the fused rows; LoopConnections = the new links across the loop"""
    be.covis_build(SLOTS)
    w, order, nc = be.connections(list(range(12)), 15)
    loop["cov"] = [[int(x) for x in order[m, :nc[m]]] for m in range(12)]
    loop["cov_w"] = [[int(w[m, x]) for x in loop["cov"][m]] for m in range(12)]
    lc = {}
    for i in loop["connected"]:
        lc[i] = set(loop["cov"][i]) - set(conn[i]) - set(loop["connected"])
    loop["loop_connections"] = lc
    out.append(("LoopConnections", dict(weights=np.asarray(w), order=np.asarray(order), n_connected=np.asarray(nc), links=[[i] + sorted(lc[i]) for i in sorted(lc)],
                                        max_weight=int(np.asarray(w).max()))))


def essential_graph(sc, be, st, res, loop, out, tree="jump", cur=CURRENT):
    """OptimizeEssentialGraph (Optimizer.cpp:623-886): the graph these key frames make, the entry, the write-back of :833-885"""
    kfs = sc["kfs"]
    PARENT = PARENTS[tree]
    children = [[c for c in range(12) if PARENT[c] == m] for m in range(12)]
    m = dict(kfs=[dict(bad=False, mnId=kfs[i]["mn_id"], parent=PARENT[i], children=children[i], loop_edges=[], cov=loop["cov"][i], cov_w=loop["cov_w"][i]) for i in range(12)],
             loop_connections=loop["loop_connections"], cur=cur, loop=res["matched"])
    vertex_kf, edges, fixed = ne.collect_essential_graph(m)
    vertex_of = {kf: v for v, kf in enumerate(vertex_kf)}
    Scw = [loop["corrected"][k] if k in loop["corrected"] else ns.sim3_from_Rts(st.R[k], st.t[k], 1.0) for k in vertex_kf]      # :660-674
    Snc = [loop["non_corrected"].get(k, Scw[v]) for v, k in enumerate(vertex_kf)]
    graph = dict(Scw=np.stack([s8(S) for S in Scw]), Snc=np.stack([s8(S) for S in Snc]), fixed=fixed, edges=np.array(edges, np.int32).reshape(-1, 3), fix_scale=0)
    r = be.essential_graph(api.ess_graph_job_state(graph))
    for v, k in enumerate(vertex_kf):                              # :834-852
        T = r["Tiw"][v].reshape(3, 4)
        st.R[k] = T[:, :3].copy(); st.t[k] = T[:, 3].copy()
    stored = push_poses(be, st, list(vertex_kf))
    ids = st.live()                                                # :855-885
    ref = [vertex_of[st.corrected_ref.get(i, st.ref_kf[i])] for i in ids]
    rr = np.array([st.row[i] for i in ids], np.int64)
    st.pos[rr] = be.correct_points(st.pos[rr], ref, graph["Scw"], r["S"])
    refresh_attributes(sc, be, st, ids)
    out.append(("Store behind the essential graph", dict(rows=read_rows(be, st), poses=[be.fetch_pose(SLOTS[m]) for m in range(12)])))      # (no search follows)
    out.append(("OptimizeEssentialGraph", dict(vertex_kf=list(vertex_kf), edges=graph["edges"], fixed=fixed, S=r["S"], Tiw=r["Tiw"], chi2_initial=r["chi2_initial"],
                                               chi2_final=r["chi2_final"], iterations_run=r["iterations_run"], trials_run=r["trials_run"], flags=r["flags"],
                                               stored_poses=stored, ids=np.array(ids, np.int64), ref=np.array(ref, np.int32), pos=st.pos[rr].copy(),
                                               normal=st.normal[rr].copy(), min_dist=st.min_dist[rr].copy(), max_dist=st.max_dist[rr].copy())))


def gba_map(sc, st):
    """the whole map in the layout Optimizer::CollectGlobalBA's host entry takes (gba_hostlib.collect)"""
    kfs = sc["kfs"]
    nkp = max(len(k["x"]) for k in kfs)
    keys = np.zeros((12, nkp, 2), f32); octave = np.zeros((12, nkp), np.int32); rays = np.zeros((12, nkp, 3), f32); rays[..., 2] = 1.0
    for m, k in enumerate(kfs):
        n = len(k["x"])
        keys[m, :n, 0] = k["x"]; keys[m, :n, 1] = k["y"]; octave[m, :n] = k["octave"]
        _, ray = synth.pixel_to_ray(F, k["x"].astype(np.float64), k["y"].astype(np.float64))
        rays[m, :n] = (ray / np.linalg.norm(ray, axis=1, keepdims=True)).astype(f32)      # mvKeyRays
    ids = st.live()
    r = np.array([st.row[i] for i in ids], np.int64)
    obs_off = np.concatenate([[0], np.cumsum([len(st.obs[i]) for i in ids])]).astype(np.int32)
    return ids, dict(F=F, n_list=12, kf_id=np.array([k["mn_id"] for k in kfs], np.int64), kf_bad=np.zeros(12, np.uint8), Tcw=np.stack([st.T(m) for m in range(12)]),
                     keys=keys, octave=octave, rays=rays, inv_level_sigma2=INV_SIGMA2, mp_id=np.array(ids, np.int64), mp_bad=np.zeros(len(ids), np.uint8), Xw=st.pos[r].copy(),
                     obs_off=obs_off, obs_kf=np.array([k for i in ids for k, _ in st.obs[i]], np.int32), obs_kp=np.array([f_ for i in ids for _, f_ in st.obs[i]], np.int32))


def global_ba(sc, be, st, out):
    """RunGlobalBundleAdjustment (LoopClosing.cpp:644-649; Optimizer.cpp:453-621): collect, ten iterations without kernel, write back"""
    ids, m = gba_map(sc, st)
    prob = gba_hostlib.collect(m)
    out.append(("CollectGlobalBA", dict(problem=prob)))
    r = be.global_ba(prob)
    for v, k in enumerate(prob["vertex_kf"]):                      # :577-598 (nLoopKF's first branch: SetPose)
        T = harness._T_from_pose7(r["poses"][v])
        st.R[k] = T[:3, :3].copy(); st.t[k] = T[:3, 3].copy()
    rr = np.array([st.row[ids[j]] for j in prob["vertex_mp"]], np.int64)
    st.pos[rr] = r["points"].astype(f32)
    out.append(("GlobalBundleAdjustment", dict(poses=r["poses"], points=r["points"], iterations_done=int(r["iterations_done"]), chi2_final=float(r["chi2_final"]))))
    live = st.live()
    out.append(("Final", dict(centres=np.stack([st.Ow(m) for m in range(12)]), ids=np.array(live, np.int64), pos=st.pos[np.array([st.row[i] for i in live], np.int64)].copy())))


LOOSE = ("GlobalBundleAdjustment", "Final")      # compared with gba_cases.close_or_cascade and by the truth, not by bits


def truth_error(sc, rec=None, sides="AC"):
    """(RMS distance of the key-frame centres, of the map points) to the ground truth, nothing removed: the old side fixes the gauge.  rec None: the
    drifted map as the scene has it.  sides: E0 / E1 share no observation with the rest, so the global BA leaves their gauge to the damping; they are
    measured with sides="ACE" where a test wants them."""
    members = [m for m, n in enumerate(NAMES) if n[0] in sides]
    true_c = np.stack([-(R.T @ t) for R, t in sc["true_poses"]])
    if rec is None:
        c = np.stack([k["Ow"] for k in sc["kfs"]]).astype(np.float64); ids = sc["points"]["ids"]; pos = sc["points"]["pos"].astype(np.float64)
    else:
        fin = stage(rec, "Final")
        c = fin["centres"].astype(np.float64); ids = fin["ids"]; pos = fin["pos"].astype(np.float64)
    phys = np.where(ids >= E_ID, ids - E_ID + NS, ids % CUR_ID)
    keep = np.array([("E" in sides) or i < E_ID for i in ids])
    dc = c[members] - true_c[members]; dp = (pos - sc["X"][phys])[keep]
    return float(np.sqrt((dc * dc).sum(1).mean())), float(np.sqrt((dp * dp).sum(1).mean()))


def stage(rec, name):
    for n, o in rec:
        if n == name:
            return o
    raise KeyError(name)


def stages(rec, prefix):
    return [o for n, o in rec if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------------------------------------------- comparing
def _flat(v, path, acc):
    if isinstance(v, dict):
        for k in sorted(v):
            _flat(v[k], path + "." + str(k), acc)
    elif isinstance(v, (list, tuple)):
        acc.append((path + ".len", ("int", len(v))))
        for i, x in enumerate(v):
            _flat(x, "%s[%d]" % (path, i), acc)
    elif isinstance(v, np.ndarray):
        acc.append((path, ("array", str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())))      # floats as bits
    elif isinstance(v, (bool, np.bool_)):
        acc.append((path, ("int", int(v))))
    elif isinstance(v, (int, np.integer)):
        acc.append((path, ("int", int(v))))
    elif isinstance(v, (float, np.floating)):
        acc.append((path, ("float", np.float64(v).tobytes())))
    elif v is None:
        acc.append((path, ("none",)))
    else:
        acc.append((path, ("str", str(v))))


def first_difference(want, got):
    """None, or the first stage and field at which two run() results differ: integers as integers, floats as bits"""
    for k, ((wn, wo), (gn, go)) in enumerate(zip(want, got)):
        if wn != gn:
            return "stage %d: %s against %s" % (k, wn, gn)
        if wn in LOOSE:
            continue
        a, b = [], []
        _flat(wo, "", a); _flat(go, "", b)
        for (pa, va), (pb, vb) in zip(a, b):
            if pa != pb or va != vb:
                show = lambda p, v: "%s %s" % (p, (np.frombuffer(v[3], v[1]).reshape(v[2]) if v[0] == "array" else v[1:]))
                return ("stage %d (%s): want %s, got %s" % (k, wn, show(pa, va), show(pb, vb)))[:1500]
        if len(a) != len(b):
            return "stage %d (%s): %d fields against %d" % (k, wn, len(a), len(b))
    if len(want) != len(got):
        return "%d stages against %d" % (len(want), len(got))
    return None


def discrete(rec):
    """the chain's discrete outputs only (candidate lists, match lists, masks, counts, iteration counts), for the tameness test"""
    acc = []
    for n, o in rec:
        part = []
        _flat(o, n, part)
        acc += [(p, v) for p, v in part if v[0] in ("int", "none", "str") or (v[0] == "array" and not v[1].startswith("float"))]
    return acc


# ------------------------------------------------------------------------------------------------------------------------------- backends
def _kf_dict(kf, with_fv=None):
    n = len(kf["x"])
    fv = with_fv or dict(node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))
    return dict(x=kf["x"], y=kf["y"], octave=kf["octave"], angle=kf["angle"], desc=kf["desc"], rays=np.zeros((n, 3), f32), mp=kf["mp"], R=kf["R"], t=kf["t"], Ow=kf["Ow"],
                median_depth=1.0, **fv)


class HostBackend:
    """every step from the CPU reference that stage's own GPU test compares against: the host builds of the vocabulary, database, covisibility, Sim3
    solver and Sim3 optimiser cores, and the numpy restatements of the three matchers"""

    def __init__(self):
        self.db = kfdb_hostlib.HostDatabase(K_SLOTS, MAXF)
        self.cv = covis_hostlib.HostBackend(K_SLOTS, MAXF)
        self.hv = None

    def close(self):
        self.db.close(); self.cv.close()
        if self.hv is not None:
            self.hv.close()

    def load(self, sc):
        self.sc = sc
        if self.hv is None:
            self.hv = vocab_hostlib.HostVocabulary(sc["tree"])
        assert self.db.clear(-1) == 0
        self.bow, self.kf_of, self.pose = {}, {}, {}
        for kf in sc["kfs"]:
            s = kf["slot"]
            b = self.hv.transform(kf["desc"], LEVELSUP)
            self.bow[s] = b; self.kf_of[s] = kf
            assert self.db.refill(s) == 0 and self.db.set_bow(s, b["word_id"], b["word_val"]) == 0
            assert self.cv.put(s, kf["mp"], kf["octave"]) == 0

    def fetch_bow(self, slot):
        b = self.bow[slot]
        return dict(word_id=b["word_id"], word_val=b["word_val"], node_id=b["node_id"], node_off=b["node_off"], node_feat=b["node_feat"])

    def db_add(self, slots): assert self.db.add(slots, [0] * len(slots)) == 0
    def db_set_covisibles(self, slots, neigh):
        for s, n in zip(slots, neigh):
            assert self.db.covis(s, n) == 0
    def covis_build(self, slots): assert self.cv.build(slots) == 0
    def connections(self, members, th): return self.cv.connections(members, th)
    def local_points(self, member_lists, cap): return self.cv.local_points(member_lists, cap)
    def bow_score(self, a, b): return self.db.bow_score(a, b)
    def detect(self, jobs): return self.db.detect(jobs)

    def search_by_bow(self, jobs):
        out = []
        for s1, n1, s2, n2, bad1, bad2 in jobs:
            a, b, fa, fb = self.kf_of[s1], self.kf_of[s2], self.bow[s1], self.bow[s2]
            out.append(npref_bow_kf.search_by_bow_kf(a["angle"], a["desc"], a["mp"] >= 0, bad1, fa, b["angle"], b["desc"], b["mp"] >= 0, bad2, fb, 0.75, True,
                                                     npref_bow_kf.feat_node_of(fa, n1), npref_bow_kf.feat_node_of(fb, n2)))
        return out

    def sim3_iterate(self, states):
        rc, res = sim3_hostlib.iterate_host(F, states)
        assert rc == 0
        return res

    @staticmethod
    def _view(kf):
        return dict(kx=kf["x"], ky=kf["y"], koct=kf["octave"], kdesc=kf["desc"], pose12=kf["pose12"])

    def search_by_sim3(self, jobs, z_as_written=True):
        return [npref_sim3_search.search_by_sim3(CAMD, SF, self._view(self.kf_of[j["slot1"]]), self._view(self.kf_of[j["slot2"]]), j["s12"], j["R12"], j["t12"], j["mp1"], j["mp2"],
                                                 th=7.5, z_as_written=z_as_written) for j in jobs]

    def sim3_optimize(self, states):
        rc, res = sim3_opt_hostlib.optimize_host(F, states)
        assert rc == 0
        return res

    def search_by_projection_sim3(self, sets, jobs):
        return [npref_sim3_projection.search_by_projection(CAMD, SF, self._view(self.kf_of[j["slot"]]), j["Scw"], sets[j["set"]], skip=j["skip"], taken=j["taken"], th=10.0)
                for j in jobs]

    def fuse_search_sim3(self, sets, jobs):
        return [npref_sim3_projection.fuse_search(CAMD, SF, self._view(self.kf_of[j["slot"]]), j["Scw"], sets[j["set"]], skip=j["skip"], th=4.0) for j in jobs]

    def correct_points(self, pos, ref, S_old, S_new): return ess_graph_hostlib.correct_points_host(pos, ref, S_old, S_new)
    def normal_and_depth(self, obs_off, pos, oOw, refOw, reflev): return orc.update_normal_and_depth(obs_off, pos, oOw, refOw, reflev, SF)
    def distinctive(self, obs_off, odesc): return orc.distinctive_descriptors(obs_off, odesc)

    def update_poses(self, slots, R, t, Ow):
        for s, r_, t_, o_ in zip(slots, R, t, Ow):
            self.pose[s] = np.concatenate([r_.reshape(9), t_, o_]).astype(f32)

    def fetch_pose(self, slot): return self.pose[slot].copy()
    def update_map_points(self, slot, feat, mp): assert self.cv.update_map_points(slot, feat, mp) == 0
    def fetch_mp(self, slot, n): return self.cv.fetch_mp(slot, n)

    def essential_graph(self, state):
        rc, res = ess_graph_hostlib.optimize_host([state])
        assert rc == 0, ess_graph_hostlib.reason()
        return res[0]

    def global_ba(self, prob):
        return npref_global_ba.run(prob, 10, False)


class DeviceBackend:
    """api.* on the loop-closing thread's context `ctx`, and a KeyframeStore on the mapping side's context (the store's stream is not ctx's); the
    handles are made once and serve every chain run on this object.  one_by_one: every entry that takes several jobs gets them one per call."""

    def __init__(self, one_by_one=False):
        self.cg = api.Context(CAMD, nfeatures=2000, max_batch=1)
        self.ctx = api.Context(CAMD, nfeatures=2000, max_batch=2)
        self.st = api.KeyframeStore(self.cg, max_keyframes=K_SLOTS, max_features=MAXF, max_nodes=MAX_NODES)
        self.cv = api.Covisibility(self.st, K_SLOTS)
        self.solver = api.Sim3Solver(max_jobs=8, max_corr_total=4096, max_hyp_total=4096, device=0)
        self.opt = api.Sim3Optimizer(max_jobs=8, max_corr_total=4096, device=0)
        self.eg = api.EssentialGraphOptimizer(2, 64, 512, 2048, device=0)
        self.voc = None
        self.one = one_by_one

    def close(self):
        for h in (self.eg, self.opt, self.solver, self.cv, self.st, self.voc, self.ctx, self.cg):
            if h is not None:
                h.close()

    def load(self, sc):
        if self.voc is None:
            self.voc = api.Vocabulary.from_dict(sc["tree"])
        self.st.db_clear(-1)
        for kf in sc["kfs"]:
            K, keep = api.make_keyframe(_kf_dict(kf))
            self.st.put(kf["slot"], K)
        self.st.compute_bow(self.voc, [kf["slot"] for kf in sc["kfs"]], LEVELSUP)

    def fetch_bow(self, slot):
        b = self.st.fetch_bow(slot, feature_vector=True)
        return dict(word_id=b["word_id"], word_val=b["word_val"], node_id=b["node_id"], node_off=b["node_off"], node_feat=b["node_feat"])

    def _each(self, fn, jobs):
        if not self.one:
            return fn(jobs)
        return [fn([j])[0] for j in jobs]

    def db_add(self, slots): self.st.db_add(slots)
    def db_set_covisibles(self, slots, neigh): self.st.db_set_covisibles(slots, neigh)
    def covis_build(self, slots): self.cv.build(slots)
    def connections(self, members, th): return self.cv.connections(members, th)
    def local_points(self, member_lists, cap): return self.cv.local_points(self.ctx, member_lists, cap)
    def bow_score(self, a, b): return self.st.bow_score(a, b)
    def detect(self, jobs): return self.st.detect_candidates(self.ctx, jobs)
    def search_by_bow(self, jobs): return self._each(lambda j: self.st.search_by_bow_keyframes(self.ctx, j, nnratio=0.75, check_orientation=True), jobs)
    def sim3_iterate(self, states): return self._each(lambda s: self.solver.run(self.ctx, s), states)
    def search_by_sim3(self, jobs, z_as_written=True): return self._each(lambda j: self.st.search_by_sim3(self.ctx, j, th=7.5, z_as_written=z_as_written), jobs)
    def sim3_optimize(self, states): return self._each(lambda s: self.opt.run(self.ctx, s), states)
    def search_by_projection_sim3(self, sets, jobs): return self.st.search_by_projection_sim3(self.ctx, sets, jobs, th=10.0)
    def fuse_search_sim3(self, sets, jobs): return self.st.fuse_search_sim3(self.ctx, sets, jobs, th=4.0)
    def correct_points(self, pos, ref, S_old, S_new): return api.sim3_correct_points(self.ctx, pos, ref, S_old, S_new)
    def distinctive(self, obs_off, odesc): return api.distinctive_descriptors(self.ctx, obs_off, odesc)
    def update_poses(self, slots, R, t, Ow): self.st.update_poses(slots, R, t, Ow)
    def fetch_pose(self, slot): return self.st.debug_fetch(slot)["header"][6:21].view(f32).copy()
    def update_map_points(self, slot, feat, mp): self.st.update_map_points(slot, feat, mp)
    def fetch_mp(self, slot, n): return self.st.debug_fetch(slot)["mp"][:n].copy()
    def essential_graph(self, state): return self.eg.run(self.ctx, [state])[0]

    def normal_and_depth(self, obs_off, pos, oOw, refOw, reflev):
        n = len(obs_off) - 1
        nrm = np.zeros((n, 3), f32); mn = np.zeros(n, f32); mx = np.zeros(n, f32)
        api.update_normal_and_depth(self.ctx, obs_off, pos, oOw, refOw, reflev, nrm, mn, mx)
        return nrm, mn, mx

    def global_ba(self, prob):
        r = api.ba_run_global(prob, iterations=10, robust=False)
        assert r["rc"] == 0
        return dict(poses=r["poses"], points=r["points"], iterations_done=r["stats"].iterations_done[0], chi2_final=r["stats"].chi2_final[0])

    def snapshot(self):
        """every store row (debug_fetch of every filled slot) and the covisibility answers, as bytes"""
        acc = []
        for s in sorted(SLOTS):
            _flat({k: v for k, v in self.st.debug_fetch(s).items()}, "slot%d" % s, acc)
        w, order, nc = self.cv.connections(list(range(12)), 15)
        _flat(dict(w=w, order=order, nc=nc), "covis", acc)
        _flat(self.cv.local_points(self.ctx, [list(range(12))], K_SLOTS * MAXF)[2], "local_points", acc)
        return acc
