"""LoopClosing's GLUE restated in float64 over objects, from the reference's text: DetectLoop's consistency groups (src/LoopClosing.cpp:102-228),
ComputeSim3's bookkeeping around its matchers and solvers (:230-399), CorrectLoop (:401-584), SearchAndFuse (:586-612), the write-back of
OptimizeEssentialGraph (src/Optimizer.cpp:833-885) and of the global BA (:577-598).  Key frames and map points are objects that point at each other,
as in the reference; nothing is shared with the index arithmetic of tests/loop_cases.py, whose chain this file judges.  The stage BODIES (vocabulary,
database, covisibility, matchers, solvers, optimisers) are not restated here: they are the existing npref_* restatements and host cores, reached
through the `stages` object (loop_cases.HostBackend), so that only the glue differs between the two chains.

Arithmetic: every pose, similarity and point of the glue is float64; a value is narrowed only where the reference stores a cv::Mat of floats
(SetPose, SetWorldPos, mScw) or an entry's record is float by its ABI."""
import numpy as np

import gba_hostlib
import kfdb_cases as kc
import npref_essential_graph as ne
import npref_sim3_opt as ns
from cubemapslam_amd import api, harness, synth
from npref_pnp import rays_to_cubemap

F = 550
TH_CONSISTENCY = 3
SIGMA2 = ((np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)
f32, f64 = np.float32, np.float64


class MapPoint:
    def __init__(self, pid, P, r):
        self.id = pid
        self.pos = P["pos"][r].astype(f64); self.normal = P["normal"][r].copy(); self.min_dist = P["min_dist"][r]; self.max_dist = P["max_dist"][r]; self.desc = P["desc"][r].copy()
        self.obs = {}                                               # KeyFrame -> index, in AddObservation order
        self.bad = False
        self.ref_kf = None
        self.corrected_by = -1; self.corrected_ref = None
        self.loop_point_for = -1


class KeyFrame:
    def __init__(self, m, kf):
        self.m = m; self.slot = kf["slot"]; self.mn_id = kf["mn_id"]; self.name = kf["name"]
        self.kf = kf
        self.R = kf["R"].reshape(3, 3).astype(f64); self.t = kf["t"].astype(f64)
        self.mps = [None] * len(kf["mp"])
        self.ordered = []                                           # mvpOrderedConnectedKeyFrames
        self.parent = None; self.children = set(); self.loop_edges = set()

    def set_pose(self, R, t):
        """SetPose: a cv::Mat of floats"""
        self.R = np.asarray(R, f64).astype(f32).astype(f64); self.t = np.asarray(t, f64).astype(f32).astype(f64)

    def centre(self):
        return (-(self.R.T @ self.t)).astype(f32)


def build_map(sc):
    P = sc["points"]
    kfs = [KeyFrame(m, kf) for m, kf in enumerate(sc["kfs"])]
    mps = {}
    for kf in kfs:
        for i, pid in enumerate(kf.kf["mp"]):
            if pid >= 0:
                mp = mps.get(int(pid))
                if mp is None:
                    mp = mps[int(pid)] = MapPoint(int(pid), P, P["row"][int(pid)])
                    mp.ref_kf = kf
                kf.mps[i] = mp; mp.obs[kf] = i
    return kfs, mps


def replace(old, new):
    """MapPoint::Replace (MapPoint.cpp:198-241) -> the (key frame, index, new id or -1) entries it rewrote"""
    if old.id == new.id:
        return []
    obs, old.obs, old.bad = old.obs, {}, True
    touched = []
    for kf, idx in obs.items():
        if kf not in new.obs:
            kf.mps[idx] = new; new.obs[kf] = idx; touched.append((kf, idx, new.id))
        else:
            kf.mps[idx] = None; touched.append((kf, idx, -1))
    return touched


def per_keypoint(kf, already):
    n = len(kf.mps)
    o = dict(skip=np.ones(n, np.uint8), pos=np.zeros((n, 3), f32), min_dist=np.zeros(n, f32), max_dist=np.zeros(n, f32), desc=np.zeros((n, 32), np.uint8))
    for i, mp in enumerate(kf.mps):
        if mp is None:
            continue
        o["skip"][i] = 1 if (already[i] or mp.bad) else 0
        o["pos"][i] = mp.pos; o["min_dist"][i] = mp.min_dist; o["max_dist"][i] = mp.max_dist; o["desc"][i] = mp.desc
    return o


def point_set(pts):
    return dict(pos=np.array([p.pos for p in pts], f32), normal=np.array([p.normal for p in pts], f32), min_dist=np.array([p.min_dist for p in pts], f32),
                max_dist=np.array([p.max_dist for p in pts], f32), desc=np.array([p.desc for p in pts], np.uint8))


def in_a_face(X):
    _, u, v = rays_to_cubemap(F, np.array([X[0]], f32), np.array([X[1]], f32), np.array([X[2]], f32))
    return not (u[0] < 0 or v[0] < 0)


def update_connections(stages, kfs, which):
    """KeyFrame::UpdateConnections through the covisibility index (the stage body), stored on the objects"""
    w, order, nc = stages.connections([k.m for k in which], 15)
    for j, k in enumerate(which):
        k.ordered = [kfs[int(x)] for x in order[j, :nc[j]]]
        k.weights = {kfs[int(x)]: int(w[j, int(x)]) for x in order[j, :nc[j]]}


def refresh(stages, sc, pts):
    """UpdateNormalAndDepth on the present poses (as loop_cases states: once behind the loop, not inside it)"""
    pts = [p for p in pts if p.obs]
    if not pts:
        return
    off = np.concatenate([[0], np.cumsum([len(p.obs) for p in pts])]).astype(np.int32)
    oOw = np.array([k.centre() for p in pts for k in p.obs], f32)
    ref = [(p.ref_kf, p.obs[p.ref_kf]) if p.ref_kf in p.obs else next(iter(p.obs.items())) for p in pts]
    nrm, mn, mx = stages.normal_and_depth(off, np.array([p.pos for p in pts], f32), oOw, np.array([k.centre() for k, _ in ref], f32),
                                          np.array([k.kf["octave"][i] for k, i in ref], np.int32))
    for j, p in enumerate(pts):
        p.normal, p.min_dist, p.max_dist = nrm[j], mn[j], mx[j]


def redescribe(stages, pts):
    pts = [p for p in pts if p.obs]
    if not pts:
        return
    off = np.concatenate([[0], np.cumsum([len(p.obs) for p in pts])]).astype(np.int32)
    od = np.array([k.kf["desc"][i] for p in pts for k, i in p.obs.items()], np.uint8)
    best = stages.distinctive(off, od)
    for j, p in enumerate(pts):
        p.desc = od[off[j] + best[j]].copy()


def run(sc, stages, detect, current, draws_of, parents, z_as_written=True):
    """-> dict of the chain's results.  detect: the members DetectLoop runs for, in turn; current: mpCurrentKF's member; draws_of(member, N): the
    recorded draws; parents: the spanning tree (member -> member or -1); z_as_written: SearchBySim3's reading of ORBMatcher.cpp:1507"""
    out = {}
    stages.load(sc)
    kfs, mps = build_map(sc)
    by_slot = {k.slot: k for k in kfs}
    for k in kfs:
        if parents[k.m] >= 0:
            k.parent = kfs[parents[k.m]]; k.parent.children.add(k)
    stages.db_add([k.slot for k in kfs if k.m not in detect])
    stages.covis_build([k.slot for k in kfs])
    update_connections(stages, kfs, kfs)
    neigh = np.full((len(kfs), 10), -1, np.int32)
    for k in kfs:
        best = k.ordered[:10]
        neigh[k.m, :len(best)] = [b.slot for b in best]
    stages.db_set_covisibles([k.slot for k in kfs], neigh)
    # ---------------------------------------------------------------- DetectLoop, :102-228
    groups, enough = [], []
    out["candidates"] = []
    for m in detect:
        cur = kfs[m]
        scores = stages.bow_score([cur.slot] * len(cur.ordered), [k.slot for k in cur.ordered])
        min_score = f32(1)
        for s in scores:
            if f32(s) < min_score:
                min_score = f32(s)
        cands = [by_slot[s] for s in stages.detect([kc.job(kc.LOOP, ("slot", cur.slot), min_score=min_score, connected=[k.slot for k in cur.ordered])])[0][0]]
        out["candidates"].append([c.m for c in cands])
        enough = []
        if not cands:
            stages.db_add([cur.slot]); groups = []
            continue
        now, used = [], [False] * len(groups)
        for c in cands:
            grp = set(c.ordered) | {c}
            ok_enough = consistent_some = False
            for g, (prev, n) in enumerate(groups):
                if any(x in prev for x in grp):
                    consistent_some = True
                    if not used[g]:
                        now.append((grp, n + 1)); used[g] = True
                    if n + 1 >= TH_CONSISTENCY and not ok_enough:
                        enough.append(c); ok_enough = True
            if not consistent_some:
                now.append((grp, 0))
        groups = now
        stages.db_add([cur.slot])
    out["enough"] = [c.m for c in enough]
    # ---------------------------------------------------------------- ComputeSim3, :230-399
    cur = kfs[current]
    n1 = len(cur.mps)
    bow = stages.search_by_bow([(cur.slot, n1, c.slot, len(c.mps), None, None) for c in enough])
    out["bow_matches"] = [b[1] for b in bow]
    solvers = {}
    for c, (idx2, nm) in zip(enough, bow):
        if nm < 20:
            continue
        matched12 = [c.mps[i2] if i2 >= 0 else None for i2 in idx2]      # vvpMapPointMatches[i]
        ind, x1, x2, e1, e2 = [], [], [], [], []
        for i1, mp2 in enumerate(matched12):                      # Sim3Solver.cpp:66-127
            mp1 = cur.mps[i1]
            if mp2 is None or mp1 is None or mp1.bad or mp2.bad:
                continue
            k1, k2 = mp1.obs.get(cur, -1), mp2.obs.get(c, -1)
            if k1 < 0 or k2 < 0:
                continue
            X1 = cur.R @ mp1.pos + cur.t; X2 = c.R @ mp2.pos + c.t
            if not in_a_face(X1) or not in_a_face(X2):
                continue
            ind.append(i1); x1.append(X1); x2.append(X2)
            e1.append(f32(9.210 * f64(SIGMA2[cur.kf["octave"][k1]]))); e2.append(f32(9.210 * f64(SIGMA2[c.kf["octave"][k2]])))
        N = len(ind)
        solvers[c] = dict(matched12=matched12, ind=ind, carried={}, draws=draws_of(c.m, N),
                          prob=dict(x3dc1=np.array(x1, f32), x3dc2=np.array(x2, f32), max_err1=np.array(e1, f32), max_err2=np.array(e2, f32), fix_scale=0, min_inliers=20,
                                    max_its=api.sim3_ransac_parameters(N, 0.99, 20, 300)))
    live = [c for c in enough if c in solvers]
    out["solvers"] = [c.m for c in live]; out["solver_N"] = [len(solvers[c]["ind"]) for c in live]; out["indices1"] = [list(solvers[c]["ind"]) for c in live]
    out["passes"] = 0; out["accepted"] = False; out["hypotheses"] = []; out["pass"] = []
    ids_of = lambda vp: [p.id if p is not None else -1 for p in vp]
    matched_kf = None
    while live and matched_kf is None:
        out["passes"] += 1
        states = [api.sim3_job_state(dict(solvers[c]["prob"], **solvers[c]["carried"]), 5, solvers[c]["draws"][solvers[c]["carried"].get("iterations", 0):]) for c in live]
        rs = stages.sim3_iterate(states)
        rec = dict(live=[c.m for c in live], status=[int(r["status"]) for r in rs], no_more=[int(r["no_more"]) for r in rs], n_inliers=[int(r["n_inliers"]) for r in rs],
                   iterations=[int(r["iterations"]) for r in rs], masks=[[int(v) for v in r["inliers"]] for r in rs])
        out["pass"].append(rec)
        hyps = []
        for c, r in zip(list(live), rs):
            s = solvers[c]
            s["carried"] = dict(iterations=r["iterations"], best_inliers=r["best_inliers"], best_mask=r["best_mask"].copy(), best_s=float(r["best_s"][0]),
                                best_R=r["best_R"].copy(), best_t=r["best_t"].copy(), best_T12=r["best_T12"].copy())
            if r["no_more"]:
                live.remove(c)
            if r["status"] == 1:
                vp = [None] * n1                                    # :312-317
                for j, i1 in enumerate(s["ind"]):
                    if r["inliers"][j]:
                        vp[i1] = s["matched12"][i1]
                hyps.append((c, vp, r["best_R"].reshape(3, 3).astype(f64), r["best_t"].astype(f64), f64(r["best_s"][0])))
        if not hyps:
            continue
        jobs = []
        for c, vp, R, t, s_ in hyps:                                # ORBMatcher.cpp:1390-1400
            a1 = [p is not None for p in vp]; a2 = [False] * len(c.mps)
            for p in vp:
                if p is not None and p.obs.get(c, -1) >= 0:
                    a2[p.obs[c]] = True
            jobs.append(dict(slot1=cur.slot, slot2=c.slot, s12=f32(s_), R12=R.astype(f32), t12=t.astype(f32), mp1=per_keypoint(cur, a1), mp2=per_keypoint(c, a2)))
        found = stages.search_by_sim3(jobs, z_as_written=z_as_written)
        for (c, vp, R, t, s_), (idx2, nf) in zip(hyps, found):
            for i1 in np.flatnonzero(np.asarray(idx2) >= 0):
                vp[i1] = c.mps[idx2[i1]]
        rec.update(sim3_idx2=[[int(v) for v in f[0]] for f in found], n_found=[int(f[1]) for f in found], matches_searched=[ids_of(h[1]) for h in hyps])
        probs = []
        for c, vp, R, t, s_ in hyps:                                # Optimizer.cpp:941-978
            idx = [i for i, p2 in enumerate(vp) if p2 is not None and cur.mps[i] is not None and not cur.mps[i].bad and not p2.bad and p2.obs.get(c, -1) >= 0]
            i2 = [vp[i].obs[c] for i in idx]
            probs.append((idx, dict(x3dc1=np.array([cur.R @ cur.mps[i].pos + cur.t for i in idx], f32), x3dc2=np.array([c.R @ vp[i].pos + c.t for i in idx], f32),
                                    kp1=np.array([(cur.kf["x"][i], cur.kf["y"][i]) for i in idx], f32), kp2=np.array([(c.kf["x"][j], c.kf["y"][j]) for j in i2], f32),
                                    inv_sigma2_1=INV_SIGMA2[cur.kf["octave"][idx]], inv_sigma2_2=INV_SIGMA2[c.kf["octave"][i2]], R12=R, t12=t, s12=float(s_), fix_scale=0)))
        ro = stages.sim3_optimize([api.sim3_opt_job_state(p, th2=10.0) for _, p in probs])
        out["hypotheses"].append([(h[0].m, int(r["n_inliers"])) for h, r in zip(hyps, ro)])
        for (c, vp, R, t, s_), (idx, _), r in zip(hyps, probs, ro):
            for k, i in enumerate(idx):
                if r["keep"][k] == 0:
                    vp[i] = None
        rec.update(keep=[[int(v) for v in r["keep"]] for r in ro], opt_iterations=[[int(v) for v in r["iterations"]] for r in ro], matches_optimised=[ids_of(h[1]) for h in hyps])
        for (c, vp, R, t, s_), r in zip(hyps, ro):
            if r["n_inliers"] >= 20:                                # :328-338
                matched_kf = c
                gScm = (np.asarray(r["q12"], f64), np.asarray(r["t12"], f64), f64(r["s12"][0]))
                gScw = ns.sim3_times(gScm, ns.sim3_from_Rts(c.R, c.t, 1.0))
                current_matched = vp
                break
    if matched_kf is None:
        return out
    q, t, s = gScw
    mScw = np.hstack([s * ns.quat_to_R(q), t[:, None]]).astype(f32)
    out.update(matched=matched_kf.m, Scw=mScw, gScw=ne.to8(gScw))
    loop_kfs = list(matched_kf.ordered) + [matched_kf]              # :352-371
    loop_pts = []
    for k in loop_kfs:
        for p in k.mps:
            if p is not None and not p.bad and p.loop_point_for != cur.mn_id:
                loop_pts.append(p); p.loop_point_for = cur.mn_id
    found = set(p for p in current_matched if p is not None)
    job = dict(slot=cur.slot, n=n1, Scw=mScw, set=0, skip=np.array([p in found for p in loop_pts], np.uint8), taken=np.array([p is not None for p in current_matched], np.uint8))
    match_kp, nm = stages.search_by_projection_sim3([point_set(loop_pts)], [job])[0]
    for j in np.flatnonzero(np.asarray(match_kp) >= 0):
        current_matched[match_kp[j]] = loop_pts[j]
    total = sum(p is not None for p in current_matched)
    out.update(loop_ids=[p.id for p in loop_pts], matches=[p.id if p is not None else -1 for p in current_matched], total=total, accepted=total >= 40)
    if total < 40:
        return out
    # ---------------------------------------------------------------- CorrectLoop, :431-534
    stages.covis_build([k.slot for k in kfs])
    update_connections(stages, kfs, [cur])
    connected = list(cur.ordered) + [cur]
    Twc = np.eye(4); Twc[:3, :3] = cur.R.T; Twc[:3, 3] = -(cur.R.T @ cur.t)
    corrected, non_corrected = {}, {}
    for k in connected:
        Tiw = np.eye(4); Tiw[:3, :3] = k.R; Tiw[:3, 3] = k.t
        if k is not cur:
            Tic = Tiw @ Twc
            corrected[k] = ns.sim3_times(ns.sim3_from_Rts(Tic[:3, :3], Tic[:3, 3], 1.0), gScw)
        else:
            corrected[k] = gScw
        non_corrected[k] = ns.sim3_from_Rts(k.R, k.t, 1.0)
    order = sorted(corrected, key=lambda k: k.mn_id)
    moved = []
    for k in order:                                                 # :471-511
        Swi = ns.sim3_inverse(corrected[k])
        for p in k.mps:
            if p is None or p.bad or p.corrected_by == cur.mn_id:
                continue
            p.pos = ns.sim3_map(Swi, ns.sim3_map(non_corrected[k], p.pos)).astype(f32).astype(f64)      # SetWorldPos: floats
            p.corrected_by = cur.mn_id; p.corrected_ref = k
            moved.append(p)
    for k in order:
        q, t, s = corrected[k]
        k.set_pose(ns.quat_to_R(q), t * (1. / s))
    stages.update_poses([k.slot for k in order], np.array([k.R.astype(f32).reshape(9) for k in order]), np.array([k.t.astype(f32) for k in order]), np.array([k.centre() for k in order]))
    refresh(stages, sc, moved)
    out.update(connected=[k.m for k in connected], corrected_ids=[p.id for p in moved], corrected_pos=np.array([p.pos for p in moved], f32),
               corrected_poses=np.array([np.concatenate([k.R.reshape(9), k.t]) for k in order], f32))
    touched, fused_replaced, fused_added = [], [], []
    for i, pl in enumerate(current_matched):                        # :519-534
        if pl is None:
            continue
        pc = cur.mps[i]
        if pc is not None:
            fused_replaced.append((pc.id, pl.id)); touched += replace(pc, pl)
        else:
            cur.mps[i] = pl; pl.obs[cur] = i; touched.append((cur, i, pl.id)); fused_added.append((i, pl.id))
    last = {}
    for k, i, v in touched:
        last[(k.slot, i)] = v
    stages.update_map_points([a for a, _ in last], [b for _, b in last], list(last.values()))
    redescribe(stages, sorted(set(p for p in current_matched if p is not None), key=lambda p: p.id))
    out.update(fused_replaced=fused_replaced, fused_added=fused_added)
    # ---------------------------------------------------------------- SearchAndFuse, :586-612
    jobs = []
    for k in order:
        q, t, s = corrected[k]
        held = set(p for p in k.mps if p is not None)
        jobs.append(dict(slot=k.slot, n=len(k.mps), Scw=np.hstack([s * ns.quat_to_R(q), t[:, None]]).astype(f32), set=0, skip=np.array([p.bad or p in held for p in loop_pts], np.uint8)))
    touched, sf_replaced, sf_added = [], [], []
    for k, (bi, bd) in zip(order, stages.fuse_search_sim3([point_set(loop_pts)], jobs)):
        reps = [None] * len(loop_pts)
        for j, p in enumerate(loop_pts):                            # ORBMatcher.cpp:1268, :1347-1358
            if bi[j] < 0 or p.bad or k in p.obs:
                continue
            inkf = k.mps[bi[j]]
            if inkf is not None:
                if not inkf.bad:
                    reps[j] = inkf
            else:
                p.obs[k] = int(bi[j]); k.mps[bi[j]] = p; touched.append((k, int(bi[j]), p.id)); sf_added.append((k.m, int(bi[j]), p.id))
        for j, rep in enumerate(reps):
            if rep is not None:
                if rep.obs:
                    sf_replaced.append((k.m, rep.id, loop_pts[j].id))
                touched += replace(rep, loop_pts[j])
    last = {}
    for k, i, v in touched:
        last[(k.slot, i)] = v
    stages.update_map_points([a for a, _ in last], [b for _, b in last], list(last.values()))
    out.update(sf_replaced=sf_replaced, sf_added=sf_added)
    # ---------------------------------------------------------------- LoopConnections, :545-563
    previous = {k: list(k.ordered) for k in connected}
    stages.covis_build([k.slot for k in kfs])
    update_connections(stages, kfs, kfs)
    loop_conn = {k: set(k.ordered) - set(previous[k]) - set(connected) for k in connected}
    out["loop_connections"] = [[k.m] + sorted(x.m for x in loop_conn[k]) for k in sorted(loop_conn, key=lambda k: k.m)]
    # ---------------------------------------------------------------- OptimizeEssentialGraph, Optimizer.cpp:650-885
    verts = sorted(kfs, key=lambda k: k.mn_id)
    v_of = {k: v for v, k in enumerate(verts)}
    vScw = [corrected[k] if k in corrected else ns.sim3_from_Rts(k.R, k.t, 1.0) for k in verts]
    vSnc = [non_corrected.get(k, vScw[v_of[k]]) for k in verts]
    edges, inserted = [], set()
    for k in sorted(loop_conn, key=lambda k: k.m):                  # :693-722
        for n in sorted(loop_conn[k], key=lambda k: k.m):
            if (k is not cur or n is not matched_kf) and k.weights.get(n, 0) < 100:
                continue
            edges.append((v_of[k], v_of[n], 0)); inserted.add((min(k.mn_id, n.mn_id), max(k.mn_id, n.mn_id)))
    for k in kfs:                                                   # :724-825
        if k.parent is not None:
            edges.append((v_of[k], v_of[k.parent], 1))
        for n in sorted(k.loop_edges, key=lambda k: k.m):
            if n.mn_id < k.mn_id:
                edges.append((v_of[k], v_of[n], 1))
        for n in k.ordered:                                         # GetCovisiblesByWeight(100)
            if k.weights[n] < 100:
                break
            if n is k.parent or n in k.children or n in k.loop_edges:
                continue
            if n.mn_id < k.mn_id and (min(k.mn_id, n.mn_id), max(k.mn_id, n.mn_id)) not in inserted:
                edges.append((v_of[k], v_of[n], 1))
    graph = dict(Scw=np.stack([ne.to8(S) for S in vScw]), Snc=np.stack([ne.to8(S) for S in vSnc]), fixed=v_of[matched_kf], edges=np.array(edges, np.int32).reshape(-1, 3), fix_scale=0)
    r = stages.essential_graph(api.ess_graph_job_state(graph))
    out.update(edges=[tuple(int(x) for x in e) for e in edges], eg_iterations=int(r["iterations_run"]))
    S_out = [ne.from8(x) for x in r["S"]]
    for v, k in enumerate(verts):                                   # :834-852
        q, t, s = S_out[v]
        k.set_pose(ns.quat_to_R(q), t * (1. / s))
    stages.update_poses([k.slot for k in verts], np.array([k.R.astype(f32).reshape(9) for k in verts]), np.array([k.t.astype(f32) for k in verts]), np.array([k.centre() for k in verts]))
    live = [p for p in sorted(mps.values(), key=lambda p: p.id) if not p.bad and p.obs]
    for p in live:                                                  # :855-885
        ref = p.corrected_ref if p.corrected_by == cur.mn_id else p.ref_kf
        p.pos = ns.sim3_map(ns.sim3_inverse(S_out[v_of[ref]]), ns.sim3_map(vScw[v_of[ref]], p.pos)).astype(f32).astype(f64)
    refresh(stages, sc, live)
    out.update(eg_ids=[p.id for p in live], eg_pos=np.array([p.pos for p in live], f32), eg_poses=np.array([np.concatenate([k.R.reshape(9), k.t]) for k in kfs], f32))
    # ---------------------------------------------------------------- the global BA, Optimizer.cpp:453-621
    nkp = max(len(k.mps) for k in kfs)
    keys = np.zeros((len(kfs), nkp, 2), f32); octave = np.zeros((len(kfs), nkp), np.int32); rays = np.zeros((len(kfs), nkp, 3), f32); rays[..., 2] = 1
    Tcw = np.zeros((len(kfs), 4, 4), f32)
    for k in kfs:
        n = len(k.mps)
        keys[k.m, :n, 0] = k.kf["x"]; keys[k.m, :n, 1] = k.kf["y"]; octave[k.m, :n] = k.kf["octave"]
        _, ray = synth.pixel_to_ray(F, k.kf["x"].astype(f64), k.kf["y"].astype(f64))
        rays[k.m, :n] = (ray / np.linalg.norm(ray, axis=1, keepdims=True)).astype(f32)
        Tcw[k.m] = np.eye(4); Tcw[k.m, :3, :3] = k.R; Tcw[k.m, :3, 3] = k.t
    m = dict(F=F, n_list=len(kfs), kf_id=np.array([k.mn_id for k in kfs], np.int64), kf_bad=np.zeros(len(kfs), np.uint8), Tcw=Tcw, keys=keys, octave=octave, rays=rays,
             inv_level_sigma2=INV_SIGMA2, mp_id=np.array([p.id for p in live], np.int64), mp_bad=np.zeros(len(live), np.uint8), Xw=np.array([p.pos for p in live], f32),
             obs_off=np.concatenate([[0], np.cumsum([len(p.obs) for p in live])]).astype(np.int32), obs_kf=np.array([k.m for p in live for k in p.obs], np.int32),
             obs_kp=np.array([i for p in live for i in p.obs.values()], np.int32))
    prob = gba_hostlib.collect(m)
    g = stages.global_ba(prob)
    for v, km in enumerate(prob["vertex_kf"]):
        T = harness._T_from_pose7(g["poses"][v])
        kfs[km].set_pose(T[:3, :3], T[:3, 3])
    for v, j in enumerate(prob["vertex_mp"]):
        live[j].pos = g["points"][v].astype(f32).astype(f64)
    out.update(gba_iterations=int(g["iterations_done"]), final_ids=[p.id for p in live], final_pos=np.array([p.pos for p in live], f32),
               final_centres=np.array([k.centre() for k in kfs], f32))
    return out
