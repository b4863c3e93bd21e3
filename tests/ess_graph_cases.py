"""Seeded graphs for the OptimizeEssentialGraph tests (numpy only, so the GPU tests can build them where they run): a ring of N key frames with
drift in scale and rotation; chain edges i -> i - span for the given spans (kind 1: measured from the non-corrected poses, :724-825); the last
`ncorr` key frames corrected by one Sim3 of about 0.03 rad, 0.3 m and scale e^0.1 (none under fix_scale), so Snc != Scw on that tail only; loop-
connection edges from the tail to the far side (kind 0: measured from Scw, :693-722), added first as the reference adds them; a fixed vertex that is
not vertex 0 unless asked for."""
import numpy as np

import npref_essential_graph as ne
import npref_sim3_opt as ns


def _rot(ax, a):
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def graph(seed, N, fix_scale=0, fixed=None, ncorr=None, spans=(1, 3), loop="far", double_edge=False):
    """loop: "far" (every tail vertex to fixed + i % 3), "fixed" (every tail vertex to the fixed vertex), "last_first" (one kind-0 edge from the last to
    the first free vertex), "none".  double_edge: the first chain edge once more as a kind-0 edge, so one pair carries two edges."""
    rng = np.random.default_rng(seed)
    fixed = min(3, N - 1) if fixed is None else int(fixed)
    ncorr = min(6, max(1, N // 3)) if ncorr is None else int(ncorr)
    est = []
    for i in range(N):
        a = 2 * np.pi * i / N * (1 + 0.02)
        R = _rot(np.array([0, 1, .05 * i / N]), a)
        c = (1 + 0.1 * i / N) * np.array([5 * np.cos(a), 0.02 * i * 40.0 / max(N, 40), 5 * np.sin(a)])
        est.append(ns.sim3_from_Rts(R, -R @ c, 1.0))
    corr = ns.sim3_exp(np.concatenate([rng.normal(0, .03, 3), rng.normal(0, .3, 3), [0. if fix_scale else 0.1]]))
    S = list(est)
    tail = list(range(N - ncorr, N)) if N > 1 else []
    for i in tail:
        S[i] = ns.sim3_times(est[i], corr)
    edges = []
    free = [v for v in range(N) if v != fixed]
    if loop in ("far", "fixed"):
        for i in tail:
            j = fixed if loop == "fixed" else (fixed + i % 3) % N
            if j != i and j not in tail:
                edges.append((i, j, 0))
    elif loop == "last_first" and len(free) > 1:
        edges.append((free[-1], free[0], 0))
    for i in range(1, N):
        for sp in spans:
            if i >= sp:
                edges.append((i, i - sp, 1))
    if double_edge and N > 2:
        a, b = [(i, j) for i, j, k in edges if k == 1 and i != fixed and j != fixed][0]
        edges.append((a, b, 0))
    return dict(N=N, Scw=np.stack([ne.to8(s) for s in S]), Snc=np.stack([ne.to8(s) for s in est]), fixed=fixed,
                edges=np.array(edges, np.int32).reshape(-1, 3), fix_scale=int(fix_scale), tail=tail)


def points(seed, n, K):
    """n map points with a reference key frame in [0, K), a tenth of them without (ref < 0)"""
    rng = np.random.default_rng(seed)
    pos = rng.normal(0, 4, (n, 3)).astype(np.float32)
    ref = rng.integers(0, max(K, 1), n).astype(np.int32)
    ref[rng.uniform(size=n) < 0.1] = -1
    return pos, ref


def broken_states(good):
    """(what, states) for every cause of CMS_ERR_ARG that lies in a job record"""
    def broken(j=1, **kw):
        st = good()
        st[j].update(kw)
        return st
    out = [("null Scw", broken(Scw=None)), ("null Snc", broken(Snc=None)), ("null S_out", broken(S_out=None)), ("null Tiw_out", broken(Tiw_out=None)),
           ("null edges", broken(edges=None)), ("fixed -1", broken(fixed=-1)), ("fixed N", broken(fixed=good()[1]["N"])), ("iterations -1", broken(iterations=-1))]
    for lam in (0.0, -1e-16, float("nan"), float("inf")):
        out.append(("lambda %r" % lam, broken(lambda_init=lam)))
    for what, edge in (("index N", (3, good()[1]["N"], 1)), ("index -1", (-1, 2, 0)), ("v0 == v1", (4, 4, 1)), ("kind 2", (4, 3, 2)), ("kind -1", (4, 3, -1))):
        st = good(); st[1]["edges"][5] = edge
        out.append((what, st))
    for what, key, col, val in (("nan", "Scw", 2, float("nan")), ("inf", "Snc", 5, float("inf")), ("s 0", "Scw", 7, 0.0), ("s < 0", "Snc", 7, -1.0)):
        st = good(); st[0][key][3, col] = val
        out.append((what, st))
    st = good()      # a vertex with no path to fixed: the last vertex loses its edges to a pair among the others
    e = st[1]["edges"]; last = st[1]["N"] - 1
    e[(e[:, 0] == last) | (e[:, 1] == last)] = (1, 0, 1)
    out.append(("no path", st))
    return out


# a handle of (max_jobs, max_vertices_total, max_edges_total, max_envelope_blocks_total) and calls of graph() arguments that exceed one capacity each
SMALL_HANDLE = (2, 75, 120, 200)
GOOD_CASE = [((91, 12, 0), {}), ((92, 20, 1), {})]                                       # 32 vertices, 66 edges, 140 blocks
CAPACITY_CASES = [("jobs", [((93, 5, 0), {})] * 3),
                  ("vertices", [((94, 40, 0), {}), ((95, 40, 0), {})]),                  # 80 vertices; 82 edges each
                  ("edges", [((96, 40, 0), dict(spans=(1, 2, 3, 4), loop="none"))])]    # 150 edges
OVERFLOW_CASE = [((97, 70, 0), dict(spans=(1,), loop="last_first"))]                     # 70 edges, 69 + 66 + 68 = 203 blocks


def mirror_case(seed=7, fix_scale=0):
    """A small map for Optimizer::OptimizeEssentialGraph's mirror that exercises every rule of :650-825: 14 key frames on the ring whose mnIds do not
    follow their index, one of them bad; a spanning tree; an old loop edge; covisibles by descending weight, among them the parent, a child and the loop-edge
    partner (all >= minFeat and to be left out), neighbours under minFeat, and one pair the loop connections insert first; LoopConnections with a pair
    under minFeat (dropped), pairs over it, and (pCurKF, pLoopKF) under minFeat (exempt).  The last four key frames in mnId order carry corrected poses.
    Map points hang on reference key frames; a few were corrected by pCurKF and name mnCorrectedReference, a few are bad."""
    rng = np.random.default_rng(seed)
    nkf = 14
    g = graph(seed, nkf, fix_scale, ncorr=4, loop="none")
    order = rng.permutation(nkf)                      # key frame index -> position on the ring
    mnId = [int(2 * order[i] + 1) for i in range(nkf)]
    at = {int(order[i]): i for i in range(nkf)}       # ring position -> key frame index
    bad_pos = 5
    kfs = []
    for i in range(nkf):
        pos = int(order[i])
        q, t, s = ne.from8(g["Snc"][pos])
        T = np.zeros((3, 4), np.float32); T[:, :3] = ns.quat_to_R(q).astype(np.float32); T[:, 3] = t.astype(np.float32)
        parent = -1 if pos == 0 else at[pos - 1 if pos - 1 != bad_pos else pos - 2]      # the bad key frame's child was handed to its grandparent
        kfs.append(dict(mnId=mnId[i], bad=pos == bad_pos, Tcw=T.ravel(), parent=parent, children=set(), loop_edges=set(), cov=[], cov_w=[], pos=pos))
    for i, k in enumerate(kfs):
        if k["parent"] >= 0:
            kfs[k["parent"]]["children"].add(i)
    cur, loop = at[nkf - 1], at[1]
    kfs[at[9]]["loop_edges"].add(at[2]); kfs[at[2]]["loop_edges"].add(at[9])             # an old loop edge
    w = {}
    for a in range(nkf):
        for b in range(a):
            d = a - b
            w[(a, b)] = 260 if d == 1 else (150 if d == 2 else (110 if d == 3 else (60 if d == 4 else 0)))
    w[(9, 2)] = 140                                   # the loop-edge partners see each other
    w[(12, 2)] = 120; w[(11, 1)] = 130                # loop connections over minFeat ...
    w[(12, 3)] = 40                                   # ... one under it ...
    w[(13, 1)] = 15                                   # ... and (pCurKF, pLoopKF) under it: exempt
    w[(12, 0)] = 105                                  # a covisible pair that is no loop connection
    for a in range(nkf):
        nb = sorted([(w.get((max(a, b), min(a, b)), 0), b) for b in range(nkf) if b != a and w.get((max(a, b), min(a, b)), 0) > 0], key=lambda x: (-x[0], x[1]))
        kfs[at[a]]["cov"] = [at[b] for _, b in nb]; kfs[at[a]]["cov_w"] = [int(x) for x, _ in nb]
    loop_connections = {at[12]: {at[2], at[3]}, at[11]: {at[1]}, at[13]: {at[1], at[0]}}
    tail = [10, 11, 12, 13]
    corrected = {at[p]: g["Scw"][p].copy() for p in tail}
    non_corrected = {at[p]: g["Snc"][p].copy() for p in tail}
    nmp = 90
    mp_pos = rng.normal(0, 4, (nmp, 3)).astype(np.float32)
    mp_ref = np.array([at[int(p)] for p in rng.integers(0, nkf, nmp)], np.int32)
    mp_ref[mp_ref == at[bad_pos]] = at[0]
    mp_bad = (rng.uniform(size=nmp) < 0.1).astype(np.uint8)
    by = rng.uniform(size=nmp) < 0.2
    mp_by = np.where(by, mnId[cur], 0).astype(np.int32)
    mp_cref = np.where(by, np.array([mnId[at[int(p)]] for p in rng.integers(8, nkf, nmp)]), 0).astype(np.int32)
    return dict(kfs=kfs, cur=cur, loop=loop, loop_connections=loop_connections, corrected=corrected, non_corrected=non_corrected, fix_scale=int(fix_scale),
                mp_pos=mp_pos, mp_ref=mp_ref, mp_bad=mp_bad, mp_by=mp_by, mp_cref=mp_cref)
