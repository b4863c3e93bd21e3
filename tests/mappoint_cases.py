"""Named cases of the map-point table, shared by tests/test_mappoints_cpu.py (host core against the oracle) and tests/test_gpu_mappoints.py (device
against host core and oracle).  A case is a map (per member: the slot it lives in, the mp row, the octaves, the descriptors and the camera centre)
and the points to refresh (id, world position, reference slot).  A backend (tests/mappoint_hostlib.py) offers load / set / erase / refresh / fetch;
run() is load -> set -> refresh(both halves) -> fetch, and expected() is what orc.distinctive_descriptors and orc.update_normal_and_depth make of the
observation lists the case builds in ASCENDING MEMBER ORDER, on top of empty rows.  Every comparison is exact: same() compares floats by their bits."""
import numpy as np

import npref_covis
import npref_reloc
import orc

K, MAXF = 64, 256
MAX_POINTS = 1024
NLEVELS = 8
SF = npref_reloc.scale_factors(1.2, NLEVELS)
DESCRIPTOR, NORMAL_DEPTH, BOTH = 1, 2, 3
f32 = np.float32


def make(rows, octs, descs, Ows, slots, ids, pos, ref, K_=K, maxf=MAXF, name=""):
    rows = [np.asarray(r, np.int32) for r in rows]
    octs = [np.asarray(o, np.int32) for o in octs]
    descs = [np.ascontiguousarray(d, np.uint8).reshape(len(r), 32) for d, r in zip(descs, rows)]
    Ows = [np.asarray(o, np.float32).reshape(3) for o in Ows]
    assert len(set(slots)) == len(slots) and all(len(r) <= maxf for r in rows) and max(slots) < K_
    return dict(rows=rows, octs=octs, descs=descs, Ows=Ows, slots=list(slots), ids=np.asarray(ids, np.int32), pos=np.asarray(pos, np.float32).reshape(-1, 3),
                ref=np.asarray(ref, np.int32), K=K_, maxf=maxf, name=name)


def permuted(c, order, name):
    """the same slots listed in another member order"""
    g = lambda k: [c[k][m] for m in order]
    return make(g("rows"), g("octs"), g("descs"), g("Ows"), g("slots"), c["ids"], c["pos"], c["ref"], c["K"], c["maxf"], name)


def observations(c, id_):
    """(member, feature, octave) of an id in ascending member position"""
    out = []
    for m, r in enumerate(c["rows"]):
        f = np.flatnonzero(r == id_)
        assert len(f) <= 1
        if len(f):
            out.append((m, int(f[0]), int(c["octs"][m][f[0]])))
    return out


def empty_rows(n):
    return dict(pos=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32), min_dist=np.zeros(n, f32), max_dist=np.zeros(n, f32), desc=np.zeros((n, 32), np.uint8),
                best_member=np.full(n, -1, np.int32), best_feature=np.full(n, -1, np.int32))


def oracle_refresh(c, ids, pos, ref, what=BOTH, rows=None, Ows=None):
    """status and rows after a refresh of `ids` over rows `rows` (default: empty ones holding pos); Ows: the camera centres at that moment"""
    ids = np.asarray(ids, np.int32); pos = np.asarray(pos, f32).reshape(-1, 3); ref = np.asarray(ref, np.int32)
    Ows = c["Ows"] if Ows is None else Ows
    out = empty_rows(len(ids)) if rows is None else {k: v.copy() for k, v in rows.items()}
    out["pos"] = pos.copy()
    status = np.zeros(len(ids), np.uint8)
    live, obs_off, odesc, oOw, refOw, reflev, lists = [], [0], [], [], [], [], []
    for i, id_ in enumerate(ids):
        obs = observations(c, int(id_))
        if not obs:
            status[i] = 1
            continue
        kref = [k for k, (m, f, o) in enumerate(obs) if c["slots"][m] == int(ref[i])]
        if (what & NORMAL_DEPTH) and not kref:
            status[i] = 2
            continue
        live.append(i); lists.append(obs)
        obs_off.append(obs_off[-1] + len(obs))
        odesc += [c["descs"][m][f] for m, f, o in obs]; oOw += [Ows[m] for m, f, o in obs]
        refOw.append(Ows[obs[kref[0]][0]] if kref else np.zeros(3, f32)); reflev.append(obs[kref[0]][2] if kref else 0)
    if live:
        obs_off = np.asarray(obs_off, np.int32)
        if what & DESCRIPTOR:
            best = orc.distinctive_descriptors(obs_off, np.stack(odesc))
            for j, i in enumerate(live):
                m, f, o = lists[j][int(best[j])]
                out["desc"][i] = c["descs"][m][f]; out["best_member"][i] = m; out["best_feature"][i] = f
        if what & NORMAL_DEPTH:
            nrm, mn, mx = orc.update_normal_and_depth(obs_off, pos[live], np.stack(oOw), np.stack(refOw), np.asarray(reflev, np.int32), SF)
            for j, i in enumerate(live):
                out["normal"][i] = nrm[j]; out["min_dist"][i] = mn[j]; out["max_dist"][i] = mx[j]
    return status, out


def medians(c, id_):
    """the row medians of the Hamming matrix of an id's observations, in member order (numpy, for the conditions on the inputs)"""
    obs = observations(c, id_)
    D = np.stack([c["descs"][m][f] for m, f, o in obs])
    H = np.unpackbits(D[:, None, :] ^ D[None, :, :], axis=2).sum(axis=2)
    return np.sort(H, axis=1)[:, int(0.5 * (len(obs) - 1))]


def flipped(base, nflip, rng):
    d = base.copy()
    for b in rng.choice(256, nflip, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _known3():
    """three key frames by hand.  Camera centres and positions make every ni an axis vector of length 4 or 2: the sums are exact.
    id 10: all three, descriptors 0 bits / 8 bits / 2 of those 8 -> medians 2, 6, 2: the tie goes to member 0.  Reference = member 1 (octave 2).
    id 11: members 0 and 2, N = 2: both medians are the row's own 0, member 0 wins.  Reference = member 0 (octave 0).
    id 12: member 1 alone.  Reference = member 1 (octave 3).
    id 13: all three, descriptors 32 bits / 0 bits / 1 bit -> medians 32, 1, 1: member 1 wins.  Reference = member 2, the last (octave 1)."""
    z = np.zeros(32, np.uint8)
    b8 = z.copy(); b8[0] = 0xFF
    b2 = z.copy(); b2[0] = 0x03
    b32 = z.copy(); b32[:4] = 0xFF
    b1 = z.copy(); b1[31] = 0x80
    junk = np.full(32, 0xA5, np.uint8)
    rows = [[10, 11, 13, -1], [13, 10, 12], [-1, 11, 10, 13]]
    octs = [[5, 0, 6, 7], [4, 2, 3], [7, 6, 5, 1]]
    descs = [[z, z, b32, junk], [z, b8, junk], [junk, b1, b2, b1]]
    Ows = [[0, 0, 0], [4, 0, 4], [0, -2, 4]]
    slots = [5, 12, 19]
    ids = [10, 11, 12, 13]
    pos = [[0, 0, 4], [0, -2, 0], [4, 0, 0], [0, 0, 4]]
    ref = [12, 5, 12, 19]
    return make(rows, octs, descs, Ows, slots, ids, pos, ref, name="known3")


def known3_by_hand():
    third = f32(1.0 / 3.0)
    e = empty_rows(4)
    z = np.zeros(32, np.uint8)
    e["pos"] = np.array([[0, 0, 4], [0, -2, 0], [4, 0, 0], [0, 0, 4]], f32)
    e["best_member"][:] = [0, 0, 1, 1]; e["best_feature"][:] = [0, 1, 2, 0]
    e["desc"][2] = 0xA5      # member 1's feature 2
    e["normal"][0] = [-third, third, third]      # (0,0,1) + (-1,0,0) + (0,1,0), times (float)(1/3)
    e["normal"][1] = [0, -0.5, -0.5]             # (0,-1,0) + (0,0,-1), times 0.5
    e["normal"][2] = [0, 0, -1]
    e["normal"][3] = [-third, third, third]
    dist = np.array([4, 2, 4, 2], f32)           # |P - Ow_ref|
    lev = [2, 0, 3, 1]
    e["max_dist"] = np.array([f32(d * SF[l]) for d, l in zip(dist, lev)], f32)
    e["min_dist"] = np.array([f32(m / SF[NLEVELS - 1]) for m in e["max_dist"]], f32)
    return np.zeros(4, np.uint8), e


def _random_map(seed, M, F, n_ids, per_row, slots, K_, maxf, nflip=20, name=""):
    rng = np.random.default_rng(seed)
    ids = rng.permutation(MAX_POINTS)[:n_ids]
    base = rng.integers(0, 256, (MAX_POINTS, 32), dtype=np.uint8)
    pos = rng.normal(0, 3, (MAX_POINTS, 3)).astype(f32)
    rows, octs, descs, Ows = [], [], [], []
    for m in range(M):
        r = np.full(F, -1, np.int32)
        r[:per_row] = rng.choice(ids, per_row, replace=False)
        rng.shuffle(r)
        rows.append(r); octs.append(rng.integers(0, NLEVELS, F).astype(np.int32))
        descs.append(np.stack([flipped(base[i], nflip, rng) if i >= 0 else rng.integers(0, 256, 32, dtype=np.uint8) for i in r]))
        Ows.append(rng.normal(0, 2, 3).astype(f32))
    c = make(rows, octs, descs, Ows, slots, np.sort(ids), pos[np.sort(ids)], np.zeros(n_ids, np.int32), K_, maxf, name)
    for i, id_ in enumerate(c["ids"]):      # the reference slot: a random observer's
        obs = observations(c, int(id_))
        c["ref"][i] = c["slots"][obs[int(rng.integers(len(obs)))][0]] if obs else c["slots"][0]
    return c


def _random():
    return _random_map(11, 12, 200, 300, 170, [(5 + 7 * m) % K for m in range(12)], K, MAXF, name="random12x200")


COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 130]


def _counts():
    """130 members in a store of 136 slots x 64 features; point j is observed by COUNTS[j] members chosen at random"""
    rng = np.random.default_rng(5)
    M, F = 130, 64
    slots = [(3 + 11 * m) % 136 for m in range(M)]
    ids = [700 + 3 * j for j in range(len(COUNTS))]
    base = rng.integers(0, 256, (len(ids), 32), dtype=np.uint8)
    rows = [np.full(F, -1, np.int32) for _ in range(M)]
    descs = [rng.integers(0, 256, (F, 32), dtype=np.uint8) for _ in range(M)]
    octs = [rng.integers(0, NLEVELS, F).astype(np.int32) for _ in range(M)]
    Ows = [rng.normal(0, 2, 3).astype(f32) for _ in range(M)]
    ref = []
    for j, (id_, n) in enumerate(zip(ids, COUNTS)):
        members = rng.choice(M, n, replace=False)
        for m in members:
            f = int(rng.choice(np.flatnonzero(rows[m] < 0)))
            rows[m][f] = id_; descs[m][f] = flipped(base[j], 20, rng)
        ref.append(slots[int(members[int(rng.integers(n))])])
    return make(rows, octs, descs, Ows, slots, ids, rng.normal(0, 3, (len(ids), 3)), ref, 136, 64, "counts")


def _ties():
    """eight members listed in DESCENDING slots; every point is seen by 4 to 8 of them, and its observers hold one of only two descriptor variants,
    so whole groups of rows have the same median"""
    rng = np.random.default_rng(9)
    M, F, n_ids = 8, 40, 30
    slots = [61 - 7 * m for m in range(M)]
    ids = np.arange(100, 100 + n_ids)
    rows = [np.full(F, -1, np.int32) for _ in range(M)]
    descs = [rng.integers(0, 256, (F, 32), dtype=np.uint8) for _ in range(M)]
    octs = [rng.integers(0, NLEVELS, F).astype(np.int32) for _ in range(M)]
    Ows = [rng.normal(0, 2, 3).astype(f32) for _ in range(M)]
    ref = []
    for id_ in ids:
        members = rng.choice(M, int(rng.integers(4, M + 1)), replace=False)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        variants = [base, flipped(base, 6, rng)]
        for m in members:
            f = int(rng.choice(np.flatnonzero(rows[m] < 0)))
            rows[m][f] = id_; descs[m][f] = variants[int(rng.integers(2))]
        ref.append(slots[int(members[0])])
    return make(rows, octs, descs, Ows, slots, ids, rng.normal(0, 3, (n_ids, 3)), ref, name="ties")


def _ties_permuted():
    return permuted(case("ties"), [3, 7, 0, 5, 1, 6, 2, 4], "ties_permuted")


_BUILDERS = {"known3": _known3, "counts": _counts, "ties": _ties, "ties_permuted": _ties_permuted, "random12x200": _random}
NAMES = ["known3", "counts", "ties", "ties_permuted", "random12x200"]
_cases, _expected = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def expected(name):
    if name not in _expected:
        c = case(name)
        _expected[name] = oracle_refresh(c, c["ids"], c["pos"], c["ref"])
    return _expected[name]


def run(c, backend):
    backend.load(c)
    backend.set(c["ids"], c["pos"], c["ref"])
    status = backend.refresh(c["ids"], BOTH)
    return status, backend.fetch(c["ids"])


FLOATS = ("pos", "normal", "min_dist", "max_dist")
INTS = ("desc", "best_member", "best_feature")


def rows_difference(want, got):
    for k in FLOATS:
        a, b = np.ascontiguousarray(want[k], f32).view(np.uint32), np.ascontiguousarray(got[k], f32).view(np.uint32)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[0])
            return "%s of row %d: want %s, got %s" % (k, i, want[k][i], got[k][i])
    for k in INTS:
        if not np.array_equal(want[k], got[k]):
            i = int(np.flatnonzero((np.asarray(want[k]) != np.asarray(got[k])).reshape(len(want[k]), -1).any(axis=1))[0])
            return "%s of row %d: want %s, got %s" % (k, i, want[k][i], got[k][i])
    return None


def difference(want, got):
    """None, or where (status, rows) differ"""
    if not np.array_equal(want[0], got[0]):
        return "status: want %s, got %s" % (want[0].tolist(), got[0].tolist())
    return rows_difference(want[1], got[1])


def reference_observations(c):
    """{id: [(member, feature)]} from the restatement of the reference's bookkeeping (tests/npref_covis.py), member = address order"""
    kfs, points = npref_covis.make_map(c["rows"], c["octs"])
    pos = {kf: m for m, kf in enumerate(kfs)}
    return {id_: [(pos[kf], idx) for kf, idx in p.observations()] for id_, p in points.items()}


# ---- the inputs of the two consumer tests: a frame of 500 key points (Lafida, F = 150) with the local map synth.local_map_problem puts behind it, as
# test_search_local_points_matches_oracle builds them, and three observer key frames through which the points enter the table by set + refresh
F_SEARCH = 150
SEARCH_K, SEARCH_MAXF = 8, 1024
OBS_SLOTS = [6, 1, 4]                       # the observers, in member order
TARGET_SLOTS = [0, 3, 5]                    # the Fuse targets


def search_case(F=F_SEARCH, nkp=500, maxf=SEARCH_MAXF, key="search"):
    """(the defaults are the tests' case; tools/prof_mappoints.py asks for a larger frame)"""
    if key in _cases:
        return _cases[key]
    import test_area_emu as te
    from cubemapslam_amd import synth
    kx, ky, ko = te._keypoints(F, nkp, 43)
    kd = synth.descriptors(len(kx), 44)
    pr = synth.local_map_problem(F, kx, ky, ko, kd, seed=45, order="random")
    rng = np.random.default_rng(46)
    n = len(pr["pos"])
    assert n <= maxf and n <= MAX_POINTS * 4
    Ow = pr["pose15"][12:15]
    dist = np.linalg.norm(pr["pos"].astype(np.float64) - Ow.astype(np.float64), axis=1)
    lvl = np.clip(np.rint(np.log(pr["max_dist"] / dist) / np.log(1.2)), 0, NLEVELS - 1).astype(np.int32)      # the level the problem meant
    rows, octs, descs, Ows = [], [], [], []
    for m in range(3):
        perm = rng.permutation(n)
        rows.append(perm.astype(np.int32)); octs.append(lvl[perm])
        descs.append(np.stack([flipped(pr["desc"][i], int(rng.integers(0, 4)), rng) for i in perm]))
        Ows.append((Ow + (0 if m == 0 else 1) * rng.normal(0, 0.05, 3)).astype(f32))      # member 0 stands where the frame does
    c = make(rows, octs, descs, Ows, OBS_SLOTS, np.arange(n), pr["pos"], np.full(n, OBS_SLOTS[0]), SEARCH_K, maxf, key)
    c.update(kx=kx, ky=ky, ko=ko, kd=kd, pose15=pr["pose15"])
    _cases[key] = c
    return c


def fuse_jobs(c):
    """two sets (even and odd ids) shared by six jobs: each set into each of the three targets -> (sets, [(slot, set)])"""
    sets = [c["ids"][0::2], c["ids"][1::2]]
    return sets, [(slot, s) for s in (0, 1) for slot in TARGET_SLOTS]


def fuse_skip(sets, jobs):
    rng = np.random.default_rng(7)
    return [(rng.random(len(sets[s])) < 0.3).astype(np.uint8) for _, s in jobs]


def target_keyframes(c):
    """the Fuse targets: the frame's key points in three arrangements, all at the frame's pose -> [(slot, dict(x, y, octave, desc))]"""
    n = len(c["kx"])
    orders = [np.arange(n), np.arange(n)[::-1], np.arange(0, n - 100)]
    return [(s, dict(x=c["kx"][o].copy(), y=c["ky"][o].copy(), octave=c["ko"][o].copy(), desc=c["kd"][o].copy())) for s, o in zip(TARGET_SLOTS, orders)]
