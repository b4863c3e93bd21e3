"""Named cases of the local BA window (csrc/cms_ba_window_core.h), shared by tests/test_ba_window_cpu.py (host core against the restatement
tests/npref_ba_window.py) and tests/test_gpu_ba_window.py (device against host core).  A case is a small synthetic map: per member the slot it lives
in, its mp row, octaves, key points (on all five faces, a few in a corner block that belongs to no face), key rays (a few with z below cos_fov) and
a float pose; the rows of the table that hold a position; and the jobs (local members in list order, first_member).  Ids reach max_points - 1."""
import numpy as np

import npref_reloc
from cubemapslam_amd import synth

F = 150
CAMD = synth.camera("lafida", F)
NLEVELS = 8
SF = npref_reloc.scale_factors(1.2, NLEVELS)
INV_SIGMA2 = (np.float32(1.0) / (SF * SF).astype(np.float32)).astype(np.float32)
f32 = np.float32
NAMES = ("tiny", "fixed_order", "first_member", "filters", "waves", "many_members", "group")
# face -> (column, row) of its block in the 3 x 3 cubemap: 0 front, 1 left, 2 right, 3 upper, 4 lower
BLOCK = {0: (1, 1), 1: (0, 1), 2: (2, 1), 3: (1, 0), 4: (1, 2)}
CORNER = (0, 0)


def rotation(rng, kind):
    """float32 rotation: kind 0 a random one, 1..3 a turn of nearly 180 degrees about x, y, z (trace < 0: the quaternion's three other branches)"""
    if kind == 0:
        q = rng.normal(size=4)
    else:
        q = np.zeros(4); q[kind - 1] = 1.0; q += rng.normal(scale=0.02, size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(f32)


def member(rng, row, kind=0, corner=(), low_ray=()):
    """a member around an mp row: features listed in `corner` get a key point in the corner block, those in `low_ray` a ray with z = -0.5"""
    row = np.asarray(row, np.int32)
    n = len(row)
    face = rng.integers(0, 5, n)
    col = np.array([BLOCK[int(f)][0] for f in face]); r = np.array([BLOCK[int(f)][1] for f in face])
    for f in corner:
        col[f], r[f] = CORNER
    x = (col * F + rng.uniform(0.5, F - 0.5, n)).astype(f32); y = (r * F + rng.uniform(0.5, F - 0.5, n)).astype(f32)
    rays = rng.normal(size=(n, 3)); rays[:, 2] = np.abs(rays[:, 2]) + 0.05
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    rays = rays.astype(f32)
    for f in low_ray:
        rays[f] = (0.5, 0.7, -0.5)
    return dict(mp=row, oct=rng.integers(0, NLEVELS, n).astype(np.int32), x=x, y=y, rays=rays, R=rotation(rng, kind), t=rng.normal(scale=3.0, size=3).astype(f32))


def make(name, members, jobs, max_points, caps, slots=None, seed=0):
    rng = np.random.default_rng(1000 + seed)
    M = len(members)
    slots = list(rng.permutation(M + 2)[:M]) if slots is None else list(slots)      # members do not sit in their own slot numbers
    ids = np.unique(np.concatenate([m["mp"][m["mp"] >= 0] for m in members] + [np.zeros(0, np.int32)])).astype(np.int32)
    assert len(ids) == 0 or ids.max() < max_points
    pos = rng.normal(scale=5.0, size=(len(ids), 3)).astype(f32)
    ref = np.array([slots[min(m for m in range(M) if i in members[m]["mp"])] for i in ids], np.int32) if M <= 16 else np.full(len(ids), slots[0], np.int32)
    return dict(name=name, members=members, slots=[int(s) for s in slots], K=M + 2, maxf=max(1, max(len(m["mp"]) for m in members)), max_points=int(max_points),
                pos_ids=ids, pos=pos, ref=ref, jobs=[(list(j[0]), int(j[1])) for j in jobs], caps=tuple(caps))


def fixed_order_members(rng):
    """8 members, locals 2 and 5: the local points are 10 11 12 13 14 15.  Member 7 meets point 10 (list position 0), members 3 and 4 both meet 11 first,
    member 0 meets 13 (position 3), member 1 meets 15 (position 5), member 6 none: lFixedCameras is 7 3 4 0 1, not the member order"""
    rows = {0: [40, 13, 41], 1: [15, 42], 2: [10, 11, 12, 13], 3: [43, 11], 4: [11, 15, 44], 5: [14, 11, 15], 6: [99, 45], 7: [46, 47, 10]}
    return [member(rng, rows[m], kind=m % 4) for m in range(8)]


FIXED_ORDER_KF = [2, 5, 7, 3, 4, 0, 1]


def tiny_members(rng, base):
    """3 members, 5 points, all in member 0's row; members 1 and 2 observe nothing of it"""
    return [member(rng, [base + 4, base, -1, base + 2, base + 1, base + 3]), member(rng, [base + 7, -1]), member(rng, [base + 8])]


def windowed_map(rng, M, nfeat, per_member, stride, width, max_points):
    """M members of nfeat features; member m holds per_member ids drawn from a window of the id pool that moves by `stride` per member, so neighbours in
    position share points.  The pool is a random subset of [0, max_points) that holds max_points - 1"""
    n_pool = stride * M + width
    pool = rng.permutation(max_points - 1)[:n_pool - 1].astype(np.int32)
    pool = np.concatenate([pool, [max_points - 1]]).astype(np.int32)
    pool = pool[rng.permutation(n_pool)]
    members = []
    for m in range(M):
        row = np.full(nfeat, -1, np.int32)
        ids = pool[m * stride + rng.permutation(width)[:per_member]]
        row[rng.permutation(nfeat)[:per_member]] = ids
        n_bad = max(1, nfeat // 40)
        members.append(member(rng, row, kind=(m % 9) % 4 if m % 9 < 4 else 0, corner=rng.permutation(nfeat)[:n_bad], low_ray=rng.permutation(nfeat)[:n_bad]))
    return members


_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = _case(name)
    return _CACHE[name]


def _case(name):
    rng = np.random.default_rng(sum(ord(ch) for ch in name))
    if name == "tiny":
        return make(name, tiny_members(rng, 1015), [([0], -1)], 1024, (4, 8, 8))
    if name == "fixed_order":
        return make(name, fixed_order_members(rng), [([2, 5], -1)], 128, (8, 8, 32))
    if name == "first_member":      # the member of mnId 0 among the locals, among the fixed ones, nowhere
        return make(name, fixed_order_members(rng), [([2, 5], 5), ([2, 5], 3), ([2, 5], -1), ([2, 5], 6)], 128, (8, 8, 32))
    if name == "filters":
        # locals 0 and 1.  id 20: both observations dropped (a low ray in member 0, a corner key point in member 2): it stays in P without an edge.
        # id 21: member 0's ray is low, member 3 keeps its edge; id 22: member 1 lies in the corner, member 2 keeps; member 4 holds no point at all
        ms = [member(rng, [20, 21, 23, -1, 24], low_ray=[0, 1]), member(rng, [22, 25, 23], corner=[0]), member(rng, [26, 20, 22], corner=[1]),
              member(rng, [21, 25, 27], low_ray=[2]), member(rng, [-1, -1, -1])]
        return make(name, ms, [([0, 1], -1), ([4], -1), ([1, 4, 0], 0)], 64, (8, 16, 32))
    if name == "waves":             # more than one wavefront of members; the point list and the edge list pass 1 024
        ms = windowed_map(rng, 70, 300, 220, 60, 700, 1 << 16)
        return make(name, ms, [([30 + (7 * k) % 25 for k in range(25)], 31)], 1 << 16, (70, 6000, 24000))
    if name == "many_members":      # more than one member per thread of a 1 024-thread workgroup; locals and fixed ones beyond position 1 024
        ms = windowed_map(rng, 1100, 12, 10, 3, 40, 1 << 14)
        return make(name, ms, [([1099 - (11 * k) % 40 for k in range(40)], 1050)], 1 << 14, (128, 512, 2048))
    if name == "group":             # three jobs of different sizes in one call: tiny's, waves' and a middle one
        ms = windowed_map(rng, 70, 300, 220, 60, 700, 1 << 16)
        used = set(int(v) for m in ms for v in m["mp"])
        base = next(b for b in range(100, 60000) if not used & set(range(b, b + 9)))
        ms += tiny_members(rng, base)
        return make(name, ms, [([70], -1), ([30 + (7 * k) % 25 for k in range(25)], 31), ([5, 4, 6, 3, 7], 0)], 1 << 16, (70, 6000, 24000))
    raise KeyError(name)


def concat(c):
    """the members' arrays concatenated, as hm_ba_window_create takes them"""
    ms = c["members"]
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(m[k]).reshape(-1) for m in ms]), dt)
    return dict(n=np.array([len(m["mp"]) for m in ms], np.int32), mp=cat("mp", np.int32), oct=cat("oct", np.int32), x=cat("x", f32), y=cat("y", f32),
                ray_z=np.ascontiguousarray(np.concatenate([m["rays"][:, 2] for m in ms]), f32), R=cat("R", f32), t=cat("t", f32))


KEYS_INT = ("counts", "kf_member", "point_id", "fixed", "e_pose", "e_point", "e_face", "e_feat")
KEYS_F64 = ("poses", "points", "e_obs", "e_invsig2")


def difference(want, got):
    """None, or the first (job, key) at which two lists of windows differ; doubles are compared by value with array_equal, as the integers"""
    if len(want) != len(got):
        return "number of windows", len(want), len(got)
    for j, (w, g) in enumerate(zip(want, got)):
        for k in KEYS_INT + KEYS_F64:
            a, b = np.asarray(w[k]), np.asarray(g[k])
            if a.shape != b.shape or not np.array_equal(a, b):
                return j, k, a.shape, b.shape
    return None


def to_text(c, cos_fov, counts):
    """the case for tests/emu/ba_window_core_emu.cpp (its head comment has the format); floats travel as their bits; counts: per job K n_local P E"""
    b = lambda a: " ".join(str(int(v)) for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))
    ms = c["members"]
    out = ["case %s %d %s %d %d %d %d %d %d %d" % ((c["name"], F, b([cos_fov]), len(ms), c["max_points"], len(c["pos_ids"]), len(c["jobs"])) + tuple(c["caps"]))]
    out.append(b(np.concatenate([INV_SIGMA2, np.zeros(16 - NLEVELS, f32)])))
    for m in ms:
        xb, yb, zb = (np.ascontiguousarray(v, f32).view(np.uint32) for v in (m["x"], m["y"], m["rays"][:, 2]))
        out.append("%d %s" % (len(m["mp"]), " ".join("%d %d %d %d %d" % (m["mp"][f], m["oct"][f], xb[f], yb[f], zb[f]) for f in range(len(m["mp"])))))
        out.append(b(m["R"]) + " " + b(m["t"]))
    for i, p in zip(c["pos_ids"], c["pos"]):
        out.append("%d %s" % (i, b(p)))
    for (mem, first), n in zip(c["jobs"], counts):
        out.append("%d %d %s %s" % (len(mem), first, " ".join(str(v) for v in mem), " ".join(str(int(v)) for v in n)))
    return "\n".join(out) + "\n"
