"""Named cases of the map-point statistics, shared by tests/test_mpstats_cpu.py (host core against the restatement tests/npref_mpstats.py) and
tests/test_gpu_mpstats.py (device against host core).  A case is a function that drives a backend -- npref_mpstats.Model, mpstats_hostlib.HostBackend or
mpstats_hostlib.DeviceBackend, all with the same methods -- and returns a list of (label, value) pairs; difference() compares two such lists exactly:
integers and verdict bytes by value, depths by their bits.  Calls the entries must refuse are made on the two real backends only (`real`); what a
case records after them shows that nothing was written.

Stores (STORES): the two of tests/mappoint_cases.py, 64 slots x 256 features with 1 024 table rows and 136 x 64 for long observation lists, and one
of 4 slots x 4 096 features with 8 192 rows for the outer loops of the selection kernel.  4 096 is the most a key frame may hold
(cms_kfstore_put and cms_kfstore_put_from_frames refuse more), so the longest depth list is 4 095, not the 4 999 a 5 000-feature row would give.
Slot K - 1 of every store stays empty."""
import numpy as np

import mappoint_cases as mc
import npref_mpstats as ref
from mappoint_hostlib import Refused

STORES = dict(std=(mc.K, mc.MAXF, mc.MAX_POINTS), long=(136, 64, mc.MAX_POINTS), big=(4, 4096, 8192))
SF, NLEVELS = mc.SF, mc.NLEVELS
VISIBLE, FOUND = 1, 2
f32 = np.float32


def refused(f, *a, **kw):
    """the reason the call was refused with; fails if it went through"""
    try:
        f(*a, **kw)
    except Refused as e:
        return str(e)
    raise AssertionError("the call was not refused: %s %s" % (getattr(f, "__name__", f), (a, kw)))


def is_real(b):
    return not isinstance(b, ref.Model)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def difference(want, got):
    """None, or the first label whose values differ"""
    if [k for k, _ in want] != [k for k, _ in got]:
        return "labels: %s against %s" % ([k for k, _ in want], [k for k, _ in got])
    for (k, a), (_, b) in zip(want, got):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = bits(a), bits(b)
        if a.shape != b.shape or not np.array_equal(a, b):
            return "%s: want %s, got %s" % (k, a.tolist(), b.tolist())
    return None


# ---------------------------------------------------------------------------------------------------------------------------------------------
# count, set_stats, add_stats, fetch_stats
N_COUNT = 200


def count_jobs():
    """four jobs, 769 entries: one id 130 times (collisions inside and across wavefronts), two jobs sharing ids with -1 entries, an empty job; block
    edges (256, 512, 768) fall inside jobs"""
    rng = np.random.default_rng(21)
    pool = np.concatenate([np.arange(N_COUNT), np.full(40, -1)])
    jobs = [np.full(130, 7), rng.choice(pool, 300), np.zeros(0, np.int64), rng.choice(pool, 339)]
    flags = [rng.integers(0, 2, len(j)).astype(np.uint8) * rng.integers(1, 255, len(j)).astype(np.uint8) for j in jobs]
    assert sum(len(j) for j in jobs) == 769 and len(set(jobs[1]) & set(jobs[3])) > 50 and (jobs[1] < 0).any() and (jobs[3] < 0).any()
    return jobs, flags


def case_count(b):
    out = []
    ids = np.arange(N_COUNT)
    b.set(ids, np.zeros((N_COUNT, 3), f32), np.zeros(N_COUNT, np.int32))
    out.append(("fresh rows", np.stack(b.fetch_stats(ids))))
    jobs, flags = count_jobs()
    b.count(VISIBLE, jobs, flags, 1)                                  # in_view next to the local ids
    b.count(FOUND, jobs, flags, 0)                                    # outlier next to the frame's ids
    b.count(VISIBLE, [jobs[3], jobs[0]], None, 1, ctx=1)              # another frame context, no flags: the sums add up
    b.count(FOUND, [], None, 1)                                       # zero jobs
    b.count(FOUND, [[], []], None, 1)                                 # empty jobs only
    b.count(VISIBLE, [[500, 7, -1]], [[0, 1, 1]], 1)                  # row 500 was never set, but its entry is not counted
    st = np.stack(b.fetch_stats(ids))
    out.append(("after the counts", st))
    if is_real(b):
        for args in ((VISIBLE, [[3, STORES["std"][2]]]), (VISIBLE, [[3, -2]]), (FOUND, [[3, 500]]), (FOUND, [[3, 500]], [[0, 0]], 0), (3, [[3]])):
            refused(b.count, *args)      # beyond the table, below -1, a counted row never set (without and with flags), no such column
        out.append(("after refused counts", np.stack(b.fetch_stats(ids))))
    else:
        out.append(("after refused counts", st))
    b.set_stats([10, 11, 12], first_kf=[5, 6, 0], found=[0, 2, 3])
    b.set_stats([13], visible=[9])
    b.add_stats([11, 12], d_visible=[3, 0])
    b.add_stats([12, 13], None, [4, 1])
    b.set_stats([14], None, None, None)
    if is_real(b):
        for call in (lambda: b.set_stats([20], visible=[0]), lambda: b.set_stats([20], found=[-1]), lambda: b.set_stats([20], first_kf=[-2]),
                     lambda: b.set_stats([20, 20], found=[1, 1]), lambda: b.set_stats([500], found=[1]), lambda: b.set_stats([STORES["std"][2]], found=[1]),
                     lambda: b.add_stats([20], d_visible=[-1]), lambda: b.add_stats([20, 500], d_found=[1, 1]), lambda: b.add_stats([21, 21], d_found=[1, 1])):
            refused(call)
    out.append(("after set and add", np.stack(b.fetch_stats(ids))))
    b.erase([7, 11])
    out.append(("erased rows read (1, 1, -1)", np.stack(b.fetch_stats([7, 11, 12, 600]))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# culling: every branch at its edge.  Three members; ids 100.. are seen by all three, 200.. by the first two, 300.. by none
CULL_SLOTS = [5, 12, 19]
# (id, found, visible, first_kf, the verdict by hand) of job A, current_kf = 10, th_obs = 2
CULL_A = [(100, 1, 4, 10, 0),                      # ratio exactly 0.25: stays
          (101, 1, 5, 10, 1),                      # 0.2: bad
          (102, 4194305, 16777217, 10, 0),         # (float)visible rounds to 2^24: 0.25000006 in float
          (103, 4194304, 16777217, 10, 0),         # 2^22 / 2^24 after the rounding: exactly 0.25, where the exact quotient is below it
          (200, 1, 1, 9, 0),                       # one key frame on, 2 observations
          (201, 1, 1, 8, 2),                       # two on, 2 observations <= th_obs
          (104, 1, 1, 8, 0),                       # two on, 3 observations
          (202, 1, 1, 7, 2),                       # three on, 2 observations: the earlier branch
          (105, 1, 1, 7, 3),                       # three on, 3 observations: leaves the list
          (106, 1, 1, 9, 0),                       # one on, 3 observations
          (107, 1, 1, -1, 3),                      # first_kf never set: eleven on
          (300, 1, 1, 20, 0),                      # first_kf > current_kf: a negative difference, no observation
          (301, 1, 1, 8, 2),                       # unknown to the index: Observations = 0
          (302, 0, 1, 10, 1)]                      # found = 0
CULL_EMPTY = 400                                   # a row never set: 4
# job B, current_kf = 12
CULL_B = [(108, 1, 1, 10, 0), (109, 1, 1, 9, 3), (203, 3, 4, 10, 2), (204, 1, 4, 11, 0)]


def _cull_rows():
    all3 = [r[0] for r in CULL_A + CULL_B if 100 <= r[0] < 200]
    first2 = [r[0] for r in CULL_A + CULL_B if 200 <= r[0] < 300]
    rng = np.random.default_rng(3)
    rows = []
    for m in range(3):
        ids = all3 + (first2 if m < 2 else [])
        row = np.full(70 + 11 * m, -1, np.int32)
        row[rng.choice(len(row), len(ids), replace=False)] = ids
        rows.append(row)
    return rows


def case_culling(b):
    out = []
    for s, row in zip(CULL_SLOTS, _cull_rows()):
        b.put(s, row)
    b.build(CULL_SLOTS)
    rows = CULL_A + CULL_B
    ids = [r[0] for r in rows]
    b.set(ids, np.zeros((len(ids), 3), f32), np.full(len(ids), CULL_SLOTS[0]))
    b.set_stats(ids, [r[3] for r in rows], [r[2] for r in rows], [r[1] for r in rows])
    jobs = [[r[0] for r in CULL_A] + [CULL_EMPTY], [r[0] for r in CULL_B]]
    v = b.culling(jobs, [10, 12], 2, False)
    out += [("verdicts A", v[0]), ("verdicts B", v[1])]
    out.append(("th_obs = 3", np.concatenate(b.culling(jobs, [10, 12], 3, False))))
    out.append(("th_obs = 0, jobs swapped", np.concatenate(b.culling(jobs[::-1], [12, 10], 0, False))))
    out.append(("no job", np.zeros(0, np.uint8) if not b.culling([], [], 2, False) else None))
    out.append(("nothing was applied", np.stack(b.fetch_stats(ids))))
    return out


def culling_by_hand():
    return np.array([r[4] for r in CULL_A] + [4], np.uint8), np.array([r[4] for r in CULL_B], np.uint8)


# ---- culling with apply, on the 136-slot store: id 900 is seen by 70 members, 901 by two, 902 by five, 903 by three
APPLY_M = 130
APPLY_SLOTS = [(3 + 11 * m) % 136 for m in range(APPLY_M)]
APPLY_IDS = [900, 901, 902, 903]


def _apply_rows():
    rng = np.random.default_rng(8)
    rows = [np.full(64, -1, np.int32) for _ in range(APPLY_M)]
    seen = {}
    for id_, n in zip(APPLY_IDS, (70, 2, 5, 3)):
        seen[id_] = sorted(int(m) for m in rng.choice(APPLY_M, n, replace=False))
        for m in seen[id_]:
            rows[m][int(rng.choice(np.flatnonzero(rows[m] < 0)))] = id_
    return rows, seen


def case_culling_apply(b):
    out = []
    rows, seen = _apply_rows()
    if is_real(b):
        b.set([5], np.zeros((1, 3), f32), [0])
        refused(b.culling, [[5]], [3], 2, True)      # no index yet
        b.erase([5])
    for s, row in zip(APPLY_SLOTS, rows):
        b.put(s, row)
    b.build(APPLY_SLOTS)
    b.set(APPLY_IDS, np.ones((4, 3), f32), [APPLY_SLOTS[seen[i][0]] for i in APPLY_IDS])
    b.set_stats(APPLY_IDS, first_kf=[4, 4, 4, 4], visible=[5, 1, 1, 8], found=[1, 1, 1, 2])      # 900: ratio 0.2; 901: two observations; 902, 903 stay
    b.count(VISIBLE, [[903, 903, 902]], None, 1)                                                  # 903: 2 / 10 when the culling runs, behind the count
    # one of 900's entries changes after the build: the application must leave it alone
    m0 = seen[900][10]
    f0 = int(np.flatnonzero(rows[m0] == 900)[0])
    b.update_map_points([APPLY_SLOTS[m0]], [f0], [905])
    if is_real(b):
        refused(b.culling, [[900, 901], [902, 900]], [6, 6], 2, True)      # an id twice
        refused(b.culling, [[900, 1024]], [6], 2, True)
        refused(b.culling, [[900]], [6], -1, True)
    v = b.culling([[900, 902], [901, 903, 904]], [6, 7], 2, True)
    out += [("verdicts", np.concatenate(v))]
    out.append(("mp rows", np.concatenate([b.fetch_mp(s) for s in APPLY_SLOTS])))
    out.append(("the changed entry", b.fetch_mp(APPLY_SLOTS[m0])[f0:f0 + 1]))
    out.append(("counters", np.stack(b.fetch_stats(APPLY_IDS))))
    out.append(("the index is stale", np.array([b.observations(i) for i in APPLY_IDS])))
    out.append(("again: empty rows", np.concatenate(b.culling([APPLY_IDS], [7], 2, True))))
    if is_real(b):
        refused(b.set_stats, [900], found=[1])       # the row is empty on the host side too
    b.build(APPLY_SLOTS)
    out.append(("after the rebuild", np.array([b.observations(i) for i in APPLY_IDS + [905]])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# tracked: rows of 0, 63, 64, 65 and 256 features; id 500 + k is seen by (k % 4) + 1 of the members that have room for it
TRACK_SLOTS = [2, 9, 40, 41, 50]
TRACK_N = [0, 63, 64, 65, 256]


def _track_rows():
    rng = np.random.default_rng(13)
    rows = [np.full(n, -1, np.int32) for n in TRACK_N]
    for k in range(150):
        want = k % 4 + 1
        free = [m for m in range(5) if (rows[m] < 0).sum() > TRACK_N[m] // 5]      # (a fifth of every row stays without a point)
        for m in rng.permutation(free)[:want]:
            rows[m][int(rng.choice(np.flatnonzero(rows[m] < 0)))] = 500 + k
    return rows


def case_tracked(b):
    out = []
    rows = _track_rows()
    for s, row in zip(TRACK_SLOTS, rows):
        b.put(s, row)
    b.build(TRACK_SLOTS)
    members = np.repeat(np.arange(5), 5)
    min_obs = np.tile([0, 1, 2, 3, 4], 5)
    c = b.tracked(members, min_obs)
    out.append(("counts", c))
    out.append(("no job", b.tracked([], [])))
    # a row changes after the build: the snapshot answers
    f = np.flatnonzero(rows[4] >= 0)[:30]
    b.update_map_points(np.full(len(f), TRACK_SLOTS[4]), f, np.full(len(f), -1))
    out.append(("after a change, before the build", b.tracked(members, min_obs, ctx=1)))
    b.build(TRACK_SLOTS)
    out.append(("after the build", b.tracked(members, min_obs)))
    if is_real(b):
        refused(b.tracked, [5], [0]); refused(b.tracked, [-1], [0])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# median depth
def rotation(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return (q * np.sign(np.linalg.det(q))).astype(f32)


def double_sum_case():
    """a pose and a point whose three products do not sum exactly in float: the float-only sum differs from the reference's in the last bit"""
    rng = np.random.default_rng(77)
    R = rotation(5)
    t = np.array([0.3, -0.2, 0.7], f32)
    for _ in range(1000):
        X = rng.normal(0, 3, 3).astype(f32)
        if ref.depth(R, t, X) != ref.depth_float_only(R, t, X):
            return R, t, X
    raise AssertionError("no such point")


def case_median_small(b):
    """the std store: 1, 2, 3, 64, 65, 255, 256 depths and none; q of 1 and 2; ids without a position skipped"""
    out = []
    rng = np.random.default_rng(31)
    counts = [1, 2, 3, 64, 65, 255, 256, 0]
    slots = [1, 4, 8, 15, 16, 23, 42, 30]
    pos = rng.normal(0, 4, (1000, 3)).astype(f32)
    b.set(np.arange(1000), pos, np.zeros(1000, np.int32))
    b.erase(np.arange(900, 1000))                       # ids 900.. have no position
    for s, n in zip(slots, counts):
        row = np.full(256, -1, np.int32)
        row[:n] = rng.choice(900, n, replace=False)
        if n < 250:
            row[n:n + 4] = [950, 1023, 999, 901]        # ... and take no part
        rng.shuffle(row)
        b.put(s, row, None, rotation(s), rng.normal(0, 1, 3).astype(f32))
    for q in (1, 2, 3):
        d, n = b.median_depth(slots, q)
        out += [("depth q=%d" % q, d), ("n q=%d" % q, n)]
    d, n = b.median_depth(slots[::-1][:3], 2)
    out += [("a subset in another order", d), ("n of the subset", n), ("no slot", b.median_depth([], 2)[0])]
    if is_real(b):
        refused(b.median_depth, [1, 4, 1], 2); refused(b.median_depth, [1, 63], 2); refused(b.median_depth, [1], 0); refused(b.median_depth, [64], 2)
    return out


def case_median_edges(b):
    """equal depths around the selected index, negative depths, -0.0f and +0.0f, the current pose and position, the double accumulation"""
    out = []
    I = np.eye(3, dtype=f32)
    # a point on the optical axis: x = y = 0 with the sign of z, so that with R = I every product and the sum keep the sign of a zero
    z = lambda v: np.stack([np.copysign(f32(0), np.asarray(v, f32)), np.copysign(f32(0), np.asarray(v, f32)), np.asarray(v, f32)], axis=1)
    # slot 0: R = I, t = 0: the depth is the point's z.  Seven depths, the middle three equal; q = 2 reads index 3, q = 1 index 6, q = 7 index 0
    b.set(np.arange(7), z([5, 2, 3, 3, 3, -1, 9]), np.zeros(7, np.int32))
    b.put(0, np.arange(7))
    # slot 1: all negative
    b.set(np.arange(10, 15), z([-3, -1, -2, -8, -0.5]), np.zeros(5, np.int32))
    b.put(1, np.arange(10, 15))
    # slots 2 and 3, t = (0, 0, -0.0f): -0.0f and +0.0f around the index.  (n - 1) / 2 of [-1, -0, -0, +0, +0, 2] is index 2 (-0), of
    # [-1, -0, +0, +0, 2] index 2 (+0)
    b.set(np.arange(20, 26), z([0.0, -0.0, 2, -1, -0.0, 0.0]), np.zeros(6, np.int32))
    b.put(2, np.arange(20, 26), None, I, np.array([0, 0, -0.0], f32))
    b.put(3, [20, 21, 22, 23, 25], None, I, np.array([0, 0, -0.0], f32))
    for q in (1, 2, 7):
        d, n = b.median_depth([0, 1, 2, 3], q)
        out += [("depth q=%d" % q, d), ("n q=%d" % q, n)]
    # the double accumulation
    R, t, X = double_sum_case()
    b.set([30], X[None], [0])
    b.put(4, [30], None, R, t)
    out.append(("double sum", b.median_depth([4], 2)[0]))
    # the current values answer: a pose update and a moved point, both asynchronous, then the call with no wait of the caller's in between
    b.update_poses([0], rotation(9)[None], np.array([[0.1, 0.2, 0.3]], f32))
    b.set([2, 3], z([40, -40]))
    b.update_map_points([0], [0], [-1])
    d, n = b.median_depth([0, 4], 2)
    out += [("after update_poses, set and update_map_points", d), ("n after", n)]
    return out


BIG_N = [4095, 4096, 257]


def case_median_big(b):
    """the big store: rows of 4 096 features, 16 turns of the kernel's strided loops; many equal depths"""
    out = []
    rng = np.random.default_rng(41)
    pos = rng.normal(0, 4, (8192, 3)).astype(f32)
    pos[:, 2] = np.round(pos[:, 2] * 8) / 8             # many ties
    b.set(np.arange(8192), pos, np.zeros(8192, np.int32))
    for s, n in enumerate(BIG_N):
        row = np.full(4096, -1, np.int32)
        row[:n] = rng.choice(8192, n, replace=False)
        rng.shuffle(row)
        b.put(s, row, None, rotation(60 + s) if s else None, rng.normal(0, 1, 3).astype(f32))
    for q in (1, 2):
        d, n = b.median_depth([0, 1, 2], q)
        out += [("depth q=%d" % q, d), ("n q=%d" % q, n)]
    return out


CASES = dict(count=("std", case_count), culling=("std", case_culling), culling_apply=("long", case_culling_apply), tracked=("std", case_tracked),
             median_small=("std", case_median_small), median_edges=("std", case_median_edges), median_big=("big", case_median_big))
NAMES = list(CASES)
_expected = {}


def run(name, make):
    """the case on a fresh backend of its store: make(kind) -> backend"""
    kind, f = CASES[name]
    b = make(kind)
    try:
        return f(b)
    finally:
        if not hasattr(b, "reset"):
            b.close()


def expected(name):
    """what the restatement makes of the case"""
    if name not in _expected:
        _expected[name] = run(name, lambda kind: ref.Model(*STORES[kind]))
    return _expected[name]
