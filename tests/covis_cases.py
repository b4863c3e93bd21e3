"""Named cases of the covisibility index, shared by tests/test_covis_cpu.py (host core against tests/npref_covis.py) and tests/test_gpu_covis.py
(device against host core).  A case is a table (per member: the slot it lives in, the mp row, the octaves) and a list of queries:

    ("votes", [ids of frame 0, ...])                                    -> votes[njobs, M]
    ("connections", [members], th)                                     -> (weights[njobs, M], order[njobs, M], n_connected[njobs])
    ("culling", [[members of chain 0], ...], [[erasable ...], ...], th_obs)   -> (n_mps, n_redundant, redundant) over all jobs
    ("local_points", [[members of frame 0], ...], cap)                 -> (rc, n_out, [ids written per job])

A backend offers load(case) -> the build's code, and one method per query.  expected(name) is the restatement's answer, with the one rule the
reference leaves to the allocator pinned the way csrc/cms_covis_core.h pins it: inside a run of equal weights the ordered list goes by member
position (the reference sorts pair<int, KeyFrame*>, so its ties go by DESCENDING pointer; pin_ties states the rule once)."""
import numpy as np

import npref_covis as ref

K = 64            # slots of the small store
MAXF = 256
MAX_ID = (1 << 30) - 1


def table(rows, octs=None, slots=None, maxf=MAXF, K_=K):
    rows = [np.asarray(r, np.int32) for r in rows]
    octs = [np.zeros(len(r), np.int32) for r in rows] if octs is None else [np.asarray(o, np.int32) for o in octs]
    slots = [(5 + 7 * m) % K_ for m in range(len(rows))] if slots is None else list(slots)      # slot != member position
    assert len(set(slots)) == len(slots) and all(len(r) <= maxf and len(r) == len(o) for r, o in zip(rows, octs))
    return dict(rows=rows, octs=octs, slots=slots, maxf=maxf, K=K_)


def random_table(seed, M, F, pool, n_none, maxf=MAXF, K_=K, max_octave=7):
    """M members x F features: F - n_none ids per row drawn without repetition from a sparse pool in [0, 2^30), the rest -1, shuffled"""
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(0, 1 << 30, 2 * pool))[:pool]
    rng.shuffle(ids)
    rows, octs = [], []
    for m in range(M):
        r = np.full(F, -1, np.int32)
        r[:F - n_none] = rng.choice(ids, F - n_none, replace=False)
        rng.shuffle(r)
        rows.append(r); octs.append(rng.integers(0, max_octave + 1, F).astype(np.int32))
    return table(rows, octs, maxf=maxf, K_=K_), ids


def _known3():
    t = table([[10, 11, 12, 13, -1], [11, 12, 13, 14], [13, 10, -1]])
    q = [("connections", [0, 1, 2], 2), ("connections", [0, 1, 2], 15), ("connections", [0], 3),
         ("votes", [[10, 13, 13, 99], [14], []]),
         ("culling", [[0, 1, 2]], [[1, 1, 1]], 3), ("culling", [[2]], [[1]], 1),
         ("local_points", [[0, 1, 2], [2, 1], [1]], 8), ("local_points", [[0, 1, 2]], 4)]
    return t, q


def _random():
    t, ids = random_table(11, 12, 200, 300, 30, max_octave=2)
    rng = np.random.default_rng(12)
    frames = [list(rng.choice(ids, 120)) for _ in range(5)]                       # (with repetition: an id listed twice counts twice)
    frames.append(list(rng.choice(ids, 40)) + [7, 1 << 29, MAX_ID] + list(ids[:3]) * 2)      # unknown ids add nothing
    chains = [list(rng.permutation(12)[:8]), list(rng.permutation(12)[:5]), [3]]
    er = [[int(x) for x in rng.integers(0, 2, len(c))] for c in chains]
    q = [("votes", frames), ("connections", list(range(12)), 15), ("connections", [4, 4, 0], 60), ("connections", [1, 7], 1),
         ("culling", chains, er, 3), ("culling", [list(range(12))], [[1] * 12], 3), ("culling", [list(range(11, -1, -1))], [[1] * 12], 2),
         ("culling", [[0, 5]], [[1, 1]], 0),
         ("local_points", [list(range(12)), [7, 2, 9], [], [5]], 1400), ("local_points", [[0, 1], [3]], 180)]
    return t, q


def _bits():
    """ids that differ only above bit 24, and only in bit 29: a table keyed by the low bits, or 24-bit packing, would merge them"""
    base = 0x00ABCDEF
    hi = [base | (k << 24) for k in range(64)]                 # bits 24..29
    pair = [0x12345, 0x12345 | (1 << 29)]
    rows = [hi[0:40] + [pair[0]], hi[20:60] + [pair[1]], hi[0:64:2] + pair, [pair[1], hi[63], -1, hi[1]]]
    t = table(rows)
    q = [("connections", [0, 1, 2, 3], 1), ("connections", [0, 1, 2, 3], 15), ("votes", [hi, pair, [pair[0]], [pair[1]], [base, base ^ 1, base ^ (1 << 23)]]),
         ("local_points", [[3, 2, 1, 0]], 128), ("culling", [[0, 1, 2, 3]], [[1, 1, 1, 1]], 1)]
    return t, q


def _edges():
    """an all-(-1) member, weight ties, nobody reaches th (with tied maxima), an empty KFcounter"""
    a = list(range(1000, 1030))
    rows = [a,                                            # 0: the member asked about
            [-1] * 20,                                    # 1: nothing at all
            a[0:16] + [5000],                             # 2: weight 16
            a[10:26],                                     # 3: weight 16 (tie with 2)
            a[0:20],                                      # 4: weight 20
            a[14:30] + [5001, 5002],                      # 5: weight 16 (tie with 2 and 3)
            [6000, 6001, 6002],                           # 6: shares with nobody: an empty KFcounter
            a[0:4], a[4:8] + [6003], a[26:30]]            # 7, 8, 9: weight 4 each
    t = table(rows)
    q = [("connections", list(range(10)), 15), ("connections", [0], 16), ("connections", [0], 17), ("connections", [0], 21), ("connections", [7, 8, 9, 1, 6], 15),
         ("connections", [0], 4), ("votes", [a, [], [6000, 6000, 6000], [1 << 20]]), ("culling", [[1, 6, 0]], [[1, 1, 1]], 3),
         ("local_points", [[1, 6, 2], [1]], 64)]
    return t, q


def _cull_strict():
    """exactly 3 against 4 observers: Observations(id) > thObs is strict; and exactly thObs other observers is enough"""
    p3 = list(range(100, 110))      # observed by members 0, 1, 2: Observations = 3, not > 3
    p4 = list(range(200, 210))      # observed by 0, 1, 2, 3: 4 > 3, and 3 others
    rows = [p3 + p4, p3 + p4, p3 + p4, p4 + [300], p4[:5]]
    t = table(rows)
    q = [("culling", [[0], [3], [4]], [[0], [0], [0]], 3), ("culling", [[0, 1, 2, 3, 4]], [[0] * 5], 3), ("culling", [[0, 1, 2, 3, 4]], [[1] * 5], 3),
         ("culling", [[0]], [[0]], 2), ("culling", [[0]], [[0]], 4)]
    return t, q


def _cull_octave():
    """the gate scaleLeveli <= scaleLevel + 1: observers at +1 count, at +2 they do not"""
    p = list(range(500, 520))
    rows = [p, p, p, p, p]
    octs = [[2] * 20, [3] * 20, [3] * 10 + [4] * 10, [0] * 20, [4] * 5 + [1] * 15]
    t = table(rows, octs)
    q = [("culling", [[0], [1], [2], [3], [4]], [[0]] * 5, 3), ("culling", [[0, 1, 2, 3, 4]], [[1] * 5], 3), ("culling", [[3, 0]], [[1, 1]], 3)]
    return t, q


def _cascade():
    """removing job 0 drives ids to 2 observations: they become bad, vanish from every member, and change job 1's n_mps and verdict"""
    a = list(range(1000, 1040))      # members 0, 1, 2, 3
    qq = [2000, 2001, 2002]          # members 0, 1, 4: 3 observations; 2 once member 0 is gone
    r = list(range(3000, 3020))      # members 1, 2, 3, 4
    rows = [a + qq, a + qq + r, a + r, a + r, qq + r + [4000]]
    t = table(rows)
    q = [("culling", [[0, 1, 4]], [[1, 1, 1]], 3), ("culling", [[0, 1, 4]], [[0, 1, 1]], 3), ("culling", [[0, 1, 4], [0, 1, 4], [1, 0]], [[1, 1, 1], [0, 0, 0], [1, 1]], 3),
         ("connections", [0, 1, 4], 15)]
    return t, q


def _large():
    """40 members x 2048 features: more than 65 536 observations, several workgroups per kernel"""
    t, ids = random_table(21, 40, 2048, 6000, 48, maxf=2048, K_=48)
    t["slots"] = [(3 + 11 * m) % 48 for m in range(40)]
    rng = np.random.default_rng(22)
    q = [("votes", [list(rng.choice(ids, 900)), list(rng.choice(ids, 300)) + [5, 6]]), ("connections", [0, 17, 39], 15), ("connections", [5], 700),
         ("culling", [[4, 9, 30, 2, 21], [9, 4]], [[1, 0, 1, 1, 1], [1, 1]], 3), ("local_points", [[3, 38, 12], [0]], 6000), ("local_points", [[1, 2]], 2100)]
    return t, q


def _wide():
    """8 400 members x 8 features: more members than a workgroup has threads (the strides over members), more than 8 192 of them (the counters and the
    candidate list of `connections` need more than 64 KB of LDS) and more than 1 024 candidates to rank.  Two hub points are seen by 3 000 and 4 500 key
    frames; the rest are tracked over four consecutive key frames."""
    M = 8400
    rng = np.random.default_rng(41)
    p = np.unique(rng.integers(0, 1 << 30, 2 * M))[:M + 8]
    rng.shuffle(p)
    hub_a, hub_b = int(p[M + 4]), int(p[M + 5])
    rows = []
    for m in range(M):
        r = [int(p[k]) for k in range(max(m - 3, 0), m + 1)]      # point k is seen by members k .. k + 3
        if m < 3000:
            r.append(hub_a)
        if 1500 <= m < 6000:
            r.append(hub_b)
        r += [-1] * (8 - len(r))
        rows.append([r[i] for i in rng.permutation(8)])
    octs = [rng.integers(0, 3, 8) for _ in range(M)]
    t = table(rows, octs, slots=[(3 + 11 * m) % M for m in range(M)], maxf=8, K_=M)
    far = [int(p[k]) for k in range(0, M, 7)]
    q = [("votes", [[hub_a, hub_b, hub_a], far, [int(p[M - 1]), int(p[M + 6])]]),
         ("connections", [0, 2000, 8399, 7000], 1), ("connections", [2000, 2999], 2), ("connections", [2000, 7000], 15),
         ("culling", [[2000, 2001, 10, 8000, 5000, 2002], [2002, 5000, 8000, 10, 2001, 2000]], [[1] * 6, [1, 0, 1, 1, 1, 1]], 3),
         ("local_points", [list(range(0, M, 3)), [8399, 0]], 20000), ("local_points", [list(range(5000, 7000))], 1500)]
    return t, q


_BUILDERS = {"wide8400x8": _wide, "known3": _known3, "random12x200": _random, "high_bits": _bits, "edges": _edges, "cull_strict": _cull_strict, "cull_octave": _cull_octave,
             "cascade": _cascade, "large40x2048": _large}
SMALL = ["known3", "random12x200", "high_bits", "edges", "cull_strict", "cull_octave", "cascade"]
NAMES = SMALL + ["large40x2048", "wide8400x8"]
_cases, _expected = {}, {}


def case(name):
    if name not in _cases:
        t, q = _BUILDERS[name]()
        _cases[name] = dict(t, queries=q, name=name)
    return _cases[name]


def pin_ties(order_members, weights):
    """the ordered list with every run of equal weights sorted by member position"""
    return sorted(order_members, key=lambda m: (-weights[m], m))


def reference_query(c, q, addresses=None, pin=True):
    """one query through the restatement, on a fresh map"""
    M = len(c["rows"])
    kfs, points = ref.make_map(c["rows"], c["octs"], addresses)
    pos = {kf: m for m, kf in enumerate(kfs)}
    if q[0] == "votes":
        out = np.zeros((len(q[1]), M), np.int32)
        for j, ids in enumerate(q[1]):
            counter, _ = ref.update_local_keyframes_votes([points[int(i)] for i in ids if int(i) in points])
            for kf, n in counter.items():
                out[j, pos[kf]] = n
        return out
    if q[0] == "connections":
        nj = len(q[1])
        w = np.zeros((nj, M), np.int32); order = np.full((nj, M), -1, np.int32); nc = np.zeros(nj, np.int32)
        for j, m in enumerate(q[1]):
            counter, lKFs, lWs = ref.update_connections(kfs[m], q[2])
            for kf, n in counter.items():
                w[j, pos[kf]] = n
            o = [pos[kf] for kf in lKFs]
            assert lWs == [int(w[j, x]) for x in o]
            o = pin_ties(o, w[j]) if pin else o
            order[j, :len(o)] = o; nc[j] = len(o)
        return w, order, nc
    if q[0] == "culling":
        nm, nr, red = [], [], []
        for chain, er in zip(q[1], q[2]):
            kfs, points = ref.make_map(c["rows"], c["octs"], addresses)      # chains are independent
            for m, e in zip(chain, er):
                kfs[m].mbNotErase = not e
            for a, b, r in ref.keyframe_culling([kfs[m] for m in chain], q[3]):
                nm.append(a); nr.append(b); red.append(int(r))
        return np.array(nm, np.int32), np.array(nr, np.int32), np.array(red, np.uint8)
    if q[0] == "local_points":
        n_out, lists = [], []
        for j, members in enumerate(q[1]):
            ids = ref.update_local_points([kfs[m] for m in members], frame_id=j + 1)
            n_out.append(len(ids)); lists.append(ids[:q[2]])
        return (-4 if any(n > q[2] for n in n_out) else 0), np.array(n_out, np.int32), lists
    raise ValueError(q[0])


def expected(name):
    if name not in _expected:
        c = case(name)
        _expected[name] = [reference_query(c, q) for q in c["queries"]]
    return _expected[name]


def run(c, backend):
    assert backend.load(c) == 0
    out = []
    for q in c["queries"]:
        out.append(getattr(backend, q[0])(*q[1:]))
    return out


def _flat(r):
    if isinstance(r, tuple):
        return [x for part in r for x in _flat(part)]
    if isinstance(r, list):
        return [("list", [[int(v) for v in x] for x in r])] if r and isinstance(r[0], (list, np.ndarray)) else [("list", [int(v) for v in r])]
    if isinstance(r, np.ndarray):
        return [("array", r.shape, [int(v) for v in r.reshape(-1)])]
    return [("int", int(r))]


def first_difference(want, got):
    if len(want) != len(got):
        return "number of queries: %d against %d" % (len(want), len(got))
    for i, (a, b) in enumerate(zip(want, got)):
        fa, fb = _flat(a), _flat(b)
        if fa != fb:
            for k, (x, y) in enumerate(zip(fa, fb)):
                if x != y:
                    return "query %d, part %d: want %s, got %s" % (i, k, str(x)[:300], str(y)[:300])
            return "query %d: %d parts against %d" % (i, len(fa), len(fb))
    return None


def offsets(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.array([int(v) for x in lists for v in x], np.int32) if int(off[-1]) else np.zeros(1, np.int32)
    return off, flat


def to_text(c, results):
    """the case and its expected results as the token stream tests/emu/covis_core_emu.cpp replays: ints only"""
    M = len(c["rows"])
    t = ["case", c["K"], c["maxf"], M]
    for s, r, o in zip(c["slots"], c["rows"], c["octs"]):
        t += [s, len(r)] + [int(v) for v in r] + [int(v) for v in o]
    t.append(len(c["queries"]))
    for q, r in zip(c["queries"], results):
        if q[0] == "votes":
            off, flat = offsets(q[1])
            t += [1, len(q[1])] + off.tolist() + flat[:off[-1]].tolist() + r.reshape(-1).tolist()
        elif q[0] == "connections":
            t += [2, len(q[1]), q[2]] + list(q[1]) + r[0].reshape(-1).tolist() + r[1].reshape(-1).tolist() + r[2].tolist()
        elif q[0] == "culling":
            off, flat = offsets(q[1])
            er = [int(v) for x in q[2] for v in x]
            t += [3, len(q[1]), q[3]] + off.tolist() + flat[:off[-1]].tolist() + er + r[0].tolist() + r[1].tolist() + r[2].tolist()
        else:
            off, flat = offsets(q[1])
            t += [4, len(q[1]), q[2]] + off.tolist() + flat[:off[-1]].tolist() + [r[0]] + r[1].tolist()
            for ids in r[2]:
                t += [int(v) for v in ids]
    return " ".join(str(int(v)) if not isinstance(v, str) else v for v in t) + "\n"
