"""Seeded cases for the key-frame database (csrc/cms_kfdb_core.h, cms_kfdb_detect): each is a script of operations on a store of K slots, replayed by
run() on a backend -- the numpy restatement (npref_kfdb.World), the host core (kfdb_hostlib.HostDatabase), the device (test_gpu_kfdb.py) or, as a
text file, the stand-alone program tests/emu/kfdb_core_emu.cpp.  The shapes are the smallest at which each mechanism can break.

An operation is a tuple: ("set_bow", slot, ids, vals), ("refill", slot), ("covis", slot, [10 slots]), ("add", slots, groups), ("erase", slots),
("clear", group), ("detect", [job, ...]).  A job is dict(mode, group, query=("words", ids, vals) | ("slot", s), min_score, connected).  run()
returns, per detect operation, a list with one (candidate slots, common words int32[K], score bits uint32[K]) per job."""
import numpy as np

import npref_kfdb as ref

K, MAXF = 160, 256
RELOC, LOOP = ref.RELOC, ref.LOOP
LENGTHS = (1, 63, 64, 65, 200)


def job(mode, query, group=0, min_score=0.0, connected=()):
    return dict(mode=mode, group=group, query=query, min_score=float(np.float32(min_score)), connected=[int(c) for c in connected])


def words(ids, vals):
    return ("words", np.asarray(ids, np.int32), np.asarray(vals, np.float64))


def random_bow(rng, n, vocab):
    ids = np.sort(rng.choice(vocab, size=n, replace=False)).astype(np.int32)
    v = rng.random(n) + 0.05
    return ids, v / v.sum()


def shared_bow(common_ids, private_ids, a=None, rng=None):
    """A BowVector with the given common and private words; a: the share of the L1 mass on the common words (uniform there), else random values"""
    ids = np.array(sorted(list(common_ids) + list(private_ids)), np.int32)
    if a is None:
        v = rng.random(len(ids)) + 0.05
        return ids, v / v.sum()
    is_c = np.isin(ids, np.asarray(list(common_ids), np.int32))
    v = np.where(is_c, a / max(len(common_ids), 1), (1.0 - a) / max(len(private_ids), 1))
    return ids, v.astype(np.float64)


def pad10(n):
    n = list(n)
    return n + [-1] * (10 - len(n))


# ---- degenerate
def case_empty_db():
    rng = np.random.default_rng(1)
    ops = [("set_bow", s, *random_bow(rng, 20, 60)) for s in range(3)]
    ops += [("detect", [job(RELOC, words(*random_bow(rng, 20, 60))), job(LOOP, ("slot", 1), min_score=0.01)])]
    return ops


def case_query_0_words():
    rng = np.random.default_rng(2)
    ops = [("set_bow", s, *random_bow(rng, 20, 60)) for s in range(4)] + [("add", [0, 1, 2, 3], [0] * 4)]
    ops += [("detect", [job(RELOC, words([], [])), job(LOOP, words([], []), min_score=0.0)])]
    return ops


def case_no_shared_word():
    rng = np.random.default_rng(3)
    ops = [("set_bow", s, *random_bow(rng, 20, 60)) for s in range(4)] + [("add", [0, 1, 2, 3], [0] * 4)]
    ids, v = random_bow(rng, 20, 60)
    ops += [("detect", [job(RELOC, words(ids + 1000, v)), job(LOOP, words(ids + 1000, v), min_score=0.0)])]
    return ops


def case_one_entry():
    rng = np.random.default_rng(4)
    ops = [("set_bow", 5, *random_bow(rng, 30, 60)), ("add", [5], [0]), ("covis", 5, pad10([5, 6]))]
    ops += [("detect", [job(RELOC, words(*random_bow(rng, 30, 60))), job(LOOP, words(*random_bow(rng, 30, 60)), min_score=0.0)])]
    return ops


def case_own_only_sharer():
    rng = np.random.default_rng(5)
    ops = []
    for s in range(4):
        ids, v = random_bow(rng, 20, 60)
        ops.append(("set_bow", s, ids + 100 * s, v))
    ops += [("add", [0, 1, 2, 3], [0] * 4), ("detect", [job(LOOP, ("slot", 2), min_score=0.5), job(RELOC, ("slot", 2))])]
    return ops


# ---- lane striding: list lengths 1, 63, 64, 65, 200 on both sides; 1, 2, 65 and 130 entries
def case_stride(E):
    rng = np.random.default_rng(10 + E)
    ops = []
    slots = list(rng.permutation(K)[:E])
    rounds = len(LENGTHS) if E < len(LENGTHS) else 1
    for r in range(rounds):
        if r:
            ops.append(("erase", slots))
        for i, s in enumerate(slots):
            ops.append(("set_bow", int(s), *random_bow(rng, LENGTHS[(i + r) % len(LENGTHS)], 400)))
        ops.append(("add", [int(s) for s in slots], [0] * E))
        for i, s in enumerate(slots):
            ops.append(("covis", int(s), pad10(int(slots[(i + d) % E]) for d in range(1, min(E, 8)))))
        jobs = [job(RELOC if i % 2 == 0 else LOOP, words(*random_bow(rng, n, 400)), min_score=0.02, connected=[int(slots[0])] if i == 3 else []) for i, n in enumerate(LENGTHS)]
        ops.append(("detect", jobs))
    return ops


# ---- the threshold: maxCommonWords M, entries at M (a tie), at minCommonWords (excluded), at minCommonWords + 1, at 1
def case_threshold(M):
    rng = np.random.default_rng(20 + M)
    minc = int(np.float32(M) * np.float32(0.8))
    q_ids = np.arange(100, 100 + 20)
    counts = [M, M, minc, minc + 1, 1, minc]
    ops = []
    for s, c in enumerate(counts):
        ops.append(("set_bow", s, *shared_bow(q_ids[rng.permutation(20)[:c]], 1000 + 50 * s + np.arange(6), rng=rng)))
    ops.append(("add", list(range(len(counts))), [0] * len(counts)))
    for s in range(len(counts)):
        ops.append(("covis", s, pad10((s + d) % len(counts) for d in (1, 2, 3))))
    v = rng.random(20) + 0.05
    ops.append(("detect", [job(RELOC, words(q_ids, v / v.sum())), job(LOOP, words(q_ids, v / v.sum()), min_score=0.05)]))
    return ops


# ---- the order of lKFsSharingWords: smallest common word, then add order
def case_order():
    q_ids = np.arange(100, 110)
    ops = []
    # every entry has 9 of the query's 10 words with the same values: equal-sized scores, so every entry is retained and the candidates ARE the list
    first = {7: 100, 3: 101, 9: 100, 1: 102, 12: 101, 4: 100}      # slot -> smallest common word
    for s, f in first.items():
        c = list(q_ids[q_ids >= f])[:9]
        ops.append(("set_bow", s, *shared_bow(c, [2000 + s], a=0.9)))
    ops.append(("add", [7, 3, 9, 1, 12, 4], [0] * 6))      # not in slot order
    q = words(q_ids, np.full(10, 0.1))
    ops.append(("detect", [job(RELOC, q), job(LOOP, q, min_score=0.1)]))
    ops += [("erase", [7]), ("add", [7], [0])]             # 7 moves behind 9 and 4 among the entries whose first common word is 100
    ops.append(("detect", [job(RELOC, q), job(LOOP, q, min_score=0.1)]))
    ops += [("erase", [3, 100]), ("detect", [job(RELOC, q)])]      # (100 is not in the database: erase leaves it alone)
    return ops


# ---- accumulation over the covisibles
ACC_A = [0.7, 0.0018133, 0.31, 0.0005738, 0.05, 0.6, 0.0011246, 0.11, 0.003459, 0.43, 0.2]      # the share of mass on the common words ~ the entry's score


def acc_scores():
    q = list(zip(range(100, 120), [0.05] * 20))
    out = []
    for a in ACC_A:
        ids, v = shared_bow(range(100, 120), [3000], a=a)
        out.append(np.float32(ref.score(q, list(zip(ids.tolist(), v.tolist())))))
    return out


def _sum32(start, values):
    x = np.float32(start)
    for v in values:
        x = np.float32(x + v)
    return x


def acc_sums():
    """entry 10's accumulated score over its ten covisibles 0..9 in stored, ascending and descending order"""
    s = acc_scores()
    return _sum32(s[10], s[:10]), _sum32(s[10], sorted(s[:10])), _sum32(s[10], sorted(s[:10], reverse=True))


def case_accumulation():
    """Group 0 proves the order of the float sum: entry 10 (ten covisibles, 1e-3 next to 0.7) has the best accumulated score S, and the two witnesses
    30 and 32 accumulate exactly max(0.75f * S_stored, 0.75f * S_sorted) for the ascending and the descending order: each is retained under one order
    of summation and cut under the other.  Group 2 holds the take-over rules."""
    q_ids = np.arange(100, 120)
    ops = []
    for s, a in enumerate(ACC_A):
        ops.append(("set_bow", s, *shared_bow(q_ids, [3000 + s], a=a)))
    stored, asc, desc = acc_sums()
    group0 = list(range(11))
    for w, other in ((30, asc), (32, desc)):
        target = max(np.float32(np.float32(0.75) * stored), np.float32(np.float32(0.75) * other))
        own = np.float32(ref.score(list(zip(q_ids.tolist(), [0.05] * 20)), list(zip(*[x.tolist() for x in shared_bow(q_ids, [3000 + w], a=0.9)]))))
        ops.append(("set_bow", w, *shared_bow(q_ids, [3000 + w], a=0.9)))
        ops.append(("set_bow", w + 1, *shared_bow(q_ids, [3001 + w], a=float(np.float32(target - own)))))      # (exact: Sterbenz)
        ops.append(("covis", w, pad10([w + 1])))
        group0 += [w, w + 1]
    ops.append(("covis", 10, pad10(range(10))))             # ten covisibles in an order that is not sorted
    # group 2: 21 has 20's vector (an equal score must NOT take over), 22 is strictly greater than 24 and 23 (takes over, named twice: kept once),
    # 12 lives in group 1 and 13 is never added (both would be the best of 23 if they counted)
    for s, a in ((20, 0.5), (21, 0.5), (22, 0.6), (24, 0.45), (23, 0.44), (12, 0.99), (13, 0.98)):
        ops.append(("set_bow", s, *shared_bow(q_ids, [3020 if s == 21 else 3000 + s], a=a)))
    ops.append(("add", group0 + [20, 21, 22, 24, 23, 12], [0] * len(group0) + [2] * 5 + [1]))
    ops += [("covis", 20, pad10([21])), ("covis", 24, pad10([22])), ("covis", 23, pad10([12, 13, 22]))]
    q = words(q_ids, np.full(20, 0.05))
    ops.append(("detect", [job(RELOC, q), job(LOOP, q, min_score=1e-4), job(RELOC, q, group=2), job(LOOP, q, group=2, min_score=0.1)]))
    return ops


# ---- the reloc_score an earlier query left
def case_stale(variant):
    """X = 0 is scored by query A (0.9) and falls under the threshold of query B while it shares a word with it and is a covisible of Y = 1."""
    qa = np.arange(100, 110)
    qb = np.arange(200, 210)
    ops = [("set_bow", 0, *shared_bow(list(qa) + [200], [4000], a=0.9)),        # 10 common with A, 1 with B
           ("set_bow", 1, *shared_bow(qb, [4001], a=0.4)),
           ("set_bow", 2, *shared_bow(qb, [4002], a=0.2)),
           ("add", [0, 1, 2], [0, 0, 0]), ("covis", 1, pad10([0])), ("covis", 2, pad10([1]))]
    ja = job(RELOC, words(qa, np.full(10, 0.1)))
    jb = job(RELOC, words(qb, np.full(10, 0.1)))
    if variant == "one_call":
        ops.append(("detect", [ja, jb]))
    elif variant == "two_calls":
        ops += [("detect", [ja]), ("detect", [jb])]
    else:      # "readd": erase + add between the calls, the score is 0 again
        ops += [("detect", [ja]), ("erase", [0]), ("add", [0], [0]), ("detect", [jb])]
    return ops


# ---- groups
def case_groups():
    rng = np.random.default_rng(40)
    ops = []
    for s in range(6):
        ids, v = random_bow(rng, 40, 90)
        ops += [("set_bow", s, ids, v), ("set_bow", 20 + s, ids, v)]
    ops.append(("add", [0, 20, 1, 21, 2, 22, 3, 23, 4, 24, 5, 25], [0, 1] * 6))
    for s in range(6):
        ops += [("covis", s, pad10([20 + (s + 1) % 6, (s + 2) % 6])), ("covis", 20 + s, pad10([(s + 1) % 6, 20 + (s + 2) % 6]))]
    q = words(*random_bow(rng, 40, 90))
    d = ("detect", [job(RELOC, q, group=0), job(RELOC, q, group=1), job(LOOP, q, group=1, min_score=0.01), job(RELOC, q, group=2)])
    ops += [d, ("clear", 1), d, ("clear", -1), d]
    return ops


# ---- loop mode
def case_loop():
    q_ids = np.arange(100, 120)
    a = {0: 0.5, 1: 0.6, 2: 0.02, 3: 0.3, 4: 0.8, 5: 0.45}
    ops = [("set_bow", 9, q_ids, np.full(20, 0.05))]
    for s, x in a.items():
        ops.append(("set_bow", s, *shared_bow(q_ids, [5000 + s], a=x)))
    ops.append(("add", [0, 1, 2, 3, 4, 5, 9], [0] * 7))        # the query slot 9 itself is in the database
    ops += [("covis", 0, pad10([4, 2])),        # 4 is connected: out of the sum; 2 is below min_score but adds
            ("covis", 3, pad10([2, 1])), ("covis", 5, pad10([9]))]
    ops.append(("detect", [job(LOOP, ("slot", 9), min_score=0.25, connected=[4, 77]),
                           job(LOOP, ("slot", 9), min_score=0.25),
                           job(LOOP, ("slot", 9), min_score=0.25, connected=[9, 4])]))
    return ops


def case_loop_strict():
    """min_score 0 and an entry whose common words weigh 0: si = 0 >= 0 enters lScoreAndMatch, but its sum 0 is not > 0.75f * 0 (the strict >);
    the same entry with a little weight on them (group 1) is retained"""
    q_ids = np.arange(100, 110)
    ids = np.array(list(q_ids) + [6000], np.int32)
    ops = [("set_bow", 0, ids, np.array([0.0] * 10 + [1.0])), ("set_bow", 1, ids, np.array([1e-3] * 10 + [0.99])), ("add", [0, 1], [0, 1])]
    q = words(q_ids, np.full(10, 0.1))
    ops.append(("detect", [job(LOOP, q, min_score=0.0), job(LOOP, q, group=1, min_score=0.0), job(LOOP, q, min_score=0.5), job(RELOC, q)]))
    return ops


# ---- seeded random worlds: 1, 3 and 9 jobs per call, mixing modes and query forms
def case_random(seed, njobs):
    rng = np.random.default_rng(seed)
    E = int(rng.integers(20, 90))
    slots = [int(s) for s in rng.permutation(K)[:E]]
    ops = []
    for s in slots:
        ops.append(("set_bow", s, *random_bow(rng, int(rng.integers(5, 120)), 300)))
    ops.append(("add", slots, [int(g) for g in rng.integers(0, 2, E)]))
    for s in slots:
        ops.append(("covis", s, pad10(int(x) for x in rng.choice(slots, size=int(rng.integers(0, 11)), replace=False))))
    for _ in range(3):
        jobs = []
        for _j in range(njobs):
            mode = int(rng.integers(0, 2))
            q = ("slot", int(rng.choice(slots))) if rng.random() < 0.4 else words(*random_bow(rng, int(rng.integers(5, 150)), 300))
            jobs.append(job(mode, q, group=int(rng.integers(0, 2)), min_score=float(rng.random() * 0.1),
                            connected=[int(x) for x in rng.choice(slots, size=int(rng.integers(0, 6)), replace=False)]))
        ops.append(("detect", jobs))
        moved = [int(x) for x in rng.choice(slots, size=5, replace=False)]
        ops += [("erase", moved), ("add", moved[::-1], [int(g) for g in rng.integers(0, 2, 5)])]
    return ops


CASES = {
    "empty_db": case_empty_db, "query_0_words": case_query_0_words, "no_shared_word": case_no_shared_word, "one_entry": case_one_entry,
    "own_only_sharer": case_own_only_sharer,
    "stride_1": lambda: case_stride(1), "stride_2": lambda: case_stride(2), "stride_65": lambda: case_stride(65), "stride_130": lambda: case_stride(130),
    "threshold_5": lambda: case_threshold(5), "threshold_6": lambda: case_threshold(6), "threshold_10": lambda: case_threshold(10),
    "threshold_15": lambda: case_threshold(15),
    "order": case_order, "accumulation": case_accumulation,
    "stale_one_call": lambda: case_stale("one_call"), "stale_two_calls": lambda: case_stale("two_calls"), "stale_readd": lambda: case_stale("readd"),
    "groups": case_groups, "loop": case_loop, "loop_strict": case_loop_strict,
    "random_1": lambda: case_random(71, 1), "random_3": lambda: case_random(73, 3), "random_9": lambda: case_random(79, 9),
}
NAMES = sorted(CASES)


def case_ops(name):
    return CASES[name]()


def run(ops, backend):
    """Replay on a backend with set_bow / refill / covis / add / erase / clear / detect(jobs); the detect results in order"""
    out = []
    for op in ops:
        if op[0] == "detect":
            out.append(backend.detect(op[1]))
        else:
            getattr(backend, op[0])(*op[1:])
    return out


class NumpyBackend:
    def __init__(self):
        self.w = ref.World(K)

    def set_bow(self, slot, ids, vals): self.w.set_bow(slot, ids, vals)
    def refill(self, slot): self.w.refill(slot)
    def covis(self, slot, neigh): self.w.covisibles(slot, neigh)
    def add(self, slots, groups): self.w.add(slots, groups)
    def erase(self, slots): self.w.erase(slots)
    def clear(self, group): self.w.clear(group)
    def detect(self, jobs): return [self.w.detect(j) for j in jobs]


_expected = {}


def expected(name):
    """The numpy restatement's results of a case, computed once"""
    if name not in _expected:
        _expected[name] = run(case_ops(name), NumpyBackend())
    return _expected[name]


def first_difference(want, got):
    """None, or where two run() results differ"""
    if len(want) != len(got):
        return "detect calls: %d != %d" % (len(want), len(got))
    for d, (wd, gd) in enumerate(zip(want, got)):
        if len(wd) != len(gd):
            return "detect %d: jobs %d != %d" % (d, len(wd), len(gd))
        for j, (w, g) in enumerate(zip(wd, gd)):
            if list(w[0]) != list(g[0]):
                return "detect %d job %d: candidates %s != %s" % (d, j, list(w[0]), list(g[0]))
            for k, what in ((1, "common words"), (2, "score bits")):
                if not np.array_equal(w[k], g[k]):
                    s = int(np.flatnonzero(np.asarray(w[k]) != np.asarray(g[k]))[0])
                    return "detect %d job %d: %s of slot %d: %s != %s" % (d, j, what, s, w[k][s], g[k][s])
    return None


def to_text(ops, results):
    """The case and its expected results as the token stream tests/emu/kfdb_core_emu.cpp replays: doubles and floats as their bit patterns"""
    t = []
    bits64 = lambda v: ["%d" % x for x in np.asarray(v, np.float64).view(np.uint64)]
    d = 0
    for op in ops:
        if op[0] == "set_bow":
            t += ["set_bow", str(op[1]), str(len(op[2]))] + [str(int(i)) for i in op[2]] + bits64(op[3])
        elif op[0] in ("refill", "clear"):
            t += [op[0], str(op[1])]
        elif op[0] == "covis":
            t += ["covis", str(op[1])] + [str(int(n)) for n in op[2]]
        elif op[0] == "add":
            t += ["add", str(len(op[1]))] + [str(int(s)) for s in op[1]] + [str(int(g)) for g in op[2]]
        elif op[0] == "erase":
            t += ["erase", str(len(op[1]))] + [str(int(s)) for s in op[1]]
        else:
            t += ["detect", str(len(op[1]))]
            for j, res in zip(op[1], results[d]):
                q = j["query"]
                t += ["job", str(j["mode"]), str(j["group"]), str(int(np.float32(j["min_score"]).view(np.uint32))), str(len(j["connected"]))] + [str(c) for c in j["connected"]]
                if q[0] == "slot":
                    t += ["slot", str(q[1])]
                else:
                    t += ["words", str(len(q[1]))] + [str(int(i)) for i in q[1]] + bits64(q[2])
                t += ["expect", str(len(res[0]))] + [str(int(c)) for c in res[0]] + [str(int(c)) for c in res[1]] + [str(int(b)) for b in res[2]]
            d += 1
    t.append("end")
    return " ".join(t) + "\n"
