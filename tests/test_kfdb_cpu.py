"""KeyFrameDatabase without a GPU: the host build of csrc/cms_kfdb_core.h -- the definition of record of cms_kfdb_detect -- against
tests/npref_kfdb.py, a literal restatement of the reference's KeyFrameDatabase.cpp with a real inverted file.  Every comparison is exact: candidate
lists as lists (which pins the order rule -- smallest common word, then add order -- from outside), common-word counts as ints, scores as float32
bits.  The core's score is ORBVocabulary::score bit for bit, and a stand-alone program replays every case plain and under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_hostlib
import npref_kfdb as ref
import vocab_cases
import vocab_hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "kfdb_core_emu.cpp")
BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}


def host_run(name):
    db = kfdb_hostlib.HostDatabase(kc.K, kc.MAXF)

    class B:
        detect = staticmethod(db.detect)

        def __getattr__(self, op):
            def call(*a):
                assert getattr(db, op)(*a) == 0, (op, a[:1])
            return call
    out = kc.run(kc.case_ops(name), B())
    db.close()
    return out


@pytest.mark.parametrize("name", kc.NAMES)
def test_host_core_equals_restatement(name):
    want = kc.expected(name)
    assert len(want) > 0
    assert kc.first_difference(want, host_run(name)) is None, kc.first_difference(want, host_run(name))


def test_cases_are_not_vacuous():
    """the cases produce candidates, exclusions at the threshold and reorderings -- not empty answers all the way"""
    n_cand = sum(len(j[0]) for name in kc.NAMES for d in kc.expected(name) for j in d)
    assert n_cand > 200
    for M in (5, 6, 10, 15):
        minc = int(np.float32(M) * np.float32(0.8))
        cand, common, score = kc.expected("threshold_%d" % M)[0][0]
        assert list(common[:6]) == [M, M, minc, minc + 1, 1, minc]
        scored = score.view(np.float32)[:6] >= 0
        assert list(scored) == [True, True, False, True, False, False]      # exactly minCommonWords is excluded, one more is scored, the tie stays


def test_order_contract():
    d = kc.expected("order")
    # first common word 100: slots 7, 9, 4 in add order; then 101: 3, 12; then 102: 1
    assert d[0][0][0] == [7, 9, 4, 3, 12, 1] and d[0][1][0] == [7, 9, 4, 3, 12, 1]
    assert d[1][0][0] == [9, 4, 7, 3, 12, 1]      # erase + add moved 7 to the back of its word's list
    assert d[2][0][0] == [9, 4, 7, 12, 1]


def test_accumulation_case_proves_the_order():
    stored, asc, desc = kc.acc_sums()
    r = lambda x: np.float32(np.float32(0.75) * x)
    assert r(stored) != r(asc) and r(stored) != r(desc)      # the order of the ten float adds changes the cut
    reloc, loop, rules, rules_loop = kc.expected("accumulation")[0]
    for d in (reloc, loop):
        assert d[0][0] == 0                                  # entry 10's best is its covisible 0
        # a witness accumulates max(0.75f * S_stored, 0.75f * S_other): kept iff the stored order gives the smaller sum
        assert (len([c for c in d[0] if c in (30, 31)]) == 1) == bool(stored < asc)
        assert (len([c for c in d[0] if c in (32, 33)]) == 1) == bool(stored < desc)
    assert len(reloc[0]) in (2, 3)                           # (one of the two witnesses at least tells the orders apart by being there)
    # 20 stays its own best beside the equal 21; 24's best is the strictly greater 22; 23 names 22 again (kept once); 12 and 13 never count
    assert rules[0] == [20, 22] and rules_loop[0] == [20, 22]
    assert rules[1][12] == 0 and rules[1][13] == 0


def test_stale_reloc_score():
    one, two, readd = kc.expected("stale_one_call"), kc.expected("stale_two_calls"), kc.expected("stale_readd")
    assert one[0][1][0] == two[1][0][0] == [0]       # query B's candidate is X = slot 0, through the score query A left in it
    assert readd[1][0][0] == [1]                     # after erase + add the score is 0 again
    assert np.array_equal(one[0][1][2], two[1][0][2]) and one[0][1][2].view(np.float32)[0] == -1.0      # X was not scored by query B


def test_loop_cases():
    d = kc.expected("loop")[0]
    assert d[0][1][4] == 0 and d[1][1][4] == 20      # a connected slot is out of the list
    assert d[0][0] != d[1][0]
    assert 2 not in d[1][0]                          # below min_score: never a candidate of its own
    strict = kc.expected("loop_strict")[0]
    assert strict[0][0] == [] and strict[1][0] == [1] and strict[2][0] == [] and strict[3][0] == []
    assert strict[0][2].view(np.float32)[0] == 0.0 and strict[0][1][0] == 10


def test_core_score_is_the_mirrors_score():
    rng = np.random.default_rng(5)
    voc = vocab_hostlib.HostVocabulary(vocab_cases.case_tree("k10_L3"))
    pairs = [(kc.random_bow(rng, int(n1), 300), kc.random_bow(rng, int(n2), 300)) for n1, n2 in rng.integers(1, 200, (40, 2))]
    a = kc.random_bow(rng, 30, 300)
    pairs += [(a, a), (a, (a[0] + 1000, a[1])), (a, (np.zeros(0, np.int32), np.zeros(0))), ((a[0], -a[1]), a)]
    for v1, v2 in pairs:
        got, want = kfdb_hostlib.core_score(v1, v2), voc.score(v1, v2)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
        py = ref.score(list(zip(v1[0].tolist(), v1[1].tolist())), list(zip(v2[0].tolist(), v2[1].tolist())))
        assert np.float64(py).view(np.uint64) == np.float64(want).view(np.uint64)
    assert kfdb_hostlib.core_score(a, (a[0] + 1000, a[1])) == 0.0
    voc.close()


def test_host_refusals_change_nothing():
    db = kfdb_hostlib.HostDatabase(8, 16)
    ids, v = np.arange(4, dtype=np.int32), np.full(4, 0.25)
    assert db.add([0], [0]) == -1                                   # no BowVector
    assert db.set_bow(0, [3, 2, 5], [0.1, 0.2, 0.7]) == -1          # unsorted
    assert db.set_bow(0, [2, 2], [0.5, 0.5]) == -1                  # not strictly ascending
    assert db.set_bow(0, np.arange(17), np.ones(17)) == -1          # more than max_features
    assert db.add([0], [0]) == -1
    assert db.set_bow(0, ids, v) == 0 and db.set_bow(1, ids, v) == 0
    assert db.add([1, 0, 1], [0, 0, 0]) == -1 and db.add([0, 1], [0, 0]) == 0 and db.add([0], [0]) == -1
    assert db.set_bow(0, ids, v) == -1                              # in the database
    j = [kc.job(kc.RELOC, kc.words(ids, v))]
    assert db.detect(j)[0][0] == [0, 1]
    assert db.detect(j, cand_cap=1)[0][0] == [0] and db.last_rc == -4 and db.last_n_cand[0] == 2
    assert db.refill(0) == 0 and db.detect(j)[0][0] == [1]          # a refilled slot has left the database
    assert db.erase([5]) == 0 and db.detect(j)[0][0] == [1]
    db.close()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_core_emulation(build, tmp_path):
    exe = str(tmp_path / ("kfdb_core_emu_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + BUILDS[build] + [SRC, "-o", exe])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for name in kc.NAMES:
            f.write("case %s %d %d " % (name, kc.K, kc.MAXF) + kc.to_text(kc.case_ops(name), kc.expected(name)))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "kfdb_core_emu: ok (%d cases" % len(kc.NAMES) in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-4000:]
