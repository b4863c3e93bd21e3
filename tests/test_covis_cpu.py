"""Covisibility without a GPU: the host build of csrc/cms_covis_core.h -- the definition of record of cms_covis_* -- against tests/npref_covis.py, a
literal restatement of KeyFrame::UpdateConnections, LocalMapping::KeyFrameCulling (with the SetBadFlag cascade), the votes of
Tracking::UpdateLocalKeyFrames and Tracking::UpdateLocalPoints on Python objects.  Every comparison is exact: counts, lists and flags.  A stand-alone
program replays every case plain and under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import covis_cases as cc
import covis_hostlib as hl
import npref_covis as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "covis_core_emu.cpp")
BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}


def host_run(name):
    c = cc.case(name)
    b = hl.HostBackend(c["K"], c["maxf"])
    out = cc.run(c, b)
    b.close()
    return out


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_core_equals_restatement(name):
    want = cc.expected(name)
    assert len(want) > 0
    assert cc.first_difference(want, host_run(name)) is None, cc.first_difference(want, host_run(name))


def test_known_answer():
    """three key frames by hand: 0 = {10, 11, 12, 13}, 1 = {11, 12, 13, 14}, 2 = {13, 10}"""
    conn2, conn15, conn3, votes, cull, cull1, lp, lp4 = cc.expected("known3")
    assert conn2[0].tolist() == [[0, 3, 2], [3, 0, 1], [2, 1, 0]]
    assert conn2[1].tolist() == [[1, 2, -1], [0, -1, -1], [0, -1, -1]] and conn2[2].tolist() == [2, 1, 1]
    assert conn15[1].tolist() == [[1, -1, -1], [0, -1, -1], [0, -1, -1]] and conn15[2].tolist() == [1, 1, 1]      # nobody reaches 15: the maximum alone
    assert conn3[1].tolist() == [[1, -1, -1]]
    assert votes.tolist() == [[3, 2, 3], [0, 1, 0], [0, 0, 0]]                                              # 13 listed twice counts twice, 99 is unknown
    assert cull[0].tolist() == [4, 4, 2] and cull[1].tolist() == [0, 0, 0] and cull[2].tolist() == [0, 0, 0]   # no id has more than 3 observations
    assert cull1[0].tolist() == [2] and cull1[1].tolist() == [2] and cull1[2].tolist() == [1]
    assert lp[2] == [[10, 11, 12, 13, 14], [13, 10, 11, 12, 14], [11, 12, 13, 14]] and lp[0] == 0
    assert lp4[0] == -4 and lp4[1].tolist() == [5] and lp4[2] == [[10, 11, 12, 13]]


def test_cases_are_not_vacuous():
    e = cc.expected("edges")
    w, order, nc = e[0]
    assert w[0].tolist() == [0, 0, 16, 16, 20, 16, 0, 4, 4, 4]
    assert order[0, :4].tolist() == [4, 2, 3, 5] and nc[0] == 4                   # the tie 16 = 16 = 16 goes by member position
    assert nc[1] == 0 and nc[6] == 0                                              # the all-(-1) member and the one that shares nothing: an empty KFcounter
    assert e[3][1][0, :2].tolist() == [4, -1] and e[3][2].tolist() == [1]         # th = 21: nobody reaches it, the maximum alone
    assert e[4][1][:3, 0].tolist() == [0, 0, 0]
    strict = cc.expected("cull_strict")
    assert strict[0][0].tolist() == [20, 11, 5] and strict[0][1].tolist() == [10, 10, 5]      # p3 has exactly 3 observers: not > 3; p4 has 4 and 3 others
    assert strict[3][1].tolist() == [20] and strict[4][1].tolist() == [5]      # thObs = 4: only the five ids that member 4 sees too have 5 observers
    octave = cc.expected("cull_octave")
    # member 3 (octave 0) has a single observer within + 1 (member 4's octave-1 features); member 4's octave-1 features have two (octaves 2 and 0)
    assert octave[0][1].tolist() == [20, 20, 20, 0, 5]
    casc = cc.expected("cascade")
    erased, kept = casc[0], casc[1]
    assert erased[2].tolist() == [1, 0, 1] and kept[2].tolist() == [1, 1, 0]      # job 0 gone: job 1 is no longer redundant, and job 2 becomes so
    assert erased[0].tolist() == [43, 60, 21] and erased[1].tolist() == [40, 20, 20]      # ... three points of jobs 1 and 2 have become bad
    assert kept[0].tolist() == [43, 63, 21] and kept[1].tolist() == [40, 60, 0]           # job 0 stays (mbNotErase), job 1 goes instead
    two = casc[2]
    assert two[0].tolist()[:3] == erased[0].tolist() and two[0].tolist()[3:6] == [43, 63, 24] and two[2].tolist()[3:6] == [1, 1, 0]      # chains do not see each other
    big = cc.case("large40x2048")
    assert sum(int((r >= 0).sum()) for r in big["rows"]) > 65536
    rnd = cc.expected("random12x200")
    assert 0 < rnd[5][2].sum() < 12 and rnd[6][0].min() < 150 and rnd[8][1][0] == 300      # verdicts of both kinds, a cascade that removes points, the whole pool


def test_another_address_order_changes_only_the_ties():
    """the reference's ordered list depends on the allocator only inside runs of equal weights, and its maximum rule on the lowest address"""
    c = cc.case("edges")
    M = len(c["rows"])
    q = ("connections", list(range(M)), 15)
    w0, o0, n0 = cc.reference_query(c, q, pin=False)
    w1, o1, n1 = cc.reference_query(c, q, addresses=[M - 1 - m for m in range(M)], pin=False)
    assert np.array_equal(w0, w1) and np.array_equal(n0, n1)
    assert not np.array_equal(o0, o1)
    for j in range(M):
        a, b = o0[j, :n0[j]], o1[j, :n1[j]]
        if n0[j] > 1 or (n0[j] == 1 and w0[j, a[0]] >= 15):
            assert w0[j, a].tolist() == w1[j, b].tolist() and cc.pin_ties(list(a), w0[j]) == cc.pin_ties(list(b), w0[j])
        elif n0[j] == 1:      # nobody reached th: any member of maximal weight, by address
            assert w0[j, a[0]] == w1[j, b[0]] == w0[j].max()
    assert o0[0, :4].tolist() == [4, 5, 3, 2] and o1[0, :4].tolist() == [4, 2, 3, 5]      # (descending pointer inside the tie)


def test_host_refusals():
    b = hl.HostBackend(8, 16, max_members=4)
    assert b.put(0, [1, 2, 3], [0, 0, 0]) == 0 and b.put(1, [3, 4], [0, 0]) == 0 and b.put(2, [5, 9, 5], [0, 0, 0]) == 0
    assert b.put(3, list(range(17)), [0] * 17) == -1 and b.put(8, [1], [0]) == -1
    assert b.build([0, 1]) == 0
    before = b.connections([0, 1], 1)
    assert before[0].tolist() == [[0, 1], [1, 0]]
    assert b.build([0, 2]) == -1                     # an id twice in a row
    assert b.build([0, 5]) == -1                     # an empty slot
    assert b.build([0, 1, 0]) == -1                  # a slot named twice
    assert b.build([0, 1, 2, 3, 4]) == -1            # more than max_members
    assert cc.first_difference([before], [b.connections([0, 1], 1)]) is None      # the previous index stays
    assert b.votes([[3, -2]], code=True) == -1       # a negative id
    assert b.votes([[3, 77]]).tolist() == [[1, 1]]
    assert b.update_map_points([0, 0], [1, 1], [7, 8]) == -1 and b.update_map_points([0], [3], [7]) == -1 and b.update_map_points([5], [0], [7]) == -1
    assert b.update_map_points([0], [0], [1 << 30]) == -1 and b.fetch_mp(0, 3).tolist() == [1, 2, 3]
    assert b.update_map_points([2, 0], [2, 1], [6, -1]) == 0 and b.fetch_mp(2, 3).tolist() == [5, 9, 6] and b.fetch_mp(0, 3).tolist() == [1, -1, 3]
    assert b.connections([0], 1)[0].tolist() == [[0, 1]]      # not seen before the next build
    assert b.build([0, 1, 2]) == 0 and b.connections([0], 1)[0].tolist() == [[0, 1, 0]]
    b.close()


def test_more_than_16384_members_is_unsupported():
    b = hl.HostBackend(4, 4)
    assert b.build(np.zeros(16385, np.int32)) == -3
    b.close()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_core_emulation(build, tmp_path):
    exe = str(tmp_path / ("covis_core_emu_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + BUILDS[build] + [SRC, "-o", exe])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for name in cc.NAMES:
            f.write(cc.to_text(cc.case(name), cc.expected(name)))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "covis_core_emu: ok (%d cases" % len(cc.NAMES) in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-4000:]
