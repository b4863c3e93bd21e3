"""The host build of the map-point statistics (csrc/cms_mpstats_core.h through hm_mpstats_*, the definition of record of cms_mpstore_set_stats /
add_stats / fetch_stats / count / culling, cms_covis_tracked_map_points and cms_kfstore_scene_median_depth) against the literal restatement of the
reference in tests/npref_mpstats.py, on every case of tests/mpstats_cases.py, and the mirror's methods through its HOST_CORE engine.  Every
comparison is exact: integers and verdict bytes by value, depths by their bits."""
import numpy as np
import pytest

import mpstats_cases as sc
import mpstats_hostlib as hl
import npref_mpstats as ref

f32 = np.float32
hl.H()      # (the feature's names, at import: hm_mpstats_*)
_host = {}


def host_run(name):
    """the host core's outputs of a case (computed once; tests/test_gpu_mpstats.py compares the device with them)"""
    if name not in _host:
        _host[name] = sc.run(name, lambda kind: hl.HostBackend(*sc.STORES[kind]))
    return _host[name]


@pytest.mark.parametrize("name", sc.NAMES)
def test_host_core_equals_the_restatement(name):
    d = sc.difference(sc.expected(name), host_run(name))
    assert d is None, d


def test_verdicts_by_hand():
    """the restatement itself against the table written next to the case, and against the branches' arithmetic spelled out"""
    got = dict(sc.expected("culling"))
    a, b = sc.culling_by_hand()
    assert np.array_equal(got["verdicts A"], a) and np.array_equal(got["verdicts B"], b)
    assert set(a.tolist()) == {0, 1, 2, 3, 4}
    # both conversions of 4 194 305 / 16 777 217 round (the second to 2^24): the float quotient is above 0.25, 4 194 304 / 16 777 217 is exactly
    # 0.25 in float although the exact quotient is below it
    assert f32(16777217) == f32(16777216) and ref.found_ratio(4194304, 16777217) == f32(0.25) and 4194304 / 16777217 < 0.25
    assert ref.culling_verdict(1, 4, 0, 5, 0, 2) == 0 and ref.culling_verdict(1, 5, 0, 5, 0, 2) == 1


def test_counts_by_hand():
    """the counting rule against np.bincount"""
    jobs, flags = sc.count_jobs()
    ids = np.concatenate(jobs); fl = np.concatenate(flags)
    vis = np.ones(sc.N_COUNT, np.int64); found = np.ones(sc.N_COUNT, np.int64)
    vis += np.bincount(ids[(ids >= 0) & (fl != 0)], minlength=sc.N_COUNT)
    found += np.bincount(ids[(ids >= 0) & (fl == 0)], minlength=sc.N_COUNT)
    again = np.concatenate([jobs[3], jobs[0]])
    vis += np.bincount(again[again >= 0], minlength=sc.N_COUNT)
    vis[7] += 1
    got = dict(host_run("count"))
    assert np.array_equal(got["after the counts"][0], vis) and np.array_equal(got["after the counts"][1], found)
    assert (got["after the counts"][2] == -1).all() and (got["fresh rows"] == np.array([[1], [1], [-1]])).all()
    assert np.array_equal(got["after refused counts"], got["after the counts"])
    after = got["after set and add"]
    assert after[:, 10].tolist() == [vis[10], 0, 5] and after[:, 11].tolist() == [vis[11] + 3, 2, 6] and after[:, 12].tolist() == [vis[12], 7, 0]
    assert after[:, 13].tolist() == [9, found[13] + 1, -1] and np.array_equal(after[:, 14:], got["after the counts"][:, 14:])
    # rows 7 and 11 erased, row 12 as it was, row 600 never set
    assert np.array_equal(got["erased rows read (1, 1, -1)"], np.array([[1, 1, vis[12], 1], [1, 1, 7, 1], [-1, -1, 0, -1]]))


def test_apply_by_hand():
    got = dict(host_run("culling_apply"))
    assert got["verdicts"].tolist() == [1, 0, 2, 1, 4]          # 900 by ratio, 902 stays, 901 by observations, 903 by the ratio the count made, 904 empty
    assert got["the changed entry"].tolist() == [905]
    assert got["counters"].T.tolist() == [[1, 1, -1], [1, 1, -1], [2, 1, 4], [1, 1, -1]]
    assert got["the index is stale"].tolist() == [70, 2, 5, 3] and got["after the rebuild"].tolist() == [0, 0, 5, 0, 1]
    assert got["again: empty rows"].tolist() == [4, 4, 3, 4]
    rows = got["mp rows"]
    assert (rows == 900).sum() == 0 and (rows == 905).sum() == 1 and (rows == 902).sum() == 5 and (rows == 901).sum() == 0 and (rows == 903).sum() == 0


def test_tracked_by_hand():
    got = dict(host_run("tracked"))
    rows = sc._track_rows()
    ids, n_obs = np.unique(np.concatenate([r[r >= 0] for r in rows]), return_counts=True)
    seen = dict(zip(ids.tolist(), n_obs.tolist()))
    want = [sum(1 for v in rows[m] if v >= 0 and (need <= 0 or seen[int(v)] >= need)) for m in range(5) for need in (0, 1, 2, 3, 4)]
    assert got["counts"].tolist() == want and want[:5] == [0] * 5
    assert sorted(set(n_obs.tolist())) == [1, 2, 3, 4]           # ids with exactly min_obs - 1 and min_obs observations, for every min_obs
    assert np.array_equal(got["after a change, before the build"], got["counts"]) and got["after the build"][20] == got["counts"][20] - 30


def test_median_edges_by_hand():
    got = dict(host_run("median_edges"))
    B = lambda v: sc.bits(np.array(v, f32)).tolist()
    assert sc.bits(got["depth q=2"]).tolist() == B([3, -2, -0.0, 0.0]) and got["n q=2"].tolist() == [7, 5, 6, 5]
    assert sc.bits(got["depth q=1"]).tolist() == B([9, -0.5, 2, 2]) and sc.bits(got["depth q=7"]).tolist() == B([-1, -8, -1, -1])
    # the double accumulation is visible: the float-only sum of the case differs in the last bit
    R, t, X = sc.double_sum_case()
    lone = ref.depth(R, t, X)
    assert sc.bits(got["double sum"]).tolist() == B([lone]) and abs(int(sc.bits(lone)[0]) - int(sc.bits(ref.depth_float_only(R, t, X))[0])) == 1
    empty = dict(host_run("median_small"))
    assert sc.bits(empty["depth q=2"])[-1] == sc.bits(f32(-1.0)) and empty["n q=2"].tolist() == [1, 2, 3, 64, 65, 255, 256, 0]
    assert dict(host_run("median_big"))["n q=1"].tolist() == sc.BIG_N


def test_depth_key_is_monotone():
    """the integer image orders like the floats, -0.0f before +0.0f, and decodes to the same bits (through the host core: one slot per pair)"""
    vals = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.float32(1.0) + np.float32(2 ** -23), 7e37, np.inf], f32)
    b = hl.HostBackend(*sc.STORES["std"])
    b.set(np.arange(len(vals)), np.stack([np.copysign(f32(0), vals), np.copysign(f32(0), vals), vals], axis=1), np.zeros(len(vals), np.int32))
    for i in range(len(vals) - 1):
        b.put(i, [i, i + 1], None, np.eye(3, dtype=f32), np.array([0, 0, -0.0], f32))
    lo, n = b.median_depth(np.arange(len(vals) - 1), 2)      # index 0 of two: the smaller
    hi, _ = b.median_depth(np.arange(len(vals) - 1), 1)      # index 1: the larger
    assert np.array_equal(sc.bits(lo), sc.bits(vals[:-1])) and np.array_equal(sc.bits(hi), sc.bits(vals[1:])) and (n == 2).all()
    b.close()


def test_store_keeps_the_median():
    b = hl.HostBackend(*sc.STORES["std"])
    b.set([1, 2, 3], np.array([[0, 0, 2], [0, 0, 5], [0, 0, 9]], f32), [0, 0, 0])
    b.put(0, [1, 2, 3]); b.put(1, [-1, -1])
    assert b.stored_median(0) == f32(1.0)
    d, n = b.median_depth([0, 1], 2, store=False)
    assert b.stored_median(0) == f32(1.0)
    d, n = b.median_depth([0, 1], 2, store=True)
    assert d.tolist() == [5.0, -1.0] and n.tolist() == [3, 0]
    assert b.stored_median(0) == f32(5.0) and b.stored_median(1) == f32(1.0)      # a slot without a depth keeps what it had
    b.close()


def test_mirror_host_core_equals_the_restatement():
    """CubemapSLAM::MapPointStore (host/cubemap_hot_path.h): UpdateTrackStatistics, MapPointCulling with its list handling, TrackedMapPoints and
    ComputeSceneMedianDepth through HOST_CORE"""
    c = hl.mirror_case()
    want, got = hl.mirror_expected(c), hl.mirror(1, c)
    assert sc.difference(want, got) is None, sc.difference(want, got)
    v = dict(got)["verdict"]
    assert {0, 1, 2, 3} <= set(v.tolist()), np.bincount(v)
