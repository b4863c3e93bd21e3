"""Resident map points without a GPU: the host build of csrc/cms_mappoint_core.h -- the definition of record of cms_mpstore_* -- against the oracle
(orc.distinctive_descriptors, orc.update_normal_and_depth, which tests/test_oracle_tri.py holds against numpy) fed the observation lists of
tests/mappoint_cases.py in ascending member order.  Every comparison is exact: indices, descriptors and status by value, floats by their bits.  The
conditions the GPU suite's inputs must satisfy are asserted here, under the oracle."""
import numpy as np
import pytest

import mappoint_cases as mc
import mappoint_hostlib as hl
import orc
from cubemapslam_amd import synth

hl.H()      # the host build's hm_mpstore_* entries, now: without them no test of this file means anything
_host = {}


def host_run(name):
    if name not in _host:
        c = mc.case(name)
        b = hl.HostBackend(c["K"], c["maxf"])
        _host[name] = mc.run(c, b)
        b.close()
    return _host[name]


@pytest.mark.parametrize("name", mc.NAMES)
def test_host_core_equals_oracle(name):
    want = mc.expected(name)
    assert len(want[0]) > 0 and (want[0] == 0).any()
    assert mc.difference(want, host_run(name)) is None, mc.difference(want, host_run(name))


def test_known_answer():
    """three key frames by hand: winners, normals and bounds as written out in mappoint_cases.known3_by_hand"""
    hand = mc.known3_by_hand()
    assert mc.difference(hand, mc.expected("known3")) is None, mc.difference(hand, mc.expected("known3"))
    assert mc.difference(hand, host_run("known3")) is None
    c = mc.case("known3")
    assert mc.medians(c, 10).tolist() == [2, 6, 2] and mc.medians(c, 13).tolist() == [32, 1, 1] and mc.medians(c, 11).tolist() == [0, 0]


def test_counts_cover_both_sides_of_the_wavefront():
    c = mc.case("counts")
    assert [len(mc.observations(c, int(i))) for i in c["ids"]] == mc.COUNTS == [1, 2, 3, 4, 5, 63, 64, 65, 130]
    assert (mc.expected("counts")[0] == 0).all()
    assert c["slots"] != sorted(c["slots"])      # slot order is not member order


def test_ties_follow_the_member_order():
    """identical descriptors among the observers: the winner is the earliest member position of each listing, and the two listings of the same map
    differ in a winner or in the normal's bits for some point -- otherwise the case would not test the rule"""
    a, b = mc.case("ties"), mc.case("ties_permuted")
    assert a["slots"] == sorted(a["slots"], reverse=True) and sorted(b["slots"]) == sorted(a["slots"]) and b["slots"] != a["slots"]
    ea, eb = mc.expected("ties"), mc.expected("ties_permuted")
    n_tied = 0
    for c, e in ((a, ea), (b, eb)):
        for i, id_ in enumerate(c["ids"]):
            med = mc.medians(c, int(id_))
            first = int(np.flatnonzero(med == med.min())[0])
            assert mc.observations(c, int(id_))[first][0] == e[1]["best_member"][i]
            n_tied += int((med == med.min()).sum() > 1)
    assert n_tied >= 20
    slot_a = [a["slots"][m] for m in ea[1]["best_member"]]; slot_b = [b["slots"][m] for m in eb[1]["best_member"]]
    other_winner = sum(x != y for x, y in zip(slot_a, slot_b))
    other_normal = int((ea[1]["normal"].view(np.uint32) != eb[1]["normal"].view(np.uint32)).any(axis=1).sum())
    print("ties: %d points with another winner, %d with other normal bits under the permuted listing" % (other_winner, other_normal))
    assert other_winner + other_normal > 0
    assert np.array_equal(ea[1]["min_dist"].view(np.uint32), eb[1]["min_dist"].view(np.uint32))      # the bounds do not depend on the order


def test_random_case_has_tied_medians():
    c = mc.case("random12x200")
    tied = 0
    for id_ in c["ids"]:
        if mc.observations(c, int(id_)):
            med = mc.medians(c, int(id_))
            tied += int((med == med.min()).sum() > 1)
    assert tied >= 10, tied
    assert len(c["ids"]) == 300 and (mc.expected("random12x200")[0] == 0).sum() > 250


@pytest.mark.parametrize("name", ["known3", "random12x200", "counts"])
def test_host_index_with_features_equals_the_restatement(name):
    c = mc.case(name)
    b = hl.HostBackend(c["K"], c["maxf"])
    b.load(c)
    want = mc.reference_observations(c)
    assert len(want) > 0
    for id_, obs in want.items():
        got = b.observations(id_)
        assert [(m, f) for m, f, o in got] == obs and got == mc.observations(c, id_), id_
    assert b.observations(999) == []
    b.close()


@pytest.mark.parametrize("name", ["known3", "ties", "counts", "random12x200"])
def test_mirror_host_core_equals_host_core(name):
    """CubemapSLAM::MapPointStore (host/cubemap_hot_path.h) with HOST_CORE: Build, SetMapPoints, Refresh and Fetch give the host core's rows"""
    got = hl.mirror(1, mc.case(name))
    assert mc.difference(host_run(name), got) is None, mc.difference(host_run(name), got)


def _ref_scenario(b):
    """`ref`: the reference slot first in member order, last, a member that does not observe the point, no member at all; and an id the index does not know"""
    c = mc.case("known3")
    b.load(c)
    ids = [10, 13, 11, 12, 77]
    pos = [[0, 0, 4], [0, 0, 4], [0, -2, 0], [4, 0, 0], [1, 2, 3]]
    ref = [5, 19, 12, 40, 5]      # 10: member 0; 13: member 2; 11: member 1 does not observe it; 12: slot 40 is no member; 77: unknown
    b.set(ids, pos, ref)
    before = b.fetch(ids)
    status = b.refresh(ids, mc.BOTH)
    return c, ids, pos, ref, before, status, b.fetch(ids)


def check_ref_scenario(b):
    c, ids, pos, ref, before, status, after = _ref_scenario(b)
    assert status.tolist() == [0, 0, 2, 2, 1]
    want = mc.oracle_refresh(c, ids, pos, ref)
    assert mc.difference(want, (status, after)) is None, mc.difference(want, (status, after))
    for i in (2, 3, 4):      # rows with status 1 or 2 keep their previous contents
        assert mc.rows_difference({k: v[i:i + 1] for k, v in before.items()}, {k: v[i:i + 1] for k, v in after.items()}) is None
    # ... also when they held something: refresh rows 11 and 12 properly, then again with a reference that fails
    b.set([11, 12], None, [5, 12])
    assert b.refresh([11, 12], mc.BOTH).tolist() == [0, 0]
    held = b.fetch([11, 12])
    assert held["best_member"].tolist() == [0, 1]
    b.set([11, 12], None, [12, 40])
    assert b.refresh([11, 12], mc.BOTH).tolist() == [2, 2]
    assert mc.rows_difference(held, b.fetch([11, 12])) is None
    assert b.refresh([11, 12], mc.DESCRIPTOR).tolist() == [0, 0]      # the descriptor alone asks for no reference


def test_ref_statuses_host():
    b = hl.HostBackend()
    check_ref_scenario(b)
    b.close()


def check_what_scenario(b):
    """CMS_MP_NORMAL_DEPTH alone leaves descriptor and best (member, feature) untouched, and vice versa"""
    c = mc.case("known3")
    b.load(c)
    b.set(c["ids"], c["pos"], c["ref"])
    assert (b.refresh(c["ids"], mc.NORMAL_DEPTH) == 0).all()
    got = b.fetch(c["ids"])
    want = mc.oracle_refresh(c, c["ids"], c["pos"], c["ref"], mc.NORMAL_DEPTH)[1]
    assert mc.rows_difference(want, got) is None and (got["best_member"] == -1).all() and not got["desc"].any()
    assert (got["max_dist"] > 0).all()
    b.erase(c["ids"]); b.set(c["ids"], c["pos"], c["ref"])
    assert (b.refresh(c["ids"], mc.DESCRIPTOR) == 0).all()
    got = b.fetch(c["ids"])
    want = mc.oracle_refresh(c, c["ids"], c["pos"], c["ref"], mc.DESCRIPTOR)[1]
    assert mc.rows_difference(want, got) is None and not got["normal"].any() and not got["max_dist"].any()
    assert got["best_member"].tolist() == [0, 0, 1, 1]
    # the halves one after the other give what both at once give
    assert (b.refresh(c["ids"], mc.NORMAL_DEPTH) == 0).all()
    assert mc.rows_difference(mc.expected("known3")[1], b.fetch(c["ids"])) is None


def test_what_selects_the_half_host():
    b = hl.HostBackend()
    check_what_scenario(b)
    b.close()


def check_snapshot_scenario(b):
    """a pose update after the build is used by the next refresh; a map-point update after the build is not seen until the next build"""
    c = mc.case("known3")
    b.load(c)
    b.set(c["ids"], c["pos"], c["ref"])
    assert (b.refresh(c["ids"]) == 0).all()
    first = b.fetch(c["ids"])
    moved = [o.copy() for o in c["Ows"]]
    moved[1] = np.array([4, 0, 8], np.float32)      # member 1 moves: id 10's and 12's ni and the bounds of the points it is the reference of
    b.update_poses([c["slots"][1]], moved[1])
    s0, s2 = c["slots"][0], c["slots"][2]
    b.update_map_points([s0, s2], [3, 0], [12, 12])      # id 12 gains two observers in the store's rows: not in the index yet
    assert (b.refresh(c["ids"]) == 0).all()
    want = mc.oracle_refresh(c, c["ids"], c["pos"], c["ref"], Ows=moved)
    got = b.fetch(c["ids"])
    assert mc.rows_difference(want[1], got) is None, mc.rows_difference(want[1], got)
    assert mc.rows_difference(first, got) is not None and got["max_dist"][0] != first["max_dist"][0]
    assert np.array_equal(got["normal"][2], [0, 0, -1])      # id 12 is still member 1's alone
    c2 = dict(c, rows=[r.copy() for r in c["rows"]])
    c2["rows"][0][3] = 12; c2["rows"][2][0] = 12
    b.build(c["slots"])
    assert (b.refresh(c["ids"]) == 0).all()
    want2 = mc.oracle_refresh(c2, c["ids"], c["pos"], c["ref"], Ows=moved)
    assert mc.rows_difference(want2[1], b.fetch(c["ids"])) is None
    assert mc.rows_difference(want[1], want2[1]) is not None


def test_snapshot_rule_host():
    b = hl.HostBackend()
    check_snapshot_scenario(b)
    b.close()


def check_table_refusals(b):
    """id out of range, an id twice, a row never set: refused with nothing written"""
    c = mc.case("known3")
    b.load(c)
    b.set(c["ids"], c["pos"], c["ref"])
    assert (b.refresh(c["ids"]) == 0).all()
    before = b.fetch(c["ids"])
    reasons = []
    for call in (lambda: b.set([10, mc.MAX_POINTS], [[1, 1, 1], [2, 2, 2]], [5, 5]), lambda: b.set([10, -1], [[1, 1, 1], [2, 2, 2]], [5, 5]),
                 lambda: b.set([10, 11, 10], [[1, 1, 1]] * 3, [5, 5, 5]), lambda: b.set([10, 500], [[1, 1, 1], [2, 2, 2]], None),
                 lambda: b.set([10], [[1, 1, 1]], [c["K"]]), lambda: b.erase([10, 10]), lambda: b.erase([11, mc.MAX_POINTS]),
                 lambda: b.refresh([10, 11, 10]), lambda: b.refresh([10, mc.MAX_POINTS]), lambda: b.refresh([10, 500]), lambda: b.refresh([10], 0), lambda: b.refresh([10], 4),
                 lambda: b.fetch([10, mc.MAX_POINTS])):
        with pytest.raises(hl.Refused) as ei:
            call()
        reasons.append(str(ei.value))
    assert mc.rows_difference(before, b.fetch(c["ids"])) is None
    assert not b.fetch([500])["pos"].any()      # the row a refused set named was not created
    b.erase([11])
    with pytest.raises(hl.Refused):
        b.refresh([11])                          # erased: the row is empty again
    e = b.fetch([11])
    assert mc.rows_difference(mc.empty_rows(1), e) is None
    return reasons


def test_host_refusals():
    b = hl.HostBackend()
    check_table_refusals(b)
    b.close()


# ---- the inputs of the GPU suite's consumer tests satisfy their conditions under the oracle
def search_table():
    """the search case's rows from the host core (which equals the oracle's refresh)"""
    if "search" not in _host:
        c = mc.search_case()
        b = hl.HostBackend(c["K"], c["maxf"])
        _host["search"] = mc.run(c, b)
        b.close()
    return _host["search"]


def test_search_case_rows_equal_the_oracle():
    c = mc.search_case()
    want = mc.oracle_refresh(c, c["ids"], c["pos"], c["ref"])
    assert (want[0] == 0).all() and mc.difference(want, search_table()) is None


def test_search_input_has_matches_under_the_oracle():
    c = mc.search_case()
    rows = search_table()[1]
    ocam = orc.make_camera(synth.camera("lafida", mc.F_SEARCH))
    fr = orc.is_in_frustum(ocam, c["pose15"], rows["pos"], rows["normal"], rows["min_dist"], rows["max_dist"])
    kp_mp = np.full(len(c["kx"]), -1, np.int32); kp_mp[::9] = 10 ** 6
    match, nm = orc.search_local_points(ocam, c["kx"], c["ky"], c["ko"], c["kd"], mc.SF, fr, rows["desc"], kp_mp, th=5.0)
    assert nm >= 50, nm


def test_fuse_input_has_hits_under_the_oracle():
    c = mc.search_case()
    rows = search_table()[1]
    ocam = orc.make_camera(synth.camera("lafida", mc.F_SEARCH))
    sets, jobs = mc.fuse_jobs(c)
    targets = dict(mc.target_keyframes(c))
    sigma2 = (mc.SF * mc.SF).astype(np.float32); inv_s2 = (np.float32(1.0) / sigma2).astype(np.float32)
    hits = 0
    for slot, s in jobs:
        t = targets[slot]
        n = len(t["x"])
        kf = dict(t, angle=np.zeros(n, np.float32), mp=np.full(n, -1, np.int32), R=c["pose15"][:9].reshape(3, 3), t=c["pose15"][9:12], Ow=c["pose15"][12:15],
                  node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32), median_depth=1.0)
        K, keep = orc.make_keyframe(ocam, kf)
        ids = sets[s]
        bi, bd = orc.fuse_search(ocam, K, np.zeros(len(ids), np.uint8), rows["pos"][ids], rows["normal"][ids], rows["min_dist"][ids], rows["max_dist"][ids],
                                 rows["desc"][ids], 3.0, mc.SF, inv_s2)
        hits += int((bi >= 0).sum())
    assert hits >= 20, hits
