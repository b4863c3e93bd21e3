"""Map-point statistics on the device (cms_mpstore_set_stats / add_stats / fetch_stats / count / culling, cms_covis_tracked_map_points,
cms_kfstore_scene_median_depth) against the host build of csrc/cms_mpstats_core.h, which tests/test_mpstats_cpu.py holds against the restatement of
the reference.  Every comparison is exact: integers and verdict bytes by value, depths by their bits.  The cases are tests/mpstats_cases.py's, on
stores of 64 slots x 256 features, 136 x 64 and 4 x 4 096; the last two tests run on the generator of tests/test_gpu_mapping_sequence.py."""
import ctypes as C

import numpy as np
import pytest

import mappoint_hostlib as mhl
import mpstats_cases as sc
import mpstats_hostlib as hl
import test_gpu_mapping_sequence as gen
import test_mpstats_cpu as cpu
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

F = 150
f32 = np.float32
culling = api.MapPointStore.culling      # (the feature's names, at import)


@pytest.fixture(scope="module")
def ctxs():
    """two frame contexts: their streams are not the store's, and not each other's"""
    c = [api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1) for _ in range(2)]
    yield c
    for x in c:
        x.close()


@pytest.fixture(scope="module")
def cg():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1)      # the mapping side's context
    yield c
    c.close()


@pytest.fixture(scope="module")
def backends(cg, ctxs):
    made = {}

    def make(kind):
        if kind not in made:
            K, maxf, max_points = sc.STORES[kind]
            made[kind] = hl.DeviceBackend(api.KeyframeStore(cg, max_keyframes=K, max_features=maxf, max_nodes=8), ctxs, K, max_points)
        made[kind].reset()
        return made[kind]
    yield make
    for b in made.values():
        b.close(); b.st.close()


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_equals_host_core(backends, name):
    got = sc.run(name, backends)
    d = sc.difference(cpu.host_run(name), got)
    assert d is None, d


def test_mirror_device_equals_host_core():
    """CubemapSLAM::MapPointStore (host/cubemap_hot_path.h) through both engines"""
    c = hl.mirror_case()
    d, h = hl.mirror(0, c), hl.mirror(1, c)
    assert sc.difference(h, d) is None, sc.difference(h, d)


def test_refusals_name_their_reason(backends, cg):
    b = backends("std")
    b.put(0, [1, 2, 3])
    b.set([1, 2, 3], np.zeros((3, 3), f32), [0, 0, 0])
    why = sc.refused(b.culling, [[1]], [0], 2, True)
    assert "cms_mpstore_culling" in why and "no index" in why
    b.build([0])
    other = api.KeyframeStore(cg, max_keyframes=4, max_features=16, max_nodes=8)
    cv = api.Covisibility(other, 4)
    cv.build([])
    with pytest.raises(api.CmsError) as ei:
        b.mp.culling(cv, [[1]], [0], 2, True)
    assert "another store" in str(ei.value)
    mp2 = api.MapPointStore(other, 16)
    with pytest.raises(api.CmsError) as ei:
        b.st.scene_median_depth(mp2, [0])
    assert "another store" in str(ei.value)
    mp2.close(); cv.close(); other.close()
    assert "twice" in sc.refused(b.culling, [[1, 2], [1]], [0, 0], 2, True)
    assert "outside the table" in sc.refused(b.culling, [[1, 5000]], [0], 2, True)
    assert "outside the table" in sc.refused(b.count, sc.VISIBLE, [[1, 5000]])
    assert "never set" in sc.refused(b.count, sc.VISIBLE, [[1, 9]])
    assert "never set" in sc.refused(b.set_stats, [9], found=[1])
    assert "visible >= 1" in sc.refused(b.set_stats, [1], visible=[0])
    assert "no member" in sc.refused(b.tracked, [1], [0])
    assert "twice" in sc.refused(b.median_depth, [0, 0]) and "empty" in sc.refused(b.median_depth, [7])
    # nothing was written by any of them
    assert np.stack(b.fetch_stats([1, 2, 3])).tolist() == [[1, 1, 1], [1, 1, 1], [-1, -1, -1]] and b.fetch_mp(0).tolist() == [1, 2, 3]


def test_a_culled_point_is_refused_by_the_search(backends, ctxs):
    """after culling with apply, cms_search_local_points_ids on the id is refused like an erased row"""
    c = mhl.mc.case("known3")
    b = backends("std")
    for s, r, o, d, w in zip(c["slots"], c["rows"], c["octs"], c["descs"], c["Ows"]):
        K, keep = mhl.keyframe(r, o, d, w)
        b.st.put(int(s), K)
    b.build(c["slots"])
    b.set(c["ids"], c["pos"], c["ref"])
    assert (b.mp.refresh(b.cv, c["ids"]) == 0).all()
    kps = np.zeros(4, api.KP_DTYPE); kps["x"] = [20, 30, 40, 50]; kps["y"] = 20
    ctx = ctxs[0]
    ctx.area_set_keypoints(0, kps); ctx.area_set_descriptors(0, np.zeros((4, 32), np.uint8)); ctx.area_grid(1)
    pose15 = np.concatenate([np.eye(3).reshape(9), np.zeros(6)]).astype(f32)
    kp = np.full(4, -1, np.int32)
    ctx.search_local_points_ids(0, pose15, b.mp, c["ids"], kp)      # all four rows can be searched
    b.set_stats([11], found=[0])                                    # id 11: found ratio 0
    v = b.culling([c["ids"]], [0], 2, True)[0]
    assert v.tolist() == [0, 1, 0, 0]
    with pytest.raises(api.CmsError) as ei:
        ctx.search_local_points_ids(0, pose15, b.mp, [11], kp)
    assert "erased, or never refreshed" in str(ei.value)
    ctx.search_local_points_ids(0, pose15, b.mp, [10, 12, 13], kp)


# ---- on the generator of tests/test_gpu_mapping_sequence.py: four rendered frames of the box room, extracted on the device, resident in a store
@pytest.fixture(scope="module")
def room():
    Fr = 550
    camd = synth.camera("lafida", Fr)
    camd["nfeatures"] = 2000
    scene = synth.room_scene(0xC0FFEE)
    gts = [synth.room_pose(i, 300) for i in (0, 6, 12, 18)]
    frames = np.stack([synth.render_fisheye(camd, scene, R, t) for R, t in gts])
    ctx = api.Context(camd, nfeatures=2000, max_batch=4)
    ctx.set_mask(synth.cubemap_valid_mask(camd))
    ctx.upload(frames); ctx.process(4, True); ctx.area_grid(4); ctx.sync()
    kfs = []
    for b in range(4):
        k, d = ctx.fetch(b)
        kfs.append(gen._kf_from_frame(k, d, gts[b][0], gts[b][1]))
    cg = api.Context(camd, nfeatures=2000, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=5, max_features=4096, max_nodes=1024)
    st.put_from_frames(ctx, [(b, b, len(kfs[b]["x"]), kfs[b]) for b in range(4)])
    yield dict(ctx=ctx, cg=cg, st=st, kfs=kfs)
    st.close(); cg.close(); ctx.close()


def _new_points(st, kfs, first_id):
    """CreateNewMapPoints of key frame 0 against 1, 2, 3 and the bookkeeping of LocalMapping.cpp:359-381: ids from first_id, the key frames' rows (a
    key point named by two new points keeps the later one) -> (ids, positions, the records)"""
    rec = st.create_new_map_points([(0, [1, 2, 3])], cap=4096)[0]
    gn, g1, g2, gx = rec
    ids = np.arange(first_id, first_id + len(gn))
    for j, pid in enumerate(ids):
        kfs[0]["mp"][g1[j]] = pid; kfs[1 + gn[j]]["mp"][g2[j]] = pid
    for b in range(4):
        st.update(b, mp=kfs[b]["mp"])
    return ids, gx, rec


def _same_records(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(sc.bits(a[3]), sc.bits(b[3]))


def test_mapping_step_on_device_statistics(room, ctxs):
    """count over eight frames -> culling with apply -> rebuild -> median depth with store -> CreateNewMapPoints -> tracked count; every stage equals
    the host core fed the same calls, and CreateNewMapPoints returns the records it returns after the same median went through cms_kfstore_update"""
    st, kfs = room["st"], room["kfs"]
    for kf in kfs:
        kf["mp"][:] = -1
    for b in range(4):
        st.update(b, mp=kfs[b]["mp"], median_depth=2.0)
    cv = api.Covisibility(st, 4); mp = api.MapPointStore(st, 8192)
    host = hl.HostBackend(5, 4096, 8192)
    ids, pos, _ = _new_points(st, kfs, 0)
    n = len(ids)
    assert n > 100
    mp.set(ids, pos, np.zeros(n, np.int32)); host.set(ids, pos, np.zeros(n, np.int32))
    for b in range(4):
        host.put(b, kfs[b]["mp"], kfs[b]["octave"], kfs[b]["R"], kfs[b]["t"])
    cv.build([0, 1, 2, 3]); host.build([0, 1, 2, 3])
    rng = np.random.default_rng(1)
    first = rng.integers(0, 3, n)
    for t in (mp, host):
        t.set_stats(ids, first_kf=first)
    # ---- eight frames: the local ids with in_view, then the frame's ids with outlier
    frames = [np.where(rng.random(1500) < 0.8, rng.integers(0, n, 1500), -1) for _ in range(8)]
    in_view = [(rng.random(1500) < 0.7).astype(np.uint8) for _ in range(8)]
    outlier = [(rng.random(1500) < 0.75).astype(np.uint8) for _ in range(8)]
    mp.count(ctxs[0], api.MP_VISIBLE, frames[:5], in_view[:5], 1); mp.count(ctxs[1], api.MP_VISIBLE, frames[5:], in_view[5:], 1)
    mp.count(ctxs[1], api.MP_FOUND, frames, outlier, 0)
    host.count(sc.VISIBLE, frames, in_view, 1); host.count(sc.FOUND, frames, outlier, 0)
    # ---- MapPointCulling of key frame 3 (no host wait between the counts and the call)
    v = mp.culling(cv, [ids], [3], 2, True)[0]
    hv = host.culling([ids], [3], 2, True)[0]
    assert np.array_equal(v, hv) and {0, 1, 2} <= set(v.tolist()), np.bincount(v)
    assert all(np.array_equal(a, b) for a, b in zip(mp.fetch_stats(ids), host.fetch_stats(ids)))
    for b in range(4):
        row = st.debug_fetch(b)["mp"]
        assert np.array_equal(row, host.fetch_mp(b))
        kfs[b]["mp"][:] = row
    cv.build([0, 1, 2, 3]); host.build([0, 1, 2, 3])
    # ---- the scene median depth of the key frame and its neighbours, kept in the store
    want_d, want_n = host.median_depth([0, 1, 2, 3], 2, True)
    assert (want_n > 0).all() and (want_d > 0).all()
    jobs = [(0, [1, 2, 3])]
    for b in range(4):
        st.update(b, median_depth=float(want_d[b]))
    through_update = st.create_new_map_points(jobs, cap=4096)[0]
    for b in range(4):
        st.update(b, median_depth=1e6)                 # a stale value: every baseline is too short against it
    assert len(st.create_new_map_points(jobs, cap=4096)[0][0]) == 0
    d, nd = st.scene_median_depth(mp, [0, 1, 2, 3], 2, store=False)
    assert np.array_equal(sc.bits(d), sc.bits(want_d)) and np.array_equal(nd, want_n)
    assert len(st.create_new_map_points(jobs, cap=4096)[0][0]) == 0      # store = 0 keeps the stale value
    d, nd = st.scene_median_depth(mp, [0, 1, 2, 3], 2, store=True)
    assert np.array_equal(sc.bits(d), sc.bits(want_d)) and np.array_equal(nd, want_n)
    # ---- CreateNewMapPoints reads it without the host ever seeing a position
    ids2, pos2, rec = _new_points(st, kfs, n)
    assert len(ids2) > 0 and _same_records(rec, through_update)
    mp.set(ids2, pos2, np.zeros(len(ids2), np.int32)); host.set(ids2, pos2, np.zeros(len(ids2), np.int32))
    for b in range(4):
        f = np.flatnonzero(kfs[b]["mp"] >= n)
        host.update_map_points(np.full(len(f), b), f, kfs[b]["mp"][f])
    cv.build([0, 1, 2, 3]); host.build([0, 1, 2, 3])
    # ---- NeedNewKeyFrame's count
    members, min_obs = np.repeat(np.arange(4), 4), np.tile([0, 1, 2, 3], 4)
    c = cv.tracked_map_points(ctxs[0], members, min_obs)
    assert np.array_equal(c, host.tracked(members, min_obs)) and c[0] >= c[2] >= c[3] and c[0] > 0
    host.close(); mp.close(); cv.close()
