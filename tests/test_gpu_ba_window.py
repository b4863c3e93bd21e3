"""The local BA window assembled on the device (cms_covis_local_ba_windows) against the host build of csrc/cms_ba_window_core.h, which
tests/test_ba_window_cpu.py holds against the restatement of Optimizer.cpp:194-357.  Every output is compared with array_equal.  The cases are
tests/ba_window_cases.py's; each store is filled once per module."""
import copy

import numpy as np
import pytest

import ba_window_cases as bc
import ba_window_hostlib as bh
from cubemapslam_amd import api

pytestmark = pytest.mark.gpu

ARRAYS = ("counts",) + api.BA_WINDOW_ARRAYS
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(bc.CAMD, nfeatures=500, max_batch=1)
    g = c.geom
    assert g.F == bc.F and g.nlevels == bc.NLEVELS and np.array_equal(np.array([g.inv_sigma2[l] for l in range(g.nlevels)], np.float32), bc.INV_SIGMA2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def maps(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = bh.DeviceMap(ctx, bc.case(name))
        return made[name]
    yield get
    for m in made.values():
        m.close()


def untouched(o):
    return all((o[k].view(np.uint8) == SENTINEL).all() for k in ARRAYS)


@pytest.mark.parametrize("pinned", (False, True))
@pytest.mark.parametrize("name", bc.NAMES)
def test_device_equals_host_core(maps, name, pinned):
    c = bc.case(name)
    rc, want = bh.host_windows(c)
    got = maps(name).windows(pinned=pinned)
    assert rc == 0 and bc.difference(want, got) is None, bc.difference(want, got)


def test_a_pinned_window_stops_at_its_counts(maps):
    c = bc.case("filters")
    o = api.ba_window_arrays(len(c["jobs"]) + 1, *c["caps"], pinned=True, fill=SENTINEL)
    got = maps("filters").windows(pinned=True, out=o)
    want = bh.host_windows(c)[1]
    assert bc.difference(want, got) is None
    for j, w in enumerate(want + [None]):
        K, _, P, E = (0, 0, 0, 0) if w is None else (int(v) for v in w["counts"])
        for k in api.BA_WINDOW_ARRAYS:
            n = K if k in ("kf_member", "poses", "fixed") else P if k in ("point_id", "points") else E
            assert (o[k][j, n:].view(np.uint8) == SENTINEL).all(), (j, k)


def test_snapshot_rule(ctx):
    """rows, features and octaves are the build's; poses and positions are what the store and the table hold when the call runs"""
    c = copy.deepcopy(bc.case("fixed_order"))
    dm = bh.DeviceMap(ctx, c)
    before = bh.host_windows(c)[1]
    # member 6 would join the fixed key frames through point 12: not seen before the next build
    dm.st.update_map_points([c["slots"][6]], [0], [12])
    assert bc.difference(before, dm.windows()) is None
    # a new pose of local member 2 and of fixed member 7, a new position of point 11: seen
    rng = np.random.default_rng(5)
    for m in (2, 7):
        c["members"][m]["R"] = bc.rotation(rng, 2); c["members"][m]["t"] = rng.normal(size=3).astype(np.float32)
    R = np.stack([c["members"][m]["R"] for m in (2, 7)]); t = np.stack([c["members"][m]["t"] for m in (2, 7)])
    dm.st.update_poses([c["slots"][2], c["slots"][7]], R, t, np.zeros((2, 3), np.float32))
    i11 = int(np.flatnonzero(c["pos_ids"] == 11)[0])
    c["pos"][i11] = (1.5, -2.25, 7.0)
    dm.mp.set([11], c["pos"][i11])
    after = bh.host_windows(c)[1]
    assert bc.difference(before, after) is not None and bc.difference(after, dm.windows()) is None
    # ... and after the next build the row is seen as well
    dm.cv.build(c["slots"])
    c["members"][6]["mp"][0] = 12
    rebuilt = bh.host_windows(c)[1]
    assert 6 in rebuilt[0]["kf_member"].tolist() and bc.difference(rebuilt, dm.windows()) is None
    dm.close()


def test_refusals_name_their_reason_and_write_nothing(ctx, maps):
    c = bc.case("fixed_order")
    dm = maps("fixed_order")

    def refused(cv, mp, jobs, caps, word):
        o = api.ba_window_arrays(len(jobs), *[max(v, 1) for v in caps], fill=SENTINEL)
        with pytest.raises(api.CmsError, match=word):
            cv.local_ba_windows(mp, jobs, *caps, out=o)
        assert untouched(o), word
    ok = [([2, 5], -1)]
    for jobs, caps, word in (([([], -1)], c["caps"], "n_local < 1"), ([([2, 8], -1)], c["caps"], "names no member"), ([([2, -1], -1)], c["caps"], "names no member"),
                             ([([2, 5, 2], -1)], c["caps"], "twice"), ([([2, 5], 8)], c["caps"], "first_member"), ([([2, 5], -2)], c["caps"], "first_member"),
                             (ok, (0, 8, 32), "cap"), (ok, (8, 0, 32), "cap"), (ok, (8, 8, 0), "cap")):
        refused(dm.cv, dm.mp, jobs, caps, word)
    cv2 = api.Covisibility(dm.st, 8)
    refused(cv2, dm.mp, ok, c["caps"], "no index")
    cv2.close()
    other = bh.DeviceMap(ctx, bc.case("tiny"))
    refused(dm.cv, other.mp, ok, c["caps"], "different stores")
    refused(other.cv, dm.mp, [([0], -1)], c["caps"], "different stores")
    other.close()


def test_a_local_point_without_position_is_refused_with_its_job(ctx):
    c = bc.case("fixed_order")
    dm = bh.DeviceMap(ctx, c)
    dm.mp.erase([14])
    o = api.ba_window_arrays(2, *c["caps"], fill=SENTINEL)
    with pytest.raises(api.CmsError, match="job 1"):
        dm.windows(jobs=[([7], -1), ([2, 5], -1)], out=o)
    assert untouched(o)
    keep = c["pos_ids"] != 14
    hw = bh.HostWindows(c, pos_ids=c["pos_ids"][keep], pos=c["pos"][keep])
    with pytest.raises(bh.Refused, match="job 1"):
        hw.run([([7], -1), ([2, 5], -1)], c["caps"])
    hw.close()
    assert bc.difference(bh.host_windows(c, jobs=[([7], -1)])[1], dm.windows(jobs=[([7], -1)])) is None      # a job that does not touch the row is served
    dm.close()


@pytest.mark.parametrize("pinned", (False, True))
@pytest.mark.parametrize("which", (0, 1, 2))
def test_overflow_delivers_counts_and_writes_nothing_past_a_cap(maps, which, pinned):
    c = bc.case("group")
    full = bh.host_windows(c)[1]
    caps = list(c["caps"])
    caps[which] = [int(full[1]["counts"][0]) - 1, int(full[1]["counts"][2]) - 1, int(full[1]["counts"][3]) - 1][which]
    nj = len(c["jobs"])
    o = api.ba_window_arrays(nj + 1, *caps, pinned=pinned, fill=SENTINEL)      # one row more than jobs: the guard behind the last job
    with pytest.raises(api.CmsOverflow) as e:
        maps("group").windows(caps=caps, pinned=pinned, out=o)
    assert e.value.counts.tolist() == [f["counts"].tolist() for f in full]
    hw = bh.HostWindows(c)
    ho = api.ba_window_arrays(nj + 1, *caps, fill=SENTINEL)
    rc, _, _ = hw.run(c["jobs"], caps, out=ho)
    hw.close()
    assert rc == -4
    for k in ARRAYS:      # the host core's arrays hold the same prefixes, and the same sentinel bytes behind them
        assert np.array_equal(o[k].view(np.uint8), ho[k].view(np.uint8)), k
    got = bh.trim(o, nj)
    assert bc.difference([full[0], full[2]], [got[0], got[2]]) is None      # the jobs that fit are complete


@pytest.mark.parametrize("name", ("fixed_order", "waves"))
def test_mirror_device_equals_host_core(name):
    """MapPointStore::LocalBAWindow (host/cubemap_hot_path.h) through both engines"""
    c = bc.case(name)
    local, first = c["jobs"][0]
    mn = np.arange(1, len(c["members"]) + 1)
    if first >= 0:
        mn[first] = 0
    d, h = bh.mirror(0, c, local, mn_ids=mn), bh.mirror(1, c, local, mn_ids=mn)
    assert bc.difference([h], [d]) is None, bc.difference([h], [d])
    assert bc.difference(bh.host_windows(c, jobs=[(local, first)])[1], [d]) is None


def test_mirror_local_bundle_adjustment_writes_back():
    """Optimizer::LocalBundleAdjustment(mps, &window): cms_ba_run on the assembled arrays, the write-back through float into the views and the store"""
    c = bc.case("fixed_order")
    local, _ = c["jobs"][0]
    before = bh.mirror(0, c, local)
    w, n_erase, Tcw = bh.mirror(0, c, local, run_ba=True)
    assert np.array_equal(w["kf_member"], before["kf_member"]) and np.array_equal(w["e_feat"], before["e_feat"]) and 0 <= n_erase <= len(w["e_pose"])
    for k, m in enumerate(w["kf_member"]):
        moved = not np.array_equal(Tcw[m, :3, 3], c["members"][m]["t"])
        assert (not moved) if w["fixed"][k] else np.array_equal(Tcw[m, :3, 3], w["poses"][k, :3].astype(np.float32))
    assert all(np.array_equal(Tcw[m], np.vstack([np.hstack([c["members"][m]["R"], c["members"][m]["t"][:, None]]), [[0, 0, 0, 1]]]).astype(np.float32))
               for m in range(len(c["members"])) if m not in local)


def test_one_mapping_step_ends_in_a_local_ba_on_resident_data():
    """The sequence of test_one_mapping_step_on_resident_map_points (tests/test_gpu_mappoints.py) on six rendered frames, up to the refreshed table, then the
    local BA of the new key frame without a host walk: connections -> the window straight into pinned blocks -> cms_ba_create_many with
    CMS_BA_INPUTS_PINNED -> optimise -> read.  Bit for bit what the same calls make of the window the mirror's HOST_CORE engine assembles from host copies."""
    import orc
    import test_gpu_mapping_sequence as gen
    from cubemapslam_amd import synth
    F = 550
    camd = synth.camera("lafida", F)
    camd["nfeatures"] = 2000
    ocam = orc.make_camera(camd)
    scene = synth.room_scene(0xC0FFEE)
    gts = [synth.room_pose(i, 300) for i in (0, 6, 12, 18, 24, 30)]
    NK = len(gts)
    frames = np.stack([synth.render_fisheye(camd, scene, R, t) for R, t in gts])
    ctx = api.Context(camd, nfeatures=2000, max_batch=NK)
    ctx.set_mask(synth.cubemap_valid_mask(camd))
    ctx.upload(frames); ctx.process(NK, True); ctx.area_grid(NK); ctx.sync()
    g = ctx.geom
    sf = np.array([g.scale[l] for l in range(g.nlevels)], np.float32); sigma2 = (sf * sf).astype(np.float32)
    kfs, rays = [], []
    for b in range(NK):
        k, d = ctx.fetch(b)
        kfs.append(gen._kf_from_frame(k, d, gts[b][0], gts[b][1]))
        rays.append(ctx.fetch_rays(b)[:len(k)])

    def okfs():
        return [orc.make_keyframe(ocam, dict(kf)) for kf in kfs]

    def prune(pts):
        for pid, p in enumerate(pts):
            p["obs"] = [(k, f) for k, f in p["obs"] if kfs[k]["mp"][f] == pid]
    # scene set-up (oracle only): the neighbours already share map points
    oks = okfs()
    qn, q1, q2, qx = orc.create_new_map_points(ocam, oks[1][0], [q[0] for q in oks[2:]], sf, sigma2, kfs[1]["mp"].copy())
    pts = []
    for j in range(len(qn)):
        pts.append(dict(pos=qx[j].copy(), obs=[(1, int(q1[j])), (2 + int(qn[j]), int(q2[j]))]))
        kfs[1]["mp"][q1[j]] = j; kfs[2 + qn[j]]["mp"][q2[j]] = j
    prune(pts)
    nQ = len(pts)
    cg = api.Context(camd, nfeatures=2000, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=NK + 1, max_features=4096, max_nodes=1024)
    st.put_from_frames(ctx, [(b, b, len(kfs[b]["x"]), kfs[b]) for b in range(NK)])
    cv = api.Covisibility(st, NK)
    mp = api.MapPointStore(st, 8192)
    mp.set(np.arange(nQ), np.stack([p["pos"] for p in pts]), np.ones(nQ, np.int32))
    # ---- create_new_map_points -> set -> update_map_points -> build -> refresh
    gn, g1, g2, gx = st.create_new_map_points([(0, list(range(1, NK)))], cap=4096)[0]
    assert len(gn) > 100
    new = np.arange(nQ, nQ + len(gn))
    mp.set(new, gx, np.zeros(len(gn), np.int32))
    before = [kf["mp"].copy() for kf in kfs]
    for j, pid in enumerate(new):
        pts.append(dict(pos=gx[j].copy(), obs=[(0, int(g1[j])), (1 + int(gn[j]), int(g2[j]))]))
        kfs[0]["mp"][g1[j]] = pid; kfs[1 + gn[j]]["mp"][g2[j]] = pid
    prune(pts)
    trip = [(k, int(f), int(kfs[k]["mp"][f])) for k in range(NK) for f in np.flatnonzero(kfs[k]["mp"] != before[k])]
    st.update_map_points(*zip(*trip))
    cv.build(list(range(NK)))
    live = [i for i, p in enumerate(pts) if p["obs"]]
    mp.set(live, None, [sorted(pts[i]["obs"])[0][0] for i in live])
    assert (mp.refresh(cv, live) == 0).all()
    # ---- the local BA of key frame 0: lLocalKeyFrames from the index, the window from the stores
    _, order, nc = cv.connections([0], th=15)
    local = [0] + [int(v) for v in order[0, :int(nc[0])]]
    first = local[-1]      # the map's first key frame is the weakest neighbour: it stays fixed although it is local
    assert len(local) >= 3
    P_cap = sum(len(kfs[k]["x"]) for k in local)
    win = cv.local_ba_windows(mp, [(local, first)], NK, P_cap, 8 * P_cap, pinned=True)[0]
    K, nl, P, E = (int(v) for v in win["counts"])
    assert nl == len(local) and P >= 150 and E >= 2 * P - 50 and win["fixed"][nl - 1] == 1 and not win["fixed"][:nl - 1].any()
    # the same window from host copies through the mirror's HOST_CORE engine
    case = dict(members=[dict(mp=kf["mp"], oct=kf["octave"], x=kf["x"], y=kf["y"], rays=r, R=kf["R"], t=kf["t"]) for kf, r in zip(kfs, rays)], slots=list(range(NK)),
                max_points=8192, pos_ids=np.array(live, np.int32), pos=np.stack([pts[i]["pos"] for i in live]).astype(np.float32), ref=np.zeros(len(live), np.int32))
    mn = np.arange(1, NK + 1); mn[first] = 0
    mwin = bh.mirror(1, case, local, mn_ids=mn, camd=camd)
    assert bc.difference([mwin], [win]) is None, bc.difference([mwin], [win])
    f = F / 2.0
    mprob = api.pin_problem(dict(mwin, fx=f, fy=f, cx=f, cy=f))
    api.ba_set_deterministic(1)
    try:
        outs = []
        for prob in (win, mprob):
            bas = api.ba_create_many([prob])
            rc, stats = api.ba_optimize_many(bas)
            outs.append((api.ba_read_many(bas)[0], list(stats[0].iterations_done)))
            for b in bas:
                b.close()
    finally:
        api.ba_set_deterministic(0)
    (gp, gq, gf), (wp, wq, wf) = outs[0][0], outs[1][0]
    assert outs[0][1] == outs[1][1] and sum(outs[0][1]) > 0
    assert np.array_equal(gp.view(np.uint64), wp.view(np.uint64)) and np.array_equal(gq.view(np.uint64), wq.view(np.uint64)) and np.array_equal(gf, wf)
    assert not np.array_equal(gq, win["points"])      # the optimisation moved the points
    mp.close(); cv.close(); st.close(); cg.close(); ctx.close()
