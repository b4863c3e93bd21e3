"""Covisibility on the device (cms_covis_create / build / votes / connections / culling / local_points, cms_kfstore_update_map_points) against the
host build of csrc/cms_covis_core.h (hm_covis_*), which tests/test_covis_cpu.py holds against a literal restatement of the reference.  Every
comparison is exact: counts, lists and flags.  The cases are tests/covis_cases.py's: a store of 64 slots with max_features 256, one of 48 slots with
max_features 2048 for the case with more than 65 536 observations, and one of 8 400 slots with max_features 8 for the case with many members."""
import numpy as np
import pytest

import covis_cases as cc
import covis_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

F = 150


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1)      # the frame thread's context: its stream is not the store's
    yield c
    c.close()


@pytest.fixture(scope="module")
def cg():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1)      # the mapping side's context
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx, cg):
    st = api.KeyframeStore(cg, max_keyframes=cc.K, max_features=cc.MAXF, max_nodes=8)
    b = hl.DeviceBackend(st, ctx, cc.K)
    yield b
    b.close(); st.close()


_host = {}


def host_expected(name):
    """the host core's results of a case, computed once"""
    if name not in _host:
        c = cc.case(name)
        h = hl.HostBackend(c["K"], c["maxf"])
        _host[name] = cc.run(c, h)
        h.close()
    return _host[name]


@pytest.mark.parametrize("name", cc.SMALL)
def test_device_equals_host_core(dev, name):
    want = host_expected(name)
    got = cc.run(cc.case(name), dev)
    assert cc.first_difference(want, got) is None, cc.first_difference(want, got)
    assert cc.first_difference(cc.expected(name), got) is None      # ... and so the restatement of the reference


@pytest.mark.parametrize("name", ["large40x2048", "wide8400x8"])
def test_large_cases(ctx, cg, name):
    """40 members x 2048 features, more than 65 536 observations: several workgroups per build kernel, nothing packed into 16 bits.  8 400 members x 8
    features: the strides over members, more than 64 KB of LDS in `connections`, more than 1 024 candidates to rank"""
    c = cc.case(name)
    st = api.KeyframeStore(cg, max_keyframes=c["K"], max_features=c["maxf"], max_nodes=8)
    b = hl.DeviceBackend(st, ctx, len(c["slots"]))
    try:
        got = cc.run(c, b)
        want = host_expected(name)
        assert cc.first_difference(want, got) is None, cc.first_difference(want, got)
        assert cc.first_difference(cc.expected(name), got) is None
    finally:
        b.close(); st.close()


def _load_pair(dev):
    """the `known3` table on the device and on the host core"""
    c = cc.case("known3")
    h = hl.HostBackend(c["K"], c["maxf"])
    assert h.load(c) == 0 and dev.load(c) == 0
    return c, h


def _same(dev, h, members=(0, 1, 2)):
    q = [dev.connections(list(members), 1), dev.culling([list(members)], [[1] * len(members)], 1), dev.local_points([list(members)], 16), dev.votes([[10, 13, 77, 14]])]
    w = [h.connections(list(members), 1), h.culling([list(members)], [[1] * len(members)], 1), h.local_points([list(members)], 16), h.votes([[10, 13, 77, 14]])]
    return cc.first_difference(w, q)


def test_a_build_sees_updates_and_nothing_before(dev):
    c, h = _load_pair(dev)
    s0, s1, s2 = c["slots"]
    before = dev.connections([0, 1, 2], 1)
    # a full-row update of member 2 and a sparse update of members 0 and 1: the index answers from its snapshot until the next build
    row2 = np.array([14, 11, 12], np.int32)
    dev.st.update(s2, mp=row2); assert h.put(s2, row2, c["octs"][2]) == 0
    dev.st.update_map_points([s0, s1], [4, 0], [77, -1]); assert h.update_map_points([s0, s1], [4, 0], [77, -1]) == 0
    assert cc.first_difference([before], [dev.connections([0, 1, 2], 1)]) is None
    assert _same(dev, h) is None
    dev.cv.build(c["slots"]); assert h.build(c["slots"]) == 0
    after = dev.connections([0, 1, 2], 1)
    assert cc.first_difference([before], [after]) is not None
    assert after[0].tolist() == [[0, 2, 2], [2, 0, 2], [2, 2, 0]]      # 0 = {10..13, 77}, 1 = {12, 13, 14}, 2 = {14, 11, 12}
    assert _same(dev, h) is None
    h.close()


def test_update_map_points_equals_the_full_row_update(dev):
    rng = np.random.default_rng(3)
    rows = [rng.integers(-1, 1 << 30, n).astype(np.int32) for n in (200, 256, 1)]
    slots = [60, 61, 62]
    for s, r in zip(slots, rows):
        dev.put(s, r, np.zeros(len(r), np.int32))
    new = [r.copy() for r in rows]
    trip = []
    for k, (s, r) in enumerate(zip(slots, new)):
        for f in rng.choice(len(r), min(len(r), 37), replace=False):
            r[f] = int(rng.integers(-1, 1 << 30)); trip.append((s, int(f), int(r[f])))
    order = rng.permutation(len(trip))
    dev.st.update_map_points([trip[i][0] for i in order], [trip[i][1] for i in order], [trip[i][2] for i in order])
    sparse = [dev.st.debug_fetch(s)["mp"].copy() for s in slots]
    for s, r in zip(slots, rows):
        dev.st.update(s, mp=r)                       # back to the old rows, then the new ones by the full-row update
    for s, r in zip(slots, new):
        dev.st.update(s, mp=r)
    for s, r, got in zip(slots, new, sparse):
        assert np.array_equal(dev.st.debug_fetch(s)["mp"], r) and np.array_equal(got, r)
    dev.st.update_map_points([], [], [])
    for bad in (([60, 60], [3, 3], [1, 2]), ([60], [200], [1]), ([63], [0], [1]), ([60], [0], [1 << 30]), ([60], [0], [-2]), ([64], [0], [1])):
        with pytest.raises(api.CmsError):
            dev.st.update_map_points(*bad)
    for s, r in zip(slots, new):
        assert np.array_equal(dev.st.debug_fetch(s)["mp"], r)      # a refused call writes nothing


def test_votes_on_the_frame_stream_right_after_a_build(dev, ctx):
    """the build runs on the store's stream, the votes on the frame context's: the wait between them is on the device, no host wait in between"""
    c = cc.case("random12x200")
    h = hl.HostBackend(c["K"], c["maxf"])
    assert h.load(c) == 0 and dev.load(c) == 0
    frames = c["queries"][0][1]
    members = list(range(len(c["slots"])))
    for rnd in range(3):
        sub = members[rnd:] + members[:rnd]      # another member order: stale votes would sit in other columns
        slots = [c["slots"][m] for m in sub]
        dev.cv.build(slots); got = dev.votes(frames); lp = dev.local_points([[0, 1, 2]], 600)
        assert h.build(slots) == 0
        assert np.array_equal(got, h.votes(frames)) and got.sum() > 0
        assert cc.first_difference([h.local_points([[0, 1, 2]], 600)], [lp]) is None
    h.close()


def test_the_index_is_unchanged_after_culling(dev):
    c = cc.case("cascade")
    assert dev.load(c) == 0
    before = (dev.connections([0, 1, 2, 3, 4], 1), dev.votes([list(range(1000, 1040)) + [2000, 2001]]), dev.local_points([[4, 1]], 128))
    first = dev.culling([[0, 1, 4]], [[1, 1, 1]], 3)
    assert first[2].tolist() == [1, 0, 1] and first[0].tolist() == [43, 60, 21]      # members left the chain's scratch state, points became bad
    after = (dev.connections([0, 1, 2, 3, 4], 1), dev.votes([list(range(1000, 1040)) + [2000, 2001]]), dev.local_points([[4, 1]], 128))
    assert cc.first_difference(list(before), list(after)) is None
    assert cc.first_difference([first], [dev.culling([[0, 1, 4]], [[1, 1, 1]], 3)]) is None
    # ... nor is the call's scratch: the same handle answers another chain, and then three chains, as a fresh one would
    kept = dev.culling([[0, 1, 4]], [[0, 1, 1]], 3)
    assert kept[0].tolist() == [43, 63, 21] and kept[2].tolist() == [1, 1, 0]
    three = dev.culling([[0, 1, 4], [0, 1, 4], [1, 0]], [[1, 1, 1], [0, 0, 0], [1, 1]], 3)
    assert cc.first_difference([cc.expected("cascade")[2]], [three]) is None


def test_refusals(dev, ctx):
    c, h = _load_pair(dev)
    h.close()
    before = dev.connections([0, 1, 2], 1)
    dev.put(50, [5, 9, 5], [0, 0, 0])
    for slots in ([c["slots"][0], 50], [c["slots"][0], 51], [c["slots"][0], c["slots"][1], c["slots"][0]], [c["slots"][0], 64], [-1]):
        with pytest.raises(api.CmsError):
            dev.cv.build(slots)                      # an id twice in a row, an empty slot, a slot twice, no such slot
    assert cc.first_difference([before], [dev.connections([0, 1, 2], 1)]) is None      # the previous index stays
    with pytest.raises(api.CmsError):
        dev.votes([[10, -3]])
    with pytest.raises(api.CmsError):
        dev.votes([[10, 1 << 31]])                   # not a 32-bit int: refused before it could wrap
    with pytest.raises(api.CmsError):
        dev.connections([3], 1)
    with pytest.raises(api.CmsError):
        dev.culling([[0, 1, 0]], [[1, 1, 1]], 3)     # a member twice in a chain
    with pytest.raises(api.CmsError):
        dev.local_points([[0, 0]], 8)
    with pytest.raises(api.CmsError):
        api.Covisibility(dev.st, 16385)
    fresh = api.Covisibility(dev.st, 4)
    with pytest.raises(api.CmsError):
        fresh.connections([0], 1)                    # no index yet
    with pytest.raises(api.CmsError):
        fresh.build([c["slots"][0], c["slots"][1], c["slots"][2], 50, 60])      # more than max_members
    fresh.build([])
    assert fresh.votes(ctx, [[1, 2]]).shape == (1, 0)
    fresh.close()


def test_mirror_device_equals_host_core():
    """CubemapSLAM::Covisibility (host/cubemap_hot_path.h) through both engines on the random table: UpdateConnections, KeyFrameCulling,
    UpdateLocalKeyFrames and UpdateLocalPoints give the same key frames, weights, counters and ids"""
    c = cc.case("random12x200")
    frames = c["queries"][0][1]
    args = (c["rows"], c["octs"], [0, 5, 11], list(range(11, -1, -1)), [1, 0] * 6, frames[0], [7, 2, 9])
    d, h = hl.mirror(0, *args), hl.mirror(1, *args)
    assert cc.first_difference([h], [d]) is None
    e = cc.expected("random12x200")
    assert h[0] == [int(v) for j in (0, 5, 11) for v in e[1][1][j][:e[1][2][j]]]      # the ordered connections of the restatement
