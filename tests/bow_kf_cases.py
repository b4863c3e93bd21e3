"""Cases for ORBMatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (src/ORBMatcher.cpp:541-674): hand-built known answers and seeded key-frame pairs,
shared by test_search_by_bow_kf_cpu.py (the restatement alone) and test_gpu_search_by_bow_kf.py (the device entry against the restatement).

A case is a dict: kf1 / kf2 = dict(angle, desc, mp (>= 0: the feature holds a map point), node_id, node_off, node_feat), bad1 / bad2 (uint8 per
feature or None), nnratio, ori.  Hand-built cases carry `idx2` and `n`, written out by hand."""
import functools

import numpy as np

import npref_bow_kf
from cubemapslam_amd import synth
from test_search_by_bow_cpu import desc_at, fv as _fv_csr


def fv(nodes):
    """{node id: [features]} -> CSR dict"""
    return dict(zip(("node_id", "node_off", "node_feat"), _fv_csr(nodes)))


def _side(desc, nodes, angle, has_mp):
    n = len(desc)
    mp = np.where(np.ones(n, bool) if has_mp is None else np.asarray(has_mp, bool), 100 + np.arange(n), -1).astype(np.int32)
    return dict(angle=np.zeros(n, np.float32) if angle is None else np.asarray(angle, np.float32), desc=desc, mp=mp, **fv(nodes))


def hand(name, n1, rows2, fv1, fv2, idx2, n, angle1=None, angle2=None, mp1=None, mp2=None, bad1=None, bad2=None, nnratio=0.75, ori=False):
    """key frame 1: n1 features, all with the zero descriptor; key frame 2: feature i at Hamming distance rows2[i] from zero, so the distance of any
    pair is rows2[i2]"""
    d2 = np.stack([desc_at(d, 7 * i) for i, d in enumerate(rows2)])
    u8 = lambda a: None if a is None else np.asarray(a, np.uint8)
    return dict(name=name, kf1=_side(np.zeros((n1, 32), np.uint8), fv1, angle1, mp1), kf2=_side(d2, fv2, angle2, mp2), bad1=u8(bad1), bad2=u8(bad2),
                nnratio=nnratio, ori=ori, idx2=list(idx2), n=n)


_ONE = {1: [0]}
_SEP12 = {i: [i] for i in range(12)}
HAND = [
    # 1. TH_LOW is strict here: 50 is rejected (the (KeyFrame, Frame) overload accepts it), 49 is accepted
    hand("dist_50_rejected", 1, [50], _ONE, _ONE, [-1], 0),
    hand("dist_49_accepted", 1, [49], _ONE, _ONE, [0], 1),
    # 2. the nearest key-frame-2 feature has no map point / a bad one: ignored, the next one (30 < 0.75 * 256) is taken
    hand("nearest_without_map_point", 1, [10, 30], _ONE, {1: [0, 1]}, [1], 1, mp2=[False, True]),
    hand("nearest_bad", 1, [10, 30], _ONE, {1: [0, 1]}, [1], 1, bad2=[1, 0]),
    # 3. 20 against a second nearest of 22 fails the ratio test; with the 22 filtered the second nearest is 40: 20 < 30
    hand("second_nearest_filtered", 1, [20, 22, 40], _ONE, {1: [0, 1, 2]}, [0], 1, mp2=[True, False, True]),
    hand("second_nearest_present", 1, [20, 22, 40], _ONE, {1: [0, 1, 2]}, [-1], 0),
    # 4. two candidates at the same distance: the second becomes bestDist2, 20 < 0.75 * 20 fails
    hand("tie", 1, [20, 20], _ONE, {1: [0, 1]}, [-1], 0),
    # 5. node 5 lists key frame 1's features as [1, 0]: feature 1 is first and takes key-frame-2 feature 0 (10), feature 0 then takes feature 1 (30, alone);
    #    node 9: feature 2 takes 2 (10), feature 3 is left with 3 (60 >= 50): none
    hand("taken_feature", 4, [10, 30, 10, 60], {5: [1, 0], 9: [2, 3]}, {5: [0, 1], 9: [2, 3]}, [1, 0, 2, -1], 3),
    # 6. nodes 1 and 7 are in key frame 1 only, 2 and 9 in key frame 2 only: node 4 alone takes part
    hand("node_on_one_side", 3, [10, 10, 10], {1: [0], 4: [1], 7: [2]}, {2: [0], 4: [1], 9: [2]}, [-1, 1, -1], 1),
    hand("empty_vector_2", 1, [10], {3: [0]}, {}, [-1], 0),
    hand("empty_vector_1", 1, [10], {}, {3: [0]}, [-1], 0),
    # 7. 11 matches in bin 0 and one in bin 10 (angle1 - angle2 = 120): 1 < 0.1 * 11, the bin is dropped and nmatches follows
    hand("histogram_removes", 12, [10] * 12, _SEP12, _SEP12, list(range(11)) + [-1], 11, angle1=[130.0] * 11 + [250.0], angle2=[130.0] * 12, ori=True),
    hand("histogram_off", 12, [10] * 12, _SEP12, _SEP12, list(range(12)), 12, angle1=[130.0] * 11 + [250.0], angle2=[130.0] * 12, ori=False),
    # (the histogram is over angle1 - angle2: 12 -> bin 1 and 6 -> 0.5 -> bin 1, all kept; angle2 - angle1 would give 348 -> bin 29 and 354 -> 29.5 -> bin 30 = 0,
    #  a bin of one next to a bin of 11, dropped)
    hand("histogram_sign", 12, [10] * 12, _SEP12, _SEP12, list(range(12)), 12, angle1=[12.0] * 11 + [6.0], angle2=[0.0] * 12, ori=True),
    # 8. float32(0.8) * 30.0f is 24.0f exactly (the product 24.00000036 rounds down): 24 < 24 fails.  In double, or with the multiply fused into the
    #    comparison, 24 < 24.00000036 would pass
    hand("ratio_unfused_float", 1, [24, 30], _ONE, {1: [0, 1]}, [-1], 0, nnratio=0.8),
    hand("ratio_below", 1, [23, 30], _ONE, {1: [0, 1]}, [0], 1, nnratio=0.8),
    # 9. malformed vectors under the feat_node rule.  Key frame 1 lists feature 0 in nodes 3 and 5: the store records node 5, where it takes
    #    key-frame-2 feature 1.  Key frame 2 lists feature 2 in nodes 7 and 8: it is a candidate in node 8 only, so key frame 1's feature 1 (node 7)
    #    finds nothing and feature 2 (node 8) takes it.  (The reference as it stands gives [1, 2, -1] with nmatches 3.)
    hand("listed_twice_across_nodes", 3, [10, 12, 14], {3: [0], 5: [0], 7: [1], 8: [2]}, {3: [0], 5: [1], 7: [2], 8: [2]}, [1, -1, 2], 2),
    #    listed twice in one node: key frame 1's feature is matched once; key frame 2's feature ties with itself
    hand("listed_twice_in_a_node_1", 1, [10, 30], {3: [0, 0]}, {3: [0, 1]}, [0], 1),
    hand("listed_twice_in_a_node_2", 1, [10], {3: [0]}, {3: [0, 0]}, [-1], 0),
]


def _fv_of(desc, kind):
    """FeatureVector stand-in (DBoW2 is the host's): features binned by descriptor bits, a node's features in feature order.  coarse: 16 nodes (more
    than 64 features each), fine: up to 1024 nodes, many: up to 2048 nodes of one or two features"""
    n = len(desc)
    b0, b1 = desc[:, 0].astype(np.int32), desc[:, 1].astype(np.int32)
    node = {"coarse": b0 >> 4, "fine": (b0 * 4 + (b1 >> 6)) % 1024, "many": b0 * 8 + (b1 >> 5)}[kind]
    order = np.lexsort((np.arange(n), node))
    ids, starts = np.unique(node[order], return_index=True)
    return dict(node_id=ids.astype(np.int32), node_off=np.concatenate([starts, [n]]).astype(np.int32), node_feat=order.astype(np.int32))


@functools.lru_cache(maxsize=None)
def seeded_pair(kind):
    """two key frames of synth.keyframe_set looking at one scene: 40 % of the map-point slots empty and 10 % bad flags on each side; one angle per scene
    point plus noise, so that the histogram keeps the true matches and drops most of the false ones"""
    ks = synth.keyframe_set(550, n_kf=2, n_pts=2600, seed=61)
    rng = np.random.default_rng(7)
    sides, bads = [], []
    for k in ks["kfs"]:
        n = len(k["x"])
        ang = (((k["point"] * 37) % 360).astype(np.float32) + rng.normal(0, 5, n).astype(np.float32)) % np.float32(360)
        mp = np.where(rng.random(n) < 0.6, 1000 + np.arange(n), -1).astype(np.int32)
        sides.append(dict(angle=ang.astype(np.float32), desc=np.ascontiguousarray(k["desc"]), mp=mp, x=k["x"], y=k["y"], octave=k["octave"], **_fv_of(k["desc"], kind)))
        bads.append((rng.random(n) < 0.1).astype(np.uint8))
    return sides[0], sides[1], bads[0], bads[1]


SEEDED = [(kind, nnratio, ori) for kind in ("coarse", "fine", "many") for nnratio in (0.75, 0.7) for ori in (True, False)]


def seeded(kind, nnratio, ori):
    kf1, kf2, bad1, bad2 = seeded_pair(kind)
    return dict(name="%s_%g_%d" % (kind, nnratio, ori), kf1=kf1, kf2=kf2, bad1=bad1, bad2=bad2, nnratio=nnratio, ori=ori)


def restate(c, feat_node=True):
    """the restatement's (idx2, nmatches) for a case; feat_node=False: the reference as it stands (no rule for malformed vectors)"""
    k1, k2 = c["kf1"], c["kf2"]
    fn1 = npref_bow_kf.feat_node_of(k1, len(k1["mp"])) if feat_node else None
    fn2 = npref_bow_kf.feat_node_of(k2, len(k2["mp"])) if feat_node else None
    return npref_bow_kf.search_by_bow_kf(k1["angle"], k1["desc"], k1["mp"] >= 0, c["bad1"], k1, k2["angle"], k2["desc"], k2["mp"] >= 0, c["bad2"], k2,
                                         c["nnratio"], c["ori"], fn1, fn2)


@functools.lru_cache(maxsize=None)
def seeded_reference(kind, nnratio, ori):
    """computed once per session and shared; callers do not write into it"""
    idx2, n = restate(seeded(kind, nnratio, ori))
    idx2.setflags(write=False)
    return idx2, n
