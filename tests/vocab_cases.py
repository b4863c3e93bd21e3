"""Synthetic, seeded vocabulary trees and descriptor sets for the ComputeBoW tests (the reference's ORBvoc.txt is not part of the repository: a vocabulary
is data).  A tree is a dict in the text format's terms: k, L, scoring, weighting and one entry per node with node 0 = the root -- parent (parent[i] < i),
is_leaf, desc (n x 32 uint8), weight (float64).  A child's descriptor is its parent's with a few bits flipped, so a descriptor near a leaf walks to it;
weights are random doubles, a share of the leaves has weight 0 and a few a negative one (neither enters a vector)."""
import functools

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5


def _flip(rng, desc, bits):
    """each row of desc (m x 32 uint8) with `bits` random bit positions toggled"""
    out = desc.copy()
    m = len(out)
    for _ in range(bits):
        pos = rng.integers(0, 256, m)
        out[np.arange(m), pos >> 3] ^= (1 << (pos & 7)).astype(np.uint8)
    return out


def tree(seed, k, L, scoring=L1_NORM, weighting=TF_IDF, flips=20, zero_share=0.2, leaf_share_level1=0.0, ragged=False, duplicate_siblings=False, shuffle=True,
         random_desc=False):
    """A tree of branching factor k and depth L, generated level by level.  leaf_share_level1: that share of the root's children are words themselves
    (an unbalanced tree); ragged: inner nodes have 1..k children; duplicate_siblings: the last child of every family repeats the first one's descriptor
    (a distance tie between child 0 and child k - 1); shuffle: node ids are a random order that keeps parents in front of their children (children
    order = ascending id, as the text format defines it) instead of level order; random_desc: descriptors are independent random bytes."""
    rng = np.random.default_rng(seed)
    parent = [np.zeros(1, np.int64)]; leaf = [np.zeros(1, bool)]; desc = [np.zeros((1, 32), np.uint8)]
    prev_ids = np.zeros(1, np.int64); prev_desc = rng.integers(0, 256, (1, 32)).astype(np.uint8)
    total = 1
    for level in range(1, L + 1):
        m = len(prev_ids)
        cnt = rng.integers(1, k + 1, m) if (ragged and level > 1) else np.full(m, k)
        par = np.repeat(prev_ids, cnt)
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        pos = np.arange(len(par)) - first
        d = rng.integers(0, 256, (len(par), 32)).astype(np.uint8) if (random_desc or level == 1) else _flip(rng, np.repeat(prev_desc, cnt, axis=0), flips)
        if duplicate_siblings:
            last = pos == np.repeat(cnt, cnt) - 1
            d[last] = d[first[last]]
        is_leaf = np.full(len(par), level == L)
        if level == 1 and L > 1 and leaf_share_level1 > 0:
            is_leaf |= rng.random(len(par)) < leaf_share_level1
            is_leaf[0] = True; is_leaf[-1] = False      # at least one of each
        ids = total + np.arange(len(par))
        parent.append(par); leaf.append(is_leaf); desc.append(d)
        total += len(par)
        prev_ids, prev_desc = ids[~is_leaf], d[~is_leaf]
    parent = np.concatenate(parent); leaf = np.concatenate(leaf); desc = np.concatenate(desc)
    n = len(parent)
    weight = np.where(leaf, rng.uniform(0.05, 6.0, n), rng.uniform(0.0, 1.0, n))
    u = rng.random(n)
    weight[leaf & (u < zero_share)] = 0.0
    weight[leaf & (u >= zero_share) & (u < zero_share + 0.03)] *= -1.0
    if shuffle:
        # a random order with parents first: repeatedly take a random node among those whose parent is placed
        children = [[] for _ in range(n)]
        for i in range(1, n):
            children[parent[i]].append(i)
        order = [0]; avail = list(children[0])
        while avail:
            j = int(rng.integers(0, len(avail)))
            avail[j], avail[-1] = avail[-1], avail[j]
            x = avail.pop()
            order.append(x); avail.extend(children[x])
        order = np.array(order); new_of = np.empty(n, np.int64); new_of[order] = np.arange(n)
        parent = new_of[parent[order]]; parent[0] = 0
        leaf, desc, weight = leaf[order], desc[order], weight[order]
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=parent.astype(np.int32), is_leaf=leaf.astype(np.uint8), desc=np.ascontiguousarray(desc),
                weight=np.ascontiguousarray(weight, np.float64))


def with_weights(t, **kw):
    o = dict(t)
    o.update(kw)
    return o


def all_stopped(t):
    """the same tree with every word's weight <= 0: both vectors of every transform are empty"""
    w = t["weight"].copy()
    w[t["is_leaf"] != 0] = np.where(np.arange(int((t["is_leaf"] != 0).sum())) % 2 == 0, 0.0, -1.5)
    return with_weights(t, weight=w)


def descriptors(seed, t, n, near=0.8, flips=12):
    """n descriptors: a share `near` of them a random leaf's descriptor with a few bits flipped, the rest random bytes"""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(t["is_leaf"])
    d = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    if n:
        pick = rng.random(n) < near
        src = t["desc"][leaves[rng.integers(0, len(leaves), n)]]
        d[pick] = _flip(rng, src, flips)[pick]
    return np.ascontiguousarray(d)


def word_ids(t):
    """node -> word id (leaves in node order), -1 for inner nodes"""
    w = np.full(len(t["parent"]), -1, np.int64)
    lv = np.flatnonzero(t["is_leaf"])
    w[lv] = np.arange(len(lv))
    return w


def text(t):
    """the tree in the reference's text format (saveToTextFile): weights in the stream's default format, 6 significant digits"""
    lines = ["%d %d  %d %d" % (t["k"], t["L"], t["scoring"], t["weighting"])]
    for i in range(1, len(t["parent"])):
        lines.append("%d %d %s  %s" % (t["parent"][i], 1 if t["is_leaf"][i] else 0, " ".join(str(int(v)) for v in t["desc"][i]), "%g" % t["weight"][i]))
    return "\n".join(lines) + "\n"


NS = (0, 1, 63, 64, 65, 257, 2000)      # below, at and above a workgroup's 16 / 8 features and the build kernel's 256-key floor; one typical frame

# name -> (tree arguments, feature counts, levelsup values).  The smallest shapes at which each mechanism can go wrong.
CASES = {
    # lane groups: both sides of the 16-lane group and the format's maximum; ragged families leave lanes of a group without a child
    "k2_L1": (dict(seed=102, k=2, L=1), NS, (1,)),
    "k3_L2": (dict(seed=103, k=3, L=2, ragged=True), NS, (1,)),
    "k10_L3": (dict(seed=110, k=10, L=3), NS, (1,)),
    "k16_L2": (dict(seed=116, k=16, L=2), NS, (1,)),
    "k17_L2": (dict(seed=117, k=17, L=2, ragged=True), NS, (1,)),
    "k20_L2": (dict(seed=120, k=20, L=2), NS, (0,)),
    # distance ties: child k - 1 repeats child 0's descriptor (level order, so the positions are exact), child 0 must win
    "ties": (dict(seed=7, k=10, L=3, duplicate_siblings=True, shuffle=False), (257,), (1,)),
    # leaves at level 1 under L = 3: the nid level at, above and below the leaf, and L - levelsup <= 0
    "unbalanced": (dict(seed=8, k=6, L=3, leaf_share_level1=0.5), (257,), (0, 1, 2, 3, 4)),
    # the four weightings with L1, then L2 and the scoring that does not normalise (TF: the division by v.size())
    "tf_idf_l1": (dict(seed=9, k=5, L=3, weighting=TF_IDF), (257,), (1,)),
    "tf_l1": (dict(seed=9, k=5, L=3, weighting=TF), (257,), (1,)),
    "idf_l1": (dict(seed=9, k=5, L=3, weighting=IDF), (257,), (1,)),
    "binary_l1": (dict(seed=9, k=5, L=3, weighting=BINARY), (257,), (1,)),
    "tf_idf_l2": (dict(seed=9, k=5, L=3, weighting=TF_IDF, scoring=L2_NORM), (257,), (1,)),
    "tf_dot": (dict(seed=9, k=5, L=3, weighting=TF, scoring=DOT_PRODUCT), (257,), (1,)),
    "binary_dot": (dict(seed=9, k=5, L=3, weighting=BINARY, scoring=DOT_PRODUCT), (257,), (1,)),
}


@functools.lru_cache(maxsize=None)
def case_tree(name):
    if name == "all_stopped":
        return all_stopped(case_tree("k10_L3"))
    if name == "full_size":
        # ORBvoc.txt's shape: k = 10, L = 6, complete (1 111 111 nodes), random descriptors, level order
        return tree(11, 10, 6, shuffle=False, random_desc=True)
    return tree(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def case_descriptors(name, n):
    t = case_tree(name)
    if name == "ties":
        # descriptors AT the duplicated children: the tie is exact at every level
        rng = np.random.default_rng(5)
        lv = np.flatnonzero(t["is_leaf"])
        return np.ascontiguousarray(t["desc"][lv[rng.integers(0, len(lv), n)]])
    return descriptors(1000 + n, t, n)


def repeated_descriptor(name="k10_L3", copies=300):
    """`copies` times one descriptor whose word is not stopped: one word with the repeated-addition value, one node listing every feature"""
    t = case_tree(name)
    lv = np.flatnonzero((t["is_leaf"] != 0) & (t["weight"] > 0))
    return np.ascontiguousarray(np.repeat(t["desc"][lv[len(lv) // 2]][None, :], copies, axis=0))
