"""k_describe evaluates the column pass of the 7 x 7 Gaussian only at the 512 positions steered BRIEF samples, straight from the row sums.
Descriptors and angles against the oracle's extractor, 0 differing bits, under both definitions of the Gaussian; the inputs are checked to
hold the two situations the per-sample evaluation can get wrong: a patch that crosses the level edge (REFLECT_101 staging) and samples on
both sides of the SSE2 column limit width & ~3."""
import os
import re

import numpy as np
import pytest
import orc
from cubemapslam_amd import api, synth
from oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

F = 75
PR = 21      # half width of the staged patch: 18 (farthest sample) + 3 (blur taps)


def _pattern():
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "orb_pattern.inc")).read()
    body = src[src.index("{") + 1:src.index("}")]
    return np.array([int(t) for t in re.findall(r"-?\d+", body)], np.float64).reshape(512, 2)


def _inputs(camd):
    """(fisheye frames for the remapped path, caller canvases): a texture, and dense noise smoothed a little so that FAST fires everywhere,
    up to the border the extractor allows (19 pixels from the level edge)"""
    fish = np.stack([synth.texture(camd["Ih"], camd["Iw"], 31), synth.texture(camd["Ih"], camd["Iw"], 32)])
    W = 3 * F
    canv = []
    for seed in (5, 6):
        n = np.random.RandomState(seed).randint(0, 256, size=(W // 3 + 2, W // 3 + 2)).astype(np.uint8)
        canv.append(np.ascontiguousarray(np.kron(n, np.ones((3, 3), np.uint8))[1:W + 1, 2:W + 2]))
    return fish, canv


@pytest.fixture(scope="module")
def cases():
    camd = synth.camera("lafida", F)
    fish, canv = _inputs(camd)
    mask = np.full((3 * F, 3 * F), 255, np.uint8)
    want = {}
    for mode in (0, 1):
        ob = OracleBackend(dict(camd, nfeatures=2000), mask, gaussian_mode=mode)
        rows = [ob.extract(f, False) for f in fish]
        rows += [ob.orb_trk.extract(ob.cam, c, mask) for c in canv]
        want[mode] = rows
    return camd, fish, canv, mask, want, OracleBackend(dict(camd, nfeatures=2000), mask).sf


def test_inputs_hold_edge_patches_and_both_sides_of_the_sse2_limit(cases):
    camd, fish, canv, mask, want, sf = cases
    pat = _pattern()
    ws = [int(np.rint(np.float64(np.float32(3 * F) * (np.float32(1.0) / s)))) for s in sf]
    assert any(w % 4 for w in ws)
    n_edge = n_left = n_right = 0
    for k, _ in want[1]:
        lvl = k["octave"].astype(int)
        xl = np.rint(k["x"].astype(np.float64) / sf[lvl]).astype(int); yl = np.rint(k["y"].astype(np.float64) / sf[lvl]).astype(int)
        w = np.array(ws)[lvl]
        n_edge += int(((xl < PR) | (yl < PR) | (xl + PR >= w) | (yl + PR >= w)).sum())
        # columns the steered samples of key points near the right edge land in, against width & ~3 (levels whose width is no multiple of 4)
        for i in np.nonzero((w % 4 != 0) & (xl + 18 >= (w & ~3)))[0]:
            a = np.deg2rad(np.float64(k["angle"][i]))
            fx = pat[:, 0] * np.cos(a) - pat[:, 1] * np.sin(a)
            sure = np.abs(fx - np.floor(fx) - 0.5) > 0.01          # away from a rounding tie: the column is certain
            col = xl[i] + np.rint(fx[sure]).astype(int)
            n_right += int((col >= (w[i] & ~3)).sum()); n_left += int((col < (w[i] & ~3)).sum())
    print("edge patches %d, samples left / right of the limit %d / %d" % (n_edge, n_left, n_right))
    assert n_edge > 20 and n_right > 0 and n_left > 0, (n_edge, n_left, n_right)


@pytest.mark.parametrize("mode", [0, 1])
def test_descriptors_and_angles_equal_the_oracles(cases, mode):
    camd, fish, canv, mask, want, sf = cases
    ctx = api.Context(camd, nfeatures=2000, max_batch=len(fish))
    ctx.set_mask(mask)
    if mode:
        ctx.set_gaussian_mode(mode)
    ctx.upload(fish)
    ctx.process(len(fish), True)
    ctx.sync()
    got = [ctx.fetch(b) for b in range(len(fish))] + [ctx.extract(c) for c in canv]
    ctx.close()
    for j, ((gk, gd), (wk, wd)) in enumerate(zip(got, want[mode])):
        assert len(gk) == len(wk) and len(wk) > 100, (j, len(gk), len(wk))
        assert np.array_equal(gk.view(np.uint8), wk.view(np.uint8)), (j, "key points / angle bits")
        nbits = int(np.unpackbits(gd ^ wd).sum())
        print("input %d, Gaussian mode %d: %d key points, %d differing descriptor bits" % (j, mode, len(wk), nbits))
        assert nbits == 0, (j, mode, nbits)
