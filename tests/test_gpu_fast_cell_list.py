"""A remapped batch runs FAST without the cells that hold one value in every remapped frame (cms_fast_cell_lists): key points and descriptors
stay the oracle's, with a fisheye pixel (0, 0) of 255 so that the never-written face pixels stand out against the picture and the zero
corner blocks, and through the three canvas transitions remapped -> caller canvas (every cell again) -> remapped."""
import numpy as np
import pytest
import orc
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    (gk, gd), (wk, wd) = got, want
    assert len(gk) == len(wk) and len(wk) > 50, (tag, len(gk), len(wk))
    assert np.array_equal(gk.view(np.uint8), wk.view(np.uint8)), (tag, "key points")
    assert np.array_equal(gd, wd), (tag, "descriptors")


# the issue's F = 75 (there the Lafida list happens to drop nothing: a cell is half a face wide), and two shapes whose list drops 1 and 39 cells
@pytest.mark.parametrize("name,F,n_dropped", [("lafida", 75, 0), ("front", 75, 1), ("front", 150, 39)])
def test_remapped_caller_canvas_remapped(name, F, n_dropped):
    camd = synth.camera(name, F)
    ocam = orc.make_camera(camd)
    lists = [set(zip(*(a.tolist() for a in api.fast_cells_host(camd, which, nfeatures=1000)))) for which in range(3)]
    assert len(lists[1]) - len(lists[2]) == n_dropped
    W = 3 * F
    mask = np.full((W, W), 255, np.uint8)
    fish = np.stack([synth.texture(camd["Ih"], camd["Iw"], 41 + i) for i in range(3)])
    fish[:, 0, 0] = 255
    noise = np.random.RandomState(7).randint(0, 256, size=(W // 3 + 1, W // 3 + 1)).astype(np.uint8)
    canvas = np.ascontiguousarray(np.kron(noise, np.ones((3, 3), np.uint8))[:W, :W])        # corners everywhere: corner blocks, never-written face pixels
    m1, m2 = orc.build_lut(ocam)
    o = orc.Orb(nfeatures=1000)
    cubes = [orc.fisheye_to_cubemap(ocam, m1, m2, f) for f in fish]
    # the border of the never-written region is a 255 step: strong corners right next to the cells that are left out
    assert any((c == 255).sum() > F for c in cubes)
    want = [o.extract(ocam, c, mask) for c in cubes]
    want_canvas = o.extract(ocam, canvas, mask)
    if n_dropped:
        # the caller canvas has key points inside cells the remapped list leaves out: FAST has to run there for it
        sf = o.tables()["scale"]
        hit = 0
        for (l, ci, cj) in lists[1] - lists[2]:
            w = int(np.rint(np.float64(np.float32(W) * (np.float32(1.0) / sf[l]))))
            n = int(np.float32(w - 32) / np.float32(30)); cell = int(np.ceil(np.float32(w - 32) / np.float32(n)))
            k = want_canvas[0]
            xl = k["x"] / sf[l]; yl = k["y"] / sf[l]
            hit += int(((k["octave"] == l) & (xl >= 19 + cj * cell) & (xl < 19 + (cj + 1) * cell) & (yl >= 19 + ci * cell) & (yl < 19 + (ci + 1) * cell)).sum())
        assert hit > 0
    ctx = api.Context(camd, nfeatures=1000, max_batch=2)
    ctx.set_mask(mask)
    ctx.upload(fish[:2])
    ctx.process(2, True)
    ctx.sync()
    for b in range(2):
        _same(ctx.fetch(b), want[b], "remapped batch, frame %d" % b)
    _same(ctx.extract(canvas), want_canvas, "caller canvas")
    _same(ctx.remap_extract(fish[2]), want[2], "remapped after a caller canvas")
    ctx.upload(fish[:2])
    ctx.process(2, True)
    ctx.sync()
    _same(ctx.fetch(1), want[1], "remapped batch after a caller canvas, frame 1")
    ctx.close()
