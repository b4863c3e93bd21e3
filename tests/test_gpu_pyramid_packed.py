"""k_resize with the compact tap addressing (fixed LDS row stride, the second source row at an immediate offset, first / last source row staged
twice instead of a clamp per pixel, the right tap of the last column read with weight 0): every level byte for byte against orc.resize
applied level by level, through the remapped path (zero-corner tiles are skipped) and through a caller canvas of random bytes (no skip: the
row and column clamps see non-zero data on all four sides)."""
import numpy as np
import pytest
import orc
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

# F, levels, scale.  The first three are the shapes the change was specified with (level widths 225 .. 63: one x-tile, the last level just above
# the 62-pixel minimum; tap spacing 1.5; W = 258).  None of their RESIZED levels is wider than 256, so two more reach the second x-tile of a
# destination row: 312 -> 260 (a four-pixel tile at xb = 256, spacing 1.2), 387 -> 258 (a two-pixel one, spacing 1.5) and 309 -> 258
# (a two-pixel one, spacing 1.2).
SHAPES = [(75, 8, 1.2), (100, 4, 1.5), (86, 3, 1.2), (104, 3, 1.2), (129, 3, 1.5), (103, 2, 1.2)]


def _oracle_levels(img, widths):
    out = [img]
    for w in widths[1:]:
        out.append(orc.resize(out[-1], w, w))
    return out


def _check(ctx, b, want, tag):
    for l, w in enumerate(want):
        got = ctx.debug_level(b, l)
        assert got.shape == w.shape, (tag, l, got.shape, w.shape)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, (tag, "level %d: %d differing pixels, first at (y, x) = %s" % (l, len(bad), bad[:4].tolist()))


@pytest.mark.parametrize("F,levels,scale", SHAPES)
def test_every_level_equals_the_oracles(F, levels, scale):
    camd = synth.camera("lafida", F)
    ocam = orc.make_camera(camd)
    ctx = api.Context(camd, nfeatures=300, scale_factor=scale, nlevels=levels, max_batch=2)
    widths = [ctx.geom.level_w[l] for l in range(levels)]
    assert widths[0] == 3 * F and all(ctx.geom.level_h[l] == widths[l] for l in range(levels))
    if F in (104, 129, 103):
        assert 256 < widths[1] <= 260
    # remapped: two frames, corner tiles skipped
    fish = np.stack([synth.texture(camd["Ih"], camd["Iw"], 61), np.random.RandomState(62).randint(0, 256, size=(camd["Ih"], camd["Iw"])).astype(np.uint8)])
    m1, m2 = orc.build_lut(ocam)
    ctx.upload(fish)
    ctx.process(2, True)
    ctx.sync()
    for b in range(2):
        _check(ctx, b, _oracle_levels(orc.fisheye_to_cubemap(ocam, m1, m2, fish[b]), widths), "remapped frame %d" % b)
    # caller canvas: random bytes everywhere, extremes in the first / last rows and columns
    canvas = np.random.RandomState(63).randint(0, 256, size=(3 * F, 3 * F)).astype(np.uint8)
    canvas[0, ::2] = 255; canvas[-1, 1::2] = 255; canvas[::2, 0] = 255; canvas[1::2, -1] = 255
    ctx.extract(canvas)
    _check(ctx, 0, _oracle_levels(canvas, widths), "caller canvas")
    # ... and back: the remapped batch behind it rewrites the corner blocks and every level
    ctx.process(2, True)
    ctx.sync()
    _check(ctx, 0, _oracle_levels(orc.fisheye_to_cubemap(ocam, m1, m2, fish[0]), widths), "remapped after a caller canvas")
    ctx.close()
