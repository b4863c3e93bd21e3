"""The remap's 2-D tile table (cubemapslam_amd/csrc/cms_remap_tiles.h), checked on the host through cms_remap_lut_host /
cms_remap_tiles_host: no GPU.  The kernel reads the four taps X .. X + 1, Y .. Y + 1 of every written LUT entry from the tile's staged
source rectangle, so every such tap must lie inside it unless the tile is flagged for direct gathers; cells the reference never
writes (LUT entry 0) get the frame's pixel (0, 0) and must not stretch a rectangle to the image origin."""
import numpy as np
import pytest
from cubemapslam_amd import api, build, synth

CAMERAS = [("lafida", 550, None), ("lafida", 450, None), ("front", 650, None), ("front", 650, 1024), ("lafida", 120, None)]
SHAPES = [(32, 32), (64, 16), (128, 8)]


def _cross(F):
    m = np.zeros((3 * F, 3 * F), bool)
    for (ox, oy) in synth._FACE_ORIGIN.values():
        m[oy * F:(oy + 1) * F, ox * F:(ox + 1) * F] = True
    return m


def _table(name, F, Ih, tw, th, budget=api.RT_LDS_MAX):
    build.build(verbose=False)
    camd = synth.camera(name, F, Ih)
    lut = api.remap_lut_host(camd)
    tiles, n_live, lds = api.remap_tiles_host(camd, lut, tw, th, budget)
    return camd, lut, tiles, n_live, lds


def _tile_extents(lut, written, tw, th):
    """per tile (ty, tx): min X, max X + 1, min Y, max Y + 1 over the written cross entries (np.nan-free: masked with sentinels)"""
    W = lut.shape[0]
    nty, ntx = -(-W // th), -(-W // tw)
    X = (lut & 0x7FF).astype(np.int64); Y = ((lut >> 11) & 0x7FF).astype(np.int64)
    pad = lambda a, v: np.pad(a, ((0, nty * th - W), (0, ntx * tw - W)), constant_values=v).reshape(nty, th, ntx, tw)
    big = 1 << 20
    xlo = pad(np.where(written, X, big), big).min(axis=(1, 3)); xhi = pad(np.where(written, X + 1, -1), -1).max(axis=(1, 3))
    ylo = pad(np.where(written, Y, big), big).min(axis=(1, 3)); yhi = pad(np.where(written, Y + 1, -1), -1).max(axis=(1, 3))
    return xlo, xhi, ylo, yhi


@pytest.mark.parametrize("tw,th", SHAPES)
@pytest.mark.parametrize("name,F,Ih", CAMERAS)
def test_every_tap_lies_in_its_tiles_rectangle(name, F, Ih, tw, th):
    camd, lut, tiles, n_live, lds = _table(name, F, Ih, tw, th)
    W = 3 * F
    cross = _cross(F)
    written = cross & (lut != 0)
    assert 0.4 < written.sum() / cross.sum() < 0.9          # both cameras leave a good part of the cross unwritten
    nty, ntx = -(-W // th), -(-W // tw)
    # one entry per tile, live tiles first, dead tiles (wholly in the corner blocks) behind them
    assert len(tiles) == nty * ntx and len(set(zip(tiles["ty"].tolist(), tiles["tx"].tolist()))) == len(tiles)
    any_cross = np.pad(cross, ((0, nty * th - W), (0, ntx * tw - W))).reshape(nty, th, ntx, tw).any(axis=(1, 3))
    dead = (tiles["flags"] & 2) != 0
    assert not dead[:n_live].any() and dead[n_live:].all()
    assert np.array_equal(any_cross[tiles["ty"], tiles["tx"]], ~dead)
    xlo, xhi, ylo, yhi = (a[tiles["ty"], tiles["tx"]] for a in _tile_extents(lut, written, tw, th))
    has = xhi >= 0
    x0 = tiles["x0"].astype(np.int64); y0 = tiles["y0"].astype(np.int64)
    x1 = x0 + 4 * tiles["nd"].astype(np.int64) - 1; y1 = y0 + tiles["rows"].astype(np.int64) - 1
    staged = has & ~dead & ((tiles["flags"] & 1) == 0)
    if (tw, th) == (64, 16) and F >= 450:
        # the shape the library uses, at the face sizes the cameras run at: the largest rectangle is 5.2 KB per frame (front camera, F = 650,
        # tools/remap_tile_model.py) against a budget of 8 KB, so no tile falls back.  (Small faces put more of the image under a tile.)
        assert staged.sum() == (has & ~dead).sum()
    # every tap of every written entry: X, X + 1 in [x0, x1], Y, Y + 1 in [y0, y1]  (or the tile is flagged as fallback)
    assert np.all(x0[staged] <= xlo[staged]) and np.all(xhi[staged] <= x1[staged])
    assert np.all(y0[staged] <= ylo[staged]) and np.all(yhi[staged] <= y1[staged])
    assert np.all(x0 % 4 == 0)
    # tiles without a written entry stage nothing
    assert np.all(tiles["nd"][~has] == 0) and np.all(tiles["rows"][~has] == 0)
    # the budget the launch asks for covers the largest staged rectangle (four frames side by side), and stays within the limit
    need = 16 * tiles["nd"].astype(np.int64) * tiles["rows"].astype(np.int64)
    assert need[staged].max() <= lds <= api.RT_LDS_MAX
    assert np.all(need[has & ~dead & ~staged] > api.RT_LDS_MAX)


@pytest.mark.parametrize("name,F,Ih", [("lafida", 550, None), ("front", 650, None)])
def test_unwritten_cells_do_not_enlarge_a_rectangle(name, F, Ih):
    tw, th = 64, 16
    camd, lut, tiles, n_live, lds = _table(name, F, Ih, tw, th)
    cross = _cross(F)
    written = cross & (lut != 0)
    xlo, xhi, ylo, yhi = (a[tiles["ty"], tiles["tx"]] for a in _tile_extents(lut, written, tw, th))
    has = xhi >= 0
    # the rectangles are tight: exactly the extent of the written entries, the left edge rounded down to a dword
    assert np.array_equal(tiles["x0"][has], (xlo[has] & ~3)) and np.array_equal(tiles["y0"][has], ylo[has])
    assert np.array_equal(tiles["rows"][has], (yhi - ylo + 1)[has])
    assert np.array_equal(tiles["nd"][has], ((xhi - (xlo & ~3)) // 4 + 1)[has])
    # tiles that mix written and unwritten cross cells exist, lie far from the image origin, and stay small
    unwritten = cross & (lut == 0)
    W = 3 * F
    nty, ntx = -(-W // th), -(-W // tw)
    mixed = np.pad(unwritten, ((0, nty * th - W), (0, ntx * tw - W))).reshape(nty, th, ntx, tw).any(axis=(1, 3))[tiles["ty"], tiles["tx"]] & has
    assert mixed.sum() > 20
    far = mixed & ((tiles["x0"] > 64) | (tiles["y0"] > 64))
    assert far.sum() > 20
    assert np.all(4 * tiles["nd"][far].astype(np.int64) * tiles["rows"][far] <= 8192)
    # with the unwritten cells counted as taps of pixel (0, 0) those rectangles would reach the origin and blow the budget
    stretched = (tiles["x0"][far].astype(np.int64) + 4 * tiles["nd"][far]) * (tiles["y0"][far].astype(np.int64) + tiles["rows"][far])
    assert np.median(stretched) > 8192


def test_budget_flags_and_argument_checks():
    camd, lut, tiles, n_live, lds = _table("front", 650, None, 64, 16, budget=4096)
    has = tiles["nd"] > 0
    need = 16 * tiles["nd"].astype(np.int64) * tiles["rows"]
    assert np.array_equal((tiles["flags"] & 1) != 0, has & (need > 4096)) and ((tiles["flags"] & 1) != 0).any()
    assert lds <= 4096
    with pytest.raises(api.CmsError):
        api.remap_tiles_host(camd, lut, 48, 16)
    with pytest.raises(api.CmsError):
        api.remap_tiles_host(camd, lut, 64, 8)
