"""The FAST work list of a remapped batch (cms_fast_cell_lists in cms_api_frames.hip), checked on the host through cms_fast_cells_host: no GPU.
The list leaves out every cell whose ROI holds one value whatever the picture shows: the zero corner blocks of the cross, and the face pixels
the reference never writes, which the remap fills with the frame's pixel (0, 0).  Both are followed down the pyramid through the resize
tables, which rests on one step: the bilinear blend of four equal taps c is c.  (a) establishes that step on the oracle, exhaustively;
(b) compares the list with an oracle pyramid."""
import numpy as np
import pytest
import orc
from cubemapslam_amd import api, build, synth

MINB = 16      # EDGE_THRESHOLD - 3 (ORBExtractor.cpp:747)


def _level_widths(W, nlevels=8, scale_factor=1.2):
    """ORBextractor's level sizes: cvRound(W * mvInvScaleFactor[l]) in float (ORBExtractor.cpp:386-403, 932-933)"""
    sf = [np.float32(1.0)]
    for _ in range(nlevels - 1):
        sf.append(np.float32(np.float64(sf[-1]) * np.float64(np.float32(scale_factor))))
    return [int(np.rint(np.float64(np.float32(W) * (np.float32(1.0) / s)))) for s in sf]


@pytest.mark.parametrize("F", [550, 650])
def test_four_equal_taps_blend_to_their_value(F):
    """(a) every coefficient pair of the x and y tables of every level of bench.py's configurations (8 levels, 1.2), every c = 0 .. 255: a
    constant level resizes to the same constant, pixel for pixel."""
    ws = _level_widths(3 * F)
    assert ws[0] == 3 * F and ws[-1] >= 2 * MINB + 30
    for l in range(1, len(ws)):
        src = np.empty((ws[l - 1], ws[l - 1]), np.uint8)
        for c in range(256):
            src[:] = c
            out = orc.resize(src, ws[l], ws[l])
            assert out.min() == c and out.max() == c, (F, l, c)


def _cells(w):
    """the cells of a w x w level the reference loop visits (ORBExtractor.cpp:745-781): {(row, column): (iniX, maxX, iniY, maxY)}"""
    width = np.float32(w - 2 * MINB)
    n = int(width / np.float32(30))
    cell = int(np.ceil(width / np.float32(n)))
    maxB = w - MINB
    out = {}
    for ci in range(n):
        for cj in range(n):
            iniY, iniX = MINB + ci * cell, MINB + cj * cell
            if iniY >= maxB - 3 or iniX >= maxB - 6:
                continue
            maxY, maxX = min(iniY + cell + 6, maxB), min(iniX + cell + 6, maxB)
            if maxX - iniX - 6 <= 0 or maxY - iniY - 6 <= 0:
                continue
            out[(ci, cj)] = (iniX, maxX, iniY, maxY)
    return out


def _lists(camd, **kw):
    build.build(verbose=False)
    return [set(zip(*(a.tolist() for a in api.fast_cells_host(camd, which, **kw)))) for which in range(3)]


# F = 75 is the size of the GPU tests: there the Lafida list drops nothing (a cell's ROI is half a face wide), the front camera's one cell
@pytest.mark.parametrize("name,F,drops", [("lafida", 75, False), ("lafida", 100, True), ("front", 75, True), ("front", 150, True)])
def test_dropped_cells_are_constant_in_an_oracle_pyramid(name, F, drops):
    """(b) a random fisheye image whose pixel (0, 0) is 255, remapped and resized level by level by the oracle: every cell the remapped batch's
    list drops has a constant ROI there, every cell it keeps is in the parent's list (the one without the zero corners), and that one in the
    full list, which is the reference loop's."""
    camd = synth.camera(name, F)
    ocam = orc.make_camera(camd)
    every, nz, live = _lists(camd)
    assert live <= nz <= every
    fish = np.random.RandomState(F).randint(0, 255, size=(camd["Ih"], camd["Iw"])).astype(np.uint8)
    fish[0, 0] = 255
    m1, m2 = orc.build_lut(ocam)
    img = orc.fisheye_to_cubemap(ocam, m1, m2, fish)
    ws = _level_widths(3 * F)
    n_dropped = {0: 0, 255: 0}
    for l, w in enumerate(ws):
        if l:
            img = orc.resize(img, w, w)
        cells = _cells(w)
        assert {(l, ci, cj) for ci, cj in cells} == {e for e in every if e[0] == l}
        for (ci, cj), (x0, x1, y0, y1) in cells.items():
            roi = img[y0:y1, x0:x1]
            if (l, ci, cj) not in live:
                assert roi.min() == roi.max() and int(roi[0, 0]) in (0, 255), (l, ci, cj)
                if (l, ci, cj) in nz:
                    n_dropped[int(roi[0, 0])] += 1
            elif (l, ci, cj) not in nz:
                assert roi.max() == 0, (l, ci, cj)
    # the new list is shorter than the parent's, by cells of never-written face pixels; a cell that is constant zero inside a face (a face pixel
    # next to the corner block blends with it) may be among them
    assert (n_dropped[255] > 0) == drops and n_dropped[0] + n_dropped[255] == len(nz) - len(live)


@pytest.mark.parametrize("name,F,n_nz,n_dropped", [("lafida", 550, 5081, 844), ("front", 650, 7130, 2479)])
def test_list_lengths_of_the_benchmark_configurations(name, F, n_nz, n_dropped):
    """the counts of the two cameras at the face sizes they run at, from the library's own LUT and tables"""
    camd = synth.camera(name, F)
    every, nz, live = _lists(camd, nfeatures=camd["nfeatures"])
    assert live <= nz <= every
    assert (len(nz), len(nz) - len(live)) == (n_nz, n_dropped)


def test_argument_checks_and_kernel_order():
    camd = synth.camera("lafida", 75)
    build.build(verbose=False)
    cam = api.make_camera(camd)
    orb = api.OrbParams(2000, 1.2, 8, 20, 7)
    f = api.lib().cms_fast_cells_host
    import ctypes as C
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    n = C.c_int()
    assert f(C.byref(cam), C.byref(orb), 3, None, 0, C.byref(n)) < 0
    assert f(C.byref(cam), C.byref(orb), 2, None, 0, C.byref(n)) == 0 and n.value > 0
    small = np.zeros(1, np.int32)
    assert f(C.byref(cam), C.byref(orb), 2, small.ctypes.data_as(C.c_void_p), 1, C.byref(n)) < 0
    # the XCD striping is kept: entry j of the list is entry (j % 8) * per + j // 8 of the row-major order
    l, r, c = api.fast_cells_host(camd, 2)
    key = (l.astype(np.int64) << 16) | (r.astype(np.int64) << 8) | c
    per = (len(key) + 7) // 8
    order = [x * per + j for j in range(per) for x in range(8) if x * per + j < len(key)]
    assert np.array_equal(np.sort(key)[order], key)
