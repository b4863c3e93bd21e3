"""The tiled remap kernels (k_remap_t*: 2-D tiles, source rectangle staged in LDS or gathered directly) against the row-strip kernel
k_remap (CMS_REMAP_TILES=0) and the oracle's remap: canvases byte for byte; and cms_frames_process_device (resident batch read in place)
against cms_frames_upload_device + cms_frames_process."""
import ctypes as C

import numpy as np
import pytest
import orc
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

MAXB = 8
# (CMS_REMAP_TILES, CMS_REMAP_TILE_W): the default (staged, 64 x 16), the other shapes, direct gathers from the 2-D shape, the old kernel
MODES = [("1", "64"), ("1", "32"), ("1", "128"), ("2", "64"), ("2", "128"), ("0", "64")]


def _faces(F):
    m = np.zeros((3 * F, 3 * F), bool)
    for (ox, oy) in synth._FACE_ORIGIN.values():
        m[oy * F:(oy + 1) * F, ox * F:(ox + 1) * F] = True
    return m


def _ctx(monkeypatch, camd, mode, tw, nfeatures=500, max_batch=MAXB):
    monkeypatch.setenv("CMS_REMAP_TILES", mode)
    monkeypatch.setenv("CMS_REMAP_TILE_W", tw)
    return api.Context(camd, nfeatures=nfeatures, max_batch=max_batch)


def _frames(camd, n, seed):
    fr = np.stack([synth.texture(camd["Ih"], camd["Iw"], seed + b) for b in range(n)])
    fr[:, 0, 0] = 200 + np.arange(n)          # pixel (0, 0) is what the unwritten cells of the cross show: make it tell the frames apart
    fr[:, -1, -1] = 100 + np.arange(n)        # ... and the image's last byte (the pair read of the old kernel ends behind it)
    return fr


@pytest.mark.parametrize("name,F,Ih", [("lafida", 450, None), ("lafida", 550, None), ("front", 650, None), ("lafida", 120, None)])
def test_canvases_identical_tiled_old_and_oracle(monkeypatch, name, F, Ih):
    camd = synth.camera(name, F, Ih)
    ocam = orc.make_camera(camd)
    m1, m2 = orc.build_lut(ocam)
    frames = _frames(camd, MAXB, 31)
    faces = _faces(F)
    ref = [orc.fisheye_to_cubemap(ocam, m1, m2, frames[b]) for b in range(MAXB)]
    for mode, tw in MODES:
        ctx = _ctx(monkeypatch, camd, mode, tw)
        ctx.set_mask(synth.cubemap_valid_mask(camd))
        for B in (1, 5, MAXB):                 # 5: not a multiple of the frame group of 4
            # frames in another order per B, so a canvas left over from the previous launch cannot pass for this one's
            order = [(b + B) % MAXB for b in range(B)]
            ctx.upload(frames[order])
            ctx.process(B, True); ctx.sync()
            for b in range(B):
                got = ctx.debug_level(b, 0)
                assert np.array_equal(got[faces], ref[order[b]][faces]), (name, F, mode, tw, B, b, int((got[faces] != ref[order[b]][faces]).sum()))
                assert not got[~faces].any(), (name, F, mode, tw, B, b)          # corner blocks of the batched path are 0
        # the single-frame entry: the caller's corner blocks stay as they are
        canvas = np.full((3 * F, 3 * F), 77, np.uint8)
        got = ctx.remap(frames[3], canvas)
        assert np.array_equal(got[faces], ref[3][faces]) and np.all(got[~faces] == 77), (name, F, mode, tw)
        ctx.close()


def test_more_frame_groups_than_workgroups_per_tile(monkeypatch):
    """69 frames = 18 frame groups: a workgroup of the tiled kernels walks two of them (the staged rectangle is replaced under a barrier), the
    last group holds one frame."""
    F, B = 450, 69
    camd = synth.camera("lafida", F)
    ocam = orc.make_camera(camd)
    m1, m2 = orc.build_lut(ocam)
    base = _frames(camd, 8, 83)
    frames = np.stack([np.roll(base[b % 8], 7 * (b // 8), axis=1) for b in range(B)])
    faces = _faces(F)
    ref = [orc.fisheye_to_cubemap(ocam, m1, m2, frames[b]) for b in range(B)]
    for mode, tw in (("1", "64"), ("2", "64"), ("0", "64")):
        ctx = _ctx(monkeypatch, camd, mode, tw, max_batch=B)
        ctx.upload(frames)
        ctx.process(B, True); ctx.sync()
        for b in range(B):
            got = ctx.debug_level(b, 0)
            assert np.array_equal(got[faces], ref[b][faces]) and not got[~faces].any(), (mode, b)
        ctx.close()


def test_corner_blocks_dirtied_by_a_caller_canvas_are_rewritten(monkeypatch):
    F = 450
    camd = synth.camera("lafida", F)
    ocam = orc.make_camera(camd)
    m1, m2 = orc.build_lut(ocam)
    frames = _frames(camd, 5, 57)
    faces = _faces(F)
    dirty = synth.texture(3 * F, 3 * F, 5)
    for mode, tw in MODES:
        ctx = _ctx(monkeypatch, camd, mode, tw)
        ctx.extract(dirty)                     # a caller-supplied canvas goes through frame 0 of the pyramid buffer, corner blocks included
        assert ctx.debug_level(0, 0)[~faces].any()
        ctx.upload(frames)
        ctx.process(5, True); ctx.sync()
        for b in range(5):
            got = ctx.debug_level(b, 0)
            ref = orc.fisheye_to_cubemap(ocam, m1, m2, frames[b])
            assert np.array_equal(got[faces], ref[faces]) and not got[~faces].any(), (mode, tw, b)
        ctx.process(5, True); ctx.sync()       # ... and the launch after it (no corner writes any more) still sees zeros there
        assert not ctx.debug_level(0, 0)[~faces].any(), (mode, tw)
        ctx.close()


def _hip():
    api.lib()
    with open("/proc/self/maps") as f:        # the HIP runtime the library itself is linked against, not a second copy
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "libamdhip64 is not loaded"
    paths = [p for p in paths if "torch" not in p] or paths      # (torch ships a runtime of its own, see conftest.py)
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.mark.parametrize("name,F,B", [("lafida", 550, MAXB), ("front", 650, 5), ("lafida", 450, 1)])
def test_process_device_equals_upload_device_and_process(monkeypatch, name, F, B):
    camd = synth.camera(name, F)
    hip = _hip()
    frames = _frames(camd, B, 71)
    results = {}
    for mode, tw in (("1", "64"), ("2", "64"), ("0", "64")):
        ctx = _ctx(monkeypatch, camd, mode, tw, nfeatures=camd["nfeatures"])
        ctx.set_mask(synth.cubemap_valid_mask(camd))
        fs = ctx.geom.fisheye_stride
        staged = np.zeros((B, camd["Ih"], fs), np.uint8)
        staged[:, :, :camd["Iw"]] = frames
        staged[:, :, camd["Iw"]:] = 171        # the row padding is never part of a result
        d_src = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_src), staged.nbytes) == 0          # exactly B x pitch bytes: nothing behind the last row belongs to us
        try:
            assert hip.hipMemcpy(d_src, staged.ctypes.data_as(C.c_void_p), staged.nbytes, 1) == 0
            ctx.upload_device(d_src.value, B)
            ctx.process(B, True); ctx.sync()
            want = [ctx.fetch(b) for b in range(B)]
            canv = [ctx.debug_level(b, 0) for b in range(B)]
            # poison the staging buffer: the in-place entry must not read it
            ctx.upload(np.full((ctx.max_batch, camd["Ih"], camd["Iw"]), 255, np.uint8))
            ctx.process_device(d_src.value, B); ctx.sync()
            for b in range(B):
                k, d = ctx.fetch(b)
                assert len(k) > 100 and np.array_equal(k.view(np.uint8), want[b][0].view(np.uint8)) and np.array_equal(d, want[b][1]), (mode, b)
                assert np.array_equal(ctx.debug_level(b, 0), canv[b]), (mode, b)
            if mode != "0":                    # (the old kernel keeps the copy: see cms_frames_process_device)
                ctx.process(B, True); ctx.sync()
                assert len(ctx.fetch(0)[0]) != len(want[0][0]) or not np.array_equal(ctx.fetch(0)[1], want[0][1])     # the poison was really there
            results[mode] = want
            with pytest.raises(api.CmsError):
                ctx.process_device(d_src.value + 1, B)                     # not dword aligned
            with pytest.raises(api.CmsError):
                ctx.process_device(d_src.value, ctx.max_batch + 1)
        finally:
            ctx.sync()
            hip.hipFree(d_src)
            ctx.close()
    for mode in ("2", "0"):
        for b in range(B):
            assert np.array_equal(results[mode][b][0].view(np.uint8), results["1"][b][0].view(np.uint8)) and np.array_equal(results[mode][b][1], results["1"][b][1])
