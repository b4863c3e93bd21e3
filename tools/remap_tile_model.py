"""CPU model of the remap's memory access per wavefront / workgroup shape (no GPU, only cubemapslam_amd.synth).

    python tools/remap_tile_model.py [lafida|front] [F]

The LUT is modelled in float64 from synth.world_to_img (not the library's bit-exact table: this is about access patterns).  Two tables:

  1. the distinct 128-byte lines one 64-lane gather instruction touches (a lane = 4 consecutive canvas pixels, one gather = tap row 0
     or 1 of pixel i of every lane), over wavefronts whose pixels are all written, for the wavefront shapes 256 x 1 (k_remap), 128 x 2,
     64 x 4 and 32 x 8 (the 2-D tiles of 128 x 8, 64 x 16 and 32 x 32 pixels);
  2. the source bounding box of a 1024-pixel workgroup tile (the bytes k_remap_t* stages in LDS per frame, rows padded to dwords), and
     the staged bytes per written output pixel.

Cells the reference never writes (outside the fisheye image) are left out, as in cms_remap_tiles.h.
"""
import sys
import numpy as np
sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), ".."))
from cubemapslam_amd import synth


def model_lut(cam):
    """(X, Y, written) per canvas pixel: integer tap origin and whether the reference writes the cell"""
    F = cam["face"]; W = 3 * F
    X = np.zeros((W, W), np.int64); Y = np.zeros((W, W), np.int64); ok = np.zeros((W, W), bool)
    jj, ii = np.meshgrid(np.arange(F, dtype=np.float64), np.arange(F, dtype=np.float64))
    for f, (cx, cy) in synth._FACE_ORIGIN.items():
        x = (jj - F / 2.0) / (F / 2.0); y = (ii - F / 2.0) / (F / 2.0); z = np.ones_like(x)
        rx, ry, rz = synth._F2R[f](x, y, z)
        u, v = synth.world_to_img(cam, np.stack([rx, ry, rz], -1))
        w = (u >= 0) & (u < cam["Iw"]) & (v >= 0) & (v < cam["Ih"])
        sl = (slice(cy * F, (cy + 1) * F), slice(cx * F, (cx + 1) * F))
        X[sl] = np.where(w, np.floor(u), 0); Y[sl] = np.where(w, np.floor(v), 0); ok[sl] = w
    return X, Y, ok


def lines_per_gather(X, Y, ok, stride, ww, wh):
    """wavefront = ww x wh canvas pixels (ww / 4 lanes per row); per gather: distinct 128-byte lines of the 64 lanes' 2-byte reads"""
    W = X.shape[0]
    out = []
    for y0 in range(0, W - wh + 1, wh):
        for x0 in range(0, W - ww + 1, ww):
            if not ok[y0:y0 + wh, x0:x0 + ww].all():
                continue
            for i in range(4):                      # pixel i of every lane
                xs = X[y0:y0 + wh, x0 + i:x0 + ww:4].ravel(); ys = Y[y0:y0 + wh, x0 + i:x0 + ww:4].ravel()
                for r in (0, 1):                    # tap row
                    a = (ys + r) * stride + xs
                    out.append(len(np.unique(np.concatenate([a // 128, (a + 1) // 128]))))
    return np.array(out)


def tile_boxes(X, Y, ok, tw, th):
    W = X.shape[0]
    bytes_, px = [], []
    for y0 in range(0, W, th):
        for x0 in range(0, W, tw):
            m = ok[y0:y0 + th, x0:x0 + tw]
            if not m.any():
                continue
            xs = X[y0:y0 + th, x0:x0 + tw][m]; ys = Y[y0:y0 + th, x0:x0 + tw][m]
            xl = xs.min() & ~3
            bytes_.append(((xs.max() + 1 - xl) // 4 + 1) * 4 * (ys.max() + 1 - ys.min() + 1)); px.append(m.sum())
    return np.array(bytes_), np.array(px)


if __name__ == "__main__":
    name = sys.argv[1] if len(sys.argv) > 1 else "lafida"
    F = int(sys.argv[2]) if len(sys.argv) > 2 else (550 if name == "lafida" else 650)
    cam = synth.camera(name, F)
    stride = (cam["Iw"] + 63) // 64 * 64
    X, Y, ok = model_lut(cam)
    cross = 5 * F * F
    print("%s F = %d, source %d x %d, row stride %d; %.0f %% of the cross is never written" % (name, F, cam["Iw"], cam["Ih"], stride, 100 - 100.0 * ok.sum() / cross))
    print("\n| wavefront shape | 128-byte lines per gather: mean / p90 / max |\n|---|---|")
    for ww, wh in ((256, 1), (128, 2), (64, 4), (32, 8)):
        n = lines_per_gather(X, Y, ok, stride, ww, wh)
        print("| %d x %d | %.1f / %.1f / %d |" % (ww, wh, n.mean(), np.percentile(n, 90), n.max()))
    print("\n| tile (1024 px) | source box bytes: mean / max | staged bytes per written output px |\n|---|---|---|")
    for tw, th in ((1024, 1), (128, 8), (64, 16), (32, 32)):
        b, p = tile_boxes(X, Y, ok, tw, th)
        print("| %d x %d | %.0f / %d | %.2f |" % (tw, th, b.mean(), b.max(), b.sum() / p.sum()))
