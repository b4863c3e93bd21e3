"""Stand-alone time of the window query (cms_area_launch: Frame::GetFeaturesInArea for a batch of windows) at the three shapes of bench.py's step:
  mm    the motion-model windows: ~358 k queries on 256 frames (radius 15 x scale of the octave, levels [o - 1, o + 1]);
  lm    the local-map windows:    ~550 k queries on 256 frames (radius 4 x scale of the level, levels [l - 1, l]);
  fuse  one store-wide cms_kfstore_fuse_search_sets call with ~240 k projections (21 resident key frames, 320 jobs of 750 map points); this entry
        uploads, projects, queries, scans and synchronises, so its figure is the whole call, not the query alone.
python tools/prof_window_query.py [reps, default 20]
mm / lm: `reps` query sequences are enqueued back to back on the context's stream after a warm-up and the stream is synchronised once; the sequence's
kernels take hundreds of microseconds against a few for their launches, so the queue never runs dry and wall time / reps is the device time of one sequence.
Set CMS_HIP_LIB to time another build of the library with the same inputs."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
torch.cuda.init()
from cubemapslam_amd import api, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
F, B, NKP = 550, 256, 2000
ORIGIN = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)])      # face -> (col, row) on the cross
camd = synth.camera("lafida", F)
rs = np.random.RandomState(5)
dev = torch.device("cuda", 0)


def keypoints(n):
    face = rs.randint(0, 5, n)
    kps = np.zeros(n, api.KP_DTYPE)
    kps["x"] = ORIGIN[face, 0] * F + rs.uniform(0, F, n); kps["y"] = ORIGIN[face, 1] * F + rs.uniform(0, F, n); kps["octave"] = rs.randint(0, 8, n)
    return kps


ctx = api.Context(camd, nfeatures=NKP, max_batch=B)
frames = [keypoints(NKP) for _ in range(B)]
for b, k in enumerate(frames):
    ctx.area_set_keypoints(b, k)
ctx.area_grid(B)
sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)


def windows(per_frame, radius, lo_d, hi_d):
    """per frame: windows around a sample of its key points, moved by a few pixels"""
    qf, qx, qy, qr, lo, hi = [], [], [], [], [], []
    for b, k in enumerate(frames):
        pick = rs.randint(0, len(k), per_frame)
        qf.append(np.full(per_frame, b, np.int32))
        qx.append(k["x"][pick] + rs.normal(0, 3, per_frame)); qy.append(k["y"][pick] + rs.normal(0, 3, per_frame))
        o = k["octave"][pick].astype(np.int32)
        qr.append(np.float32(radius) * sf[o]); lo.append(o + lo_d); hi.append(o + hi_d)
    cat = lambda v, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(v), dt)).to(dev)
    return cat(qf, np.int32), [cat(qx, np.float32), cat(qy, np.float32), cat(qr, np.float32), cat(lo, np.int32), cat(hi, np.int32)]


def time_batch(name, per_frame, radius, lo_d, hi_d):
    d_qf, dq = windows(per_frame, radius, lo_d, hi_d)
    nq = int(d_qf.numel())
    d_cnt = torch.zeros(nq, dtype=torch.int32, device=dev); d_off = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int32, device=dev); d_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    call = lambda cap: ctx.features_in_area_batch_device(nq, d_qf.data_ptr(), [t.data_ptr() for t in dq], d_cnt.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), cap, d_tot.data_ptr())
    call(0); ctx.sync()                                          # the dry run sizes the candidate array, as bench.py does
    total = int(d_tot.item())
    d_idx = torch.zeros(total + 64, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(3):
        call(total)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call(total)
    ctx.sync()
    us = 1e6 * (time.perf_counter() - t0) / reps
    cnt = d_cnt.cpu().numpy()
    print("%-5s nq %7d  candidates %8d (%.2f per window, %.2f %% of the windows above 8)  %8.1f us per query sequence" %
          (name, nq, total, total / nq, 100.0 * (cnt > 8).mean(), us), flush=True)


time_batch("mm", 1400, 15.0, -1, 1)
time_batch("lm", 2150, 4.0, -1, 0)

# ---- the store-wide Fuse call of the mapping side
NKF, NSET, NCUR = 21, 750, 8
store = api.KeyframeStore(ctx, max_keyframes=NKF, max_features=2048, max_nodes=16)
sets = []
for s in range(NKF):
    k = frames[s]
    kd = synth.descriptors(len(k), 100 + s)
    pr = synth.local_map_problem(F, k["x"], k["y"], k["octave"], kd, seed=9)       # the same seed: every key frame has the same pose
    kf = dict(x=k["x"], y=k["y"], octave=k["octave"].astype(np.int32), angle=np.zeros(len(k), np.float32), desc=kd, mp=np.full(len(k), -1, np.int32), R=pr["pose15"][:9],
              t=pr["pose15"][9:12], Ow=pr["pose15"][12:], node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32), median_depth=1.0,
              rays=np.zeros((len(k), 3), np.float32))
    K, _keep = api.make_keyframe(kf)
    store.put(s, K)
    sets.append({n: pr[n][:NSET] for n in ("pos", "normal", "min_dist", "max_dist", "desc")})
jobs = []
for c in range(NCUR):
    for n in range(NKF):
        if n != c:
            jobs.append((n, c, None)); jobs.append((c, n, None))
for _ in range(3):
    got = store.fuse_search_sets(sets, jobs, th=3.0)
t0 = time.perf_counter()
for _ in range(reps):
    got = store.fuse_search_sets(sets, jobs, th=3.0)
ms = 1e3 * (time.perf_counter() - t0) / reps
print("fuse  %d jobs, %d projections, %d matched  %8.3f ms per call (uploads, projection, query, scan and read-back included)" %
      (len(jobs), sum(len(g[0]) for g in got), sum(int((g[0] >= 0).sum()) for g in got), ms), flush=True)
store.close(); ctx.close()
