"""bench.py's step through the C++ batch driver (cubemapslam_amd/host/batch_driver.cpp) and through its own Python loop: the same calls in the same order.
Both must run, the windows of the step that bench.py verifies must agree with the oracle under either driver (iteration counts, outlier flags, estimates:
config.ba_check), and the two figures must be of the same order -- a driver that skipped work would be much faster, one that serialised it much slower.
Their --dump-outputs of the last step must agree bit for bit where the product is bit-exact (key points, descriptors, matches, new map points)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(env_extra, dump_dir):
    env = dict(os.environ); env.update(env_extra)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "6", "--warmup", "2", "--batch", "64", "--cpu-frames", "0", "--no-streaming-pass", "--verify-windows", "4",
           "--optimise-only-steps", "0", "--closed-loop-frames", "0", "--confined-steps", "0", "--extract-only-steps", "0", "--random-views-steps", "0",
           "--mapping-only-steps", "0", "--unpipelined-steps", "0", "--deterministic-steps", "0", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-1000:]
    return json.loads(lines[-1])


def test_cpp_driver_and_python_loop_run_the_same_step(tmp_path):
    a = _run({}, tmp_path / "cpp")
    b = _run({"CMS_BENCH_PY_DRIVER": "1"}, tmp_path / "py")
    assert a["config"]["host"]["step_driver"].startswith("c++") and b["config"]["host"]["step_driver"].startswith("python")
    for j in (a, b):
        chk = j["config"]["ba_check"]
        n_ba = j["config"]["ba_windows_per_step"]
        assert chk["windows_with_iterations_and_outlier_flags_equal_to_the_oracle"] == n_ba, chk
        assert chk["worst_relative_update_error"] <= 1e-4 or chk["windows_with_a_float_rounding_cascade"], chk
        assert j["roofline"]["launches_per_step"] > 10 and j["config"]["new_map_points_per_step"] > 0
    assert a["config"]["python_step_loop"] is not None
    # (two four-step runs of a small configuration on a box other jobs share: the throughputs only have to be of the same order -- a 0.6 .. 1.7 window failed
    # once in ~40 runs with 1.78 -- what the two drivers compute is held to the oracle above)
    ratio = a["value"] / b["value"]
    assert 0.25 < ratio < 4.0, (a["value"], b["value"])
    # --dump-outputs: float32 / float64 arrays under 64 MB, and the same last step from either driver
    files = sorted(f.name for f in (tmp_path / "cpp").iterdir())
    assert files == sorted(f.name for f in (tmp_path / "py").iterdir()) and "frame_poses.npy" in files, files
    assert sum(f.stat().st_size for f in (tmp_path / "cpp").iterdir()) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "cpp" / f), np.load(tmp_path / "py" / f)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), f
    for name in ("keypoints", "descriptors", "keypoint_map_points", "motion_model_matches", "local_map_matches", "new_map_point_pairs", "new_map_points"):
        x, y = np.load(tmp_path / "cpp" / (name + ".npy")), np.load(tmp_path / "py" / (name + ".npy"))
        assert len(x) > 0 and np.array_equal(x, y), name
