"""cms_essential_graph_optimize and cms_sim3_correct_points on the device against the host build of the same core
(cubemapslam_amd/csrc/cms_ess_graph_core.h: hm_essential_graph_optimize_host, hm_sim3_correct_points_host) on the same records: every output field
-- the optimised Sim3 of every vertex, Tiw, chi2_initial, chi2_final, lambda_final, the iteration and trial counts, the flags -- is equal bit for
bit.  Every operation of the core is IEEE-rounded on both sides and log / acos / exp / sin / cos are the core's own, so any difference is a finding.
The shapes are the smallest at which the pivot loop, the slot fold (256) and the thread count (1024) can go wrong."""
import numpy as np
import pytest

import ess_graph_cases as gc
import ess_graph_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
MAX_JOBS, MAX_V, MAX_E, MAX_B = 8, 2200, 8000, 40000
SMALL = gc.SMALL_HANDLE


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def opt():
    s = api.EssentialGraphOptimizer(MAX_JOBS, MAX_V, MAX_E, MAX_B, device=0)
    yield s
    s.close()


_GRAPHS = {}


def state(seed, N, fix_scale=0, iterations=20, **kw):
    key = (seed, N, fix_scale, tuple(sorted(kw.items())))
    if key not in _GRAPHS:
        _GRAPHS[key] = gc.graph(seed, N, fix_scale, **kw)
    return api.ess_graph_job_state(_GRAPHS[key], iterations=iterations)


def same(want, got):
    assert len(want) == len(got)
    diff = api.ess_graph_first_difference(want, got)
    assert diff is None, diff


def host(states):
    rc, want = hl.optimize_host(states)
    assert rc == 0, hl.reason()
    return want


def improved(r, by=0.5):
    return r["iterations_run"] >= 1 and float(r["chi2_final"][0]) < by * float(r["chi2_initial"][0])


FREE = (1, 2, 7, 63, 64, 65, 300)


@pytest.mark.parametrize("fix_scale", (0, 1))
def test_free_vertex_counts(ctx, opt, fix_scale):
    """1, 2, 7, 63, 64, 65 and 300 free vertices in one call"""
    make = lambda: [state(20 + n, n + 1, fix_scale) for n in FREE]
    want = host(make())
    same(want, opt.run(ctx, make()))
    assert all(improved(r, 0.9) for r in want) and improved(want[-1], 0.05)
    if fix_scale:
        assert all((r["S"][:, 7] == s["Scw"][:, 7]).all() for r, s in zip(want, make()))


@pytest.mark.parametrize("where", ("first", "middle", "last", "loop_target"))
def test_fixed_vertex_placement(ctx, opt, where):
    N = 40
    kw = dict(first=dict(fixed=0), middle=dict(fixed=20), last=dict(fixed=N - 1), loop_target=dict(fixed=7, loop="fixed"))[where]
    make = lambda: [state(31, N, fs, **kw) for fs in (0, 1)]
    want = host(make())
    same(want, opt.run(ctx, make()))
    for r, s in zip(want, make()):
        assert improved(r) and r["S"][kw["fixed"]].tobytes() == s["Scw"][kw["fixed"]].tobytes()


@pytest.mark.parametrize("shape", ("chain", "last_first", "double_edge"))
def test_envelope_shapes(ctx, opt, shape):
    """A chain only (envelope width 1), one loop edge from the last to the first free vertex (one full-width row), two edges on one pair"""
    N = 20
    kw = dict(chain=dict(spans=(1,), loop="none"), last_first=dict(spans=(1,), loop="last_first"), double_edge=dict(double_edge=True))[shape]
    make = lambda: [state(41, N, fs, **kw) for fs in (0, 1)]
    g = _GRAPHS.get((41, N, 0, tuple(sorted(kw.items())))) or gc.graph(41, N, 0, **kw)
    first, B = hl.envelope(N, g["fixed"], g["edges"])
    if shape == "chain":
        assert B == (N - 1) + (N - 2) - 1      # one block left of every diagonal block but the first, and none across the fixed vertex
    if shape == "last_first":
        assert first[-1] == 0
    if shape == "double_edge":
        pairs = [tuple(sorted(e[:2])) for e in g["edges"]]
        assert len(set(pairs)) < len(pairs)
    want = host(make())
    same(want, opt.run(ctx, make()))
    assert all(r["iterations_run"] >= 1 for r in want)


def test_more_vertices_than_threads(ctx, opt):
    """1030 free vertices with span-1 and span-3 edges: device against host core only"""
    make = lambda: [state(51, 1031, 0)]
    want = host(make())
    same(want, opt.run(ctx, make()))
    assert improved(want[0], 0.05)


def four_states():
    return [state(61, 12, 0), state(62, 130, 1, loop="fixed"), state(63, 40, 0, spans=(1,), loop="last_first"), state(64, 70, 1, fixed=69)]


def test_four_jobs_in_one_call_equal_each_alone(ctx, opt):
    want = host(four_states())
    got = opt.run(ctx, four_states())
    same(want, got)
    same(got, [opt.run(ctx, [s])[0] for s in four_states()])


def test_handle_reuse_and_identical_bytes(ctx, opt):
    """A smaller job after a larger one on one handle, then the larger one again: the same bits every time"""
    big = lambda: [state(71, 200, 0)]
    small = lambda: [state(72, 9, 1)]
    first = opt.run(ctx, big())
    second = opt.run(ctx, small())
    again = opt.run(ctx, big())
    same(first, again)
    same(host(big()), first)
    same(host(small()), second)


def test_zero_iterations_return_the_input(ctx, opt):
    make = lambda: [state(81, 40, 0, iterations=0), state(82, 1, 0)]      # ... and N == 1 with E == 0
    want = host(make())
    got = opt.run(ctx, make())
    same(want, got)
    for r, s in zip(got, make()):
        assert r["S"].tobytes() == s["Scw"].tobytes() and r["iterations_run"] == 0 and r["trials_run"] == 0
        assert r["chi2_final"][0] == r["chi2_initial"][0]
    assert got[0]["chi2_initial"][0] > 0 and got[1]["chi2_initial"][0] == 0


def _refused(ctx, opt, states, njobs=None, arr=None):
    arr = api.ess_graph_jobs(states) if arr is None else arr
    with pytest.raises(api.CmsError) as e:
        opt.optimize(ctx, arr, len(states) if njobs is None else njobs)
    for q, s in zip(arr, states):      # the records untouched
        assert q.iterations_run == -7 and q.trials_run == -7 and q.flags == -7 and q.chi2_initial == -7.0 and q.chi2_final == -7.0 and q.lambda_final == -7.0
        assert all(s[k] is None or (s[k] == 7.0).all() for k in ("S_out", "Tiw_out"))
    return str(e.value)


def test_error_paths_leave_the_records_untouched(ctx):
    small = api.EssentialGraphOptimizer(*SMALL, device=0)
    good = lambda: [state(*a, **kw) for a, kw in gc.GOOD_CASE]
    want = host(good())
    msgs = [_refused(ctx, small, st) for _, st in gc.broken_states(good)]
    msgs += [_refused(ctx, small, [state(*a, **kw) for a, kw in case]) for _, case in gc.CAPACITY_CASES]
    assert all("cms_essential_graph_optimize" in m and "(-1)" in m for m in msgs), msgs
    over = _refused(ctx, small, [state(*a, **kw) for a, kw in gc.OVERFLOW_CASE])
    assert "(-4)" in over and "need 203 blocks" in over, over
    with pytest.raises(api.CmsError):
        api._chk(api.lib().cms_essential_graph_optimize(small.h, ctx.h, 2, None), "cms_essential_graph_optimize")
    small.optimize(ctx, api.ess_graph_jobs([]), 0)      # njobs == 0 is CMS_OK with no launch, and the next valid call is correct
    same(want, small.run(ctx, good()))
    small.close()


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1000))
def test_correct_points(ctx, n):
    g = gc.graph(5, 12)
    pos, ref = gc.points(100 + n, n, 12)
    got = api.sim3_correct_points(ctx, pos, ref, g["Snc"], g["Scw"])
    want = hl.correct_points_host(pos, ref, g["Snc"], g["Scw"])
    assert got.shape == (n, 3) and got.tobytes() == want.tobytes()
    if n >= 63:
        assert (ref < 0).any() and (got[ref < 0] == pos[ref < 0]).all() and (got[ref >= 9] != pos[ref >= 9]).any()
    with pytest.raises(api.CmsError):
        api.sim3_correct_points(ctx, np.zeros((2, 3), np.float32), np.array([0, 12], np.int32), g["Snc"], g["Scw"])


@pytest.mark.parametrize("fix_scale", (0, 1))
def test_mirror_default_engine_equals_host_core(fix_scale):
    """Optimizer::OptimizeEssentialGraph of cubemap_hot_path.h with its default engine (the device) against the same class over HOST_CORE: the graph, the
    poses and the map points afterwards, bit for bit"""
    m = gc.mirror_case(fix_scale=fix_scale)
    want = hl.mirror(1, m)
    got = hl.mirror(0, m)
    assert len(want["edges"]) > 30 and (want["Tcw"] != np.stack([k["Tcw"] for k in m["kfs"]])).any() and (want["mp_pos"] != m["mp_pos"]).any()
    for k in want:
        assert np.asarray(want[k]).tobytes() == np.asarray(got[k]).tobytes(), k
