"""LoopClosing as one composite on the device (tests/loop_cases.py): every stage's own parity test runs on inputs built for that stage alone; here
the entries run in the order LoopClosing makes them -- DetectLoop, ComputeSim3, CorrectLoop with SearchAndFuse and OptimizeEssentialGraph, the
global BA -- on one consistent map with a known drift, each fed by the previous entry's OUTPUT, on the loop-closing thread's context against a store
that lives on the mapping side's and is rewritten between the searches, and every intermediate result is compared with the host chain (the CPU
reference each stage's own test compares against): up to the global BA exactly, integers as integers and floats as bits; the global BA by the bar of
tests/test_gpu_global_ba.py.  The bars to the ground truth are the ones tests/test_loop_closing_cpu.py measured on the float64 restatement.

Every chain runs once, in two module-scoped fixtures; the tests only compare."""
import pytest

import gba_cases
import loop_cases as lc
import npref_global_ba

pytestmark = pytest.mark.gpu
VARIANTS = dict(jump=dict(tree="jump"), split=dict(tree="split"), probed=dict(tree="jump", probe=True), fixed=dict(tree="jump", zw=False))


@pytest.fixture(scope="module")
def sc():
    return lc.scene()


@pytest.fixture(scope="module")
def host(sc):
    """the host chains, and per chain the global BA's reference from a 1e-12 m perturbation (gba_cases.close_or_cascade's cascade bar)"""
    be = lc.HostBackend()
    out = {name: lc.run(sc, be, **kw) for name, kw in VARIANTS.items()}
    out["rejected"] = lc.run_rejected(sc, be)
    be.close()
    out["gba_perturbed"] = {name: npref_global_ba.run(gba_cases.perturbed(lc.stage(out[name], "CollectGlobalBA")["problem"]), 10, False) for name in VARIANTS}
    return out


@pytest.fixture(scope="module")
def device(sc):
    """the device chains, all on ONE set of handles (store, covisibility index, solver, optimisers) in this order: "jump", "split", "probed", "fixed",
    the rejected pass between two snapshots of the store, "jump" again; then, on handles of its own, the chain up to ComputeSim3 with one candidate per
    call"""
    be = lc.DeviceBackend()
    out = {name: lc.run(sc, be, **kw) for name, kw in VARIANTS.items()}
    snaps = []
    out["rejected"] = lc.run_rejected(sc, be, before=lambda: snaps.append(be.snapshot()))
    snaps.append(be.snapshot())
    out["snapshots"] = snaps
    out["again"] = lc.run(sc, be, tree="jump")
    be.close()
    one = lc.DeviceBackend(one_by_one=True)
    out["single"] = lc.run(sc, one, upto_sim3=True)
    one.close()
    return out


def _gba_close(tag, want_rec, got_rec, want_perturbed):
    """the global BA of two chains: the same collected problem, equal iteration counts, updates by gba_cases.close_or_cascade"""
    prob = lc.stage(want_rec, "CollectGlobalBA")["problem"]
    want, got = lc.stage(want_rec, "GlobalBundleAdjustment"), lc.stage(got_rec, "GlobalBundleAdjustment")
    assert got["iterations_done"] == want["iterations_done"], (tag, got["iterations_done"], want["iterations_done"])
    rel = abs(got["chi2_final"] - want["chi2_final"]) / abs(want["chi2_final"])
    worst, cascaded = gba_cases.close_or_cascade(prob, got, want, want_perturbed, tag=tag)
    print("%s: global BA %d iterations, chi2 rel %.3g, worst block %.3g, cascaded %s" % (tag, got["iterations_done"], rel, worst, cascaded))
    assert rel <= 1e-6, (tag, rel)


@pytest.mark.parametrize("name", ["jump", "fixed"])
def test_chain_device_equals_host_stage_by_stage(host, device, name):
    """"jump": the chain as the bridge calls it; "fixed": with SearchBySim3 reading component 2, where that matcher's answers enter the match list"""
    diff = lc.first_difference(host[name], device[name])
    assert diff is None, diff
    assert lc.stage(device[name], "ComputeSim3")["accepted"] and "Final" in [n for n, _ in device[name]]
    _gba_close(name, host[name], device[name], host["gba_perturbed"][name])


def test_chain_reaches_the_truth(sc, host, device):
    """the device chain on the spanning tree that can end on the truth: the recovered Scw, all key-frame centres and all points, RMS, nothing removed"""
    rec = device["split"]
    diff = lc.first_difference(host["split"], rec)
    assert diff is None, diff
    _gba_close("split", host["split"], rec, host["gba_perturbed"]["split"])
    scw = lc.scw_error(sc, lc.stage(rec, "Scw")["Scw"])
    before, after = lc.truth_error(sc, None, "ACE"), lc.truth_error(sc, rec, "ACE")
    print("Scw %.3g m (bar %.3g); centres %.3g -> %.3g m (bar %.3g); points %.3g -> %.3g m (bar %.3g)" % (scw, lc.SCW_BAR, before[0], after[0], lc.CENTRE_BAR, before[1], after[1],
                                                                                                       lc.POINT_BAR))
    assert scw <= lc.SCW_BAR and after[0] <= lc.CENTRE_BAR and after[1] <= lc.POINT_BAR
    assert before[0] >= 20 * lc.CENTRE_BAR and before[1] >= 20 * lc.POINT_BAR      # (doing nothing does not pass)
    assert lc.scw_error(sc, lc.stage(device["jump"], "Scw")["Scw"]) == scw           # the tree does not reach back into ComputeSim3


def test_store_read_back_after_every_rewrite(host, device):
    """the chain with ComputeBoW's vectors and the store's poses and rows fetched behind every rewrite: what the store holds is what the map holds
    (asserted inside the chain) and what the host chain holds; nothing else changes through the extra waits"""
    rec = device["probed"]
    diff = lc.first_difference(host["probed"], rec)
    assert diff is None, diff
    assert len(lc.stage(rec, "SearchAndFuse")["rows"]) == 12 and len(lc.stage(rec, "CorrectLoop: Sim3 propagation")["stored_poses"]) == 5
    assert lc.first_difference([("", lc.stage(rec, "ComputeBoW, read at once"))], [("", lc.stage(rec, "ComputeBoW"))]) is None
    strip = lambda r: [(n, {k: v for k, v in o.items() if k not in ("rows", "stored_poses")}) for n, o in r if n != "ComputeBoW, read at once"]
    diff = lc.first_difference(strip(device["jump"]), strip(rec))
    assert diff is None, diff


def test_rejected_pass_leaves_everything_as_it_was(host, device):
    rej, snaps = device["rejected"], device["snapshots"]
    diff = lc.first_difference(host["rejected"], rej)
    assert diff is None, diff
    last = lc.stages(rej, "Sim3Solver pass")[-1]
    assert last["no_more"] == [1] and lc.stage(rej, "ComputeSim3")["accepted"] is False
    assert len(snaps[0]) == len(snaps[1]) and snaps[0] == snaps[1], [a[0] for a, b in zip(*snaps) if a != b][:5]


def test_chain_twice_on_one_store(host, device):
    """the same store, covisibility, solver and optimiser handles after re-putting the scene, and after the other chains and the rejected pass ran on
    them (rows and poses rewritten by CorrectLoop, the index rebuilt): the same bits up to the global BA, which repeats within its bar"""
    diff = lc.first_difference(device["jump"], device["again"])
    assert diff is None, diff
    _gba_close("again", device["jump"], device["again"], host["gba_perturbed"]["jump"])


def test_candidates_in_one_call_equal_one_by_one(device):
    """SearchByBoW, Sim3Solver::iterate, SearchBySim3 and OptimizeSim3 with every candidate of a pass in one call per entry, against one call per candidate"""
    chain, single = device["jump"], device["single"]
    assert len(lc.stage(chain, "SearchByBoW")["n"]) >= 3 and len(lc.stage(chain, "OptimizeSim3 pass 1")["candidates"]) >= 2
    upto = [n for n, _ in chain].index("ComputeSim3") + 1
    same_part = chain[:upto] + [("ComputeBoW", lc.stage(chain, "ComputeBoW"))]
    assert [n for n, _ in single] == [n for n, _ in same_part]
    diff = lc.first_difference(same_part, single)
    assert diff is None, diff
