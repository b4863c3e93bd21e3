"""The loop-closing composite on the CPU (tests/loop_cases.py): the reference chain (HostBackend: the host cores and numpy restatements every stage's
own GPU test compares against) accepts the loop of the synthetic scene by LoopClosing's own thresholds with margin; its glue equals the independent
float64 restatement tests/npref_loop_closing.py (every discrete output identical, floats inside measured bars); the chain recovers the drift and ends
on the ground truth; and the scene is tame (a 1e-12 m perturbation changes no discrete output).  The numbers printed here are the ones the header
of loop_cases.py records, and the bars the GPU test holds the device chain to."""
import numpy as np
import pytest

import loop_cases as lc
import npref_loop_closing as ref


@pytest.fixture(scope="module")
def sc():
    return lc.scene()


@pytest.fixture(scope="module")
def host(sc):
    be = lc.HostBackend()
    out = dict(jump=lc.run(sc, be, tree="jump", probe=True), split=lc.run(sc, be, tree="split", probe=True), fixed=lc.run(sc, be, tree="jump", probe=True, zw=False),
               rejected=lc.run_rejected(sc, be))
    be.close()
    return out


@pytest.fixture(scope="module")
def restated(sc):
    be = lc.HostBackend()
    go = lambda tree, zw: ref.run(sc, be, lc.DETECT, lc.CURRENT, lambda m, N: lc.solver_draws(sc, m, N), lc.PARENTS[tree], z_as_written=zw)
    out = dict(jump=go("jump", True), split=go("split", True), fixed=go("jump", False))
    be.close()
    return out


def test_scene_is_what_the_header_says(sc):
    kfs = sc["kfs"]
    assert len(kfs) == 12 and all(len(k["x"]) <= 400 for k in kfs)
    assert len(sc["X"]) == lc.NS + lc.NE
    c4 = kfs[lc.CURRENT]
    faces = set(int(f) for f in lc.synth.face_of_pixel(lc.F, c4["x"][c4["mp"] >= 0].astype(np.float64), c4["y"][c4["mp"] >= 0].astype(np.float64)))
    assert len(faces) >= 3, faces                                  # the shared points land on at least three cube faces of C4
    for k in kfs:                                                  # about a third of the key points hold no map point of two observations
        assert 0.25 <= float((k["mp"] < 0).mean()) <= 0.9, (k["name"], float((k["mp"] < 0).mean()))
    again = lc.scene()
    assert all(np.array_equal(a[f], b[f]) for a, b in zip(kfs, again["kfs"]) for f in ("x", "y", "octave", "desc", "mp", "R", "t"))      # deterministic


def test_reference_chain_accepts_the_loop_with_margin(sc, host):
    rec = host["jump"]
    E0, E1 = lc.NAMES.index("E0"), lc.NAMES.index("E1")
    d = lc.stage(rec, "DetectLoop C4")
    old = [m for m in d["enough"] if lc.NAMES[m][0] == "A"]
    matched = lc.stage(rec, "Scw")["matched"]
    bow = dict(zip(d["enough"], lc.stage(rec, "SearchByBoW")["n"]))
    passes = lc.stage(rec, "Scw")["passes"]
    opt = lc.stage(rec, "OptimizeSim3 pass %d" % passes)
    n_opt = dict(zip(opt["candidates"], opt["n_inliers"]))
    sbp = lc.stage(rec, "SearchByProjection(Scw)")
    fixed = lc.stage(rec, "SearchBySim3 pass %d, component 2" % passes)["n_found"]
    fusion, sf, links = lc.stage(rec, "CorrectLoop: loop fusion"), lc.stage(rec, "SearchAndFuse"), lc.stage(rec, "LoopConnections")
    eg, gba = lc.stage(rec, "OptimizeEssentialGraph"), lc.stage(rec, "GlobalBundleAdjustment")
    rej = host["rejected"]
    rej_bow = lc.stage(rej, "SearchByBoW")["n"]
    rej_last = lc.stages(rej, "Sim3Solver pass")[-1]
    print("C4's consistent candidates %s (matched %s); SearchByBoW %s; hypotheses of pass %d: OptimizeSim3 inliers %s; SearchBySim3 as written %s, with component 2 %s; "
          "after SearchByProjection(Scw) %d matches over %d loop points; loop fusion replaced %d added %d; SearchAndFuse replaced %d added %d; loop links %s; largest covisibility "
          "weight %d; essential graph (jump) %d edges, %d iterations; global BA %d points %d edges %d iterations; rejected pass: SearchByBoW %s, E0 walked %d iterations in %d passes"
          % ([lc.NAMES[m] for m in d["enough"]], lc.NAMES[matched], bow, passes, n_opt, lc.stage(rec, "SearchBySim3 pass %d" % passes)["n_found"], fixed, sbp["total"],
             len(sbp["loop_ids"]), len(fusion["replaced"]), len(fusion["added"]), len(sf["replaced"]), len(sf["added"]), links["links"], links["max_weight"], len(eg["edges"]),
             eg["iterations_run"], len(gba["points"]), len(lc.stage(rec, "CollectGlobalBA")["problem"]["e_pose"]), gba["iterations_done"], rej_bow, rej_last["iterations"][0],
             len(lc.stages(rej, "Sim3Solver pass"))))
    assert len(old) >= 2 and E0 in d["enough"] and matched in old          # the true side and the impostor are both consistent for C4
    assert bow[matched] >= 30 and bow[E0] >= 20
    assert len(opt["candidates"]) >= 2                                      # more than one hypothesis in a pass: the batched entries have company
    assert n_opt[matched] >= 30
    assert sbp["total"] >= 60 and sbp["accepted"]
    assert max(fixed) >= 8                                                  # the solver's s12 / R12 / t12 mean to the guided matcher what they mean to the solver
    assert len(fusion["replaced"]) >= 30 and len(sf["replaced"]) + len(sf["added"]) >= 30 and len(sf["added"]) >= 1
    assert all(len(l) >= 2 for l in links["links"] if l[0] == lc.CURRENT)   # C4 gained links across the loop
    old_side = [m for m, n in enumerate(lc.NAMES) if n[0] == "A"]
    assert links["weights"][np.ix_(old_side, old_side)].max() < 100 <= links["max_weight"]      # covisibility edges (minFeat = 100) on the current side only
    assert eg["iterations_run"] >= 2 and eg["chi2_final"][0] < eg["chi2_initial"][0]
    assert gba["iterations_done"] >= 2
    # the rejected pass: E1 below 20 matches (:266), E0 to bNoMore, false at :343-349
    assert rej_bow[0] >= 20 and rej_bow[1] < 20
    assert rej_last["no_more"] == [1] and rej_last["iterations"][0] == lc.stage(rej, "Sim3Solver set-up")["max_its"][0] and all(s == [0] for s in
                                                                                                                           [p["status"] for p in lc.stages(rej, "Sim3Solver pass")])
    assert lc.stage(rej, "ComputeSim3") == dict(accepted=False, passes=len(lc.stages(rej, "Sim3Solver pass")), at=":343-349")


def _against_restatement(rec, r, tree):
    """discrete outputs: equal; floats: the largest difference per quantity.  One count is left out: the essential graph's iterations on the "split"
    tree, where every edge agrees with the corrected poses and Levenberg starts at chi2 ~ 1e-14 -- how often it still finds a smaller number is
    noise by construction.  The "jump" tree's count, the one with an optimisation behind it, is asserted, and so is the global BA's on both."""
    passes = lc.stage(rec, "Scw")["passes"]
    sbp = lc.stage(rec, "SearchByProjection(Scw)")
    prop, fusion, sf, eg, fin = (lc.stage(rec, n) for n in ("CorrectLoop: Sim3 propagation", "CorrectLoop: loop fusion", "SearchAndFuse", "OptimizeEssentialGraph", "Final"))
    ints = lambda a: [int(v) for v in a]
    assert r["candidates"] == [lc.stage(rec, "DetectLoop %s" % lc.NAMES[m])["candidates"] for m in lc.DETECT]
    assert r["enough"] == lc.stage(rec, "DetectLoop C4")["enough"]
    assert r["bow_matches"] == lc.stage(rec, "SearchByBoW")["n"]
    su = lc.stage(rec, "Sim3Solver set-up")
    assert r["solvers"] == su["live"] and r["solver_N"] == su["N"] and r["indices1"] == [ints(a) for a in su["indices1"]]
    assert r["passes"] == passes == len(r["pass"])
    for k in range(passes):
        sv, p = lc.stage(rec, "Sim3Solver pass %d" % (k + 1)), r["pass"][k]
        assert [p[f] for f in ("live", "status", "no_more", "n_inliers", "iterations")] == [sv[f] for f in ("live", "status", "no_more", "n_inliers", "iterations")]
        assert p["masks"] == [ints(m) for m in sv["inliers"]]                                     # the solvers' inlier masks, in correspondence order
        ss, o = lc.stage(rec, "SearchBySim3 pass %d" % (k + 1)), lc.stage(rec, "OptimizeSim3 pass %d" % (k + 1))
        assert p["sim3_idx2"] == [ints(a) for a in ss["idx2"]] and p["n_found"] == ss["n_found"] and p["matches_searched"] == [ints(a) for a in ss["matches"]]
        assert p["keep"] == [ints(a) for a in o["keep"]] and p["opt_iterations"] == [ints(a) for a in o["iterations"]] and p["matches_optimised"] == [ints(a) for a in o["matches"]]
        assert r["hypotheses"][k] == list(zip(o["candidates"], o["n_inliers"]))
    assert r["matched"] == lc.stage(rec, "Scw")["matched"] and r["accepted"]
    assert r["loop_ids"] == ints(sbp["loop_ids"]) and r["matches"] == ints(sbp["matches"]) and r["total"] == sbp["total"]
    assert r["connected"] == prop["connected"] and r["corrected_ids"] == ints(prop["ids"])
    assert r["fused_replaced"] == [tuple(ints(x)) for x in fusion["replaced"]] and r["fused_added"] == [tuple(ints(x)) for x in fusion["added"]]
    assert r["sf_replaced"] == [tuple(ints(x)) for x in sf["replaced"]] and r["sf_added"] == [tuple(ints(x)) for x in sf["added"]]
    assert r["loop_connections"] == lc.stage(rec, "LoopConnections")["links"]
    assert r["edges"] == [tuple(ints(e)) for e in eg["edges"]]
    if tree == "jump":
        assert r["eg_iterations"] == eg["iterations_run"], (r["eg_iterations"], eg["iterations_run"])
    assert r["eg_ids"] == ints(eg["ids"]) and r["final_ids"] == ints(fin["ids"])
    gba_it = lc.stage(rec, "GlobalBundleAdjustment")["iterations_done"]
    assert r["gba_iterations"] == gba_it, (r["gba_iterations"], gba_it)
    worst = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    stored = np.stack([p[:12] for p in prop["stored_poses"]])
    eg_stored = np.stack([p[:12] for p in eg["stored_poses"]])
    return dict(Scw=worst(r["Scw"], lc.stage(rec, "Scw")["Scw"]), corrected_pos=worst(r["corrected_pos"], prop["pos"]), corrected_poses=worst(r["corrected_poses"], stored),
                eg_pos=worst(r["eg_pos"], eg["pos"]), eg_poses=worst(r["eg_poses"], eg_stored[np.argsort(eg["vertex_kf"])]), final_pos=worst(r["final_pos"], fin["pos"]),
                final_centres=worst(r["final_centres"], fin["centres"]))


@pytest.mark.parametrize("tree", ["jump", "split", "fixed"])
def test_glue_equals_the_float64_restatement(host, restated, tree):
    """"fixed": the "jump" chain with SearchBySim3 reading component 2, the one in which that matcher's answers are written into the match list"""
    m = _against_restatement(host[tree], restated[tree], "jump" if tree == "fixed" else tree)
    if tree == "fixed":
        found = lc.stage(host[tree], "SearchBySim3 pass 1")["n_found"]
        assert max(found) >= 8 and lc.stage(host[tree], "ComputeSim3")["accepted"], found
    print("host chain against the float64 restatement of the glue (%s): %s" % (tree, ", ".join("%s %.3g" % kv for kv in m.items())))
    for k, v in m.items():
        assert v <= lc.GLUE_BARS[tree][k], (k, v, lc.GLUE_BARS[tree][k])


def test_chain_recovers_the_drift_and_ends_on_the_truth(sc, host, restated):
    r = restated["split"]
    scw_ref = lc.scw_error(sc, r["Scw"])
    ids = np.array(r["final_ids"]); phys = np.where(ids >= lc.E_ID, ids - lc.E_ID + lc.NS, ids % lc.CUR_ID)
    true_c = np.stack([-(R.T @ t) for R, t in sc["true_poses"]])
    rms = lambda d: float(np.sqrt((d * d).sum(1).mean()))
    ref_c, ref_p = rms(r["final_centres"].astype(np.float64) - true_c), rms(r["final_pos"].astype(np.float64) - sc["X"][phys])
    before_c, before_p = lc.truth_error(sc, None, "ACE")
    got_c, got_p = lc.truth_error(sc, host["split"], "ACE")
    got_scw = lc.scw_error(sc, lc.stage(host["split"], "Scw")["Scw"])
    nothing = lc.scw_error(sc, np.hstack([np.eye(3), np.zeros((3, 1))]))
    print("truth (RMS metres, nothing removed): Scw restatement %.3g host %.3g identity %.3g; centres before %.3g restatement %.3g host %.3g; points before %.3g restatement %.3g "
          "host %.3g; with the jump tree the host chain ends at centres %.3g points %.3g (old and current side)" % ((scw_ref, got_scw, nothing, before_c, ref_c, got_c, before_p,
                                                                                                                   ref_p, got_p) + lc.truth_error(sc, host["jump"], "AC")))
    # the bars are twice the restatement's own error; what the header records must be what is measured here
    assert lc.SCW_BAR >= 2 * scw_ref * 0.999 and lc.CENTRE_BAR >= 2 * ref_c * 0.999 and lc.POINT_BAR >= 2 * ref_p * 0.999
    assert lc.SCW_BAR <= 2 * scw_ref * 1.3 and lc.CENTRE_BAR <= 2 * ref_c * 1.3 and lc.POINT_BAR <= 2 * ref_p * 1.3
    assert got_scw <= lc.SCW_BAR and got_c <= lc.CENTRE_BAR and got_p <= lc.POINT_BAR
    assert nothing >= 20 * lc.SCW_BAR and before_c >= 20 * lc.CENTRE_BAR and before_p >= 20 * lc.POINT_BAR      # doing nothing does not pass


def test_scene_is_tame(sc, host):
    """the chain from points moved by 1e-12 m: every discrete output unchanged"""
    be = lc.HostBackend()
    sc2 = lc.scene(perturb=1e-12)
    assert np.abs(sc2["X"] - sc["X"]).max() > 0
    for tree in ("jump", "split"):
        assert lc.discrete(lc.run(sc2, be, tree=tree, probe=True)) == lc.discrete(host[tree]), tree
    assert lc.discrete(lc.run(sc2, be, tree="jump", probe=True, zw=False)) == lc.discrete(host["fixed"])
    assert lc.discrete(lc.run_rejected(sc2, be)) == lc.discrete(host["rejected"])
    be.close()


def test_first_difference_names_the_stage(host):
    rec = host["jump"]
    assert lc.first_difference(rec, rec) is None
    k = [n for n, _ in rec].index("Scw")
    bent = list(rec)
    o = dict(rec[k][1]); o["Scw"] = o["Scw"].copy(); o["Scw"][0, 0] = np.nextafter(o["Scw"][0, 0], np.float32(2))      # one unit in the last place
    bent[k] = ("Scw", o)
    assert "stage %d (Scw)" % k in lc.first_difference(rec, bent) and ".Scw" in lc.first_difference(rec, bent)
    assert lc.first_difference(rec, rec[:-1]) is not None
