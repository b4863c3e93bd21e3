"""One context's CmsStage (csrc/cms_stage.h: its scratch block and its pinned block) is shared by every host-buffer entry that runs on the context.
Entries of different kinds and sizes, one after the other on ONE context -- a small block, larger ones, the largest, then the small ones again in
blocks kept from the largest -- must each return what the same call returns on a fresh context.  Call against call: there is no tolerance."""
import numpy as np
import pytest

import npref_vocab
import reloc_cases
import vocab_cases as vc
from cubemapslam_amd import api, synth
from test_gpu_search_by_bow import CASES, _place, hand_built

pytestmark = pytest.mark.gpu


def _context():
    return api.Context(synth.camera("lafida", reloc_cases.F_HAND), nfeatures=1000, max_batch=2)


def test_entries_share_one_contexts_blocks():
    tree = vc.case_tree("k10_L3")
    vocab = api.Vocabulary.from_dict(tree)
    d1, d4097 = vc.descriptors(71, tree, 1), vc.descriptors(72, tree, 4097)      # 4097: one above a 4096 row, the largest block of the sequence
    kf, skip, fk, fd, ffv, nnr, ori = hand_built(max(CASES, key=lambda c_: len(c_[1])))
    K, keep = api.make_keyframe(kf)
    rc = [case for name, case, *_ in reloc_cases.hand_cases() if name == "minority bin removed"][0]
    rk = np.zeros(len(rc["kx"]), api.KP_DTYPE); rk["x"] = rc["kx"]; rk["y"] = rc["ky"]; rk["octave"] = rc["koct"]; rk["angle"] = rc["kangle"]

    def prepared():
        c = _context()
        _place(c, 0, rk, rc["kdesc"]); _place(c, 1, fk, fd)
        c.area_grid(1)
        return c

    def transform(c, d):
        return ("bow", vocab.transform(c, d, 1))

    def by_bow(c):
        return ("idx",) + api.search_by_bow(c, 1, len(fk), ffv, K, skip=skip, nnratio=nnr, check_orientation=ori)

    def by_projection(c):
        kp_mp = rc["kp_mp"].copy()
        m, n = c.search_by_projection_keyframe(0, rc["pose12"], rc["kf_angle"], rc["pos"], rc["min_dist"], rc["max_dist"], rc["desc"], kp_mp, th=rc["th"],
                                               orb_dist=rc["orb"], check_ori=rc["ori"])
        return ("idx", m, n, kp_mp)

    first = [lambda c: transform(c, d1), by_bow, by_projection]
    calls = first + [lambda c: transform(c, d4097)] + first

    def same(want, got, what):
        if want[0] == "bow":
            diff = npref_vocab.first_difference(want[1], got[1])
            assert diff is None, (what, diff)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(want[1:], got[1:])), (what, want, got)

    try:
        want = []
        for call in calls[:4]:
            c = prepared()
            try:
                want.append(call(c))
            finally:
                c.close()
        want += want[:3]
        assert want[1][2] == 11 and want[2][2] == 7 and len(want[3][1]["node_feat"]) > 2000      # (the cases' own expectations: the calls did work)
        c = prepared()
        try:
            for i, (call, w) in enumerate(zip(calls, want)):
                same(w, call(c), "call %d" % i)
        finally:
            c.close()
    finally:
        vocab.close()
