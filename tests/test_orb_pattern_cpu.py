"""The rBRIEF test pattern (a10: steered BRIEF) is reference-held DATA: 256 x 4 integers in src/ORBExtractor.cpp:121-379 (`bit_pattern_31_`), committed here as
generated tables for the product (cubemapslam_amd/csrc/orb_pattern.inc) and the oracle (oracle/orc_pattern.inc) by tools/gen_orb_pattern.py.  Both tables must be
the same 1024 numbers, their digest must be the one recorded when they were generated, and they must be the reference's numbers as its source holds them
(tests/golden/reference_constants.npz, read out of the reference's text by tests/golden/make_reference_fixtures.py)."""
import hashlib
import os
import re

import numpy as np

import refdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGEST = "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"


def _table(path):
    txt = open(path).read()
    body = txt[txt.index("{") + 1:txt.rindex("}")]
    v = np.array([int(x) for x in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024, (path, v.size)
    return v


def test_product_and_oracle_hold_the_same_pattern_and_its_digest_is_the_recorded_one():
    a = _table(os.path.join(ROOT, "cubemapslam_amd", "csrc", "orb_pattern.inc"))
    b = _table(os.path.join(ROOT, "oracle", "orc_pattern.inc"))
    assert np.array_equal(a, b)
    assert np.abs(a).max() <= 15                       # every test point lies inside the 31 x 31 patch
    assert hashlib.sha256(a.astype(np.int8).tobytes()).hexdigest() == DIGEST


def test_pattern_equals_the_reference_source_where_it_is_present():
    nums = refdata.reference_constants()["orb_bit_pattern_31"]
    assert nums.size == 1024
    assert np.array_equal(nums.astype(np.int64), _table(os.path.join(ROOT, "cubemapslam_amd", "csrc", "orb_pattern.inc")))


def test_the_oracles_named_constants_are_the_references_where_it_is_present():
    """TH_HIGH / TH_LOW / HISTO_LENGTH (ORBMatcher.cpp:42-44: 12 bins here, not ORB-SLAM2's 30), PATCH_SIZE / HALF_PATCH_SIZE / EDGE_THRESHOLD
    (ORBExtractor.cpp:43-45), the chi2 gate 5.991 and the Huber widths sqrt(5.991) of PoseOptimization / LocalBundleAdjustment (Optimizer.cpp:77,300,384,411):
    read out of the reference's text (tests/golden/reference_constants.npz) and out of the oracle's sources, compared as numbers."""
    ref = refdata.reference_constants()
    def const(path, name):
        m = re.search(r"\b%s\s*=\s*(-?[0-9.]+)" % re.escape(name), open(path).read())
        assert m, (path, name)
        return float(m.group(1))
    orc = os.path.join(ROOT, "oracle")
    for name, orc_file in (("TH_HIGH", None), ("TH_LOW", "orc_track.cpp"), ("HISTO_LENGTH", "orc_track.cpp"),
                           ("PATCH_SIZE", "orc_orb.cpp"), ("HALF_PATCH_SIZE", "orc_orb.cpp"), ("EDGE_THRESHOLD", "orc_orb.cpp")):
        r = float(ref[name])
        if orc_file:
            assert const(os.path.join(orc, orc_file), name) == r, name
        else:
            assert r == 100.0                      # (TH_HIGH is an argument of the oracle's matchers: the tests pass 100)
    assert list(ref["deltaMono_sqrt_of"]) == [5.991] and list(ref["thHuberMono_sqrt_of"]) == [5.991] and list(ref["local_ba_chi2_gates"]).count(5.991) >= 2
    ba = open(os.path.join(orc, "orc_ba.cpp")).read()
    assert ba.count("std::sqrt(5.991)") >= 2 and "c2 > 5.991" in ba and "chi2 > 5.991f" in ba
