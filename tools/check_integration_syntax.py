"""integration/CubemapHipBridge.cpp + OrbExtractorHip.h are written against the reference's REAL headers (Frame.h, KeyFrame.h, MapPoint.h, Map.h,
Converter.h, CamModelGeneral.h, ORBMatcher.h) and cannot be built without OpenCV / Eigen.  This check stops typos from shipping: `g++ -fsyntax-only`
over the bridge, with the reference's include/ directory as a maintainer would have it after the integration step (ORBExtractor.h replaced by
OrbExtractorHip.h) and DECLARATIONS-ONLY stand-ins for OpenCV / Eigen / g2o / DBoW2 under tests/stubs/.  It pins nothing about parity -- no body
is compiled into anything, nothing is linked or run.  A second pass breaks one C-ABI call in each file and must fail: both files are really parsed.

    python tools/check_integration_syntax.py REFERENCE_CHECKOUT/include

The reference's headers are not part of this repository, so the check is a maintainer's tool rather than a test."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def syntax_check(ref_inc, work, integration_dir):
    inc = os.path.join(work, "refinc")
    os.mkdir(inc)
    for f in os.listdir(ref_inc):
        if f != "ORBExtractor.h":
            os.symlink(os.path.join(ref_inc, f), os.path.join(inc, f))
    shutil.copy(os.path.join(integration_dir, "OrbExtractorHip.h"), os.path.join(inc, "ORBExtractor.h"))      # integration/README.md: the header the extractor's users include
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", integration_dir, "-I", os.path.join(ROOT, "include"),
           "-I", inc, os.path.join(integration_dir, "CubemapHipBridge.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def main(ref_inc):
    with tempfile.TemporaryDirectory() as td:
        os.mkdir(os.path.join(td, "ok"))
        r = syntax_check(ref_inc, os.path.join(td, "ok"), os.path.join(ROOT, "integration"))
        if r.returncode != 0 or "error" in r.stderr:
            print(r.stderr[-4000:])
            return 1
        # a misspelt C-ABI call in either file must fail the check
        for i, (fname, old, new) in enumerate((("OrbExtractorHip.h", "cms_extract(ctx,", "cms_extrakt(ctx,"), ("CubemapHipBridge.cpp", "cms_area_grid(ctx, 1)", "cms_area_grid(ctx)"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_fuse_search_sets(store, 2, set_off,", "cms_kfstore_fuse_search_sets(store, set_off,"),
                                               ("CubemapHipBridge.cpp", "cms_pnp_iterate_frames(pnp, frameCtx, (int)n, jobs.data())", "cms_pnp_iterate_frame(pnp, frameCtx, (int)n, jobs.data())"),
                                               ("CubemapHipBridge.cpp", "cms_init_two_view_frames(init, frameCtx, 1, &q)", "cms_init_two_view_frame(init, frameCtx, 1, &q)"),
                                               ("CubemapHipBridge.cpp", "cms_sim3_iterate(sim3, frameCtx, (int)n, jobs.data())", "cms_sim3_iterat(sim3, frameCtx, (int)n, jobs.data())"),
                                               ("CubemapHipBridge.cpp", "cms_kfdb_detect(store, frameCtx, 1, &job,", "cms_kfdb_detect(store, 1, &job,"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_search_by_bow_keyframes(store, ctx, (int)jobs.size(),",
                                                "cms_kfstore_search_by_bow_keyframes(store, (int)jobs.size(),"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_search_by_sim3(store, ctx, (int)jobs.size(),", "cms_kfstore_search_by_sim3(store, (int)jobs.size(),"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_fuse_search_sim3(store, ctx, 1, set_off,", "cms_kfstore_fuse_search_sim3(store, 1, set_off,"),
                                               ("CubemapHipBridge.cpp", "cms_covis_votes(covis, frameCtx, 1, id_off,", "cms_covis_votes(covis, 1, id_off,"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_update_map_points(store, (int)up_slot.size(),", "cms_kfstore_update_map_points(store,"),
                                               ("CubemapHipBridge.cpp", "cms_mpstore_refresh(mps, covis, (int)n,", "cms_mpstore_refresh(mps, (int)n,"),
                                               ("CubemapHipBridge.cpp", "cms_search_local_points_ids(ctx, 0, pose15, mps, n,", "cms_search_local_points_ids(ctx, 0, pose15, n,"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_fuse_search_sets_ids(store, mps, 2, set_off,", "cms_kfstore_fuse_search_sets_ids(store, 2, set_off,"),
                                               ("CubemapHipBridge.cpp", "cms_mpstore_culling(mps, covis, 1, off,", "cms_mpstore_culling(mps, 1, off,"),
                                               ("CubemapHipBridge.cpp", "cms_kfstore_scene_median_depth(store, mps, 1, &slot,", "cms_kfstore_scene_median_depth(store, 1, &slot,"))):
            d = os.path.join(td, "broken_%d" % i)
            shutil.copytree(os.path.join(ROOT, "integration"), d)
            src = open(os.path.join(d, fname)).read()
            if old not in src:
                print("%s no longer contains %r: update this check" % (fname, old))
                return 1
            open(os.path.join(d, fname), "w").write(src.replace(old, new, 1))
            sub = os.path.join(td, "t_%d" % i)
            os.mkdir(sub)
            r = syntax_check(ref_inc, sub, d)
            if r.returncode == 0 or "error" not in r.stderr:
                print("a broken %s passed the check: it is not parsed" % fname)
                return 1
    print("integration/ parses against %s" % ref_inc)
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit("usage: check_integration_syntax.py REFERENCE_CHECKOUT/include")
    sys.exit(main(sys.argv[1]))
