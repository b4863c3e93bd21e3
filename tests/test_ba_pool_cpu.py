"""The per-device caches of the local-BA host code (cubemapslam_amd/csrc/cms_ba_pool.h: idle streams and events, device slabs, pinned blocks) are the
one piece of the library that every host thread runs concurrently.  The header has no HIP in it; tests/emu/ba_pool_emu.cpp drives it with fake handles
and exits non-zero unless the best-fit rule, the caps, drain, the device range, the handle lists' maxima and the accounting of 16 threads x 20 000
random operations all hold.  Built three ways -- plain, AddressSanitizer + UBSan, ThreadSanitizer -- and each build run as a child process (the
sanitizer runtimes are linked into the program)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "ba_pool_emu.cpp")

BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_pool_emulation(build, tmp_path):
    exe = str(tmp_path / ("ba_pool_emu_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + BUILDS[build] + [SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ba_pool_emu: ok" in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-4000:]
