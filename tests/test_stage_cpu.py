"""CmsStage (cubemapslam_amd/csrc/cms_stage.h) is the device block + pinned block behind every host-buffer entry of the C-ABI: grown on demand,
never shrunk, and the one place that knows a block's capacity when a copy is made.  The header has no HIP in it; tests/emu/stage_emu.cpp drives it
with a counting malloc policy and exits non-zero unless a sufficient block is kept, an insufficient one becomes need + need / 2, the stream is
waited for before (and only before) a held block is freed, every block of 10 000 random reservations is freed exactly once, a failing allocation
leaves an empty block that the next call fills, up / back refuse a range one byte beyond either capacity, and zero-sized sides allocate nothing.
Built plain and with AddressSanitizer + UBSan, and each build run as a child process (the sanitizer runtimes are linked into the program)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "stage_emu.cpp")

BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_stage_emulation(build, tmp_path):
    exe = str(tmp_path / ("stage_emu_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + BUILDS[build] + [SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "stage_emu: ok" in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-4000:]
