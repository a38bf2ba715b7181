"""The host side of the ring in which the class-table builds publish their counts (kangaroo_amd/csrc/summary_ring_host.h): slot
packing, build stamps, ring slots and the bounded wait the tracked RaycastSdf steers by, exercised by the stand-alone program
scripts/summary_ring_host_check.cpp under the address and undefined-behaviour sanitizers.  No GPU, no library: a host compiler only."""
import os
import subprocess

import kfx_testlib as T


def test_the_ring_host_check_program_passes_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "summary_ring_host_check")
    src = os.path.join(T.ROOT, "scripts", "summary_ring_host_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "summary_ring_host_check: ok" in out.stdout, out.stdout + out.stderr


def test_the_header_is_host_only():
    """It must compile without HIP (the check program does), so it includes nothing of the device side."""
    text = open(os.path.join(T.ROOT, "kangaroo_amd", "csrc", "summary_ring_host.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"], includes
