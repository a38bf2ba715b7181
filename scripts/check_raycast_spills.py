#!/usr/bin/env python3
"""Register-spill guard for raycast.hip (CPU only: hipcc cross-compiles gfx950).

The march through the class tables is a chain of dependent instructions issued by one or two waves per SIMD; a scalar
register the allocator could not keep is parked in a VGPR lane and comes back with a v_readlane on that chain.  The LDS-mode
class kernels had grown to 47-55 spilled SGPRs.  This script compiles raycast.hip with the Makefile's flags and hipcc's
resource-usage remarks and fails when
  * any k_raycast_* kernel uses scratch or spills VGPRs,
  * any of them spills more SGPRs than it did before this guard existed (BEFORE), or
  * one of the LDS-mode class kernels of the product path spills more than the number pinned here (PINNED: what they reach
    with the table descriptors parked in vector registers and no level derived in the prologue -- the two march kernels as few
    as their global-table twins; the pyramid-levels kernel, which also carries its level's descriptors, 14 / 16).
Usage: python scripts/check_raycast_spills.py"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kangaroo_amd", "csrc")


def makefile_flags(obj="raycast.o"):
    """CXXFLAGS of csrc/Makefile plus what it adds for `obj` (EXTRA, the A/B hook, left out)"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    found = [re.search(rx, text, re.M) for rx in (r"^CXXFLAGS\s*:=\s*(.*)$", r"^%s:\s*CXXFLAGS\s*\+=\s*(.*)$" % re.escape(obj), r"^ARCH\s*\?=\s*(\S+)")]
    assert all(found), "csrc/Makefile: 'CXXFLAGS :=', '%s: CXXFLAGS +=' or 'ARCH ?=' not found -- makefile_flags() reads those three lines" % obj
    base, extra, arch = (m.group(1) for m in found)
    flags = (base + " " + extra).replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-function")]


# SGPR spills per kernel before this guard (same flags, same compiler); kernels not listed had none
BEFORE = {
    "k_raycast_sdf<RayF32,1>": 4,
    "k_raycast_sdf_classes<RayF32,1>": 2, "k_raycast_sdf_classes<RayF32,0>": 47,
    "k_raycast_sdf_classes<RayF16,1>": 8, "k_raycast_sdf_classes<RayF16,0>": 51,
    "k_raycast_sdf_classes_count<RayF32,1>": 18, "k_raycast_sdf_classes_count<RayF32,0>": 57,
    "k_raycast_sdf_classes_count<RayF16,1>": 24, "k_raycast_sdf_classes_count<RayF16,0>": 61,
    "k_raycast_sdf_levels_classes<RayF32>": 55, "k_raycast_sdf_levels_classes<RayF16>": 55,
}
# the LDS-mode class kernels (the headline's, its half-cell twin, the pyramid levels' one launch, fp32 and half): what they reach now
PINNED = {
    "k_raycast_sdf_classes<RayF32,0>": 2,
    "k_raycast_sdf_classes<RayF16,0>": 8,
    "k_raycast_sdf_levels_classes<RayF32>": 14,
    "k_raycast_sdf_levels_classes<RayF16>": 16,
}


def short_name(mangled):
    """_ZN3kfx21k_raycast_sdf_classesINS_6RayF32ELb0EEEv... -> k_raycast_sdf_classes<RayF32,0>"""
    m = re.match(r"_ZN3kfx\d+(k_raycast\w*?)(?:I(.*?)EEv|E)", mangled)
    if not m:
        return mangled
    name, targs = m.group(1), m.group(2)
    if not targs:
        return name
    args = re.findall(r"NS_\d+(Ray\w\d\d)|Lb([01])", targs)
    return "%s<%s>" % (name, ",".join(a or b for a, b in args))


def resource_usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc] + makefile_flags() + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                                            "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "raycast.hip")],
                         capture_output=True, text=True, check=True)
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return {short_name(k): v for k, v in kernels.items() if "k_raycast" in k}


def main():
    res = resource_usage()
    bad = []
    for k in sorted(res):
        v = res[k]
        limit = min(BEFORE.get(k, 0), PINNED.get(k, 1 << 30))
        flag = ""
        if v.get("ScratchSize", 0) or v.get("VGPRs Spill", 0):
            flag = "  <-- scratch / VGPR spills"
        elif v.get("SGPRs Spill", 0) > limit:
            flag = "  <-- more than %d SGPR spills" % limit
        if flag:
            bad.append(k)
        print("  %-48s VGPRs %3d  SGPR spills %2d (limit %2d)  scratch %d%s" % (k, v.get("VGPRs", -1), v.get("SGPRs Spill", -1), limit, v.get("ScratchSize", -1), flag))
    missing = [k for k in PINNED if k not in res]
    print("%d k_raycast kernels, %d over their spill limits, %d pinned kernels missing" % (len(res), len(bad), len(missing)))
    return 1 if (bad or missing or not res) else 0


if __name__ == "__main__":
    sys.exit(main())
