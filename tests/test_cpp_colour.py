"""The headless application's --color (the reference application's fuse_color branch through the roo:: overloads): the brick
summary and the fused launches change neither the depth nor the colour image of the last rendering, with known and with tracked
poses; the colour image is not the grey run's shade; --save-mesh writes the colour volume's values."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
BASE = ["--color", "--res", "64", "--width", "160", "--height", "120", "--frames", "6"]


def _make(target):
    subprocess.check_call(["make", "-C", APPS, target], stdout=subprocess.DEVNULL)


def run(args):
    out = subprocess.run([os.path.join(APPS, "kinectfusion_headless")] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"last raycast hits (\d+)/\d+.*depth checksum ([0-9a-f]{16}), (\w+) checksum ([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    return dict(hits=int(m.group(1)), depth=m.group(2), kind=m.group(3), image=m.group(4), out=out.stdout)


def test_headless_color_option_builds():
    _make("kinectfusion_headless")
    src = open(os.path.join(APPS, "kinectfusion_headless.cpp")).read()
    assert "--color" in src and "SdfReset(colorVol)" in src and "SaveMesh(save_mesh, vol, colorVol)" in src


@pytest.mark.gpu
@pytest.mark.parametrize("poses", [[], ["--track"]])
def test_cpp_headless_colour_hashes_do_not_depend_on_the_fast_paths(poses):
    _make("kinectfusion_headless")
    ref = run(BASE + poses)
    assert ref["kind"] == "colour" and ref["hits"] > 160 * 120 // 4
    for extra in (["--summary"], ["--fused-launches"], ["--summary", "--fused-launches"]):
        got = run(BASE + poses + extra)
        assert (got["depth"], got["image"]) == (ref["depth"], ref["image"]), (extra, got["out"], ref["out"])
        assert ("(brick summary)" in got["out"]) == ("--summary" in extra)
    grey = run(BASE[1:] + poses)
    assert grey["kind"] == "shade" and grey["image"] != ref["image"]


@pytest.mark.gpu
def test_cpp_headless_colour_save_mesh(tmp_path):
    _make("kinectfusion_headless")
    prefix = str(tmp_path / "model")
    got = run(BASE + ["--save-mesh", prefix])
    m = re.search(r"mesh: (\d+) triangles written to (\S+)\.ply", got["out"])
    assert m and m.group(2) == prefix, got["out"]
    raw = open(prefix + ".ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    assert nv == 3 * int(m.group(1)) > 300
    assert all(b"property float %s" % c in head for c in (b"red", b"green", b"blue", b"alpha"))
    v = np.frombuffer(body[:nv * 40], dtype="<f4").reshape(nv, 10)
    grey = v[:, 6]
    assert np.isfinite(v).all() and (grey >= 0).all() and (grey <= 1).all() and np.ptp(grey) > 0.02   # the albedo, not the reset value
