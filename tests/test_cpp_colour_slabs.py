"""Colour mode on Z-slabs driven from C++ only (apps/kinectfusion_slabs --color -> include/kangaroo/SlabVolume.h ->
include/kfx_slab_color.h): rank threads of one process sharing the GPU.  Every compared run -- 2 / 3 / 4 / 8 ranks, ghost planes
exchanged or recomputed, 1 or 4 row-tiles, the roo:: calls or one kfx_slab_frame_step per frame, pipelined frames or not, both
in-process transports -- ends with the depth, normal and colour images, the SDF volume and the colour volume of the one-rank run, bit
for bit (checksums).  The cross product of the options would be several hundred launches; the dozen below touch every value of every
option."""
import os
import re
import struct
import subprocess

import pytest

import kfx_testlib as T

APP = os.path.join(T.ROOT, "apps", "kinectfusion_slabs")
pytestmark = pytest.mark.gpu

COMMON = ("--res", 128, "--frames", 4, "--width", 320, "--height", 240)
_ref = {}


def run(*args):
    out = subprocess.run([APP] + [str(a) for a in COMMON + args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"checksums depth=(\w+) norm=(\w+) img=(\w+) volume=(\w+) history=(\w+) hits=(\d+) ranks_agree=(\d)", out.stdout)
    assert m, out.stdout
    c = re.search(r" colour=([0-9a-f]{8})$", out.stdout, re.M)
    return dict(depth=m.group(1), norm=m.group(2), img=m.group(3), volume=m.group(4), history=m.group(5), hits=int(m.group(6)), agree=int(m.group(7)),
                colour=c.group(1) if c else None, text=out.stdout)


def reference():
    """the one-rank colour run and the one-rank grey run, once"""
    if not _ref:
        _ref["colour"] = run("--ranks", 1, "--raycast", "exact", "--color")
        _ref["grey"] = run("--ranks", 1, "--raycast", "exact")
    return _ref["colour"], _ref["grey"]


def test_cpp_colour_one_rank_renders_colour():
    """The colour run's img is not the grey run's.  Its depth, normals and SDF volume are not compared with the grey run's: the colour
    SdfFuse updates a voxel only where BOTH cameras see it (the reference's fuse_color), and the colour camera stands 25 mm beside the
    depth camera, so the colour run leaves a margin of voxels untouched that the grey run integrates."""
    ref, grey = reference()
    assert ref["agree"] == 1 and ref["hits"] > 320 * 240 // 3 and ref["colour"] is not None
    assert grey["agree"] == 1 and grey["hits"] > 320 * 240 // 3 and grey["colour"] is None
    assert ref["img"] != grey["img"], "the colour run's img is the grey run's Phong shade"


# (ranks, halo, tiles, driver, pipeline, transport): every value of every option at least once
RUNS = [(2, "exchange", 1, "roo", 0, "threads"), (3, "recompute", 4, "roo", 0, "threads-p2p"), (4, "exchange", 4, "frame", 0, "threads"),
        (8, "recompute", 1, "frame", 3, "threads-p2p"), (2, "recompute", 4, "frame", 3, "threads"), (3, "exchange", 1, "frame", 0, "threads-p2p"),
        (4, "recompute", 1, "roo", 0, "threads-p2p"), (8, "exchange", 4, "frame", 0, "threads"), (3, "exchange", 4, "frame", 3, "threads"),
        (1, "exchange", 4, "frame", 0, "threads")]


@pytest.mark.parametrize("ranks,halo,tiles,driver,pipeline,transport", RUNS)
def test_cpp_colour_slabs_equal_the_one_rank_run(ranks, halo, tiles, driver, pipeline, transport):
    ref, _ = reference()
    args = ["--ranks", ranks, "--raycast", "exact", "--color", "--halo", halo, "--tiles", tiles, "--transport", transport]
    if driver == "frame":
        args += ["--driver", "frame"]
    if pipeline:
        args += ["--pipeline", pipeline]
    got = run(*args)
    assert got["agree"] == 1
    for k in ("depth", "norm", "img", "volume", "colour", "history", "hits"):
        assert got[k] == ref[k], (k, got["text"], ref["text"])


@pytest.mark.parametrize("ranks", [3, 4])
def test_cpp_colour_slabs_composite_runs_and_ranks_agree(ranks):
    """The composite variant has no kernel of its own: every rank renders its local view in colour, the merge carries img.  The fused
    volumes are the one-rank run's; the images are the composite's (the march restarts at each slab), the same from the roo:: calls
    and from kfx_slab_frame_step."""
    ref, _ = reference()
    ops = run("--ranks", ranks, "--raycast", "composite", "--color")
    got = run("--ranks", ranks, "--raycast", "composite", "--color", "--driver", "frame")
    for r in (ops, got):
        assert r["agree"] == 1 and r["hits"] > 320 * 240 // 3
        assert r["volume"] == ref["volume"] and r["colour"] == ref["colour"]
    for k in ("depth", "norm", "img", "hits"):
        assert got[k] == ops[k], (k, got["text"], ops["text"])


def ply_header(path):
    with open(path, "rb") as f:
        head = f.read(1024)
    return head[:head.index(b"end_header")].decode().split("\n")


def test_cpp_colour_slabs_save_mesh_writes_colours(tmp_path):
    prefix = str(tmp_path / "room")
    got = run("--ranks", 3, "--raycast", "exact", "--color", "--save-mesh", prefix)
    total = int(re.search(r"mesh: (\d+) triangles", got["text"]).group(1))
    assert total > 1000
    seen = 0
    for r in range(3):
        path = "%s.r%d.ply" % (prefix, r)
        head = ply_header(path)
        for name in ("red", "green", "blue", "alpha"):
            assert "property float %s" % name in head, (path, head)
        nv = int([ln for ln in head if ln.startswith("element vertex")][0].split()[-1])
        seen += nv // 3
        if nv:   # the first vertex: x y z nx ny nz r g b a, a grey level in (0, 1) with alpha 1
            with open(path, "rb") as f:
                data = f.read()
            off = data.index(b"end_header\n") + len(b"end_header\n")
            v = struct.unpack("<10f", data[off:off + 40])
            assert v[6] == v[7] == v[8] and 0.0 < v[6] < 1.0 and v[9] == 1.0, v
    assert seen == total
