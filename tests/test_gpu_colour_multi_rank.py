"""Colour mode on Z-slabs under real collectives: two and three ranks sharing the box's one GPU over gloo (at most three GPU
processes), SlabPipeline(color=True) with the Python driver and with the C driver against the single-GPU colour pipeline.  See
tests/mp_colour_slab_gpu.py."""
import os
import socket
import subprocess
import sys

import pytest

import kfx_testlib as T

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world,halo,raycast", [(2, "exchange", "exact"), (3, "recompute", "exact"), (3, "exchange", "composite")])
def test_gpu_colour_slab_pipeline_ranks_sharing_one_gpu(world, halo, raycast):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(T.ROOT, "tests", "mp_colour_slab_gpu.py"), halo, raycast]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert out.returncode == 0 and out.stdout.count("MP_OK") == world, out.stdout[-3000:] + out.stderr[-3000:]
