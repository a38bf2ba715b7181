"""bench.py --gpus 1 on the GPU: a plain run times the headline alone and prints it; --dump-outputs writes what the last timed
step computed, the same bits in two runs with the same arguments (the volume is reset after the clock-dependent priming);
--full adds the figures reported beside the headline.  Small volumes and short priming: the shape of the line, not the figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T

BENCH = os.path.join(T.ROOT, "bench.py")
QUICK = ["--gpus", "1", "--res", "128", "--prime-seconds", "0.05", "--prime-cap-seconds", "0.3"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KFX_BENCH_BACKEND")}
    out = subprocess.run([sys.executable, BENCH] + QUICK + list(args), capture_output=True, text=True, timeout=timeout, cwd=T.ROOT, env=env)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [["--math", "exact"], ["--math", "fast", "--summary", "on"]], ids=["exact", "fast_tables"])
def test_gpu_bench_plain_run_dumps_the_same_outputs_twice(tmp_path, numerics):
    runs = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        line = _bench(["--steps", "5", "--warmup", "2", "--dump-outputs", d] + numerics)
        assert all(key in line for key in HEADLINE) and line["steps"] == 5 and line["warmup"] == 2
        assert line["metric"] == "kinectfusion_frames_per_sec_640x480_to_512cubed_tsdf" and line["unit"] == "frames/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32"
        assert abs(line["value"] * line["ms_per_step"] - 1e3) < 10.0   # both from the same K timed steps (rounded)
        for extra in ("roofline", "cpu_baseline", "sdf_fuse_other_mode", "plain_variant", "room_variant", "summary"):
            assert extra not in line
        assert line["config"]["restart"]["frames"] > 0 and line["outputs"]["dir"] == d
        files = sorted(os.listdir(d))
        assert files == line["outputs"]["files"]
        arrays = {f: np.load(os.path.join(d, f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["raycast_depth.npy"].shape == arrays["raycast_depth_finite.npy"].shape == (480, 640)
        hit = arrays["raycast_depth_finite.npy"] == 1   # pixels with a hit: finite depth; elsewhere 0 beside a 0 in the mask
        assert hit.sum() > 1000 and (arrays["raycast_depth.npy"][hit] > 0).all() and not arrays["raycast_depth.npy"][~hit].any()
        assert arrays["volume_sample.npy"].shape == (1 << 20, 2) and arrays["volume_sample_finite.npy"].shape == (1 << 20,)
        runs.append(arrays)
    for f in runs[0]:
        assert runs[0][f].tobytes() == runs[1][f].tobytes(), f


@pytest.mark.gpu
def test_gpu_bench_full_run_reports_the_extras():
    line = _bench(["--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-extra-legs"])
    assert all(key in line for key in HEADLINE) and line["steps"] == 4
    assert line["roofline"]["avg_launch_ms"] == line["kernels_ms"]["sdf_fuse"] and line["roofline"]["algorithmic_bytes_per_launch"] > 0
    assert line["kernels_ms"]["parts"]["raycast_sdf"] > 0 and line["sdf_fuse_other_mode"]["math"] == "exact"
    assert "roofline_raycast" in line and "bilateral" in line and "summary" in line and "cpu_baseline" not in line
