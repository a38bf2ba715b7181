#!/usr/bin/env python3
"""bench.py -- KinectFusion frames/s (640x480 depth -> 512^3 TSDF) on MI355X, plus the SdfFuse
HBM roofline and the CPU baseline.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scene full|room] [--math fast|exact] [--full [--no-cpu-baseline]]
                    [--dump-outputs DIR]

A "step" is one frame of the headless KinectFusion loop on synthetic depth that is already
resident in HBM: BilateralFilter -> DepthToVbo -> NormalsFromVbo -> SdfFuse -> RaycastSdf
(BASELINE.json configs[1]: 512^3 TSDF SdfFuse + RaycastSdf, 640x480, 1x MI355X; the cheap
preprocess chain is included so that a step is a whole frame).  Frames follow a 30-pose orbit
with known poses (no ICP).  N > 1: the 512^3 volume is Z-slab partitioned over
the ranks (strong scaling), see kangaroo_amd/pipeline.py: every rank integrates and renders its slab, the renderings are merged by
direct sends over the xGMI mesh (image strips to their owners by all-to-all, nearest hit per pixel, strips back by all-gather),
the merge of frame k overlapped with frame k+1 where it is the only traffic; the line also times the other policies
(`multi_gpu_variants`) and every rank's parts (`per_rank`).

1 GPU: every frame is ONE library call (kfx_frame_step, include/kfx.h) that enqueues the frame's launches and records
device events around its parts, so neither the launch rate nor the kernel times depend on the interpreter.  Before the W
warm-up steps the stream runs untimed until its frame time is stationary (blocks of 60 frames: the last three within 2 %,
at least --prime-seconds of GPU work, at most --prime-cap-seconds); --summary auto decides between the tracked and the plain
pair of kernels on whole frames AFTER that (three blocks of 60 frames: tracked, plain, tracked), then the stream settles
again.  The number of untimed frames is in the line ("prime").  Then the volume is reset and the stream restarts from the
first pose of the orbit for RESTART_FRAMES untimed frames, so that the W warm-up and the K timed steps see the same volume
and the same poses in every run, however long the priming took.

1 GPU, plain run (the default): set-up, the untimed frames, the W warm-up steps, the K timed steps, the outputs of the last
timed step if --dump-outputs is given, the line.  --full: everything else the line reports beside the headline as well --
the parts of a frame, the SdfFuse / RaycastSdf rooflines, the other numerics mode and pair of kernels, the CPU baseline and
the legs on other scenes and sizes.  N > 1: the line is the same either way.

--dump-outputs DIR: after the timed steps, what the last one computed -- the frame's images (filtered depth, vertices,
normals, the three raycast images) and a fixed sample of the volume's cells -- as DIR/<name>.npy, float32 (float64 for the
sample's cell indices), for comparing two builds output for output.  Every array is finite: where the operators leave NaN (no
depth, no hit, a cell never observed) it holds 0, and DIR/<name>_finite.npy is 1 where the pixel / cell was finite, 0 where not.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
N_ORBIT = 30
PMC_TRAFFIC_FILES = ("profiles/r06_pmc_traffic.json", "profiles/r05_pmc_traffic.json")   # the first that was taken on the loaded kernels
BLOCK = 60   # frames per priming / calibration block: two orbits (launch times depend on the pose)
RESTART_FRAMES = 60 * BLOCK   # untimed frames between the volume reset and the warm-up (the priming of a default run is ~6000)
DUMP_SAMPLE_CELLS, DUMP_SEED = 1 << 20, 1234   # --dump-outputs: cells of the volume sampled (fixed seed), at most 8 MiB of them
DUMP_LIMIT_BYTES = 64 << 20


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--config", default="c2", choices=["c2", "c3"],
                    help="c2 (default) = BASELINE configs[1], the configuration the metric is quoted on: 640x480 -> 512^3, scene S_full; "
                         "c3 = BASELINE configs[2]: the same chain on 1280x960 depth (scene S_room unless --scene says otherwise) -- a reported "
                         "variant, never the driver's line")
    ap.add_argument("--scene", default=None, choices=["room", "full"],
                    help="full (default) = S_full of SURVEY 8(d), the roofline scene: a wall behind the volume, ~98 %% of the "
                         "voxels are updated every frame (the heaviest SdfFuse traffic); room = S_room, a furnished room "
                         "(61 %% updated)")
    ap.add_argument("--math", default="fast", choices=["fast", "exact"],
                    help="numerics mode of SdfFuse: fast = rcp/rsq/FMA perf build (reference's own -use_fast_math regime, "
                         "tolerance-tested), exact = IEEE, bit-identical to the oracle")
    ap.add_argument("--res", type=int, default=512, help="volume resolution N (N^3 voxels)")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--raycast", default="exact", choices=["exact", "composite", "exact_allreduce"],
                    help="multi-GPU raycast: exact (default) = the march state handed from slab to slab over the neighbour links, bit-identical to the "
                         "single volume; composite = per-slab march + nearest-hit merge (rays restart at slab entries: a throughput variant outside "
                         "the image tolerance); exact_allreduce = the hand-over's cross-check with an all-reduce per round (--driver python)")
    ap.add_argument("--driver", default="c", choices=["c", "python"],
                    help="N > 1: c (default) = one kfx_slab_frame_step call per frame and rank, collectives enqueued by the library (libkfx_rccl.so); "
                         "python = SlabPipeline issues the operators and torch.distributed collectives one by one")
    ap.add_argument("--tiles", type=int, default=0, help="N > 1, exact raycast, --driver c: image row-tiles of the hand-over (0: the library's default, 4)")
    ap.add_argument("--halo", default="recompute", choices=["recompute", "exchange"],
                    help="N > 1: how ghost planes are kept current -- recomputed by each rank (no traffic) or "
                         "exchanged with the neighbours over RCCL point-to-point after each SdfFuse")
    ap.add_argument("--inputs", default="replicate", choices=["replicate", "broadcast"],
                    help="N > 1: every rank preprocesses the frame itself, or rank 0 does and broadcasts the filtered depth + normal map")
    ap.add_argument("--images", default="all", choices=["all", "root"],
                    help="N > 1, composite raycast: every rank ends up with the merged images (all-reduce of the winners' payload), or "
                         "only rank 0 does (reduce: half the traffic)")
    ap.add_argument("--merge", default="direct", choices=["direct", "allreduce"],
                    help="N > 1, composite raycast: direct = every rank owns a strip of the image: all-to-all of the strips, nearest hit per "
                         "pixel at the owner, all-gather of the merged strips (each byte crosses one xGMI link once per phase, all links at once); "
                         "allreduce = MIN all-reduce of (depth, rank) keys + SUM all-reduce of the winners' payload.  Same images")
    ap.add_argument("--overlap", dest="overlap", action="store_true", default=None,
                    help="N > 1, composite raycast: merge frame k's images on a second stream under frame k+1's preprocess + SdfFuse "
                         "(default where nothing else communicates: composite raycast, ghost planes recomputed, inputs replicated)")
    ap.add_argument("--no-overlap", dest="overlap", action="store_false", help="N > 1: merge each frame's images before the next frame starts")
    ap.add_argument("--summary", nargs="?", const="on", default="auto", choices=["auto", "on", "off"],
                    help="fast math, 1 GPU: the brick summary (kfx_sdf_summary: SdfFuse keeps value ranges per 8^3 cells, RaycastSdf "
                         "marches through class tables built from them and crosses free / never-observed space without reading the "
                         "volume).  auto (default): once the stream is stationary, FramePipeline(track='auto') times three blocks of 60 "
                         "whole frames -- tracked pair, plain pair, tracked pair -- and keeps the tables only if both tracked blocks beat "
                         "the plain block's median frame by 5 %% (S_full: they do, +15-19 %% frames/s; S_room: the plain pair stays); on: "
                         "always; off: the plain kernels.  The line reports the other variant beside the headline")
    ap.add_argument("--prime", type=int, default=None,
                    help="1 GPU: at least this many untimed frames of the stream before the W warm-up steps (default 0: --prime-seconds decides); "
                         "N > 1: exactly this many (default: --prime-seconds of frames at the pace of a first block, at least 450)")
    ap.add_argument("--prime-seconds", type=float, default=2.0,
                    help="untimed frames run until the frame time is stationary AND at least this much GPU time has passed: a GPU "
                         "that was idle takes on the order of a second of work to settle its clocks (KFX_BENCH_DUMP=1 prints the blocks)")
    ap.add_argument("--prime-cap-seconds", type=float, default=8.0, help="give up waiting for a stationary frame time after this much GPU time")
    ap.add_argument("--full", action="store_true",
                    help="1 GPU: also measure what the line reports beside the headline (parts of a frame, rooflines, the other numerics mode and "
                         "pair of kernels, ceilings of the GPU, the CPU baseline, the legs below); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="1 GPU: write what the last timed step computed (the frame's images, a fixed sample of the volume) as DIR/<name>.npy; "
                         "NaN (no depth / hit, a cell never observed) is written as 0, with DIR/<name>_finite.npy marking the finite entries")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="--full, 1 GPU, default configuration: skip the reported legs that follow the headline in the same process -- `room_variant` "
                         "(the same loop on scene S_room, the fps scene of SURVEY 8(d)), `tracked_variant` (the application's loop with the "
                         "projective ICP between rendering and integration: TrackingPipeline(device_icp=True) on S_room; + the drop-in application "
                         "itself as a child process), `noise_variant` (S_room with 2 mm depth noise), `c3_variant` (1280x960), `c4_one_gpu_variant` "
                         "(1024^3) and `c5_variant` (2048^3 fp16, raycast-only)")
    ap.add_argument("--cpu-frames", type=int, default=30, help="upper bound on the timed CPU-baseline frames (the sample also stops after ~12 s)")
    args = ap.parse_args()
    if args.scene is None:
        args.scene = "room" if args.config == "c3" else "full"
    if args.width is None:
        args.width = 1280 if args.config == "c3" else 640
    if args.height is None:
        args.height = 960 if args.config == "c3" else 480
    return args


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, scene, n_frames):
    """The oracle (kind "port") timed on this host's cores: full frames of the same workload
    (same volume size, image size, scene, poses).  Two figures: all cores (OpenMP
    over z-slices / rows) = `value`, and one full frame on a single thread.  The library is
    rebuilt -O3 -march=native for this host (oracle/_native, same -ffp-contract=off arithmetic);
    if that build fails the portable -O2 build of the parity tests is timed instead."""
    import oracle
    from kangaroo_amd import scenes
    build = oracle.use_native_build()
    N, w, h = args.res, args.width, args.height
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    threads = oracle.max_threads()
    vol = oracle.Volume(N, N, N, bmin, bmax)
    oracle.sdf_reset(vol, float("nan"))
    f, vbo, nrm = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h, channels=4)
    rd, rn, ri = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h)

    def frame(i, nt):
        T_wc = scenes.orbit_pose(i, N_ORBIT)
        raw = oracle.Image.from_numpy(scenes.render_depth(scene, w, h, T_wc, K))
        t0 = time.perf_counter()
        oracle.bilateral(f, raw, nthreads=nt, **scenes.BILATERAL)
        oracle.depth_to_vbo(vbo, f, K)
        oracle.normals_from_vbo(nrm, vbo)
        oracle.sdf_fuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=nt)
        oracle.raycast_sdf(rd, rn, ri, vol, T_wc, K, near, far, tr, True, nthreads=nt)
        return time.perf_counter() - t0

    # a bounded sample that does not hang on one reading of a shared host (round-5 verdict: 3.17 -> 2.56 frames/s between two rounds
    # on unchanged code): three blocks of >= 6 timed frames each, `value` = the MEDIAN of the blocks' rates, spread beside it; the
    # blocks shrink (never below 2 frames) where a frame is so slow that three of them would not fit ~9 s of CPU work
    frame(0, threads)                      # untimed: page faults of the volume
    t_probe = frame(1, threads)            # untimed too: sizes the blocks
    per_block = int(max(2, min(n_frames // 3 if n_frames >= 6 else 2, 6 if 18 * t_probe <= 9.0 else 3.0 / max(t_probe, 1e-3))))
    blocks, i = [], 2
    for _ in range(3):
        ts = [frame(i + k, threads) for k in range(per_block)]
        i += per_block
        blocks.append(per_block / sum(ts))
    fps = float(np.median(blocks))
    total_s = sum(per_block / b for b in blocks)
    single_s = frame(i, 1) if threads > 1 else 1.0 / fps   # one full frame on one thread
    return {"value": round(fps, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "blocks_fps": [round(b, 4) for b in blocks], "spread": round((max(blocks) - min(blocks)) / fps, 4),
            "single_thread": {"value": round(1.0 / single_s, 4), "unit": "frames/s", "cores": 1, "sample": "1 full frame = %.1f s" % single_s},
            "cpu_model": cpu_model(), "build": build,
            "sample": "median of 3 blocks of %d full frames (%.1f s together; %d^3 volume, %dx%d, scene %s, orbit poses) of the C restatement "
                      "oracle/kfx_oracle.c, OpenMP over z-slices/rows on %d threads; 2 untimed warm frames; then 1 full frame on 1 thread"
                      % (per_block, total_s, N, w, h, scene, threads)}


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (one per GPU, RCCL) through
    torch.distributed.run as a CHILD of this process -- which has not imported torch or touched a GPU --, relay the
    ranks' output and exit with the child's code.  Never exec: a process that has initialised the GPU must not be replaced."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env)
    sys.exit(proc.returncode)


def workload_text(args, n_prime, distributed):
    N, w, h = args.res, args.width, args.height
    return ("BASELINE configs[%d]: %d^3 TSDF (SDF_t f32 val+weight, %.2f GiB), %dx%d synthetic depth resident in HBM, scene S_%s, "
            "%d-pose orbit with known poses; per frame: BilateralFilter(7x7) -> DepthToVbo -> NormalsFromVbo -> SdfFuse -> RaycastSdf%s; "
            "%d untimed frames of the stream precede the warm-up steps%s" % (
                2 if args.config == "c3" else 1, N, 8.0 * N ** 3 / 2 ** 30, w, h, args.scene, N_ORBIT,
                "" if distributed else " (one kfx_frame_step call per frame)", n_prime,
                "" if distributed else ", the last %d of them after a reset of the volume, from the first pose" % RESTART_FRAMES))


MATH_TEXT = {"fast": "fast (fp32 rcp/rsq + FMA: the reference's own -use_fast_math regime, running average as old + (new - old) w / (w + old.w); whole chain against the exact oracle at this size, "
                     "tests/test_gpu_chain.py: TSDF L-inf < 1e-4 on identically classified voxels (<= 2e-6 of them classified differently); raycast images: "
                     "no hit / miss flip, depth < 1e-4 m on all but <= 2e-5 of the hits, normals < 2e-2 rad, shade < 1e-2; 300-frame streams against the oracle: tests/test_gpu_stream.py)",
             "exact": "exact (IEEE fp32, no FMA contraction, reference operation order; bit-identical to the oracle)"}


def pmc_traffic(key):
    """HBM bytes per launch from PMC passes.  Counters need their own rocprofv3 runs (FETCH_SIZE and WRITE_SIZE do not fit one pass
    and must not be combined with the timed run), so the figure comes from the committed summary of those passes over this same
    command (scripts/gpu_profile.sh -> profiles/<tag>/summary.txt -> the traffic file); `traffic_source` names the file and what it
    was collected on: it is NOT measured in this run.  The file records the digest of the kernel sources it was taken on
    (kfx_kernel_source_id, scripts/make_pmc_traffic.py): a figure of other kernels than the loaded library's is not reported --
    traffic comes back None and the source says why (round-4 verdict, item 8)."""
    from kangaroo_amd import _lib
    L = _lib.load()
    family = "raycast" if key.startswith("raycast_") else "fuse"
    have = L.kfx_kernel_source_id(family.encode()).decode()
    why = None
    for name in PMC_TRAFFIC_FILES:
        try:
            with open(os.path.join(ROOT, name)) as fh:
                tj = json.load(fh)
        except (OSError, ValueError):
            continue
        t = tj.get(key, {}).get("traffic_bytes")
        if t is None:
            continue
        took = (tj.get("_kernel_source_id") or {}).get(family)
        if took != have or tj.get("_kfx_version") != int(L.kfx_version()):
            why = why or ("not reported: %s was taken on %s kernels %s (libkfx %s), this library is built from %s (libkfx %d) -- re-run "
                          "scripts/gpu_profile.sh and scripts/make_pmc_traffic.py" % (name, family, took or "of an unrecorded revision", tj.get("_kfx_version", "?"), have, int(L.kfx_version())))
            continue
        return t, "%s (separate rocprofv3 --pmc passes of this command on the %s kernels %s; not measured in this run)" % (name, family, have)
    return None, why


def prime_stream(kf, step, min_s, cap_s, min_frames, tol=0.02):
    """Run the stream untimed, in blocks of BLOCK frames, until the mean frame period of the last three blocks agrees within `tol`
    and at least min_s seconds of GPU time / min_frames frames have passed (give up after cap_s).  The block before the one just
    issued is read back, so the GPU always has a block of frames queued while the host looks at numbers."""
    firsts, means, issued, gpu_s, stationary = [], [], 0, 0.0, False
    while True:
        firsts.append(kf.count)
        for _ in range(BLOCK):
            step()
        issued += BLOCK
        if len(firsts) >= 2:
            t = kf.timings(firsts[-2], BLOCK)
            means.append(float(np.mean(t[:, 4])))
            if not np.isfinite(means[-1]):   # (frames stepped without the SdfFuse events have no period: nothing to wait for)
                break
            gpu_s += means[-1] * BLOCK * 1e-3
        if len(means) >= 3:
            a, b, c = means[-3:]
            stationary = abs(c - b) <= tol * b and abs(c - a) <= tol * a
            if stationary and gpu_s >= min_s and issued >= min_frames:
                break
        if gpu_s >= cap_s:
            break
    return {"frames": issued, "gpu_s": round(gpu_s, 3), "stationary": bool(stationary), "block_frames": BLOCK, "tolerance": tol,
            "block_mean_frame_ms": [round(m, 4) for m in means]}


NOISE_SIGMA_M, NOISE_SEED = 0.002, 1234   # "where noise is wanted use seed = 1234, Gaussian sigma = 2 mm on depth"
_DEPTH_CACHE = {}


def depth_frames(scenes, scene, w, h, K, noise=False):
    """The orbit's N_ORBIT analytic depth images (host arrays), rendered once per (scene, size) and process.  noise: Gaussian
    sigma = 2 mm per pixel, a different draw per frame of the orbit (seed 1234 + frame)."""
    key = (scene, int(w), int(h), bool(noise))
    if key not in _DEPTH_CACHE:
        _DEPTH_CACHE[key] = [scenes.render_depth(scene, w, h, scenes.orbit_pose(i, N_ORBIT), K, noise_sigma=NOISE_SIGMA_M if noise else 0.0, seed=NOISE_SEED + i)
                             for i in range(N_ORBIT)]
    return _DEPTH_CACHE[key]


def scene_leg(args, torch, roo, scenes, n_steps, N=None, w=None, h=None, scene="room", noise=False, label="S_room", prime_s=0.5, prime_cap_s=2.0):
    """The headline's loop on another scene / size (S_room is the scene for parity + frames/s; S_full, the roofline scene,
    is what `value` is quoted on): same protocol in short -- untimed frames until the frame time is stationary (the clocks are warm),
    the pipeline's own choice of kernels (three blocks of 60 whole frames), settle, n_steps timed frames between two
    synchronisations.  N / w / h default to the headline's; noise: SURVEY 8(d)'s sigma = 2 mm depth noise (seed 1234 + frame)."""
    from kangaroo_amd.pipeline import FramePipeline
    N = args.res if N is None else N
    w = args.width if w is None else w
    h = args.height if h is None else h
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    policy = args.summary if args.math == "fast" else "off"
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, track={"auto": "auto", "on": True, "off": False}[policy],
                         cal_first=-1, cal_block=BLOCK, timing_slots=max(256, n_steps + 4 * BLOCK + 64))
    kf = pipe.kframe
    pipe.set_timing(kf.EVENTS_FUSE)
    poses = [scenes.orbit_pose(i, N_ORBIT) for i in range(N_ORBIT)]
    frames = []
    for d in depth_frames(scenes, scene, w, h, K, noise):
        im = roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
        im.MemcpyFromHost(d)
        frames.append(im)
    n_updated = []
    for i in range(N_ORBIT):
        pipe.preprocess(frames[i])
        n_updated.append(roo.SdfFuseCount(pipe.vol, pipe.filtered, pipe.normals, scenes.se3_inverse(poses[i]), K, pipe.trunc, pipe.mincostheta))
    cursor = [0]

    def step():
        i = cursor[0] % N_ORBIT
        cursor[0] += 1
        pipe.step(poses[i], frames[i])
        return i
    prime = [prime_stream(kf, step, prime_s, prime_cap_s, 0)]
    if pipe.track_policy == "auto":
        pipe.recalibrate()
        guard = 0
        while pipe.track_decision is None and guard < 8 * BLOCK:
            step()
            guard += 1
        prime.append(prime_stream(kf, step, 0.1, 1.0, 3 * BLOCK))
    torch.cuda.synchronize()
    first = kf.count
    t0 = time.perf_counter()
    idx = [step() for _ in range(n_steps)]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    t = kf.timings(first, n_steps)
    fuse_ms = float(np.mean(t[:, 1]))
    pipe.set_timing(kf.EVENTS_ALL)
    for _ in range(N_ORBIT):
        step()
    f_parts = kf.count
    for _ in range(2 * N_ORBIT):
        step()
    tp = kf.timings(f_parts, 2 * N_ORBIT)
    bytes_avg = float(np.mean([16.0 * n_updated[i] + 20.0 * w * h for i in idx]))
    use_summary = bool(pipe.track)
    traffic, traffic_source = (pmc_traffic("%s_%s%s" % (scene, args.math, "_tracked" if use_summary else ""))
                               if (N, w, h) == (512, 640, 480) and not noise else (None, None))
    out = {"scene": label, "volume": [N, N, N], "image": [w, h], "frames_per_sec": round(n_steps / elapsed, 1), "steps": n_steps,
           "prime": cursor[0] - n_steps - 3 * N_ORBIT, "ms_per_step": round(1e3 * elapsed / n_steps, 4),
           "sdf_fuse_ms": round(fuse_ms, 5), "sdf_fuse_achieved_GBps": round(bytes_avg / (fuse_ms * 1e-3) / 1e9, 1),
           "sdf_fuse_frac_of_peak": round(bytes_avg / (fuse_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": round(bytes_avg),
           "updated_fraction": round(float(np.mean([n_updated[i] for i in idx])) / (N ** 3), 4),
           "sdf_fuse_traffic": traffic, "sdf_fuse_traffic_source": traffic_source,
           "raycast_sdf_ms": round(float(np.mean(tp[:, 2])), 5), "preprocess_ms": round(float(np.mean(tp[:, 0])), 5),
           "raycast": "march through the class tables (tracked SdfFuse)" if use_summary else "plain march (kfx_raycast_sdf)",
           "summary_policy": {"requested": policy, "decision": pipe.track_decision},
           "priming_block_mean_frame_ms": [pl["block_mean_frame_ms"][-3:] for pl in prime],
           "note": "the headline's loop (one kfx_frame_step per frame, same numerics) on %s, %d^3, %dx%d%s, timed in the same process after the "
                   "headline: %d steps between two synchronisations" % (label, N, w, h, ", depth noise sigma = 2 mm (seed 1234 + frame)" if noise else "", n_steps)}
    del pipe, frames
    torch.cuda.empty_cache()
    return out


def room_leg(args, torch, roo, scenes, n_steps):
    return scene_leg(args, torch, roo, scenes, n_steps)


def c5_leg(args, torch, roo, scenes, n_steps):
    """BASELINE configs[4] on the one GPU: a 2048^3 fp16 TSDF (32 GiB) resident in HBM, raycast-only.  The volume encodes the
    analytic sphere of roo::SdfSphere (the reference's own synthetic volume; tests/test_gpu_parity.py checks the rendering against
    the ray-sphere intersection); per launch: ms between device events, samples and distinct cells by the counting march."""
    N, w, h = 2048, 640, 480
    K = scenes.intrinsics(w, h)
    free, _total = torch.cuda.mem_get_info()
    if free < 36 * 2 ** 30:
        return {"skipped": "needs 36 GiB of free device memory, %.1f GiB are free" % (free / 2 ** 30)}
    vol = roo.BoundedVolume(N, N, N, (-1, -1, -1), (1, 1, 1), kind="f16")
    roo.SdfSphere(vol, (0.0, 0.0, 0.0), 0.9)
    tr = float(2.0 * np.linalg.norm(vol.VoxelSizeUnits()))
    rd, rn, ri = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)
    poses = []
    for i in range(N_ORBIT):   # the orbit's motion in front of the sphere (camera 2.6 m before its centre)
        T = scenes.orbit_pose(i, N_ORBIT).copy()
        T[2, 3] -= 2.6
        poses.append(T)
    for i in range(N_ORBIT):
        roo.RaycastSdf(rd, rn, ri, vol, poses[i], K, 0.1, 10.0, tr, True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(n_steps):
        roo.RaycastSdf(rd, rn, ri, vol, poses[k % N_ORBIT], K, 0.1, 10.0, tr, True)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / n_steps
    hits = int(torch.isfinite(rd.tensor()).sum())
    cnt = [roo.RaycastSdfCount(vol, w, h, poses[i], K, 0.1, 10.0, tr, True) for i in (0, 7, 15, 22)]
    smp, U = float(np.mean([c["samples"] for c in cnt])), float(np.mean([c["U"] for c in cnt]))
    out = {"volume": [N, N, N], "cells": "fp16 {val, w} (4 B), %.0f GiB" % (4.0 * N ** 3 / 2 ** 30), "image": [w, h], "steps": n_steps,
           "raycast_ms": round(ms, 5), "frames_per_sec_raycast_only": round(1e3 / ms, 1), "Mrays_per_s": round(w * h / (ms * 1e-3) / 1e6, 1),
           "samples_per_launch": round(smp), "Gsamples_per_s": round(smp / (ms * 1e-3) / 1e9, 3),
           "gather_32B_GBps": round(32.0 * 4 * smp / (ms * 1e-3) / 1e9, 1), "distinct_cells": round(U),
           "unique_bytes_GBps": round((4.0 * U + 24.0 * w * h) / (ms * 1e-3) / 1e9, 1),
           "frac_of_peak_by_unique_bytes": round((4.0 * U + 24.0 * w * h) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "hits": hits,
           "note": "kfx_raycast_sdf_h on the SdfSphere volume (radius 0.9 in a [-1, 1]^3 box), %d launches back to back after %d untimed, device events; a "
                   "trilinear sample = four 8-byte gathers of two x-adjacent half cells (32 B); samples / distinct cells from kfx_raycast_sdf_count_h "
                   "(4 of the %d poses)" % (n_steps, N_ORBIT, N_ORBIT)}
    del vol, rd, rn, ri
    torch.cuda.empty_cache()
    return out


def reference_sequence_leg(args, n_frames=150, warm=30):
    """The drop-in application's own number (round-5 verdict, item 5a): apps/kinectfusion_headless --track is the reference
    application's frame loop (main.cpp:200-356) restricted to the reference's signatures -- per-level DepthToVbo / NormalsFromVbo /
    RaycastSdf, PoseRefinementProjectiveIcpPointPlane returning its system to the host every iteration, the 6 x 6 solve on the host,
    SdfFuse -- compiled against include/kangaroo/ and linked to libkfx.so, run here as a CHILD process on the same GPU (512^3, S_room,
    640x480, fast numerics; the first `warm` frames do not count)."""
    import re
    import subprocess
    exe = os.path.join(ROOT, "apps", "kinectfusion_headless")
    if not os.path.exists(exe):
        return {"error": "apps/kinectfusion_headless is not built"}
    cmd = [exe, "--res", str(args.res), "--width", str(args.width), "--height", str(args.height), "--frames", str(n_frames), "--warmup", str(warm), "--track"]
    if args.math == "fast":
        cmd.append("--fast")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    m = re.search(r"([0-9.]+) ms/frame \(([0-9.]+) fps\)", p.stdout)
    e = re.search(r"worst position error ([0-9.]+) mm", p.stdout)
    if p.returncode != 0 or not m:
        return {"error": "rc %d: %s" % (p.returncode, (p.stdout + p.stderr)[-300:])}
    return {"frames_per_sec": float(m.group(2)), "ms_per_step": float(m.group(1)), "frames": n_frames - warm, "warmup": warm,
            "worst_position_error_mm": float(e.group(1)) if e else None, "command": " ".join(["apps/kinectfusion_headless"] + cmd[1:])}


def tracked_leg(args, torch, roo, scenes, n_steps, noise=False):
    """True end-to-end KinectFusion (main.cpp:200-356 with pose estimation on): per frame the depth pyramid, the
    model rendered at the last pose on the ICP levels, the projective point-plane ICP (device-resident loop, kfx_icp_refine: one
    synchronisation per frame for the pose), SdfFuse at the refined pose.  Scene S_room (S_full is a single wall: its in-plane motion
    is unobservable); the orbit's poses are NOT given after frame 0 -- `worst_position_error_mm` is what the tracker ends up with."""
    from kangaroo_amd.pipeline import TrackingPipeline
    N, w, h, scene = args.res, args.width, args.height, "room"
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    pipe = TrackingPipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, device_icp=True, track=False)
    poses = [scenes.orbit_pose(i, N_ORBIT) for i in range(N_ORBIT)]
    frames = []
    for d in depth_frames(scenes, scene, w, h, K, noise):
        im = roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
        im.MemcpyFromHost(d)
        frames.append(im)
    worst, lost = 0.0, 0

    def run(n, first):
        nonlocal worst, lost
        for k in range(n):
            i = (first + k) % N_ORBIT
            T = pipe.step(poses[i] if first + k == 0 else None, frames[i], next_image=frames[(i + 1) % N_ORBIT])
            worst = max(worst, float(np.linalg.norm(T[:3, 3] - poses[i][:3, 3])))
            lost += 0 if pipe.tracking_good else 1
    run(2 * N_ORBIT, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(n_steps, 2 * N_ORBIT)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    out = {"scene": "S_room" + (", depth noise sigma = 2 mm (seed 1234 + frame)" if noise else ""),
           "frames_per_sec": round(n_steps / elapsed, 1), "steps": n_steps, "ms_per_step": round(1e3 * elapsed / n_steps, 4),
           "worst_position_error_mm": round(1e3 * worst, 3), "frames_lost": lost, "resets": pipe.resets, "final_rmse": round(float(pipe.rmse), 6),
           "loop": "TrackingPipeline(device_icp=True): BilateralFilter -> depth pyramid with DepthToVbo / NormalsFromVbo of every level (one launch) -> RaycastSdf on levels "
                   "0, 2, 3 (one launch) -> kfx_icp_refine (6 iterations over 3 levels, its = {1, 0, 2, 3}, solved on the device) -> one pose read-back "
                   "-> SdfFuse at the estimated pose; the Python loop issues the operators (the C++ application's loop: apps/kinectfusion_headless --device-icp)",
           "note": "%d frames of the orbit tracked from depth alone after %d untimed ones; position error against the known orbit over all of them "
                   "(steps between poses up to 10.5 mm)" % (n_steps, 2 * N_ORBIT)}
    del pipe, frames
    torch.cuda.empty_cache()
    return out


def finite_split(name, a, channels):
    """{name: a with its non-finite entries as 0, name_finite: 1 where every channel of the pixel / cell is finite, else 0}: NaN
    is what the operators write where there is no depth or hit and what a never-observed cell holds; the dump stays finite."""
    ok = np.isfinite(a)
    return {name: np.where(ok, a, np.float32(0)).astype(a.dtype),
            name + "_finite": (ok.all(axis=-1) if channels else ok).astype(np.float32)}


def snapshot_outputs(torch, pipe):
    """What the last frame left in the caller's containers, copied to the host: the frame's images and the cells (val, w) of a
    fixed sample of the volume (DUMP_SEED: the same cells in every run of the same size), each beside its `_finite` mask (see
    finite_split).  Images too large for DUMP_LIMIT_BYTES beside the sample keep every k-th row only.  Returns (arrays, row stride)."""
    vol = pipe.vol
    n_cells = vol.w * vol.h * vol.d
    if n_cells <= DUMP_SAMPLE_CELLS:
        cells = np.arange(n_cells, dtype=np.int64)
    else:
        cells = np.sort(np.random.default_rng(DUMP_SEED).choice(n_cells, DUMP_SAMPLE_CELLS, replace=False)).astype(np.int64)
    t = torch.from_numpy(cells).to(vol.storage.device)
    x, y, z = t % vol.w, (t // vol.w) % vol.h, t // (vol.w * vol.h)
    out = finite_split("volume_sample", vol.tensor()[z, y, x].float().cpu().numpy(), True)   # (n, 2): val, w
    out["volume_sample_cells"] = cells.astype(np.float64)                                      # x + w (y + h z)
    images = {"filtered_depth": pipe.filtered, "vertices": pipe.vbo, "normals": pipe.normals,
              "raycast_depth": pipe.ray_d, "raycast_normals": pipe.ray_n, "raycast_image": pipe.ray_i}
    split = {}
    for name, im in images.items():
        split.update(finite_split(name, np.ascontiguousarray(im.MemcpyToHost(), dtype=np.float32), im.channels > 1))
    room = DUMP_LIMIT_BYTES - sum(a.nbytes for a in out.values())
    stride = max(1, -(-sum(a.nbytes for a in split.values()) // room))
    out.update({name: np.ascontiguousarray(a[::stride]) for name, a in split.items()})
    return out, stride


def write_outputs(outputs, stride, directory):
    total = sum(a.nbytes for a in outputs.values())
    assert total <= DUMP_LIMIT_BYTES, "outputs of %d bytes exceed the dump limit" % total
    os.makedirs(directory, exist_ok=True)
    for name, a in outputs.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
        np.save(os.path.join(directory, name + ".npy"), a)
    return {"dir": directory, "files": sorted(n + ".npy" for n in outputs), "bytes": int(total), "image_row_stride": int(stride),
            "volume_sample_seed": DUMP_SEED}


def run_single(args, torch, roo, scenes, rank):
    """1 GPU: the headline, and with --full everything reported beside it.  Returns the JSON object (without cpu_baseline)."""
    import gc
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h, scene = args.res, args.width, args.height, args.scene
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    # fast numerics: SdfFuse keeps a brick summary of the volume as a by-product and RaycastSdf takes its steps through
    # uniformly free / never-observed regions from it (same volume bits; depth within the fast-mode tolerance of the plain
    # march, tests/test_gpu_summary.py).  Exact numerics gain nothing from it (averaged +trunc values are not bit-uniform).
    policy = args.summary if args.math == "fast" else "off"
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, track={"auto": "auto", "on": True, "off": False}[policy],
                         cal_first=-1, cal_block=BLOCK, timing_slots=max(256, args.steps + 4 * BLOCK + 64))
    kf = pipe.kframe
    if kf is None:
        sys.exit("bench.py: the operator set has no kfx_frame (libkfx too old?)")
    # An event is a marker between two launches and costs the stream a few microseconds (all four of a frame: 2.7 % of frames/s,
    # measured): the untimed and the timed frames record the two around SdfFuse -- its window for `roofline`, and the frame period
    # (before-SdfFuse to before-SdfFuse) -- and the parts of a frame are read from frames with all four events afterwards.
    pipe.set_timing(kf.EVENTS_FUSE)

    # synthetic depth stream, uploaded once: the timed region starts with inputs resident in HBM
    poses = [scenes.orbit_pose(i, N_ORBIT) for i in range(N_ORBIT)]
    frames = []
    for d in depth_frames(scenes, scene, w, h, K):
        im = roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
        im.MemcpyFromHost(d)
        frames.append(im)

    # algorithmic bytes: 16 B x N_updated + 20 B x w*h per SdfFuse launch; N_updated counted per pose by
    # the diagnostics kernel (same predicate, no volume traffic), outside timing (--full: the roofline)
    n_updated = []
    if args.full:
        for i in range(N_ORBIT):
            pipe.preprocess(frames[i])
            n_updated.append(roo.SdfFuseCount(pipe.vol, pipe.filtered, pipe.normals, scenes.se3_inverse(poses[i]), K, pipe.trunc, pipe.mincostheta))
    alg = [16.0 * n_updated[i] + 20.0 * w * h for i in range(len(n_updated))]

    cursor = [0]   # the stream's frame counter: poses / depth images cycle through the orbit

    def step():
        i = cursor[0] % N_ORBIT
        cursor[0] += 1
        pipe.step(poses[i], frames[i])
        return i

    gc.collect()
    gc.disable()   # a generation-2 collection inside the timed region stalls the launching thread for tens of ms (seen at --steps 200)
    # ---- untimed: until the frame time is stationary, then the pipeline's own choice of kernels, then stationary again ----
    prime_log = [prime_stream(kf, step, args.prime_seconds, args.prime_cap_seconds, args.prime or 0)]
    if pipe.track_policy == "auto":
        pipe.recalibrate()
        guard = 0
        while pipe.track_decision is None and guard < 8 * BLOCK:
            step()
            guard += 1
        prime_log.append(prime_stream(kf, step, 0.25, 2.0, 3 * BLOCK))
    use_summary = bool(pipe.track)   # what the timed frames run with
    # ---- restart: how many frames the priming took depends on the clocks; the volume the timed steps see must not.  Reset
    # (cells and, with the tables, the summary), then RESTART_FRAMES frames from the first pose, the warm-up, the timed steps ----
    n_primed = cursor[0]
    kf.reset()
    cursor[0] = 0
    for _ in range(RESTART_FRAMES):
        step()
    for _ in range(args.warmup):
        step()
    n_prime = n_primed + RESTART_FRAMES
    torch.cuda.synchronize()
    # ---- the timed region: exactly K steps between two synchronisations ----
    first = kf.count
    t0 = time.perf_counter()
    idx = [step() for _ in range(args.steps)]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc.enable()

    t = kf.timings(first, args.steps)   # device events recorded by kfx_frame_step on the launch stream around SdfFuse
    fuse_ms = t[:, 1]
    fuse_avg_ms = float(np.mean(fuse_ms))
    hits = int(torch.isfinite(pipe.ray_d.tensor()).sum())
    assert hits > 0, "raycast produced no hits"
    dumped = write_outputs(*snapshot_outputs(torch, pipe), args.dump_outputs) if args.dump_outputs else None
    if os.environ.get("KFX_BENCH_DUMP"):   # per-step windows of the timed region and the priming blocks (transients)
        for pl in prime_log:
            print("prime_blocks_ms " + " ".join("%.4f" % v for v in pl["block_mean_frame_ms"]), file=sys.stderr)
        print("fuse_ms " + " ".join("%.3f" % v for v in fuse_ms[:64]), file=sys.stderr)
        print("period_ms " + " ".join("%.3f" % v for v in t[:64, 4]), file=sys.stderr)
    restart = {"frames": RESTART_FRAMES, "after_priming_frames": n_primed,
               "note": "the volume is reset after the priming and the stream restarts from the first pose: the warm-up and the timed steps "
                       "see the same volume in every run"}
    kernels_ms = {"sdf_fuse": round(fuse_avg_ms, 5), "frame_total": round(1e3 * elapsed / args.steps, 5),
                  "frame_period_events": round(float(np.nanmean(t[:, 4])), 5)}
    out = {
        "metric": "kinectfusion_frames_per_sec_640x480_to_512cubed_tsdf",
        "value": round(args.steps / elapsed, 3),
        "unit": "frames/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "prime": n_prime,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": workload_text(args, n_prime, False),
            "volume": [N, N, N], "image": [w, h], "scene": scene, "backend": None, "ranks_agree": None,
            "raycast": ("march through the class tables of the brick summary, kept current by the tracked SdfFuse (kfx_sdf_fuse_tracked + kfx_raycast_sdf_tracked)"
                        if use_summary else "plain march (kfx_raycast_sdf)"),
            "summary_policy": {"requested": args.summary if args.math == "fast" else "off (exact numerics)", "decision": pipe.track_decision},
            "priming": prime_log,
            "restart": restart,
            "partition": "single volume",
            "math": MATH_TEXT[args.math],
        },
        "kernels_ms": kernels_ms,
    }
    if dumped is not None:
        out["outputs"] = dumped
    if not args.full:
        return out

    # ==== --full: everything below is reported beside the headline; none of it is `value` ====
    # the parts of the same frames, from 60 more of them with all four events (untimed; they cost 2-3 % of the frame rate)
    pipe.set_timing(kf.EVENTS_ALL)
    for _ in range(N_ORBIT):
        step()
    f_parts = kf.count
    i_parts = [step() for _ in range(2 * N_ORBIT)]
    tp = kf.timings(f_parts, 2 * N_ORBIT)
    pre_ms, ray_ms, frame_ms = tp[:, 0], tp[:, 2], tp[:, 3]
    if os.environ.get("KFX_BENCH_DUMP"):
        print("parts: ray_ms " + " ".join("%.3f" % v for v in ray_ms[:30]), file=sys.stderr)
        print("parts: pre_ms " + " ".join("%.3f" % v for v in pre_ms[:30]), file=sys.stderr)
    ray_avg_ms = float(np.mean(ray_ms))
    ray_idx = i_parts   # the poses RaycastSdf's figures are averaged over
    bytes_avg = float(np.mean([alg[i] for i in idx]))
    achieved = bytes_avg / (fuse_avg_ms * 1e-3) / 1e9
    voxels = pipe.vol.w * pipe.vol.h * pipe.vol.d

    def timed_steps(n, untimed):
        """`untimed` frames, a synchronisation, n frames between two host clock readings; (frames/s, per-frame timings)."""
        for _ in range(untimed):
            step()
        torch.cuda.synchronize()
        f0 = kf.count
        c0 = time.perf_counter()
        ii = [step() for _ in range(n)]
        torch.cuda.synchronize()
        dt = time.perf_counter() - c0
        return n / dt, kf.timings(f0, n), ii

    # ---- the other pair of kernels on the same frames (not part of `value`) ----
    summary_variant, plain_variant = None, None
    n_v = min(args.steps, 2 * N_ORBIT)
    if args.math == "fast" and use_summary:
        try:   # the headline ran through the tables: the same frames with the plain kernels beside it (a reported extra must never cost the line)
            pipe.set_track(False)
            fps_v, tv, iv = timed_steps(n_v, N_ORBIT)
            pv_bytes = float(np.mean([alg[i] for i in iv]))
            pv_fuse = float(np.mean(tv[:, 1]))
            plain_variant = {"frames_per_sec": round(fps_v, 1), "steps": n_v, "sdf_fuse_ms": round(pv_fuse, 5),
                             "sdf_fuse_frac_of_peak": round(pv_bytes / (pv_fuse * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                             "raycast_sdf_ms": round(float(np.mean(tv[:, 2])), 5),
                             "note": "kfx_sdf_fuse + kfx_raycast_sdf (no summary), same frames, %d steps after %d untimed ones (bench.py --summary off makes it the headline)" % (n_v, N_ORBIT)}
            pipe.set_track(True)   # (the summary is rebuilt from the volume)
            for _ in range(N_ORBIT):
                step()
        except Exception as e:   # noqa: BLE001
            plain_variant = {"error": repr(e)[:300]}
    elif args.math == "fast" and hasattr(roo, "SdfSummary"):
        try:
            pipe.set_track(True)
            fps_v, tv, iv = timed_steps(n_v, 2 * N_ORBIT)
            summary_variant = {"frames_per_sec": round(fps_v, 1), "steps": n_v, "sdf_fuse_tracked_ms": round(float(np.mean(tv[:, 1])), 5),
                               "raycast_sdf_tracked_ms": round(float(np.mean(tv[:, 2])), 5),
                               "note": "kfx_sdf_fuse_tracked + kfx_raycast_sdf_tracked, summary rebuilt from the volume, same frames, %d steps after %d untimed ones "
                                       "(bench.py --summary on makes it the headline)" % (n_v, 2 * N_ORBIT)}
            pipe.set_track(False)
            for _ in range(N_ORBIT):
                step()
        except Exception as e:   # noqa: BLE001
            summary_variant = {"error": repr(e)[:300]}
            pipe.set_track(False)

    # ---- the same SdfFuse launched back to back (no RaycastSdf in between), 24 launches after 66 untimed: in the frame loop the
    # plain march leaves ~250 MB of the volume in the 256 MiB memory-side cache and the SdfFuse that follows reads them from
    # there; back to back nothing precedes a launch but the previous sweep (EXPERIMENTS.md 5.4) ----
    back_to_back = None
    try:
        f0 = kf.count
        ib = []
        for k in range(90):
            i = (cursor[0] + k) % N_ORBIT
            pipe.preprocess(frames[i])
            pipe.fuse(poses[i])
            ib.append(i)
        tb = kf.timings(f0, 180)[1::2, 1][66:]
        bb_ms = float(np.mean(tb))
        bb_bytes = float(np.mean([alg[i] for i in ib[66:]]))
        back_to_back = {"avg_launch_ms": round(bb_ms, 5), "achieved": round(bb_bytes / (bb_ms * 1e-3) / 1e9, 1),
                        "frac": round(bb_bytes / (bb_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "note": "the same frames with no RaycastSdf between the SdfFuse launches (24 timed after 66): in the frame loop the plain march leaves part of the volume in the 256 MiB memory-side cache for the next SdfFuse"}
        for _ in range(N_ORBIT):   # back to whole frames (the images of the last pose are current again)
            step()
    except Exception as e:   # noqa: BLE001
        back_to_back = {"error": repr(e)[:300]}

    # ---- RaycastSdf and BilateralFilter by SURVEY 8(d)'s figures (the volume is in the timed loop's steady state).
    # RaycastSdf: algorithmic bytes 8 B x U + 24 B x w h, U = distinct voxels the TIMED kernel reads for the pose: the plain march's
    # (kfx_raycast_sdf_count) or the table march's own (kfx_raycast_sdf_count_tracked: its samples' cells + the class tables),
    # counted untimed with a bitmap; `reference_U` is the reference march's figure either way.  The march is bound by its chain of
    # dependent misses, so the sample rate and the 64-byte gather rate are given beside it.
    roofline_raycast, bilateral_line, transfer_line = None, None, None
    try:
        ref_cnt = [roo.RaycastSdfCount(pipe.vol, w, h, poses[i], K, near, far, pipe.trunc, True) for i in range(N_ORBIT)]
        cnt = [roo.RaycastSdfCount(pipe.vol, w, h, poses[i], K, near, far, pipe.trunc, True, summary=pipe.summary) for i in range(N_ORBIT)] if use_summary else ref_cnt
        U = float(np.mean([cnt[i]["U"] for i in ray_idx]))
        smp = float(np.mean([cnt[i]["samples"] for i in ray_idx]))
        tab = float(np.mean([cnt[i].get("table_bytes", 0) for i in ray_idx]))
        U_ref = float(np.mean([ref_cnt[i]["U"] for i in ray_idx]))
        ray_bytes = 8.0 * U + tab + 24.0 * w * h
        ray_traffic, ray_traffic_src = pmc_traffic("raycast_%s_%s%s" % (scene, args.math, "_tracked" if use_summary else "")) if (N, w, h) == (512, 640, 480) else (None, None)
        roofline_raycast = {
            "kernel": "k_raycast_sdf_classes (march through the class tables)" if use_summary else "k_raycast_sdf (plain march)",
            "bound": "hbm (by the unique bytes this kernel reads; the march itself is latency-bound)", "achieved": round(ray_bytes / (ray_avg_ms * 1e-3) / 1e9, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ray_bytes / (ray_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "traffic": ray_traffic, "traffic_source": ray_traffic_src,
            "algorithmic_bytes_per_launch": round(ray_bytes), "distinct_voxels": round(U), "class_table_bytes": round(tab),
            "avg_launch_ms": round(ray_avg_ms, 5), "includes": "the per-frame build of the class tables (two small launches)" if use_summary else None,
            "timing": "hipEvents around the RaycastSdf call of %d frames of the same stream stepped with all four events right after the timed region" % (2 * N_ORBIT),
            "samples_per_launch": round(smp), "Gsamples_per_s": round(smp / (ray_avg_ms * 1e-3) / 1e9, 3),
            "gather_64B_GBps": round(64.0 * 4 * smp / (ray_avg_ms * 1e-3) / 1e9, 1),
            "table_lookups_per_launch": round(float(np.mean([cnt[i].get("lookups", 0) for i in ray_idx]))),
            "rays_in_box": round(float(np.mean([cnt[i]["rays"] for i in ray_idx]))), "hits": round(float(np.mean([cnt[i]["hits"] for i in ray_idx]))),
            "reference_U": round(U_ref), "reference_samples": round(float(np.mean([ref_cnt[i]["samples"] for i in ray_idx]))),
            "reference_bytes": round(8.0 * U_ref + 24.0 * w * h),
            "note": "U, samples and look-ups are this kernel's own (counted by a bitmap instantiation of the same march); reference_* are the "
                    "reference march's for the same poses (what the images depend on)"}
    except Exception as e:   # noqa: BLE001
        roofline_raycast = {"error": repr(e)[:300]}
    try:
        # BilateralFilter: 8 B x w h of traffic, 2 x (2r+1)^2 = 98 exponentials per pixel in the reference's loop
        # (cu_bilateral.cu:72-88); the kernel here evaluates the 49 range weights per pixel, the spatial ones once per workgroup
        nb = 200
        for _ in range(10):
            roo.BilateralFilter(pipe.filtered, frames[0], **scenes.BILATERAL)
        b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b0.record()
        for k in range(nb):
            roo.BilateralFilter(pipe.filtered, frames[k % N_ORBIT], **scenes.BILATERAL)
        b1.record()
        torch.cuda.synchronize()
        bil_ms = b0.elapsed_time(b1) / nb
        bilateral_line = {"kernel": "k_bilateral%s<float, 3>" % ("_fast" if args.math == "fast" else ""), "avg_launch_ms": round(bil_ms, 5),
                          "GBps": round(8.0 * w * h / (bil_ms * 1e-3) / 1e9, 1), "Gexp_per_s": round(98.0 * w * h / (bil_ms * 1e-3) / 1e9, 1),
                          "Gexp_per_s_evaluated": round(49.0 * w * h / (bil_ms * 1e-3) / 1e9, 1),
                          "note": "%d launches back to back; 98 exp per pixel is the reference loop's count (radius 3), 49 of them are evaluated per pixel here" % nb}
    except Exception as e:   # noqa: BLE001
        bilateral_line = {"error": repr(e)[:300]}
    try:
        # the same frames with the depth image uploaded every frame, as the application does (main.cpp:203,
        # dKinectMeters.CopyFrom): 4 B x w h from page-locked host memory, asynchronous on the launch stream, inside the
        # timed loop -- the PCIe-inclusive rate (never `value`)
        pinned = [pipe.raw.pinned_like(d) for d in depth_frames(scenes, scene, w, h, K)]
        n_tr = min(args.steps, 4 * N_ORBIT)

        def upload_step():
            i = cursor[0] % N_ORBIT
            cursor[0] += 1
            pipe.raw.MemcpyFromPinned(pinned[i])
            pipe.step(poses[i])
        for _ in range(N_ORBIT):
            upload_step()
        torch.cuda.synchronize()
        t_tr = time.perf_counter()
        for _ in range(n_tr):
            upload_step()
        torch.cuda.synchronize()
        dt_tr = time.perf_counter() - t_tr
        transfer_line = {"frames_per_sec": round(n_tr / dt_tr, 1), "steps": n_tr, "bytes_per_frame": 4 * w * h,
                         "note": "per frame: hipMemcpyAsync of the raw depth image from pinned host memory on the launch stream, then the same kfx_frame_step"}
        del pinned
    except Exception as e:   # noqa: BLE001
        transfer_line = {"error": repr(e)[:300]}

    # ---- the other numerics mode, same frames, plain kernels (reported beside the headline; not part of `value`) ----
    other = "exact" if args.math == "fast" else "fast"
    other_line = None
    try:
        roo.set_math_mode(other)
        pipe.set_track(False)   # the other mode is timed on the plain kernels
        n_other = min(args.steps, 2 * N_ORBIT)   # whole orbits: launch times depend on the pose
        fps_o, to, io = timed_steps(n_other, 2 * N_ORBIT)   # untimed first: cold instruction caches / a settling clock after the switch
        o_ms = float(np.mean(to[:, 1]))
        o_bytes = float(np.mean([alg[i] for i in io]))
        other_line = {"math": other, "avg_launch_ms": round(o_ms, 5), "achieved_GBps": round(o_bytes / (o_ms * 1e-3) / 1e9, 1),
                      "frac": round(o_bytes / (o_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "frames_per_sec": round(fps_o, 1),
                      "kernels_ms": {"preprocess": round(float(np.mean(to[:, 0])), 5), "raycast_sdf": round(float(np.mean(to[:, 2])), 5),
                                     "frame_events": round(float(np.mean(to[:, 3])), 5), "period": round(float(np.nanmean(to[:, 4])), 5)},
                      "note": "same frames, whole step (preprocess + fuse + raycast), plain kernels, %d steps after %d untimed ones" % (n_other, 2 * N_ORBIT)}
    except Exception as e:   # noqa: BLE001
        other_line = {"math": other, "error": repr(e)[:300]}
    roo.set_math_mode(args.math)

    # ---- measured ceilings of this GPU in the same run: in-place 16-byte read-modify-write sweeps of a volume of the
    # same size with no arithmetic (libkfx_debug.so, kfx_debug_rmw: the fuse kernel's own brick mapping with and without
    # nontemporal accesses, other brick shapes, a linear sweep) -- the access pattern SdfFuse has to live with -- and a plain
    # device-to-device copy.  Each probe: 2 untimed + 5 timed launches; bytes = 16 B x cells (8 B read + 8 B written). ----
    rmw_probe, copy_GBps = None, None
    try:
        import ctypes as C
        from kangaroo_amd import _lib
        D = _lib.load_debug()
        D.kfx_debug_rmw.restype = C.c_int
        D.kfx_debug_rmw.argtypes = [_lib.PV, C.c_int, C.c_void_p]
        scratch = roo.BoundedVolume(N, N, N, bmin, bmax)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        best, per = 0.0, {}
        for variant in (0, 1, 10, 11, 12, 13, 14, 15, 16, 17):
            if D.kfx_debug_rmw(scratch.ref(), variant, st) != 0:
                continue
            D.kfx_debug_rmw(scratch.ref(), variant, st)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            for _ in range(5):
                D.kfx_debug_rmw(scratch.ref(), variant, st)
            c1.record()
            torch.cuda.synchronize()
            gbps = 5 * 16.0 * N ** 3 / (c0.elapsed_time(c1) * 1e-3) / 1e9
            per[str(variant)] = round(gbps, 1)
            best = max(best, gbps)
        rmw_probe = {"best_GBps": round(best, 1), "per_variant_GBps": per,
                     "note": "kfx_debug_rmw variants (include/kfx_debug.h): 0 linear sweep, 1 the fuse kernel's 64x8x16 brick, 10-17 generated brick shapes with / without nontemporal accesses; launched back to back"}
        del scratch
        src = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        dst.copy_(src)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(5):
            dst.copy_(src)
        c1.record()
        torch.cuda.synchronize()
        copy_GBps = 5 * 2.0 * src.numel() * 4 / (c0.elapsed_time(c1) * 1e-3) / 1e9
        del src, dst
    except Exception as e:   # noqa: BLE001  (reported extras never cost the headline line)
        rmw_probe = {"error": repr(e)[:200]}

    traffic, traffic_source = pmc_traffic("%s_%s%s" % (scene, args.math, "_tracked" if use_summary else "")) if (N, w, h) == (512, 640, 480) else (None, None)
    # ---- the two legs SURVEY 8(d) / 8(f) name beside the roofline scene, driver-timed in the default command: S_room (the fps scene)
    # through the same loop, and the tracked loop (ICP between rendering and integration).  Reported extras: never `value`. ----
    room_variant, tracked_variant, noise_variant, c3_variant, c4_variant, c5_variant = None, None, None, None, None, None
    if args.config == "c2" and scene == "full" and not args.no_extra_legs:
        del pipe, kf, frames   # (one 512^3 volume at a time is plenty; the legs build their own pipelines)
        torch.cuda.empty_cache()
        gc.collect()
        try:
            room_variant = room_leg(args, torch, roo, scenes, min(args.steps, 4 * N_ORBIT))
        except Exception as e:   # noqa: BLE001
            room_variant = {"error": repr(e)[:300]}
        try:
            tracked_variant = tracked_leg(args, torch, roo, scenes, min(args.steps, 2 * N_ORBIT))
        except Exception as e:   # noqa: BLE001
            tracked_variant = {"error": repr(e)[:300]}
        # the drop-in application itself, restricted to the reference's signatures (a child process on the same GPU)
        try:
            ref_seq = reference_sequence_leg(args)
            if isinstance(tracked_variant, dict):
                tracked_variant["reference_sequence_fps"] = ref_seq.get("frames_per_sec")
                tracked_variant["reference_sequence"] = ref_seq
        except Exception as e:   # noqa: BLE001
            if isinstance(tracked_variant, dict):
                tracked_variant["reference_sequence"] = {"error": repr(e)[:300]}
        # SURVEY 8(d)'s noisy input (sigma = 2 mm, seed 1234): the headline's loop and the tracked loop on S_room with depth noise
        n_short = min(args.steps, 2 * N_ORBIT)
        try:
            noise_variant = scene_leg(args, torch, roo, scenes, n_short, noise=True, label="S_room + noise")
            try:
                tn = tracked_leg(args, torch, roo, scenes, n_short, noise=True)
                noise_variant["tracked"] = {k: tn[k] for k in ("frames_per_sec", "ms_per_step", "worst_position_error_mm", "frames_lost", "resets", "final_rmse", "steps")}
            except Exception as e:   # noqa: BLE001
                noise_variant["tracked"] = {"error": repr(e)[:300]}
        except Exception as e:   # noqa: BLE001
            noise_variant = {"error": repr(e)[:300]}
        # the other single-GPU BASELINE configs, driver-timed in short: C3 (1280x960 chain), C4's volume on one GPU (1024^3), C5 (2048^3 fp16)
        try:
            c3_variant = scene_leg(args, torch, roo, scenes, n_short, w=1280, h=960, label="BASELINE configs[2] (C3): S_room at 1280x960")
        except Exception as e:   # noqa: BLE001
            c3_variant = {"error": repr(e)[:300]}
        try:
            c4_variant = scene_leg(args, torch, roo, scenes, n_short, N=1024, label="BASELINE configs[3]'s volume on ONE GPU (C4): S_room, 1024^3 f32 = 8 GiB",
                                   prime_s=0.3, prime_cap_s=1.5)
        except Exception as e:   # noqa: BLE001
            c4_variant = {"error": repr(e)[:300]}
        try:
            c5_variant = c5_leg(args, torch, roo, scenes, n_short)
        except Exception as e:   # noqa: BLE001
            c5_variant = {"error": repr(e)[:300]}
    outputs = out.pop("outputs", None)
    del out["kernels_ms"]   # (re-inserted after the roofline: the order of the line's keys)
    out.update({
        "roofline": {
            "kernel": "k_sdf_fuse_tiled<%s%s> (SdfFuse, %s math%s)" % ("true" if args.math == "fast" else "false", ", TRACK" if use_summary else "", args.math,
                                                                        ", keeping the brick summary current" if use_summary else ""),
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": round(bytes_avg),
            "avg_launch_ms": round(fuse_avg_ms, 5),
            "median_launch_ms": round(float(np.median(fuse_ms)), 5),
            "timing": "hipEvents recorded by kfx_frame_step on the launch stream around the SdfFuse call of every timed step",
            "updated_fraction": round(float(np.mean([n_updated[i] for i in idx])) / voxels, 4),
            "full_sweep_GBps": round(16.0 * voxels / (fuse_avg_ms * 1e-3) / 1e9, 1),
            "back_to_back": back_to_back,
            "rmw_probe": rmw_probe,
            "full_sweep_frac_of_best_rmw_probe": (round(16.0 * voxels / (fuse_avg_ms * 1e-3) / 1e9 / rmw_probe["best_GBps"], 4)
                                                  if rmw_probe and rmw_probe.get("best_GBps") else None),
            "torch_copy_GBps": None if copy_GBps is None else round(copy_GBps, 1),
            "note": "whole volume",
        },
        "kernels_ms": dict(kernels_ms,
                           parts={"preprocess": round(float(np.mean(pre_ms)), 5), "sdf_fuse": round(float(np.mean(tp[:, 1])), 5),
                                  "raycast_sdf": round(ray_avg_ms, 5), "frame_events": round(float(np.mean(frame_ms)), 5),
                                  "period": round(float(np.nanmean(tp[:, 4])), 5),
                                  "note": "%d frames of the same stream with all four events recorded, right after the timed region; the timed "
                                          "steps record the two around SdfFuse only (an event is a marker between launches: four per frame cost "
                                          "2-3 %% of the frame rate)" % (2 * N_ORBIT)}),
        "sdf_fuse_other_mode": other_line,
    })
    if outputs is not None:
        out["outputs"] = outputs
    for key, val in (("roofline_raycast", roofline_raycast), ("bilateral", bilateral_line), ("transfer_inclusive", transfer_line),
                     ("brick_summary_variant", summary_variant), ("plain_variant", plain_variant), ("room_variant", room_variant),
                     ("tracked_variant", tracked_variant), ("noise_variant", noise_variant), ("c3_variant", c3_variant),
                     ("c4_one_gpu_variant", c4_variant), ("c5_variant", c5_variant)):
        if val is not None:
            out[key] = val
    return out


def make_summary(out):
    """The figures reported beside the headline, once more as ONE compact dict at the very END of the line (after cpu_baseline), so
    that a reader who keeps only the tail of the line still has every secondary number (round-5 verdict, item 2a).  < 700 chars."""
    def g(key, *path):
        v = out.get(key)
        for k in path:
            v = v.get(k) if isinstance(v, dict) else None
        return v
    return {
        "fps": out.get("value"), "fuse_frac": g("roofline", "frac"), "fuse_ms": g("roofline", "avg_launch_ms"),
        "room_fps": g("room_variant", "frames_per_sec"), "room_fuse_frac": g("room_variant", "sdf_fuse_frac_of_peak"),
        "tracked_fps": g("tracked_variant", "frames_per_sec"), "tracked_err_mm": g("tracked_variant", "worst_position_error_mm"),
        "reference_sequence_fps": g("tracked_variant", "reference_sequence_fps"),
        "plain_fps": g("plain_variant", "frames_per_sec") or g("brick_summary_variant", "frames_per_sec"),
        "exact_fuse_frac": g("sdf_fuse_other_mode", "frac"), "transfer_inclusive_fps": g("transfer_inclusive", "frames_per_sec"),
        "noise_fps": g("noise_variant", "frames_per_sec"), "noise_fuse_frac": g("noise_variant", "sdf_fuse_frac_of_peak"),
        "noise_tracked_fps": g("noise_variant", "tracked", "frames_per_sec"), "noise_tracked_err_mm": g("noise_variant", "tracked", "worst_position_error_mm"),
        "c3_room_fps": g("c3_variant", "frames_per_sec"), "c3_room_fuse_ms": g("c3_variant", "sdf_fuse_ms"), "c3_room_fuse_frac": g("c3_variant", "sdf_fuse_frac_of_peak"),
        "c4_one_gpu_fps": g("c4_one_gpu_variant", "frames_per_sec"), "c4_fuse_frac": g("c4_one_gpu_variant", "sdf_fuse_frac_of_peak"),
        "c5_raycast_ms": g("c5_variant", "raycast_ms"), "c5_Gsamples_per_s": g("c5_variant", "Gsamples_per_s"),
        "cpu_fps": g("cpu_baseline", "value"),
    }


def run_slabs(args, torch, dist, roo, scenes, rank, world):
    """N > 1: the volume in Z-slabs, one rank per GPU (strong scaling).  Returns the JSON object on rank 0, None elsewhere.
    --driver c (default): every frame is ONE kfx_slab_frame_step call per rank (include/kfx_slab.h) -- the launches and the
    collectives are enqueued by the library, through libkfx_rccl.so's RCCL communicator (one process per GPU) or, for the tests'
    gloo ranks sharing a GPU, through the process group; --driver python: SlabPipeline issues operators and torch.distributed
    collectives one by one (the cross-check; timed beside the headline as `driver_python_fps`)."""
    import gc
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    N, w, h, scene = args.res, args.width, args.height, args.scene
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    # the overlapped merge issues its collectives from a second stream: allowed only where the main stream issues none (ghost planes
    # recomputed, inputs replicated) -- two streams of collectives could interleave in rank-dependent order
    c_driver = args.driver == "c"
    # --raycast exact, --driver c: frames pipelined across the ranks (frame k's final exchange on the frame object's side stream and
    # second communicator under frame k + 1: include/kfx_slab.h) -- the default; bit-identical to the unpipelined hand-over, which
    # is timed beside it (`multi_gpu_variants.raycast_exact_fps`).  KFX_BENCH_PIPELINE=0 / --no-overlap: the unpipelined one.
    can_pipeline = args.raycast == "exact" and c_driver and world > 1 and os.environ.get("KFX_BENCH_PIPELINE", "1") != "0"
    can_overlap = (args.raycast == "composite" and args.halo == "recompute" and args.inputs == "replicate") or can_pipeline
    if args.overlap and not can_overlap:
        sys.exit("bench.py: --overlap needs --raycast composite with --halo recompute and --inputs replicate (collective ordering, kangaroo_amd/pipeline.py), "
                 "or --raycast exact with --driver c (pipelined frames)")
    overlap = can_overlap if args.overlap is None else bool(args.overlap)
    if c_driver and (args.images != "all" or args.raycast == "exact_allreduce"):
        sys.exit("bench.py: --images root and --raycast exact_allreduce are options of --driver python")
    comm, comm_text = None, "torch.distributed (%s)" % dist.get_backend()
    driver, driver_note = args.driver, None
    if c_driver:
        from kangaroo_amd import slab as kslab
        err = None
        try:
            if dist.get_backend() == "nccl":
                # the library's own RCCL communicator (libkfx_rccl.so): the ncclUniqueId travels through a file named after the launch
                rdv = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kfx_bench.%d.%s.id" % (os.getuid(), os.environ.get("MASTER_PORT", "0")))
                comm = kslab.Comm.rccl(rank, world, rdv, 180)
                comm_text = "libkfx_rccl.so: RCCL communicator of the library (grouped ncclSend / ncclRecv, ncclAllReduce, ncclAllGather), collectives enqueued on the launch stream by kfx_slab_frame_step"
            else:
                comm = kslab.Comm.torch(dist)
                comm_text = "kfx_slab_frame_step with its collectives routed through torch.distributed (%s) callbacks -- the smoke-test transport for ranks sharing a GPU" % dist.get_backend()
        except Exception as e:   # noqa: BLE001
            err = repr(e)[:200]
        # every rank must drive the same way: if the library's communicator did not come up on ANY rank, all of them route the
        # frame call's collectives through the process group instead (still one C call per frame) and the line says so
        ok = torch.tensor([0 if err else 1], dtype=torch.int32, device="cuda")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            if comm is not None and dist.get_backend() == "nccl":
                comm.destroy()
            comm = kslab.Comm.torch(dist)
            driver_note = "libkfx_rccl.so's communicator did not come up on every rank (%s): collectives routed through torch.distributed (%s)" % (err or "another rank failed", dist.get_backend())
            comm_text = "kfx_slab_frame_step with its collectives routed through torch.distributed (%s) callbacks (fallback: %s)" % (dist.get_backend(), driver_note)
    steps_cap = max(256, args.steps + 4 * BLOCK + 64)
    pipeline_note = None

    def make_pipe(ovl):
        return SlabPipeline(roo, dist, (N, N, N), bmin, bmax, w, h, halo=args.halo, raycast=args.raycast, K=K, near=near, far=far,
                            overlap=ovl, inputs=args.inputs, images=args.images, merge=args.merge, driver=args.driver, comm=comm, tiles=args.tiles,
                            timing_slots=steps_cap)
    if overlap and args.raycast == "exact":
        # the pipelined frames need a second communicator (kfx_comm::dup = ncclCommSplit): if that fails on any rank, every rank runs
        # the unpipelined hand-over and the line says so (kfx_slab_frame_create agrees on nothing by itself: the ranks vote here)
        pipe, err = None, None
        try:
            pipe = make_pipe(True)
        except Exception as e:   # noqa: BLE001
            err = repr(e)[:200]
        ok = torch.tensor([0 if err else 1], dtype=torch.int32, device="cuda")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            del pipe
            overlap = False
            pipeline_note = "pipelined frames not available (%s): unpipelined hand-over" % (err or "another rank failed")
            pipe = make_pipe(False)
    else:
        pipe = make_pipe(overlap)
    sf = pipe.sframe
    poses = [scenes.orbit_pose(i, N_ORBIT) for i in range(N_ORBIT)]
    frames = []
    for T_wc in poses:
        im = roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
        im.MemcpyFromHost(scenes.render_depth(scene, w, h, T_wc, K))
        frames.append(im)

    def sync_all():
        pipe.wait_composite()   # (pipelined frames: the trailing final exchanges are enqueued, ray_d / ray_n / ray_i become the last frame's set)
        if sf is not None:
            sf.sync()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    n_updated = []
    for i in range(N_ORBIT):
        pipe.preprocess(frames[i])
        n_updated.append(roo.SdfFuseCount(pipe.vol, pipe.filtered, pipe.normals, scenes.se3_inverse(poses[i]), K, pipe.trunc, pipe.mincostheta, full_extent=True))
    # everything the host has to prepare comes BEFORE the priming frames (an idle gap right before the timed region lets the clocks drop)
    ev = None
    if sf is None:
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]
        for e4 in ev:   # (torch creates an event at its first record(): not inside the timed region)
            for e in e4:
                e.record()
    gc.collect()
    gc.disable()
    # untimed frames: --prime says exactly how many; otherwise as many as make --prime-seconds of work at the pace of a first
    # block (at least 450): at 8 ranks a frame is a fraction of a 1-GPU frame and 450 of them would be over before the clocks of a
    # GPU that was idle have settled.  The count is agreed between the ranks (every frame has collectives).
    if sf is not None:
        sf.set_timing(False)
    if args.prime is not None:
        n_prime = max(args.prime, 0)
        for i in range(n_prime):
            pipe.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
    else:
        sync_all()
        t_b = time.perf_counter()
        for i in range(BLOCK):
            pipe.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
        sync_all()
        tb = torch.tensor([time.perf_counter() - t_b], dtype=torch.float64, device="cuda")
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)
        per_frame = max(float(tb.item()) / BLOCK, 1e-6)
        n_prime = BLOCK + max(450 - BLOCK, min(int(args.prime_seconds / per_frame), 60000))
        for i in range(BLOCK, n_prime):
            pipe.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
    if sf is not None:
        sf.set_timing(sf.EVENTS_FUSE)   # the two markers around SdfFuse (its window; the frame period from one to the next): each costs ~3 us of a ~0.15 ms frame
    for i in range(args.warmup):
        pipe.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
    sync_all()
    first = sf.count if sf is not None else 0
    t0 = time.perf_counter()
    if sf is not None:
        for s in range(args.steps):
            i = (args.warmup + s) % N_ORBIT
            pipe.step(poses[i], frames[i])
    else:
        for s in range(args.steps):
            i = (args.warmup + s) % N_ORBIT
            T_wc = poses[i]
            pipe.preprocess(frames[i])
            ev[s][0].record()            # events on the stream the kernels are launched on (torch's current stream: the one roo passes to libkfx)
            pipe.fuse(T_wc)
            ev[s][1].record()
            ev[s][2].record()
            pipe.raycast(T_wc)
            ev[s][3].record()
    sync_all()
    elapsed = time.perf_counter() - t0
    gc.enable()
    tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    elapsed = float(tt.item())

    pre_avg_ms, merge_avg_ms, frame_ev_ms, period_ms = None, None, None, None
    if sf is not None:
        t = sf.timings(first, args.steps)   # preprocess, sdf_fuse (+ ghost planes), raycast, merge, frame, period
        fuse_ms = t[:, 1]
        period_ms = float(np.nanmean(t[:, 5]))
        # the parts of a frame, from as many frames with all five events right after the timed region (untimed)
        sf.set_timing(sf.EVENTS_ALL)
        n_parts = min(args.steps, 2 * N_ORBIT)
        for s in range(3):
            pipe.step(poses[s % N_ORBIT], frames[s % N_ORBIT])
        f_parts = sf.count
        for s in range(n_parts):
            i = (args.warmup + s) % N_ORBIT
            pipe.step(poses[i], frames[i])
        sync_all()
        tp = sf.timings(f_parts, n_parts)
        sf.set_timing(sf.EVENTS_NONE)
        ray_ms = tp[:, 2] + np.nan_to_num(tp[:, 3])
        pre_avg_ms, frame_ev_ms = float(np.mean(tp[:, 0])), float(np.mean(tp[:, 4]))
        merge_avg_ms = float(np.mean(tp[:, 3])) if np.isfinite(tp[:, 3]).all() else None
    else:
        fuse_ms = [ev[s][0].elapsed_time(ev[s][1]) for s in range(args.steps)]
        ray_ms = [ev[s][2].elapsed_time(ev[s][3]) for s in range(args.steps)]
    idx = [(args.warmup + s) % N_ORBIT for s in range(args.steps)]
    fuse_avg_ms, ray_avg_ms = float(np.mean(fuse_ms)), float(np.mean(ray_ms))
    bytes_avg = float(np.mean([16.0 * n_updated[i] + 20.0 * w * h for i in idx]))
    achieved = bytes_avg / (fuse_avg_ms * 1e-3) / 1e9
    local_voxels = pipe.vol.w * pipe.vol.h * pipe.vol.d
    hits = int(torch.isfinite(pipe.ray_d.tensor()).sum()) if (args.images == "all" or rank == 0) else 1
    assert hits > 0, "raycast produced no hits"
    ranks_agree = None
    if args.images != "root":   # after the merge every rank must hold the same images: compare a checksum of the depth bits
        bits = torch.nan_to_num(pipe.ray_d.tensor(), nan=-1.0).contiguous().view(torch.int32).to(torch.int64)
        chk = torch.stack([bits.sum(), -bits.sum()])
        dist.all_reduce(chk, op=dist.ReduceOp.MAX)
        ranks_agree = bool(int(chk[0].item()) == -int(chk[1].item()))
        assert ranks_agree, "ranks hold different images"

    # ---- what a first run on real links has to show without a second attempt (round-3 verdict item 8): every rank's kernel
    # times, the ghost-plane exchange and the image merge timed by themselves, and what the communicator sees ----
    def event_ms(fn, reps):
        fn()
        torch.cuda.synchronize()
        dist.barrier()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    comm_info = {"n_ranks": dist.get_world_size(), "backend": dist.get_backend(), "frame_collectives": comm_text}
    try:
        comm_info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
    except Exception as e:   # noqa: BLE001
        comm_info["rccl_version"] = "unknown (%r)" % (e,)
    per_rank = None
    try:
        lo_ghost, hi_ghost = pipe.z0 - pipe.s0, pipe.s1 - pipe.z1
        halo_bytes = (lo_ghost * (1 if rank > 0 else 0) + hi_ghost * (1 if rank < world - 1 else 0)) * pipe.vol.img_pitch   # received (= sent) per SdfFuse
        halo_ms = event_ms(pipe.exchange_halos, 5) if world > 1 else 0.0   # (torch.distributed point-to-point of the ghost planes, by itself)
        merge_ms, other_merge_ms = merge_avg_ms, None
        if sf is None and args.raycast == "composite" and world > 1:
            pipe.wait_composite()
            merge_ms = event_ms(lambda: pipe.composite(pipe.ray_d, pipe.ray_n, pipe.ray_i), 5)
            pipe.merge = "allreduce" if args.merge == "direct" else "direct"   # the other merge on the same images, by itself
            pipe.raycast(poses[idx[-1]])
            pipe.wait_composite()
            other_merge_ms = event_ms(lambda: pipe.composite(pipe.ray_d, pipe.ray_n, pipe.ray_i), 5)
            pipe.merge = args.merge
            pipe.raycast(poses[idx[-1]])   # (the images are a rendering again)
            pipe.wait_composite()
        mine = torch.tensor([fuse_avg_ms, ray_avg_ms, halo_ms, -1.0 if merge_ms is None else merge_ms, float(halo_bytes), float(pipe.z1 - pipe.z0),
                             float(local_voxels), -1.0 if other_merge_ms is None else other_merge_ms, -1.0 if pre_avg_ms is None else pre_avg_ms,
                             -1.0 if frame_ev_ms is None else frame_ev_ms], dtype=torch.float64, device="cuda")
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        opt = lambda x: None if float(x) < 0 else round(float(x), 5)   # noqa: E731
        per_rank = [{"rank": r, "preprocess_ms": opt(v[8]), "sdf_fuse_ms": round(float(v[0]), 5), "raycast_sdf_plus_merge_ms": round(float(v[1]), 5),
                     "frame_events_ms": opt(v[9]), "halo_exchange_ms": round(float(v[2]), 5),
                     "composite_merge_ms": opt(v[3]) if args.raycast == "composite" else None,
                     # pipelined exact frames: the final exchange's window on the side stream (from the end of the rank's own march to its images)
                     "final_exchange_ms": opt(v[3]) if args.raycast == "exact" else None,
                     "composite_merge_%s_ms" % ("allreduce" if args.merge == "direct" else "direct"): opt(v[7]),
                     "halo_bytes_received_per_fuse": int(v[4]), "planes_owned": int(v[5]), "voxels_stored": int(v[6])} for r, v in enumerate(allr)]
    except Exception as e:   # noqa: BLE001  (symmetric across ranks: every rank takes the same path)
        per_rank = {"error": repr(e)[:300]}

    # ---- the same frames under the other policies, reported beside the headline so that ONE multi-GPU run of the default command
    # measures all of them (not part of `value`): the north-star sentence itself -- ghost planes exchanged over RCCL + the ray
    # hand-over --, the hand-over with other tile counts, the composite (a throughput variant outside the image tolerance) with
    # its merges and the merge overlapped with the next frame, the input broadcast, and the interpreter-driven loop ----
    def timed_fps(n):
        for s in range(3):
            i = (args.warmup + s) % N_ORBIT
            pipe.step(poses[i], frames[i])
        sync_all()
        t_v = time.perf_counter()
        for s in range(n):
            i = (args.warmup + s) % N_ORBIT
            pipe.step(poses[i], frames[i])
        sync_all()
        tv = torch.tensor([time.perf_counter() - t_v], dtype=torch.float64, device="cuda")
        dist.all_reduce(tv, op=dist.ReduceOp.MAX)
        return round(n / float(tv.item()), 1)
    n_var = min(args.steps, 2 * N_ORBIT)
    variants = {"steps": n_var}
    base = dict(halo=args.halo, raycast=args.raycast, merge=args.merge, inputs=args.inputs, overlap=overlap)
    try:   # reported extras must never cost the headline line (errors in collectives are symmetric across ranks)
        variants["as_configured_fps"] = timed_fps(n_var)
        if sf is not None:
            plan = [("raycast_exact_fps", dict(base, raycast="exact", overlap=False)),
                    ("raycast_exact_pipelined_fps", dict(base, raycast="exact", overlap=True)),
                    # the hand-over's last stage kept although the ghost planes are wide enough to do without (kfx_slab_exact_ghost)
                    ("raycast_exact_pipelined_with_last_stage_fps", dict(base, raycast="exact", overlap=True, normals_stage=1)),
                    ("halo_exchange+raycast_exact_pipelined_fps", dict(base, raycast="exact", halo="exchange", overlap=True)),
                    ("raycast_exact_pipelined_tiles_1_fps", dict(base, raycast="exact", overlap=True, tiles=1)),
                    ("halo_exchange+raycast_exact_fps", dict(base, raycast="exact", halo="exchange", overlap=False)),
                    ("raycast_exact_tiles_1_fps", dict(base, raycast="exact", overlap=False, tiles=1)),
                    ("raycast_exact_tiles_8_fps", dict(base, raycast="exact", overlap=False, tiles=8)),
                    ("raycast_composite_fps", dict(base, raycast="composite", overlap=False)),
                    ("raycast_composite_overlapped_fps", dict(base, raycast="composite", halo="recompute", inputs="replicate", overlap=True)),
                    ("raycast_composite_merge_allreduce_fps", dict(base, raycast="composite", merge="allreduce", overlap=False)),
                    ("halo_%s_fps" % ("exchange" if args.halo == "recompute" else "recompute"),
                     dict(base, halo="exchange" if args.halo == "recompute" else "recompute", overlap=False)),
                    ("inputs_%s_fps" % ("broadcast" if args.inputs == "replicate" else "replicate"),
                     dict(base, inputs="broadcast" if args.inputs == "replicate" else "replicate", overlap=False))]
            for name, cfg in plan:
                cfg = dict(cfg)
                cfg.setdefault("tiles", args.tiles)
                if "pipelined" in name and pipeline_note is not None:
                    continue
                keep_stage = cfg.pop("normals_stage", 0)
                if keep_stage and pipe.GHOST <= 2:
                    continue   # (the stage is there anyway)
                pipe.configure(**cfg)
                if keep_stage:
                    sync_all()
                    kslab.set_normals_stage(1)
                variants[name] = timed_fps(n_var)
                if keep_stage:
                    sync_all()
                    kslab.set_normals_stage(0)
            pipe.configure(**dict(base, tiles=args.tiles))
            # the interpreter-driven loop on the same slabs (operators and torch.distributed collectives one by one)
            keep = pipe
            try:
                py = SlabPipeline(roo, dist, (N, N, N), bmin, bmax, w, h, halo=args.halo, raycast=args.raycast, K=K, near=near, far=far,
                                  overlap=False, inputs=args.inputs, merge=args.merge, driver="python")
                pipe = py
                for s in range(N_ORBIT):
                    pipe.step(poses[s % N_ORBIT], frames[s % N_ORBIT])
                variants["driver_python_fps"] = timed_fps(n_var)
                pipe = keep
                del py
            except Exception as e:   # noqa: BLE001
                pipe = keep
                variants["driver_python_error"] = repr(e)[:200]
        else:
            base_halo, base_overlap, base_inputs, base_images, base_merge = pipe.halo, pipe.overlap, pipe.inputs, pipe.images, pipe.merge
            pipe.wait_composite()
            pipe.overlap = False   # the ghost-plane exchange and the input broadcast never run beside an overlapped merge (SlabPipeline.__init__)
            pipe.halo = "exchange" if base_halo == "recompute" else "recompute"
            variants["halo_%s_fps" % pipe.halo] = timed_fps(n_var)
            pipe.halo = base_halo
            pipe.inputs = "broadcast" if base_inputs == "replicate" else "replicate"
            variants["inputs_%s_fps" % pipe.inputs] = timed_fps(n_var)
            pipe.inputs = base_inputs
            if args.raycast == "composite":
                if base_overlap or can_overlap:   # the merge overlapped / not overlapped with the next frame
                    pipe.overlap = not base_overlap
                    variants["overlap_%s_fps" % ("on" if pipe.overlap else "off")] = timed_fps(n_var)
                    pipe.wait_composite()
                pipe.overlap = base_overlap
                pipe.images = "root" if base_images == "all" else "all"
                variants["images_%s_fps" % pipe.images] = timed_fps(n_var)
                pipe.wait_composite()
                pipe.images = base_images
                pipe.merge = "allreduce" if base_merge == "direct" else "direct"
                variants["merge_%s_fps" % pipe.merge] = timed_fps(n_var)
                pipe.wait_composite()
            pipe.halo, pipe.overlap, pipe.inputs, pipe.images, pipe.merge = base_halo, base_overlap, base_inputs, base_images, base_merge
    except Exception as e:   # noqa: BLE001
        variants["error"] = repr(e)[:300]

    # ---- the N = 1 point of THIS machine with the SAME kernels (the plain SdfFuse + plain march, one kfx_frame_step per frame, no
    # brick summary -- slabs march without it): what a strong-scaling efficiency of `value` is to be computed against.  Every rank
    # runs it on its own GPU (1 GiB more), rank 0's figure is reported. ----
    baseline = None
    try:
        sync_all()
        one = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, track=False, timing_slots=256)
        for i in range(4 * N_ORBIT):
            one.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
        torch.cuda.synchronize()
        t_1 = time.perf_counter()
        n_1 = 2 * N_ORBIT
        for i in range(n_1):
            one.step(poses[i % N_ORBIT], frames[i % N_ORBIT])
        torch.cuda.synchronize()
        baseline = {"frames_per_sec": round(n_1 / (time.perf_counter() - t_1), 1), "steps": n_1,
                    "note": "this rank's GPU alone on the whole %d^3 volume: kfx_sdf_fuse + kfx_raycast_sdf (no brick summary), one kfx_frame_step per frame, "
                            "%d steps after %d untimed ones -- the same kernels the slabs run (the N = 1 headline of bench.py --gpus 1 may "
                            "run the tracked pair, which slabs do not have)" % (N, n_1, 4 * N_ORBIT)}
        del one
        torch.cuda.empty_cache()
        dist.barrier()
    except Exception as e:   # noqa: BLE001
        baseline = {"error": repr(e)[:300]}

    out = None
    if rank == 0:
        tiles_text = "" if args.raycast != "exact" or sf is None else ", %d image row-tiles" % (args.tiles or 4)
        partition = "z-slabs x%d, inputs %s, ghost planes %s%s, raycast %s" % (
            world, "preprocessed by every rank" if args.inputs == "replicate" else "preprocessed by rank 0 and broadcast", args.halo,
            ", merge overlapped with the next frame" if overlap and args.raycast == "composite" else "",
            {"composite": ("composite = all_to_all(image strips to their owners) + nearest hit per pixel + %s(merged strips)" % ("gather-to-rank-0" if args.images == "root" else "all_gather")
                           if args.merge == "direct" else
                           "composite = all_reduce(MIN key) + %s(SUM payload)" % ("reduce-to-rank-0" if args.images == "root" else "all_reduce")),
             "exact": ("exact = march state handed from slab to slab as tokens over image row-tiles (world + tiles - 1 steps of one tile-sized neighbour "
                       "send/recv each, one whole-image stage for the normals of hits that fell back across a slab boundary -- dropped when the ghost planes are wide enough for the finder to hold every hit's gradient stencil --, then the finalised pixels by "
                       "all_to_all + all_gather of image strips)%s%s" % (tiles_text, ("; frames pipelined: frame k's final exchange on the side stream / second "
                                                                                      "communicator under frame k + 1" if overlap and args.raycast == "exact" else ""))
                       if sf is not None else
                       "exact = march state handed from slab to slab: world + 1 stages, neighbour send/recv between them, one all_reduce of the finalised pixels at the end"),
             "exact_allreduce": "exact (cross-check) = one SUM all_reduce of the march state + a host-side termination test per round"}[args.raycast])
        parity = ("bit-identical to RaycastSdf on the single volume (tests/test_cpp_slabs.py, tests/mp_slab_gpu.py: 2 / 3 / 4 / 8 ranks, 1 / 4 / 8 tiles)"
                  if args.raycast != "composite" else
                  "OUTSIDE the single-GPU image tolerance: the march restarts at each slab entry, so silhouette rays can end differently -- 512^3 / 8 slabs, "
                  "S_room: 85 of 307 200 pixels change between hit and miss (2.8e-4 against the 2e-5 of tests/test_gpu_chain.py), depth of common hits "
                  "within 2.3e-5 m (99 %%); a throughput variant, --raycast exact is the default")
        out = {
            "metric": "kinectfusion_frames_per_sec_640x480_to_512cubed_tsdf",
            "value": round(args.steps / elapsed, 3),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "prime": n_prime,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "strong_scaling_baseline_fps": None if not baseline else baseline.get("frames_per_sec"),
            "strong_scaling_baseline": baseline,
            "config": {
                "workload": workload_text(args, n_prime, True),
                "volume": [N, N, N], "image": [w, h], "scene": scene,
                "backend": os.environ.get("KFX_BENCH_BACKEND", "nccl (RCCL)"), "ranks_agree": ranks_agree,
                "driver": ("c: one kfx_slab_frame_step call per frame and rank (launches and collectives enqueued by libkfx)" if sf is not None else
                           "python: SlabPipeline issues operators and torch.distributed collectives one by one"),
                "driver_note": driver_note, "pipeline_note": pipeline_note,
                "frames_pipelined": bool(overlap and args.raycast == "exact"),
                # ghost planes per side; wider than 2 = kfx_slab_exact_ghost: every rank finalises the hits it finds, the hand-over runs without its last stage
                "ghost_planes": int(pipe.GHOST),
                "raycast": "plain march (kfx_raycast_sdf%s) per slab" % ("_slab, state carried across slabs" if args.raycast != "composite" else ""),
                "raycast_mode": args.raycast, "raycast_parity": parity, "summary_policy": None,
                "partition": partition, "communicator": comm_info,
                "math": MATH_TEXT[args.math],
            },
            "roofline": {
                "kernel": "k_sdf_fuse_tiled<%s> (SdfFuse, %s math)" % ("true" if args.math == "fast" else "false", args.math),
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": None, "traffic_source": None,
                "algorithmic_bytes_per_launch": round(bytes_avg), "avg_launch_ms": round(fuse_avg_ms, 5),
                "timing": ("hipEvents recorded by kfx_slab_frame_step on the launch stream around the SdfFuse call of every timed step" if sf is not None else
                           "torch.cuda events on torch's current stream, which is the stream every launch of this run is issued on"),
                "updated_fraction": round(float(np.mean([n_updated[i] for i in idx])) / local_voxels, 4),
                "full_sweep_GBps": round(16.0 * local_voxels / (fuse_avg_ms * 1e-3) / 1e9, 1),
                "note": "rank-0 slab (with its ghost planes when they are recomputed)",
            },
            "kernels_ms": {"preprocess": None if pre_avg_ms is None else round(pre_avg_ms, 5), "sdf_fuse": round(fuse_avg_ms, 5),
                           "raycast_sdf+%s" % ("handover" if args.raycast != "composite" else "composite"): round(ray_avg_ms, 5),
                           "frame_events": None if frame_ev_ms is None else round(frame_ev_ms, 5), "frame_total": round(1e3 * elapsed / args.steps, 5),
                           "frame_period_events": None if period_ms is None else round(period_ms, 5),
                           "host_gap": None if period_ms is None else round(1e3 * elapsed / args.steps - period_ms, 5),
                           "note": "sdf_fuse: events of the timed steps; preprocess / raycast / frame_events: frames with all five events right after the "
                                   "timed region; host_gap = frame by the host clock - frame period by the events of the timed steps"},
            "per_rank": per_rank,
            "multi_gpu_variants": variants,
        }
    if comm is not None and c_driver and dist.get_backend() == "nccl" and driver_note is None:
        pipe.sframe = None
        del sf
        comm.destroy()
    return out


def main():
    args = parse()
    if args.dump_outputs and args.gpus > 1:
        sys.exit("bench.py: --dump-outputs is an option of --gpus 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)   # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (the product path has no CPU fallback)")
    ndev = torch.cuda.device_count()
    dev = local_rank % max(ndev, 1)
    torch.cuda.set_device(dev)
    distributed = world > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL needs one GPU per rank; KFX_BENCH_BACKEND=gloo lets several ranks share a GPU to smoke-test the
        # distributed code path on a 1-GPU box (never used for reported numbers)
        backend = os.environ.get("KFX_BENCH_BACKEND", "nccl")
        if backend == "nccl" and ndev < world:
            sys.exit("bench.py: --gpus %d needs %d GPUs, this node shows %d (KFX_BENCH_BACKEND=gloo lets ranks share a GPU "
                     "for smoke tests only)" % (world, world, ndev))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)

    from kangaroo_amd import roo, scenes
    roo.set_math_mode(args.math)
    if distributed:
        # a collective that never completes (a communicator that came up wrong, mismatched legs) would hang the ranks for ever: a
        # watchdog ends the process instead, with a line on stderr that says where it stood (KFX_BENCH_WATCHDOG_S, default 900 s)
        import threading
        limit = float(os.environ.get("KFX_BENCH_WATCHDOG_S", "900"))
        done = threading.Event()

        def watchdog():
            if not done.wait(limit):
                print("bench.py: rank %d: no result after %.0f s -- a collective seems to hang; giving up (KFX_BENCH_PIPELINE=0 selects the "
                      "unpipelined hand-over, --driver python the torch.distributed collectives)" % (rank, limit), file=sys.stderr, flush=True)
                os._exit(3)
        threading.Thread(target=watchdog, daemon=True).start()
        out = run_slabs(args, torch, dist, roo, scenes, rank, world)
        done.set()
    else:
        out = run_single(args, torch, roo, scenes, rank)
    if rank == 0:
        if args.full and not args.no_cpu_baseline and not distributed:
            try:
                out["cpu_baseline"] = cpu_baseline(args, args.scene, args.cpu_frames)
            except Exception as e:  # the baseline is a reported extra; never lose the GPU number
                out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        if args.full and not distributed:
            out["summary"] = make_summary(out)   # last key of the line
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
