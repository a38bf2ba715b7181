"""Recorders for tests/test_pipeline_trace_cpu.py: an operator set and a `dist` that perform nothing and write down every call
kangaroo_amd/pipeline.py makes -- name, arguments, keywords -- with buffers named by the pipeline attribute they are.  The traces of
a fixed list of configurations are kept under tests/golden/pipeline_trace/; `python tests/pipeline_trace.py --write` records them.
No GPU, no libkfx, no oracle."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "pipeline_trace")
N, W, H = 16, 32, 24   # two bricks per axis; four pyramid levels down to 4 x 3
BOXMIN, BOXMAX = (-1.0, -1.0, 0.5), (1.0, 1.0, 2.5)


class Obj:
    """a buffer or handle: `label` is what it is called when no pipeline attribute holds it; a view is named after its parent"""

    def __init__(self, label, parent=None):
        self.label, self.parent = label, parent


class Tensor(Obj):
    """what Image.tensor() / BoundedVolume.planes() hand to a collective"""
    is_cuda = False
    device = torch.device("cpu")


class Trace:
    def __init__(self):
        self.lines, self.pipe = [], None

    # -- names ---------------------------------------------------------------------------------------------------------
    def _names(self):
        names, tensors = {}, []

        def add(obj, name):
            if isinstance(obj, Obj):
                old = names.get(id(obj))
                if old is None or (old.startswith("_"), old) > (name.startswith("_"), name):
                    names[id(obj)] = name
                for l, img in enumerate(getattr(obj, "imgs", ())):
                    add(img, "%s[%d]" % (name, l))
            elif isinstance(obj, (tuple, list)):
                for k, v in enumerate(obj):
                    add(v, "%s[%d]" % (name, k))
            elif torch.is_tensor(obj):
                tensors.append((name, obj))
            elif hasattr(obj, "pool") and torch.is_tensor(obj.pool):   # a bricks.DeviceBrickStore
                tensors.append((name + ".pool", obj.pool))
                if torch.is_tensor(obj._scratch):
                    tensors.append((name + ".scratch", obj._scratch))
        if self.pipe is not None:
            for name, v in sorted(self.pipe.__dict__.items()):
                if name == "_scratch_cache":
                    for (n, shape), t in v.items():
                        tensors.append(("scratch:%s%s" % (n, list(shape)), t))
                else:
                    add(v, name)
        return names, tensors

    def fmt(self, x, names=None, tensors=None):
        if names is None:
            names, tensors = self._names()
        f = lambda v: self.fmt(v, names, tensors)
        if isinstance(x, Obj):
            if id(x) in names:
                return names[id(x)]
            return (f(x.parent) + "." if x.parent is not None else "") + x.label
        if torch.is_tensor(x):
            for name, t in tensors:
                base, size = t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()
                if size and base <= x.data_ptr() < base + size:
                    off, n = x.data_ptr() - base, x.numel() * x.element_size()
                    return name if (off == 0 and n == size) else "%s[+%d:%d]" % (name, off, n)
            return "tensor<%s,%s>" % (str(x.dtype).replace("torch.", ""), list(x.shape))
        if isinstance(x, np.ndarray):
            if x.size > 16:
                return "array<%s,%s>" % (x.dtype, list(x.shape))
            return "[" + ",".join(f(v) for v in x.reshape(-1).tolist()) + "]"
        if isinstance(x, (bool, np.bool_)):
            return str(bool(x))
        if isinstance(x, (float, np.floating)):
            return "%.6g" % float(x)
        if isinstance(x, (int, np.integer)):
            return str(int(x))
        if isinstance(x, (tuple, list)):
            return "(" + ",".join(f(v) for v in x) + ")"
        if isinstance(x, dict):
            return "{" + ",".join("%s:%s" % (k, f(x[k])) for k in sorted(x)) + "}"
        if isinstance(x, P2POp):
            return "P2POp(%s,%s,%d)" % (x.op.__name__, f(x.tensor), x.peer)
        if callable(x):
            return "<callable>"
        return str(x)

    def add(self, name, *args, **kw):
        names, tensors = self._names()
        parts = [self.fmt(a, names, tensors) for a in args] + ["%s=%s" % (k, self.fmt(v, names, tensors)) for k, v in kw.items()]
        self.lines.append("%s(%s)" % (name, ", ".join(parts)))


# -- the operator set ---------------------------------------------------------------------------------------------------
class Image(Obj):
    def __init__(self, w, h, kind="f32", pitch=None):
        super().__init__("Image<%dx%d,%s>" % (w, h, kind))
        self.w, self.h, self.kind = int(w), int(h), kind
        self._tensor = Tensor("tensor()", self)

    def tensor(self):
        return self._tensor

    def SubImage(self, x, y, w, h):
        sub = Image(w, h, self.kind)
        sub.label, sub.parent = "SubImage(%d,%d,%d,%d)" % (x, y, w, h), self
        return sub


class Pyramid(Obj):
    def __init__(self, w, h, levels, kind="f32"):
        super().__init__("Pyramid<%dx%d,%d,%s>" % (w, h, levels, kind))
        self.imgs = [Image(w >> l, h >> l, kind) for l in range(levels)]
        for l, img in enumerate(self.imgs):
            img.label, img.parent = "[%d]" % l, self

    def __getitem__(self, l):
        return self.imgs[l]

    def __len__(self):
        return len(self.imgs)


class Volume(Obj):
    def __init__(self, label, w, h, d, boxmin, boxmax, kind, parent=None):
        super().__init__(label, parent)
        self.w, self.h, self.d, self.kind = int(w), int(h), int(d), kind
        self.boxmin, self.boxmax = np.asarray(boxmin, np.float32), np.asarray(boxmax, np.float32)

    def SubVolume(self, start, size):
        return Volume("SubVolume(%s,%s)" % (tuple(start), tuple(size)), size[0], size[1], size[2], self.boxmin, self.boxmax, self.kind, self)

    def ZSlab(self, z0, z1):
        return Volume("ZSlab(%d,%d)" % (z0, z1), self.w, self.h, z1 - z0, self.boxmin, self.boxmax, self.kind, self)

    def planes(self, z0, z1):
        return Tensor("planes(%d,%d)" % (z0, z1), self)

    def moved(self, shift):
        voxel = (self.boxmax - self.boxmin) / (np.array([self.w, self.h, self.d], np.float32) - 1)
        self.boxmin, self.boxmax = self.boxmin + voxel * np.asarray(shift, np.float32), self.boxmax + voxel * np.asarray(shift, np.float32)


class Method:
    """obj.name(...) written down as "<obj>.name(...)" """

    def __init__(self, t, obj, name, result=None):
        self.t, self.obj, self.name, self.result = t, obj, name, result

    def __call__(self, *a, **kw):
        self.t.add(self.t.fmt(self.obj) + "." + self.name, *a, **kw)
        return self.result(*a, **kw) if callable(self.result) else self.result


class Ops:
    """Every operator pipeline.py names, except those in `without`.  rmse: what the refinements of the frames report, in turn."""
    NAMES = ("DepthToVboNormals DepthToVbo NormalsFromVbo BrickUnpack BrickPoolSpill BrickPoolRestore BrickPoolInit "
             "SdfReset ColorReset RaycastSdf RaycastSdfColor SdfFuseColor SdfFuse BilateralFilter DepthPyramidVboNormals BoxReduceIgnoreInvalid "
             "RaycastSdfColorLevels RaycastSdfLevels SdfFuseColorSlab RaycastStateToImages CompositePack CompositeSelect "
             "CompositeUnpack CompositeStripsPack CompositeStripsMerge CompositeStripsUnpack").split()
    OBJECTS = "Image Pyramid BoundedVolume Frame SdfSummary DepthInput SdfFuseBound".split()
    CANNED = ("shift_scratch BrickPoolBytes BrickPoolScratchBytes BrickPoolStats IcpRefine PoseStep PoseRefinementProjectiveIcpPointPlane "
              "CompositeStripPixels RaycastSdfSlab RaycastSdfSlabColor VolumeShift BrickPack").split()

    def __init__(self, t, without=(), rmse=()):
        self.t, self.without, self.rmse = t, set(without), list(rmse)
        self.Image, self.Pyramid = Image, Pyramid

    def __getattr__(self, name):
        if name.startswith("_") or name in self.without or name not in self.NAMES + self.OBJECTS + self.CANNED:
            raise AttributeError(name)
        if name in self.NAMES:
            return lambda *a, **kw: self.t.add(name, *a, **kw)
        return getattr(self, "_" + name)

    def _BoundedVolume(self, w, h, d, boxmin, boxmax, kind="f32"):
        self.t.add("BoundedVolume", w, h, d, np.asarray(boxmin, np.float32), np.asarray(boxmax, np.float32), kind)
        return Volume("Volume<%s>" % kind, w, h, d, boxmin, boxmax, kind)

    def _SdfSummary(self, vol):
        self.t.add("SdfSummary", vol)
        s = Obj("SdfSummary")
        s.rebuild = Method(self.t, s, "rebuild")
        return s

    def _SdfFuseBound(self, vol, depth, *a, **kw):
        self.t.add("SdfFuseBound", vol, depth, *a, **kw)
        b = Obj("bound:" + self.t.fmt(depth))
        return Method(self.t, b, "call")

    def _DepthInput(self, *a):
        self.t.add("DepthInput", *a)
        d = Obj("DepthInput")
        d.submit, d.filter = Method(self.t, d, "submit"), Method(self.t, d, "filter")
        return d

    def _Frame(self, vol, *a, **kw):
        self.t.add("Frame", vol, *a, **kw)
        f, t = Obj("Frame"), self.t
        f.count, f.track, f.EVENTS_FUSE, f.PREPROCESS, f.FUSE, f.RAYCAST = 0, False, 2, 1, 2, 4
        summary = Obj("summary()", f)
        summary.rebuild = Method(t, summary, "rebuild")

        def step(*a, **kw):
            f.count += 1

        def set_track(on):
            f.track = bool(on)
        f.step, f.set_track, f.shift = Method(t, f, "step", step), Method(t, f, "set_track", set_track), Method(t, f, "shift", lambda s, scratch: vol.moved(s))
        f.summary, f.set_timing, f.reset, f.set_input = lambda: summary, Method(t, f, "set_timing"), Method(t, f, "reset"), Method(t, f, "set_input")
        f.timings = Method(t, f, "timings", lambda first, n: np.ones((n, 5), np.float32))
        return f

    def _shift_scratch(self, vol, shift):
        self.t.add("shift_scratch", vol, shift)
        return Obj("shift_scratch")

    def _VolumeShift(self, vol, shift, *a, **kw):
        self.t.add("VolumeShift", vol, shift, *a, **kw)
        vol.moved(shift)   # (as the operator does: follow_shift reads the box)

    def _BrickPack(self, vol, fill):
        self.t.add("BrickPack", vol, fill)
        return torch.zeros(1, dtype=torch.int32), torch.zeros((1, 512 * (8 if vol.kind == "f32" else 4)), dtype=torch.uint8)

    def _BrickPoolBytes(self, kind, capacity):
        return 64

    def _BrickPoolScratchBytes(self, view, capacity):
        return 16

    def _BrickPoolStats(self, pool, kind, capacity):
        self.t.add("BrickPoolStats", pool, kind, capacity)
        return dict(occupied=0, spilled=0, restored=0, dropped=0)

    def _IcpRefine(self, *a, before_wait=None, **kw):
        self.t.add("IcpRefine", *a, before_wait=before_wait, **kw)
        if before_wait is not None:
            before_wait()
        rmse = self.rmse.pop(0) if self.rmse else 0.01
        return np.eye(4), rmse, 10, bool(rmse < 0.1)

    def _PoseStep(self, T_wl, T_lp):
        self.t.add("PoseStep", T_wl, T_lp)
        return np.eye(4), np.eye(4, dtype=np.float32)[:3]

    def _PoseRefinementProjectiveIcpPointPlane(self, *a):
        self.t.add("PoseRefinementProjectiveIcpPointPlane", *a)
        lss = Obj("lss")
        lss.JTJ, lss.JTy, lss.sqErr, lss.obs = np.zeros((6, 6)), np.zeros(6), 0.0, 1
        return lss

    def _CompositeStripPixels(self, w, h, world):
        return ((w * h + world - 1) // world + 63) // 64 * 64

    def _RaycastSdfSlab(self, state, *a, name="RaycastSdfSlab"):
        self.t.add(name, state, *a)
        state[3] = 1.0                        # every ray final ...
        state.view(torch.int32)[4] = 1        # ... and touched by this rank

    def _RaycastSdfSlabColor(self, state, *a):
        self._RaycastSdfSlab(state, *a, name="RaycastSdfSlabColor")


# -- dist ---------------------------------------------------------------------------------------------------------------
class P2POp:
    def __init__(self, op, tensor, peer):
        self.op, self.tensor, self.peer = op, tensor, peer


class Dist:
    """torch.distributed as far as pipeline.py uses it: nothing is transferred"""
    P2POp = P2POp

    class ReduceOp:
        MIN, SUM = "MIN", "SUM"

    class _Req:
        def wait(self):
            pass

    def __init__(self, t, rank, world):
        self.t, self.rank, self.world = t, rank, world

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def get_backend(self):
        return "gloo"

    def isend(self, *a):
        raise AssertionError("point-to-point operations go through batch_isend_irecv")

    def irecv(self, *a):
        raise AssertionError("point-to-point operations go through batch_isend_irecv")

    def all_reduce(self, tensor, **kw):
        self.t.add("dist.all_reduce", tensor, **kw)

    def reduce(self, tensor, **kw):
        self.t.add("dist.reduce", tensor, **kw)

    def broadcast(self, tensor, **kw):
        self.t.add("dist.broadcast", tensor, **kw)
        if torch.is_tensor(tensor) and tensor.numel() == 18 and self.rank != 0:   # the tracker's pose message: identity, rmse, good
            tensor[:16], tensor[16], tensor[17] = torch.eye(4, dtype=tensor.dtype).reshape(16), 0.01, 1.0

    def batch_isend_irecv(self, ops):
        self.t.add("dist.batch_isend_irecv", list(ops))
        return [self._Req() for _ in ops]


# -- the configurations ---------------------------------------------------------------------------------------------------
def pose(k):
    """camera k of a stream: the identity, moved 1 cm per frame along x"""
    T = np.eye(4, dtype=np.float32)[:3].copy()
    T[0, 3] = 0.01 * k
    return T


def state(t, p, names):
    vals = {n: getattr(p, n) for n in names}
    if "track_decision" in vals and vals["track_decision"] is not None:
        d = vals["track_decision"]
        vals["track_decision"] = (d["chosen"], d["clock"], d["frame_tracked_ms"], d["frame_plain_ms"])
    if "_cal" in vals:
        vals["_cal"] = vals["_cal"] is not None
    t.add("state", **vals)


FRAME_STATE = ("frames_done", "track", "track_policy", "track_decision", "_cal", "shifts", "origin", "_restored")
TRACK_STATE = FRAME_STATE + ("frame", "resets", "rmse", "tracking_good", "T_wl")


def device_store_on_host(monkeypatch):
    """bricks.DeviceBrickStore allocates its pool on "cuda": here on the host"""
    from kangaroo_amd import bricks

    class HostPool(bricks.DeviceBrickStore):
        def __init__(self, kind, capacity, ops=None, device="cpu"):
            super().__init__(kind, capacity, ops, device)
    monkeypatch.setattr(bricks, "DeviceBrickStore", HostPool)


def fake_clock(monkeypatch):
    """track="auto" on the host clock: every reading one second after the last, so the decision is the same everywhere"""
    now = [0.0]

    def tick():
        now[0] += 1.0
        return now[0]
    monkeypatch.setattr(time, "perf_counter", tick)


def follow_pose(p, shift):
    """the pose whose camera centre is `shift` cells from the box centre (focus 0: the target is the camera centre)"""
    lo, hi = np.asarray(p.vol.boxmin, np.float64), np.asarray(p.vol.boxmax, np.float64)
    T = np.eye(4, dtype=np.float32)[:3].copy()
    T[:, 3] = 0.5 * (lo + hi) + np.asarray(shift, np.float64) * (hi - lo) / (N - 1)
    return T


def run_frame_follow_pool(monkeypatch):
    from kangaroo_amd import pipeline
    device_store_on_host(monkeypatch)
    t = Trace()
    p = t.pipe = pipeline.FramePipeline(Ops(t), (N, N, N), BOXMIN, BOXMAX, W, H, track=True, follow=dict(focus=0.0, quantum=8, slack=4, spill="device"))
    for shift in ((0, 0, 0), (8, 0, 0), (8, -8, 0), (8, 8, -8), (0, 0, 0)):
        p.step(follow_pose(p, shift))
    p.preprocess(), p.fuse(pose(1)), p.raycast(pose(1))
    t.add("restored", p.restored)
    state(t, p, FRAME_STATE)
    p.reset()
    return t.lines


def run_frame_colour_host_store(monkeypatch):
    from kangaroo_amd import pipeline
    t = Trace()
    p = t.pipe = pipeline.FramePipeline(Ops(t), (N, N, N), BOXMIN, BOXMAX, W, H, color=True, track=True, follow=dict(focus=0.0, quantum=8, slack=4, spill=True))
    for k, shift in enumerate(((0, 0, 0), (8, 0, 0), (-8, 0, 0), (0, 0, 0))):
        p.step(follow_pose(p, shift), rgb_image=Image(W, H, "u8x3") if k == 3 else None)
    state(t, p, FRAME_STATE)
    p.reset()
    state(t, p, FRAME_STATE)
    return t.lines


def run_frame_plain(monkeypatch, **kw):
    """the separate operators of the known-pose loop (an operator set without the one-call frame)"""
    from kangaroo_amd import pipeline
    t = Trace()
    p = t.pipe = pipeline.FramePipeline(Ops(t, without=("Frame", "DepthToVboNormals") if kw.get("kind") else ("Frame",)), (N, N, N), BOXMIN, BOXMAX, W, H, **kw)
    if kw.get("sensor"):
        p.submit(np.zeros((H, W), np.uint16))
    for k in range(3):
        p.step(pose(k), None if kw.get("sensor") or k == 0 else Image(W, H))
    p.shift_volume((1, 0, -2))
    state(t, p, FRAME_STATE)
    p.reset()
    return t.lines


def run_auto_frame(monkeypatch):
    from kangaroo_amd import pipeline
    t = Trace()
    p = t.pipe = pipeline.FramePipeline(Ops(t), (N, N, N), BOXMIN, BOXMAX, W, H, track="auto", cal_first=1, cal_block=2)
    for k in range(9):
        p.step(pose(k))
    state(t, p, FRAME_STATE)
    p.recalibrate(1)
    p.step(pose(9)), p.step(pose(10))
    p.reset()
    state(t, p, FRAME_STATE)
    return t.lines


def run_auto_tracking(monkeypatch):
    from kangaroo_amd import pipeline
    fake_clock(monkeypatch)
    t = Trace()
    p = t.pipe = pipeline.TrackingPipeline(Ops(t), (N, N, N), BOXMIN, BOXMAX, W, H, track="auto", cal_first=1, cal_block=2, device_icp=True)
    for k in range(9):
        p.step(pose(0) if k == 0 else None)
    state(t, p, TRACK_STATE)
    return t.lines


def run_tracking_device(monkeypatch, **kw):
    """device_icp with the next frame's pre-amble prefetched; frame 3's refinement finds nothing, so frame 4 recovers"""
    from kangaroo_amd import pipeline
    t = Trace()
    nan = float("nan")
    p = t.pipe = pipeline.TrackingPipeline(Ops(t, rmse=(0.01, 0.01, nan, 0.01, 0.5, 0.01)), (N, N, N), BOXMIN, BOXMAX, W, H, device_icp=True, track=True, **kw)
    sensor = kw.get("sensor") is not None
    images = [Image(W, H) for _ in range(8)]
    if sensor:
        p.submit(np.zeros((H, W), np.uint16))
    for k in range(7):
        if sensor:
            p.submit(np.zeros((H, W), np.uint16))
            p.step(pose(0) if k in (0, 4) else None, next_image=pipeline.FROM_SENSOR if k != 2 else None)
        else:
            p.step(pose(0) if k in (0, 4) else None, images[k], next_image=images[k + 1] if k != 2 else None)
    p.shift_volume((0, 8, 0))   # (the bound SdfFuse calls are marshalled again)
    p.step(None, None if sensor else images[7])
    state(t, p, TRACK_STATE)
    p.reset()
    return t.lines


def run_tracking_per_level(monkeypatch):
    from kangaroo_amd import pipeline
    t = Trace()
    o = Ops(t, without=("IcpRefine", "PoseStep", "RaycastSdfLevels", "RaycastSdfColorLevels", "DepthPyramidVboNormals"))
    p = t.pipe = pipeline.TrackingPipeline(o, (N, N, N), BOXMIN, BOXMAX, W, H, device_icp=True, track=True, follow=dict(focus=0.0, slack=4))
    for k in range(3):
        p.step(None, Image(W, H))
    p.T_wl = np.vstack([follow_pose(p, (8, 0, 0)), [0, 0, 0, 1]]).astype(np.float64)
    p.step(None, Image(W, H))
    state(t, p, TRACK_STATE)
    return t.lines


def run_tracking_colour(monkeypatch, **kw):
    from kangaroo_amd import pipeline
    t = Trace()
    p = t.pipe = pipeline.TrackingPipeline(Ops(t, rmse=(0.01, float("nan"), 0.01), **kw), (N, N, N), BOXMIN, BOXMAX, W, H, color=True, track=True,
                                           device_icp=bool(kw), color_size=(16, 12))
    for k in range(4):
        p.step(None, Image(W, H), rgb_image=Image(16, 12, "u8x3") if k == 1 else None)
    state(t, p, TRACK_STATE)
    return t.lines


def run_slab(monkeypatch, rank, frames=3, **kw):
    from kangaroo_amd import pipeline
    t = Trace()
    p = t.pipe = pipeline.SlabPipeline(Ops(t), Dist(t, rank, 3), (N, N, N), BOXMIN, BOXMAX, W, H, driver="python", **kw)
    for k in range(frames):
        p.step(pose(k), rgb_image=Image(W, H, "u8x3") if kw.get("color") and k == 1 else None)
    if kw.get("raycast") == "composite":
        L = 3
        p.raycast_levels_into([(Image(W >> l, H >> l), Image(W >> l, H >> l, "f32x4"), Image(W >> l, H >> l)) for l in range(L)], [p.K] * L, pose(0))
        p.raycast_levels_into([(p.ray_d, p.ray_n, p.ray_i)], [p.K], pose(0))
        p.composite()
    t.add("rounds", getattr(p, "rounds", None))
    state(t, p, ("frames_done", "track", "z0", "z1", "s0", "s1", "GHOST"))
    return t.lines


def run_tracking_slab(monkeypatch, rank, **kw):
    from kangaroo_amd import pipeline
    t = Trace()
    o = Ops(t, rmse=(), **({"without": kw.pop("without")} if "without" in kw else {}))
    p = t.pipe = pipeline.TrackingSlabPipeline(o, Dist(t, rank, 2), (N, N, N), BOXMIN, BOXMAX, W, H, **kw)
    for k in range(3):
        p.step(pose(0) if k == 0 else None, Image(W, H))
    p.rmse = float("nan")   # the next frame recovers
    p.step(None, Image(W, H))
    state(t, p, ("track", "frame", "resets", "rmse", "tracking_good", "T_wl"))
    return t.lines


def _slab_cases():
    cases = {}
    for rank in (1, 0):
        for halo in ("exchange", "recompute"):
            for merge in ("direct", "allreduce"):
                for images in ("all", "root"):
                    cases["slab_composite_%s_%s_%s_r%d" % (merge, images, halo, rank)] = (
                        run_slab, dict(rank=rank, raycast="composite", merge=merge, images=images, halo=halo))
            for raycast in ("exact", "exact_allreduce"):
                cases["slab_%s_%s_r%d" % (raycast, halo, rank)] = (run_slab, dict(rank=rank, raycast=raycast, halo=halo))
        cases["slab_broadcast_composite_r%d" % rank] = (run_slab, dict(rank=rank, raycast="composite", inputs="broadcast"))
        cases["slab_broadcast_exact_r%d" % rank] = (run_slab, dict(rank=rank, raycast="exact", inputs="broadcast", halo="recompute"))
        cases["slab_colour_exact_r%d" % rank] = (run_slab, dict(rank=rank, raycast="exact", color=True))
        cases["slab_colour_composite_r%d" % rank] = (run_slab, dict(rank=rank, raycast="composite", color=True, merge="allreduce", images="root"))
        cases["slab_f16_exact_r%d" % rank] = (run_slab, dict(rank=rank, raycast="exact", kind="f16", frames=2))
    return cases


CASES = {
    "frame": {
        "frame_follow_pool": (run_frame_follow_pool, {}),
        "frame_colour_host_store": (run_frame_colour_host_store, {}),
        "frame_auto": (run_auto_frame, {}),
        "frame_plain_tracked": (run_frame_plain, dict(track=True)),
        "frame_plain_untracked_sensor": (run_frame_plain, dict(track=False, sensor="u16")),
        "frame_plain_f16": (run_frame_plain, dict(track=True, kind="f16")),
    },
    "tracking": {
        "tracking_auto": (run_auto_tracking, {}),
        "tracking_device_icp": (run_tracking_device, {}),
        "tracking_device_icp_sensor": (run_tracking_device, dict(sensor="u16")),
        "tracking_per_level": (run_tracking_per_level, {}),
        "tracking_colour": (run_tracking_colour, {}),
        "tracking_colour_per_level": (run_tracking_colour, dict(without=("RaycastSdfLevels", "RaycastSdfColorLevels", "PoseStep"))),
    },
    "slab": _slab_cases(),
    "tracking_slab": {
        "tracking_slab_root_r0": (run_tracking_slab, dict(rank=0, images="root", raycast="composite")),
        "tracking_slab_root_r1": (run_tracking_slab, dict(rank=1, images="root", raycast="composite")),
        "tracking_slab_exact_r1": (run_tracking_slab, dict(rank=1, raycast="exact", without=("PoseStep", "DepthPyramidVboNormals", "RaycastSdfLevels"))),
        "tracking_slab_allreduce_r0": (run_tracking_slab, dict(rank=0, raycast="composite", merge="allreduce", halo="recompute", without=("RaycastSdfLevels",))),
    },
}


def record(group, name, monkeypatch):
    fn, kw = CASES[group][name]
    return fn(monkeypatch, **kw)


def load(group):
    """{case: [lines]} of a fixture: the file keeps every distinct line once and each trace as indices into them"""
    with open(os.path.join(GOLDEN, group + ".json")) as f:
        z = json.load(f)
    return {name: [z["lines"][k] for k in idx] for name, idx in z["traces"].items()}


def write(group, traces):
    lines = sorted({l for tr in traces.values() for l in tr})
    at = {l: k for k, l in enumerate(lines)}
    os.makedirs(GOLDEN, exist_ok=True)
    with open(os.path.join(GOLDEN, group + ".json"), "w") as f:
        f.write('{"lines": [\n' + ",\n".join(json.dumps(l) for l in lines) + '\n],\n"traces": {\n')
        f.write(",\n".join('%s: %s' % (json.dumps(n), json.dumps([at[l] for l in tr], separators=(",", ":"))) for n, tr in traces.items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    import pytest
    assert sys.argv[1:] == ["--write"], "usage: python tests/pipeline_trace.py --write"
    mp = pytest.MonkeyPatch()
    for group in CASES:
        traces = {}
        for name in CASES[group]:
            with mp.context() as m:
                traces[name] = record(group, name, m)
        write(group, traces)
        print(group, len(traces), "traces,", sum(len(v) for v in traces.values()), "calls")
