"""Headless KinectFusion frame loop on the `roo::` operators (known poses, no ICP).

Mirrors the per-frame call order of the reference application
(applications/kinectfusion/main.cpp:200-356):

    BilateralFilter -> DepthToVbo -> NormalsFromVbo          (main.cpp:209-215)
    [RaycastSdf of the model from the current pose]           (main.cpp:286)
    SdfFuse of the new frame                                  (main.cpp:345-356)

`FramePipeline` is the single-GPU loop.  `SlabPipeline` partitions the volume into Z-slabs,
one per rank (one process per GPU): SdfFuse is embarrassingly parallel per voxel, so every
rank integrates its own slab (+ ghost planes, recomputed redundantly -- the update is
deterministic per voxel, so neighbours hold bit-identical ghosts without any exchange) and
ray-casts its own slab; the per-rank images are merged with one min-reduction over
(depth, rank) keys and one sum-reduction of the winner's payload (RCCL over xGMI through
torch.distributed; MiB-scale, latency-bound messages).

The operator set is injected (`ops`): the product passes `kangaroo_amd.roo` (HIP kernels behind
the C ABI); the CPU tests inject an oracle-backed stand-in from tests/ to exercise the
partitioning and compositing logic under gloo without a GPU.
"""
import numpy as np

from . import bricks, scenes


def vbo_normals(ops, vbo, normals, depth, K):
    """DepthToVbo + NormalsFromVbo (main.cpp:213-214); one launch where the operator set offers the fused entry point
    (identical outputs), else the two operators."""
    if hasattr(ops, "DepthToVboNormals"):
        ops.DepthToVboNormals(vbo, normals, depth, K)
    else:
        ops.DepthToVbo(vbo, depth, K)
        ops.NormalsFromVbo(normals, vbo)


def follow_shift(boxmin, boxmax, dims, T_wc, focus, quantum=8, slack=16):
    """The whole-cell shift that lets the box follow the camera (host, float64).  target = camera centre + focus * the camera's +z
    axis in the world; o = (target - box centre) / voxel size; per axis 0 while |o| < slack, else quantum * rint(o / quantum)
    (rint: ties to even)."""
    lo, hi = np.asarray(boxmin, np.float64).reshape(3), np.asarray(boxmax, np.float64).reshape(3)
    T = np.asarray(T_wc, np.float64).reshape(-1, 4)[:3]
    target = T[:, 3] + float(focus) * T[:, 2]
    voxel = (hi - lo) / (np.asarray(dims, np.float64).reshape(3) - 1.0)
    o = (target - 0.5 * (lo + hi)) / voxel
    q = float(quantum)
    return tuple(0 if abs(v) < slack else int(q * np.rint(v / q)) for v in o)


class WorldView:
    """What FramePipeline.world_view() returns: the model's brick lists on one frame (bricks.world_bricks) and the plan of their
    ray-cast (ops.RaycastBricksPlan), device tensors kept alive here.  lo: the frame's first world cell; dims, boxmin, boxmax: the frame;
    ids / cells the SDF list (cells of `kind`), cids / ccells the colour list (None without colour); plan: the scratch."""

    def __init__(self, kind, lo, dims, boxmin, boxmax, ids, cells, cids, ccells, plan):
        self.kind, self.lo, self.dims, self.boxmin, self.boxmax = kind, tuple(int(v) for v in lo), tuple(int(v) for v in dims), boxmin, boxmax
        self.ids, self.cells, self.cids, self.ccells, self.plan = ids, cells, cids, ccells, plan


class FramePipeline:
    # track="auto": the stream itself is the benchmark.  From frame CAL_FIRST on, three blocks of CAL_BLOCK frames each:
    # tracked pair (SdfFuse keeping the summary + march through the class tables), plain pair (the summary goes stale), tracked
    # pair again (summary rebuilt from the volume, kfx_sdf_summary_rebuild) -- whole frames, timed start to start.  The tables
    # stay only if BOTH tracked blocks beat the plain block's median frame by CAL_MARGIN; otherwise the plain pair runs from
    # then on.  Nothing is assumed about what tracking costs SdfFuse: the plain SdfFuse is in the plain block's frames.
    CAL_FIRST, CAL_BLOCK, CAL_MARGIN = 8, 60, 0.05
    USE_FRAME = True   # issue a frame through ONE library call (ops.Frame = kfx_frame) where the operator set has it

    def __init__(self, ops, dims, boxmin, boxmax, w, h, K=None, near=0.4, far=8.0, bilateral=None,
                 trunc_factor=scenes.TRUNC_DIST_FACTOR, max_w=scenes.MAX_W, mincostheta=scenes.MIN_COS_THETA,
                 contiguous_images=False, track=False, cal_first=None, cal_block=None, cal_margin=None, timing_slots=None, kind=None,
                 color=False, color_size=None, T_cd=None, sensor=None, sensor_scale=1e-3, sensor_slots=2, follow=None):
        """follow: None, or dict(focus=, quantum=, slack=) -- a volume that follows the camera.  At the start of a step, before anything
        is enqueued for the frame, follow_shift() of the current box and the frame's pose (the tracking loop: the previous frame's)
        gives a whole-cell shift; when it is not zero the volume is shifted in place on the device (ops.VolumeShift, fill NaN; the
        one-call frame: its shift()), the colour volume with it (fill 0.5), the summary is rebuilt when tracking, vol.boxmin / boxmax
        move, and (frame index, shift) is appended to self.shifts.  focus=None: the distance from the camera centre to the box centre
        at the first step.  trunc stays what it was at construction.
        follow=dict(..., spill=True): the volume keeps what leaves.  Before a shift the live 8^3 bricks of the boxes it discards are
        packed on the device (ops.BrickPack), copied to the host and kept in self.store (a bricks.BrickStore; colour: self.cstore, fill
        0.5) under world brick keys; after it the bricks the store holds of the boxes that entered are unpacked into them, and a shift
        that restored something rebuilds the summary once more.  self.origin is the running sum of the shifts in cells.  Needs a
        quantum and dims that are multiples of 8 (leaving and entering boxes are whole bricks of one world lattice); reset() forgets
        the store.  Off by default: nothing changes and no brick code runs.
        follow=dict(..., spill="device", pool_bricks=N): the same, with the stores on the device (bricks.DeviceBrickStore over
        include/kfx_brick_pool.h: one pool of N bricks for the SDF volume and one for the colour volume; N defaults to the number of
        bricks of the volume).  A shift then makes one spill call per leaving box and one restore call per entering box, all
        launches on the stream: no copy to the host, no read-back, no synchronisation.  Whether a restore put anything back is not
        known on the host, so a tracking pipeline rebuilds the summary once after the restores of every shift, and that is the
        shift's only rebuild.  A pool that is full DROPS the bricks that do not fit: they are lost, as they are without a store;
        pipe.store.dropped > 0 (a blocking read of the pool's counter) says that pool_bricks was too small.  self.restored reads the
        pools' counters (blocking).
        sensor: "u16" or "f32" -- the frames arrive as raw sensor images on the host (main.cpp:202-209): the pipeline owns an upload
        ring (ops.DepthInput, `input`) of sensor_slots slots that converts with sensor_scale (millimetres: 1e-3) while it filters.
        submit(array) hands it the next image -- one frame ahead, its copy runs beside the current frame -- and a step / preprocess
        that is given no image consumes the oldest submitted one; self.raw then holds that frame's depth in metres.
        color: the reference application's fuse_color mode (main.cpp:233, :238, :284, :353): the pipeline owns a colour volume
        (kind "c32", `cvol`) beside the SDF volume and an RGB image (`rgb`, "u8x3", color_size = (w, h) of the colour camera,
        default the depth camera's; its intrinsics `Kimg` are the application's for that size); step() fuses with SdfFuseColor at
        T_iw = T_cd * T_cw (T_cd: colour <- depth camera, 3x4 or 4x4, default identity) and renders the colour volume into ray_i.
        It runs the separate operators (the one-call frame is grey) and takes track=True / False; the tracking loop, whose
        calibration uses the host clock, also takes "auto".
        kind: the volume's cells, "f32" (SDF_t, the default) or "f16" (SDF_h, config C5); an f16 volume runs the separate
        operators (the one-call frame is fp32-only) and takes track=True / False, not "auto" (its host-clock calibration does not
        synchronise the frames it times).
        track: keep a brick summary of the volume (ops.SdfSummary) current in SdfFuse and let RaycastSdf step through
        uniformly free / never-observed space without reading the volume (same volume bits; images bit-identical in
        exact numerics, within the fast-mode tolerance in fast numerics).  True / False, or "auto": start with the summary,
        time whole frames of the stream itself with and without it and keep whichever makes the frame shorter (see CAL_*):
        the table march wins where rays cross much free space (S_full: RaycastSdf 0.15 -> 0.05 ms) and loses where the
        longest rays graze silhouettes (S_room), and which it is depends on the scene, not on anything known up front.
        During the calibration blocks the images come from the march of the block (bit-identical in exact numerics, within
        the fast-mode tolerance otherwise); reset() re-arms the calibration for the new stream, recalibrate() at any frame."""
        self.ops = ops
        if kind is not None or not hasattr(self, "kind"):   # (SlabPipeline sets its own before it gets here)
            self.kind = "f32" if kind is None else kind
        if self.kind not in ("f32", "f16"):
            raise ValueError("FramePipeline: kind must be 'f32' or 'f16', not %r" % (self.kind,))
        if track == "auto" and self.kind != "f32":
            raise ValueError("FramePipeline: track='auto' needs fp32 cells (its calibration times whole frames of the one-call frame)")
        self.color = bool(color)
        if self.color and self.kind != "f32":
            raise ValueError("FramePipeline: color=True needs fp32 cells")
        if self.color and track == "auto" and self.USE_FRAME:
            raise ValueError("FramePipeline: color=True takes track=True / False (track='auto' times whole frames of the one-call frame, which is grey)")
        self.track_policy = "auto" if track == "auto" else ("on" if track else "off")
        self.track = bool(track) and hasattr(ops, "SdfSummary")
        if self.track_policy == "auto" and not self.track:
            self.track_policy = "off"
        self.cal_first = self.CAL_FIRST if cal_first is None else int(cal_first)
        self.cal_block = self.CAL_BLOCK if cal_block is None else int(cal_block)
        self.cal_margin = self.CAL_MARGIN if cal_margin is None else float(cal_margin)
        self.track_decision = None   # auto: dict(chosen=..., ...) once decided
        self.frames_done = 0         # frames stepped since construction / reset
        self._cal = None
        self.summary = None
        self.kframe = None
        self.input = None
        self.follow, self.shifts, self._shift_scratch = None, [], None
        self.spill, self.store, self.cstore, self.origin, self._restored = False, None, None, (0, 0, 0), 0
        if follow is not None:
            if not hasattr(ops, "VolumeShift"):
                raise ValueError("FramePipeline: follow= needs an operator set with VolumeShift")
            unknown = set(follow) - {"focus", "quantum", "slack", "spill", "pool_bricks"}
            if unknown:
                raise ValueError("FramePipeline: follow= takes focus, quantum, slack and spill (and pool_bricks with spill='device'), not %s" % sorted(unknown))
            if follow.get("spill") not in (None, False, True, "device"):
                raise ValueError("FramePipeline: follow=dict(spill=) is True (a store on the host) or 'device' (a brick pool), not %r" % (follow["spill"],))
            if follow.get("pool_bricks") is not None and follow.get("spill") != "device":
                raise ValueError("FramePipeline: follow=dict(pool_bricks=) belongs to spill='device'")
            self.follow = {"focus": follow.get("focus"), "quantum": int(follow.get("quantum", 8)), "slack": float(follow.get("slack", 16))}
            if self.follow["quantum"] < 1:
                raise ValueError("FramePipeline: follow= needs quantum >= 1")
            if follow.get("spill"):
                # leaving and entering regions must be whole bricks of one world brick lattice
                if self.follow["quantum"] % bricks.BRICK or any(int(d) % bricks.BRICK for d in dims):
                    raise ValueError("FramePipeline: follow=dict(spill=True) needs a quantum and dimensions that are multiples of 8, not "
                                     "quantum %d and dims %s" % (self.follow["quantum"], tuple(int(d) for d in dims)))
                if not hasattr(ops, "BrickPack"):
                    raise ValueError("FramePipeline: follow=dict(spill=True) needs an operator set with BrickPack")
                self.spill = True
                if follow["spill"] == "device":
                    if not hasattr(ops, "BrickPoolSpill"):
                        raise ValueError("FramePipeline: follow=dict(spill='device') needs an operator set with BrickPoolSpill")
                    self.spill = "device"
                    n = follow.get("pool_bricks")
                    n = int(np.prod([int(d) // bricks.BRICK for d in dims])) if n is None else int(n)
                    if n < 1:
                        raise ValueError("FramePipeline: follow=dict(pool_bricks=) is at least 1, not %d" % n)
                    self.store = bricks.DeviceBrickStore(self.kind, n, ops)
                    self.cstore = bricks.DeviceBrickStore("c32", n, ops) if self.color else None
                else:
                    self.store = bricks.BrickStore(self.kind, ops)
                    self.cstore = bricks.BrickStore("c32", ops) if self.color else None
        if sensor is not None:
            if not hasattr(ops, "DepthInput"):
                raise ValueError("FramePipeline: sensor= needs an operator set with DepthInput")
            if sensor not in ("u16", "f32"):
                raise ValueError("FramePipeline: sensor must be 'u16' or 'f32', not %r" % (sensor,))
        self.dims = tuple(int(d) for d in dims)
        self.w, self.h = int(w), int(h)
        self.K = scenes.intrinsics(w, h) if K is None else np.asarray(K, np.float32)
        self.near, self.far = float(near), float(far)
        self.bil = dict(scenes.BILATERAL if bilateral is None else bilateral)
        self.max_w, self.mincostheta = float(max_w), float(mincostheta)
        # trunc_dist = factor * length(VoxelSizeUnits()) of the FULL volume (main.cpp:221)
        self.trunc = scenes.trunc_dist(boxmin, boxmax, self.dims, trunc_factor)
        self.vol = self._alloc_volume(boxmin, boxmax)
        pf = (lambda e: self.w * e) if contiguous_images else (lambda e: None)
        I = ops.Image
        self.raw = I(w, h, "f32", pitch=pf(4))
        self.filtered = I(w, h, "f32", pitch=pf(4))
        self.vbo = I(w, h, "f32x4", pitch=pf(16))
        self.normals = I(w, h, "f32x4", pitch=pf(16))
        self.ray_d = I(w, h, "f32", pitch=pf(4))
        self.ray_n = I(w, h, "f32x4", pitch=pf(16))
        self.ray_i = I(w, h, "f32", pitch=pf(4))
        if self.color:
            cw, ch = (self.w, self.h) if color_size is None else (int(color_size[0]), int(color_size[1]))
            self.cvol = self._alloc_color_volume(boxmin, boxmax)
            self.rgb = I(cw, ch, "u8x3")
            self.Kimg = scenes.intrinsics(cw, ch)
            T_cd = scenes.identity_pose() if T_cd is None else np.asarray(T_cd, np.float32).reshape(-1, 4)[:3]
            self.T_cd = np.vstack([T_cd, [0, 0, 0, 1]]).astype(np.float32)
            self._rgb_now = self.rgb
        if self.USE_FRAME and hasattr(ops, "Frame") and getattr(self.vol, "kind", "f32") == "f32" and not self.color:
            self.kframe = ops.Frame(self.vol, self.raw, self.filtered, self.vbo, self.normals, self.ray_d, self.ray_n, self.ray_i, self.K,
                                    self.bil, self.near, self.far, self.trunc, self.max_w, self.mincostheta,
                                    timing_slots=max(256, 3 * self.cal_block + 16, int(timing_slots or 0)))
        # the frame's device events are markers between launches and cost the stream a few microseconds each (all four: 2.7 % of a
        # 0.42 ms frame): none are recorded unless the caller asks (set_timing) or the auto policy is timing its blocks
        self.timing = 0
        if self.kframe is not None:
            self.kframe.set_timing(self.timing)
        if sensor is not None:
            self.input = ops.DepthInput(self.w, self.h, sensor, sensor_scale, 0.0, sensor_slots)
            if self.kframe is not None:
                self.kframe.set_input(self.input)
        track_now, self.track = self.track, False
        self.set_track(track_now)
        self.reset()

    # -- overridable pieces ------------------------------------------------------
    def _alloc_volume(self, boxmin, boxmax):
        if self.kind != "f32":   # (the CPU tests' oracle-backed volumes are fp32 and take no kind)
            return self.ops.BoundedVolume(self.dims[0], self.dims[1], self.dims[2], boxmin, boxmax, kind=self.kind)
        return self.ops.BoundedVolume(self.dims[0], self.dims[1], self.dims[2], boxmin, boxmax)

    def _alloc_color_volume(self, boxmin, boxmax):
        return self.ops.BoundedVolume(self.dims[0], self.dims[1], self.dims[2], boxmin, boxmax, kind="c32")

    def set_track(self, on):
        """Switch between the tracked pair of kernels and the plain pair.  Switching on (re)builds the summary from what the
        volume holds, so it may follow any number of untracked frames."""
        on = bool(on) and hasattr(self.ops, "SdfSummary")
        if self.kframe is not None:
            self.kframe.set_track(on)
            self.summary = self.kframe.summary() if on else None
        elif on and not self.track:
            if self.summary is None:
                self.summary = self.ops.SdfSummary(self.vol)
            self.summary.rebuild()
        self.track = on

    def set_timing(self, mask):
        """Which device events kfx_frame_step records from now on (ops.Frame.EVENTS_ALL / EVENTS_FUSE / EVENTS_NONE): what
        self.kframe.timings() can answer afterwards."""
        self.timing = int(mask)
        if self.kframe is not None:
            self.kframe.set_timing(self.timing)

    def recalibrate(self, first=None):
        """track="auto": time the three blocks again, starting `first` frames from now (default: at once) -- e.g. once a
        stream has reached its steady state."""
        if self.track_policy != "auto":
            return
        self.track_decision = None
        self._cal = {"first": self.frames_done + (0 if first is None else int(first)), "t": [], "clock": None}
        self.set_track(True)

    def reset(self):
        """SdfReset(vol, NaN): 'never observed' = (NaN, 0) (main.cpp:229).  A new stream: track="auto" starts over with the
        summary and calibrates on the new stream."""
        self.frames_done = 0
        if self.track_policy == "auto":
            self.track_decision = None
            # cal_first < 0: no calibration until the caller asks for one (recalibrate()); the tracked pair runs meanwhile
            self._cal = {"first": self.cal_first, "t": [], "clock": None} if self.cal_first >= 0 else None
            if not self.track:
                self.set_track(True)
        self._reset_model()

    def _summary_kw(self):
        """the keyword that makes an operator keep (SdfFuse, SdfReset) or use (RaycastSdf) the brick summary, when tracking"""
        return {"summary": self.summary} if self.track else {}

    def _reset_model(self):
        """SdfReset(vol, NaN) (main.cpp:229) with the brick summary set to match -- the one-call frame: its reset() --, SdfReset(colorVol)
        (main.cpp:233); the model starts over, so what its predecessor left outside the box (the stores) is not part of it."""
        if self.kframe is not None:
            self.kframe.reset()
        else:
            self.ops.SdfReset(self.vol, float("nan"), **self._summary_kw())
        if self.color:
            self.ops.ColorReset(self.cvol)
        for store in (self.store, self.cstore):
            if store is not None:
                store.clear()

    def shift_volume(self, shift):
        """Shift the model by whole cells (ops.VolumeShift): the SDF volume with fill NaN -- through the one-call frame where it is in
        use -- the colour volume with fill 0.5, the summary rebuilt when tracking; vol.boxmin / boxmax (and cvol's) move.
        follow=dict(spill=): before the shift the live bricks of the boxes that leave go to the stores under their world keys, after it
        (self.origin is the new one) the bricks the stores hold of the boxes that entered go back into them.  A host store says how
        many: the shift runs tracked, and only a restore that put something back rebuilds the summary once more.  A device pool cannot
        say (launches only, nothing read back): the shift runs untracked and the summary is rebuilt once, after the restores,
        whatever they put back."""
        shift = tuple(int(s) for s in shift)
        if self.spill and any(s % bricks.BRICK for s in shift):
            raise ValueError("FramePipeline: with follow=dict(spill=True) a shift is whole bricks (multiples of 8), not %s" % (shift,))
        if self._shift_scratch is None:   # one scratch for both volumes: 16 packed planes of the SDF volume's cells
            self._shift_scratch = self.ops.shift_scratch(self.vol, shift)
        volumes = [(self.vol, self.store, float("nan"))] + ([(self.cvol, self.cstore, 0.5)] if self.color else [])
        key = lambda start: tuple((o + s) // bricks.BRICK for o, s in zip(self.origin, start))
        pool = self.spill == "device"
        if self.spill:
            for vol, store, fill in volumes:
                for start, size in bricks.leaving_boxes(self.dims, shift):
                    store.spill(vol.SubVolume(start, size), fill, key(start))
        untrack = pool and self.track and self.kframe is not None and self.kframe.track
        if untrack:
            self.kframe.set_track(False)   # (host state only: the frame's summary goes stale, and set_track(True) below rebuilds it)
        if self.kframe is not None:
            self.kframe.shift(shift, self._shift_scratch)
        else:
            kw = {} if pool else {"summary": self.summary if self.track else None}   # (a pool: the shift runs untracked)
            self.ops.VolumeShift(self.vol, shift, float("nan"), self._shift_scratch, **kw)
        if self.color:
            self.ops.VolumeShift(self.cvol, shift, 0.5, self._shift_scratch)
        self.origin = tuple(o + s for o, s in zip(self.origin, shift))
        if not self.spill:
            return
        restored = [store.restore(vol.SubVolume(start, size), key(start)) for vol, store, _ in volumes
                    for start, size in bricks.entering_boxes(self.dims, shift)]
        if pool:
            rebuild = self.track and self.kframe is None
        else:
            self._restored += sum(restored)
            rebuild = self.track and sum(restored) > 0
        if untrack:
            self.kframe.set_track(True)
        elif rebuild:   # the summary and the class tables describe the volume as it is after the restore
            self.summary.rebuild()

    @property
    def restored(self):
        """bricks put back so far; follow=dict(spill="device"): the pools' counters, read on demand (blocking)"""
        if self.spill == "device":
            return sum(store.restored for store in (self.store, self.cstore) if store is not None)
        return self._restored

    def world_bricks(self):
        """Everything the model holds as brick lists on one frame: (sdf, colour) with each bricks.world_bricks()'s tuple (lo, dims,
        boxmin, boxmax, ids, cells) -- the live volume's bricks and, with follow=dict(spill=True), the store's; colour None without
        color=True.  The two lists share the frame (each covers the other's store).  The stores are left as they are."""
        if not hasattr(self.ops, "BrickPack"):
            raise ValueError("FramePipeline: the world mesh needs an operator set with BrickPack")
        ckeys = self.cstore.keys() if self.cstore is not None else None
        sdf = bricks.world_bricks(self.store, self.vol, self.origin, float("nan"), ops=self.ops, cover=ckeys)
        if not self.color:
            return sdf, None
        skeys = self.store.keys() if self.store is not None else None
        return sdf, bricks.world_bricks(self.cstore, self.cvol, self.origin, 0.5, ops=self.ops, cover=skeys)

    def ExtractWorldMesh(self, with_index=False, indexed=False, min_faces=0, largest=False, simplify_cell=None, smooth=None):
        """The mesh of everything the model has seen -- the live volume and what it spilled -- as mesh.ExtractBrickMesh returns it:
        continuous across the faces of the volume that no longer exist.  Without a store: the brick mesh of the live volume.
        indexed=True: (verts, norms, colors, faces), welded by lattice edge on the device (mesh.ExtractBrickMesh's); min_faces / largest:
        without its small components (mesh.FilterMesh's); simplify_cell: then clustered on a grid of that cell anchored at the world origin
        (mesh.SimplifyMesh's) -- two world meshes taken at different times simplify to the same vertices where the surface has not changed;
        smooth: then smoothed, the normals recomputed from the faces (mesh.SmoothMesh's: None, an iteration count or a dict of its keywords)."""
        from . import mesh
        mesh._filter_args("ExtractWorldMesh", indexed, None, min_faces, largest)   # (before the bricks are packed)
        mesh._simplify_args("ExtractWorldMesh", indexed, None, simplify_cell)
        mesh._smooth_args("ExtractWorldMesh", indexed, None, smooth)
        (lo, dims, bmin, bmax, ids, cells), col = self.world_bricks()
        cids, ccells = (col[4], col[5]) if col is not None else (None, None)
        return mesh.ExtractBrickMesh(dims, bmin, bmax, self.kind, ids, cells, cids, ccells, with_index=with_index, indexed=indexed,
                                     min_faces=min_faces, largest=largest, simplify_cell=simplify_cell, smooth=smooth)

    def SaveWorldMesh(self, filename, binary=True, indexed=False, min_faces=0, largest=False, simplify_cell=None, smooth=None):
        """ExtractWorldMesh's mesh as filename + ".ply"; returns the triangle count.  indexed=True: V welded vertices and T faces;
        min_faces / largest / simplify_cell / smooth: ExtractWorldMesh's."""
        from . import mesh
        arrays = self.ExtractWorldMesh(indexed=indexed, min_faces=min_faces, largest=largest, simplify_cell=simplify_cell, smooth=smooth)
        return mesh._save_mesh(filename, arrays, binary, indexed)

    def world_view(self):
        """Everything the model holds, ready to be rendered (include/kfx_raycast_bricks.h): world_bricks() packed and planned once.
        Returns a WorldView that keeps the lists, the frame and the plan alive; RaycastWorld(..., view=) renders it from any number of
        poses.  It is the caller's snapshot: a later frame or shift changes the model, not the view."""
        import torch
        if not hasattr(self.ops, "RaycastSdfBricks"):
            raise ValueError("FramePipeline: the world view needs an operator set with RaycastSdfBricks")
        (lo, dims, bmin, bmax, ids, cells), col = self.world_bricks()
        dev = cells.device
        ids = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).to(dev)
        cids = ccells = None
        if col is not None:
            cids, ccells = torch.from_numpy(np.ascontiguousarray(col[4], np.uint32).view(np.int32)).to(dev), col[5]
        plan = self.ops.RaycastBricksPlan(dims, ids, cids)
        return WorldView(self.kind, lo, dims, bmin, bmax, ids, cells, cids, ccells, plan)

    def RaycastWorld(self, T_wc, K=None, w=None, h=None, color=False, view=None):
        """The model seen from T_wc -- the live volume and what it spilled, so also from a pose that looks back at where the camera
        has been: (depth, norm, img), new images of w x h pixels (default: the pipeline's) at the intrinsics K (default: the
        pipeline's), RaycastSdf's of the dense volume of the whole walk, bit for bit; color=True (a color=True pipeline): RaycastSdfColor's.
        view: a world_view() to render (None: one is taken for this call).  Without a store (no follow=dict(spill=True)) and without
        a view the live volume is the world, and it is rendered as it is."""
        if color and not self.color:
            raise ValueError("FramePipeline: RaycastWorld(color=True) needs a color=True pipeline")
        w, h = int(self.w if w is None else w), int(self.h if h is None else h)
        K = self.K if K is None else np.asarray(K, np.float32)
        I = self.ops.Image
        out = (I(w, h, "f32"), I(w, h, "f32x4"), I(w, h, "f32"))
        if view is None and self.store is None:
            if color:
                self.ops.RaycastSdfColor(*out, self.vol, self.cvol, T_wc, K, self.near, self.far, self.trunc, True)
            else:
                self.ops.RaycastSdf(*out, self.vol, T_wc, K, self.near, self.far, self.trunc, True)
            return out
        v = self.world_view() if view is None else view
        self.ops.RaycastSdfBricks(*out, v.dims, v.boxmin, v.boxmax, v.kind, v.ids, v.cells, T_wc, K, self.near, self.far, self.trunc, True,
                                  cids=v.cids, ccells=v.ccells, color=color, plan=v.plan)
        return out

    def _follow(self, T_wc):
        """follow=: the shift this pose asks for, applied before the frame's first launch"""
        f = self.follow
        T = np.asarray(T_wc, np.float64).reshape(-1, 4)[:3]
        if f["focus"] is None:
            centre = 0.5 * (np.asarray(self.vol.boxmin, np.float64) + np.asarray(self.vol.boxmax, np.float64))
            f["focus"] = float(np.linalg.norm(centre - T[:, 3]))
        shift = follow_shift(self.vol.boxmin, self.vol.boxmax, self.dims, T, f["focus"], f["quantum"], f["slack"])
        if any(shift):
            self.shift_volume(shift)
            self.shifts.append((self.frames_done, shift))

    def color_pose(self, T_cw):
        """T_iw = T_cd * T_cw (3x4 float32): world -> colour camera"""
        return (self.T_cd @ np.vstack([np.asarray(T_cw, np.float32).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32))[:3].astype(np.float32)

    def _fuse_color(self, maps_d, maps_n, T_cw):
        """SdfFuse(vol, colorVol, ...) of the given maps and the current RGB image (main.cpp:238 / :353)"""
        self.ops.SdfFuseColor(self.vol, self.cvol, maps_d, maps_n, T_cw, self.K, self._rgb_now, self.color_pose(T_cw), self.Kimg,
                              self.trunc, self.max_w, self.mincostheta, **self._summary_kw())

    def _integrate(self, maps_d, maps_n, T_cw):
        """SdfFuse of the given maps at T_cw (3x4 float32) into the model (main.cpp:345-356), keeping the summary when tracking"""
        if self.color:
            self._fuse_color(maps_d, maps_n, T_cw)
        else:
            self.ops.SdfFuse(self.vol, maps_d, maps_n, T_cw, self.K, self.trunc, self.max_w, self.mincostheta, **self._summary_kw())

    def _march(self, d, n, i, T_wc, K, **kw):
        """RaycastSdf of the model from T_wc into d / n / i; color=True: RaycastSdf(..., vol, colorVol, ...) (main.cpp:284), the colour into i"""
        if self.color:
            self.ops.RaycastSdfColor(d, n, i, self.vol, self.cvol, T_wc, K, self.near, self.far, self.trunc, True, **kw)
        else:
            self.ops.RaycastSdf(d, n, i, self.vol, T_wc, K, self.near, self.far, self.trunc, True, **kw)

    def submit(self, array):
        """sensor=: the next frame's raw image (h x w, the sensor's type) into the upload ring; its copy is enqueued at once."""
        self.input.submit(array)

    def _filter(self, filtered, raw_image):
        """BilateralFilter of the frame's image into `filtered`: the given image, else the oldest one in the upload ring (whose
        metres go to self.raw), else self.raw"""
        b = self.bil
        if raw_image is None and self.input is not None:
            self.input.filter(filtered, self.raw, b["gs"], b["gr"], b["size"], b["minval"])
        else:
            self.ops.BilateralFilter(filtered, self.raw if raw_image is None else raw_image, b["gs"], b["gr"], b["size"], b["minval"])

    def preprocess(self, raw_image=None):
        if self.kframe is not None:   # (with an upload ring attached, a step without an image consumes from it)
            self.kframe.step(_IDENTITY, None, raw_image, self.kframe.PREPROCESS)
            return
        self._filter(self.filtered, raw_image)
        vbo_normals(self.ops, self.vbo, self.normals, self.filtered, self.K)

    # -- the auto policy ------------------------------------------------------------
    def _policy_before(self):
        """Called at the start of a frame while a calibration is pending: puts the pipeline into the state of the frame's block."""
        c, B = self._cal, self.cal_block
        k = self.frames_done - c["first"]   # this frame's index within the blocks
        if k == 0 and self.kframe is not None:
            c["kfirst"] = self.kframe.count
            self.kframe.set_timing(self.timing | self.kframe.EVENTS_FUSE)   # the SdfFuse window and the frame period, for all blocks alike
        if k == B:
            self.set_track(False)
        elif k == 2 * B:
            self.set_track(True)
        if self.kframe is None:   # host clock (loops that synchronise every frame: the tracking loop's pose read-back)
            import time
            c["clock"] = time.perf_counter()

    def _policy_after(self):
        """Called at the end of a frame (frames_done counts it already): once the three blocks and one more frame -- whose start
        ends the last period -- have been issued, read their times and decide."""
        c, B = self._cal, self.cal_block
        k = self.frames_done - 1 - c["first"]
        if self.kframe is None and 0 <= k < 3 * B and c["clock"] is not None:
            import time
            c["t"].append((time.perf_counter() - c["clock"]) * 1e3)
        if k < 3 * B:
            return
        parts = None
        if self.kframe is not None:
            if self.kframe.count - c.get("kfirst", -1) != self.frames_done - c["first"]:
                # the caller issued parts of frames by themselves in between (preprocess / fuse / raycast): the ring's frames are
                # not the blocks' frames -- start over from here
                self._cal = {"first": self.frames_done, "t": [], "clock": None}
                self.set_track(True)
                return
            t = self.kframe.timings(c["kfirst"], 3 * B)   # waits for the last block's frames only; what is queued behind keeps the GPU busy
            self.kframe.set_timing(self.timing)
            period = t[:, 4].astype(np.float64)
            parts = t
        else:
            period = np.asarray(c["t"][:3 * B], np.float64)
        med = [float(np.median(period[i * B:(i + 1) * B])) for i in range(3)]
        keep = max(med[0], med[2]) <= (1.0 - self.cal_margin) * med[1]
        d = {"chosen": "table march (tracked SdfFuse)" if keep else "plain march",
             "frame_tracked_ms": [round(med[0], 5), round(med[2], 5)], "frame_plain_ms": round(med[1], 5),
             "frames_per_block": B, "first_frame": c["first"], "margin": self.cal_margin,
             "rule": "tables stay iff max(tracked block medians) <= (1 - margin) x plain block median (whole frames)",
             "clock": "device events, frame start to next frame start" if self.kframe is not None else "host clock around step()"}
        if parts is not None:   # what the frames were made of: SdfFuse, and the rest (preprocess, table build, RaycastSdf, gaps)
            fuse, rest = parts[:, 1].astype(np.float64), period - parts[:, 1]
            for name, v in (("sdf_fuse", fuse), ("rest_of_frame", rest)):
                d[name + "_tracked_ms"] = round(float(np.median(np.concatenate([v[:B], v[2 * B:]]))), 5)
                d[name + "_plain_ms"] = round(float(np.median(v[B:2 * B])), 5)
        self.track_decision = d
        self._cal = None
        if not keep:
            self.set_track(False)

    def fuse(self, T_wc):
        if self.kframe is not None:
            self.kframe.step(T_wc, scenes.se3_inverse(T_wc), None, self.kframe.FUSE)
            return
        self._integrate(self.filtered, self.normals, scenes.se3_inverse(T_wc))

    def raycast(self, T_wc):
        if self.kframe is not None:
            self.kframe.step(T_wc, None, None, self.kframe.RAYCAST)
            return
        self._march(self.ray_d, self.ray_n, self.ray_i, T_wc, self.K, **self._summary_kw())

    def step(self, T_wc, raw_image=None, rgb_image=None):
        """One frame: preprocess the new depth image, integrate it, render the model.  rgb_image (color=True): the frame's RGB
        image ("u8x3", the colour camera's size; default self.rgb)."""
        if self.color:
            self._rgb_now = self.rgb if rgb_image is None else rgb_image
        if self.follow is not None:
            self._follow(T_wc)
        cal = self._cal is not None and self.frames_done >= self._cal["first"]
        if cal:
            self._policy_before()
        if self.kframe is not None:
            self.kframe.step(T_wc, scenes.se3_inverse(T_wc), raw_image)
        else:
            self.preprocess(raw_image)
            self.fuse(T_wc)
            self.raycast(T_wc)
        self.frames_done += 1
        if cal:
            self._policy_after()


_IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)

# TrackingPipeline.step(next_image=FROM_SENSOR): the next frame's image is the next one in the upload ring (sensor=)
FROM_SENSOR = "the next image of the upload ring"


class _TrackingLoop:
    """The reference application's loop with pose estimation switched on (main.cpp:200-356), written once for TrackingPipeline and
    TrackingSlabPipeline (a mixin in front of FramePipeline / SlabPipeline): depth pyramid, per-level vertex / normal maps, raycast
    of the model at the last pose on every level that has ICP iterations, coarse-to-fine projective point-plane ICP, then SdfFuse at
    the refined pose when tracking is good.  It owns the tracker's state and step(); a class supplies what really differs:
    _render_levels (how the model is rendered into pyr_*), _refine (where the refinement comes from; default: the host loop of
    kangaroo_amd/tracking.py around the HIP operator) and _fuse_at (how a pose is integrated)."""

    LEVELS = 4

    def _init_tracker(self, its, icp_c, max_rmse, pose_step):
        """pose_step: update the pose with ops.PoseStep (one host call that also returns the inverse SdfFuse needs) and hand that
        inverse to _fuse_at"""
        from . import tracking
        ops, w, h, L = self.ops, self.w, self.h, self.LEVELS
        self.tracking = tracking
        self.its = tuple(tracking.DEFAULT_ITS if its is None else its)
        self.icp_c, self.max_rmse, self._pose_step = float(icp_c), float(max_rmse), bool(pose_step)
        P = ops.Pyramid
        self.kin_d, self.kin_v, self.kin_n = P(w, h, L, "f32"), P(w, h, L, "f32x4"), P(w, h, L, "f32x4")
        # a second set for the NEXT frame's pre-amble (step(..., next_image=...)): enqueued while the pose of this frame is on
        # its way to the host, it must not overwrite the maps SdfFuse is about to read
        self._kin_back = None
        self._prefetched = None   # the image whose pre-amble the back set holds
        self.pyr_d, self.pyr_i = P(w, h, L, "f32"), P(w, h, L, "f32")
        self.pyr_n, self.pyr_v = P(w, h, L, "f32x4"), P(w, h, L, "f32x4")
        self.K_levels = [scenes.intrinsics_level(self.K, l) for l in range(L)]
        # main.cpp:110-111: debug image and a scratch image of w * sizeof(LeastSquaresSystem<float,12>) x h bytes
        self.debug = ops.Image(w, h, "f32x4")
        self.scratch = ops.Image(w * 232, h, "u8")
        self.T_wl = np.eye(4)
        self.frame = 0
        self.rmse, self.tracking_good = 0.0, True
        self.resets = 0   # recoveries after tracking was lost altogether (main.cpp:223-242)

    def preprocess(self, raw_image=None, into=None):
        o = self.ops
        kin_d, kin_v, kin_n = (self.kin_d, self.kin_v, self.kin_n) if into is None else into
        self._filter(kin_d[0], None if raw_image is FROM_SENSOR else raw_image)
        if hasattr(o, "DepthPyramidVboNormals"):   # the pyramid and its maps from one launch (same images)
            o.DepthPyramidVboNormals(kin_d, kin_v, kin_n, self.K_levels)
            return
        o.BoxReduceIgnoreInvalid(kin_d)
        for l in range(self.LEVELS):
            vbo_normals(o, kin_v[l], kin_n[l], kin_d[l], self.K_levels[l])

    def _prefetch(self, image):
        """The pre-amble of `image` into the back set of maps (called between enqueueing the refinement and waiting for its pose)."""
        if self._kin_back is None:
            P, L = self.ops.Pyramid, self.LEVELS
            self._kin_back = (P(self.w, self.h, L, "f32"), P(self.w, self.h, L, "f32x4"), P(self.w, self.h, L, "f32x4"))
        self.preprocess(image, into=self._kin_back)
        self._prefetched = image

    def _refine(self, next_image):
        """(T_lp, rmse, tracking_good) of the frame's maps against the rendered model: main.cpp:301-336 on the host, one
        PoseRefinementProjectiveIcpPointPlane call + solve per iteration"""
        return self.tracking.refine_pose(self.ops, self.kin_v, self.pyr_v, self.pyr_n, self.K_levels, self.scratch, self.debug, self.its,
                                         self.icp_c, self.max_rmse)

    def step(self, T_wl_init=None, raw_image=None, next_image=None, rgb_image=None):
        """One frame.  The first frame is fused at T_wl_init (identity if None); later frames are tracked
        against the model.  Returns the current T_wl (4x4 float64).
        next_image: the depth image the NEXT step will be given (already in device memory; sensor=: FROM_SENSOR, the image
        submitted after this frame's, and the next step is given no image).  With the device-resident
        refinement its pre-amble -- which does not depend on any pose -- is enqueued behind the refinement, before this thread
        waits for the pose: the device works on it while the thread wakes up instead of idling until SdfFuse arrives.  The
        next step finds its maps ready when it is given the same image object; same images, same poses.
        rgb_image (color=True): the frame's RGB image (default self.rgb).
        TrackingSlabPipeline: next_image and rgb_image are accepted and ignored (no prefetch hook, no colour); follow=, track=, color=
        and sensor= are refused there, so those branches never run.)"""
        if self.color:
            self._rgb_now = self.rgb if rgb_image is None else rgb_image
        if self.follow is not None and self.frame > 0:   # the previous frame's pose: this frame's is not known yet
            self._follow(self.T_wl)
        cal = self._cal is not None and self.frames_done >= self._cal["first"]
        if cal:   # track="auto": whole frames of the three blocks, host clock around the step (the pose read-back synchronises)
            self._policy_before()
        if raw_image is None and self.input is not None:
            raw_image = FROM_SENSOR
        if raw_image is not None and self._prefetched is raw_image:
            (self.kin_d, self.kin_v, self.kin_n), self._kin_back = self._kin_back, (self.kin_d, self.kin_v, self.kin_n)
        else:
            self.preprocess(raw_image)
        self._prefetched = None
        # main.cpp:223-242, `if (Pushed(reset) || !std::isfinite(f_rmse))`: when the last refinement found no correspondence at all
        # (rmse = sqrt(0 / 0): a frame without depth, a model out of view) the application starts over -- T_wl = identity (the world
        # frame restarts at the current camera; T_wl_init if the caller gives one), the volume back to "never observed", the current
        # frame fused -- and the frame then goes on like any other: it is tracked against the model it has just founded.
        # (On slabs every rank sees the same rmse.)
        recover = self.frame > 0 and not np.isfinite(self.rmse)
        if recover:
            self.T_wl = np.eye(4)
            self._reset_model()
            self.rmse, self.tracking_good = 0.0, True
            self.resets += 1
        if self.frame == 0 or recover:
            if T_wl_init is not None:
                self.T_wl = np.vstack([np.asarray(T_wl_init, np.float64).reshape(3, 4), [0, 0, 0, 1]])
            self._fuse_at(self.T_wl)
        if self.frame > 0:
            self._render_levels([l for l in range(self.LEVELS) if self.its[l] > 0], self.T_wl[:3].astype(np.float32))
            T_lp, self.rmse, self.tracking_good = self._refine(next_image)
            if self.tracking_good and self._pose_step:
                # the device idles from the pose's arrival to the SdfFuse launch: the update in one host call (kfx_pose_step; the
                # same arithmetic as the lines below: the same poses, bit for bit)
                self.T_wl, T_cw = self.ops.PoseStep(self.T_wl, T_lp)
                self._fuse_at(self.T_wl, T_cw)
            elif self.tracking_good:
                self.T_wl = self.T_wl @ self.tracking.se3_inv(T_lp)
                self._fuse_at(self.T_wl)
        self.frame += 1
        self.frames_done += 1
        if cal:
            self._policy_after()
        return self.T_wl


class TrackingPipeline(_TrackingLoop, FramePipeline):
    """The tracking loop (_TrackingLoop) on one volume."""

    USE_FRAME = False   # its frame has the pose estimation between rendering and integration: the operators are issued here

    def __init__(self, ops, dims, boxmin, boxmax, w, h, its=None, icp_c=0.1, max_rmse=0.10, device_icp=False, one_raycast=None, **kw):
        """device_icp: run the whole refinement loop on the GPU (ops.IcpRefine, one synchronisation per frame) instead
        of one PoseRefinementProjectiveIcpPointPlane call + host solve per iteration.  one_raycast: render all pyramid
        levels with one launch (ops.RaycastSdfLevels; default: when the operator set has it).  color=True (see FramePipeline):
        SdfFuseColor at the tracked pose and colour renderings of every level (ops.RaycastSdfColorLevels, or the per-level calls)."""
        super().__init__(ops, dims, boxmin, boxmax, w, h, **kw)
        self.device_icp = bool(device_icp) and hasattr(ops, "IcpRefine")
        self.one_raycast = hasattr(ops, "RaycastSdfLevels") if one_raycast is None else (bool(one_raycast) and hasattr(ops, "RaycastSdfLevels"))
        self._bound = {}          # SdfFuseBound per set of maps
        # (PoseStep's inverse goes to the SdfFuse call whose other arguments are bound beforehand; the colour fuse has no such call)
        self._init_tracker(its, icp_c, max_rmse, pose_step=hasattr(ops, "PoseStep") and hasattr(ops, "SdfFuseBound") and not self.color)

    def _render_levels(self, lv, T34):
        """RaycastSdf + DepthToVbo of the levels lv (main.cpp:280-288; color=True: main.cpp:284, the colour image into pyr_i): one launch
        -- same images, overlapping marches -- or the per-level calls"""
        o, kw = self.ops, self._summary_kw()
        if not self.one_raycast:
            for l in lv:
                self._march(self.pyr_d[l], self.pyr_n[l], self.pyr_i[l], T34, self.K_levels[l], **kw)
                o.DepthToVbo(self.pyr_v[l], self.pyr_d[l], self.K_levels[l])
            return
        outs, Ks = [(self.pyr_d[l], self.pyr_n[l], self.pyr_i[l], self.pyr_v[l]) for l in lv], [self.K_levels[l] for l in lv]
        if self.color:
            o.RaycastSdfColorLevels(outs, self.vol, self.cvol, T34, Ks, self.near, self.far, self.trunc, True, **kw)
        else:
            o.RaycastSdfLevels(outs, self.vol, T34, Ks, self.near, self.far, self.trunc, True, **kw)

    def _refine(self, next_image):
        if not self.device_icp:
            return super()._refine(next_image)
        hook = (lambda: self._prefetch(next_image)) if next_image is not None else None
        T_lp, rmse, _, good = self.ops.IcpRefine(self.kin_v, self.pyr_v, self.pyr_n, self.K_levels, self.its, self.icp_c, self.max_rmse,
                                                 self.scratch, self.debug, before_wait=hook)
        return T_lp, rmse, good

    def shift_volume(self, shift):
        super().shift_volume(shift)
        self._bound = {}   # (the bound SdfFuse calls marshalled the volume with its old box)

    def _fuse_bound(self, T_cw):
        """SdfFuse of the frame's maps at T_cw (3x4 float32) through a call whose other arguments were marshalled once (per set of
        maps and per tracked / plain choice)."""
        key = (id(self.kin_d[0]), bool(self.track), id(self.summary) if self.track else 0)
        b = self._bound.get(key)
        if b is None:
            b = self._bound[key] = self.ops.SdfFuseBound(self.vol, self.kin_d[0], self.kin_n[0], self.K, self.trunc, self.max_w, self.mincostheta,
                                                         summary=self.summary if self.track else None)
        b(T_cw)

    def _fuse_at(self, T_wl, T_cw=None):
        """T_cw: PoseStep's inverse of T_wl (the bound call); None: inverted here in float64 (main.cpp:345-356)"""
        if T_cw is not None:
            self._fuse_bound(T_cw)
        else:
            self._integrate(self.kin_d[0], self.kin_n[0], self.tracking.se3_inv(T_wl)[:3].astype(np.float32))


def slab_range(d, rank, world):
    """Z-planes [z0, z1) owned by `rank`: contiguous, sizes differ by at most one plane."""
    base, rem = divmod(d, world)
    z0 = rank * base + min(rank, rem)
    return z0, z0 + base + (1 if rank < rem else 0)


class SlabPipeline(FramePipeline):
    """Z-slab partition across ranks.  Rank r stores planes
    [z0 - G, z1 + G) clipped to the volume (G ghost planes each side) as an ordinary
    BoundedVolume whose bbox is VoxelPositionInUnits of its first / last stored plane -- the
    view BoundedVolume::SubBoundingVolume produces (BoundedVolume.h:156-164)."""

    GHOST = 2  # >= 1 for the trilinear z+1 corner and the gradient's z-1 / z+1 cells (Volume.h:240-289)
    USE_FRAME = False   # slabs: the operators take slab arguments and collectives sit between them

    def __init__(self, ops, dist, dims, boxmin, boxmax, w, h, halo="exchange", raycast="exact", kind="f32", overlap=False,
                 inputs="replicate", images="all", merge="direct", driver="python", comm=None, tiles=0, unchecked=False, pipeline=3, ghost=None, **kw):
        """driver = "c": every frame is ONE library call per rank (kfx_slab_frame_step, include/kfx_slab.h: the launches AND the
        collectives are enqueued by the library through `comm`, a kangaroo_amd.slab.Comm -- RCCL for one process per GPU; default:
        Comm.torch(dist), the collectives of the process group the caller has set up); driver = "python": this class issues the
        operators and torch.distributed collectives one by one (the cross-check, and what the CPU tests run on the oracle-backed
        operator set).  Same bits either way.  tiles: row-tiles of the exact hand-over (C driver; 0 = the library's default);
        unchecked: do not fail when the exact march leaves rays open (loop-back measurements of ONE rank: scripts/slab_host_floor.py).
        ghost: ghost planes per side; None = 2, or -- driver "c", exact raycast, recomputed ghost planes -- kfx_slab_exact_ghost's width
        (as far as a hit can fall back behind the sample that found it + the gradient stencil: every rank finalises the hits it
        finds and the hand-over drops its last stage, include/kfx_slab.h), where every rank owns that many planes.

        halo = "exchange": every rank integrates only the planes it owns and the ghost planes are
        refreshed from the two neighbours after each SdfFuse (point-to-point send/recv: one xGMI link
        per direction); halo = "recompute": every rank integrates its ghost planes itself (the update is
        deterministic per voxel, so no traffic is needed) -- the cross-check of the exchange path."""
        assert halo in ("exchange", "recompute")
        assert raycast in ("composite", "exact", "exact_allreduce")
        if (kw.get("follow") or {}).get("spill") == "device":
            raise ValueError("SlabPipeline: follow=dict(spill='device') (a brick pool) is a single-volume option: a pool per rank is a later step")
        if kw.get("follow") is not None:
            raise ValueError("SlabPipeline: follow= (a volume that follows the camera) is a single-volume option: a shift along z moves "
                             "planes from one rank's slab to another's, and shifts on Z-slabs are not implemented")
        if kw.get("sensor") is not None:
            raise ValueError("SlabPipeline: sensor= (the upload ring of raw sensor images) is a single-GPU option; give the slab pipelines "
                             "depth images in metres")
        # inputs (SURVEY.md 8(e) "input distribution"): "replicate" = every rank filters the frame and derives the normal map
        # itself (no traffic); "broadcast" = rank 0 does, and its filtered depth + normal map (20 B per pixel) are broadcast
        assert inputs in ("replicate", "broadcast")
        self.inputs = inputs
        # images (composite mode): "all" = every rank ends up with the merged images (the second collective is an all-reduce);
        # "root" = only rank 0 does (a reduce: half the traffic of the payload's all-reduce) -- a known-pose stream has one
        # consumer of the rendering, and the tracking loop can solve on rank 0 and broadcast the 4 x 4 pose (TrackingSlabPipeline)
        assert images in ("all", "root")
        if images == "root" and raycast != "composite":
            raise ValueError("SlabPipeline: images='root' is an option of the composite raycast")
        self.images = images
        # merge (composite mode): how the per-slab images become one.  "direct" = every rank owns one strip of the image: one
        # all-to-all sends each strip to its owner, the owner keeps the nearest hit per pixel, one all-gather (images = "root": a
        # gather) returns the merged strips -- each byte crosses one link once per phase, all links of the xGMI mesh at once;
        # "allreduce" = a MIN all-reduce of (depth, rank) keys + a SUM all-reduce of the winners' payload (whole images through
        # whatever ring / tree the library builds).  Same winner per pixel, same images.
        assert merge in ("direct", "allreduce")
        self.merge = merge
        # overlap (composite mode, known-pose streams): the merge of frame k's per-slab images -- two latency-bound
        # all-reduces and three small kernels -- runs on a second stream while the main stream already preprocesses and
        # integrates frame k + 1; step() then returns before ray_d / ray_n / ray_i are merged: they are valid only after
        # wait_composite() (bench.py's sync_all calls it; the next raycast_into waits for it by itself).
        self.overlap = bool(overlap)
        # The overlapped merge issues its all-reduces from a side stream while the main stream may issue the ghost-plane
        # send / recv of the next SdfFuse: two NCCL call sequences whose relative order can differ between ranks (and torch may
        # route point-to-point through a communicator of its own) -- the classic collective-ordering deadlock.  Not allowed.
        if self.overlap and raycast == "composite" and (halo == "exchange" or inputs == "broadcast"):
            raise ValueError("SlabPipeline: overlap=True needs halo='recompute' and inputs='replicate' (an overlapped merge next to the "
                             "ghost-plane exchange or the input broadcast would interleave collectives in rank-dependent order)")
        # overlap with raycast = "exact" (driver "c"): frames pipelined across the ranks -- frame k's final exchange of the finalised
        # pixels runs on the frame object's side stream through a second communicator while the main stream carries frame k + 1
        # (include/kfx_slab.h); `pipeline` image sets are in flight, step() returns before the rendering exists, and
        # wait_composite() makes ray_d / ray_n / ray_i the last frame's images.  Same bits as without overlap.
        if self.overlap and raycast != "composite" and (driver != "c" or raycast != "exact"):
            raise ValueError("SlabPipeline: overlap=True with the exact raycast (pipelined frames) is a feature of driver='c'")
        self.pipeline = max(2, min(int(pipeline), 4))
        if kw.get("track"):
            raise ValueError("SlabPipeline: track=True (brick summary) is a single-volume feature; slabs march without it")
        self._side = self._merged = None
        self.halo = halo
        self.raycast_mode = raycast
        self.kind = kind            # "f32": SDF_t cells; "f16": SDF_h cells (config C5: 2048^3 over 8 GPUs = 4 GiB per rank)
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.full_boxmin = np.asarray(boxmin, np.float32)
        self.full_boxmax = np.asarray(boxmax, np.float32)
        d = int(dims[2])
        if ghost is None:
            ghost = self.GHOST
            if driver == "c" and raycast == "exact" and halo == "recompute" and self.world > 1 and kind == "f32":
                from . import slab as S
                Kk = kw.get("K")
                Kk = scenes.intrinsics(w, h) if Kk is None else Kk
                wide = S.exact_ghost(dims, boxmin, boxmax, scenes.trunc_dist(boxmin, boxmax, dims, kw.get("trunc_factor", scenes.TRUNC_DIST_FACTOR)), Kk, w, h)
                if d // self.world >= wide:
                    ghost = wide
        self.GHOST = int(ghost)   # (shadows the class default for this pipeline)
        # exchange_halos takes the ghost planes from the immediate neighbours: every rank must own at least GHOST planes
        assert self.world == 1 or d // self.world >= self.GHOST, "slabs thinner than the ghost width (%d planes / %d ranks)" % (d, self.world)
        self.z0, self.z1 = slab_range(d, self.rank, self.world)
        self.s0, self.s1 = max(self.z0 - self.GHOST, 0), min(self.z1 + self.GHOST, d)
        kw["contiguous_images"] = True  # collectives operate on dense tensors
        assert driver in ("python", "c")
        self.driver, self.sframe, self.comm = driver, None, comm
        timing_slots = kw.pop("timing_slots", None)
        # color=True (FramePipeline): the colour volume is partitioned like the SDF volume -- `cvol` holds this rank's planes with the
        # local box -- and every path stays bit-identical to the single-volume colour pipeline (include/kfx_slab_color.h)
        if kw.get("color"):
            if kind != "f32":
                raise ValueError("SlabPipeline: color=True needs fp32 cells (kind='f16': the colour operators have no half-cell form)")
            if raycast == "exact_allreduce":
                raise ValueError("SlabPipeline: color=True renders with raycast='exact' or 'composite' ('exact_allreduce' is the grey hand-over's "
                                 "cross-check: its state merge does not carry the colour plane's rank)")
        super().__init__(ops, dims, boxmin, boxmax, w, h, **kw)
        if driver == "c":
            if raycast == "exact_allreduce" or images != "all" or kind != "f32":
                raise ValueError("SlabPipeline(driver='c'): raycast 'exact' or 'composite', images='all', fp32 cells")
            from . import slab as S
            if self.comm is None:
                self.comm = S.Comm.torch(dist)
            lay = S.layout(d, float(self.full_boxmin[2]), float(self.full_boxmax[2]), self.rank, self.world, self.GHOST)
            assert (lay.z0, lay.z1, lay.s0, lay.s1) == (self.z0, self.z1, self.s0, self.s1)
            # the image sets 1 .. of the pipelined exact raycast (set 0: ray_d / ray_n / ray_i), there from the start so that
            # configure(overlap=True) can switch to pipelined frames on the same object (bench.py times the variants on one pipeline)
            I = ops.Image
            extra = [(I(w, h, "f32", pitch=w * 4), I(w, h, "f32x4", pitch=w * 16), I(w, h, "f32", pitch=w * 4)) for _ in range(self.pipeline - 1)] if self.world > 1 else []
            self.sframe = S.SlabFrame(self.comm, self.vol, lay, self.raw, self.filtered, self.vbo, self.normals, self.ray_d, self.ray_n, self.ray_i, self.K,
                                      self.bil, self.near, self.far, self.trunc, self.max_w, self.mincostheta, halo=halo, raycast=raycast, merge=merge,
                                      inputs=inputs, overlap=overlap, tiles=tiles, unchecked=unchecked, timing_slots=int(timing_slots or 256),
                                      pipe_images=extra)
            if self.color:
                self.sframe.set_color(self.cvol, self.rgb, self.Kimg, self.T_cd)

    def configure(self, **kw):
        """Change policies between frames (halo, raycast, merge, inputs, overlap, tiles): bench.py times the variants on one pipeline."""
        names = {"halo": "halo", "raycast": "raycast_mode", "merge": "merge", "inputs": "inputs", "overlap": "overlap"}
        self.wait_composite()
        if self.sframe is not None:
            self.sframe.configure(**kw)
            self.ray_d, self.ray_n, self.ray_i = self.sframe.image_sets[0]   # (pipelined frames re-point these at the last frame's set)
        for k, v in kw.items():
            if k in names:
                setattr(self, names[k], v)

    def step(self, T_wc, raw_image=None, rgb_image=None):
        """rgb_image (color=True): the frame's RGB image; the C driver reads the image it was bound to (self.rgb) unless another one
        is given, which it is then bound to from this frame on."""
        if self.sframe is not None:
            if self.color and rgb_image is not None and rgb_image is not self._rgb_now:
                self._rgb_now = rgb_image
                self.sframe.set_color(self.cvol, rgb_image, self.Kimg, self.T_cd)
            self.sframe.step(T_wc, scenes.se3_inverse(T_wc), raw_image)
            self.frames_done += 1
            return
        super().step(T_wc, raw_image, rgb_image)

    def _alloc_volume(self, boxmin, boxmax):
        W, H, D = self.dims
        f = np.float32
        size_z = f(boxmax[2]) - f(boxmin[2])
        # plane positions exactly as VoxelPositionInUnits computes them (BoundedVolume.h:115-125)
        zlo = f(boxmin[2]) + size_z * f(self.s0) / f(D - 1)
        zhi = f(boxmin[2]) + size_z * f(self.s1 - 1) / f(D - 1)
        lo = np.array([boxmin[0], boxmin[1], zlo], f)
        hi = np.array([boxmax[0], boxmax[1], zhi], f)
        if self.kind != "f32":
            return self.ops.BoundedVolume(W, H, self.s1 - self.s0, lo, hi, kind=self.kind)
        return self.ops.BoundedVolume(W, H, self.s1 - self.s0, lo, hi)

    def _alloc_color_volume(self, boxmin, boxmax):
        """This rank's planes [s0, s1) of the colour volume, with the SDF slab's box."""
        return self.ops.BoundedVolume(self.vol.w, self.vol.h, self.vol.d, self.vol.boxmin, self.vol.boxmax, kind="c32")

    def preprocess(self, raw_image=None):
        if self.sframe is not None:
            self.sframe.step(_IDENTITY, None, raw_image, 1)   # KFX_FRAME_PREPROCESS (the broadcast included)
            return
        if self.inputs == "broadcast" and self.world > 1:
            if self.rank == 0:
                super().preprocess(raw_image)
            self.dist.broadcast(self.filtered.tensor(), src=0)
            self.dist.broadcast(self.normals.tensor(), src=0)
        else:
            super().preprocess(raw_image)

    def fuse(self, T_wc, T_cw=None):
        """T_cw: world -> camera transform to use instead of the float32 inverse of T_wc (the tracking loop inverts
        its pose in float64, main.cpp:345-356)."""
        if self.sframe is not None:
            self.sframe.step(T_wc, scenes.se3_inverse(T_wc) if T_cw is None else T_cw, None, 2)   # KFX_FRAME_FUSE (+ ghost planes)
            return
        # a slab's plane count is usually not a multiple of 8: full_extent="slab" integrates exactly the voxels roo::SdfFuse
        # integrates on the whole volume (x / y extents (dim/8)*8, planes below (D/8)*8), whatever the partition
        D = self.dims[2]
        zmin, zmax = float(self.full_boxmin[2]), float(self.full_boxmax[2])
        ctarget = self.cvol if self.color else None
        if self.halo == "recompute" or self.world == 1:
            target, first = self.vol, self.s0
        else:
            target, first = self.vol.ZSlab(self.z0 - self.s0, self.z1 - self.s0), self.z0  # owned planes only
            if self.color:
                ctarget = self.cvol.ZSlab(self.z0 - self.s0, self.z1 - self.s0)
                ctarget.boxmin, ctarget.boxmax = target.boxmin, target.boxmax   # (the SDF view's box, bit for bit)
        # slab entry point: voxel positions by the FULL volume's expression, so every plane is integrated
        # bit-identically to the same plane of a single-GPU volume
        T_cw = scenes.se3_inverse(T_wc) if T_cw is None else T_cw
        if self.color:
            self.ops.SdfFuseColorSlab(target, ctarget, (D, first, zmin, zmax), self.filtered, self.normals, T_cw, self.K, self._rgb_now,
                                      self.color_pose(T_cw), self.Kimg, self.trunc, self.max_w, self.mincostheta, full_extent="slab")
        else:
            self.ops.SdfFuse(target, self.filtered, self.normals, T_cw, self.K, self.trunc,
                             self.max_w, self.mincostheta, full_extent="slab", slab=(D, first, zmin, zmax))
        if target is not self.vol:
            self.exchange_halos()

    def _p2p(self, ops):
        """One batched group of point-to-point operations, complete on return as far as the current stream is concerned.
        RCCL (backend "nccl") is stream-ordered: the requests' wait() chains the current stream behind the transfers.  gloo
        with device tensors -- ranks sharing one GPU in the tests -- goes through host copies made here, with the device
        synchronised on both sides of the batch."""
        if not ops:
            return
        dist = self.dist
        if ops[0].tensor.is_cuda and dist.get_backend() != "nccl":
            # gloo's own path for device tensors takes ~0.1 s per message: stage through host copies here (test transport only)
            import torch
            torch.cuda.synchronize()
            host = [(op, op.tensor.cpu() if op.op is dist.isend else torch.empty(op.tensor.shape, dtype=op.tensor.dtype)) for op in ops]
            for req in dist.batch_isend_irecv([dist.P2POp(op.op, t, op.peer) for op, t in host]):
                req.wait()
            for op, t in host:
                if op.op is not dist.isend:
                    op.tensor.copy_(t)
            torch.cuda.synchronize()
            return
        for req in dist.batch_isend_irecv(ops):
            req.wait()

    def exchange_halos(self):
        """Refresh the ghost planes from the neighbours' owned planes (contiguous img_pitch-sized
        slices): rank r sends its first / last G owned planes down / up and receives the matching
        planes of its neighbours.  One batched group of point-to-point operations."""
        dist = self.dist
        ops = []
        lo_ghost = self.z0 - self.s0              # planes [s0, z0) come from rank-1
        hi_ghost = self.s1 - self.z1              # planes [z1, s1) come from rank+1
        own0, own1 = self.z0 - self.s0, self.z1 - self.s0   # local indices of the owned range
        for vol in (self.vol, self.cvol) if self.color else (self.vol,):   # (the colour planes in the same batch, behind the SDF planes on every rank)
            if self.rank > 0 and lo_ghost > 0:
                ops.append(dist.P2POp(dist.isend, vol.planes(own0, own0 + lo_ghost), self.rank - 1))
                ops.append(dist.P2POp(dist.irecv, vol.planes(0, lo_ghost), self.rank - 1))
            if self.rank < self.world - 1 and hi_ghost > 0:
                ops.append(dist.P2POp(dist.isend, vol.planes(own1 - hi_ghost, own1), self.rank + 1))
                ops.append(dist.P2POp(dist.irecv, vol.planes(own1, own1 + hi_ghost), self.rank + 1))
        self._p2p(ops)

    def world_bricks(self):
        raise ValueError("SlabPipeline: the world mesh belongs to a volume that follows the camera (follow=), a single-volume option; "
                         "a rank's part of the model's mesh is ExtractMesh")

    def RaycastWorld(self, *args, **kw):
        raise ValueError("SlabPipeline: the world view belongs to a volume that follows the camera (follow=), a single-volume option; "
                         "the model's rendering is the frame's composite")

    def ExtractMesh(self, indexed=False, min_faces=0, largest=False, simplify_cell=None, smooth=None):
        """This rank's part of the model's mesh (include/kfx_mesh.h): the cubes whose lower plane it owns, [z0, min(z1, D - 1)),
        every triangle bit-identical to the single-volume mesh's, in emission order; (verts, norms) device tensors, or -- color=True --
        (verts, norms, colors) with the single-volume mesh's colours.
        With halo = "exchange" the ghost planes the normals read are refreshed first (a collective step: every rank calls).
        indexed=True: (verts, norms[, colors], faces) -- the weld of this rank's part by lattice edge (include/kfx_mesh_index.h): V
        vertices, faces (T, 3); a vertex on a slab boundary exists once per rank that uses it.
        min_faces / largest: refused (ValueError) -- a rank's mesh is welded within the rank, its components are cut at the slab boundaries."""
        from . import mesh
        if min_faces or largest:
            raise ValueError("SlabPipeline.ExtractMesh: a rank's mesh is welded within its rank, so its components are cut at the slab "
                             "boundaries; min_faces / largest need the whole volume's mesh")
        if simplify_cell:   # (refused as the filter is: a cluster that straddles a slab boundary would be two)
            raise ValueError("SlabPipeline.ExtractMesh: a rank's mesh is welded within its rank; simplify_cell needs the whole volume's mesh")
        if smooth is not None:   # (refused as the filter is: a vertex on a slab boundary would be smoothed as a boundary vertex, once per rank)
            raise ValueError("SlabPipeline.ExtractMesh: a rank's mesh is welded within its rank, so its components are cut at the slab "
                             "boundaries; smooth needs the whole volume's mesh")
        if self.sframe is not None:
            self.wait_composite()
        elif self.halo == "exchange" and self.world > 1:
            self.exchange_halos()     # (the C driver's fuse step leaves them current itself)
        D = self.dims[2]
        slab = (D, self.s0, float(self.full_boxmin[2]), float(self.full_boxmax[2]), self.z0, self.z1)
        verts, norms, colors, *faces = mesh.ExtractMesh(self.vol, self.cvol if self.color else None, slab=slab, indexed=indexed)
        return ((verts, norms, colors) if self.color else (verts, norms)) + tuple(faces)

    def SaveMesh(self, prefix, binary=True, indexed=False, min_faces=0, largest=False, simplify_cell=None, smooth=None):
        """Writes this rank's part as prefix.r<rank>.ply (with colours when color=True); returns its triangle count.
        indexed=True: welded vertices and a face list (ExtractMesh's).  min_faces / largest: refused, as ExtractMesh's."""
        from . import mesh
        verts, norms, *rest = self.ExtractMesh(indexed=indexed, min_faces=min_faces, largest=largest, simplify_cell=simplify_cell, smooth=smooth)
        faces = rest.pop().cpu().numpy().view("uint32") if indexed else None
        mesh.write_ply("%s.r%d.ply" % (prefix, self.rank), verts.cpu().numpy(), norms.cpu().numpy(),
                       rest[0].cpu().numpy() if rest and rest[0] is not None else None, binary, faces)
        return len(verts) // 3 if faces is None else len(faces)

    def raycast(self, T_wc):
        """raycast = "composite": every rank marches its own slab from the slab's entry point and the nearest
        hit wins (one MIN + one SUM all-reduce; rays re-enter each slab with a fresh step, so depths can differ
        from the single-volume march in the last bits).  raycast = "exact": the march state travels with the
        ray from slab to slab (raycast_exact), bit-identical to RaycastSdf on the whole volume."""
        if self.sframe is not None:
            self.sframe.step(T_wc, None, None, 4)   # KFX_FRAME_RAYCAST (+ the hand-over / the merge)
            return
        self.raycast_into(self.ray_d, self.ray_n, self.ray_i, self.K, T_wc)

    def raycast_into(self, d, n, i, K, T_wc):
        """The model rendered from T_wc with intrinsics K into the images d / n / i (any size: pyramid levels),
        identical on every rank afterwards."""
        if self.raycast_mode == "exact":
            self.raycast_exact(T_wc, d, n, i, K)
            return
        if self.raycast_mode == "exact_allreduce":
            self.raycast_exact_allreduce(T_wc, d, n, i, K)
            return
        self.wait_composite()   # the previous frame's merge still reads these images
        self._march(d, n, i, T_wc, K)   # (color=True: each rank renders its local view in colour; the merge carries img as it carries the shade)
        if self.world > 1:
            if self.overlap and (self.halo == "exchange" or self.inputs == "broadcast"):
                raise RuntimeError("SlabPipeline: overlapped merge with halo='exchange' or inputs='broadcast' (see __init__)")
            if self.overlap:
                import torch
                if self._side is None:
                    self._side = torch.cuda.Stream()
                marched = torch.cuda.Event()
                marched.record()
                with torch.cuda.stream(self._side):
                    self._side.wait_event(marched)
                    self.composite(d, n, i)
                    self._merged = torch.cuda.Event()
                    self._merged.record(self._side)
            else:
                self.composite(d, n, i)

    def wait_composite(self):
        """Make the current stream wait for an overlapped merge (no-op otherwise)."""
        if self.sframe is not None:
            self.sframe.wait()
            if self.overlap and self.raycast_mode == "exact" and self.world > 1 and self.sframe.count > 0:
                self.ray_d, self.ray_n, self.ray_i = self.sframe.images()   # the set the last frame was rendered into
            return
        if self._merged is not None:
            import torch
            torch.cuda.current_stream().wait_event(self._merged)
            self._merged = None

    def raycast_levels_into(self, outputs, K_levels, T_wc):
        """Several renderings of the model from one pose (the tracking loop's pyramid levels): outputs = [(d, n, i), ...].
        Composite mode renders them with one launch where the operator set has RaycastSdfLevels and merges them with ONE
        pair of collectives (the strips -- or keys and payloads -- of all levels side by side) instead of a pair per level; the
        images equal those of per-level raycast_into calls.  Exact mode hands the march over level by level."""
        if self.raycast_mode == "exact":
            for (d, n, i), K in zip(outputs, K_levels):
                self.raycast_exact(T_wc, d, n, i, K)
            return
        if hasattr(self.ops, "RaycastSdfLevels") and len(outputs) > 1:
            self.ops.RaycastSdfLevels(outputs, self.vol, T_wc, K_levels, self.near, self.far, self.trunc, True)
        else:
            for (d, n, i), K in zip(outputs, K_levels):
                self.ops.RaycastSdf(d, n, i, self.vol, T_wc, K, self.near, self.far, self.trunc, True)
        if self.world > 1:
            self.composite_levels(outputs)

    def _sum_payload(self, payload):
        """The winners' normals / shade, summed over the ranks: on every rank, or (images = "root") on rank 0 only."""
        if self.images == "root":
            self.dist.reduce(payload, dst=0, op=self.dist.ReduceOp.SUM)
        else:
            self.dist.all_reduce(payload, op=self.dist.ReduceOp.SUM)

    def _scratch(self, name, shape, dtype, like):
        """Per-shape device scratch tensors (march state, composite key / payload), allocated once."""
        import torch
        cache = self.__dict__.setdefault("_scratch_cache", {})
        key = (name, tuple(shape))
        if key not in cache:
            cache[key] = torch.empty(shape, dtype=dtype, device=like.tensor().device)
        return cache[key]

    def _exact_setup(self, d, n, i, K):
        """What both exact marches start from: the images and intrinsics (default: the frame's), the slab tuple of the operators, the
        state scratch (9 planes) and its march planes as integers"""
        import torch
        d, n, i = (self.ray_d, self.ray_n, self.ray_i) if d is None else (d, n, i)
        K = self.K if K is None else K
        slab = (self.dims[2], self.s0, float(self.full_boxmin[2]), float(self.full_boxmax[2]))
        st = self._scratch("state", (9, d.h, d.w), torch.float32, d)
        return d, n, i, K, d.w, d.h, slab, st, st[0:5].view(torch.int32)   # (march: contiguous planes 0..4)

    def raycast_exact(self, T_wc, d=None, n=None, i=None, K=None):
        """The march state travels with the ray (the exact variant): world + 1 stages of kfx_raycast_sdf_slab
        -- a rank advances the rays whose current sample lies in the planes it owns --, between them the march planes
        (lambda, last_sdf, delta, status, touched) go to the two NEIGHBOUR ranks only, and a rank adopts the rays a
        neighbour advanced that are still under way (status 0 marching, 3 hit with its normal pending).  A stale copy is
        never acted on: its position lies in planes of a rank the ray has left.  A ray entering at one end needs `world`
        stages, one more lets a hit on a slab boundary get its normal from the neighbour owning the gradient's base plane.
        At the end ONE all-reduce sums the results of the ranks that finalised each pixel (integer bit patterns; rank 0
        answers for rays that never enter the box).  No host synchronisation between the stages.  Depth, normals and
        shade equal RaycastSdf on the whole volume bit for bit."""
        import torch
        dist, o = self.dist, self.ops
        d, n, i, K, w, h, slab, st, march = self._exact_setup(d, n, i, K)
        stages = self.world + 1 if self.world > 1 else 1
        fin = torch.zeros((h, w), dtype=torch.bool, device=st.device)
        from_lo = self._scratch("from_lo", (5, h, w), torch.int32, d) if self.rank > 0 else None
        from_hi = self._scratch("from_hi", (5, h, w), torch.int32, d) if self.rank < self.world - 1 else None
        for stage in range(stages):
            if self.color:   # the finalising rank writes the hit's colour into the shade plane: it travels where the shade travels
                o.RaycastSdfSlabColor(st, stage == 0, self.vol, self.cvol, slab, self.z0, self.z1, w, h, T_wc, K, self.near, self.far, self.trunc, True)
            else:
                o.RaycastSdfSlab(st, stage == 0, self.vol, slab, self.z0, self.z1, w, h, T_wc, K, self.near, self.far, self.trunc, True)
            if self.world == 1:
                break
            status, touched = st[3], march[4] != 0
            fin |= touched & ((status == 1) | (status == 2))
            if stage == 0 and self.rank == 0:
                fin |= ~touched & (status == 2)
            if stage + 1 == stages:
                break
            ops = []
            if from_lo is not None:
                ops += [dist.P2POp(dist.isend, march, self.rank - 1), dist.P2POp(dist.irecv, from_lo, self.rank - 1)]
            if from_hi is not None:
                ops += [dist.P2POp(dist.isend, march, self.rank + 1), dist.P2POp(dist.irecv, from_hi, self.rank + 1)]
            self._p2p(ops)
            taken = torch.zeros_like(fin)
            for buf in (from_lo, from_hi):
                if buf is None:
                    continue
                bstat = buf[3].view(torch.float32)
                take = (buf[4] != 0) & ((bstat == 0) | (bstat == 3)) & ~taken
                march[0:4].copy_(torch.where(take.unsqueeze(0), buf[0:4], march[0:4]))
                taken |= take
        if self.world > 1:
            allst = st.view(torch.int32)
            contrib = torch.stack([allst[0], allst[3], allst[5], allst[6], allst[7], allst[8]])
            contrib = torch.where(fin.unsqueeze(0), contrib, torch.zeros_like(contrib)).contiguous()
            dist.all_reduce(contrib, op=dist.ReduceOp.SUM)
            for k, p in enumerate((0, 3, 5, 6, 7, 8)):
                allst[p].copy_(contrib[k])
            final = (st[3] == 1) | (st[3] == 2)
            assert bool(final.all()), "slab march: %d rays without a final status after world + 1 stages" % int((~final).sum())
        self.rounds = stages
        o.RaycastStateToImages(d, n, i, st)

    def raycast_exact_allreduce(self, T_wc, d=None, n=None, i=None, K=None):
        """The cross-check of raycast_exact: the same kernels with the state merged over ALL ranks after every round.  In a
        round exactly one rank advances a given ray (the owner of the trilinear base plane of its current sample), so the
        merge is one integer SUM all-reduce of the touched pixels' march planes; a host-side termination test follows every
        round (at most world + 2 of them).  The normals (planes 5-8, written by one rank per pixel) are merged once at the end."""
        import torch
        dist, o = self.dist, self.ops
        d, n, i, K, w, h, slab, st, march = self._exact_setup(d, n, i, K)
        rounds = 0
        while True:
            o.RaycastSdfSlab(st, rounds == 0, self.vol, slab, self.z0, self.z1, w, h, T_wc, K,
                             self.near, self.far, self.trunc, True)
            rounds += 1
            if self.world > 1:
                touched = march[4] != 0
                contrib = torch.where(touched.unsqueeze(0), march, torch.zeros_like(march))
                dist.all_reduce(contrib, op=dist.ReduceOp.SUM)
                march.copy_(torch.where((contrib[4] != 0).unsqueeze(0), contrib, march))
            status = st[3]
            if not bool(((status == 0) | (status == 3)).any()):
                break
            assert rounds <= self.world + 3, "slab march did not terminate"
        if self.world > 1:
            out = st[5:9].view(torch.int32)
            dist.all_reduce(out, op=dist.ReduceOp.SUM)
        self.rounds = rounds
        o.RaycastStateToImages(d, n, i, st)

    def _gloo_table(self, mine):
        """gloo with device tensors (the tests' ranks sharing one GPU): its point-to-point path takes ~0.1 s per message, its
        all-reduce does not -- every rank's `mine` summed as integers into one table, (world,) + mine's shape (bits survive)"""
        import torch
        table = torch.zeros((self.world,) + tuple(mine.shape), dtype=torch.int32, device=mine.device)
        table[self.rank] = mine.view(torch.int32)
        self.dist.all_reduce(table)
        return table.view(torch.float32)

    def _gloo_ring(self, send_to, recv_from):
        """gloo, host tensors (the CPU tests): one batch in which this rank sends send_to(r) to every other rank r and receives
        into recv_from(r) from it (None: nothing to send / to receive)"""
        dist, ops = self.dist, []
        for k in range(1, self.world):
            to, frm = (self.rank + k) % self.world, (self.rank - k) % self.world
            out, into = send_to(to), recv_from(frm)
            if out is not None:
                ops.append(dist.P2POp(dist.isend, out, to))
            if into is not None:
                ops.append(dist.P2POp(dist.irecv, into, frm))
        self._p2p(ops)

    def _all_to_all(self, recv, send):
        """recv[r] = rank r's send[self.rank] (dense tensors of shape (world, ...))."""
        if self.dist.get_backend() == "nccl":
            self.dist.all_to_all_single(recv, send)   # RCCL: one grouped send / recv per peer, every link of the mesh at once
        elif send.is_cuda:
            recv.copy_(self._gloo_table(send)[:, self.rank])
        else:
            recv[self.rank].copy_(send[self.rank])
            self._gloo_ring(lambda to: send[to], lambda frm: recv[frm])

    def _gather_strips(self, full, part):
        """full[r] = rank r's part: on every rank, or (images = "root") on rank 0 only."""
        dist, root = self.dist, self.images == "root"
        if dist.get_backend() == "nccl":
            if root:
                dist.gather(part, [full[r] for r in range(self.world)] if self.rank == 0 else None, dst=0)
            else:
                dist.all_gather_into_tensor(full, part)
        elif part.is_cuda:   # (every rank ends up with the strips)
            full.copy_(self._gloo_table(part.reshape(full[self.rank].shape)))
        else:
            full[self.rank].copy_(part)
            sends = (lambda to: part if to == 0 else None) if root else (lambda to: part)   # (images = "root": to rank 0 only ...
            recvs = (lambda frm: None) if root and self.rank != 0 else (lambda frm: full[frm])   # ... and only rank 0 receives)
            self._gloo_ring(sends, recvs)

    def composite_direct_levels(self, outputs):
        """The direct-send merge of several images at once (pyramid levels: outputs = [(d, n, i), ...]): a rank's strips of all
        levels lie side by side in one buffer, so the whole set costs ONE all-to-all and ONE all-gather."""
        import torch
        o, W = self.ops, self.world
        planes = 5
        S = [o.CompositeStripPixels(d.w, d.h, W) for d, _, _ in outputs]
        offs = [0]
        for s_l in S:
            offs.append(offs[-1] + planes * s_l)
        total = offs[-1]
        like = outputs[0][0]
        send = self._scratch("strips_send", (W, total), torch.float32, like)
        recv = self._scratch("strips_recv", (W, total), torch.float32, like)
        merged = self._scratch("strips_merged", (total,), torch.float32, like)
        for (d, n, i), off in zip(outputs, offs):
            o.CompositeStripsPack(d, n, i, send, W, offset=off, rank_stride=total)
        self._all_to_all(recv, send)
        for s_l, off in zip(S, offs):
            o.CompositeStripsMerge(recv, merged, s_l, W, offset=off, rank_stride=total, merged_offset=off)
        self._gather_strips(recv, merged)      # (recv is free again: it becomes the gathered strips)
        if self.images != "root" or self.rank == 0:
            for (d, n, i), off in zip(outputs, offs):
                o.CompositeStripsUnpack(d, n, i, recv, W, offset=off, rank_stride=total)

    def composite_allreduce_levels(self, outputs, scratch=("keys", "payloads")):
        """The all-reduce merge of several images at once: key = depth bits (positive floats order like ints) in the high word, rank in
        the low byte; misses use +inf.  One MIN all-reduce picks the winners, one SUM all-reduce (images = "root": a reduce, only rank
        0's payload is the sum) broadcasts their normal / shade (four floats per pixel; the depth and the hit flag travel in the key).
        The keys and payloads of all images lie side by side, so the whole set costs ONE pair of collectives.  scratch: the names
        of the key / payload scratch (composite(), whose overlapped merge runs on the side stream, keeps its own pair)."""
        import torch
        sizes = [d.w * d.h for d, _, _ in outputs]
        total = sum(sizes)
        key = self._scratch(scratch[0], (total,), torch.int64, outputs[0][0])
        payload = self._scratch(scratch[1], (total * 4,), torch.float32, outputs[0][0])
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        parts = [(key[offs[k]:offs[k + 1]], payload[4 * offs[k]:4 * offs[k + 1]]) for k in range(len(outputs))]
        for (d, n, i), (kk, _) in zip(outputs, parts):
            self.ops.CompositePack(d, n, i, kk, self.rank)
        self.dist.all_reduce(key, op=self.dist.ReduceOp.MIN)
        for (d, n, i), (kk, pp) in zip(outputs, parts):
            self.ops.CompositeSelect(d, n, i, kk, pp, self.rank)
        self._sum_payload(payload)
        for (d, n, i), (kk, pp) in zip(outputs, parts):
            self.ops.CompositeUnpack(d, n, i, kk, pp)

    def composite_levels(self, outputs, **kw):
        """Nearest hit over all slabs for each of outputs = [(d, n, i), ...], by the pipeline's merge: same winner per pixel, same
        images either way.  The per-pixel glue is the operator set's fused kernels (kfx_composite_*, kfx_composite_strips_*)."""
        if self.merge == "direct":
            self.composite_direct_levels(outputs)
        else:
            self.composite_allreduce_levels(outputs, **kw)

    def composite(self, d=None, n=None, i=None):
        """composite_levels of one image (default: the frame's)"""
        self.composite_levels([(self.ray_d, self.ray_n, self.ray_i) if d is None else (d, n, i)], scratch=("key", "payload"))


class TrackingSlabPipeline(_TrackingLoop, SlabPipeline):
    """Tracked KinectFusion on Z-slabs: the tracking loop (_TrackingLoop) with the model spread over the ranks.  The
    raycast of every pyramid level is merged across ranks (raycast_levels_into), after which all ranks hold the same model
    images; the ICP normal equations are image-space work of < 0.1 ms and are evaluated redundantly on every rank
    (deterministic: every rank derives the same pose without a broadcast); SdfFuse then integrates each rank's slab.
    With raycast="exact" the poses and the fused slabs equal the single-GPU TrackingPipeline bit for bit."""

    def __init__(self, ops, dist, dims, boxmin, boxmax, w, h, its=None, icp_c=0.1, max_rmse=0.10, **kw):
        if kw.get("color"):
            raise ValueError("TrackingSlabPipeline: color=True is not built (tracked colour slabs: the tracker fuses its pyramids' level 0 and renders "
                             "pyramid levels, the colour slab path fuses and renders the frame's own images)")
        if kw.get("inputs", "replicate") != "replicate":
            raise ValueError("TrackingSlabPipeline: inputs='broadcast' is not implemented (every rank builds the frame's pyramids itself)")
        if kw.get("overlap"):
            raise ValueError("TrackingSlabPipeline: overlap=True is for known-pose streams (the tracker reads the merged images at once)")
        if kw.get("driver", "python") != "python":
            # the C frame object is bound to SlabPipeline's filtered / normals images at construction; this loop integrates the
            # pyramids' level 0 (kin_d[0] / kin_n[0]) and renders pyramid levels, which kfx_slab_frame_step knows nothing about
            raise ValueError("TrackingSlabPipeline: driver='c' is for known-pose streams (kfx_slab_frame_step integrates the images it was created "
                             "with, not the tracker's pyramids); use driver='python'")
        super().__init__(ops, dist, dims, boxmin, boxmax, w, h, **kw)
        self._init_tracker(its, icp_c, max_rmse, pose_step=hasattr(ops, "PoseStep"))

    def _render_levels(self, lv, T34):
        self.raycast_levels_into([(self.pyr_d[l], self.pyr_n[l], self.pyr_i[l]) for l in lv], [self.K_levels[l] for l in lv], T34)
        for l in lv:
            self.ops.DepthToVbo(self.pyr_v[l], self.pyr_d[l], self.K_levels[l])

    def _refine(self, next_image):
        if self.images != "root" or self.world == 1:
            return super()._refine(next_image)
        # only rank 0 holds the merged model images: it solves, the others receive the pose (and the verdict)
        import torch
        msg = torch.zeros(18, dtype=torch.float64)
        if self.rank == 0:
            T_lp, rmse, good = super()._refine(next_image)
            msg[:16] = torch.from_numpy(np.asarray(T_lp, np.float64).reshape(16))
            msg[16], msg[17] = float(rmse), 1.0 if good else 0.0
        if self.dist.get_backend() == "nccl":
            msg = msg.to(self.pyr_d[0].tensor().device)
        self.dist.broadcast(msg, src=0)
        msg = msg.cpu()
        return msg[:16].numpy().reshape(4, 4).copy(), float(msg[16]), bool(msg[17] != 0)

    def _fuse_at(self, T_wl, T_cw=None):
        # SlabPipeline.fuse integrates self.filtered / self.normals at T_wc; point them at pyramid level 0
        self.filtered, self.normals = self.kin_d[0], self.kin_n[0]
        self.fuse(T_wl[:3].astype(np.float32), T_cw=self.tracking.se3_inv(T_wl)[:3].astype(np.float32) if T_cw is None else T_cw)
