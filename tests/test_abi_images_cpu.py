"""The one rule for image arguments (kangaroo_amd/csrc/host_args.h: check_image), as tests/test_abi_cpu.py pins the one for volumes:
for every family of entry points that takes images, one image argument breaks exactly one rule and the call returns that rule's
code -- KFX_E_NULL, then KFX_E_SHAPE (smaller than the launch, a row of its own width beyond its pitch), then KFX_E_ALIGN -- before
any launch.  An empty launch keeps each entry point's answer: 0 where it returns before it compares sizes.  The pointers are fake and
every row is a rejection or an empty launch, so no device is needed and none is touched."""
import ctypes as C

from kangaroo_amd import _lib, slab

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
FAKE = 1 << 20
W, H = 16, 8
R = C.byref

NULL, PITCH, PTR_ALIGN, PITCH_ALIGN, NARROW, LOW = ("null pointer", "pitch one pixel short of its row", "pointer misaligned by half a pixel",
                                                    "pitch misaligned", "one pixel narrower than the lead", "one pixel lower than the lead")
EMPTY = "one pixel narrower than the lead of an empty launch"


def image(elem, w=W, h=H, pitch=None, ptr=FAKE):
    return _lib.KfxImage(w * elem if pitch is None else pitch, ptr, w, h)


def volume(cell, d=16, ptr=FAKE):
    return _lib.KfxVolume(16 * cell, ptr, 16, 16, 16 * cell * 16, d)


def broken(elem, w, h, companion):
    """(rule, image, code): images of `elem`-byte pixels that break exactly one rule; the size rows only for a companion of the lead image"""
    rows = [(NULL, image(elem, w, h, ptr=None), E_NULL), (PITCH, image(elem, w, h, pitch=w * elem - elem), E_SHAPE)]
    if elem % 2 == 0:   # (bytes and 3-byte RGB have no alignment to break)
        rows += [(PTR_ALIGN, image(elem, w, h, ptr=FAKE + elem // 2), E_ALIGN), (PITCH_ALIGN, image(elem, w, h, pitch=w * elem + elem // 2), E_ALIGN)]
    if companion:
        rows += [(NARROW, image(elem, w - 1, h), E_SHAPE), (LOW, image(elem, w, h - 1), E_SHAPE)]
    return rows


class Family:
    """An entry point and its image arguments: args = [(name, elem, companion of the lead?, (w, h))], call(images by name) -> code"""
    def __init__(self, name, args, call, codes=None, empty=E_SHAPE):
        self.name, self.call, self.codes, self.empty = name, call, codes or {}, empty
        self.args = [(a[0], a[1], a[2], a[3] if len(a) > 3 else (W, H)) for a in args]

    def rows(self):
        good = {n: image(e, *wh) for n, e, _, wh in self.args}
        for n, e, companion, wh in self.args:
            for rule, im, code in broken(e, wh[0], wh[1], companion):
                yield self.name, n, rule, (lambda im=im, n=n: self.call(dict(good, **{n: im}))), self.codes.get((n, rule), self.codes.get(rule, code))
        # an empty launch (the lead is w x 0) keeps the entry point's answer: 0 where it returns before it compares sizes, else the size rule's code
        lead = next(((n, e, wh) for n, e, companion, wh in self.args if not companion and n != "rgb"), None)
        for n, e, companion, wh in self.args:
            if companion and lead:
                arg = {lead[0]: image(lead[1], lead[2][0], 0), n: image(e, wh[0] - 1, wh[1])}
                yield self.name, n, EMPTY, (lambda arg=arg: self.call(dict(good, **arg))), self.codes.get((n, EMPTY), self.empty)


def families():
    L = slab._L()
    K = (C.c_float * 4)(500, 500, 7.5, 3.5)
    Tm = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    v3 = (C.c_float * 3)(0.1, 0.2, 0.3)
    vol8, vol4, cvol = volume(8), volume(4), volume(4)
    TRIO = [("depth", 4, True), ("norm", 16, True), ("img", 4, False)]
    out = []

    def add(name, args, call, codes=None, empty=E_SHAPE):
        out.append(Family(name, args, call, codes, empty))

    # ---- preprocess ----
    add("kfx_bilateral_f32", [("out", 4, False), ("in", 4, True)], lambda a: L.kfx_bilateral_f32(R(a["out"]), R(a["in"]), 1.5, 0.1, 3, 0.2, 1, None), empty=0)
    add("kfx_bilateral_u16", [("out", 4, False), ("in", 2, True)], lambda a: L.kfx_bilateral_u16(R(a["out"]), R(a["in"]), 1.5, 0.1, 3, 1, None), empty=0)
    add("kfx_bilateral_u8", [("out", 4, False), ("in", 1, True)], lambda a: L.kfx_bilateral_u8(R(a["out"]), R(a["in"]), 1.5, 0.1, 3, None), empty=0)
    add("kfx_bilateral_guided_f32", [("out", 4, False), ("in", 4, True), ("guide", 4, True)],
        lambda a: L.kfx_bilateral_guided_f32(R(a["out"]), R(a["in"]), R(a["guide"]), 1.5, 0.1, 0.1, 3, None), empty=0)
    add("kfx_bilateral_guided_u8", [("out", 4, False), ("in", 4, True), ("guide", 1, True)],
        lambda a: L.kfx_bilateral_guided_u8(R(a["out"]), R(a["in"]), R(a["guide"]), 1.5, 0.1, 0.1, 3, None), empty=0)
    add("kfx_depth_to_vbo_f32", [("vbo", 16, False), ("depth", 4, True)], lambda a: L.kfx_depth_to_vbo_f32(R(a["vbo"]), R(a["depth"]), K, 1.0, None), empty=0)
    add("kfx_depth_to_vbo_u16", [("vbo", 16, False), ("depth", 2, True)], lambda a: L.kfx_depth_to_vbo_u16(R(a["vbo"]), R(a["depth"]), K, 1.0, None), empty=0)
    add("kfx_normals_from_vbo", [("nrm", 16, False), ("vbo", 16, True)], lambda a: L.kfx_normals_from_vbo(R(a["nrm"]), R(a["vbo"]), None), empty=0)
    add("kfx_depth_to_vbo_normals_f32", [("vbo", 16, False), ("nrm", 16, True), ("depth", 4, True)],
        lambda a: L.kfx_depth_to_vbo_normals_f32(R(a["vbo"]), R(a["nrm"]), R(a["depth"]), K, 1.0, None), empty=0)
    add("kfx_elementwise_scale_bias_f32", [("out", 4, False), ("in", 4, True)], lambda a: L.kfx_elementwise_scale_bias_f32(R(a["out"]), R(a["in"]), 2.0, 1.0, None), empty=0)
    add("kfx_box_half_ignore_invalid_f32", [("out", 4, False), ("in", 4, True, (2 * W, 2 * H))],   # (the input covers twice the output)
        lambda a: L.kfx_box_half_ignore_invalid_f32(R(a["out"]), R(a["in"]), None), empty=0)
    add("kfx_disp2depth", [("out", 4, False), ("in", 4, True)], lambda a: L.kfx_disp2depth(R(a["in"]), R(a["out"]), 500.0, 0.1, 0.0, None), empty=0)
    add("kfx_filter_bad_kinect_f32", [("out", 4, False), ("in", 4, True)], lambda a: L.kfx_filter_bad_kinect_f32(R(a["out"]), R(a["in"]), None), empty=0)
    add("kfx_filter_bad_kinect_u16", [("out", 4, False), ("in", 2, True)], lambda a: L.kfx_filter_bad_kinect_u16(R(a["out"]), R(a["in"]), None), empty=0)
    add("kfx_colour_vbo", [("id", 4, False), ("vbo", 16, True), ("rgb", 3, False)], lambda a: L.kfx_colour_vbo(R(a["id"]), R(a["vbo"]), R(a["rgb"]), Tm, None), empty=0)
    kf = _lib.KfxKeyframe()
    kf.img = image(3)
    add("kfx_texture_depth", [("img", 16, False), ("depth", 4, True), ("norm", 16, True), ("phong", 4, True)],
        lambda a: L.kfx_texture_depth(R(a["img"]), R(kf), 1, R(a["depth"]), R(a["norm"]), R(a["phong"]), Tm, K, None), empty=0)

    # ---- RaycastSdf ----
    def trio(a):
        return R(a["depth"]), R(a["norm"]), R(a["img"])
    zeros = C.create_string_buffer(4096)   # a summary of the wrong cell type (0 bytes): looked at only after the images
    add("kfx_raycast_sdf", TRIO, lambda a: L.kfx_raycast_sdf(*trio(a), R(vol8), Tm, K, 0.1, 1.0, 0.1, 1, None))
    add("kfx_raycast_sdf_h", TRIO, lambda a: L.kfx_raycast_sdf_h(*trio(a), R(vol4), Tm, K, 0.1, 1.0, 0.1, 1, None))
    add("kfx_raycast_sdf_tracked", TRIO, lambda a: L.kfx_raycast_sdf_tracked(*trio(a), R(vol8), zeros, Tm, K, 0.1, 1.0, 0.1, 1, None))
    add("kfx_raycast_sdf_color", TRIO, lambda a: L.kfx_raycast_sdf_color(*trio(a), R(vol8), R(cvol), Tm, K, 0.1, 1.0, 0.1, 1, None))

    def levels(a):
        one = lambda im: (_lib.PI * 1)(C.pointer(im))
        return L.kfx_raycast_sdf_levels(1, one(a["depth"]), one(a["norm"]), one(a["img"]), one(a["vbo"]), R(vol8), Tm, K, 0.1, 1.0, 0.1, 1, None)
    add("kfx_raycast_sdf_levels", TRIO + [("vbo", 16, True)], levels, {("vbo", EMPTY): 0})   # (an empty level is skipped)

    def colour_pass(a):
        one = lambda im: (_lib.PI * 1)(C.pointer(im))
        return L.kfx_raycast_color_hits(1, one(a["depth"]), one(a["img"]), R(cvol), Tm, K, None)
    add("kfx_raycast_color_hits", [("depth", 4, False), ("img", 4, True)], colour_pass)
    # HOLE CLOSED: took any pitch and any alignment before
    add("kfx_raycast_state_to_images", TRIO, lambda a: L.kfx_raycast_state_to_images(*trio(a), FAKE, None), empty=0)

    # ---- analytic ----  CODE CORRECTED: a misaligned image was KFX_E_SHAPE in these three before
    add("kfx_raycast_box", [("imgd", 4, False)], lambda a: L.kfx_raycast_box(R(a["imgd"]), Tm, K, v3, v3, None))
    add("kfx_raycast_sphere", [("imgd", 4, False), ("img", 4, True)], lambda a: L.kfx_raycast_sphere(R(a["imgd"]), R(a["img"]), Tm, K, v3, 0.5, None),
        {("img", NULL): None})   # (an image without a pointer is "no image" here: the call is valid)
    add("kfx_raycast_plane", [("imgd", 4, False), ("img", 4, True)], lambda a: L.kfx_raycast_plane(R(a["imgd"]), R(a["img"]), Tm, K, v3, None))
    add("kfx_sdf_distance", [("dist", 4, True), ("depth", 4, False)], lambda a: L.kfx_sdf_distance(R(a["dist"]), R(a["depth"]), R(vol8), Tm, K, 0.1, None), empty=0)

    # ---- SdfFuse ----
    add("kfx_sdf_fuse", [("depth", 4, False), ("norm", 16, True)], lambda a: L.kfx_sdf_fuse(R(vol8), R(a["depth"]), R(a["norm"]), Tm, K, 0.1, 100.0, 0.1, 0, None))
    add("kfx_sdf_fuse_color", [("depth", 4, False), ("norm", 16, True), ("rgb", 3, False)],
        lambda a: L.kfx_sdf_fuse_color(R(vol8), R(cvol), R(a["depth"]), R(a["norm"]), Tm, K, R(a["rgb"]), Tm, K, 0.1, 100.0, 0.1, 0, None))

    # ---- composite: the depth image bounds the launch ----  HOLE CLOSED: no pitch test in the five before
    COMP = [("depth", 4, False), ("norm", 16, True), ("img", 4, True)]
    add("kfx_composite_pack", COMP, lambda a: L.kfx_composite_pack(*trio(a), FAKE, 0, None))
    add("kfx_composite_select", COMP, lambda a: L.kfx_composite_select(*trio(a), FAKE, FAKE, 0, None))
    add("kfx_composite_unpack", COMP, lambda a: L.kfx_composite_unpack(*trio(a), FAKE, FAKE, None))
    add("kfx_composite_strips_pack", COMP, lambda a: L.kfx_composite_strips_pack(*trio(a), FAKE, 0, 2, None))
    add("kfx_composite_strips_unpack", COMP, lambda a: L.kfx_composite_strips_unpack(*trio(a), FAKE, 0, 2, None))

    # ---- ICP ----  HOLE CLOSED: no pitch test before; a given debug image of kfx_icp_refine was not tested at all (a misaligned one
    # was silently left unwritten)
    ICP = [("Pl", 16, False), ("Pr", 16, True), ("Nr", 16, True), ("debug", 16, True)]
    work = image(4, 4096, 64)
    lss = _lib.KfxLss6()
    add("kfx_icp_point_plane", ICP, lambda a: L.kfx_icp_point_plane(R(a["Pl"]), R(a["Pr"]), R(a["Nr"]), Tm, Tm, 0.1, R(work), R(a["debug"]), R(lss), None),
        {("debug", NULL): None}, empty=0)   # (a debug image without a pointer is "no debug image": the call is valid)

    def refine(a):
        lv = _lib.KfxIcpLevel()
        lv.Pl, lv.Pr, lv.Nr, lv.iterations = a["Pl"], a["Pr"], a["Nr"], 1
        T_lp, rmse, obs, good = (C.c_double * 12)(), C.c_float(), C.c_uint(), C.c_int()
        return L.kfx_icp_refine(R(lv), 1, 0.1, 1.0, R(work), R(a["debug"]), T_lp, R(rmse), R(obs), R(good), None)
    add("kfx_icp_refine", ICP, refine, {("debug", NULL): None, ("debug", NARROW): None, ("debug", LOW): None, ("debug", EMPTY): None})   # (a smaller debug image is not written)

    # ---- Z-slabs ----
    lb = slab.Comm.loopback(3, 8)
    lay = slab.layout(64, 2.0, 4.0, 3, 8, 2)
    local, clocal = volume(8, d=lay.s1 - lay.s0), volume(4, d=lay.s1 - lay.s0)
    # HOLE CLOSED: no alignment test before
    add("kfx_slab_broadcast_inputs", [("depth", 4, False), ("norm", 16, True)], lambda a: L.kfx_slab_broadcast_inputs(R(a["depth"]), R(a["norm"]), FAKE, 0, lb.ref(), None))
    # HOLE CLOSED: these two tested the pointers to the structs only, and left the rest to kfx_raycast_state_to_images after the march
    add("kfx_slab_raycast_exact", TRIO, lambda a: L.kfx_slab_raycast_exact(*trio(a), FAKE, FAKE, R(local), R(lay), Tm, K, 0.1, 1.0, 0.1, 1, lb.ref(), None, None))
    add("kfx_slab_raycast_exact_allreduce", TRIO,
        lambda a: L.kfx_slab_raycast_exact_allreduce(*trio(a), FAKE, FAKE, R(local), R(lay), Tm, K, 0.1, 1.0, 0.1, 1, lb.ref(), None, None))
    add("kfx_slab_raycast_exact_tiled", TRIO,
        lambda a: L.kfx_slab_raycast_exact_tiled(*trio(a), FAKE, R(local), R(lay), Tm, K, 0.1, 1.0, 0.1, 1, 4, lb.ref(), None, None, None))
    L_tiled_color = _lib.load().kfx_slab_raycast_exact_tiled_color
    add("kfx_slab_raycast_exact_tiled_color", TRIO,
        lambda a: L_tiled_color(*trio(a), FAKE, R(local), R(clocal), C.addressof(lay), Tm, K, 0.1, 1.0, 0.1, 1, 4, C.addressof(lb.c), None, None, None))

    # ---- the frame objects: a view without a pointer is a malformed configuration (KFX_E_SHAPE, as tests/test_abi_cpu.py has it) ----
    # HOLE CLOSED: the alignment of the seven views was not tested before.  CODE CORRECTED: a misaligned pipe image was KFX_E_SHAPE
    VIEWS = [("raw", 4, False), ("filtered", 4, True), ("vbo", 16, True), ("normals", 16, True)]
    RAY = [("ray_depth", 4, True), ("ray_norm", 16, True), ("ray_img", 4, False)]

    def frame_create(a):
        cfg, h = _lib.KfxFrameConfig(), C.c_void_p()
        cfg.vol = volume(8)
        for n, im in a.items():
            setattr(cfg, n, im)
        rc = L.kfx_frame_create(R(h), R(cfg))
        if rc == 0:
            L.kfx_frame_destroy(h)
        return rc
    # (kfx_frame_create leaves "rendering images smaller than ray_img" to the raycast of each step)
    add("kfx_frame_create", VIEWS + RAY, frame_create, {NULL: E_SHAPE, ("ray_depth", NARROW): None, ("ray_depth", LOW): None, ("ray_norm", NARROW): None, ("ray_norm", LOW): None})

    def slab_frame_create(a, pipe=False):
        cfg, h = slab.KfxSlabFrameConfig(), C.c_void_p()
        cfg.layout, cfg.local = lay, local
        for n, e, _ in VIEWS + RAY:
            setattr(cfg, n, image(e))
        if pipe:   # the exact raycast's overlap: image sets 1 .. pipe_depth - 1
            cfg.raycast, cfg.overlap, cfg.pipe_depth = slab.RAYCAST["exact"], 1, 2
        for n, im in a.items():
            if n.startswith("pipe"):
                cfg.pipe_images[int(n[4:])] = im
            else:
                setattr(cfg, n, im)
        rc = L.kfx_slab_frame_create(R(h), R(cfg), lb.ref())
        if rc == 0:
            L.kfx_slab_frame_destroy(h)
        return rc
    add("kfx_slab_frame_create", VIEWS + RAY, slab_frame_create, {NULL: E_SHAPE})
    add("kfx_slab_frame_create(pipe_images)", [("pipe0", 4, True), ("pipe1", 16, True), ("pipe2", 4, True)], lambda a: slab_frame_create(a, True), {NULL: E_SHAPE})
    return out


def image_rule_rows():
    """(family, argument, rule, call, code) for every row of the table; code None: the call is valid that way, no row"""
    for fam in families():
        for row in fam.rows():
            if row[4] is not None:
                yield row


def test_one_broken_rule_of_one_image_argument_gives_that_rules_code():
    """kfx_slab_frame_set_color's rgb image is not here: it needs a frame object, and kfx_slab_frame_create allocates
    (tests/test_gpu_slab_frame_ring.py has its rows, rejections only).  Against the parent of this table's commit the rows marked
    HOLE CLOSED / CODE CORRECTED in families() differ, and no other."""
    wrong, n = [], 0
    for family, arg, rule, call, code in image_rule_rows():
        got = call()
        n += 1
        if got != code:
            wrong.append((family, arg, rule, "expected %d, got %d" % (code, got)))
    assert not wrong, wrong
    assert n > 500
