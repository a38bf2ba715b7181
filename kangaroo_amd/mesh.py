"""Mesh extraction: roo::SaveMesh (reference include/kangaroo/MarchingCubes.h:205-262) with the volume left in HBM.

The reference copies the volume to the host, marches the (w-1)(h-1)(d-1) cubes one by one and hands the lists to
Assimp's PLY exporter.  Here (include/kfx_mesh.h): kfx_mesh_plan counts active cubes and triangles per z-segment of a column
and scans them in the reference's emission order on the device (one 16-byte read-back: the totals) -> kfx_mesh_emit compacts
the active cubes at their scanned offsets and emits them (one thread per active cube: vertices, normals, grey colours into
their slots).  fp32 (SDF_t) and half (SDF_h, meshed as the exactly widened volume) cells; the whole volume or one Z-slab of a
partitioned one.  The arrays equal the host algorithm's element for element (tests compare with the oracle); only the
finished arrays cross PCIe.

Indexed output (include/kfx_mesh_index.h), opt-in with indexed=True: the same mesh with one vertex per lattice edge and a face
list -- the sequential first-occurrence weld of the soup above, keyed by the lattice edge (minimum corner, axis) each vertex lies
on: a key seen for the first time gets the next id and that soup vertex's position, normal and colour bit for bit; faces[k] is the
id of soup vertex k's key.  Welded on the device (kfx_mesh_index_plan finds every active cube's owned edges by binary searches in
the compacted cube list and scans them, kfx_mesh_emit_indexed writes V vertices and T faces): a closed surface has V = T/2 + 2, so
a grey mesh shrinks from 72 to 24 bytes per triangle (24 V + 12 T) and a colour mesh from 120 to 32, and adjacency can be read off
the faces as they are.
A slab's indexed mesh is the weld of that rank's soup: vertices on a slab boundary exist once per rank.

Brick mesh (include/kfx_mesh_bricks.h), ExtractBrickMesh / SaveBrickMesh: the soup of packed 8 x 8 x 8 bricks (roo.BrickPack's lists, the
bricks a moving volume spilled) on a frame of any size -- what ExtractMesh returns for the dense volume those bricks would unpack into,
cube by cube and bit for bit, listed brick by brick -- with memory in proportion to the bricks, not the frame.  indexed=True
(include/kfx_mesh_bricks_index.h): the first-occurrence weld of THAT soup by lattice edge, welded on the device across brick faces,
edges and corners -- the vertex set of ExtractMesh(D, indexed=True) in the bricks' order, still without D.

Clean-up (include/kfx_mesh_clean.h), on an indexed mesh in device memory: MeshComponents labels its connected components (two vertices are
connected when a face contains both; numbered by their smallest vertex id), FilterMesh drops the components with fewer than min_faces
faces -- the floaters depth noise and unobserved cells leave around the surface -- or all but the largest, and compacts what is left,
order and bits kept.  min_faces= / largest= on the Extract / Save calls apply it to their indexed=True mesh before anything is downloaded.

Level of detail (include/kfx_mesh_simplify.h), on an indexed mesh in device memory: SimplifyMesh clusters the vertices on a grid anchored
in the world -- one vertex a cell, the one nearest its centre -- and drops the faces that collapse or repeat; every output bit is a
function of the mesh and the grid.  simplify_cell= on the Extract / Save calls applies it after the filter: the mesh's resolution is
no longer tied to the volume's.

Smoothing (include/kfx_mesh_smooth.h), on an indexed mesh in device memory: MeshAdjacency lists every vertex's face corners in ascending
order (and classes the vertices: boundary, non-manifold, degenerate, isolated), SmoothMesh runs Laplacian / Taubin passes over those lists
-- every float sum in the lists' order, so every output bit is a function of the mesh -- and VertexNormals recomputes the normals from the
faces.  smooth= on the Extract / Save calls applies it last, after the filter and the simplification, and replaces the normals.

Case tables: kangaroo_amd/csrc/mc_tables.inc, derived by scripts/gen_mc_tables.py.  Their boundary loops and
winding agree with the classic tables the reference uses in all 256 cases; 158 cases split a polygon along a
different interior diagonal (an equally valid triangulation of the same loop), so meshes are the same surface
patch by patch but not triangle-for-triangle identical to the reference's.

PLY: Assimp (an external library of the reference, absent here) writes the reference's file; this writer emits the
same element set -- per-vertex position, normal and, with a colour volume, RGBA floats; one triangle per three
consecutive vertices -- as a standard ascii or binary_little_endian PLY.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .roo import _stream


CELL = {"f32": 0, "f16": 1}   # KFX_CELL_F32 / KFX_CELL_F16


def _ptr(t):
    """a tensor's device address as a C argument; None (NULL) for None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _extract(dev, stream, nbytes, floor, has_color, indexed, with_index, plan, index_bytes, index_plan, emit, emit_indexed):
    """plan -> [index plan ->] allocate -> emit, for ExtractMesh and ExtractBrickMesh.  plan ... emit_indexed: the ABI calls with their
    leading arguments (the volume, or the frame and the lists) bound; each takes what follows those in its signature, the plan's scratch
    first.  nbytes: the plan's scratch; floor: the least size a scratch is allocated with."""
    empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    scratch = empty(max(nbytes, floor), torch.uint8)
    totals = (C.c_ulonglong * 2)()
    st = _stream(stream)
    code = plan(_ptr(scratch), nbytes, totals, st)
    if code == -4 and totals[1] >= 2 ** 32 // 3:   # KFX_E_RANGE
        raise ValueError("mesh too large for 32-bit vertex offsets")
    _lib.check(code)
    na, ntri = int(totals[0]), int(totals[1])
    nv = 3 * ntri
    if indexed:
        xbytes = index_bytes(totals)
        xscratch = empty(max(xbytes, floor), torch.uint8)
        nvert = C.c_ulonglong(0)
        _lib.check(index_plan(_ptr(scratch), nbytes, totals, _ptr(xscratch), xbytes, C.byref(nvert), st))
        nv = int(nvert.value)
    verts, norms = empty((nv, 3), torch.float32), empty((nv, 3), torch.float32)
    colors = empty((nv, 4), torch.float32) if has_color else None
    if indexed:
        faces = empty((ntri, 3), torch.int32)
        if na:
            _lib.check(emit_indexed(_ptr(scratch), nbytes, _ptr(xscratch), xbytes, totals, nv, _ptr(verts), _ptr(norms), _ptr(colors), _ptr(faces), st))
        return verts, norms, colors, faces
    cube_index, tri_offset = empty(na, torch.int64), empty(na, torch.int32)
    if na:
        _lib.check(emit(_ptr(scratch), nbytes, totals, _ptr(cube_index), _ptr(tri_offset), _ptr(verts), _ptr(norms), _ptr(colors), st))
    if with_index:
        return verts, norms, colors, cube_index, tri_offset
    return verts, norms, colors


def _filter_args(what, indexed, slab, min_faces, largest):
    """whether a filter is asked for; it is honoured on an indexed mesh of a whole volume"""
    if int(min_faces) < 0:
        raise ValueError("%s: min_faces is a face count" % what)
    if not (min_faces or largest):
        return False
    if not indexed:
        raise ValueError("%s: min_faces / largest filter the indexed mesh (indexed=True)" % what)
    if slab is not None:
        raise ValueError("%s: a slab's mesh is welded within its rank, so its components are cut at the slab boundaries; "
                         "min_faces / largest need the whole volume's mesh" % what)
    return True


def _clean_plan(L, faces, n_verts, st):
    """(scratch, nbytes, V, T, counts) of a labelled face list: kfx_mesh_components_plan"""
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces: a (T, 3) int32 tensor of uint32 ids")
    faces = faces.contiguous()
    nv, nt = int(n_verts), int(faces.shape[0])
    nbytes = L.kfx_mesh_components_scratch_bytes(nv, nt)
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=faces.device)
    counts = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_components_plan(_ptr(faces) if nt else None, nt, nv, _ptr(scratch), nbytes, counts, st))   # (nbytes 0: the reason)
    return faces, scratch, nbytes, nv, nt, counts


def MeshComponents(faces, n_verts, stream=None):
    """The connected components of an indexed mesh (include/kfx_mesh_clean.h): faces (T, 3) int32 device tensor of uint32 ids < n_verts.
    Returns (vertex_component (V,), component_faces (C,)), int32 device tensors of uint32 bits: components are numbered in ascending
    order of their smallest vertex id; a vertex in no face is a component of its own with 0 faces."""
    L = _lib.load()
    st = _stream(stream)
    faces, scratch, nbytes, nv, nt, counts = _clean_plan(L, faces, n_verts, st)
    vc = torch.empty(nv, dtype=torch.int32, device=faces.device)
    cf = torch.empty(int(counts[0]), dtype=torch.int32, device=faces.device)
    if nt:
        _lib.check(L.kfx_mesh_components_emit(_ptr(scratch), nbytes, nv, nt, counts, _ptr(vc), _ptr(cf), st))
    return vc, cf


def FilterMesh(verts, norms, colors, faces, min_faces=0, largest=False, stream=None):
    """The indexed mesh (verts, norms, colors, faces) without its small components (include/kfx_mesh_clean.h): min_faces keeps the
    components with at least that many faces, largest only the one with the most (ties: the smaller component id; min_faces still
    applies).  Kept vertices and faces keep their order, faces are renumbered, rows are copied bit for bit; norms / colors may be None.
    Returns new tensors (verts, norms, colors, faces); min_faces=0, largest=False returns the input's bits."""
    L = _lib.load()
    if int(min_faces) < 0:
        raise ValueError("FilterMesh: min_faces is a face count")
    st = _stream(stream)
    verts = verts.contiguous()
    norms = None if norms is None else norms.contiguous()
    colors = None if colors is None else colors.contiguous()
    for t, w, name in ((verts, 3, "verts"), (norms, 3, "norms"), (colors, 4, "colors")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (len(verts), w)):
            raise ValueError("FilterMesh: %s is a (V, %d) float32 tensor" % (name, w))
    faces, scratch, nbytes, nv, nt, counts = _clean_plan(L, faces, len(verts), st)
    kept = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_filter_plan(_ptr(scratch), nbytes, nv, nt, _ptr(faces) if nt else None, int(min_faces), int(bool(largest)), kept, st))
    kv, kt = int(kept[0]), int(kept[1])
    new = lambda t, rows: None if t is None else torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out = (new(verts, kv), new(norms, kv), new(colors, kv), new(faces, kt))
    if kv:
        _lib.check(L.kfx_mesh_filter_emit(_ptr(scratch), nbytes, nv, nt, kept, _ptr(verts), _ptr(norms), _ptr(colors), _ptr(faces),
                                          *[_ptr(t) if t is not None and t.numel() else None for t in out], st))
    return out


def _simplify_args(what, indexed, slab, simplify_cell):
    """whether a simplification is asked for (simplify_cell: None or 0 is off); it is honoured on an indexed mesh of a whole volume"""
    if simplify_cell is None or simplify_cell == 0:
        return False
    if not indexed:
        raise ValueError("%s: simplify_cell clusters the vertices of the indexed mesh (indexed=True)" % what)
    if slab is not None:
        raise ValueError("%s: a slab's mesh is welded within its rank: a cluster that straddles a slab boundary would be two; "
                         "simplify_cell needs the whole volume's mesh" % what)
    return True


def _finish(got, clean, simplify, min_faces, largest, simplify_cell, stream, smooth=None):
    """an indexed mesh after the steps its Extract call was asked for: floaters go first, because clustering changes face counts;
    smoothing (smooth: _smooth_args's keywords, or None) goes last, because it moves what the other two copy"""
    if clean:
        got = FilterMesh(*got, min_faces=min_faces, largest=largest, stream=stream)
    if simplify:
        got = SimplifyMesh(*got, cell=simplify_cell, stream=stream)
    if smooth is not None:
        verts, norms, colors, faces = got
        verts, norms = SmoothMesh(verts, faces, normals=True, stream=stream, **smooth)
        got = (verts, norms, colors, faces)
    return got


SMOOTH_KEYS = ("iterations", "lam", "mu", "pin_boundary")


def _smooth_args(what, indexed, slab, smooth):
    """SmoothMesh's keywords of a smooth= argument -- None: off (returns None); an int: that many iterations; a dict with keys of
    SMOOTH_KEYS --; it is honoured on an indexed mesh of a whole volume"""
    if smooth is None:
        return None
    if isinstance(smooth, dict):
        kw = dict(smooth)
        if set(kw) - set(SMOOTH_KEYS):
            raise ValueError("%s: smooth takes the keys %s (the normals are always recomputed)" % (what, ", ".join(SMOOTH_KEYS)))
    elif isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool):
        kw = dict(iterations=int(smooth))
    else:
        raise ValueError("%s: smooth is None, an iteration count or a dict of SmoothMesh's keywords" % what)
    if int(kw.get("iterations", 5)) < 0:
        raise ValueError("%s: smooth's iterations is a count" % what)
    if not indexed:
        raise ValueError("%s: smooth moves the vertices of the indexed mesh (indexed=True)" % what)
    if slab is not None:
        raise ValueError("%s: a slab's mesh is welded within its rank, so its components are cut at the slab boundaries; "
                         "smooth needs the whole volume's mesh" % what)
    return kw


def _mesh_faces(what, faces):
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces is a (T, 3) int32 tensor of uint32 ids" % what)
    return faces.contiguous()


def MeshAdjacency(faces, n_verts, with_flags=False, stream=None):
    """The incidence lists of an indexed mesh (include/kfx_mesh_smooth.h): faces (T, 3) int32 device tensor of uint32 ids < n_verts.
    Returns (inc_start (V + 1,), inc (3T,)), int32 device tensors of uint32 bits: inc[inc_start[v]:inc_start[v + 1]] are the corner
    slots 3 f + c with faces[f][c] == v, ascending.  with_flags=True: also vertex_flags (V,): bit 0 boundary, 1 non-manifold,
    2 degenerate, 3 isolated.  A function of (n_verts, faces) alone."""
    L = _lib.load()
    faces = _mesh_faces("MeshAdjacency", faces)
    nv, nt = int(n_verts), int(faces.shape[0])
    dev = faces.device
    nbytes = L.kfx_mesh_adjacency_scratch_bytes(nv, nt)
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    start = torch.zeros(nv + 1, dtype=torch.int32, device=dev) if nt == 0 else torch.empty(nv + 1, dtype=torch.int32, device=dev)
    inc = torch.empty(3 * nt, dtype=torch.int32, device=dev)
    flags = torch.empty(nv, dtype=torch.int32, device=dev) if with_flags else None
    _lib.check(L.kfx_mesh_adjacency(_ptr(faces) if nt else None, nt, nv, _ptr(start), _ptr(inc) if nt else None, _ptr(flags) if with_flags and nv else None,
                                    _ptr(scratch), nbytes, _stream(stream)))   # (nbytes 0: the reason)
    return (start, inc, flags) if with_flags else (start, inc)


def _mesh_verts(what, verts):
    verts = verts.contiguous()
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("%s: verts is a (V, 3) float32 tensor" % what)
    return verts


def VertexNormals(verts, faces, stream=None, adjacency=None):
    """Per-vertex normals of an indexed mesh from its faces (include/kfx_mesh_smooth.h): the sum of the cross products of every incident
    face, in the order of the vertex's incidence list, normalised; on the side the extraction's normals lie on; zero for a vertex in no
    face or with a sum of zero or non-finite length.  adjacency: MeshAdjacency's (inc_start, inc[, flags]), if the caller has it."""
    L = _lib.load()
    verts, faces = _mesh_verts("VertexNormals", verts), _mesh_faces("VertexNormals", faces)
    nv, nt = len(verts), int(faces.shape[0])
    start, inc = (adjacency if adjacency is not None else MeshAdjacency(faces, nv, stream=stream))[:2]
    norms = torch.zeros_like(verts) if nt == 0 else torch.empty_like(verts)
    scratch = torch.empty(256, dtype=torch.uint8, device=verts.device)
    _lib.check(L.kfx_mesh_vertex_normals(_ptr(verts) if nv else None, _ptr(faces) if nt else None, nt, nv, _ptr(start), _ptr(inc) if nt else None,
                                         _ptr(norms) if nv else None, _ptr(scratch), 256, _stream(stream)))
    return norms


def SmoothMesh(verts, faces, iterations=5, lam=0.5, mu=-0.53, pin_boundary=True, normals=False, stream=None):
    """The vertices of an indexed mesh after `iterations` smoothing iterations (include/kfx_mesh_smooth.h): each a pass that moves every
    vertex by lam towards the mean of its neighbour entries, then one by mu (< 0: Taubin's, which holds the volume; 0: plain Laplacian
    smoothing, which shrinks).  pin_boundary: vertices on an open boundary stay where they are, bit for bit; so do vertices in no face
    and vertices whose new position would not be finite.  Every sum runs in the order of the vertex's incidence list: the output is a
    function of the arrays and the parameters.  Returns new vertices; normals=True: (verts, norms) with VertexNormals of the new ones."""
    L = _lib.load()
    verts, faces = _mesh_verts("SmoothMesh", verts), _mesh_faces("SmoothMesh", faces)
    nv, nt = len(verts), int(faces.shape[0])
    adjacency = MeshAdjacency(faces, nv, with_flags=bool(pin_boundary), stream=stream)
    flags = adjacency[2] if pin_boundary else None
    nbytes = L.kfx_mesh_smooth_scratch_bytes(nv, nt)
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=verts.device)
    out = verts.clone() if nt == 0 else torch.empty_like(verts)
    _lib.check(L.kfx_mesh_smooth(_ptr(verts) if nv else None, _ptr(faces) if nt else None, nt, nv, _ptr(adjacency[0]), _ptr(adjacency[1]) if nt else None,
                                 _ptr(flags) if flags is not None and nv else None, int(iterations), float(lam), float(mu), 1 if pin_boundary else 0,
                                 _ptr(out) if nv else None, _ptr(scratch), nbytes, _stream(stream)))
    if not normals:
        return out
    return out, VertexNormals(out, faces, stream=stream, adjacency=adjacency)


def SimplifyMesh(verts, norms, colors, faces, cell, origin=(0.0, 0.0, 0.0), stream=None, with_map=False):
    """The indexed mesh (verts, norms, colors, faces) at the level of detail of a grid of `cell` world units anchored at `origin`
    (include/kfx_mesh_simplify.h): the vertices of one grid cell become one vertex -- the one nearest the cell's centre, ties to the
    smaller id, its row copied bit for bit --, faces that lose a corner that way are dropped, and so are all but the first of the faces
    with one set of corners.  Every output bit is a function of the arrays, cell and origin; norms / colors may be None.
    Returns new tensors (verts, norms, colors, faces); with_map=True: also vertex_cluster (V,), every input vertex's new id (uint32 bits
    in an int32 tensor, 0xffffffff where its cluster is not written)."""
    L = _lib.load()
    st = _stream(stream)
    verts = verts.contiguous()
    norms = None if norms is None else norms.contiguous()
    colors = None if colors is None else colors.contiguous()
    for t, w, name in ((verts, 3, "verts"), (norms, 3, "norms"), (colors, 4, "colors")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (len(verts), w)):
            raise ValueError("SimplifyMesh: %s is a (V, %d) float32 tensor" % (name, w))
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("SimplifyMesh: faces is a (T, 3) int32 tensor of uint32 ids")
    faces = faces.contiguous()
    nv, nt = len(verts), int(faces.shape[0])
    nbytes = L.kfx_mesh_simplify_scratch_bytes(nv, nt)
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=faces.device)
    kept = (C.c_ulonglong * 2)()
    org = (C.c_float * 3)(*[float(x) for x in origin])
    _lib.check(L.kfx_mesh_simplify_plan(_ptr(verts) if nv else None, _ptr(faces) if nt else None, nt, nv, org, float(cell), _ptr(scratch), nbytes,
                                        kept, st))   # (nbytes 0: the reason)
    kv, kt = int(kept[0]), int(kept[1])
    new = lambda t, rows: None if t is None else torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out = (new(verts, kv), new(norms, kv), new(colors, kv), new(faces, kt))
    vmap = torch.full((nv,), -1, dtype=torch.int32, device=faces.device) if with_map else None
    if nt:
        _lib.check(L.kfx_mesh_simplify_emit(_ptr(scratch), nbytes, nv, nt, kept, _ptr(verts), _ptr(norms), _ptr(colors), _ptr(faces),
                                            *[_ptr(t) if t is not None and t.numel() else None for t in out],
                                            _ptr(vmap) if with_map and nv else None, st))
    return out + (vmap,) if with_map else out


def ExtractMesh(vol, colorVol=None, stream=None, slab=None, with_index=False, indexed=False, min_faces=0, largest=False, simplify_cell=None,
                smooth=None):
    """Returns (verts, norms, colors): float32 device tensors of shape (3T, 3), (3T, 3) and (3T, 4) or None.
    indexed=True: (verts, norms, colors, faces) with V rows each and faces (T, 3), uint32 ids held in an int32 tensor (the weld
    of the arrays above by lattice edge, see the module docstring).

    vol.kind "f32" or "f16".  slab = (full_d, z_offset, full_zmin, full_zmax, own_lo, own_hi): `vol` holds planes
    [z_offset, z_offset + vol.d) of that volume and the cubes with lower plane in [own_lo, min(own_hi, full_d - 1)) are meshed,
    each triangle bit-identical to the single-volume mesh's; colorVol is then the rank's colour slab (kind "c32", the planes and the
    box of `vol`; fp32 SDF cells) and the colours equal the single-volume mesh's too.  with_index: also return cube_index (int64, global) and
    tri_offset (int32: the first triangle of each active cube, uint32 bits).
    min_faces / largest (with indexed=True, whole volumes): FilterMesh's, applied on the device to the mesh returned.
    simplify_cell (with indexed=True, whole volumes): SimplifyMesh's cell, anchored at the world origin, applied after the filter.
    smooth (with indexed=True, whole volumes): None, an iteration count or a dict of SmoothMesh's iterations / lam / mu / pin_boundary,
    applied last; the normals returned are then VertexNormals of the smoothed mesh, the colours are left as they are."""
    L = _lib.load()
    clean = _filter_args("ExtractMesh", indexed, slab, min_faces, largest)
    simplify = _simplify_args("ExtractMesh", indexed, slab, simplify_cell)
    smooth = _smooth_args("ExtractMesh", indexed, slab, smooth)
    if vol.kind not in CELL:
        raise ValueError("ExtractMesh: volume kind %r (fp32 or half SDF cells)" % vol.kind)
    cell, dev = CELL[vol.kind], vol.storage.device
    sl, lo, hi = None, 0, 0
    if slab is not None:
        full_d, z_offset, zmin, zmax, lo, hi = slab
        sl = C.byref(_lib.KfxSlab(int(full_d), int(z_offset), float(zmin), float(zmax)))
    args = (vol.ref(), cell, sl, int(lo), int(hi))
    nbytes = L.kfx_mesh_scratch_bytes(*args)
    if nbytes == 0:
        _lib.check(L.kfx_mesh_plan(*args, None, 0, None, None))   # the reason
    if indexed and with_index:
        raise ValueError("ExtractMesh: with_index lists the soup's cubes; not with indexed=True")
    # IsValid() of the colour volume -- of the FULL one where colorVol is a slab of it
    has_color = colorVol is not None and min(colorVol.w, colorVol.h, colorVol.d if slab is None else int(slab[0])) >= 8
    cref = colorVol.ref() if has_color else None
    got = _extract(dev, stream, nbytes, 0, has_color, indexed, with_index,
                    plan=lambda *a: L.kfx_mesh_plan(*args, *a),
                    index_bytes=lambda totals: L.kfx_mesh_index_scratch_bytes(*args, totals),
                    index_plan=lambda *a: L.kfx_mesh_index_plan(*args, *a),
                    emit=lambda *a: L.kfx_mesh_emit(*args, cref, *a),
                    emit_indexed=lambda scratch, nbytes, *a: L.kfx_mesh_emit_indexed(*args, cref, *a))   # (reads the index scratch alone)
    return _finish(got, clean, simplify, min_faces, largest, simplify_cell, stream, smooth)


BRICK_BYTES = {"f32": 4096, "f16": 2048, "c32": 2048}   # one packed 8 x 8 x 8 brick of each cell kind


def _brick_list(what, ids, cells, brick_bytes, dev):
    """(ids int32 tensor of uint32 bits, cells uint8 tensor, n) on `dev`; host ids are checked to ascend strictly, as roo.BrickUnpack's"""
    if not torch.is_tensor(ids):
        host = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
        if host.size and (host.min() < 0 or host.max() > 0xffffffff or np.any(np.diff(host) <= 0)):
            raise ValueError("%s: ids must be brick ids in strictly ascending order" % what)
        ids = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev)
    if not torch.is_tensor(cells):
        cells = torch.from_numpy(np.ascontiguousarray(cells).view(np.uint8).reshape(-1)).to(dev)
    ids, cells = ids.contiguous(), cells.contiguous()
    n = ids.numel()
    if cells.numel() * cells.element_size() != n * brick_bytes:
        raise ValueError("%s: %d ids need %d bytes of cells, got %d" % (what, n, n * brick_bytes, cells.numel() * cells.element_size()))
    return ids, cells, n


def BrickMeshScratchBytes(n, n_color=0):
    """kfx_mesh_bricks_scratch_bytes: the scratch of a brick mesh of n SDF and n_color colour bricks -- whatever the frame."""
    return int(_lib.load().kfx_mesh_bricks_scratch_bytes(int(n), int(n_color)))


def ExtractBrickMesh(dims, boxmin, boxmax, kind, ids, cells, color_ids=None, color_cells=None, with_index=False, stream=None, indexed=False,
                     min_faces=0, largest=False, simplify_cell=None, smooth=None):
    """The mesh of packed 8 x 8 x 8 bricks (include/kfx_mesh_bricks.h): what ExtractMesh returns for the dense volume of `dims` cells and
    the box (boxmin, boxmax) that is NaN everywhere and then gets BrickUnpack(ids, cells) -- the same cubes, each with the same triangles
    bit for bit -- without that volume; memory in proportion to the bricks and the mesh.  Only the order differs: brick by brick in
    ascending id, within a brick by ascending cube index (with_index=True returns cube_index and tri_offset, as ExtractMesh).

    kind "f32" or "f16"; ids / cells as roo.BrickPack returns them for a view of these dimensions: torch tensors, or host arrays, which
    are uploaded (host ids are checked to ascend strictly).  color_ids / color_cells: a second list of "c32" bricks on the same frame;
    an absent colour brick reads 0.5.  Colours are returned when color_ids is given and every dimension is >= 8.

    indexed=True: (verts, norms, colors, faces) with V rows each and faces (T, 3), uint32 ids held in an int32 tensor, as ExtractMesh:
    the sequential first-occurrence weld, by lattice edge, of the arrays above in their (brick) order (include/kfx_mesh_bricks_index.h).
    Not with with_index=True, which lists the soup's cubes.
    min_faces / largest (with indexed=True): FilterMesh's, applied on the device to the mesh returned.
    simplify_cell (with indexed=True): SimplifyMesh's cell, anchored at the origin of the box's coordinates, applied after the filter.
    smooth (with indexed=True): ExtractMesh's, applied last."""
    L = _lib.load()
    clean = _filter_args("ExtractBrickMesh", indexed, None, min_faces, largest)
    simplify = _simplify_args("ExtractBrickMesh", indexed, None, simplify_cell)
    smooth = _smooth_args("ExtractBrickMesh", indexed, None, smooth)
    if kind not in CELL:
        raise ValueError("ExtractBrickMesh: cell kind %r (fp32 or half SDF cells)" % (kind,))
    if indexed and with_index:
        raise ValueError("ExtractBrickMesh: with_index lists the soup's cubes; not with indexed=True")
    if (color_ids is None) != (color_cells is None):
        raise ValueError("ExtractBrickMesh: color_ids and color_cells come together (both, or neither)")
    device = ids.device if torch.is_tensor(ids) else (cells.device if torch.is_tensor(cells) else torch.device("cuda", torch.cuda.current_device()))
    ids, cells, n = _brick_list("ExtractBrickMesh", ids, cells, BRICK_BYTES[kind], device)
    want_color = color_ids is not None and min(int(d) for d in dims) >= 8
    cids, ccells, nc = (None, None, 0)
    if want_color:
        cids, ccells, nc = _brick_list("ExtractBrickMesh(colour)", color_ids, color_cells, BRICK_BYTES["c32"], device)
    frame = _lib.KfxVolume(0, None, int(dims[0]), int(dims[1]), 0, int(dims[2]))
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = float(np.float32(boxmin[i])), float(np.float32(boxmax[i]))
    nbytes = BrickMeshScratchBytes(n, nc)   # (0: the counts are refused -- the plan says why)
    sdf = (C.byref(frame), CELL[kind], _ptr(ids) if n else None, _ptr(cells) if n else None, n)
    both = sdf + (_ptr(cids) if nc else None, _ptr(ccells) if nc else None, nc)
    got = _extract(device, stream, nbytes, 256, want_color, indexed, with_index,
                    plan=lambda *a: L.kfx_mesh_bricks_plan(*sdf, *a),
                    index_bytes=lambda totals: L.kfx_mesh_bricks_index_scratch_bytes(n, totals),
                    index_plan=lambda *a: L.kfx_mesh_bricks_index_plan(*sdf, *a),
                    emit=lambda *a: L.kfx_mesh_bricks_emit(*both, *a),
                    emit_indexed=lambda *a: L.kfx_mesh_bricks_emit_indexed(*both, *a))
    return _finish(got, clean, simplify, min_faces, largest, simplify_cell, stream, smooth)


def SaveBrickMesh(filename, dims, boxmin, boxmax, kind, ids, cells, color_ids=None, color_cells=None, binary=True, indexed=False, min_faces=0,
                  largest=False, simplify_cell=None, smooth=None):
    """ExtractBrickMesh's mesh as filename + ".ply" (write_ply); returns the triangle count.  indexed=True: V welded vertices and T faces
    instead of 3T vertices; min_faces / largest / simplify_cell / smooth: ExtractBrickMesh's."""
    arrays = ExtractBrickMesh(dims, boxmin, boxmax, kind, ids, cells, color_ids, color_cells, indexed=indexed, min_faces=min_faces, largest=largest,
                              simplify_cell=simplify_cell, smooth=smooth)
    return _save_mesh(filename, arrays, binary, indexed)


def _save_mesh(filename, arrays, binary, indexed):
    """(verts, norms, colors[, faces]) of an Extract*Mesh as filename + ".ply"; returns the triangle count"""
    verts, norms, colors, *faces = arrays
    torch.cuda.synchronize() if verts.is_cuda else None
    faces = faces[0].cpu().numpy().view(np.uint32) if indexed else None
    write_ply(filename + ".ply", verts.cpu().numpy(), norms.cpu().numpy(), None if colors is None else colors.cpu().numpy(), binary, faces)
    return len(verts) // 3 if faces is None else len(faces)


def write_ply(path, verts, norms, colors=None, binary=True, faces=None):
    """faces=None: one triangle per three consecutive vertices; otherwise the (T, 3) vertex ids of an indexed mesh."""
    verts, norms = np.asarray(verts, np.float32), np.asarray(norms, np.float32)
    n = len(verts)
    ids = np.arange(n, dtype=np.uint32).reshape(-1, 3) if faces is None else np.asarray(faces).astype(np.uint32, copy=False).reshape(-1, 3)
    cols = [verts, norms] + ([np.asarray(colors, np.float32)] if colors is not None else [])
    table = np.concatenate(cols, axis=1)
    names = ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue", "alpha"] if colors is not None else [])
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"),
            "comment kangaroo_amd marching cubes", "element vertex %d" % n]
    head += ["property float %s" % nm for nm in names]
    head += ["element face %d" % len(ids), "property list uchar uint vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            f.write(table.astype("<f4").tobytes())
            rows = np.empty(len(ids), dtype=[("k", "u1"), ("i", "<u4", 3)])
            rows["k"] = 3
            rows["i"] = ids
            f.write(rows.tobytes())
        else:
            for row in table:
                f.write((" ".join("%.9g" % v for v in row) + "\n").encode())
            for a, b, c in ids:
                f.write(("3 %d %d %d\n" % (a, b, c)).encode())


def SaveMesh(filename, vol, colorVol=None, binary=True, slab=None, indexed=False, min_faces=0, largest=False, simplify_cell=None, smooth=None):
    """SaveMesh(filename, vol[, volColor]) (MarchingCubes.h:246-262): writes filename + ".ply"; returns the triangle count.
    fp32 or half volumes; slab: ExtractMesh's.  indexed=True: V welded vertices and T faces (ExtractMesh's) instead of 3T vertices;
    min_faces / largest / simplify_cell / smooth: ExtractMesh's."""
    arrays = ExtractMesh(vol, colorVol, slab=slab, indexed=indexed, min_faces=min_faces, largest=largest, simplify_cell=simplify_cell, smooth=smooth)
    return _save_mesh(filename, arrays, binary, indexed)
