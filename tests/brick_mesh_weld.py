"""The expected indexed BRICK mesh (include/kfx_mesh_bricks_index.h), built on the CPU from a brick soup: the sequential
first-occurrence weld keyed by lattice edge.  A plain helper module for the indexed brick-mesh tests; nothing here calls the library.

The brick soup holds three vertices per triangle in the bricks' order, and its cubes are listed with it (cube_index, tri_offset as
kfx_mesh_bricks_emit writes them), so soup vertex k's cube follows from the lists and its case-table edge from the volume D the
bricks unpack into: per cube the case flag is recomputed from D in numpy (mesh_weld.cube_cases) and the tables' edge lists are laid
end to end, cube by cube in the order listed.  The key is mesh_weld's, ((X h + Y) d + Z) 3 + axis in frame cells, in int64."""
import numpy as np

import mesh_weld as W
import test_mesh_cpu as TM


def soup_keys(val, cube_index, tri_offset, ntri, dims=None, origin=(0, 0, 0)):
    """Per brick-soup vertex, in the soup's order: the lattice-edge key (int64) and the position of its cube in cube_index.

    val: D's values, an array (d, h, w[, 2]) or an oracle volume.  dims = (w, h, d) of the frame and origin = the frame cell of
    val[0, 0, 0] where val is only the part of a larger frame that holds the bricks (default: val is the frame)."""
    ntab, _, tri = TM.tables()
    val = W.values(val)
    w, h, d = [int(v) for v in (dims if dims is not None else val.shape[::-1])]
    ox, oy, oz = [int(v) for v in origin]
    flag, finite = W.cube_cases(val)
    ci = np.asarray(cube_index).astype(np.int64)
    z, y, x = ci % (d - 1), (ci // (d - 1)) % (h - 1), ci // ((d - 1) * (h - 1))
    lx, ly, lz = x - ox, y - oy, z - oz
    assert finite[lx, ly, lz].all(), "a listed cube has a corner that is not finite"
    f = flag[lx, ly, lz]
    to = np.asarray(tri_offset).view(np.uint32).astype(np.int64)
    per = 3 * np.diff(np.append(to, int(ntri)))
    assert np.array_equal(per, 3 * ntab[f].astype(np.int64)), "the listed cubes' triangle counts are not the case tables'"
    cube = np.repeat(np.arange(len(ci)), per)                 # soup vertex -> listed cube
    start = np.repeat(3 * to, per)
    e = tri[f[cube], np.arange(len(cube)) - start].astype(np.int64)
    assert (e >= 0).all()
    X, Y, Z = x[cube] + W.EDGE_MIN[e, 0], y[cube] + W.EDGE_MIN[e, 1], z[cube] + W.EDGE_MIN[e, 2]
    key = ((X * h + Y) * d + Z) * 3 + W.EDGE_AXIS[e]
    return key, cube


def weld(val, soup_verts, soup_norms, soup_cols, cube_index, tri_offset, dims=None, origin=(0, 0, 0)):
    """((verts, norms, cols or None, faces uint32 (T, 3)), other): the indexed mesh of the brick soup, and the number of lattice edges
    whose first cube in the soup's order is another than their first cube in dense order (the lowest ci among the cubes using them)."""
    ntri = len(soup_verts) // 3
    key, cube = soup_keys(val, cube_index, tri_offset, ntri, dims, origin)
    assert len(key) == len(soup_verts) == len(soup_norms), (len(key), len(soup_verts))
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")                  # unique keys by first occurrence
    ident = np.empty(len(order), np.int64)
    ident[order] = np.arange(len(order))
    faces = ident[inverse].astype(np.uint32).reshape(-1, 3)
    pick = first[order]
    part = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[pick])
    ci = np.asarray(cube_index).astype(np.int64)
    dense_first = np.full(len(first), np.iinfo(np.int64).max)
    np.minimum.at(dense_first, inverse, ci[cube])
    other = int((ci[cube[first]] != dense_first).sum())
    return (part(soup_verts), part(soup_norms), part(soup_cols), faces), other


def ids_in_first_occurrence_order(faces, n_verts):
    """Vertex ids 0 .. V - 1 all occur, each for the first time after every lower one."""
    flat = np.asarray(faces).astype(np.int64).reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    return len(ids) == n_verts and (n_verts == 0 or (ids[0] == 0 and ids[-1] == n_verts - 1)) and bool(np.all(np.diff(first) > 0))


def brick_order(val, dims=None):
    """The active cubes of D in the brick soup's order -- (cube_index int64, triangles per cube) -- and, for reordering a dense soup,
    the permutation `perm` of the dense soup's TRIANGLES that puts them into that order."""
    ntab, _, _ = TM.tables()
    val = W.values(val)
    d, h, w = val.shape
    flag, finite = W.cube_cases(val)
    n = np.where(finite, ntab[flag], 0).reshape(-1).astype(np.int64)   # dense emission order = C order of [x, y, z]
    active = np.flatnonzero(n)
    x, y, z = np.unravel_index(active, flag.shape)
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    bid = ((z >> 3) * nby + (y >> 3)) * nbx + (x >> 3)
    order = np.lexsort((active, bid))                          # by brick id, then by ci
    cnt = n[active]
    start = np.cumsum(cnt) - cnt                               # first triangle of every active cube in the dense soup
    perm = np.concatenate([np.arange(start[k], start[k] + cnt[k]) for k in order]) if len(order) else np.zeros(0, np.int64)
    return active[order].astype(np.int64), cnt[order], perm
