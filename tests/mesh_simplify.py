"""The oracle of the mesh simplification (include/kfx_mesh_simplify.h) in plain numpy: vertex clustering on a world-anchored grid.  All
arithmetic is done on float32 arrays, one operation at a time, so that every operation rounds as the header states.  Nothing of the
library is used."""
import numpy as np

F = np.float32
DROPPED = 0xffffffff
CELLS = 1 << 20   # cell indices lie in [-2^20, 2^20)


def clusters(verts, cell, origin=(0.0, 0.0, 0.0)):
    """(rep int64 [V], singleton bool [V], d2 float32 [V]): rep[v] is the representative of v's cluster -- the vertex of its cell with the
    smallest d2, ties to the smaller id; a singleton (a q that is not finite, a cell index outside [-2^20, 2^20)) is its own"""
    p = np.ascontiguousarray(verts, dtype=F).reshape(-1, 3)
    n = len(p)
    o = np.asarray(origin, dtype=F)
    inv = F(1.0) / F(cell)
    with np.errstate(all="ignore"):
        q = (p - o) * inv                       # two roundings
        i = np.floor(q)
        ok = np.isfinite(q) & (i >= F(-CELLS)) & (i < F(CELLS))
        single = ~ok.all(axis=1)
        t = (q - i) - F(0.5)
        sq = t * t
        d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    assert q.dtype == F and t.dtype == F and d2.dtype == F
    ids = np.arange(n, dtype=np.int64)
    rep = ids.copy()
    live = np.flatnonzero(~single)
    if len(live):
        ii = i[live].astype(np.int64) + CELLS
        key = ii[:, 0] | ii[:, 1] << 21 | ii[:, 2] << 42
        # within a cell: ascending d2 (as a non-negative float32 its bits order as it does), then ascending id
        order = np.lexsort((live, d2[live].view(np.uint32), key))
        skey = key[order]
        first = np.ones(len(order), bool)
        first[1:] = skey[1:] != skey[:-1]
        group = np.cumsum(first) - 1
        rep[live[order]] = live[order][first][group]
    d2 = np.where(single, F(0), d2)
    return rep, single, d2


def simplify(verts, norms, colors, faces, cell, origin=(0.0, 0.0, 0.0)):
    """(verts', norms', colors', faces' uint32 [T', 3], vertex_cluster uint32 [V]): the contract of include/kfx_mesh_simplify.h"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    n = len(verts)
    assert f.size == 0 or (f.min() >= 0 and f.max() < n)
    rep, _, _ = clusters(verts, cell, origin)
    c = rep[f]
    alive = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    idx = np.flatnonzero(alive)
    keep = np.zeros(len(f), bool)
    if len(idx):
        s = np.sort(c[idx], axis=1)
        _, first = np.unique(s, axis=0, return_index=True)   # (the first occurrence: the smallest face id)
        keep[idx[first]] = True
    kept = c[keep]
    written = np.zeros(n, bool)
    written[kept.reshape(-1)] = True
    new = np.full(n, DROPPED, np.int64)
    new[written] = np.arange(int(written.sum()))
    rows = lambda a: None if a is None else np.asarray(a)[written]
    vmap = new[rep] if n else np.zeros(0, np.int64)
    return rows(verts), rows(norms), rows(colors), new[kept].astype(np.uint32).reshape(-1, 3), vmap.astype(np.uint32)


def is_identity(verts, faces, out):
    """whether `out` = simplify(verts, ..., faces, ...) is the input bit for bit"""
    v, f = np.asarray(verts, F), np.asarray(faces, np.uint32).reshape(-1, 3)
    return out[0].shape == v.shape and np.array_equal(out[0].view(np.uint32), v.view(np.uint32)) and np.array_equal(out[3], f)


def properties(out):
    """three distinct ids per face; no two faces with one id set; every vertex referenced"""
    f = out[3].astype(np.int64)
    n = len(out[0])
    if (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 0] == f[:, 2]).any():
        return False
    if len(np.unique(np.sort(f, axis=1), axis=0)) != len(f):
        return False
    return len(f) == 0 and n == 0 or (f.min() >= 0 and f.max() < n and len(np.unique(f)) == n)


# ---- hand-made cases with the answers written out: name -> (verts, faces, cell, origin, V', T', faces', vertex_cluster) ----

_NAN, _INF = float("nan"), float("inf")

HAND_MADE = {
    # two triangles across the cell face x = 1 (cell 1): vertices 0, 1 in cell (0,0,0), 2, 3 in cell (1,0,0); both faces have two equal clusters
    "across_a_face": ([[0.5, 0.5, 0.5], [0.9, 0.1, 0.5], [1.1, 0.9, 0.5], [1.5, 0.5, 0.5]], [[0, 1, 2], [1, 3, 2]], 1.0, (0, 0, 0),
                      0, 0, [], [DROPPED] * 4),
    # floorf: -0.25 and +0.25 lie in cells -1 and 0 of x; 1.0 lies exactly on a boundary and belongs to cell 1, with 1.25; the face survives
    "floor_not_trunc": ([[-0.25, 0.5, 0.5], [0.25, 0.5, 0.5], [1.0, 0.5, 0.5], [1.25, 0.5, 0.5]], [[0, 1, 2], [0, 1, 3]], 1.0, (0, 0, 0),
                        3, 1, [[0, 1, 2]], [0, 1, 2, 2]),
    # d2 tie: vertices 1 and 2 are mirror images about the centre of cell (0,0,0), vertex 0 is farther: the representative is 1
    "tie_to_smaller_id": ([[0.125, 0.5, 0.5], [0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]],
                          [[0, 3, 4], [2, 3, 5]], 1.0, (0, 0, 0), 4, 2, [[0, 1, 2], [0, 1, 3]], [0, 0, 0, 1, 2, 3]),
    # a NaN, an Inf and an out-of-range vertex (2^20 cells of 1 from the origin) stay singletons though 0, 1 and 2, 3 "share" coordinates
    "singletons": ([[_NAN, 0.5, 0.5], [_NAN, 0.5, 0.5], [_INF, 0.5, 0.5], [_INF, 0.5, 0.5], [1048576.0, 0.5, 0.5], [1048576.5, 0.5, 0.5],
                    [0.5, 0.5, 0.5], [1.5, 0.5, 0.5]],
                   [[0, 1, 6], [2, 3, 7], [4, 5, 6]], 1.0, (0, 0, 0), 8, 3, [[0, 1, 6], [2, 3, 7], [4, 5, 6]], [0, 1, 2, 3, 4, 5, 6, 7]),
    # (a, b, c) and (c, b, a) after clustering: the first is kept; so is its winding
    "mirror_pair": ([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 1.6, 0.5], [1.6, 0.6, 0.5], [0.6, 0.6, 0.5]],
                    [[1, 2, 0], [3, 4, 5], [2, 1, 5]], 1.0, (0, 0, 0), 3, 1, [[1, 2, 0]], [0, 1, 2, 2, 1, 0]),
    # a fan whose rim falls into one cell: every face has two equal clusters
    "fan_collapses": ([[0.5, 0.5, 1.5], [0.1, 0.1, 0.5], [0.9, 0.1, 0.5], [0.9, 0.9, 0.5], [0.1, 0.9, 0.5]],
                      [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], 1.0, (0, 0, 0), 0, 0, [], [DROPPED] * 5),
    # a cell small enough that every vertex has its own: the input bit for bit; an origin that is not zero
    "identity": ([[0.5, 0.5, 0.5], [0.9, 0.1, 0.5], [1.1, 0.9, 0.5], [1.5, 0.5, 0.5]], [[0, 1, 2], [1, 3, 2]], 0.125, (0.03, -0.02, 0.01),
                 4, 2, [[0, 1, 2], [1, 3, 2]], [0, 1, 2, 3]),
}


def hand_made(name):
    verts, faces, cell, origin, nv, nt, want_faces, vmap = HAND_MADE[name]
    return (np.asarray(verts, F), np.asarray(faces, np.uint32).reshape(-1, 3), cell, origin, nv, nt,
            np.asarray(want_faces, np.uint32).reshape(-1, 3), np.asarray(vmap, np.uint32))


def random_mesh(n_verts, n_faces, cells, seed, extent=1.0):
    """n_verts random vertices over cells^3 cells of [0, extent)^3 and n_faces random faces; returns (verts, faces, cell)"""
    rng = np.random.RandomState(seed)
    verts = (rng.rand(n_verts, 3) * extent).astype(F)
    faces = rng.randint(0, n_verts, size=(n_faces, 3)).astype(np.uint32)
    return verts, faces, extent / cells
