"""The oracle of the mesh smoothing (include/kfx_mesh_smooth.h) in plain numpy: per-vertex incidence lists in ascending order, the vertex
flags, Laplacian / Taubin passes and normals from the faces.  All arithmetic is done on float32 arrays, one operation at a time, so that
every operation rounds as the header states; the sums run sequentially, one vectorised fp32 add per neighbour rank.  Nothing of the
library is used."""
import numpy as np

F = np.float32
BOUNDARY, NONMANIFOLD, DEGENERATE, ISOLATED = 1, 2, 4, 8


def _faces(faces):
    return np.asarray(faces).astype(np.int64).reshape(-1, 3)


def incidence(n_verts, faces):
    """(inc_start int64 [V + 1], inc int64 [3T]): the stable counting sort of the corner slots s = 3 f + c by vertex id"""
    f = _faces(faces)
    ids = f.reshape(-1)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < n_verts)
    inc = np.argsort(ids, kind="stable")
    start = np.zeros(n_verts + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(ids, minlength=n_verts))
    return start, inc


def neighbour_entries(faces, inc):
    """int64 [3T, 2]: per incidence, in the order of inc, a = faces[f][(c + 1) % 3] and b = faces[f][(c + 2) % 3]"""
    f = _faces(faces)
    face, c = inc // 3, inc % 3
    return np.stack([f[face, (c + 1) % 3], f[face, (c + 2) % 3]], axis=1)


def adjacency(n_verts, faces):
    """(inc_start uint32 [V + 1], inc uint32 [3T], vertex_flags uint32 [V]): the contract of kfx_mesh_adjacency"""
    start, inc = incidence(n_verts, faces)
    deg = np.diff(start)
    owner = np.repeat(np.repeat(np.arange(n_verts, dtype=np.int64), deg), 2)   # the vertex of every neighbour entry
    u = neighbour_entries(faces, inc).reshape(-1)
    flags = np.zeros(n_verts, np.uint32)
    flags[deg == 0] |= ISOLATED
    flags[np.unique(owner[u == owner])] |= DEGENERATE
    other = u != owner
    pairs, cnt = np.unique(owner[other] * max(n_verts, 1) + u[other], return_counts=True)   # cnt(v, u) of every pair (v, u) that occurs
    flags[np.unique(pairs[cnt == 1] // max(n_verts, 1))] |= BOUNDARY
    flags[np.unique(pairs[cnt > 2] // max(n_verts, 1))] |= NONMANIFOLD
    return start.astype(np.uint32), inc.astype(np.uint32), flags


def _ranked_sum(n_verts, start, count, rows):
    """acc[v] = ((0 + rows[start[v]]) + rows[start[v] + 1]) + ... over count[v] rows, sequentially in fp32: one vectorised add per rank"""
    acc = np.zeros((n_verts, 3), F)
    order = np.argsort(-count, kind="stable")   # the vertices with more than r rows are a prefix of this
    more = np.searchsorted(-count[order], -np.arange(int(count.max()) if n_verts else 0), side="left")   # how many have count > r
    for r in range(len(more)):
        sel = order[:more[r]]
        acc[sel] = acc[sel] + rows[start[sel] + r]
    assert acc.dtype == F
    return acc


def smooth(verts, faces, iterations=5, lam=0.5, mu=-0.53, pin_mask=0, adj=None):
    """float32 [V, 3]: the contract of kfx_mesh_smooth.  adj: adjacency(V, faces), if the caller has it"""
    p = np.ascontiguousarray(verts, dtype=F).reshape(-1, 3).copy()
    n = len(p)
    start, inc, flags = adj if adj is not None else adjacency(n, faces)
    start, inc = start.astype(np.int64), inc.astype(np.int64)
    entries = neighbour_entries(faces, inc).reshape(-1)
    count = 2 * np.diff(start)
    still = (count == 0) | ((flags & np.uint32(pin_mask)) != 0)
    m = count.astype(F)
    for it in range(int(iterations)):
        for factor in ((lam, mu) if mu != 0 else (lam,)):
            with np.errstate(all="ignore"):
                acc = _ranked_sum(n, 2 * start[:-1], count, p[entries])
                d = acc / m[:, None] - p
                o = p + F(factor) * d
            assert d.dtype == F and o.dtype == F
            keep = still | ~np.isfinite(o).all(axis=1)
            p = np.where(keep[:, None], p.view(np.uint32), o.view(np.uint32)).view(F)   # rows are copied as words
    return p


def face_normals(verts, faces):
    """float32 [T, 3]: e2 x e1 of every face (the side the extraction's normals lie on), each product and difference rounded on its own"""
    p = np.ascontiguousarray(verts, dtype=F).reshape(-1, 3)
    f = _faces(faces)
    with np.errstate(all="ignore"):
        e1 = p[f[:, 1]] - p[f[:, 0]]
        e2 = p[f[:, 2]] - p[f[:, 0]]
        n = np.stack([e1[:, 2] * e2[:, 1] - e1[:, 1] * e2[:, 2],
                      e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0],
                      e1[:, 1] * e2[:, 0] - e1[:, 0] * e2[:, 1]], axis=1)
    assert n.dtype == F
    return n


def vertex_normals(verts, faces, adj=None):
    """float32 [V, 3]: the contract of kfx_mesh_vertex_normals"""
    n = len(np.asarray(verts).reshape(-1, 3))
    start, inc = (adj[0], adj[1]) if adj is not None else incidence(n, faces)
    start, inc = np.asarray(start).astype(np.int64), np.asarray(inc).astype(np.int64)
    deg = np.diff(start)
    with np.errstate(all="ignore"):
        acc = _ranked_sum(n, start[:-1], deg, face_normals(verts, faces)[inc // 3])
        sq = acc * acc
        l2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        out = acc / np.sqrt(l2)[:, None]
    assert out.dtype == F
    out[~(np.isfinite(l2) & (l2 > 0)) | (deg == 0)] = 0
    return out


# ---- hand-made cases with the answers written out ----
# name -> dict(verts, faces, inc_start, inc, flags, smooth: the rows after ONE pass with lambda = 0.5 (mu = 0, nothing pinned),
#              normals: {vertex: its normal} for the vertices whose normal is written out here)

_NAN = float("nan")
_T3 = F(F(2) / F(6)) * F(0.5)   # (2 / 6) * 0.5 in fp32
_T6 = F(F(1) / F(6)) * F(0.5)   # (1 / 6) * 0.5 in fp32
_R3 = F(F(1) / np.sqrt(F(3)))   # 1 / sqrtf(3)
_SQUARE = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
_DOWN = (0, 0, -1)   # of a face that winds anticlockwise seen from +z: the extraction's faces wind the other way

HAND_MADE = {
    "single_triangle": dict(
        verts=[[0, 0, 0], [1, 0, 0], [0, 1, 0]], faces=[[0, 1, 2]],
        inc_start=[0, 1, 2, 3], inc=[0, 1, 2], flags=[BOUNDARY] * 3,
        smooth=[[0.25, 0.25, 0], [0.5, 0.25, 0], [0.25, 0.5, 0]],
        normals={0: _DOWN, 1: _DOWN, 2: _DOWN}),
    # two triangles on the edge (1, 2): every vertex has a neighbour it meets once
    "two_triangles": dict(
        verts=_SQUARE, faces=[[0, 1, 2], [1, 3, 2]],
        inc_start=[0, 1, 3, 5, 6], inc=[0, 1, 3, 2, 5, 4], flags=[BOUNDARY] * 4,
        smooth=[[0.25, 0.25, 0], [0.625, 0.375, 0], [0.375, 0.625, 0], [0.75, 0.75, 0]],
        normals={0: _DOWN, 1: _DOWN, 2: _DOWN, 3: _DOWN}),
    # closed and manifold: every neighbour is met twice, no flag is set; the faces wind anticlockwise seen from outside, so the normals point inwards
    "tetrahedron": dict(
        verts=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], faces=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]],
        inc_start=[0, 3, 6, 9, 12], inc=[0, 3, 6, 2, 4, 9, 1, 8, 10, 5, 7, 11], flags=[0] * 4,
        smooth=[[_T3, _T3, _T3], [0.5, _T3, _T3], [_T3, 0.5, _T3], [_T3, _T3, 0.5]],
        normals={0: (_R3, _R3, _R3), 1: (-1, 0, 0), 2: (0, -1, 0), 3: (0, 0, -1)}),
    # a closed fan: the hub is interior, the rim is boundary
    "fan": dict(
        verts=[[0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], faces=[[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]],
        inc_start=[0, 4, 6, 8, 10, 12], inc=[0, 3, 6, 9, 1, 11, 2, 4, 5, 7, 8, 10], flags=[0] + [BOUNDARY] * 4,
        smooth=[[0, 0, 0.5], [0.5, 0, 0.25], [0, 0.5, 0.25], [-0.5, 0, 0.25], [0, -0.5, 0.25]],
        normals={0: _DOWN}),
    # face 0 names vertex 0 twice: two incidences, and 0 is its own neighbour
    "degenerate": dict(
        verts=[[0, 0, 0], [1, 0, 0], [0, 1, 0]], faces=[[0, 0, 1], [0, 1, 2]],
        inc_start=[0, 3, 5, 6], inc=[0, 1, 3, 2, 4, 5], flags=[BOUNDARY | NONMANIFOLD | DEGENERATE, BOUNDARY | NONMANIFOLD, BOUNDARY],
        smooth=[[0.25, _T6, 0], [0.5, 0.125, 0], [0.25, 0.5, 0]],
        normals={0: _DOWN, 1: _DOWN, 2: _DOWN}),
    # three faces on the edge (0, 1)
    "nonmanifold": dict(
        verts=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], faces=[[0, 1, 2], [1, 0, 3], [0, 1, 4]],
        inc_start=[0, 3, 6, 7, 8, 9], inc=[0, 4, 6, 1, 3, 7, 2, 5, 8], flags=[BOUNDARY | NONMANIFOLD] * 2 + [BOUNDARY] * 3,
        smooth=[[0.25, 0, _T6], [0.5, 0, _T6], [0.25, 0.5, 0], [0.25, -0.5, 0], [0.25, 0, 0.5]],
        normals={2: _DOWN, 3: _DOWN, 4: (0, 1, 0)}),
    # vertex 4 is in no face: it stays, and its normal is zero
    "isolated": dict(
        verts=_SQUARE + [[5, 5, 5]], faces=[[0, 1, 2], [1, 3, 2]],
        inc_start=[0, 1, 3, 5, 6, 6], inc=[0, 1, 3, 2, 5, 4], flags=[BOUNDARY] * 4 + [ISOLATED],
        smooth=[[0.25, 0.25, 0], [0.625, 0.375, 0], [0.375, 0.625, 0], [0.75, 0.75, 0], [5, 5, 5]],
        normals={0: _DOWN, 3: _DOWN, 4: (0, 0, 0)}),
    # vertex 1 has a NaN coordinate: it stays as it is, and so does every vertex that would have read it -- the whole row, not the one
    # coordinate; every face has it as a corner, so every normal is zero
    "nan_vertex": dict(
        verts=[[0, 0, 0], [_NAN, 0, 0], [0, 1, 0], [1, 1, 0]], faces=[[0, 1, 2], [1, 3, 2]],
        inc_start=[0, 1, 3, 5, 6], inc=[0, 1, 3, 2, 5, 4], flags=[BOUNDARY] * 4,
        smooth=[[0, 0, 0], [_NAN, 0, 0], [0, 1, 0], [1, 1, 0]],
        normals={0: (0, 0, 0), 1: (0, 0, 0), 2: (0, 0, 0), 3: (0, 0, 0)}),
}


def hand_made(name):
    """(verts float32 [V, 3], faces uint32 [T, 3], the case's dict)"""
    case = HAND_MADE[name]
    return np.asarray(case["verts"], F), np.asarray(case["faces"], np.uint32).reshape(-1, 3), case


def random_mesh(n_verts, n_faces, seed):
    """n_verts random vertices in [0, 1)^3 and n_faces random faces (repeated ids and unreferenced vertices among them)"""
    rng = np.random.RandomState(seed)
    verts = rng.rand(n_verts, 3).astype(F)
    faces = rng.randint(0, n_verts, size=(n_faces, 3)).astype(np.uint32)
    return verts, faces

