"""The oracle of the mesh clean-up (include/kfx_mesh_clean.h) in plain numpy: connected components of a face list by min-label
propagation to a fixed point, their numbering and face counts, and the filter.  Nothing of the library is used, nor scipy."""
import numpy as np


def smallest_ids(faces, n_verts):
    """label[v] = the smallest vertex id of v's component.  Every round gives each face's three vertices the least label among them
    and then lets every vertex take its label's label until that stops changing; the fixed point is reached when a round changes
    nothing."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    assert f.size == 0 or (f.min() >= 0 and f.max() < n_verts)
    label = np.arange(n_verts, dtype=np.int64)
    while True:
        new = label.copy()
        if len(f):
            m = label[f].min(axis=1)
            for k in range(3):
                np.minimum.at(new, f[:, k], m)
        while True:   # labels only fall, and label[v] is always a vertex of v's component
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label
        label = new


def components(faces, n_verts):
    """(vertex_component uint32 [V], component_faces uint32 [C]): components numbered in ascending order of their smallest vertex id; a
    face (degenerate or not) counts for the component of its vertices; a vertex in no face is a component with 0 faces"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    label = smallest_ids(f, n_verts)
    roots = np.flatnonzero(label == np.arange(n_verts))
    rank = np.full(n_verts, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    vc = rank[label]
    cf = np.bincount(vc[f[:, 0]], minlength=len(roots)) if len(f) else np.zeros(len(roots), np.int64)
    return vc.astype(np.uint32), cf.astype(np.uint32)


def kept_components(component_faces, min_faces=0, largest=False):
    """bool [C]: at least min_faces faces; largest: only the component with the most faces (ties: the smaller id), min_faces on top"""
    cf = np.asarray(component_faces).astype(np.int64)
    keep = cf >= min_faces
    if largest and len(cf):
        only = np.zeros(len(cf), bool)
        only[int(np.argmax(cf))] = True   # (argmax: the first of equals)
        keep &= only
    return keep


def filter_mesh(verts, norms, colors, faces, min_faces=0, largest=False):
    """(verts', norms', colors', faces' uint32): rows of the kept vertices and faces in their order, bits untouched, ids renumbered"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    n = len(verts)
    vc, cf = components(f, n)
    keep = kept_components(cf, min_faces, largest)
    kv = keep[vc] if n else np.zeros(0, bool)
    kf = kv[f[:, 0]] if len(f) else np.zeros(0, bool)
    remap = np.cumsum(kv) - 1
    rows = lambda a: None if a is None else np.asarray(a)[kv]
    return rows(verts), rows(norms), rows(colors), remap[f[kf]].astype(np.uint32).reshape(-1, 3)


# ---- hand-made face lists with known answers ----

def strip(n_tris, order):
    """a strip of n_tris triangles over n_tris + 2 vertices; position i along it has id order[i]"""
    i = np.arange(n_tris)
    return np.asarray(order)[np.stack([i, i + 1, i + 2], axis=1)].astype(np.uint32)


def permuted_strip(n_tris=5000, seed=20240611):
    return strip(n_tris, np.random.RandomState(seed).permutation(n_tris + 2)), n_tris + 2


def descending_strip(n_tris=5000):
    return strip(n_tris, np.arange(n_tris + 2)[::-1]), n_tris + 2


def fan(n_faces=4096, hub=77):
    """n_faces triangles around one hub vertex"""
    rim = np.array([v for v in range(n_faces + 2) if v != hub], dtype=np.int64)
    return np.stack([np.full(n_faces, hub), rim[:-1], rim[1:]], axis=1).astype(np.uint32), n_faces + 2


HAND_MADE = {
    # name: (faces, V, vertex_component, component_faces)
    "one_triangle": ([[0, 1, 2]], 3, [0, 0, 0], [1]),
    "shared_vertex": ([[0, 1, 2], [2, 3, 4]], 5, [0, 0, 0, 0, 0], [2]),
    "two_disjoint": ([[3, 4, 5], [0, 1, 2]], 6, [0, 0, 0, 1, 1, 1], [1, 1]),
    "isolated_between": ([[0, 2, 4], [9, 7, 6], [4, 0, 2], [6, 9, 7]], 10, [0, 1, 0, 2, 0, 3, 4, 4, 5, 4], [2, 0, 0, 0, 2, 0]),   # (V <= 3T)
    "degenerate": ([[0, 1, 2], [4, 4, 4], [5, 5, 3], [1, 1, 2]], 6, [0, 0, 0, 1, 2, 1], [2, 1, 1]),
}


def three_spheres(oracle, n=48):
    """the three-sphere volume: the minimum of three sphere distances in [-1, 1]^3, n^3 cells"""
    parts = []
    for centre, radius in (((-0.45, -0.1, 0.0), 0.35), ((0.45, 0.1, 0.05), 0.33), ((0.0, 0.7, 0.6), 0.08)):
        vol = oracle.Volume(n, n, n, (-1, -1, -1), (1, 1, 1))
        oracle.sdf_sphere(vol, centre, radius)
        parts.append(vol)
    sdf = parts[0].data[..., 0]
    sdf[...] = np.minimum(np.minimum(sdf, parts[1].data[..., 0]), parts[2].data[..., 0])
    return parts[0]


def split_parts(faces, n_verts):
    """[(faces renumbered, vertex count)] of every component that has faces, in component order"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    vc, cf = components(f, n_verts)
    out = []
    for c in np.flatnonzero(cf):
        kv = vc == c
        out.append(((np.cumsum(kv) - 1)[f[kv[f[:, 0]]]], int(kv.sum())))
    return out
