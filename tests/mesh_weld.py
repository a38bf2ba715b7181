"""The expected indexed mesh (include/kfx_mesh_index.h), built on the CPU from a marching-cubes soup: the sequential first-occurrence
weld keyed by lattice edge.  A plain helper module for the indexed-mesh tests; nothing here calls the library.

The soup holds three vertices per triangle in emission order (cubes x outer, y, z inner; within a cube the case's triangle list),
so soup vertex k's cube and case-table edge follow from the volume alone: per cube the case flag and the finiteness of its eight
corners are recomputed here in numpy (corner order of mesh.hip's corner_dx / dy / dz = gen_mc_tables.CORNER), the cubes with
triangles are walked in order, and their tables' edge lists are laid end to end."""
import numpy as np

import test_mesh_cpu as TM

CORNER = np.array(TM.G.CORNER)   # (8, 3): x, y, z offsets
EDGE = np.array(TM.G.EDGE)       # (12, 2): the corners an edge joins
EDGE_MIN = np.minimum(CORNER[EDGE[:, 0]], CORNER[EDGE[:, 1]])             # (12, 3) minimum corner of each edge
EDGE_AXIS = np.argmax(CORNER[EDGE[:, 0]] != CORNER[EDGE[:, 1]], axis=1)   # (12,) the axis in which its corners differ


def values(vol_host):
    """(d, h, w) float32 SDF values of an oracle volume, or of an array (d, h, w[, 2])."""
    a = np.asarray(getattr(vol_host, "data", vol_host))
    return np.asarray(a[..., 0] if a.ndim == 4 else a, np.float32)


def cube_cases(val):
    """flag (cx, cy, cz) and finite (cx, cy, cz) of every cube, indexed [x, y, z]."""
    d, h, w = val.shape
    flag = np.zeros((w - 1, h - 1, d - 1), np.int32)
    finite = np.ones((w - 1, h - 1, d - 1), bool)
    for i, (dx, dy, dz) in enumerate(CORNER):
        c = val[dz:d - 1 + dz, dy:h - 1 + dy, dx:w - 1 + dx].transpose(2, 1, 0)
        flag |= (c <= 0).astype(np.int32) << i
        finite &= np.isfinite(c)
    return flag, finite


def soup_keys(vol_host, z_range=None):
    """Per soup vertex of the WHOLE volume's soup, in emission order: the lattice-edge key (int64) and whether its cube's lower plane
    lies in z_range (all True without one)."""
    ntri, _, tri = TM.tables()
    val = values(vol_host)
    d, h, w = val.shape
    flag, finite = cube_cases(val)
    n = np.where(finite, ntri[flag], 0).reshape(-1)            # emission order = C order of [x, y, z]
    active = np.flatnonzero(n)
    x, y, z = np.unravel_index(active, flag.shape)
    f = flag.reshape(-1)[active]
    per = 3 * n[active].astype(np.int64)
    cube = np.repeat(np.arange(len(active)), per)              # soup vertex -> active cube
    start = np.repeat(np.cumsum(per) - per, per)
    e = tri[f[cube], np.arange(len(cube)) - start].astype(np.int64)   # its case-table edge
    assert (e >= 0).all()
    X, Y, Z = x[cube] + EDGE_MIN[e, 0], y[cube] + EDGE_MIN[e, 1], z[cube] + EDGE_MIN[e, 2]
    key = ((X.astype(np.int64) * h + Y) * d + Z) * 3 + EDGE_AXIS[e]
    mine = np.ones(len(cube), bool) if z_range is None else (z[cube] >= z_range[0]) & (z[cube] < z_range[1])
    return key, mine


def weld(vol_host, soup_verts, soup_norms, soup_cols=None, z_range=None):
    """(verts, norms, cols or None, faces uint32 (T, 3)): the indexed mesh of the soup -- of its triangles from the cubes with lower plane in
    z_range = (lo, hi) where one is given (a slab rank's part; the soup passed is always the whole volume's)."""
    key, mine = soup_keys(vol_host, z_range)
    assert len(key) == len(soup_verts) == len(soup_norms), (len(key), len(soup_verts))
    key = key[mine]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                   # unique keys by first occurrence
    ident = np.empty(len(order), np.int64)
    ident[order] = np.arange(len(order))
    faces = ident[inverse.reshape(-1)].astype(np.uint32).reshape(-1, 3)
    pick = first[order]
    part = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[mine][pick])
    return part(soup_verts), part(soup_norms), part(soup_cols), faces


def count_lattice_edges(vol_host):
    """The vertex count without the case tables: lattice edges whose endpoints are finite with different (<= 0) signs and that have at
    least one adjacent cube with eight finite corners."""
    val = values(vol_host)
    _, finite = cube_cases(val)
    pad = np.pad(finite, 1)                                    # [x + 1, y + 1, z + 1]
    v = val.transpose(2, 1, 0)                                 # [x, y, z]
    ok, neg = np.isfinite(v), v <= 0
    total = 0
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        crossing = ok[tuple(a)] & ok[tuple(b)] & (neg[tuple(a)] != neg[tuple(b)])   # edge with minimum corner [x, y, z]
        u, w_ = [k for k in range(3) if k != axis]
        near = np.zeros(crossing.shape, bool)
        for su in (0, 1):
            for sw in (0, 1):                                  # the cube at the minimum corner minus (su, sw) in the other two axes
                s = [None] * 3
                s[axis] = slice(1, 1 + crossing.shape[axis])
                s[u] = slice(1 - su, 1 - su + crossing.shape[u])
                s[w_] = slice(1 - sw, 1 - sw + crossing.shape[w_])
                near |= pad[tuple(s)]
        total += int((crossing & near).sum())
    return total


def closed_with_euler_2(faces, n_verts):
    """Every directed edge once, its reverse once, no degenerate triangle, V - E + F = 2."""
    f = np.asarray(faces, np.int64)
    if (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 2] == f[:, 0]).any():
        return False
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = de[:, 0] * n_verts + de[:, 1]
    rev = de[:, 1] * n_verts + de[:, 0]
    if len(np.unique(code)) != len(code) or not np.isin(rev, code).all():
        return False
    return n_verts - len(code) // 2 + len(f) == 2


def ulp(m):
    return float(np.spacing(np.float32(abs(m))))
