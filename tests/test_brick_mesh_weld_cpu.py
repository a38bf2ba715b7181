"""The comparator of the indexed brick mesh (tests/brick_mesh_weld.py) on the CPU, without the library: the oracle's marching-cubes
soup, reordered into the bricks' order (brick by brick in ascending id, within a brick by ascending cube index), and welded.  The
weld has one vertex per lattice edge (mesh_weld.count_lattice_edges, which knows no case tables and no order), numbers them by
first occurrence, closes the sphere -- and on the ragged volume with the NaN lattice it has edges whose first cube is another than
in dense order: the case that separates the brick index's owner rule from the dense one."""
import numpy as np
import pytest

from kfx_testlib import oracle

import brick_mesh_weld as BW
import mesh_weld as W
import test_mesh_cpu as TM

# lattice edges of the ragged volume whose first cube in brick order is not their first cube in dense order, as the oracle's
# sdf_sphere arithmetic gives them
RAGGED_OTHER_OWNERS = 44


def box_of(dims, voxel):
    return (0.0, 0.0, 0.0), tuple((d - 1) * voxel for d in dims)


def sphere():
    """test_gpu_brick_mesh.py's case 1: 40 x 24 x 32, voxel 1/16, centred on the corner eight bricks share"""
    dims = (40, 24, 32)
    ovol = oracle.Volume(*dims, *box_of(dims, 1 / 16))
    oracle.sdf_sphere(ovol, (1.0, 0.5, 1.0), 0.4)
    return ovol


def ragged():
    """its ragged case: 44 x 29 x 35, partial bricks on all three axes, the % 7 NaN lattice"""
    dims = (44, 29, 35)
    ovol = oracle.Volume(*dims, *box_of(dims, 1 / 16))
    oracle.sdf_sphere(ovol, (0.5, 0.9, 1.0), 1.15)
    ovol.data[:, :, :, 0][(np.add.outer(np.add.outer(np.arange(dims[2]), np.arange(dims[1])), np.arange(dims[0])) % 7) == 0] = np.nan
    return ovol


def brick_soup(ovol):
    """the oracle's soup in the bricks' order, with its cube list"""
    v, n, _ = oracle.marching_cubes(ovol, None, *TM.tables())
    ci, cnt, perm = BW.brick_order(ovol)
    assert cnt.sum() == len(v) // 3 == len(perm)
    take = lambda a: np.ascontiguousarray(a.reshape(-1, 3, 3)[perm].reshape(-1, 3))
    tri_offset = (np.cumsum(cnt) - cnt).astype(np.uint32)
    return take(v), take(n), ci, tri_offset


@pytest.mark.parametrize("case", ["sphere", "ragged"])
def test_the_weld_of_the_brick_ordered_oracle_soup(case):
    ovol = sphere() if case == "sphere" else ragged()
    v, n, ci, to = brick_soup(ovol)
    assert len(v) > 300 and not np.all(np.diff(ci) > 0)        # (brick order is not dense order)
    (wv, wn, wc, faces), other = BW.weld(ovol, v, n, None, ci, to)
    V, T = len(wv), len(faces)
    print("%s: T = %d, V = %d, lattice edges with another first cube than in dense order: %d" % (case, T, V, other))
    assert wc is None and faces.dtype == np.uint32 and T == len(v) // 3
    assert V == W.count_lattice_edges(ovol)
    assert BW.ids_in_first_occurrence_order(faces, V)
    # de-indexing gives the soup's keys back: every soup vertex maps to the vertex kept for its edge
    key, _ = BW.soup_keys(ovol, ci, to, T)
    flat = faces.reshape(-1).astype(np.int64)
    assert len(np.unique(key)) == V and all(len(np.unique(key[flat == i])) == 1 for i in range(0, V, max(1, V // 50)))
    # the same vertex set as the dense order's weld, in another numbering
    dense = W.weld(ovol, *oracle.marching_cubes(ovol, None, *TM.tables())[:2])
    assert len(dense[0]) == V and len(dense[3]) == T
    if case == "sphere":
        assert V == T // 2 + 2 and W.closed_with_euler_2(faces, V)
        assert other == 0                                      # every cube around an edge is active: the minimum one is first in both orders
    else:
        assert other >= 1
        assert other == RAGGED_OTHER_OWNERS
