"""The numpy oracle of the mesh simplification (tests/mesh_simplify.py, the contract of include/kfx_mesh_simplify.h) on hand-made cases
with the answers written out.  No GPU, nothing of the library."""
import numpy as np
import pytest

import mesh_simplify as MS


@pytest.mark.parametrize("name", sorted(MS.HAND_MADE))
def test_oracle_gives_the_written_answer(name):
    verts, faces, cell, origin, nv, nt, want_faces, vmap = MS.hand_made(name)
    norms = -verts
    cols = np.arange(4 * len(verts), dtype=np.float32).reshape(-1, 4)
    v, n, c, f, m = MS.simplify(verts, norms, cols, faces, cell, origin)
    assert (len(v), len(f)) == (nv, nt)
    assert f.dtype == np.uint32 and np.array_equal(f, want_faces)
    assert m.dtype == np.uint32 and np.array_equal(m, vmap)
    # rows are the representatives', bit for bit, in ascending order of their ids
    rep, _, _ = MS.clusters(verts, cell, origin)
    written = np.flatnonzero((rep == np.arange(len(verts))) & (vmap != MS.DROPPED))
    assert np.array_equal(m[written], np.arange(nv))
    for got, src in ((v, verts), (n, norms), (c, cols)):
        assert np.array_equal(got.view(np.uint32), src[written].view(np.uint32))
    assert MS.properties((v, n, c, f))


def test_two_triangles_across_a_cell_face():
    verts, faces, cell, origin, *_ = MS.hand_made("across_a_face")
    rep, single, _ = MS.clusters(verts, cell, origin)
    assert rep.tolist() == [0, 0, 3, 3] and not single.any()   # (0.5, 0.5, 0.5) and (1.5, 0.5, 0.5) are cell centres
    # with the grid moved by half a cell in x the cut falls between 1 and 2 no longer: vertices 0, 1 and 2 share cell [0.5, 1.5)
    rep, _, _ = MS.clusters(verts, cell, (0.5, 0.0, 0.0))
    assert rep[0] == rep[1] == rep[2] and rep[3] != rep[2]


def test_floorf_at_negative_coordinates_and_on_a_boundary():
    verts = np.array([[-0.25, 0, 0], [0.25, 0, 0], [-1.0, 0, 0], [-1.0000001, 0, 0], [2.0, 0, 0], [1.9999999, 0, 0]], np.float32)
    rep, single, _ = MS.clusters(verts, 1.0)
    assert not single.any()
    assert rep[0] != rep[1]             # truncation would put both into cell 0
    assert rep[2] == rep[0]             # -1.0 lies exactly on a boundary and belongs to cell -1, with -0.25
    assert rep[3] not in (rep[0], rep[2])   # the float below -1.0 lies in cell -2
    assert rep[4] != rep[5] and rep[5] != rep[1]   # 2.0 belongs to cell 2, the float below it to cell 1


def test_d2_tie_goes_to_the_smaller_id():
    verts, faces, cell, origin, *_ = MS.hand_made("tie_to_smaller_id")
    rep, _, d2 = MS.clusters(verts, cell, origin)
    assert d2[1] == d2[2] == np.float32(0.0625) and d2[0] > d2[1]
    assert rep[:3].tolist() == [1, 1, 1]
    # the same vertices in another order: the tie goes to whichever comes first, a strictly nearer one wins whatever its id
    rep, _, _ = MS.clusters(verts[[2, 1, 0, 3, 4, 5]], cell, origin)
    assert rep[:3].tolist() == [0, 0, 0]
    verts[0, 0] = 0.5
    rep, _, _ = MS.clusters(verts[[2, 1, 0, 3, 4, 5]], cell, origin)
    assert rep[:3].tolist() == [2, 2, 2]


def test_nan_inf_and_out_of_range_vertices_stay_singletons():
    verts, faces, cell, origin, *_ = MS.hand_made("singletons")
    rep, single, _ = MS.clusters(verts, cell, origin)
    assert single.tolist() == [True] * 6 + [False] * 2 and rep.tolist() == list(range(8))
    # the range is [-2^20, 2^20) cells: the last cell inside and the first outside, on both sides
    edge = np.array([[1048575.5, 0, 0], [1048575.25, 0, 0], [1048576.0, 0, 0], [-1048576.0, 0, 0], [-1048575.5, 0, 0], [-1048576.5, 0, 0]], np.float32)
    rep, single, _ = MS.clusters(edge, 1.0)
    assert single.tolist() == [False, False, True, False, False, True] and rep.tolist() == [0, 0, 2, 4, 4, 5]


def test_mirror_faces_keep_the_first_and_its_winding():
    verts, faces, cell, origin, *_ = MS.hand_made("mirror_pair")
    out = MS.simplify(verts, None, None, faces, cell, origin)
    assert out[1] is None and out[2] is None and out[3].tolist() == [[1, 2, 0]]
    out = MS.simplify(verts, None, None, faces[::-1], cell, origin)
    assert out[3].tolist() == [[2, 1, 0]]   # (2, 1, 5) comes first now: clusters (2, 1, 0)


def test_a_fan_whose_rim_falls_into_one_cell_collapses_to_nothing():
    verts, faces, cell, origin, *_ = MS.hand_made("fan_collapses")
    v, n, c, f, m = MS.simplify(verts, verts, None, faces, cell, origin)
    assert v.shape == (0, 3) and n.shape == (0, 3) and c is None and f.shape == (0, 3) and (m == MS.DROPPED).all()


def test_a_small_cell_returns_the_input_bit_for_bit():
    verts, faces, cell, origin, *_ = MS.hand_made("identity")
    out = MS.simplify(verts, -verts, None, faces, cell, origin)
    assert MS.is_identity(verts, faces, out) and np.array_equal(out[1], -verts) and out[4].tolist() == [0, 1, 2, 3]
    # ... and a vertex no face refers to is dropped all the same: that is not the identity
    more = np.concatenate([verts, [[9, 9, 9]]]).astype(np.float32)
    out = MS.simplify(more, None, None, faces, cell, origin)
    assert len(out[0]) == 4 and out[4].tolist() == [0, 1, 2, 3, MS.DROPPED]


def test_random_meshes_have_the_outputs_properties():
    for n, t, cells, seed in ((255, 400, 5, 1), (256, 400, 5, 2), (257, 400, 5, 3)):
        verts, faces, cell = MS.random_mesh(n, t, cells, seed)
        out = MS.simplify(verts, None, None, faces, cell)
        assert 0 < len(out[3]) < t and len(out[0]) <= cells ** 3 and MS.properties(out)
        # idempotent: the representatives are one per cell already, and no face repeats
        again = MS.simplify(out[0], None, None, out[3], cell)
        assert MS.is_identity(out[0], out[3], again)
