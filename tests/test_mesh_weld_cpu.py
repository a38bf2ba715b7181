"""tests/mesh_weld.py -- the CPU construction of the expected indexed mesh (include/kfx_mesh_index.h) -- checked on its own, against
the oracle's marching cubes and without the library: on a sphere and on a ragged volume with a lattice of unobserved cells,
  * V equals the number of lattice edges with finite endpoints of different sign next to an all-finite cube (no case tables),
  * the sphere's faces are closed with Euler characteristic 2 as they stand (no KD-tree weld),
  * de-indexing gives the soup back to within 4 ulp of M, M the largest |box coordinate|: the copies of a vertex are two evaluations
    of the same real point, at most four roundings each at magnitude <= M.

Measured with the oracle: sphere 32^3 V = 2212, T = 4420, copies within 5.96e-8 = 0.5 ulp of M = 1; ragged 21x13x34 V = 828,
T = 983, copies within 1.19e-7 = 1 ulp of M = 1.5, normals of copies differing by up to 1.0."""
import functools

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_weld as W
import test_mesh_cpu as TM


def ragged_volume():
    """the ragged_unobserved recipe of test_gpu_mesh_volumes.py"""
    ovol = oracle.Volume(21, 13, 34, (-1, -0.5, -1), (1, 0.7, 1.5), pitch_bytes=21 * 8 + 40)
    oracle.sdf_sphere(ovol, (0.1, 0.0, 0.2), 0.45)
    ovol.data[:, :, :, 0][(np.add.outer(np.add.outer(np.arange(34), np.arange(13)), np.arange(21)) % 7) == 0] = np.nan
    return ovol


CASES = {"sphere_32": (lambda: TM.sphere_volume(32, 0.7), 2212, 4420), "ragged_unobserved": (ragged_volume, 828, 983)}


@functools.lru_cache(maxsize=None)
def welded(name):
    make, V, Tn = CASES[name]
    ovol = make()
    sv, sn, _ = oracle.marching_cubes(ovol, None, *TM.tables())
    return ovol, sv, sn, W.weld(ovol, sv, sn), V, Tn


@pytest.mark.parametrize("name", sorted(CASES))
def test_weld_has_one_vertex_per_crossed_lattice_edge(name):
    ovol, sv, sn, (v, n, c, f), V, Tn = welded(name)
    assert c is None and f.dtype == np.uint32 and f.shape == (len(sv) // 3, 3)
    assert len(v) == len(n) == V and len(f) == Tn, (len(v), len(f))
    assert len(v) == W.count_lattice_edges(ovol)
    assert f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    # ids in first-occurrence order: the running maximum of the flattened faces grows by at most one
    flat = f.reshape(-1).astype(np.int64)
    run = np.maximum.accumulate(flat)
    assert flat[0] == 0 and (np.diff(run) <= 1).all()
    # first occurrences carry the soup's values bit for bit
    firsts = np.r_[0, np.flatnonzero(np.diff(run) > 0) + 1]
    assert T.nan_equal(v, sv[firsts]) and T.nan_equal(n, sn[firsts])


def test_welded_sphere_is_closed():
    ovol, sv, sn, (v, n, c, f), V, Tn = welded("sphere_32")
    assert len(v) == len(f) // 2 + 2
    assert W.closed_with_euler_2(f, len(v))


@pytest.mark.parametrize("name", sorted(CASES))
def test_deindexed_weld_is_the_soup_within_4_ulp(name):
    ovol, sv, sn, (v, n, c, f), V, Tn = welded(name)
    M = max(abs(float(x)) for x in tuple(ovol.boxmin) + tuple(ovol.boxmax))
    err = float(np.abs(v[f.reshape(-1)].astype(np.float64) - sv.astype(np.float64)).max())
    print("%s: copies within %.3g = %.2f ulp of M = %g; normals within %.3g" %
          (name, err, err / W.ulp(M), M, float(np.abs(n[f.reshape(-1)] - sn).max())))
    assert err <= 4 * W.ulp(M)
