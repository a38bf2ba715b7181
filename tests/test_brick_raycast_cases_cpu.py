"""The scenes of the brick ray-cast's GPU test (brick_raycast_cases.py), on the CPU oracle: the conditions that keep a bit-for-bit
comparison from passing vacuously.  The dense comparator on each case's own brick list hits on at least 15 % of the pixels and misses
on at least 15 %; with the drop rule it differs from the all-bricks rendering on at least 10 % of them; and the counts are the ones
the cases module records.  No GPU."""
import numpy as np
import pytest

import brick_raycast_cases as BC
import kfx_testlib as T  # noqa: F401  (the path of the oracle)
from kfx_testlib import oracle


def floors(hits, pixels):
    return hits >= BC.HIT_FLOOR * pixels and pixels - hits >= BC.MISS_FLOOR * pixels


@pytest.mark.parametrize("case", ["A", "A2", "B", "C", "D"])
def test_the_dropped_bricks_change_the_rendering_and_both_renderings_hit_and_miss(case):
    c = BC.CASES[case]
    vol = BC.oracle_volume(oracle, case)
    nb = int(np.prod(BC.brick_grid(c["dims"])))
    ids = np.arange(nb, dtype=np.uint32)   # every brick of these volumes differs from the fill cell
    drop = BC.drop5(ids, c["dims"])
    assert (int(drop.sum()), nb) == c["dropped"]
    full = BC.oracle_render(oracle, case, BC.oracle_dense(oracle, case, vol, ids))
    assert np.array_equal(full[0], BC.oracle_render(oracle, case, vol)[0], equal_nan=True)   # (D with every brick is the volume)
    part = BC.oracle_render(oracle, case, BC.oracle_dense(oracle, case, vol, ids[~drop]))
    pixels = c["size"][0] * c["size"][1]
    differ = BC.differing_pixels(full, part)
    print("case %s: %d / %d hits of %d pixels, %d differ" % (case, full[3]["hits"], part[3]["hits"], pixels, differ))
    assert floors(full[3]["hits"], pixels) and floors(part[3]["hits"], pixels)
    assert differ >= BC.DIFFER_FLOOR * pixels
    assert (full[3]["hits"], part[3]["hits"], differ) == c["counts"]
    assert full[3]["hits"] == int(np.count_nonzero(full[0] > 0)) and part[3]["hits"] == int(np.count_nonzero(part[0] > 0))
    if c.get("nan7"):
        assert np.isnan(vol.data[..., 0]).sum() > 0.1 * vol.data[..., 0].size


def test_the_shell_keeps_every_hit_and_marches_mostly_through_absent_bricks():
    c = BC.CASES["S"]
    vol = BC.oracle_volume(oracle, "S")
    keep = BC.shell_keep(vol.data[..., 0], c["dims"])
    assert (len(keep), int(np.prod(BC.brick_grid(c["dims"])))) == c["kept"]
    full = BC.oracle_render(oracle, "S", vol)
    shell = BC.oracle_render(oracle, "S", BC.oracle_dense(oracle, "S", vol, keep))
    pixels = c["size"][0] * c["size"][1]
    print("case S: %d / %d hits of %d pixels, %d / %d steps" % (full[3]["hits"], shell[3]["hits"], pixels, full[3]["steps"], shell[3]["steps"]))
    assert floors(shell[3]["hits"], pixels)
    assert (full[3]["hits"], shell[3]["hits"]) == c["counts"][:2]
    # a NaN sample steps by trunc where the free-space sample it replaces steps by its value: more steps, the same hits
    assert (round(full[3]["steps"] / 1000), round(shell[3]["steps"] / 1000)) == c["steps_k"]
    assert np.array_equal(full[0] > 0, shell[0] > 0)
