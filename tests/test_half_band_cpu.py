"""KFX_SUMMARY_HALF_BAND (include/kfx_summary_h.h) against the CPU oracle's half fuse: over an orbit of the room and of the
full scene, every free-space cell of a half-cell volume (trunc in the fp32 volume fused from the same frames) stays within
the band of vref = (half) trunc_dist -- what the fast-numerics class tables of a half summary rely on.  No GPU."""
import importlib.util
import os

import kfx_testlib as T


def _band_module():
    spec = importlib.util.spec_from_file_location("half_free_band", os.path.join(T.ROOT, "scripts", "half_free_band.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_half_free_space_stays_inside_the_documented_band():
    m = _band_module()
    band = m.library_band()
    assert 0.0 < band < 0.25
    for scene in ("room", "full"):
        r = m.simulate(scene, 32, 120, w=80, h=60, orbit=60, every=40)
        assert r["checkpoints"][-1]["free"] > 1000, r
        assert 0.0 < r["max_rel"] <= band, (scene, r["max_rel"], band)   # the half running average does drift; the band covers it
