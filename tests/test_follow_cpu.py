"""follow_shift (kangaroo_amd/pipeline.py, also roo.follow_shift): the whole-cell shift that lets the volume's box follow the camera,
on hand-computed cases.  The box (-1, -1, 2) - (1, 1, 4) with 33 voxels per axis has a voxel size of 1/16 and its centre at (0, 0, 3),
so every offset below is exact in float64: o = 16 * (target - centre)."""
import numpy as np
import pytest

from kangaroo_amd.pipeline import FramePipeline, SlabPipeline, TrackingSlabPipeline, follow_shift

LO, HI, DIMS = (-1.0, -1.0, 2.0), (1.0, 1.0, 4.0), (33, 33, 33)


def pose(centre, R=None):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) if R is None else R
    T[:, 3] = centre
    return T


# the camera's +z axis along the world's +x: a quarter turn about y
TURNED = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])


def test_the_target_at_the_box_centre_asks_for_nothing():
    assert follow_shift(LO, HI, DIMS, pose((0, 0, 0)), 3.0) == (0, 0, 0)
    assert follow_shift(LO, HI, DIMS, pose((-3, 0, 3), TURNED), 3.0) == (0, 0, 0)


def test_inside_the_slack_nothing_moves():
    # o = (14.4, -15.9375, 15.2): all below the slack of 16
    assert follow_shift(LO, HI, DIMS, pose((0.9, -0.99609375, 0.95)), 3.0) == (0, 0, 0)
    # |o| = 16 is no longer inside
    assert follow_shift(LO, HI, DIMS, pose((1.0, 0, 0)), 3.0) == (16, 0, 0)


def test_beyond_the_slack_the_shift_is_the_nearest_multiple_of_the_quantum():
    # o = 20.8 -> 8 * rint(2.6) = 24;  o = 18 with quantum 4 -> 4 * rint(4.5) = 16 (tie to even);  o = 35.2 -> 32
    assert follow_shift(LO, HI, DIMS, pose((1.3, 0, 0)), 3.0) == (24, 0, 0)
    assert follow_shift(LO, HI, DIMS, pose((0, 0, 2.2)), 3.0) == (0, 0, 32)
    assert follow_shift(LO, HI, DIMS, pose((1.125, 0, 0)), 3.0, quantum=4) == (16, 0, 0)


def test_a_tie_at_half_a_quantum_goes_to_the_even_multiple():
    # o = 20 = 2.5 quanta -> 2 quanta;  o = 28 = 3.5 quanta -> 4 quanta; the same below zero
    assert follow_shift(LO, HI, DIMS, pose((1.25, 1.75, 0)), 3.0) == (16, 32, 0)
    assert follow_shift(LO, HI, DIMS, pose((-1.25, -1.75, 0)), 3.0) == (-16, -32, 0)


def test_negative_offsets():
    # o = (-20.8, -17.6, -24) -> (-24, -16, -24)
    assert follow_shift(LO, HI, DIMS, pose((-1.3, -1.1, -1.5)), 3.0) == (-24, -16, -24)
    # slack 8, quantum 4: o = (-9.6, 6.4, -8) -> (-8, 0, -8)
    assert follow_shift(LO, HI, DIMS, pose((-0.6, 0.4, -0.5)), 3.0, quantum=4, slack=8) == (-8, 0, -8)


def test_a_rotated_camera_moves_the_target_along_its_own_axis():
    # the camera at (-1.5, 0.6, 3) looks along +x: target = (1.5, 0.6, 3), o = (24, 9.6, 0)
    assert follow_shift(LO, HI, DIMS, pose((-1.5, 0.6, 3), TURNED), 3.0) == (24, 0, 0)
    assert follow_shift(LO, HI, DIMS, pose((-1.5, 0.6, 3), TURNED), 3.0, quantum=4, slack=8) == (24, 8, 0)
    # a longer focus pushes the target further along that axis only: focus 4 -> o = (40, 9.6, 0)
    assert follow_shift(LO, HI, DIMS, pose((-1.5, 0.6, 3), TURNED), 4.0) == (40, 0, 0)
    # a 4 x 4 pose and float32 boxes are taken as well
    T4 = np.vstack([pose((-1.5, 0.6, 3), TURNED), [0, 0, 0, 1]])
    assert follow_shift(np.float32(LO), np.float32(HI), DIMS, T4, 3.0) == (24, 0, 0)
    # anisotropic voxels: 17 voxels along y are 1/8 apart -> o_y = 8 * 1.25 = 10
    assert follow_shift(LO, HI, (33, 17, 33), pose((0, 1.25, 0)), 3.0, quantum=2, slack=4) == (0, 10, 0)


def test_the_result_is_python_ints():
    s = follow_shift(LO, HI, DIMS, pose((1.3, 0, 0)), 3.0)
    assert all(type(v) is int for v in s)


class _Dist:
    def get_rank(self):
        return 0

    def get_world_size(self):
        return 1


@pytest.mark.parametrize("cls", [SlabPipeline, TrackingSlabPipeline])
def test_slab_pipelines_refuse_follow_and_say_why(cls):
    with pytest.raises(ValueError, match="follow=.*z.*rank"):
        cls(None, _Dist(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=8, slack=8))


def test_frame_pipeline_refuses_follow_without_the_operator():
    class Ops:
        pass
    with pytest.raises(ValueError, match="follow=.*VolumeShift"):
        FramePipeline(Ops(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=8))
