"""The single-sample variant of the fused path kernel (kernels.h: pathSmall<.., SINGLE>, k_path_small_single): the launch of a
Cornell-like scene whose units are one sample each.  It carries no pixel, sample range or partial sum, ends a camera ray that
leaves the scene in the refill and hands a finished lane its next camera hit in straight-line code.  Nothing of that may
show: every case renders with four builds of the same scene and compares bytes --
  the default (k_path_small_single),
  the counting instantiation (k_path_small<.., COUNT>: every turn of phase 1, the refill's own pass over the items),
  the per-slot wavefront kernels,
  the default with set_samples_per_unit(3), which runs k_path_small (units of three samples: another order of additions
  inside a unit, so it is compared with the per-slot path at the same setting) --
and again after set_camera."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CORNELL = "scenes/cornell.json"


@pytest.fixture(scope="module")
def libs():
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    return HipScene, LoadedScene


class Builds:
    def __init__(self, libs, width, height, camera=None):
        HipScene, LoadedScene = libs
        self.scene = LoadedScene(CORNELL, width, height)
        if camera is not None:
            self.scene.desc.contents.camera = camera(self.scene.desc.contents.camera)
        desc = self.scene.desc
        self.single = HipScene(desc, device=0)
        self.counting = HipScene(desc, device=0)
        self.counting.set_stats_mode(count=True)
        self.per_slot = HipScene(desc, device=0, shade_kernel="per-slot")
        self.units_of_three = HipScene(desc, device=0)
        self.units_of_three.set_samples_per_unit(3)
        self.per_slot_of_three = HipScene(desc, device=0, shade_kernel="per-slot")
        self.per_slot_of_three.set_samples_per_unit(3)

    def everyone(self):
        return (self.single, self.counting, self.per_slot, self.units_of_three, self.per_slot_of_three)

    def same(self, seed, begin, count, start_bounce, last_bounce):
        image = self.single.render(seed, begin, count, start_bounce, last_bounce)
        assert np.isfinite(image).all()
        assert np.array_equal(self.counting.render(seed, begin, count, start_bounce, last_bounce), image)
        assert np.array_equal(self.per_slot.render(seed, begin, count, start_bounce, last_bounce), image)
        three = self.units_of_three.render(seed, begin, count, start_bounce, last_bounce)
        assert np.array_equal(self.per_slot_of_three.render(seed, begin, count, start_bounce, last_bounce), three)
        # Units of three add ((0 + a) + b) + c before the resolve adds the unit: the same samples in another order of additions.
        # Both are sums of `count` non-negative floats, each within (count - 1) * 2^-24 of the exact sum, relatively.
        np.testing.assert_allclose(three, image, rtol=2.1 * count * 2.0 ** -24, atol=0.0)
        dropped = {gpu.stats()["dropped_samples"] for gpu in self.everyone()}
        assert len(dropped) == 1, dropped
        return image

    def set_camera(self, camera):
        for gpu in self.everyone():
            gpu.set_camera(camera)


def _moved(camera):
    moved = copy.copy(camera)
    moved.origin = (C.c_float * 3)(camera.origin[0] + 0.35, camera.origin[1] - 0.2, camera.origin[2] * 0.8)
    return moved


def _wide(camera):
    """The reference view with twice the field of view: the room covers about a quarter of the frame."""
    wide = copy.copy(camera)
    wide.vertical_fov = 2.0 * camera.vertical_fov
    return wide


def _with_moved_camera(builds, seed, begin, count, start_bounce, last_bounce, first):
    original = copy.copy(builds.scene.desc.contents.camera)
    builds.set_camera(_moved(original))
    after = builds.same(seed, begin, count, start_bounce, last_bounce)
    assert not np.array_equal(after, first)
    builds.set_camera(original)
    assert np.array_equal(builds.same(seed, begin, count, start_bounce, last_bounce), first)


def test_cornell(libs):
    builds = Builds(libs, 48, 32)
    first = builds.same(5, 0, 16, 0, 10)
    assert first.sum() > 0.0
    _with_moved_camera(builds, 5, 0, 16, 0, 10, first)


# few pixels, many samples: the 64 units a wave grabs span several sample indices, so the lanes of a wave hold different
# second keys of the random stream
@pytest.mark.parametrize("width,height,spp", [(7, 5, 64), (1, 1, 64), (1, 1, 1024)])
def test_a_grab_spans_several_sample_indices(libs, width, height, spp):
    builds = Builds(libs, width, height)
    first = builds.same(11, 0, spp, 0, 10)
    assert first.sum() > 0.0
    _with_moved_camera(builds, 11, 0, spp, 0, 10, first)


def test_camera_rays_that_leave_the_scene_end_in_the_refill(libs):
    builds = Builds(libs, 40, 40, camera=_wide)
    spp = 8
    first = builds.same(3, 0, spp, 0, 10)
    assert first.sum() > 0.0
    # The share of camera rays that miss, from the counting statistics.  In the bounce window (0, 1) a camera hit traces exactly
    # one more closest-hit ray unless it lies on an emitter (seen from the front here: the view looks into the room), and a
    # pixel with an emitter hit is non-zero in the window (0, 0), which adds the first hit's emission and nothing else:
    #   misses >= samples - (closest rays - samples) - spp * (pixels lit in the window (0, 0))
    builds.counting.reset_stats()
    builds.counting.render(3, 0, spp, 0, 1)
    stats = builds.counting.stats()
    samples, closest = stats["camera_samples"], stats["closest_rays"]
    assert samples == 40 * 40 * spp
    lit = int(np.count_nonzero(builds.single.render(3, 0, spp, 0, 0).any(axis=2)))
    misses = samples - (closest - samples) - spp * lit
    print("camera samples %d, closest rays %d, lit pixels %d: at least %d camera rays miss (%.3f)" % (samples, closest, lit, misses, misses / samples))
    assert misses >= 0.2 * samples
    # ... and a pixel all of whose camera rays miss is exactly zero
    assert np.count_nonzero(~first.any(axis=2)) >= 0.2 * 40 * 40
    _with_moved_camera(builds, 3, 0, spp, 0, 10, first)


# the first vertices end the sample; vertices beyond any per-vertex table of twelve
@pytest.mark.parametrize("start_bounce,last_bounce", [(0, 0), (0, 1), (1, 1), (0, 14), (3, 14)])
def test_bounce_windows(libs, start_bounce, last_bounce):
    builds = Builds(libs, 24, 16)
    first = builds.same(9, 0, 6, start_bounce, last_bounce)
    _with_moved_camera(builds, 9, 0, 6, start_bounce, last_bounce, first)


# the corners of the random stream: upper seed bits, and the last sample indices a call may name (a call is refused once
# spp_begin + spp_count exceeds 2^31 - 1, include/pathed_hip.h: no call reaches an index of 2^31)
@pytest.mark.parametrize("seed,begin,count", [
    (0xDEADBEEF00000005, 0, 6), (5, (1 << 31) - 9, 8), ((1 << 64) - 1, (1 << 31) - 9, 8), ((1 << 32) | 1, (1 << 24) - 3, 7),
])
def test_seeds_and_sample_indices_at_the_corners(libs, seed, begin, count):
    builds = Builds(libs, 24, 16)
    first = builds.same(seed, begin, count, 0, 10)
    assert first.sum() > 0.0
    if seed >> 32:   # the upper half is part of the key
        assert not np.array_equal(first, builds.single.render(seed & 0xFFFFFFFF, begin, count, 0, 10))


def test_two_calls_are_one(libs):
    import torch
    builds = Builds(libs, 48, 32)
    whole = torch.zeros((32, 48, 3), dtype=torch.float32, device="cuda")
    builds.single.render_device(7, 0, 16, 0, 10, whole.data_ptr())
    for gpu in (builds.single, builds.counting, builds.per_slot):
        split = torch.zeros((32, 48, 3), dtype=torch.float32, device="cuda")
        gpu.render_device(7, 0, 5, 0, 10, split.data_ptr())
        gpu.render_device(7, 5, 11, 0, 10, split.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(split, whole)
