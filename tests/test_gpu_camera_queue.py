"""The fused path kernel's camera queue (kernels.h, k_path_small): a wave starts 64 units' camera rays at full width ahead of
need, and a lane whose sample ended takes a finished camera hit from the wave's ring of 128 entries.  Which lane runs a sample
must not show: every case renders with the default (fused) kernel and with the per-slot wavefront kernel and compares bytes,
at the unit counts where the ring's bookkeeping changes path (one unit, one refill more or less, a wrap of the ring, waves
that get nothing) and where a lane takes more than one entry in an iteration (camera rays that end their sample at once)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    return HipScene, LoadedScene


def _pair(libs, scene_path, width, height, count=False):
    HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, width, height)
    fused = HipScene(scene.desc, device=0)
    per_slot = HipScene(scene.desc, device=0, shade_kernel="per-slot")
    for gpu in (fused, per_slot):
        if count:
            gpu.set_stats_mode(count=True)
            gpu.reset_stats()
    return scene, fused, per_slot


def _same(fused, per_slot, seed, spp, start_bounce, last_bounce):
    a = fused.render(seed, 0, spp, start_bounce, last_bounce)
    b = per_slot.render(seed, 0, spp, start_bounce, last_bounce)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)
    assert fused.stats()["dropped_samples"] == per_slot.stats()["dropped_samples"]
    assert fused.stats()["camera_samples"] == per_slot.stats()["camera_samples"]
    return a


# units = width x height x spp (one sample per unit)
@pytest.mark.parametrize("width,height,spp", [
    (1, 1, 1),                                   # 1
    (3, 3, 7), (8, 8, 1), (13, 5, 1),            # 63, 64, 65: one refill, full or ragged, and the first unit of a second
    (127, 1, 1), (8, 8, 2), (43, 3, 1),          # 127, 128, 129: the ring's capacity
    (1, 1, 200),                                 # one pixel through several refills of one wave
    (512, 512, 1),                               # about a unit per resident lane: waves that get nothing or a ragged batch
    (256, 256, 16),                              # many refills per wave, the ring wraps
])
def test_unit_counts_around_the_edges_of_the_queue(libs, width, height, spp):
    _, fused, per_slot = _pair(libs, "scenes/cornell.json", width, height)
    image = _same(fused, per_slot, 5, spp, 0, 10)
    assert image.shape == (height, width, 3)
    if width * height * spp >= 64:
        assert image.sum() > 0.0


@pytest.mark.parametrize("start_bounce,last_bounce", [(0, 0), (2, 3)])
def test_samples_that_end_at_their_first_vertices(libs, start_bounce, last_bounce):
    _, fused, per_slot = _pair(libs, "scenes/cornell.json", 40, 24)
    _same(fused, per_slot, 9, 6, start_bounce, last_bounce)


def test_camera_rays_that_miss_take_entry_after_entry(libs):
    _, fused, per_slot = _pair(libs, "test_scenes/environment_map_sampling.json", 24, 24)
    image = _same(fused, per_slot, 4, 12, 0, 10)
    assert image.sum() > 0.0


def test_spheres_in_the_refill(libs):
    _, fused, per_slot = _pair(libs, "scenes/mis-pbrt.json", 32, 24)
    _same(fused, per_slot, 2, 4, 0, 10)


@pytest.mark.parametrize("per_unit,spp", [(3, 7), (4, 24)])
def test_units_of_several_samples(libs, per_unit, spp):
    _, fused, per_slot = _pair(libs, "scenes/cornell.json", 24, 16)
    fused.set_samples_per_unit(per_unit)
    per_slot.set_samples_per_unit(per_unit)
    whole = _same(fused, per_slot, 7, spp, 0, 10)
    # the same sum when the call is split on a unit boundary (continued on the device: the host entry point adds a call's own
    # sum to the caller's array, which is another order of additions)
    import torch
    first = per_unit * (spp // per_unit // 2 + 1)
    split = torch.zeros((16, 24, 3), dtype=torch.float32, device="cuda")
    fused.render_device(7, 0, first, 0, 10, split.data_ptr())
    fused.render_device(7, first, spp - first, 0, 10, split.data_ptr())
    assert np.array_equal(split.cpu().numpy(), whole)


def test_the_same_call_twice_gives_the_same_bytes(libs):
    HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 96, 64)
    gpu = HipScene(scene.desc, device=0)
    first = gpu.render(3, 0, 8, 0, 10)
    assert np.array_equal(gpu.render(3, 0, 8, 0, 10), first)
    assert np.array_equal(HipScene(scene.desc, device=0).render(3, 0, 8, 0, 10), first)


# scene kinds whose counting instantiation is the fused kernel's own: Lambertian triangles, Lambertian / plastic / spheres, any BSDF
@pytest.mark.parametrize("scene_path", ["scenes/cornell.json", "scenes/mis-pbrt.json", "scenes/cornell-glass.json"])
def test_counting_renders_count_what_the_per_slot_path_counts(libs, scene_path):
    _, fused, per_slot = _pair(libs, scene_path, 32, 24, count=True)
    _same(fused, per_slot, 6, 4, 0, 10)
    a, b = fused.stats(), per_slot.stats()
    print({name: (a[name], b[name]) for name in ("closest_rays", "shadow_rays", "tris_tested")})
    assert a["closest_rays"] == b["closest_rays"]
    assert a["shadow_rays"] == b["shadow_rays"]
    assert a["tris_tested"] == b["tris_tested"]
