"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs, against the committed image fixtures, and — at the headline resolution — through
size-independent properties (batch continuation, bounce-window additivity, energy).

Tolerances: the intersector is bit-exact by specification; rendered images differ
from the oracle only through ocml-vs-glibc sinf/cosf/logf/expf/acosf/atan2f ULPs and the rare
hit/miss flip they cause: image relL2 <= 2e-3 and <= 0.1 % of pixels off by > 1 % (glass: 1e-2).
Measured values are ~1e-8..4e-5; the test bounds are the stated contract, not the observation.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURES = os.path.join(os.path.dirname(__file__), "golden", "images.npz")


@pytest.fixture(scope="module")
def libs():
    import oracle_lib
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    return oracle_lib, HipScene, LoadedScene


def _rays(n, seed, centre, extent, tnear=1e-3, tfar=1e5):
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.uniform(-extent, extent, (n, 3)) + np.asarray(centre)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 4:7] = d
    rays[:, 3] = tnear
    rays[:, 7] = tfar
    return rays


def _image_metrics(gpu, cpu):
    rel = float(np.linalg.norm(gpu - cpu) / max(np.linalg.norm(cpu), 1e-30))
    bad = float((np.abs(gpu - cpu) > 1e-2 * np.maximum(np.abs(cpu), 1e-3)).any(axis=2).mean())
    return rel, bad


SCENES = [
    ("scenes/cornell.json", (0, 1, 0), 1.0),
    ("scenes/cornell-glossy.json", (0, 1, 0), 1.0),
    ("scenes/mis-pbrt.json", (0, -1, 2), 6.0),
    ("scenes/teapot.json", (0, 4, 0), 9.0),
]


@pytest.mark.parametrize("scene_path,centre,extent", SCENES)
def test_intersector_is_bit_exact(libs, scene_path, centre, extent):
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, 32, 32)
    gpu, cpu = HipScene(scene.desc, device=0), oracle_lib.OracleScene(scene.desc)
    rays = _rays(50000, 3, centre, extent)
    # axis-parallel and zero-component directions, short and offset intervals
    rays[:100, 4:7] = [0, 0, -1]
    rays[100:200, 4:7] = [1, 0, 0]
    rays[200:300, 4:7] = [0, -1, 0]
    rays[300:2000, 7] = 0.75
    rays[2000:4000, 3] = 0.4
    hits_gpu, hits_cpu = gpu.trace(rays), cpu.trace(rays)
    assert np.array_equal(hits_gpu.view(np.int32), hits_cpu.view(np.int32))
    assert (hits_gpu[:, 3].view(np.int32) >= 0).mean() > 0.2
    assert np.array_equal(gpu.trace(rays, any_hit=True), cpu.trace(rays, any_hit=True))


def test_empty_and_ragged_inputs(libs):
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 17, 5)  # ragged: 85 slots, not a multiple of 64
    gpu, cpu = HipScene(scene.desc, device=0), oracle_lib.OracleScene(scene.desc)
    assert gpu.trace(np.zeros((0, 8), dtype=np.float32)).shape == (0, 4)
    one = _rays(1, 1, (0, 1, 0), 0.5)
    assert np.array_equal(gpu.trace(one).view(np.int32), cpu.trace(one).view(np.int32))
    image = gpu.render(3, 0, 0, 0, 10)  # zero samples: nothing is added
    assert not image.any()
    image = gpu.render(3, 5, 3, 0, 10)
    expected, _ = cpu.render(17, 5, 3, 5, 3, 0, 10)
    rel, bad = _image_metrics(image, expected)
    assert rel < 2e-3 and bad <= 0.012  # 1 of 85 pixels


def test_scene_without_geometry_or_lights(libs):
    oracle_lib, HipScene, _ = libs
    from scene_builder import BuiltScene
    built = BuiltScene(8, 8, (0, 0, 5), (0, 0, 0))
    built.material()
    desc = built.finish()
    gpu = HipScene(desc, device=0)
    assert not gpu.render(1, 0, 2, 0, 4).any()
    lit = BuiltScene(8, 8, (0, 0, 5), (0, 0, 0))
    lit.quad([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], lit.material(diffuse=(.5, .5, .5)))
    desc = lit.finish()
    assert not HipScene(desc, device=0).render(1, 0, 2, 0, 4).any()  # no lights, no env: black


CASES = {
    "cornell_32": ("scenes/cornell.json", 32, 32, 1, 0, 4, 0, 10, 2e-3),
    "cornell_window_2_3": ("scenes/cornell.json", 24, 24, 5, 3, 3, 2, 3, 2e-3),
    "cornell_glass_24": ("scenes/cornell-glass.json", 24, 24, 2, 0, 4, 0, 6, 1e-2),
    "cornell_glossy_24": ("scenes/cornell-glossy.json", 24, 24, 2, 0, 4, 0, 6, 1e-2),
    "oren_nayar_24": ("scenes/cornell-oren-nayar.json", 24, 24, 3, 0, 4, 0, 5, 2e-3),
    "ggx_24": ("scenes/cornell-ggx.json", 24, 24, 8, 0, 4, 0, 5, 2e-3),
    "mis_32x24": ("scenes/mis-pbrt.json", 32, 24, 4, 0, 4, 0, 4, 2e-3),
    "teapot_32x24": ("scenes/teapot.json", 32, 24, 6, 0, 3, 0, 8, 1e-2),
    "env_sampling_24": ("test_scenes/environment_map_sampling.json", 24, 24, 7, 0, 8, 0, 3, 2e-3),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_matches_committed_fixture_and_oracle(libs, name):
    oracle_lib, HipScene, LoadedScene = libs
    path, w, h, seed, begin, count, sb, lb, tolerance = CASES[name]
    scene = LoadedScene(path, w, h)
    gpu = HipScene(scene.desc, device=0)
    image = gpu.render(seed, begin, count, sb, lb)
    fixture = np.load(FIXTURES)[name]
    rel, bad = _image_metrics(image, fixture)
    assert rel <= tolerance, (name, rel)
    assert bad <= max(1e-3, 1.5 / (w * h)), (name, bad)
    live, _ = oracle_lib.OracleScene(scene.desc).render(w, h, seed, begin, count, sb, lb)
    assert np.array_equal(live, fixture), "the oracle no longer reproduces its committed fixture"
    assert gpu.stats()["dropped_samples"] == 0


@pytest.mark.parametrize("scene_path,size,spp,tolerance", [
    ("scenes/cornell.json", 128, 16, 2e-3),
    ("scenes/mis-pbrt.json", 96, 16, 2e-3),
    ("scenes/cornell-oren-nayar.json", 96, 8, 2e-3),
    ("scenes/teapot.json", 96, 8, 1e-2),
])
def test_render_parity_at_test_size(libs, scene_path, size, spp, tolerance):
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, size, size)
    gpu = HipScene(scene.desc, device=0)
    image = gpu.render(1, 0, spp, 0, 10)
    expected, _ = oracle_lib.OracleScene(scene.desc).render(size, size, 1, 0, spp, 0, 10, threads=os.cpu_count())
    rel, bad = _image_metrics(image, expected)
    assert rel <= tolerance and bad <= 1e-3, (scene_path, rel, bad)


def test_batches_continue_the_sum_bit_exactly(libs):
    import torch
    _, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 64, 64)
    gpu = HipScene(scene.desc, device=0)
    # samples-per-unit 1 (the default): the reference's exact per-sample order, any split is bit-identical
    gpu.set_samples_per_unit(1)
    once = torch.zeros((64, 64, 3), dtype=torch.float32, device="cuda")
    gpu.render_device(4, 0, 12, 0, 10, once.data_ptr())
    split = torch.zeros_like(once)
    for begin, count in ((0, 5), (5, 1), (6, 6)):
        gpu.render_device(4, begin, count, 0, 10, split.data_ptr())
    assert torch.equal(once, split)
    # coarser units (4 samples): splits on unit boundaries are bit-identical, and the result is
    # deterministic although slots pull work dynamically (no float atomics anywhere)
    gpu.set_samples_per_unit(4)
    once = torch.zeros_like(once)
    gpu.render_device(4, 0, 24, 0, 10, once.data_ptr())
    split = torch.zeros_like(once)
    for begin, count in ((0, 8), (8, 4), (12, 12)):
        gpu.render_device(4, begin, count, 0, 10, split.data_ptr())
    assert torch.equal(once, split)
    again = torch.zeros_like(once)
    gpu.render_device(4, 0, 24, 0, 10, again.data_ptr())
    assert torch.equal(once, again)


def test_summation_order_matches_the_oracle_bit_for_bit_on_transcendental_free_paths(libs):
    """Mirror scene, bounce window [0,0]+[1,1] through a mirror: no sinf/cosf/logf on the path, so
    GPU and oracle must agree to the last bit, including the unit-wise summation order."""
    oracle_lib, HipScene, _ = libs
    from scene_builder import BuiltScene
    from pathed_amd import _capi
    built = BuiltScene(40, 40, (0, 1, 4), (0, 1, 0), fov_degrees=40)
    mirror = built.material(type_=_capi.MAT_MIRROR)
    glass = built.material(type_=_capi.MAT_GLASS, ior=1.5)
    light = built.material(diffuse=(0, 0, 0), emit=(5, 4, 3))
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], mirror)
    built.quad([(-1, 0.5, -1), (1, 0.5, -1), (1, 2.5, -1), (-1, 2.5, -1)], glass)
    built.quad([(-3, 3, -3), (3, 3, -3), (3, 3, 3), (-3, 3, 3)], light)  # faces down
    desc = built.finish()
    gpu, cpu = HipScene(desc, device=0), oracle_lib.OracleScene(desc)
    # ... and seed 2^64 - 1 with samples 2^31 - 9 .. 2^31 - 2: the last unit ends on the last index a call may name
    for seed, begin in ((5, 0), ((1 << 64) - 1, (1 << 31) - 9)):
        for chunk in (1, 4):
            gpu.set_samples_per_unit(chunk)
            image = gpu.render(seed, begin, 8, 0, 6)
            expected, _ = cpu.render(40, 40, seed, begin, 8, 0, 6, chunk=chunk)
            assert image.any() and gpu.stats()["dropped_samples"] == 0
            assert np.array_equal(image.view(np.int32), expected.view(np.int32)), (seed, begin, chunk)


def test_stats_mode_counts_match_the_oracle(libs):
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 48, 48)
    gpu = HipScene(scene.desc, device=0)
    gpu.set_stats_mode(count=True)
    gpu.reset_stats()
    counted = gpu.render(2, 0, 4, 0, 10)
    stats = gpu.stats()
    gpu.set_stats_mode(count=False)
    plain = gpu.render(2, 0, 4, 0, 10)
    assert np.array_equal(counted, plain)  # counting does not change results
    _, cpu_stats = oracle_lib.OracleScene(scene.desc).render(48, 48, 2, 0, 4, 0, 10)
    assert stats["camera_samples"] == cpu_stats["camera_samples"] == 48 * 48 * 4
    # same estimator, same random stream: ray counts agree up to the rare decision flip
    assert abs(stats["closest_rays"] - cpu_stats["closest_rays"]) <= 0.002 * cpu_stats["closest_rays"]
    # the HIP path skips the occlusion query of a light sample that contributes exactly black either way;
    # the oracle asks like the reference does and counts the queries that matter separately
    assert cpu_stats["shadow_rays_needed"] < cpu_stats["shadow_rays"]
    assert abs(stats["shadow_rays"] - cpu_stats["shadow_rays_needed"]) <= 0.002 * cpu_stats["shadow_rays_needed"]
    # Cornell (36 triangles) takes the all-triangles kernel: no boxes, 36 tests per closest ray
    assert stats["tris_tested"] > 0
    if stats["scene_in_lds"] == 2:
        assert stats["nodes_visited"] == 0 and stats["tris_tested"] >= 36 * stats["closest_rays"]
    else:
        assert stats["nodes_visited"] > 0


def test_exported_bvh_is_the_tree_the_kernel_walks(libs):
    import ctypes as C
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell-glossy.json", 16, 16)
    gpu = HipScene(scene.desc, device=0)
    nodes, tris = gpu.export_bvh()
    assert tris.shape[0] == scene.n_triangles and nodes.shape[0] >= 1
    prims = np.sort(tris[:, 3].view(np.int32))
    assert np.array_equal(prims, np.arange(scene.n_triangles))  # a permutation of the input
    rays = _rays(2000, 9, (0, 1, 0), 1.0)
    counts = (C.c_uint64 * 2)()
    fp = C.POINTER(C.c_float)
    code = oracle_lib.load().oracle_count_exported_bvh(
        nodes.ctypes.data_as(fp), nodes.shape[0], tris.ctypes.data_as(fp), tris.shape[0],
        rays.ctypes.data_as(fp), rays.shape[0], 0, counts)
    assert code == 0 and counts[0] > rays.shape[0] and counts[1] > 0


def test_full_size_properties(libs):
    """BASELINE config 2 resolution (1024x1024): properties that need no CPU render."""
    import torch
    _, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 1024, 1024)
    gpu = HipScene(scene.desc, device=0)
    spp = 8
    full = torch.zeros((1024, 1024, 3), dtype=torch.float32, device="cuda")
    gpu.render_device(1, 0, spp, 0, 10, full.data_ptr())
    mean = (full / spp).mean(dim=(0, 1)).cpu().numpy()
    # energy of the reference's own ground truth tools/cornell-gt.exr: (0.190, 0.124, 0.036)
    assert np.allclose(mean, [0.190, 0.124, 0.0356], rtol=0.04)
    assert torch.isfinite(full).all() and (full >= 0).all()
    lower = torch.zeros_like(full)
    gpu.render_device(1, 0, spp, 0, 2, lower.data_ptr())
    upper = torch.zeros_like(full)
    gpu.render_device(1, 0, spp, 3, 10, upper.data_ptr())
    # paths are built identically whatever the window (App. A.10); only lastBounce cuts them,
    # so [0,2] evaluated on length-10 paths = [0,10] - [3,10]
    low_on_long = torch.zeros_like(full)
    gpu.render_device(1, 0, spp, 0, 10, low_on_long.data_ptr())
    assert torch.allclose(low_on_long - upper, lower, rtol=1e-3, atol=1e-3)
    # directly visible light texels equal Ke = (17, 12, 4) exactly at bounce window [0, 0]
    direct = torch.zeros_like(full)
    gpu.render_device(1, 0, 1, 0, 0, direct.data_ptr())
    lit = direct[direct[..., 0] > 0]
    assert lit.shape[0] > 1000 and torch.equal(lit, torch.tensor([17.0, 12.0, 4.0], device="cuda").expand_as(lit))


@pytest.mark.parametrize("scene_path,width,height,spp,tolerance", [
    ("scenes/mis-pbrt.json", 1024, 1024, 8, 0.05),                 # BASELINE config 3: plastic + Beckmann plates, sphere lights
    ("scenes/teapot.json", 1024, 1024, 8, 0.05),                   # config 4: glass + checkerboard + environment light
    ("assets/dragon-standin-9.json", 1920, 1080, 2, 0.05),         # config 5: the 5.2 M-triangle stand-in at 1080p
])
def test_full_size_properties_of_the_other_configurations(libs, scene_path, width, height, spp, tolerance):
    """BASELINE configurations 3-5 at THEIR resolutions (the oracle comparisons run at 96^2 / 128x72): size-independent
    properties.  Energy: the image mean equals the mean of an oracle rendering of the same camera at a sixteenth of the
    resolution (pixels are Monte Carlo estimates of one integral over the image plane, whatever the grid).  Window additivity:
    a vertex's contribution does not depend on the window it is counted in and lastBounce only cuts paths after it, so
    [0, 2] = [0, 10] - [3, 10] up to the unconditional environment term of missed camera rays (reference
    src/bounce_controller.cpp:14-25).  Nothing is dropped, everything is finite and >= 0."""
    import torch
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, width, height)
    gpu = HipScene(scene.desc, device=0, bvh_builder="ploc" if scene.n_triangles > 1000000 else "sah")
    full = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda")
    gpu.render_device(1, 0, spp, 0, 10, full.data_ptr())
    torch.cuda.synchronize()
    assert torch.isfinite(full).all() and (full >= 0).all()
    assert gpu.stats()["dropped_samples"] == 0
    mean = (full / spp).mean(dim=(0, 1)).cpu().numpy()
    small = LoadedScene(scene_path, width // 4, height // 4)
    expected, _ = oracle_lib.OracleScene(small.desc).render(width // 4, height // 4, 1, 0, 4 * spp, 0, 10, threads=os.cpu_count())
    expected_mean = (expected / (4 * spp)).reshape(-1, 3).mean(axis=0)
    assert np.allclose(mean, expected_mean, rtol=tolerance), (mean, expected_mean)
    upper = torch.zeros_like(full)
    gpu.render_device(1, 0, spp, 3, 10, upper.data_ptr())
    lower = torch.zeros_like(full)
    gpu.render_device(1, 0, spp, 0, 2, lower.data_ptr())
    torch.cuda.synchronize()
    # a camera ray that misses everything returns the environment WHATEVER the window (reference src/sample_integrator.cpp:
    # the miss branch is not gated by checkCounts): that term E is in all three images, so full - upper = lower - E; with
    # nothing emissive in view of the camera (these three scenes with an environment), E is the [0, 0] window's image
    miss = torch.zeros_like(full)
    if bool(scene.desc.contents.env):
        gpu.render_device(1, 0, spp, 0, 0, miss.data_ptr())
        torch.cuda.synchronize()
    # additivity holds per pixel up to the rounding of the sums; a handful of glass / plastic pixels carry large values
    difference = (full - upper - lower + miss).abs()
    scale = torch.maximum(full.abs(), torch.tensor(1.0, device="cuda"))
    assert (difference <= 1e-3 * scale).float().mean().item() > 0.9999, float((difference / scale).max())


def _render_with_options(libs, options, scene_path, size, seed, spp, count=False):
    """Scene-creation-time switches travel in PathedSceneOptions (include/pathed_hip.h)."""
    _, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, size, size)
    gpu = HipScene(scene.desc, device=0, **options)
    if count:
        gpu.set_stats_mode(count=True)
        gpu.reset_stats()
    return gpu.render(seed, 0, spp, 0, 10), gpu.stats()


def test_result_does_not_depend_on_scheduling_or_intersector_variant(libs):
    """One pool or two, all-triangles kernel or LDS-resident BVH walk: the image is bit-identical,
    because hits follow an order-independent acceptance rule and the per-pixel summation order is
    fixed by the unit decomposition, not by which slot happened to render which unit."""
    base, base_stats = _render_with_options(libs, {"pools": 1}, "scenes/cornell.json", 160, 11, 12)
    assert base_stats["scene_in_lds"] == 2
    for pools in (2, 3, 4):
        several, _ = _render_with_options(libs, {"pools": pools}, "scenes/cornell.json", 160, 11, 12)
        assert np.array_equal(base, several), pools
    bvh, bvh_stats = _render_with_options(libs, {"intersector": "bvh"}, "scenes/cornell.json", 160, 11, 12)
    assert bvh_stats["scene_in_lds"] == 1
    assert np.array_equal(base, bvh)
    few_slots, _ = _render_with_options(libs, {"max_slots": 4096}, "scenes/cornell.json", 160, 11, 12)
    assert np.array_equal(base, few_slots)
    # a BVH scene (1 112 triangles, nodes in HBM/L2), one pool vs two
    glass_one, stats = _render_with_options(libs, {"pools": 1, "shade_kernel": "per-slot"}, "scenes/cornell-glass.json", 128, 3, 8)
    assert stats["scene_in_lds"] == 0 and stats["path_kernel"] == 1
    for pools in (2, 3):
        glass_several, _ = _render_with_options(libs, {"pools": pools, "max_slots": 20000, "shade_kernel": "per-slot"}, "scenes/cornell-glass.json", 128, 3, 8)
        assert np.array_equal(glass_one, glass_several), pools
    # ... and what such a scene runs by default since round 5: the hybrid kernel (direct set + a tree of the rest, path_hybrid.h)
    hybrid, stats = _render_with_options(libs, {}, "scenes/cornell-glass.json", 128, 3, 8)
    assert stats["path_kernel"] == 7 and np.array_equal(glass_one, hybrid)


@pytest.mark.parametrize("scene_path,width,height,spp", [
    ("scenes/cornell.json", 97, 53, 7),          # fused kernel; ragged bands, blocks and last group
    ("scenes/cornell-glass.json", 70, 41, 5),    # wavefront, two pools
    ("scenes/teapot.json", 33, 19, 3),           # fewer chunks than queues: most queues are empty, blocks move on
])
def test_unit_orders_are_bit_identical(libs, scene_path, width, height, spp):
    """Which slot renders which (pixel, chunk) unit, and when, is scheduling: chunk stripes (default), stripes walked in
    32 x 8 tiles, pixel tiles, one or several samples per unit, any pool count -- the same floats (kernels.h: THE UNIT ORDER)."""
    _, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, width, height)
    expected = HipScene(scene.desc, device=0).render(3, 1, spp, 0, 8)
    assert expected.any()
    from conftest import has_experiments
    staged = ({"unit_order": "stripes-tiled", "shade_kernel": "staged"}, {"unit_order": "tiles", "shade_kernel": "staged", "max_slots": 4096})
    for options in ({"unit_order": "stripes-tiled"}, {"unit_order": "tiles"}, {"unit_order": "tiles", "pools": 1},
                    {"unit_order": "tiles", "shade_kernel": "per-slot", "pools": 3}) + (staged if has_experiments() else ()):
        gpu = HipScene(scene.desc, device=0, **options)
        assert np.array_equal(gpu.render(3, 1, spp, 0, 8), expected), options
    coarse = HipScene(scene.desc, device=0)
    coarse.set_samples_per_unit(3)           # ragged last unit
    tiled = HipScene(scene.desc, device=0, unit_order="tiles", pools=1)
    tiled.set_samples_per_unit(3)
    assert np.array_equal(tiled.render(3, 1, spp, 0, 8), coarse.render(3, 1, spp, 0, 8))


@pytest.mark.parametrize("scene_path,size,spp,last_bounce", [
    ("scenes/cornell.json", 96, 12, 10),            # all-triangles kernel, emitter hits, paths that run to lastBounce
    ("scenes/cornell-glass.json", 80, 8, 10),       # BVH walk, glass + Lambertian, parked rays
    ("scenes/mis-pbrt.json", 96, 8, 6),             # sphere lights, plastic plates: black-bodied emitters end samples
    ("scenes/teapot.json", 96, 8, 10),              # environment light, glass, checkerboard
    ("scenes/cornell-oren-nayar.json", 64, 6, 3),   # Oren-Nayar + microfacet, short bounce window
    ("scenes/cornell-ggx.json", 64, 6, 5),          # GGX microfacet: the any-BSDF, triangle-lit instantiation of the fused kernel
    ("test_scenes/environment_map_sampling.json", 64, 8, 4),
])
def test_shade_kernels_are_bit_identical(libs, scene_path, size, spp, last_bounce):
    """Four organisations of the same arithmetic.  k_shade: one lane per slot.  k_shade_staged: classify ->
    key-sorted dense vertex stage -> dense regeneration stage, per block of 512 or 1024 slots.  k_vertex + k_regen (BVH
    scenes): dense kernels over the hit / miss lists the trace kernel writes.  k_path_small
    (scenes of <= 64 triangles): whole paths in registers, one persistent launch.  Each performs k_shade's
    operations in k_shade's order for every path and the unit decomposition fixes the summation order: the
    radiance sums are the same floats, whatever the block size, pool count or summation granularity."""
    _, HipScene, LoadedScene = libs
    scene = LoadedScene(scene_path, size, size)
    per_slot = HipScene(scene.desc, device=0, shade_kernel="per-slot")
    from conftest import has_experiments
    from pathed_amd.integrator import PathedError
    experiments = has_experiments()   # the staged and split organisations live in libpathed_hip_experiments.so
    expected = per_slot.render(7, 3, spp, 0, last_bounce)
    assert expected.any() and per_slot.stats()["path_kernel"] == 1
    if experiments:
        for options in ({"stage_slots": 512}, {"stage_slots": 1024}, {"stage_slots": 512, "pools": 1, "max_slots": 4096},
                        {"stage_slots": 1024, "pools": 3}):
            staged = HipScene(scene.desc, device=0, shade_kernel="staged", **options)
            assert np.array_equal(staged.render(7, 3, spp, 0, last_bounce), expected), options
            assert staged.stats()["path_kernel"] == 2
    else:
        for kind in ("staged", "split"):
            with pytest.raises(PathedError, match="experiments"):
                HipScene(scene.desc, device=0, shade_kernel=kind)
    # bounce windows and units of several samples (the default is one sample per unit, the reference's summation order)
    per_slot.set_samples_per_unit(4)
    windowed = per_slot.render(2, 0, 3, 1, 2)
    if experiments:
        staged = HipScene(scene.desc, device=0, shade_kernel="staged")
        staged.set_samples_per_unit(4)
        assert np.array_equal(staged.render(2, 0, 3, 1, 2), windowed)
    automatic = HipScene(scene.desc, device=0)
    if automatic.stats()["scene_in_lds"] == 2:
        # the default for tiny scenes is the fused kernel
        assert automatic.stats()["path_kernel"] == 3
        assert np.array_equal(automatic.render(7, 3, spp, 0, last_bounce), expected)
        # ... in the instantiation narrowed to the scene's material / light kinds (shading.h: SceneTraits) where there is one
        # (Cornell, the Veach scene), and in the generic one
        generic = HipScene(scene.desc, device=0, shade_kernel="fused", generic_kernels=1)
        assert np.array_equal(generic.render(7, 3, spp, 0, last_bounce), expected)
        automatic.set_samples_per_unit(4)
        assert np.array_equal(automatic.render(2, 0, 3, 1, 2), windowed)
        automatic.set_samples_per_unit(7)
        per_slot.set_samples_per_unit(7)
        assert np.array_equal(automatic.render(9, 5, 23, 0, last_bounce), per_slot.render(9, 5, 23, 0, last_bounce))   # ragged last unit
        with pytest.raises(PathedError):
            HipScene(scene.desc, device=0, shade_kernel="split")   # the split stage follows the BVH trace kernel
    else:
        # the default for BVH scenes is the per-slot kernel; the split shade stage (k_vertex + k_regen over the trace
        # kernel's hit / miss lists) is selectable
        assert automatic.stats()["path_kernel"] == 1
        # scenes lit by the environment alone take k_shade<.., ENV_ONLY> (emitter look-ups and the triangle / sphere light
        # code compiled out): the same floats as the generic instantiation
        generic = HipScene(scene.desc, device=0, shade_kernel="per-slot", generic_kernels=1)
        assert np.array_equal(generic.render(7, 3, spp, 0, last_bounce), expected)
        if not experiments:
            return
        split = HipScene(scene.desc, device=0, shade_kernel="split")
        assert np.array_equal(split.render(7, 3, spp, 0, last_bounce), expected)
        split.set_samples_per_unit(4)
        assert np.array_equal(split.render(2, 0, 3, 1, 2), windowed)
        # any pool count, few slots (many iterations), rays parked eagerly (slots wait for a parked shadow ray on the
        # deferred lists), a tiny persistent grid of the trace kernel (long lists per wave)
        for options in ({"pools": 1}, {"pools": 3, "max_slots": 4096}, {"pools": 1, "max_slots": 1024},
                        {"suspend_lanes": 64, "suspend_patience": 1, "park_min_cards": -1, "trace_blocks_per_cu": 1},
                        {"suspend_lanes": -1}, {"stack_rows": 8, "unit_order": "tiles"}):
            split = HipScene(scene.desc, device=0, shade_kernel="split", **options)
            assert np.array_equal(split.render(7, 3, spp, 0, last_bounce), expected), options
            assert split.stats()["path_kernel"] == 5
        with pytest.raises(PathedError):
            HipScene(scene.desc, device=0, shade_kernel="fused")


def test_scene_options_are_validated(libs):
    """PathedSceneOptions: wrong struct size, unknown builder, bad stack rows are PATHED_E_INVALID, not a crash."""
    import ctypes as C
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError
    _, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/cornell.json", 16, 16)
    with pytest.raises(PathedError):
        HipScene(scene.desc, device=0, stack_rows=9)
    with pytest.raises(PathedError):
        HipScene(scene.desc, device=0, pools=7)
    with pytest.raises(PathedError):
        HipScene(scene.desc, device=4096)
    lib = _capi.load_hip()
    options = _capi.PathedSceneOptions()
    options.struct_size = 12
    handle = C.c_void_p()
    assert lib.pathed_hip_scene_create_ex(scene.desc, C.byref(options), C.byref(handle)) == -1
    assert HipScene(scene.desc, device=0).device == 0


def test_rays_carried_over_between_trace_launches_change_nothing(libs):
    """A trace wave that is out of work hands its last unfinished rays (ray, best hit so far,
    traversal stack) to the next launch instead of idling on them.  With that switched off, on, or
    set so eagerly that most waves hand rays on every launch, the image is the same bit for bit."""
    # one block per CU: each wave draws enough cards to run well past the minimum step count
    few_waves = {"trace_blocks_per_cu": 1}
    off, off_stats = _render_with_options(libs, dict(few_waves, suspend_lanes=-1), "scenes/cornell-glass.json", 384, 5, 8, count=True)
    assert off_stats["scene_in_lds"] == 0 and off_stats["parked_rays"] == 0
    default, default_stats = _render_with_options(libs, few_waves, "scenes/cornell-glass.json", 384, 5, 8, count=True)
    assert default_stats["parked_rays"] > 0
    assert np.array_equal(off, default)
    eager, eager_stats = _render_with_options(libs, dict(few_waves, suspend_lanes=64, suspend_patience=-1),
                                              "scenes/cornell-glass.json", 384, 5, 8, count=True)
    assert eager_stats["parked_rays"] > default_stats["parked_rays"]
    assert np.array_equal(off, eager)
    assert eager_stats["closest_rays"] == off_stats["closest_rays"]
    assert eager_stats["shadow_rays"] == off_stats["shadow_rays"]
    assert eager_stats["nodes_visited"] == off_stats["nodes_visited"]  # nothing is re-traversed


def test_traversal_stack_spill_to_hbm_changes_nothing(libs):
    """The per-lane traversal stack keeps its first rows in LDS and spills deeper entries to a
    per-thread column in HBM.  With only 8 LDS rows the teapot's tree (bound: 3 entries per level)
    spills for a large share of the rays, in the test hook, in the render kernel and in the
    records of parked rays: hits and image stay bit-identical."""
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("scenes/teapot.json", 96, 96)
    spilling = HipScene(scene.desc, device=0, stack_rows=8)
    assert spilling.stats()["bvh_max_depth"] * 3 + 1 > 8
    rays = _rays(100000, 21, (0, 4, 0), 9.0)
    hits = spilling.trace(rays)
    occluded = spilling.trace(rays, any_hit=True)
    # park although the pool is small
    parked_scene = HipScene(scene.desc, device=0, stack_rows=8, trace_blocks_per_cu=1, suspend_lanes=64,
                            suspend_patience=-1, park_min_cards=-1)
    parked_scene.set_stats_mode(count=True)
    image = parked_scene.render(3, 0, 8, 0, 8)
    assert parked_scene.stats()["parked_rays"] > 0
    cpu = oracle_lib.OracleScene(scene.desc)
    assert np.array_equal(hits.view(np.int32), cpu.trace(rays).view(np.int32))
    assert np.array_equal(occluded, cpu.trace(rays, any_hit=True))
    default = HipScene(scene.desc, device=0)
    assert np.array_equal(default.trace(rays).view(np.int32), hits.view(np.int32))
    assert np.array_equal(default.render(3, 0, 8, 0, 8), image)


@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_trace_hook_gives_the_same_bits_with_every_stack_row_count(libs, kind):
    """k_trace_rays<8 | 16 | 22> and k_trace_rays_instanced<8 | 16 | 22> (pathed_hip_trace): the row count the scene takes by
    default and every larger one, so that no rung spills; closest hits and occlusion flags are equal bit for bit."""
    _, HipScene, _ = libs
    if kind == "flat":
        # 8 triangles under intersector="bvh": leaves of <= 2 triangles make <= 7 leaves, which two 4-wide levels always hold
        from scene_builder import BuiltScene
        built = BuiltScene(16, 12, origin=(0, 1, 4.5), target=(0, 1, 0), fov_degrees=45.0)
        grey = built.material(diffuse=(0.5, 0.5, 0.5))
        built.quad([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], grey)
        built.quad([(-2, 0, -2), (-2, 2.4, -2), (2, 2.4, -2), (2, 0, -2)], grey)
        built.quad([(-2, 0, 2), (-2, 2.4, 2), (-2, 2.4, -2), (-2, 0, -2)], grey)
        built.quad([(-0.5, 2.2, -0.5), (0.5, 2.2, -0.5), (0.5, 2.2, 0.5), (-0.5, 2.2, 0.5)], built.material(emit=(5, 4, 3)))
        desc = built.finish()
        create = lambda rows: HipScene(desc, device=0, stack_rows=rows, intersector="bvh")
        rays = _rays(300, 5, (0, 1.2, 0), 1.5)
        rays[200:, 7] = 2.5   # short rays: occlusion flags of both kinds
    else:
        import instances_scene as S
        _, pointer, prototypes, placements = S.build(S.EXACT_PLACEMENTS, 16, 12)
        create = lambda rows: HipScene(pointer, device=0, prototypes=prototypes, instances=placements, stack_rows=rows)
        rays = _rays(300, 5, S.CAMERA["target"], 6.0)
        rays[200:, 7] = 6.0
    default = create(0)
    depth = default.stats()["bvh_max_depth"]
    if kind == "flat":
        assert 3 * depth + 1 <= 8   # the default is 8 rows: all three rungs run
    bound = 3 * depth + 1 if kind == "flat" else 3 * depth + 3   # (two trees: (3 top + 1) + (3 deepest + 1) + 1)
    first = 8 if bound <= 8 else 16 if bound <= 16 else 22
    hits, occluded = default.trace(rays), default.trace(rays, any_hit=True)
    assert 0.1 < (hits[:, 3].view(np.int32) >= 0).mean() and 0.05 < occluded.mean() < 0.95
    for rows in [rows for rows in (8, 16, 22) if rows >= first]:
        forced = create(rows)
        assert np.array_equal(forced.trace(rays).view(np.int32), hits.view(np.int32)), rows
        assert np.array_equal(forced.trace(rays, any_hit=True), occluded), rows


def test_large_mesh_intersector_and_render_parity(libs):
    """The large-BVH configuration in small: the procedural stand-in mesh at 82 K triangles (deep
    4-wide tree, nodes in L2/HBM, stack spill possible), traced and rendered against the oracle."""
    import subprocess
    import sys
    oracle_lib, HipScene, LoadedScene = libs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = LoadedScene("assets/dragon-standin-6.json", 96, 54)   # generated by tests/conftest.py before the first GPU call
    assert scene.n_triangles > 80000
    gpu, cpu = HipScene(scene.desc, device=0), oracle_lib.OracleScene(scene.desc)
    stats = gpu.stats()
    assert stats["scene_in_lds"] == 0 and stats["bvh_max_depth"] >= 8
    rng = np.random.default_rng(4)
    n = 100000
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.normal(size=(n, 3)) * 120 + [0, 0, 25]
    target = rng.normal(size=(n, 3)) * 30 + [0, 0, 25]
    direction = target - rays[:, 0:3]
    rays[:, 4:7] = direction / np.linalg.norm(direction, axis=1, keepdims=True)
    rays[:, 3] = 1e-3
    rays[:, 7] = 1e5
    hits_gpu, hits_cpu = gpu.trace(rays), cpu.trace(rays)
    assert np.array_equal(hits_gpu.view(np.int32), hits_cpu.view(np.int32))
    assert (hits_cpu[:, 3].view(np.int32) >= 0).mean() > 0.5
    assert np.array_equal(gpu.trace(rays, any_hit=True), cpu.trace(rays, any_hit=True))
    image = gpu.render(1, 0, 8, 0, 10)
    expected, _ = cpu.render(96, 54, 1, 0, 8, 0, 10, threads=os.cpu_count())
    rel, bad = _image_metrics(image, expected)
    assert rel <= 2e-3 and bad <= 2e-3, (rel, bad)


def _unpack_compressed(words):
    """(origin (n,3), scale (n,3), qlo (n,3,4), qhi (n,3,4), refs (n,4)) of exported compressed nodes (include/pathed_hip.h)"""
    as_float = words.view(np.float32)
    origin = as_float[:, 0:3].astype(np.float64)
    scale = as_float[:, 3:6].astype(np.float64)
    shifts = np.arange(4, dtype=np.uint32) * 8
    qlo = ((words[:, 6:9, None] >> shifts) & 255).astype(np.float64)
    qhi = ((words[:, 9:12, None] >> shifts) & 255).astype(np.float64)
    return origin, scale, qlo, qhi, words[:, 12:16].view(np.int32)


@pytest.mark.experiments
@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_compressed_nodes_contain_the_float_boxes_and_change_no_hit(libs, builder):
    """node_format "compressed" (trace.h: nodeQ): every child's 8-bit grid box contains its float box (exported and checked
    here in float64), the refs are the float tree's, so the triangle tests -- which alone decide a hit -- see a superset
    of the leaves: hits, occlusion and images are the bits of the 128-byte nodes and of the oracle."""
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("assets/dragon-standin-6.json", 96, 54)
    # (local_rays=1: off -- the experiments' node formats do not carry them, and the node counts below compare like with like)
    wide = HipScene(scene.desc, device=0, bvh_builder=builder, node_format="wide", local_rays=1)
    packed = HipScene(scene.desc, device=0, bvh_builder=builder, node_format="compressed")
    assert wide.export_compressed_nodes().shape[0] == 0
    nodes, _ = wide.export_bvh()
    words = packed.export_compressed_nodes()
    assert words.shape == (nodes.shape[0], 16)
    origin, scale, qlo, qhi, refs = _unpack_compressed(words)
    float_refs = nodes[:, 24:28].view(np.int32)
    assert np.array_equal(refs, float_refs)
    valid = float_refs != np.int32(-2 ** 31)                                  # (n, 4)
    lo = nodes[:, 0:12].reshape(-1, 3, 4).astype(np.float64)               # (n, axis, child)
    hi = nodes[:, 12:24].reshape(-1, 3, 4).astype(np.float64)
    grid_lo = origin[:, :, None] + qlo * scale[:, :, None]
    grid_hi = origin[:, :, None] + qhi * scale[:, :, None]
    mask = np.broadcast_to(valid[:, None, :], lo.shape)
    assert (grid_lo[mask] <= lo[mask]).all() and (grid_hi[mask] >= hi[mask]).all()
    # ... and not by much: at most two grid steps of slack per plane (one of rounding outward, the 1/256 on top)
    step = np.broadcast_to(scale[:, :, None], lo.shape)
    assert ((lo - grid_lo)[mask] <= 2 * step[mask]).all() and ((grid_hi - hi)[mask] <= 2 * step[mask]).all()
    assert (scale == 2.0 ** np.round(np.log2(np.maximum(scale, 1e-300))))[scale > 0].all()   # powers of two

    rng = np.random.default_rng(4)
    n = 100000
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.normal(size=(n, 3)) * 120 + [0, 0, 25]
    target = rng.normal(size=(n, 3)) * 30 + [0, 0, 25]
    direction = target - rays[:, 0:3]
    rays[:, 4:7] = direction / np.linalg.norm(direction, axis=1, keepdims=True)
    rays[:, 3] = 1e-3
    rays[:, 7] = 1e5
    # axis-parallel rays and rays that start on the mesh: the slab edge cases
    rays[:1000, 4:7] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 1000)] * rng.choice([-1.0, 1.0], (1000, 1)).astype(np.float32)
    cpu = oracle_lib.OracleScene(scene.desc)
    expected = cpu.trace(rays)
    on_mesh = expected[:, 3].view(np.int32) >= 0
    rays[on_mesh, 0:3] = rays[on_mesh, 0:3] + rays[on_mesh, 4:7] * expected[on_mesh, 0:1]
    rays[on_mesh, 4:7] = -rays[on_mesh, 4:7]
    expected = cpu.trace(rays)
    assert np.array_equal(packed.trace(rays).view(np.int32), expected.view(np.int32))
    assert np.array_equal(wide.trace(rays).view(np.int32), expected.view(np.int32))
    assert np.array_equal(packed.trace(rays, any_hit=True), cpu.trace(rays, any_hit=True))
    packed.set_stats_mode(count=True)
    wide.set_stats_mode(count=True)
    assert np.array_equal(packed.render(1, 0, 8, 0, 10), wide.render(1, 0, 8, 0, 10))
    # the grid boxes are a little larger: a few more boxes accepted, never fewer; the same primitives... or more
    assert wide.stats()["nodes_visited"] <= packed.stats()["nodes_visited"] <= 1.15 * wide.stats()["nodes_visited"]
    assert packed.stats()["closest_rays"] == wide.stats()["closest_rays"]


def _unpack_compressed8(words):
    as_float = words.view(np.float32)
    origin = as_float[:, 0:3].astype(np.float64)
    scale = as_float[:, 3:6].astype(np.float64)
    shifts = np.arange(4, dtype=np.uint32) * 8
    planes = ((words[:, 6:18].reshape(-1, 6, 2)[:, :, :, None] >> shifts) & 255).reshape(-1, 6, 8).astype(np.float64)
    return origin, scale, planes[:, 0:3], planes[:, 3:6], words[:, 20:28].view(np.int32)


@pytest.mark.experiments
@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_eight_wide_compressed_tree_covers_every_triangle_once_and_changes_no_hit(libs, builder):
    """node_format "compressed8" (trace.h: node8): walked from the root, the 8-wide tree reaches every leaf of the 4-wide
    tree exactly once, gets no deeper, and every child's grid box contains the triangles below it (checked on the exported
    words, level by level, in float64); hits, occlusion and image are the bits of the float nodes and of the oracle."""
    oracle_lib, HipScene, LoadedScene = libs
    scene = LoadedScene("assets/dragon-standin-6.json", 96, 54)
    # (local_rays=1: off -- the experiments' node formats do not carry them, and the node counts below compare like with like)
    wide = HipScene(scene.desc, device=0, bvh_builder=builder, node_format="wide", local_rays=1)
    packed = HipScene(scene.desc, device=0, bvh_builder=builder, node_format="compressed8")
    nodes, tris = wide.export_bvh()
    words = packed.export_compressed_nodes()
    assert words.shape == (nodes.shape[0], 32)
    origin, scale, qlo, qhi, refs = _unpack_compressed8(words)
    empty = np.int32(-2 ** 31)
    # triangle bounds per leaf-ordered triangle
    v0, e1, e2 = tris[:, 0:3].astype(np.float64), tris[:, 4:7].astype(np.float64), tris[:, 8:11].astype(np.float64)
    corners = np.stack([v0, (tris[:, 0:3] + tris[:, 4:7]).astype(np.float64), (tris[:, 0:3] + tris[:, 8:11]).astype(np.float64)])
    del e1, e2
    tri_lo, tri_hi = corners.min(axis=0), corners.max(axis=0)
    slack = 4e-6 * np.abs(corners).max()          # v0 + e rounds: the builders bound the ORIGINAL corners
    # level-order walk; per node the bounds of everything below it come back up afterwards
    order, level, depth = [], np.array([0]), 0
    seen_leaves = []
    while level.size:
        order.append(level)
        child = refs[level]                      # (m, 8)
        seen_leaves.append(child[(child <= -2) & (child != empty)])
        level = child[child >= 0]
        depth += 1
    assert depth <= wide.stats()["bvh_max_depth"]
    leaves = -np.concatenate(seen_leaves).astype(np.int64) - 1
    first, count = leaves >> 3, leaves & 7
    covered = np.zeros(tris.shape[0], dtype=np.int32)
    for k in range(1, 8):
        chosen = first[count >= k] + (k - 1)
        np.add.at(covered, chosen, 1)
    assert (covered == 1).all()
    visited = np.concatenate(order)
    assert np.unique(visited).size == visited.size and visited.size <= nodes.shape[0]
    # bounds bottom-up
    below_lo = np.full((nodes.shape[0], 3), np.inf)
    below_hi = np.full((nodes.shape[0], 3), -np.inf)
    for level in reversed(order):
        child = refs[level]
        for c in range(8):
            ref = child[:, c]
            grid_lo = origin[level] + qlo[level][:, :, c] * scale[level]
            grid_hi = origin[level] + qhi[level][:, :, c] * scale[level]
            lo = np.full((level.size, 3), np.inf)
            hi = np.full((level.size, 3), -np.inf)
            inner = ref >= 0
            lo[inner], hi[inner] = below_lo[ref[inner]], below_hi[ref[inner]]
            leaf = (ref <= -2) & (ref != empty)
            code = -ref[leaf].astype(np.int64) - 1
            leaf_lo, leaf_hi = np.full((code.size, 3), np.inf), np.full((code.size, 3), -np.inf)
            for k in range(7):
                has = (code & 7) > k
                index = (code >> 3)[has] + k
                leaf_lo[has] = np.minimum(leaf_lo[has], tri_lo[index])
                leaf_hi[has] = np.maximum(leaf_hi[has], tri_hi[index])
            lo[leaf], hi[leaf] = leaf_lo, leaf_hi
            present = inner | leaf
            assert (grid_lo[present] <= lo[present] + slack).all() and (grid_hi[present] >= hi[present] - slack).all()
            below_lo[level] = np.minimum(below_lo[level], np.where(present[:, None], lo, np.inf))
            below_hi[level] = np.maximum(below_hi[level], np.where(present[:, None], hi, -np.inf))
    filled = (refs[visited] != empty).sum(axis=1)
    # the nodes above the bottom are nearly full; a node whose children are all leaves has nothing to pull up
    has_inner = (refs[visited] >= 0).any(axis=1)
    assert filled[has_inner].mean() > 6.0 and filled.mean() > 4.5, (filled[has_inner].mean(), filled.mean())

    rng = np.random.default_rng(5)
    n = 100000
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.normal(size=(n, 3)) * 120 + [0, 0, 25]
    target = rng.normal(size=(n, 3)) * 30 + [0, 0, 25]
    direction = target - rays[:, 0:3]
    rays[:, 4:7] = direction / np.linalg.norm(direction, axis=1, keepdims=True)
    rays[:, 3] = 1e-3
    rays[:, 7] = 1e5
    rays[:1000, 4:7] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 1000)] * rng.choice([-1.0, 1.0], (1000, 1)).astype(np.float32)
    cpu = oracle_lib.OracleScene(scene.desc)
    expected = cpu.trace(rays)
    assert np.array_equal(packed.trace(rays).view(np.int32), expected.view(np.int32))
    assert np.array_equal(packed.trace(rays, any_hit=True), cpu.trace(rays, any_hit=True))
    # with 8 LDS rows the deeper stacks of the 8-wide walk spill to HBM, and parked rays carry them
    spilling = HipScene(scene.desc, device=0, bvh_builder=builder, node_format="compressed8", stack_rows=8, trace_blocks_per_cu=1,
                        suspend_lanes=64, suspend_patience=-1, park_min_cards=-1)
    assert np.array_equal(spilling.trace(rays).view(np.int32), expected.view(np.int32))
    image = wide.render(1, 0, 8, 0, 10)
    packed.set_stats_mode(count=True)
    wide.set_stats_mode(count=True)
    assert np.array_equal(packed.render(1, 0, 8, 0, 10), image)
    assert np.array_equal(wide.render(1, 0, 8, 0, 10), image)
    spilling.set_stats_mode(count=True)
    assert np.array_equal(spilling.render(1, 0, 8, 0, 10), image)
    assert spilling.stats()["parked_rays"] > 0
    assert packed.stats()["closest_rays"] == wide.stats()["closest_rays"]


@pytest.mark.experiments
def test_compressed_nodes_are_refused_where_they_do_not_apply(libs):
    oracle_lib, HipScene, LoadedScene = libs
    for path, options in (("scenes/cornell.json", {}), ("scenes/mis-pbrt.json", {"intersector": "bvh"}),
                          ("scenes/teapot.json", {"shade_kernel": "split"}), ("scenes/teapot.json", {"generic_kernels": 1})):
        scene = LoadedScene(path, 32, 32)
        with pytest.raises(RuntimeError, match="compressed nodes"):
            HipScene(scene.desc, device=0, node_format="compressed", **options)
    scene = LoadedScene("scenes/teapot.json", 64, 64)
    assert np.array_equal(HipScene(scene.desc, device=0, node_format="compressed").render(2, 0, 8, 0, 10),
                          HipScene(scene.desc, device=0, node_format="wide").render(2, 0, 8, 0, 10))


def test_threaded_bvh_build_gives_the_sequential_tree(libs):
    """Meshes of >= 200 000 triangles are built with the top of the tree on one thread and its
    subtrees on the others; the exported tree must be the one a single thread builds."""
    import subprocess
    import sys
    _, HipScene, LoadedScene = libs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = LoadedScene("assets/dragon-standin-7.json", 64, 36)   # generated by tests/conftest.py before the first GPU call
    assert scene.n_triangles >= 200000
    nodes_one, tris_one = HipScene(scene.desc, device=0, build_threads=1).export_bvh()
    threaded = HipScene(scene.desc, device=0, build_threads=8)
    nodes_many, tris_many = threaded.export_bvh()
    assert np.array_equal(nodes_one.view(np.int32), nodes_many.view(np.int32))
    assert np.array_equal(tris_one.view(np.int32), tris_many.view(np.int32))
    assert threaded.render(1, 0, 2, 0, 4).any()


def test_unbounded_last_bounce_terminates_and_matches(libs):
    """lastBounce = -1 (reference: unbounded, src/bounce_controller.cpp:20-25): paths end on a miss or
    when the throughput underflows to exactly black.  Open scene so every path escapes."""
    oracle_lib, HipScene, _ = libs
    from scene_builder import BuiltScene
    built = BuiltScene(48, 48, (0, 2, 6), (0, 0.5, 0), fov_degrees=35)
    floor = built.material(diffuse=(0.6, 0.6, 0.6))
    light = built.material(diffuse=(0, 0, 0), emit=(8, 8, 8))
    built.quad([(-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4)], floor)
    built.quad([(-1, 3, -1), (1, 3, -1), (1, 3, 1), (-1, 3, 1)], light)
    built.sphere((0, 0.6, 0), 0.6, built.material(diffuse=(0.7, 0.3, 0.2)))
    desc = built.finish()
    image = HipScene(desc, device=0).render(2, 0, 8, 0, -1)
    expected, stats = oracle_lib.OracleScene(desc).render(48, 48, 2, 0, 8, 0, -1)
    rel, bad = _image_metrics(image, expected)
    assert rel < 2e-3 and bad <= 2e-3
    assert stats["vertices"] > 0.5 * stats["camera_samples"]  # most camera rays hit and bounce
    shallow, _ = oracle_lib.OracleScene(desc).render(48, 48, 2, 0, 8, 0, 1)
    assert expected.sum() > shallow.sum() * 1.01  # the unbounded render carries indirect light


def test_bandwidth_probe_reports_a_plausible_rate():
    """pathed_hip_measure_bandwidth: the measured roofline denominator bench.py prints."""
    from pathed_amd.integrator import measure_bandwidth
    read, copy = measure_bandwidth(gib=1.0, repeats=5)
    assert 1000.0 < read < 9000.0 and 1000.0 < copy < 9000.0, (read, copy)   # GB/s on an MI355X (8 TB/s peak)


def _sphere_field(count, width=64, height=48, floor=True):
    """`count` spheres of mixed materials scattered over a floor under an area light."""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    rng = np.random.default_rng(19)
    built = BuiltScene(width, height, (0, 6, 14), (0, 1, 0), fov_degrees=40)
    materials = [built.material(diffuse=(0.7, 0.3, 0.2)), built.material(diffuse=(0.2, 0.6, 0.3)),
                 built.material(type_=_capi.MAT_MIRROR), built.material(type_=_capi.MAT_GLASS, ior=1.5),
                 built.material(type_=_capi.MAT_PLASTIC, diffuse=(0.1, 0.2, 0.6), alpha=0.1)]
    light = built.material(diffuse=(0, 0, 0), emit=(30, 28, 25))
    if floor:
        built.quad([(-12, 0, 12), (12, 0, 12), (12, 0, -12), (-12, 0, -12)], built.material(diffuse=(0.6, 0.6, 0.6)))
        built.quad([(-3, 9, -3), (3, 9, -3), (3, 9, 3), (-3, 9, 3)], light)
    for index in range(count):
        radius = float(rng.uniform(0.15, 0.6))
        centre = (float(rng.uniform(-9, 9)), radius + float(rng.uniform(0.0, 2.5)), float(rng.uniform(-9, 9)))
        built.sphere(centre, radius, materials[index % len(materials)])
    if not floor:
        built.sphere((0.0, 12.0, 0.0), 1.5, light)   # a sphere light: the scene has no triangle at all
    return built


def test_many_spheres_live_in_the_tree_not_in_a_list(libs):
    """More than 16 spheres: the host builder gives each a leaf of the 4-wide tree (count-0 leaf references), so a ray
    tests the few it comes near instead of all of them (the reference hands every sphere to Embree's tree,
    src/sphere.cpp:16-48).  Hits and images: the oracle's, which tests every sphere against every ray."""
    oracle_lib, HipScene, _ = libs
    built = _sphere_field(300)
    desc = built.finish()
    gpu, cpu = HipScene(desc, device=0), oracle_lib.OracleScene(desc)
    assert gpu.stats()["scene_in_lds"] == 0
    rays = _rays(100000, 8, (0, 2, 0), 9.0)
    expected = cpu.trace(rays)
    hit_prims = expected[:, 3].view(np.int32)
    assert (hit_prims >= 4).mean() > 0.08                       # plenty of sphere hits (prim ids 4 ..)
    assert np.array_equal(gpu.trace(rays).view(np.int32), expected.view(np.int32))
    assert np.array_equal(gpu.trace(rays, any_hit=True), cpu.trace(rays, any_hit=True))
    gpu.set_stats_mode(count=True)
    gpu.reset_stats()
    image = gpu.render(3, 0, 8, 0, 8)
    stats = gpu.stats()
    assert stats["tris_tested"] < 12 * (stats["closest_rays"] + stats["shadow_rays"])   # not 300 sphere tests per ray
    expected_image, _ = cpu.render(64, 48, 3, 0, 8, 0, 8, threads=os.cpu_count())
    rel, bad = _image_metrics(image, expected_image)
    assert rel <= 1e-2 and bad <= 5e-3, (rel, bad)              # glass and mirror spheres: a flipped decision changes a path
    # the same tree through the kernel with 8 stack rows and eager parking, and a tree of spheres ONLY (no triangle)
    again = HipScene(desc, device=0, stack_rows=8, trace_blocks_per_cu=1, suspend_lanes=64, suspend_patience=-1, park_min_cards=-1)
    assert np.array_equal(again.render(3, 0, 8, 0, 8), image)
    only = _sphere_field(40, floor=False).finish()
    gpu_only, cpu_only = HipScene(only, device=0), oracle_lib.OracleScene(only)
    assert gpu_only.stats()["scene_in_lds"] in (0, 1) and gpu_only.stats()["bvh_nodes"] > 0     # a small tree may be staged in LDS
    assert np.array_equal(gpu_only.trace(rays).view(np.int32), cpu_only.trace(rays).view(np.int32))
    image_only = gpu_only.render(5, 0, 8, 0, 6)
    expected_only, _ = cpu_only.render(64, 48, 5, 0, 8, 0, 6, threads=os.cpu_count())
    rel, bad = _image_metrics(image_only, expected_only)
    assert image_only.any() and rel <= 1e-2 and bad <= 5e-3, (rel, bad)
    # sixteen spheres or fewer beside a tiny mesh stay with the all-triangles kernels (Veach's scene has five)
    few = _sphere_field(12).finish()
    assert HipScene(few, device=0).stats()["scene_in_lds"] == 2


def test_set_camera_is_a_fresh_scene_with_that_camera(libs):
    """pathed_hip_scene_set_camera: another view of an uploaded scene, nothing rebuilt -- the same floats as a scene created
    with that camera; another resolution is refused (the caller's sums are per pixel)."""
    import copy
    import ctypes
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError
    _, HipScene, LoadedScene = libs
    for path, size in (("scenes/cornell.json", 40), ("scenes/cornell-glass.json", 36)):   # fused kernel / wavefront
        first = LoadedScene(path, size, size)
        gpu = HipScene(first.desc, device=0)
        before = gpu.render(3, 0, 4, 0, 6)
        moved = copy.copy(first.desc.contents.camera)
        moved.origin = (ctypes.c_float * 3)(0.4, 1.3, 5.5)
        moved.target = (ctypes.c_float * 3)(-0.1, 0.8, 0.0)
        gpu.set_camera(moved)
        other = _capi.PathedSceneDesc()          # a shallow copy of the description (its arrays stay the loader's)
        ctypes.memmove(ctypes.byref(other), first.desc, ctypes.sizeof(other))
        other.camera = moved
        fresh = HipScene(ctypes.pointer(other), device=0)
        image = gpu.render(3, 0, 4, 0, 6)
        assert np.array_equal(image, fresh.render(3, 0, 4, 0, 6)) and not np.array_equal(image, before)
        gpu.set_camera(first.desc.contents.camera)
        assert np.array_equal(gpu.render(3, 0, 4, 0, 6), before)
        wrong = copy.copy(moved)
        wrong.width = size + 1
        with pytest.raises(PathedError):
            gpu.set_camera(wrong)


@pytest.mark.experiments
def test_valu_clock_probe_reports_consistent_clocks():
    """pathed_hip_measure_valu_clocks: the rate from HIP events and the cycles per instruction from the waves' own clocks
    describe the same run; bad arguments are PATHED_E_INVALID."""
    from pathed_amd.integrator import PathedError, measure_valu_clocks
    probe = measure_valu_clocks(waves_per_simd=2, chains=8, repeats=2)
    assert 1e11 < probe["rate"] < 2e12 and 500.0 < probe["shader_clock_mhz"] < 4000.0 and probe["wall_clock_mhz"] > 1.0
    assert 1.5 < probe["cycles_per_instruction_events"] < 8.0 and 1.0 < probe["wave_ticks_per_instruction"] < 40.0
    for bad in (dict(waves_per_simd=0), dict(chains=12), dict(repeats=0)):
        with pytest.raises(PathedError):
            measure_valu_clocks(**dict(dict(waves_per_simd=2, chains=8, repeats=2), **bad))
