"""The BasicVolumeIntegrator (reference src/basic_volume_integrator.cpp; k_path_scatter / k_path_scatter_grid):
multiple scattering in participating media, a stack of media.

The oracle knows PathTracer and VolumePathTracer only, so this integrator is held from two sides:
  A  identities with what the oracle does pin, bit for bit: on scenes without media it IS the path tracer; with a gas of
     sigma = 0 it is VolumePathTracer; splitting a call and walking the tree instead of testing every triangle change nothing;
  B-E  image means against the float64 random walk of tests/multiple_scattering_reference.py, which restates the estimator's
     accounting on analytic geometry;
  F  the phase function against its float64 formula.

Tolerance of B-E: |mean_gpu - mean_ref| <= 7.5 * sd_ref * sqrt(1 / N_gpu + 1 / N_ref) -- five standard errors of the
difference, with the walk's OWN per-sample standard deviation, times 1.5 because the device samples the constant 32 x 64
environment map through its CDF (2 048 texel-centre directions) rather than uniformly.  N_gpu = 128 x 128 x 64, N_ref = 10^6:
about 0.007.  Each test first asserts that this is at most a quarter of the smallest gap between the reference values it is
meant to tell apart.

The walk's containers are an analytic sphere and box.  On the device a container must be a MESH: an analytic sphere reports
one root per query, so it yields one volume event where the event rule wants the two crossings.  The sphere containers are
therefore latitude-longitude meshes (48 x 96, 9 024 triangles) whose vertices lie on the radius at which the mesh encloses the
sphere's volume, 1.0006 R: the facets then lie between 0.9995 R and 1.0006 R, which moves a chord's optical depth (at most
4) by less than 0.003 and the silhouette's share of the frame (0.72) by less than 0.001: image means move by less than
0.001, a seventh of the tolerance."""
import functools

import numpy as np
import pytest

SIZE, SPP, WALKS = 128, 64, 1000000
DISTANCE, FOV = 5.0, 24.0


def _tolerance(deviation):
    return 7.5 * deviation * np.sqrt(1.0 / (SIZE * SIZE * SPP) + 1.0 / WALKS)


@functools.lru_cache(maxsize=None)
def _walk(last_bounces, start_bounce=0, stack_rule="stack", **scene):
    """{last bounce: (mean, standard deviation)} of 10^6 walks, computed once per configuration and shared"""
    import multiple_scattering_reference as reference
    values, info = reference.walk(reference.Scene(distance=DISTANCE, fov_degrees=FOV, **scene), WALKS, last_bounces, start_bounce=start_bounce,
                                  stack_rule=stack_rule)
    assert info["dropped"] == 0 and info["surface_counted"] == 0, info
    return {last: reference.mean_and_deviation(values[last]) for last in last_bounces}


def _sphere_mesh(radius, rings=48, segments=96):
    """(vertices, faces) of a closed latitude-longitude mesh, outward winding, that encloses the volume of the sphere"""
    theta = np.pi * np.arange(1, rings) / rings
    phi = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.cos(theta), np.ones(segments)), np.outer(np.sin(theta), np.sin(phi))], axis=2)
    vertices = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    at = lambda r, s: 1 + r * segments + (s % segments)
    south = len(vertices) - 1
    faces = []
    for s in range(segments):
        faces.append((0, at(0, s), at(0, s + 1)))
        faces.append((south, at(rings - 2, s + 1), at(rings - 2, s)))
        for r in range(rings - 2):
            faces.append((at(r, s), at(r + 1, s), at(r + 1, s + 1)))
            faces.append((at(r, s), at(r + 1, s + 1), at(r, s + 1)))
    faces = np.array(faces)
    a, b, c = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) < 0.0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    a, b, c = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    volume = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    assert volume > 0.0
    return vertices * radius * (4.0 / 3.0 * np.pi / volume) ** (1.0 / 3.0), faces


def _built(sigma=2.0, albedo=1.0, inner=None, inner_sigma=6.0, rho=0.5, box=None):
    """the walk's scene for the device: BuiltScene, and the medium slot of the outer container"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(SIZE, SIZE, (0, 0, DISTANCE), (0, 0, 0), fov_degrees=FOV)
    passthrough = built.material(type_=_capi.MAT_PASSTHROUGH)
    gas = built.medium((sigma,) * 3, (sigma * albedo,) * 3)
    if box is not None:
        built.box(box[0], box[1], passthrough, medium=gas)
    else:
        built.mesh(*_sphere_mesh(1.0), passthrough, medium=gas)
    if inner == "container":
        built.mesh(*_sphere_mesh(0.45), passthrough, medium=built.medium((inner_sigma,) * 3, (inner_sigma,) * 3))
    elif inner == "lambertian":
        built.sphere((0, 0, 0), 0.45, built.material(diffuse=(rho,) * 3))
    built.environment(np.ones((32, 64, 4), dtype=np.float32), scale=1.0)
    return built, gas


def _gpu_mean(gpu, start_bounce, last_bounce):
    image = gpu.render(7, 0, SPP, start_bounce, last_bounce)
    stats = gpu.stats()
    assert np.isfinite(image).all() and stats["dropped_samples"] == 0 and stats["path_kernel"] == 9
    assert np.array_equal(image[..., 0], image[..., 1]) and np.array_equal(image[..., 0], image[..., 2])      # a grey world
    return float(image[..., 0].mean(dtype=np.float64)) / SPP


def _scene(built):
    from pathed_amd.integrator import HipScene
    gpu = HipScene(built.finish(), device=0)
    gpu.set_integrator("BasicVolumeIntegrator")
    return gpu


def _compare(gpu, reference, windows, start_bounce=0):
    for last in windows:
        mean, deviation = reference[last]
        found = _gpu_mean(gpu, start_bounce, last)
        print("window (%d, %d): gpu %.5f  walk %.5f  tolerance %.5f" % (start_bounce, last, found, mean, _tolerance(deviation)))
        assert abs(found - mean) <= _tolerance(deviation), (last, found, mean, _tolerance(deviation))


# ---------------------------------------------------------------------------------------------- A: identities
def _gas_scene(sigma, width=48, height=40):
    """the gas scene of tests/test_gpu_volume.py: a room corner, an area light, a box of gas with a glass ball inside"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(width, height, (0, 1.2, 5), (0, 1, 0), fov_degrees=38)
    white = built.material(diffuse=(0.7, 0.7, 0.7))
    red = built.material(diffuse=(0.6, 0.1, 0.1))
    light = built.material(diffuse=(0, 0, 0), emit=(20, 20, 20))
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], white)
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)], red)
    built.quad([(-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (0.5, 2.9, 0.5), (-0.5, 2.9, 0.5)], light)
    gas = built.medium((sigma, sigma, sigma), (sigma, sigma, sigma))
    built.box((-1, 0.2, -1), (1, 2.2, 1), built.material(type_=_capi.MAT_PASSTHROUGH), medium=gas)
    built.sphere((0, 1.0, 0), 0.4, built.material(type_=_capi.MAT_GLASS, ior=1.5))
    return built


@pytest.mark.gpu
@pytest.mark.parametrize("scene_path,size,spp,last_bounce", [
    ("scenes/cornell.json", 64, 8, 10), ("scenes/cornell-glass.json", 48, 6, 8), ("scenes/mis-pbrt.json", 64, 6, 5)])
def test_without_media_it_is_the_path_tracer(scene_path, size, spp, last_bounce):
    """A(i): no medium, no container -- no segment scatters, the stack only ever holds "none": PathTracer's sums, bit for bit"""
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene(scene_path, size, size)
    plain = HipScene(scene.desc, device=0)
    basic = HipScene(scene.desc, device=0, generic_kernels=1)
    basic.set_integrator("BasicVolumeIntegrator")
    expected = plain.render(5, 2, spp, 0, last_bounce)
    image = basic.render(5, 2, spp, 0, last_bounce)
    assert expected.any() and basic.stats()["path_kernel"] == 9 and basic.stats()["dropped_samples"] == 0
    assert np.isfinite(image).all() and np.array_equal(image, expected)
    assert np.array_equal(basic.render(5, 0, 3, 1, 2), plain.render(5, 0, 3, 1, 2))      # a bounce window
    dispatched = HipScene(scene.desc, device=0)      # by default such a scene takes the path tracer's kernels
    dispatched.set_integrator("BasicVolumeIntegrator")
    assert np.array_equal(dispatched.render(5, 2, spp, 0, last_bounce), expected) and dispatched.stats()["path_kernel"] == plain.stats()["path_kernel"]


@pytest.mark.gpu
def test_with_a_gas_of_no_density_it_is_the_volume_path_tracer():
    """A(ii): sigma = 0, a glass ball inside the gas.  The two integrators disagree about the medium behind the ball (the
    stack keeps the gas, the single pointer loses it), and every transmittance is exp(-0) either way."""
    from pathed_amd.integrator import HipScene
    desc = _gas_scene(0.0).finish()
    single, basic = HipScene(desc, device=0), HipScene(desc, device=0)
    single.set_integrator("VolumePathTracer")
    basic.set_integrator("BasicVolumeIntegrator")
    expected, image = single.render(4, 0, 16, 0, 8), basic.render(4, 0, 16, 0, 8)
    assert expected.any() and np.isfinite(image).all() and np.array_equal(image, expected)
    assert basic.stats()["path_kernel"] == 9 and basic.stats()["dropped_samples"] == 0
    assert np.array_equal(basic.render(4, 0, 8, 2, 5), single.render(4, 0, 8, 2, 5))


@pytest.mark.gpu
def test_split_calls_and_the_tree_walk_change_nothing():
    """A(iii), A(iv), A(v) on a scene WITH a scattering medium (sigma = 2, the glass ball inside)"""
    from pathed_amd.integrator import HipScene
    desc = _gas_scene(2.0).finish()
    gpu = HipScene(desc, device=0)
    gpu.set_integrator("BasicVolumeIntegrator")
    image = gpu.render(4, 0, 8, 0, 12)
    assert image.any() and np.isfinite(image).all() and gpu.stats()["dropped_samples"] == 0 and gpu.stats()["path_kernel"] == 9
    # onto a device buffer the sums continue sample by sample (pathed_hip_render_device): 3 + 5 samples are the 8 of one call
    import torch
    parts = torch.zeros((40, 48, 3), dtype=torch.float32, device="cuda:0")
    gpu.render_device(4, 0, 3, 0, 12, parts.data_ptr())
    gpu.render_device(4, 3, 5, 0, 12, parts.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(parts.cpu().numpy(), image)
    single = HipScene(desc, device=0)
    single.set_integrator("VolumePathTracer")
    assert not np.array_equal(single.render(4, 0, 8, 0, 12), image)      # ... and the medium does scatter more than once
    for rows in (8, 16, 22):
        walked = HipScene(desc, device=0, stack_rows=rows, intersector="bvh")
        walked.set_integrator("BasicVolumeIntegrator")
        assert np.array_equal(walked.render(4, 0, 8, 0, 12), image), rows
        assert walked.stats()["dropped_samples"] == 0


@pytest.mark.gpu
def test_other_integrators_still_refuse_containers():
    from pathed_amd.integrator import HipScene, PathedError
    gpu = HipScene(_gas_scene(1.0).finish(), device=0)
    for name in ("PathTracer", "AlbedoIntegrator"):
        gpu.set_integrator(name)
        with pytest.raises(PathedError):
            gpu.render(1, 0, 1, 0, 4)


# ---------------------------------------------------------------------------------------------- B: the scattering series
SERIES = (2, 3, 5, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("albedo", [1.0, 0.8])
def test_scattering_series(albedo):
    """B: sphere R = 1, sigma_t = 2, windows (0, N): N = 2 is what single scattering gives, every further N adds orders.
    The walk (10^6): 0.602, 0.735, 0.872, 0.987 at albedo 1 and 0.554, 0.639, 0.703, 0.731 at albedo 0.8, which checks the weight."""
    reference = _walk(SERIES, albedo=albedo)
    means = [reference[last][0] for last in SERIES]
    gap = min(b - a for a, b in zip(means, means[1:]))
    assert gap >= 0.02 and all(_tolerance(reference[last][1]) <= gap / 4 for last in SERIES), (means, gap)
    assert abs(_walk(SERIES, albedo=1.0)[12][0] - _walk(SERIES, albedo=0.8)[12][0]) >= 0.2
    _compare(_scene(_built(albedo=albedo)[0]), reference, SERIES)


# ---------------------------------------------------------------------------------------------- C: the medium stack
@pytest.mark.gpu
def test_nested_containers_keep_the_outer_medium():
    """C: an inner container (R = 0.45, sigma' = 6) inside the sphere.  Leaving the inner one, the stack is back in the outer
    gas; "leaving anything clears the medium" (VolumePathTracer's rule) is in no medium until the path leaves the outer
    sphere.  The walk: 1.034 and 1.078 with the stack, 0.981 and 0.985 with the single pointer."""
    windows = (12, 40)
    reference = _walk(windows, inner="container", inner_sigma=6.0)
    wrong = _walk(windows, stack_rule="clear", inner="container", inner_sigma=6.0)
    for last in windows:
        gap = abs(reference[last][0] - wrong[last][0])
        assert gap >= 0.04 and _tolerance(reference[last][1]) <= gap / 4, (last, reference[last], wrong[last])
    _compare(_scene(_built(inner="container", inner_sigma=6.0)[0]), reference, windows)


# ---------------------------------------------------------------------------------------------- D: surface <-> scatter
@pytest.mark.gpu
def test_surface_and_scatter_interactions_alternate():
    """D: a Lambertian ball (rho = 0.5, R = 0.45) inside the gas, window (40, 40): no bounce-0 term and no surface lighting
    counts (no walk stands on the ball at bounce 40: asserted in _walk), only the scatter terms, each carrying rho for every
    visit of the ball before it.  A modulation multiplied by a stale BSDF sample after a scatter event, or not multiplied after
    a surface, moves the mean by more than the gap to rho = 1.  The walk: 0.835, and 0.878 at rho = 1."""
    reference = _walk((40,), start_bounce=40, inner="lambertian", rho=0.5)
    white = _walk((40,), start_bounce=40, inner="lambertian", rho=1.0)
    gap = abs(reference[40][0] - white[40][0])
    assert gap >= 0.03 and _tolerance(reference[40][1]) <= gap / 4, (reference, white)
    _compare(_scene(_built(inner="lambertian", rho=0.5)[0]), reference, (40,), start_bounce=40)


# ---------------------------------------------------------------------------------------------- E: grid media
BOX = ((-0.8, -0.7, -0.6), (0.8, 0.7, 0.6))


@pytest.mark.gpu
def test_grid_medium_against_the_walk_over_its_box():
    """E: a box container equal to the grid's bounds, constant density 0.5 x scale 4 = 2, albedo 1: k_path_scatter_grid.
    (0, 3) and (0, 12) differ by the higher orders, as in B."""
    from pathed_amd.integrator import HipScene
    windows = (3, 12)
    reference = _walk(windows, box=BOX)
    gap = reference[12][0] - reference[3][0]
    assert gap >= 0.04 and all(_tolerance(reference[last][1]) <= gap / 4 for last in windows), reference
    built, gas = _built(box=BOX)
    grid = dict(data=np.full((5, 6, 7), 0.5, dtype=np.float32), bounds=BOX[0] + BOX[1], albedo=1.0, scale=4.0)
    desc = built.finish()
    gpu = HipScene(desc, device=0)
    gpu.set_grid_medium(gas, **grid)
    gpu.set_integrator("BasicVolumeIntegrator")
    _compare(gpu, reference, windows)
    image = gpu.render(7, 0, 4, 0, 12)
    for rows in (8, 16, 22):      # the tree-walked grid kernels: the same image
        walked = HipScene(desc, device=0, stack_rows=rows, intersector="bvh")
        walked.set_grid_medium(gas, **grid)
        walked.set_integrator("BasicVolumeIntegrator")
        assert np.array_equal(walked.render(7, 0, 4, 0, 12), image), rows
        assert walked.stats()["path_kernel"] == 9 and walked.stats()["dropped_samples"] == 0


# ---------------------------------------------------------------------------------------------- F: the phase function
@pytest.mark.gpu
def test_phase_samples_against_the_float64_formula():
    """F: Phase::sample = UniformSampleSphere (src/monte_carlo.cpp:43-52) on 4 096 scripted pairs, the ends of [0, 1) and their
    neighbours among them: 1e-6 relative / 2e-7 absolute (the function-level tolerance, ocml sinf / cosf on the path), the
    component order (x, z, y), unit length."""
    from pathed_amd.integrator import HipScene, PathedError
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    special = np.array([0.0, np.nextafter(np.float32(0.0), np.float32(1.0)), 1e-7, 0.25, np.nextafter(np.float32(0.5), np.float32(0.0)), 0.5,
                        np.nextafter(np.float32(0.5), np.float32(1.0)), 0.75, np.nextafter(below_one, np.float32(0.0)), below_one], dtype=np.float32)
    pairs = np.array([(a, b) for a in special for b in special], dtype=np.float32)
    rng = np.random.default_rng(3)
    u = np.concatenate([pairs, rng.random((4096 - len(pairs), 2), dtype=np.float32)])
    gpu = HipScene(_gas_scene(1.0, 8, 8).finish(), device=0)
    found = gpu.phase_samples(u).astype(np.float64)
    # The formula in float64 on the float32 values the reference's statements define: z = u * 2.f - 1, z * z (1 - z * z cancels:
    # near the poles the rounding of z * z, half an ulp of 1, is a relative error of 3e-8 / (1 - z^2) in r whoever computes
    # it in float, so the float64 formula takes the rounded product as its input), and phi = 2 * M_PI * u narrowed once.
    z32 = u[:, 0] * np.float32(2.0) - np.float32(1.0)
    z, zz = z32.astype(np.float64), (z32 * z32).astype(np.float64)
    r = np.sqrt(np.maximum(0.0, 1.0 - zz))
    phi = (2.0 * np.pi * u[:, 1].astype(np.float64)).astype(np.float32).astype(np.float64)      # 2 * M_PI * u, narrowed once
    expected = np.stack([r * np.cos(phi), z, r * np.sin(phi)], axis=1)
    assert found.shape == (4096, 3)
    error = np.abs(found - expected)
    exact = np.stack([np.sqrt(np.maximum(0.0, 1.0 - z * z)) * np.cos(phi), z, np.sqrt(np.maximum(0.0, 1.0 - z * z)) * np.sin(phi)], axis=1)
    print("largest error %.3e; against the formula with an exact z * z %.3e" % (error.max(), np.abs(found - exact).max()))
    assert (error <= 1e-6 * np.abs(expected) + 2e-7).all(), float(error.max())
    assert np.array_equal(found[:, 1], z)      # the middle component is z: (x, z, y)
    assert np.abs(np.linalg.norm(found, axis=1) - 1.0).max() <= 1e-6
    with pytest.raises(PathedError):
        gpu.phase_samples([[0.5, 1.5]])
