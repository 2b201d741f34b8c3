"""Participating media: the reference's VolumePathTracer (src/volume_path_tracer.cpp) with
DirectLightingHelper::Ld, VolumeHelper and HomogeneousMedium, as k_path_volume (pathed_amd/csrc/volume.h).

Parity status: UNPINNED.  The reference's volumetric ray queries run through an Embree intersection filter
(src/scene.cpp:42-83) and none of these translation units compiles without Embree's header, so the oracle restates
them from the source text and DEFINES the one thing that depends on Embree's traversal order (which container hits
become volume events: oracle/oracle.cpp).  What the tests pin instead:
  * on scenes without media the volume integrator's sums are the path tracer's, bit for bit (the reference's two
    integrators share their direct-lighting arithmetic statement for statement) -- for the oracle and for the kernels;
  * GPU = oracle on scenes with a gas container, a glass sphere inside, area / sphere / environment lights;
  * (tests/test_gpu_volume_queries.py) the volumetric queries and rayTransmission against float64 numbers, on both sides,
    and the tree-walked queries on a container of 1 224 triangles."""
import os

import numpy as np
import pytest


def _gas_scene(sigma, width=48, height=40, env=False, sphere_light=False):
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(width, height, (0, 1.2, 5), (0, 1, 0), fov_degrees=38)
    white = built.material(diffuse=(0.7, 0.7, 0.7))
    red = built.material(diffuse=(0.6, 0.1, 0.1))
    light = built.material(diffuse=(0, 0, 0), emit=(20, 20, 20))
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], white)
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)], red)
    if sphere_light:
        built.sphere((0.0, 2.8, 0.0), 0.2, light)
    else:
        built.quad([(-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (0.5, 2.9, 0.5), (-0.5, 2.9, 0.5)], light)
    gas = built.medium((sigma, sigma, sigma), (sigma, sigma, sigma))
    built.box((-1, 0.2, -1), (1, 2.2, 1), built.material(type_=_capi.MAT_PASSTHROUGH), medium=gas)
    built.sphere((0, 1.0, 0), 0.4, built.material(type_=_capi.MAT_GLASS, ior=1.5))
    if env:
        rgba = np.ones((16, 32, 4), dtype=np.float32) * 0.4
        rgba[4:6, 10:14, :3] = 30.0
        built.environment(rgba, scale=1.0)
    return built


def test_oracle_volume_integrator_equals_its_path_tracer_without_media():
    """The restated VolumePathTracer against the (pinned-by-ground-truth) PathTracer restatement: identical sums."""
    import oracle_lib
    from pathed_amd.scene import LoadedScene
    for path, size, last_bounce in (("scenes/cornell.json", 20, 6), ("scenes/cornell-glass.json", 16, 6), ("scenes/mis-pbrt.json", 20, 4)):
        scene = LoadedScene(path, size, size)
        plain, volume = oracle_lib.OracleScene(scene.desc), oracle_lib.OracleScene(scene.desc)
        volume.set_integrator("VolumePathTracer")
        a, _ = plain.render(size, size, 3, 0, 3, 0, last_bounce, threads=os.cpu_count())
        b, _ = volume.render(size, size, 3, 0, 3, 0, last_bounce, threads=os.cpu_count())
        assert a.any() and np.array_equal(a, b), path


def test_oracle_medium_behaviour():
    """Denser gas: less light reaches the floor behind the container, more is scattered towards the camera inside it;
    sigma = 0 leaves only the passthrough surfaces (which consume bounces but change no radiance)."""
    import oracle_lib
    means = []
    for sigma in (0.0, 0.5, 4.0):
        built = _gas_scene(sigma)
        oracle = oracle_lib.OracleScene(built.finish())
        oracle.set_integrator("VolumePathTracer")
        image, stats = oracle.render(48, 40, 2, 0, 12, 0, 8, threads=os.cpu_count())
        assert np.isfinite(image).all() and stats["dropped"] == 0
        means.append(float(image.mean()))
    assert means[1] != means[0] and means[2] < means[1]      # the gas matters, thick gas absorbs


@pytest.mark.gpu
@pytest.mark.parametrize("scene_path,size,spp,last_bounce", [
    ("scenes/cornell.json", 64, 8, 10), ("scenes/cornell-glass.json", 48, 6, 8), ("scenes/mis-pbrt.json", 64, 6, 5),
    ("scenes/teapot.json", 48, 4, 6), ("test_scenes/environment_map_sampling.json", 48, 6, 4),
])
def test_volume_kernel_equals_the_path_tracer_kernels_without_media(scene_path, size, spp, last_bounce):
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene(scene_path, size, size)
    plain = HipScene(scene.desc, device=0)
    # generic_kernels: k_path_volume itself; by default a scene without media or containers under VolumePathTracer takes the
    # path tracer's kernels (the two integrators are the same estimator there -- which is what this test establishes)
    volume = HipScene(scene.desc, device=0, generic_kernels=1)
    volume.set_integrator("VolumePathTracer")
    generic = HipScene(scene.desc, device=0, generic_kernels=1)
    expected = generic.render(5, 2, spp, 0, last_bounce)
    assert expected.any() and volume.stats()["path_kernel"] == 4
    assert np.array_equal(plain.render(5, 2, spp, 0, last_bounce), expected)
    assert np.array_equal(volume.render(5, 2, spp, 0, last_bounce), expected)
    assert np.array_equal(volume.render(5, 0, 3, 1, 2), plain.render(5, 0, 3, 1, 2))      # a bounce window
    dispatched = HipScene(scene.desc, device=0)
    dispatched.set_integrator("VolumePathTracer")
    assert dispatched.stats()["path_kernel"] in (1, 3)
    assert np.array_equal(dispatched.render(5, 2, spp, 0, last_bounce), expected)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,env,sphere_light", [(0.0, False, False), (0.5, False, False), (2.0, False, True), (1.0, True, False)])
def test_volume_kernel_matches_the_oracle_with_media(sigma, env, sphere_light):
    import oracle_lib
    from pathed_amd.integrator import HipScene, PathedError
    built = _gas_scene(sigma, env=env, sphere_light=sphere_light)
    desc = built.finish()
    gpu = HipScene(desc, device=0)
    with pytest.raises(PathedError):
        gpu.render(1, 0, 1, 0, 4)          # passthrough surfaces: only the volume integrator renders the scene
    gpu.set_integrator("VolumePathTracer")
    oracle = oracle_lib.OracleScene(desc)
    oracle.set_integrator("VolumePathTracer")
    image = gpu.render(4, 0, 16, 0, 8)
    expected, stats = oracle.render(48, 40, 4, 0, 16, 0, 8, threads=os.cpu_count())
    rel = float(np.linalg.norm(image - expected) / np.linalg.norm(expected))
    bad = float((np.abs(image - expected) > 1e-2 * np.maximum(np.abs(expected), 1e-3)).any(axis=2).mean())
    assert rel <= 1e-2 and bad <= 5e-3, (rel, bad)      # a glass sphere inside: a flipped Fresnel decision changes a path
    assert stats["dropped"] == 0 and gpu.stats()["dropped_samples"] == 0
    # the tree walk (volumeQuery) instead of the all-triangles intersector, eight LDS stack rows: same image.  This 18-triangle
    # tree is too shallow to overflow eight rows; the spill to HBM is tested on a deep tree in test_gpu_volume_queries.py
    # (test_room_stack_rows_agree_and_eight_rows_spill)
    walked = HipScene(desc, device=0, stack_rows=8, intersector="bvh")
    walked.set_integrator("VolumePathTracer")
    assert np.array_equal(walked.render(4, 0, 16, 0, 8), image)


@pytest.mark.gpu
def test_reference_cornell_medium_scene_matches_the_oracle():
    """scenes/cornell-medium.json is the reference's own VolumePathTracer scene (unmodified; its two OBJs are absent
    upstream and generated by tools/make_assets.py): gas container, glass sphere inside, the Cornell room around it."""
    import oracle_lib
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    size, spp = 64, 16
    scene = LoadedScene("scenes/cornell-medium.json", size, size)
    desc = scene.desc.contents
    assert desc.n_media == 1 and desc.n_spheres == 1 and desc.geoms[0].medium == 0
    gpu = HipScene(scene.desc, device=0)
    gpu.set_integrator("VolumePathTracer")
    oracle = oracle_lib.OracleScene(scene.desc)
    oracle.set_integrator("VolumePathTracer")
    image = gpu.render(1, 0, spp, 0, 10)
    expected, stats = oracle.render(size, size, 1, 0, spp, 0, 10, threads=os.cpu_count())
    rel = float(np.linalg.norm(image - expected) / np.linalg.norm(expected))
    bad = float((np.abs(image - expected) > 1e-2 * np.maximum(np.abs(expected), 1e-3)).any(axis=2).mean())
    assert rel <= 1e-2 and bad <= 5e-3, (rel, bad)
    assert stats["dropped"] == 0 and gpu.stats()["dropped_samples"] == 0 and gpu.stats()["path_kernel"] == 4
    # the gas glows under the light: the column below it is brighter than the room's far corners seen through the gas
    mean = image / spp
    assert mean[size // 2:, size // 2 - 4:size // 2 + 4].mean() > mean[: size // 4, : size // 4].mean()


@pytest.mark.gpu
def test_volume_job_through_the_host_executable(tmp_path):
    """job.json "integrator": "VolumePathTracer" + scene JSON "media" / "internal_medium" / "passthrough" (reference
    src/job.cpp:71-72, src/scene_parser.cpp:202-229, 324-337, 593-594) through the C++ host."""
    import json
    import subprocess
    from pathed_amd import _capi
    scene = {
        "sensor": {"lookAt": {"origin": ["0", "1", "6.8"], "target": ["0", "1", "0"], "up": ["0", "1", "0"]}, "fov": "19.5"},
        "media": [{"name": "gas", "type": "homogeneous", "sigma_t": ["1.0", "1.0", "1.0"], "sigma_s": ["1.0", "1.0", "1.0"]}],
        "models": [
            {"type": "obj", "filename": "scenes/cornell-glossy/ball.obj", "internal_medium": "gas", "bsdf": {"type": "passthrough"},
             "transform": {"scale": ["0.8", "0.8", "0.8"], "translate": ["0", "0.2", "0"]}},
            {"type": "sphere", "radius": "0.25", "center": ["0.0", "0.9", "0.0"], "bsdf": {"type": "glass"}},
            {"type": "obj", "filename": "scenes/CornellBox-Original.obj"},
        ],
    }
    scene_path = str(tmp_path / "medium.json")
    json.dump(scene, open(scene_path, "w"))
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(scene=scene_path, integrator="VolumePathTracer", width=48, height=48, spp=4, output_directory=str(tmp_path / "out"))
    job_path = str(tmp_path / "job.json")
    json.dump(job, open(job_path, "w"))
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode == 0, result.stdout + result.stderr
    assert os.path.exists(os.path.join(str(tmp_path / "out"), "auto-00004spp.exr"))
    job["integrator"] = "PathTracer"          # the plain path tracer refuses a scene with containers
    json.dump(job, open(job_path, "w"))
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode != 0 and "VolumePathTracer" in (result.stdout + result.stderr)
