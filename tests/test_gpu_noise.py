"""Per-pixel second moments (pathed_hip_render_moments[_device]), the noise figure (pathed_hip_noise_estimate_device) and jobs
that stop on it.  The expected square sums use no new code: every sample is rendered alone with the existing `render`, and
the squares are chained in numpy float32 (tests/noise_reference.py).  24 x 16 = 384 pixels: one full 256-lane block and a
half; 5 samples: the resolve kernel's single-entry loop (fewer than the 8 entries it loads at a time)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_reference

pytestmark = pytest.mark.gpu

F = np.float32
WIDTH, HEIGHT, SPP, SEED = 24, 16, 5, 7
WINDOW = (0, 6)


# ------------------------------------------------------------------------------------------------------------- scenes

def _cornell():
    """scenes/cornell.json: 36 triangles, the fused kernel"""
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene("scenes/cornell.json", WIDTH, HEIGHT)
    return scene, scene.desc, {}, None


def _wavy(built, n, material):
    ys, xs = np.mgrid[0:n + 1, 0:n + 1]
    x = (xs / n * 3 - 1.5).astype(F)
    z = (ys / n * 3 - 1.5).astype(F)
    y = (0.4 + 0.25 * np.sin(2.5 * x) * np.cos(2.0 * z)).astype(F)
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            faces += [(a, c, b), (a, d, c)]
    built.mesh(np.stack([x, y, z], axis=-1).reshape(-1, 3), faces, material)


def _room(environment=False, n=8):
    """a floor, a back wall and a wavy sheet of 2 n^2 triangles under an area light (or, environment=True, under an
    environment map and nothing that emits): 65 .. 4096 triangles, no spheres"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(WIDTH, HEIGHT, origin=(0.3, 2.2, 4.2), target=(0, 0.4, 0), fov_degrees=45.0)
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], built.material(diffuse=(0.7, 0.6, 0.5)))                      # faces up
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 2.4, -2), (-2, 2.4, -2)], built.material(type_=_capi.MAT_PLASTIC, diffuse=(0.6, 0.1, 0.1), alpha=0.2))   # faces the camera
    _wavy(built, n, built.material(diffuse=(0.2, 0.5, 0.7)))
    if environment:
        built.environment(np.random.default_rng(11).random((16, 32, 4)).astype(F), scale=1.5)
    else:
        built.quad([(-0.5, 3.0, -0.5), (0.5, 3.0, -0.5), (0.5, 3.0, 0.5), (-0.5, 3.0, 0.5)], built.material(emit=(8, 8, 8)))   # faces down
    assert 65 <= len(built.indices) <= 4096
    return built, built.finish(), {}, None


def _gas():
    """volume_scenes.nested_scene: two homogeneous containers inside the emissive room"""
    import volume_scenes
    built = volume_scenes.nested_scene(width=WIDTH, height=HEIGHT)
    return built, built.finish(), {}, "VolumePathTracer"


GRID_BOX = ((-0.8, -0.7, -0.6), (0.8, 0.7, 0.6))


def _grid():
    """a box container whose medium is a voxel grid, under a white environment (the scene of tests/test_gpu_basic_volume.py E)"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(WIDTH, HEIGHT, (0, 0, 4.0), (0, 0, 0), fov_degrees=30.0)
    gas = built.medium((2.0,) * 3, (2.0,) * 3)
    built.box(GRID_BOX[0], GRID_BOX[1], built.material(type_=_capi.MAT_PASSTHROUGH), medium=gas)
    built.environment(np.ones((32, 64, 4), dtype=F), scale=1.0)
    data = (0.2 + 0.6 * np.random.default_rng(4).random((5, 6, 7))).astype(F)
    built.grid = (gas, dict(data=data, bounds=GRID_BOX[0] + GRID_BOX[1], albedo=0.9, scale=4.0))
    return built, built.finish(), {}, "BasicVolumeIntegrator"


# organisation -> (scene, HipScene options, PathedStats.path_kernel that proves which kernel ran)
ORGANISATIONS = {
    "fused": (_cornell, {}, 3),
    "hybrid": (_room, {}, 7),
    "wave": (_room, {"shade_kernel": "wave"}, 6),
    "wavefront-1-pool": (_room, {"shade_kernel": "per-slot", "pools": 1}, 1),
    "wavefront-2-pools": (_room, {"shade_kernel": "per-slot", "pools": 2}, 1),
    "wavefront-environment": (lambda: _room(environment=True), {"shade_kernel": "per-slot"}, 1),
    "volume": (_gas, {}, 4),
    "multiple-scattering": (_grid, {}, 9),
}


def _make(name, **more):
    from pathed_amd.integrator import HipScene
    builder, options, kernel = ORGANISATIONS[name]
    keep, desc, _, integrator = builder()
    gpu = HipScene(desc, device=0, **dict(options, **more))
    if getattr(keep, "grid", None):
        gpu.set_grid_medium(keep.grid[0], **keep.grid[1])
    if integrator:
        gpu.set_integrator(integrator)
    gpu._keep = keep
    return gpu, kernel


def _per_sample(gpu, first, count):
    """the colours of samples first .. first + count - 1, each rendered alone by the existing render call: (count, H, W, 3)"""
    return np.stack([gpu.render(SEED, s, 1, *WINDOW) for s in range(first, first + count)])


_cornell_cache = {}


def _cornell_case():
    """the fused Cornell case, rendered once: (gpu, per-sample colours, sums, square sums) -- read-only for every test"""
    if not _cornell_cache:
        gpu, kernel = _make("fused")
        samples = _per_sample(gpu, 0, SPP)
        sums, squares = gpu.render_moments(SEED, 0, SPP, *WINDOW)
        assert gpu.stats()["path_kernel"] == kernel
        for array in (samples, sums, squares):
            array.setflags(write=False)
        _cornell_cache.update(gpu=gpu, samples=samples, sums=sums, squares=squares)
    return _cornell_cache["gpu"], _cornell_cache["samples"], _cornell_cache["sums"], _cornell_cache["squares"]


# -------------------------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("name, spp", [(name, SPP) for name in sorted(ORGANISATIONS)] + [("wavefront-2-pools", 6)])
def test_moments_match_per_sample_renders(name, spp):
    """Per kernel organisation: the square sums are the fp32 chain q = q + c_s * c_s over the colours of the samples rendered
    alone, the sums are the existing render's, both bit for bit.  (A pass of fewer than 4 x 256 units per pool runs on ONE
    pool whatever `pools` says: 384 x 5 = 1920 < 2048, so the extra six-sample case is the one that splits its units over
    two pools.)"""
    gpu, kernel = _make(name)
    samples = _per_sample(gpu, 0, spp)
    expected_sum = gpu.render(SEED, 0, spp, *WINDOW)
    assert expected_sum.any() and np.isfinite(samples).all()
    assert (samples.reshape(spp, -1).max(axis=1) > 0).all()          # every sample carries light somewhere
    sums, squares = gpu.render_moments(SEED, 0, spp, *WINDOW)
    stats = gpu.stats()
    assert stats["path_kernel"] == kernel and stats["dropped_samples"] == 0, stats
    assert np.array_equal(sums, expected_sum)
    assert np.array_equal(squares, noise_reference.square_sums(samples))
    assert np.array_equal(sums, noise_reference.sums(samples))       # (the reference's order: one sample after the other)


def test_calls_and_passes_continue_the_sums():
    from pathed_amd.integrator import HipScene
    gpu, samples, sums, squares = _cornell_case()
    floats = sums.size
    out = np.zeros((2,) + sums.shape, dtype=F)

    def run(scene, calls, start=None):
        buffers = [scene.device_buffer(floats, None if start is None else start[k]) for k in range(2)]
        try:
            for first, count in calls:
                scene.render_moments_device(SEED, first, count, *WINDOW, buffers[0], buffers[1])
            return [scene.download_device_buffer(buffers[k], out[k].copy()) for k in range(2)]
        finally:
            for pointer in buffers:
                scene.free_device_buffer(pointer)

    # 2 + 3 samples in two calls are the 5 of one
    split = run(gpu, [(0, 2), (2, 3)])
    assert np.array_equal(split[0], sums) and np.array_equal(split[1], squares)
    # chunks_per_pass = 2: three internal passes, the last one ragged
    scene = _cornell_cache["gpu"]._keep
    passes = HipScene(scene.desc, device=0, chunks_per_pass=2)
    short = run(passes, [(0, SPP)])
    assert passes.stats()["iterations"] == 3
    assert np.array_equal(short[0], sums) and np.array_equal(short[1], squares)
    # buffers that hold something are continued, not overwritten
    rng = np.random.default_rng(2)
    start = [rng.uniform(0.0, 3.0, size=sums.shape).astype(F) for _ in range(2)]
    continued = run(gpu, [(0, SPP)], start)
    assert np.array_equal(continued[0], noise_reference.sums(samples, start[0]))
    assert np.array_equal(continued[1], noise_reference.square_sums(samples, start[1]))
    # the host-array call ADDS its own sums, like render
    added = gpu.render_moments(SEED, 0, SPP, *WINDOW, accum=start[0].copy(), squares=start[1].copy())
    assert np.array_equal(added[0], (start[0] + sums).astype(F)) and np.array_equal(added[1], (start[1] + squares).astype(F))


def test_argument_errors_launch_nothing():
    from pathed_amd.integrator import PathedError
    gpu, kernel = _make("fused")
    floats = 3 * WIDTH * HEIGHT
    buffers = [gpu.device_buffer(floats) for _ in range(2)]
    try:
        gpu.render_moments_device(SEED, 0, 1, *WINDOW, buffers[0], buffers[1])
        before = gpu.stats()["iterations"]
        assert before > 0
        gpu.set_samples_per_unit(2)
        with pytest.raises(PathedError, match=r"\(-1\).*one sample per unit"):
            gpu.render_moments_device(SEED, 0, 4, *WINDOW, buffers[0], buffers[1])
        gpu.set_samples_per_unit(1)
        gpu.set_integrator("AlbedoIntegrator")
        with pytest.raises(PathedError, match=r"\(-4\).*albedo"):
            gpu.render_moments_device(SEED, 0, 4, *WINDOW, buffers[0], buffers[1])
        gpu.set_integrator("PathTracer")
        with pytest.raises(PathedError, match=r"\(-1\)"):
            gpu.render_moments_device(SEED, 0, 4, *WINDOW, buffers[0], 0)
        with pytest.raises(PathedError, match=r"\(-1\)"):
            gpu.render_moments_device(SEED, 0, 4, *WINDOW, 0, buffers[1])
        with pytest.raises(PathedError, match=r"\(-1\).*2 samples"):
            gpu.noise_estimate(buffers[0], buffers[1], 1)
        with pytest.raises(PathedError, match=r"\(-1\).*floor"):
            gpu.noise_estimate(buffers[0], buffers[1], 4, floor=0.0)
        with pytest.raises(PathedError, match=r"\(-1\)"):
            gpu.noise_estimate(buffers[0], 0, 4)
        noise = gpu._lib.pathed_hip_noise_estimate_device   # a struct of another size
        from pathed_amd import _capi
        wrong = _capi.PathedNoise()
        wrong.struct_size = 8
        assert noise(gpu._handle, buffers[0], buffers[1], 4, 0.01, 0.0, None, C.byref(wrong), None) == -1
        assert gpu.stats()["iterations"] == before
    finally:
        for pointer in buffers:
            gpu.free_device_buffer(pointer)


def test_noise_estimate_against_the_numpy_restatement():
    gpu, samples, sums, squares = _cornell_case()
    sums, squares = sums.copy(), squares.copy()
    sums[0, 0] = 0.0
    squares[0, 0] = 0.0                                            # a pixel no light reached
    expected, invalid = noise_reference.noise(sums, squares, SPP, 0.01)
    assert not invalid.any() and expected[0, 0] == 0.0 and (expected > 0).sum() >= WIDTH * HEIGHT // 2   # (the room's margins are black)
    threshold = float(np.median(expected))
    error = np.full((HEIGHT, WIDTH), -1.0, dtype=F)
    figure = gpu.noise_estimate(sums, squares, SPP, floor=0.01, threshold=threshold, error=error)
    differ = error.view(np.uint32) != expected.view(np.uint32)
    print("pixels whose error differs from the numpy restatement: %d, largest ulp distance %d"
          % (differ.sum(), np.abs(error.view(np.int32).astype(np.int64) - expected.view(np.int32)).max()))
    assert np.array_equal(error, expected)                         # every operation is a correctly rounded fp32 one
    mean = float(expected.astype(np.float64).mean())
    print("mean error %.17g (device) %.17g (float64 mean of the fp32 values)" % (figure["mean_error"], mean))
    assert abs(figure["mean_error"] - mean) <= 1e-12 * mean        # 384 additions at 2^-53 each stay below 1e-13
    assert figure["max_error"] == float(expected.max())
    assert figure["pixels_above"] == int((expected > F(threshold)).sum()) and figure["invalid_pixels"] == 0
    # a square sum that overflowed: the pixel counts as 0 and as invalid
    squares[0, 1, 0] = np.inf
    expected, invalid = noise_reference.noise(sums, squares, SPP, 0.01)
    figure = gpu.noise_estimate(sums, squares, SPP, floor=0.01, threshold=threshold, error=error)
    assert invalid.sum() == 1 and figure["invalid_pixels"] == 1 and error[0, 1] == 0.0 and np.array_equal(error, expected)


# --------------------------------------------------------------------------------------------------------------- jobs

def _read_exr(path):
    from pathed_amd import _capi
    host = _capi.load_host()
    w, h = C.c_int(), C.c_int()
    assert host.pathed_host_read_exr_rgba(path.encode(), C.byref(w), C.byref(h), None, 0) == 0, host.pathed_host_last_error()
    data = np.zeros((h.value, w.value, 4), dtype=F)
    assert host.pathed_host_read_exr_rgba(path.encode(), C.byref(w), C.byref(h), data.ctypes.data_as(C.POINTER(C.c_float)), data.size) == 0
    return data


def _run_job(tmp_path, name, job):
    from pathed_amd import _capi
    out_dir = str(tmp_path / name)
    job = dict(job, output_directory=out_dir)
    job_path = str(tmp_path / (name + ".json"))
    json.dump(job, open(job_path, "w"))
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    return out_dir, result


def _cornell_job(size=32, **keys):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job["width"] = job["height"] = size
    job.update(keys)
    return job


def _assert_stderr_file(path, sums, squares, n):
    """auto-stderr.exr holds sqrt(v_c / n) within HALF's rounding (2^-11 relative + 2^-24 absolute); EXR row 0 is the top scanline"""
    expected = noise_reference.standard_error(sums, squares, n)[::-1]
    found = _read_exr(path)[..., :3]
    assert expected.max() > 0 and np.all(np.abs(found - expected) <= 2.0 ** -11 * expected + 2.0 ** -24)


def test_job_stops_on_noise_self_calibrated(tmp_path):
    """The run is deterministic for a seed, so the target comes from a first run of the same job: its 16-spp figure x 1.0001.
    The second run must then stop at exactly 16 samples with the first run's 16-spp image, and the Python PathTracer stops
    at the same count with the same history."""
    from pathed_amd.integrator import BounceController, HipScene, PathTracer
    from pathed_amd.scene import LoadedScene
    job = _cornell_job(spp=64, stderr_image=True, min_spp=4)
    first_dir, result = _run_job(tmp_path, "first", job)
    assert result.returncode == 0, result.stdout + result.stderr
    metrics = json.load(open(os.path.join(first_dir, "metrics.json")))
    assert metrics["stopped_on_noise"] is False and metrics["last_sample"] == 64
    recorded = {entry["spp"]: entry["mean_error"] for entry in metrics["noise"]}
    assert sorted(recorded) == [4, 8, 16, 32, 64] and all(entry["max_error"] >= entry["mean_error"] > 0 for entry in metrics["noise"])
    target = recorded[16] * 1.0001
    print("noise figures of the first run:", recorded, "target", target)
    assert recorded[8] > target and recorded[4] > target            # the precondition: no earlier checkpoint is clean enough
    for n in (2, 16, 64):
        assert os.path.exists(os.path.join(first_dir, "auto-stderr-%05dspp.exr" % n))
    assert not os.path.exists(os.path.join(first_dir, "auto-stderr-00001spp.exr"))   # one sample has no spread

    second_dir, result = _run_job(tmp_path, "second", dict(job, target_noise=target))
    assert result.returncode == 0, result.stdout + result.stderr
    stopped = json.load(open(os.path.join(second_dir, "metrics.json")))
    assert stopped["stopped_on_noise"] is True and stopped["last_sample"] == 16
    assert [(entry["spp"], entry["mean_error"]) for entry in stopped["noise"]] == [(n, recorded[n]) for n in (4, 8, 16)]
    assert "sample: 16/64" in result.stdout and "sample: 32/64" not in result.stdout and "noise target" in result.stdout
    assert open(os.path.join(second_dir, "auto.exr"), "rb").read() == open(os.path.join(first_dir, "auto-00016spp.exr"), "rb").read()
    assert not os.path.exists(os.path.join(second_dir, "auto-00032spp.exr"))

    # auto-stderr.exr against the library's own sums
    scene = LoadedScene(job["scene"], 32, 32)
    gpu = HipScene(scene.desc, device=0)
    sums, squares = gpu.render_moments(job.get("seed", 1), 0, 16, job["startBounce"], job["lastBounce"])
    _assert_stderr_file(os.path.join(second_dir, "auto-stderr.exr"), sums, squares, 16)
    assert open(os.path.join(second_dir, "auto-stderr.exr"), "rb").read() == open(os.path.join(first_dir, "auto-stderr-00016spp.exr"), "rb").read()

    # the Python integrator: the same count, the same history
    tracer = PathTracer(BounceController(job["startBounce"], job["lastBounce"]), spp=64, seed=job.get("seed", 1), target_noise=target, min_spp=4)
    image = np.zeros((32, 32, 3), dtype=F)
    counts = []
    tracer.run(image, gpu, callback=lambda done, checkpoint: counts.append(done))
    assert counts[-1] == 16 and tracer.stopped_on_noise
    assert tracer.noise_history == [(n, recorded[n]) for n in (4, 8, 16)]
    assert np.array_equal(image, sums / F(16))

    # the one-process-per-GPU runner keeps no second moments: it refuses the keys by name
    from pathed_amd import _capi
    job_path = str(tmp_path / "runner.json")
    json.dump(dict(job, output_directory=str(tmp_path / "runner"), target_noise=target), open(job_path, "w"))
    result = subprocess.run([sys.executable, "-m", "pathed_amd.run_job", job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=_capi.REPO_ROOT)
    assert result.returncode != 0 and "target_noise" in result.stderr and not os.path.exists(str(tmp_path / "runner"))


def test_two_replicas_sum_their_squares(tmp_path):
    """"gpus": [0, 0]: two replicas on one GPU, peer copies.  Each keeps its own sums and squares over its share of every
    batch; the totals the job estimates and writes are those of two scenes that render the same shares here."""
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene

    def strong_range(rank, world_size, first, count):   # pathed_amd/parallel.py's rule (that module imports torch: seconds)
        base, extra = divmod(count, world_size)
        return first + rank * base + min(rank, extra), base + (1 if rank < extra else 0)

    job = _cornell_job(spp=16, stderr_image=True, min_spp=4, gpus=[0, 0], reduce="peer-copy", metrics="basic")   # (no attempt at RCCL, no counting pass)
    out_dir, result = _run_job(tmp_path, "two", job)
    assert result.returncode == 0, result.stdout + result.stderr
    metrics = json.load(open(os.path.join(out_dir, "metrics.json")))
    assert metrics["reduce_method"] == "peer-copy" and metrics["last_sample"] == 16

    scene = LoadedScene(job["scene"], 32, 32)
    replicas = [HipScene(scene.desc, device=0) for _ in range(2)]
    shape = (32, 32, 3)
    held = [[np.zeros(shape, dtype=F), np.zeros(shape, dtype=F)] for _ in range(2)]
    buffers = [[gpu.device_buffer(3 * 32 * 32) for _ in range(2)] for gpu in replicas]
    try:
        done = 0
        while done < 16:
            next_power = 1
            while next_power <= done:
                next_power *= 2
            count = min(16, next_power) - done
            for r, gpu in enumerate(replicas):
                begin, mine = strong_range(r, 2, done, count)
                if mine:
                    gpu.render_moments_device(job.get("seed", 1), begin, mine, job["startBounce"], job["lastBounce"], buffers[r][0], buffers[r][1])
            done += count
        for r, gpu in enumerate(replicas):
            for k in range(2):
                gpu.download_device_buffer(buffers[r][k], held[r][k])
    finally:
        for r, gpu in enumerate(replicas):
            for pointer in buffers[r]:
                gpu.free_device_buffer(pointer)
    sums = (held[0][0] + held[1][0]).astype(F)
    squares = (held[0][1] + held[1][1]).astype(F)
    assert held[1][1].any()
    _assert_stderr_file(os.path.join(out_dir, "auto-stderr.exr"), sums, squares, 16)
    figure = replicas[0].noise_estimate(sums, squares, 16, floor=0.01)
    assert [entry["spp"] for entry in metrics["noise"]] == [4, 8, 16]
    assert metrics["noise"][-1]["mean_error"] == figure["mean_error"] and metrics["noise"][-1]["max_error"] == figure["max_error"]
    # ... and against one replica's: the same samples, fp32 summation order apart (the bound of the two-replica job test)
    single_sums, single_squares = replicas[0].render_moments(job.get("seed", 1), 0, 16, job["startBounce"], job["lastBounce"])
    assert np.linalg.norm(sums - single_sums) / np.linalg.norm(single_sums) < 1e-6
    assert np.linalg.norm(squares - single_squares) / np.linalg.norm(single_squares) < 1e-6
