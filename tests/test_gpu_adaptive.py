"""Adaptive sampling: render calls over a list of pixels (pathed_hip_render_pixels_device), the selection of the pixels that
are still noisy (pathed_hip_select_pixels_device) and the rounds both hosts drive with them.  The expected values use no new
code: a listed pixel must hold what the moments render of the whole image gives it, and the selection is restated in numpy
(tests/adaptive_reference.py).  Scenes, options and sizes are those of tests/test_gpu_noise.py: 24 x 16 = 384 pixels, one full
256-lane block and a half."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_reference
import noise_reference
import test_gpu_noise
from test_gpu_noise import HEIGHT, ORGANISATIONS, SEED, SPP, WIDTH, WINDOW, _make, _read_exr, _run_job

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
PIXELS = WIDTH * HEIGHT
# what the buffers hold before a call: 0.1f, 0.2f and a count no render reaches
SUM_BITS, SQUARE_BITS, COUNT_BITS = 0x3DCCCCCD, 0x3E4CCCCD, 0x00ABC123


def _lists():
    rng = np.random.default_rng(5)
    return {
        "first": np.array([0], dtype=U),
        "last": np.array([PIXELS - 1], dtype=U),
        "every-other": np.arange(0, PIXELS, 2, dtype=U),
        "65": np.sort(rng.choice(PIXELS, 65, replace=False)).astype(U),          # one more than a wave
        "191-of-384": np.sort(rng.choice(PIXELS, 191, replace=False)).astype(U),
        "all": np.arange(PIXELS, dtype=U),
    }


class Buffers:
    """the three images of a list render on the device, pre-filled with the bit patterns, and room for a list"""

    def __init__(self, gpu, pixels=PIXELS):
        self.gpu, self.pixels = gpu, pixels
        self.sums = gpu.device_words(3 * pixels, np.full(3 * pixels, SUM_BITS, dtype=U))
        self.squares = gpu.device_words(3 * pixels, np.full(3 * pixels, SQUARE_BITS, dtype=U))
        self.counts = gpu.device_words(pixels, np.full(pixels, COUNT_BITS, dtype=U))
        self.list = gpu.device_words(pixels)

    def set_list(self, entries):
        """uploads the list (a fresh buffer: device_words fills on allocation)"""
        self.gpu.free_device_buffer(self.list)
        entries = np.asarray(entries, dtype=U)
        padded = np.zeros(max(self.pixels, entries.size), dtype=U)
        padded[:entries.size] = entries
        self.list = self.gpu.device_words(padded.size, padded)
        return entries.size

    def read(self):
        """(sums (P, 3), squares (P, 3), counts (P,)) as uint32 bit patterns"""
        sums = self.gpu.download_device_words(self.sums, np.zeros(3 * self.pixels, dtype=U)).reshape(-1, 3)
        squares = self.gpu.download_device_words(self.squares, np.zeros(3 * self.pixels, dtype=U)).reshape(-1, 3)
        counts = self.gpu.download_device_words(self.counts, np.zeros(self.pixels, dtype=U))
        return sums, squares, counts

    def free(self):
        for pointer in (self.sums, self.squares, self.counts, self.list):
            self.gpu.free_device_buffer(pointer)


# ------------------------------------------------------------------------------------------------------- list renders

CASES = [(name, SPP, {}) for name in sorted(ORGANISATIONS)] + [("wavefront-2-pools", 6, {}), ("fused", SPP, {"chunks_per_pass": 2})]


@pytest.mark.parametrize("name, spp, more", CASES, ids=["%s-%d%s" % (n, s, "-3-passes" if m else "") for n, s, m in CASES])
def test_list_renders_are_the_full_renders_bits(name, spp, more):
    """Per kernel organisation and list: after a list render over buffers that hold a bit pattern, a listed pixel holds what
    the moments render of the whole image -- on the scene's own path kernel -- leaves there from the same pattern: sums and
    squares, bit for bit, and pattern + spp samples; every other pixel keeps the pattern in every bit.  3 + 2 samples in two
    list calls are the 5 of one.  The list passes themselves run on the only kernels that know the list order (kernels.h: THE
    UNIT ORDER says why): the wavefront (path_kernel 1), and for scenes on the volume integrators' kernels k_list_volume
    (path_kernel 4 and 9, as their other calls report)."""
    gpu, kernel = _make(name, **more)
    full = Buffers(gpu)
    try:
        gpu.render_moments_device(SEED, 0, spp, *WINDOW, full.sums, full.squares)
        expected_sums, expected_squares, _ = full.read()
        first3 = Buffers(gpu)                                   # ... and the state after the first three samples, for the split
        gpu.render_moments_device(SEED, 0, 3, *WINDOW, first3.sums, first3.squares)
        after3 = first3.read()
        first3.free()
    finally:
        full.free()
    assert gpu.stats()["path_kernel"] == kernel
    assert (expected_sums != SUM_BITS).any(axis=1).sum() > PIXELS // 2          # the render carries light
    for label, entries in _lists().items():
        listed = np.zeros(PIXELS, dtype=bool)
        listed[entries] = True
        buffers = Buffers(gpu)
        try:
            n_list = buffers.set_list(entries)
            before = gpu.stats()["iterations"]
            gpu.render_pixels(SEED, 0, spp, *WINDOW, buffers.list, n_list, buffers.sums, buffers.squares, buffers.counts)
            stats = gpu.stats()
            assert stats["path_kernel"] == (kernel if kernel in (4, 9) else 1) and stats["dropped_samples"] == 0 and stats["iterations"] > before, (label, stats)
            sums, squares, counts = buffers.read()
            assert np.array_equal(sums[listed], expected_sums[listed]), label
            assert np.array_equal(squares[listed], expected_squares[listed]), label
            assert (counts[listed] == COUNT_BITS + spp).all(), label
            assert (sums[~listed] == SUM_BITS).all() and (squares[~listed] == SQUARE_BITS).all() and (counts[~listed] == COUNT_BITS).all(), label
            if label != "every-other":
                continue
            split = Buffers(gpu)
            try:
                split.set_list(entries)
                gpu.render_pixels(SEED, 0, 3, *WINDOW, split.list, n_list, split.sums, split.squares, split.counts)
                middle = split.read()
                assert np.array_equal(middle[0][listed], after3[0][listed]) and np.array_equal(middle[1][listed], after3[1][listed])
                gpu.render_pixels(SEED, 3, spp - 3, *WINDOW, split.list, n_list, split.sums, split.squares, split.counts)
                for found, whole in zip(split.read(), (sums, squares, counts)):
                    assert np.array_equal(found, whole)
            finally:
                split.free()
        finally:
            buffers.free()


def _media_scene(builder, integrator, **options):
    from pathed_amd.integrator import HipScene
    keep, desc, _, _ = builder()
    gpu = HipScene(desc, device=0, **options)
    if getattr(keep, "grid", None):
        gpu.set_grid_medium(keep.grid[0], **keep.grid[1])
    gpu.set_integrator(integrator)
    gpu._keep = keep
    return gpu


# the instantiations of k_list_volume the organisations above do not reach: (scene, integrator, options, path kernel)
MEDIA_CASES = {
    "grid-single-scattering": (test_gpu_noise._grid, "VolumePathTracer", {}, 4),
    "gas-multiple-scattering": (test_gpu_noise._gas, "BasicVolumeIntegrator", {}, 9),
    "tree-walk-single": (test_gpu_noise._room, "VolumePathTracer", {"generic_kernels": 1}, 4),     # more than 64 triangles: the tree walk
    "tree-walk-multiple": (test_gpu_noise._room, "BasicVolumeIntegrator", {"generic_kernels": 1}, 9),
}


@pytest.mark.parametrize("name", sorted(MEDIA_CASES))
def test_list_renders_of_the_other_volume_kernels(name):
    """k_list_volume with a grid under VolumePathTracer, without one under BasicVolumeIntegrator, and walking a tree: every
    other pixel listed; the same bits as the scene's own kernel gives, the pattern everywhere else."""
    builder, integrator, options, kernel = MEDIA_CASES[name]
    gpu = _media_scene(builder, integrator, **options)
    full, buffers = Buffers(gpu), Buffers(gpu)
    try:
        gpu.render_moments_device(SEED, 0, SPP, *WINDOW, full.sums, full.squares)
        assert gpu.stats()["path_kernel"] == kernel
        expected_sums, expected_squares, _ = full.read()
        assert (expected_sums != SUM_BITS).any(axis=1).sum() > PIXELS // 2
        entries = _lists()["every-other"]
        listed = np.zeros(PIXELS, dtype=bool)
        listed[entries] = True
        n_list = buffers.set_list(entries)
        gpu.render_pixels(SEED, 0, SPP, *WINDOW, buffers.list, n_list, buffers.sums, buffers.squares, buffers.counts)
        stats = gpu.stats()
        assert stats["path_kernel"] == kernel and stats["dropped_samples"] == 0, stats
        sums, squares, counts = buffers.read()
        assert np.array_equal(sums[listed], expected_sums[listed]) and np.array_equal(squares[listed], expected_squares[listed])
        assert (counts[listed] == COUNT_BITS + SPP).all()
        assert (sums[~listed] == SUM_BITS).all() and (squares[~listed] == SQUARE_BITS).all() and (counts[~listed] == COUNT_BITS).all()
    finally:
        full.free()
        buffers.free()


def test_argument_errors_launch_nothing():
    from pathed_amd.integrator import PathedError
    gpu, kernel = _make("fused")
    buffers = Buffers(gpu)
    try:
        gpu.render_moments_device(SEED, 0, 1, *WINDOW, buffers.sums, buffers.squares)
        pristine = buffers.read()
        before = gpu.stats()["iterations"]
        assert before > 0

        def render(n_list, list_pointer=None, sums=None, squares=None, counts=None):
            gpu.render_pixels(SEED, 1, 4, *WINDOW, buffers.list if list_pointer is None else list_pointer, n_list,
                              buffers.sums if sums is None else sums, buffers.squares if squares is None else squares,
                              buffers.counts if counts is None else counts)

        for bad in ([5, 4, 3], [3, 7, 7, 9], [0, 1, PIXELS], [PIXELS - 1, PIXELS - 2]):
            n_list = buffers.set_list(bad)
            with pytest.raises(PathedError, match=r"\(-1\).*strictly ascending"):
                render(n_list)
        n_list = buffers.set_list([1, 2, 3])
        with pytest.raises(PathedError, match=r"\(-1\).*longer"):
            render(PIXELS + 1)
        for null in ("sums", "squares", "counts"):
            with pytest.raises(PathedError, match=r"\(-1\).*null"):
                render(n_list, **{null: 0})
        with pytest.raises(PathedError, match=r"\(-1\).*null pixel list"):
            render(n_list, list_pointer=0)
        gpu.set_samples_per_unit(2)
        with pytest.raises(PathedError, match=r"\(-1\).*one sample per unit"):
            render(n_list)
        gpu.set_samples_per_unit(1)
        gpu.set_integrator("AlbedoIntegrator")
        with pytest.raises(PathedError, match=r"\(-4\).*albedo"):
            render(n_list)
        gpu.set_integrator("PathTracer")
        render(0)                                                  # an empty list: returns 0 ...
        render(0, list_pointer=0)
        assert gpu.stats()["iterations"] == before                 # ... and none of these calls rendered anything
        for found, held in zip(buffers.read(), pristine):
            assert np.array_equal(found, held)
        # the selection's own argument errors
        with pytest.raises(PathedError, match=r"\(-1\).*floor"):
            gpu.select_pixels(buffers.sums, buffers.squares, buffers.counts, buffers.list, floor=0.0)
        with pytest.raises(PathedError, match=r"\(-1\).*null"):
            gpu.select_pixels(buffers.sums, buffers.squares, 0, buffers.list)
        with pytest.raises(PathedError, match=r"\(-1\).*null"):
            gpu.select_pixels(buffers.sums, buffers.squares, buffers.counts, 0)
        # ... and after all that a good list still renders
        render(n_list)
        assert gpu.stats()["iterations"] > before
        assert list(np.flatnonzero(buffers.read()[2] != pristine[2])) == [1, 2, 3]
    finally:
        buffers.free()


# ---------------------------------------------------------------------------------------------------- the selection

def _synthetic(pixels, rng, counts):
    """sums of pixels whose relative noise spreads over two decades: S = n m, Q = n m^2 (1 + r^2) with the pixel's own n"""
    n = np.maximum(counts, 1).astype(np.float64)[:, None]
    m = rng.uniform(0.2, 4.0, size=(pixels, 3))
    r = rng.uniform(0.1, 3.0, size=(pixels, 3)) * rng.choice([0.1, 1.0, 4.0], size=(pixels, 1))
    return (n * m).astype(F), (n * m * m * (1.0 + r * r)).astype(F)


@pytest.mark.parametrize("width, height", [(1, 1), (17, 15), (16, 16), (257, 1), (40, 25), (1920, 1080)])
def test_selection_against_the_numpy_restatement(width, height):
    """1, 255, 256, 257 and 1 000 pixels: both sides of the 256-pixel block; 1920 x 1080 = 2 073 600 pixels, 8 100 blocks: the
    size jobs run it at (the list is built from the host's block offsets; the other sizes have at most 4).  Mixed counts (0, 1, 2, 7, 4 096); thresholds that
    select none but the pixels without a spread, all, and a scattered half.  Errors, list and length exact; the mean to the
    last digit of the double.  With one count everywhere: pathed_hip_noise_estimate_device's results bit for bit."""
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene("scenes/cornell.json", width, height)
    gpu = HipScene(scene.desc, device=0)
    pixels = width * height
    rng = np.random.default_rng(100 + pixels)
    floor = 0.01
    mixed = rng.choice(np.array([0, 1, 2, 7, 4096], dtype=U), size=pixels).astype(U)
    if pixels == 1:
        mixed[:] = 7
    uniform = np.full(pixels, 7, dtype=U)
    held = []

    def on_device(words, host):
        held.append(gpu.device_words(words, host))
        return held[-1]

    try:
        for counts in (mixed, uniform):
            S, Q = _synthetic(pixels, rng, counts)
            if pixels > 3:
                Q[2, 1] = np.inf                                   # a square sum that overflowed
            e, invalid, _ = adaptive_reference.select(S, Q, counts, floor, 0.0)
            valid = e[~invalid]
            half = float(np.median(valid)) if valid.size else 0.0
            sums, squares, count_image = on_device(3 * pixels, S.view(U)), on_device(3 * pixels, Q.view(U)), on_device(pixels, counts)
            error = on_device(pixels, None)
            for threshold in (1e30, -1.0, half):
                expected_e, expected_invalid, expected_list = adaptive_reference.select(S, Q, counts, floor, threshold)
                pixel_list = on_device(pixels + 1, np.full(pixels + 1, 0xFFFFFFFF, dtype=U))
                n_list, figure = gpu.select_pixels(sums, squares, count_image, pixel_list, floor=floor, threshold=threshold, error_pointer=error)
                found_e = gpu.download_device_words(error, np.zeros(pixels, dtype=U)).view(F)
                found_list = gpu.download_device_words(pixel_list, np.zeros(pixels + 1, dtype=U))
                assert np.array_equal(found_e.view(U), expected_e.view(U))
                assert n_list == expected_list.size and np.array_equal(found_list[:n_list], expected_list)
                assert (found_list[n_list:] == 0xFFFFFFFF).all()           # nothing is written behind the list
                print("%d pixels, threshold %g: %d selected, mean %.17g (device) %.17g (numpy)"
                      % (pixels, threshold, n_list, figure["mean_error"], adaptive_reference.mean_error(expected_e)))
                assert figure["mean_error"] == adaptive_reference.mean_error(expected_e)
                assert figure["max_error"] == float(expected_e.max())
                assert figure["pixels_above"] == int((expected_e > F(threshold)).sum()) and figure["invalid_pixels"] == int(expected_invalid.sum())
                if threshold == 1e30:
                    assert n_list == int((counts < 2).sum())
                elif threshold == -1.0:
                    assert n_list == pixels
                elif pixels >= 255:
                    assert pixels // 8 < n_list < 7 * pixels // 8 and (np.diff(expected_list.astype(np.int64)) > 1).sum() > pixels // 16   # scattered
                if counts is uniform:
                    other = on_device(pixels, None)
                    plain = gpu.noise_estimate(sums, squares, 7, floor=floor, threshold=threshold, error=other)
                    assert plain == figure
                    assert np.array_equal(gpu.download_device_words(other, np.zeros(pixels, dtype=U)), found_e.view(U))
    finally:
        for pointer in held:
            gpu.free_device_buffer(pointer)


# --------------------------------------------------------------------------------------------------------- the loop

MIN_SPP, CAP, QUANTILE = 4, 32, 0.5


def test_the_adaptive_loop():
    """Cornell 24 x 16, min_spp 4, cap 32; the target is the median (quantile 0.5) of the error image at 4 samples.  Chosen with
    the CPU oracle's renders of the same scene, seed and window put through tests/adaptive_reference.py: quantile 0.5 gives
    the target 0.1233 and the counts {4: 192, 8: 33, 16: 35, 32: 124} pixels, 5 560 samples of 12 288 (0.4: {4: 154, 8: 25,
    16: 33, 32: 172}; 0.75: {4: 288, 8: 46, 16: 33, 32: 17}; below 0.3 the quantile is 0 -- a third of the image is the
    black margin -- and only 4 and 32 occur).  The GPU's renders differ from the oracle's in the last bits, not in this."""
    from pathed_amd.integrator import BounceController, PathTracer
    gpu, kernel = _make("fused")
    uniform = {}
    for count in (4, 8, 16, 32):
        sums, squares = gpu.render_moments(SEED, 0, count, *WINDOW)
        uniform[count] = (sums.reshape(-1, 3), squares.reshape(-1, 3))
    at_min, _ = noise_reference.noise(uniform[MIN_SPP][0], uniform[MIN_SPP][1], MIN_SPP, 0.01)
    target = float(np.quantile(at_min, QUANTILE))
    result = gpu.render_adaptive(SEED, CAP, *WINDOW, target, min_spp=MIN_SPP, floor=0.01)
    counts = result["counts"].reshape(-1)
    histogram = dict(zip(*[x.tolist() for x in np.unique(counts, return_counts=True)]))
    print("target %.6g, counts %s, %d samples of %d, %d rounds" % (target, histogram, result["samples_rendered"], CAP * PIXELS, result["rounds"]))
    assert len(histogram) >= 3 and histogram.get(MIN_SPP, 0) > 0 and histogram.get(CAP, 0) > 0
    for count in histogram:
        where = counts == count
        assert np.array_equal(result["sums"].reshape(-1, 3)[where].view(U), uniform[count][0][where].view(U)), count
        assert np.array_equal(result["squares"].reshape(-1, 3)[where].view(U), uniform[count][1][where].view(U)), count
    expected_counts, rounds, rendered = adaptive_reference.replay(uniform, MIN_SPP, CAP, target, 0.01)
    assert np.array_equal(counts, expected_counts) and result["rounds"] == rounds and result["samples_rendered"] == rendered
    assert int(counts.sum()) == rendered and rendered < CAP * PIXELS
    assert result["pixels_at_cap"] == histogram[CAP]
    assert [n for n, _, _ in result["history"]] == [4, 8, 16, 32] and result["history"][0][1] == int((at_min > F(target)).sum())
    # the Python integrator: the image is sum / count per pixel
    tracer = PathTracer(BounceController(*WINDOW), spp=CAP, seed=SEED, target_noise=target, min_spp=MIN_SPP, adaptive=True)
    image = np.zeros((HEIGHT, WIDTH, 3), dtype=F)
    tracer.run(image, gpu)
    assert np.array_equal(tracer.sample_counts, result["counts"])
    assert np.array_equal(image, result["sums"] / result["counts"][..., None].astype(F))
    assert [n for n, _ in tracer.noise_history] == [4, 8, 16, 32]


# ------------------------------------------------------------------------------------------------------------- jobs

def test_the_pathed_executable_runs_the_adaptive_job(tmp_path):
    """jobs/cornell-adaptive.json at 32 x 32 with min_spp 4, cap 64 and a target that a part of the image reaches early:
    auto-spp.exr holds the counts of the library's own rounds, auto.exr sum / count, metrics.json the new keys."""
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-adaptive.json")))
    assert job["adaptive"] is True
    job.update(width=32, height=32, spp=64, min_spp=4, target_noise=0.1, metrics="basic")
    out_dir, result = _run_job(tmp_path, "adaptive", job)
    assert result.returncode == 0, result.stdout + result.stderr
    metrics = json.load(open(os.path.join(out_dir, "metrics.json")))

    scene = LoadedScene(job["scene"], 32, 32)
    gpu = HipScene(scene.desc, device=0)
    expected = gpu.render_adaptive(job.get("seed", 1), 64, job["startBounce"], job["lastBounce"], 0.1, min_spp=4, floor=job["noise_floor"])
    counts = expected["counts"]
    assert len(np.unique(counts)) >= 3
    # EXR row 0 is the top scanline; the files are HALF: counts up to 2 048 are exact, the image within 2^-11 relative
    found_counts = _read_exr(os.path.join(out_dir, "auto-spp.exr"))[..., :3]
    assert np.array_equal(found_counts, np.repeat(counts[::-1, :, None], 3, axis=2).astype(F))
    image = (expected["sums"] / counts[..., None].astype(F))[::-1]
    found = _read_exr(os.path.join(out_dir, "auto.exr"))[..., :3]
    assert image.max() > 0 and np.all(np.abs(found - image) <= 2.0 ** -11 * image + 2.0 ** -24)
    for stem in ("auto", "auto-spp", "auto-stderr"):
        assert os.path.exists(os.path.join(out_dir, stem + "-00004spp.exr")), stem          # the state after the first step
    first = _read_exr(os.path.join(out_dir, "auto-spp-00004spp.exr"))[..., :3]
    assert (first == 4).all()
    assert metrics["samples_rendered"] == expected["samples_rendered"] == int(counts.sum())
    assert metrics["adaptive_rounds"] == expected["rounds"] and metrics["pixels_at_cap"] == expected["pixels_at_cap"]
    assert metrics["uniform_spp"] == int(counts.max()) and metrics["uniform_samples"] == int(counts.max()) * 1024
    assert metrics["samples_rendered"] < metrics["uniform_samples"]
    assert [entry["spp"] for entry in metrics["noise"]] == [n for n, _, _ in expected["history"]]
    assert [entry["mean_error"] for entry in metrics["noise"]] == [m for _, _, m in expected["history"]]
    assert metrics["last_sample"] == int(counts.max()) and "active pixels" in result.stdout

    # the one-process-per-GPU runner keeps no pixel lists: it refuses the key by name
    job_path = str(tmp_path / "runner.json")
    json.dump(dict(job, output_directory=str(tmp_path / "runner")), open(job_path, "w"))
    result = subprocess.run([sys.executable, "-m", "pathed_amd.run_job", job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=_capi.REPO_ROOT)
    assert result.returncode != 0 and '"adaptive"' in result.stderr and not os.path.exists(str(tmp_path / "runner"))
