"""The ends of the argument ranges of the render calls: 64-bit seeds, sample indices up to the last permitted one (2^31 - 2),
pixel indices past 2^24, and the three refusals that guard those ranges.  Every other file calls the kernels with seeds below
10, samples below 20 and at most 2^21 pixels; a kernel that dropped the seed's high word, or kept a sample or pixel index in
a float, would pass all of them.

Scenes, options and sizes of the small cases are those of tests/test_gpu_noise.py (24 x 16 = 384 pixels: one full 256-lane
block and a half).  The expected values are the CPU oracle's (tests/oracle_lib.py), rendered once per scene and shared; the
far-pixel cases use OracleScene.sample_pixel on 4 096 spot pixels of a 4 099 x 4 099 image that is never downloaded."""
import itertools
import time

import numpy as np
import pytest

import test_gpu_noise
from test_gpu_adaptive import COUNT_BITS, SQUARE_BITS, SUM_BITS, Buffers, _lists
from test_gpu_noise import HEIGHT, ORGANISATIONS, WIDTH, WINDOW, _make
from test_gpu_parity import _image_metrics

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
PIXELS = WIDTH * HEIGHT

LATE_SEED = (1 << 32) + 1
SEEDS = [1, 1 << 32, (1 << 32) + 1, 0, 1 << 63, (1 << 64) - 1, 1 << 53, (1 << 53) + 1]
# both sides of the internal pass boundary (256 samples), of 2^16 and of 2^24, and the last index a call may name
SAMPLES = [0, 255, 256, 257, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 2]
GROUPS = {"seeds": [(seed, 0) for seed in SEEDS], "samples": [(LATE_SEED, sample) for sample in SAMPLES]}
LAST_SAMPLE = 0x7ffffffe

# the project's image contract (tests/test_gpu_parity.py) and the volume kernel's (tests/test_gpu_volume.py)
PATH_TOLERANCE = (2e-3, max(1e-3, 1.5 / PIXELS))
VOLUME_TOLERANCE = (1e-2, 5e-3)
DISTINCT = 2e-2      # the oracle's own images of two inputs of a group differ by at least this: ten times the contract


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------------- the oracle's images

# scene key -> (builder of tests/test_gpu_noise.py, the oracle's integrator)
ORACLE_SCENES = {
    "cornell": (test_gpu_noise._cornell, "PathTracer"),
    "room": (test_gpu_noise._room, "PathTracer"),
    "room-environment": (lambda: test_gpu_noise._room(environment=True), "PathTracer"),
    "gas": (test_gpu_noise._gas, "VolumePathTracer"),
}
_oracle_cache = {}


def _oracle_images(key):
    """{(seed, sample): the oracle's one-sample image} for every case of both groups, rendered once per scene, read-only.
    Asserts what lets the comparisons fail: any two images of a group differ by relL2 >= DISTINCT."""
    if key not in _oracle_cache:
        import oracle_lib
        builder, integrator = ORACLE_SCENES[key]
        keep, desc, _, _ = builder()
        oracle = oracle_lib.OracleScene(desc)
        oracle.set_integrator(integrator)
        images = {}
        for seed, sample in sorted(set(GROUPS["seeds"] + GROUPS["samples"])):
            image, stats = oracle.render(WIDTH, HEIGHT, seed, sample, 1, *WINDOW)
            assert stats["dropped"] == 0 and image.any()
            image.setflags(write=False)
            images[(seed, sample)] = image
        for label, group in GROUPS.items():
            closest = min(_rel(images[a], images[b]) for a, b in itertools.combinations(group, 2))
            print("oracle, %s, %s: the two closest images differ by relL2 %.3g" % (key, label, closest))
            assert closest >= DISTINCT, (key, label, closest)
        oracle.close()
        _oracle_cache[key] = images
    return _oracle_cache[key]


def _path_scatter_on_a_media_free_scene():
    """k_path_scatter (path_kernel 9) on the media-free room: generic_kernels=1 under BasicVolumeIntegrator, which is the
    PathTracer there bit for bit (tests/test_gpu_basic_volume.py pins that identity)"""
    from pathed_amd.integrator import HipScene
    keep, desc, _, _ = test_gpu_noise._room()
    gpu = HipScene(desc, device=0, generic_kernels=1)
    gpu.set_integrator("BasicVolumeIntegrator")
    gpu._keep = keep
    return gpu, 9


# organisation -> (oracle scene, tolerance); the first seven are the organisations whose integrator the oracle restates
COMPARED = {
    "fused": ("cornell", PATH_TOLERANCE),
    "hybrid": ("room", PATH_TOLERANCE),
    "wave": ("room", PATH_TOLERANCE),
    "wavefront-1-pool": ("room", PATH_TOLERANCE),
    "wavefront-2-pools": ("room", PATH_TOLERANCE),
    "wavefront-environment": ("room-environment", PATH_TOLERANCE),
    "volume": ("gas", VOLUME_TOLERANCE),
    "multiple-scattering-without-media": ("room", PATH_TOLERANCE),
}


# ---------------------------------------------------------------------------- a. seeds and sample indices, per kernel

@pytest.mark.parametrize("name", sorted(COMPARED))
def test_seeds_and_sample_indices_match_the_oracle(name):
    """Per kernel organisation: one sample (spp_count = 1) for each of eight seeds at sample 0 and each of ten sample indices
    at seed 2^32 + 1, against the oracle's render of the same call.  Path-tracer organisations hold the image contract
    (relL2 <= 2e-3, at most max(1e-3, 1.5 / pixels) of the pixels off by more than 1 %), the volume organisation the bounds
    of tests/test_gpu_volume.py (1e-2, 5e-3).  The oracle's images of any two inputs of a group differ by relL2 >= 2e-2
    (measured: >= 0.05), so a kernel that dropped a word of the seed or cut the sample index cannot pass.
    (384 units are fewer than 4 x 256 per pool: "wavefront-2-pools" runs these one-sample calls on one pool, as
    tests/test_gpu_noise.py notes; its two-pool split is pinned there.)"""
    scene_key, (rel_bound, bad_bound) = COMPARED[name]
    expected = _oracle_images(scene_key)
    gpu, kernel = _path_scatter_on_a_media_free_scene() if name == "multiple-scattering-without-media" else _make(name)
    figures = []
    for label, group in GROUPS.items():
        for seed, sample in group:
            image = gpu.render(seed, sample, 1, *WINDOW)
            stats = gpu.stats()
            rel, bad = _image_metrics(image, expected[(seed, sample)])
            print("%s seed %d sample %d: relL2 %.3g, pixels off by > 1 %%: %.3g" % (name, seed, sample, rel, bad))
            figures.append((label, seed, sample, rel, bad, stats["path_kernel"], stats["dropped_samples"]))
    print("%s: largest relL2 %.3g, largest bad share %.3g" % (name, max(f[3] for f in figures), max(f[4] for f in figures)))
    for label, seed, sample, rel, bad, path_kernel, dropped in figures:
        assert path_kernel == kernel and dropped == 0, (label, seed, sample, path_kernel, dropped)
        assert rel <= rel_bound and bad <= bad_bound, (label, seed, sample, rel, bad)


# ------------------------------------------------------------------------------ b. kernels the oracle does not restate

def test_grid_medium_kernel_tells_seeds_and_sample_indices_apart():
    """k_path_scatter's grid instantiation (a voxel-grid medium under BasicVolumeIntegrator, path_kernel 9).  A WEAKER check
    than the others of this file: the oracle restates neither the grid medium nor multiple scattering, so no expected image
    exists.  What can be asserted: the high word of the seed and bit 24 of the sample index change the image (relL2 >= 2e-2
    between seeds 1 and 2^32 + 1, and between samples 0 and 2^24), and each call made twice gives the same bits.  A kernel
    that read another word, or the right words wrongly, would still pass; the same kernel's media-free instantiation is
    compared with the oracle above."""
    gpu, kernel = _make("multiple-scattering")
    calls = {"seed 1": (1, 0), "seed 2^32+1": (LATE_SEED, 0), "sample 2^24": (LATE_SEED, 1 << 24)}
    images = {}
    for label, (seed, sample) in calls.items():
        first = gpu.render(seed, sample, 1, *WINDOW)
        stats = gpu.stats()
        assert stats["path_kernel"] == kernel and stats["dropped_samples"] == 0, (label, stats)
        assert first.any() and np.isfinite(first).all()
        assert np.array_equal(first.view(U), gpu.render(seed, sample, 1, *WINDOW).view(U)), label
        images[label] = first
    by_seed = _rel(images["seed 1"], images["seed 2^32+1"])
    by_sample = _rel(images["seed 2^32+1"], images["sample 2^24"])
    print("grid medium: seeds 1 and 2^32+1 differ by relL2 %.3g, samples 0 and 2^24 by %.3g" % (by_seed, by_sample))
    assert by_seed >= DISTINCT and by_sample >= DISTINCT


@pytest.mark.parametrize("name", ["wavefront-1-pool", "volume"])
def test_list_passes_at_a_late_seed_and_the_last_samples(name):
    """render_pixels over every other pixel at seed 2^32 + 1, samples 2^31 - 7 .. 2^31 - 3: the listed pixels hold the bits the
    moments render of the whole image leaves there from the same pattern, the others keep the pattern, exactly as
    test_list_renders_are_the_full_renders_bits asserts it near zero."""
    begin, count = (1 << 31) - 7, 5
    gpu, kernel = _make(name)
    entries = _lists()["every-other"]
    listed = np.zeros(PIXELS, dtype=bool)
    listed[entries] = True
    full, buffers = Buffers(gpu), Buffers(gpu)
    try:
        gpu.render_moments_device(LATE_SEED, begin, count, *WINDOW, full.sums, full.squares)
        assert gpu.stats()["path_kernel"] == kernel
        expected_sums, expected_squares, _ = full.read()
        assert (expected_sums != SUM_BITS).any(axis=1).sum() > PIXELS // 2          # the render carries light
        near_zero = Buffers(gpu)                                                    # ... and is not the render of samples 0 .. 4
        try:
            gpu.render_moments_device(LATE_SEED, 0, count, *WINDOW, near_zero.sums, near_zero.squares)
            assert (near_zero.read()[0] != expected_sums).any(axis=1).sum() > PIXELS // 2
        finally:
            near_zero.free()
        n_list = buffers.set_list(entries)
        before = gpu.stats()["iterations"]
        gpu.render_pixels(LATE_SEED, begin, count, *WINDOW, buffers.list, n_list, buffers.sums, buffers.squares, buffers.counts)
        stats = gpu.stats()
        assert stats["path_kernel"] == (kernel if kernel in (4, 9) else 1) and stats["dropped_samples"] == 0 and stats["iterations"] > before, stats
        sums, squares, counts = buffers.read()
        assert np.array_equal(sums[listed], expected_sums[listed]) and np.array_equal(squares[listed], expected_squares[listed])
        assert (counts[listed] == COUNT_BITS + count).all()
        assert (sums[~listed] == SUM_BITS).all() and (squares[~listed] == SQUARE_BITS).all() and (counts[~listed] == COUNT_BITS).all()
    finally:
        full.free()
        buffers.free()


# ------------------------------------------------------------------------------------------------------ c. far pixels

FAR = 4099                        # 4099 x 4099 = 16 801 801 pixels: indices pass 2^24, a last band of 3 rows, a last block of 3 columns
FAR_PIXELS = FAR * FAR
FAR_SAMPLE = 3
N_SPOTS = 4096
FAR_TOLERANCE = (2e-3, max(1e-3, 1.5 / N_SPOTS))


def _spots():
    """4 096 distinct pixel indices, sorted: the corners, 64-pixel runs at both ends of the first and last rows, the last three
    columns of 64 rows and the last three rows of 64 columns, 2^24 - 8 .. 2^24 + 8, and random pixels (seeded) for the rest"""
    rng = np.random.default_rng(24)
    last = FAR - 1
    chosen = {0, last, last * FAR, last * FAR + last}
    for row in (0, last):
        chosen.update(row * FAR + col for col in itertools.chain(range(64), range(FAR - 64, FAR)))
    rows = np.linspace(0, last, 64).astype(np.int64)
    chosen.update(int(row) * FAR + col for row in rows for col in (FAR - 3, FAR - 2, FAR - 1))
    chosen.update(row * FAR + int(col) for row in (FAR - 3, FAR - 2, FAR - 1) for col in rows)
    chosen.update(range((1 << 24) - 8, (1 << 24) + 9))
    assert max(chosen) < FAR_PIXELS and (1 << 24) + 8 < FAR_PIXELS
    while len(chosen) < N_SPOTS:
        chosen.update(int(pixel) for pixel in rng.integers(0, FAR_PIXELS, N_SPOTS - len(chosen)))
    spots = np.array(sorted(chosen), dtype=np.int64)
    assert spots.size == N_SPOTS
    return spots


def _far_room():
    """the room of tests/test_gpu_noise.py (a floor, a back wall, a wavy sheet of 128 triangles, a lamp) at 4099 x 4099"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(FAR, FAR, origin=(0.3, 2.2, 4.2), target=(0, 0.4, 0), fov_degrees=45.0)
    built.quad([(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)], built.material(diffuse=(0.7, 0.6, 0.5)))
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 2.4, -2), (-2, 2.4, -2)], built.material(type_=_capi.MAT_PLASTIC, diffuse=(0.6, 0.1, 0.1), alpha=0.2))
    test_gpu_noise._wavy(built, 8, built.material(diffuse=(0.2, 0.5, 0.7)))
    built.quad([(-0.5, 3.0, -0.5), (0.5, 3.0, -0.5), (0.5, 3.0, 0.5), (-0.5, 3.0, 0.5)], built.material(emit=(8, 8, 8)))
    return built, built.finish()


def _far_cornell():
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene("scenes/cornell.json", FAR, FAR)
    return scene, scene.desc


_far_cache = {}


def _far_expected(key):
    """(spots, the oracle's sample of each spot (N, 3)) for the scene `key`, computed once, read-only"""
    if key not in _far_cache:
        import oracle_lib
        keep, desc = {"cornell": _far_cornell, "room": _far_room}[key]()
        oracle = oracle_lib.OracleScene(desc)
        spots = _spots()
        values = np.stack([oracle.sample_pixel(LATE_SEED, int(pixel) // FAR, int(pixel) % FAR, FAR_SAMPLE, *WINDOW) for pixel in spots])
        oracle.close()
        lit = float((values > 0).any(axis=1).mean())
        print("far pixels, %s: %.1f %% of the oracle's %d spot values carry light" % (key, 100 * lit, N_SPOTS))
        assert lit >= 0.2, (key, lit)
        spots.setflags(write=False)
        values.setflags(write=False)
        _far_cache[key] = (spots, values)
    return _far_cache[key]


def _assert_spots(label, image, spots, expected):
    """the image contract over the spot pixels; `image` is a (FAR_PIXELS, 3) device tensor, only the spots come to the host"""
    import torch
    found = image[torch.as_tensor(spots.copy(), device=image.device)].cpu().numpy()
    rel = float(np.linalg.norm(found - expected) / np.linalg.norm(expected))
    bad = float((np.abs(found - expected) > 1e-2 * np.maximum(np.abs(expected), 1e-3)).any(axis=1).mean())
    print("far pixels, %s: relL2 %.3g over %d spots, spots off by > 1 %%: %.3g" % (label, rel, N_SPOTS, bad))
    assert rel <= FAR_TOLERANCE[0] and bad <= FAR_TOLERANCE[1], (label, rel, bad)


def _far_render(desc, kernel, **options):
    import torch
    from pathed_amd.integrator import HipScene
    image = torch.zeros((FAR_PIXELS, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    started = time.perf_counter()
    gpu = HipScene(desc, device=0, **options)
    created = time.perf_counter()
    gpu.render_device(LATE_SEED, FAR_SAMPLE, 1, *WINDOW, image.data_ptr())
    torch.cuda.synchronize()
    print("far pixels, %s: scene creation %.2f s, the render of %d samples %.2f s" % (options, created - started, FAR_PIXELS, time.perf_counter() - created))
    stats = gpu.stats()
    assert stats["path_kernel"] == kernel and stats["dropped_samples"] == 0 and stats["camera_samples"] == FAR_PIXELS, stats
    return gpu, image


def test_far_pixels_on_the_fused_kernel_under_every_unit_order():
    """Cornell at 4099 x 4099 on the fused kernel, one sample, under unit orders 1, 2 and 3 (stripes, tiled stripes, tiles):
    unitPlace for all three, tileWalkPixel's ragged last band and last 32-column block, and fastDivide(pixel, divWidth) for
    pixels past 2^24.  The orders agree bit for bit over the whole image, and 4 096 spot pixels hold the oracle's sample."""
    import torch
    keep, desc = _far_cornell()
    spots, expected = _far_expected("cornell")
    first = None
    for order in ("stripes", "stripes-tiled", "tiles"):
        gpu, image = _far_render(desc, 3, unit_order=order)
        _assert_spots("fused, unit order " + order, image, spots, expected)
        if first is None:
            first = image
        else:
            assert torch.equal(image, first), order
        gpu.close()


@pytest.mark.parametrize("name, options, kernel", [("wavefront per slot", {"shade_kernel": "per-slot"}, 1), ("k_path_wave", {"shade_kernel": "wave"}, 6)])
def test_far_pixels_on_the_wavefront_and_wave_kernels(name, options, kernel):
    """The room at 4099 x 4099 under the default unit order, on the per-slot wavefront and on k_path_wave."""
    keep, desc = _far_room()
    spots, expected = _far_expected("room")
    gpu, image = _far_render(desc, kernel, **options)
    _assert_spots(name, image, spots, expected)


def test_a_list_pass_over_far_pixels():
    """render_pixels over exactly the spot list at 4099 x 4099: the spots hold the bits the moments render of the whole image
    leaves there from the same pattern, and every other pixel keeps the pattern in every bit.  Checked on the device."""
    import torch
    from pathed_amd.integrator import HipScene
    keep, desc = _far_room()
    spots = _spots()
    gpu = HipScene(desc, device=0, shade_kernel="per-slot")
    device = "cuda:0"

    def pattern(words, bits):
        return torch.full((words,), bits, dtype=torch.int32, device=device)

    full_sums, full_squares = pattern(3 * FAR_PIXELS, SUM_BITS), pattern(3 * FAR_PIXELS, SQUARE_BITS)
    gpu.render_moments_device(LATE_SEED, FAR_SAMPLE, 1, *WINDOW, full_sums.data_ptr(), full_squares.data_ptr())
    torch.cuda.synchronize()
    assert gpu.stats()["path_kernel"] == 1
    sums, squares, counts = pattern(3 * FAR_PIXELS, SUM_BITS), pattern(3 * FAR_PIXELS, SQUARE_BITS), pattern(FAR_PIXELS, COUNT_BITS)
    pixel_list = torch.as_tensor(spots.astype(np.int32), device=device)           # (indices below 2^31: the same bits as uint32)
    before = gpu.stats()["iterations"]
    gpu.render_pixels(LATE_SEED, FAR_SAMPLE, 1, *WINDOW, pixel_list.data_ptr(), N_SPOTS, sums.data_ptr(), squares.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    stats = gpu.stats()
    assert stats["path_kernel"] == 1 and stats["dropped_samples"] == 0 and stats["iterations"] > before, stats
    listed = torch.zeros(FAR_PIXELS, dtype=torch.bool, device=device)
    listed[torch.as_tensor(spots, device=device)] = True
    assert int(listed.sum()) == N_SPOTS
    full_sums, full_squares, sums, squares = (tensor.view(FAR_PIXELS, 3) for tensor in (full_sums, full_squares, sums, squares))
    assert int((full_sums[listed] != SUM_BITS).any(dim=1).sum()) >= N_SPOTS // 5      # the spots carry light
    assert torch.equal(sums[listed], full_sums[listed]) and torch.equal(squares[listed], full_squares[listed])
    assert bool((counts[listed] == COUNT_BITS + 1).all())
    assert bool((sums[~listed] == SUM_BITS).all()) and bool((squares[~listed] == SQUARE_BITS).all()) and bool((counts[~listed] == COUNT_BITS).all())


# ------------------------------------------------------------------------------------------------------ e. the refusals

def test_sample_index_overflow_is_refused_and_the_last_sample_renders():
    """spp_begin + spp_count == 2^31 is refused (-1, "sample index overflow") by render_device, render_moments_device,
    render_pixels and render_features_device: nothing is launched, pattern-filled buffers keep every bit.
    spp_begin = 2^31 - 2, spp_count = 1 -- the last permitted index -- renders through each of them."""
    from pathed_amd.integrator import PathedError
    gpu, kernel = _make("fused")
    buffers = Buffers(gpu)
    depth = gpu.device_words(PIXELS, np.full(PIXELS, SUM_BITS, dtype=U))
    try:
        n_list = buffers.set_list(_lists()["every-other"])
        gpu.render_moments_device(1, 0, 1, *WINDOW, buffers.sums, buffers.squares)          # (so that the counters are not at 0)
        pristine = buffers.read() + (gpu.download_device_words(depth, np.zeros(PIXELS, dtype=U)),)
        before = gpu.stats()["iterations"]
        assert before > 0
        calls = {
            "render_device": lambda begin, count: gpu.render_device(LATE_SEED, begin, count, *WINDOW, buffers.sums),
            "render_moments_device": lambda begin, count: gpu.render_moments_device(LATE_SEED, begin, count, *WINDOW, buffers.sums, buffers.squares),
            "render_pixels": lambda begin, count: gpu.render_pixels(LATE_SEED, begin, count, *WINDOW, buffers.list, n_list, buffers.sums, buffers.squares, buffers.counts),
            "render_features_device": lambda begin, count: gpu.render_features_device(LATE_SEED, begin, count, depth=depth),
        }
        for label, call in calls.items():
            for begin, count in ((LAST_SAMPLE, 2), (0x7fffffff, 1), (0, 0x80000000), (0xffffffff, 1), (0x40000000, 0x40000000)):
                with pytest.raises(PathedError, match=r"\(-1\).*sample index overflow"):
                    call(begin, count)
            assert gpu.stats()["iterations"] == before, label
        found = buffers.read() + (gpu.download_device_words(depth, np.zeros(PIXELS, dtype=U)),)
        for held, kept in zip(found, pristine):
            assert np.array_equal(held, kept)
        # the Python wrappers refuse a seed outside [0, 2^64) before the library sees it
        for seed in (-1, 1 << 64):
            for call in (lambda: gpu.render(seed, 0, 1, *WINDOW), lambda: gpu.render_device(seed, 0, 1, *WINDOW, buffers.sums),
                         lambda: gpu.render_moments_device(seed, 0, 1, *WINDOW, buffers.sums, buffers.squares),
                         lambda: gpu.render_pixels(seed, 0, 1, *WINDOW, buffers.list, n_list, buffers.sums, buffers.squares, buffers.counts),
                         lambda: gpu.render_features_device(seed, 0, 1, depth=depth),
                         lambda: gpu.render_adaptive(seed, 8, *WINDOW, 0.1, min_spp=4)):
                with pytest.raises(PathedError, match=r"seed must be an integer in \[0, 2\^64\)"):
                    call()
        assert gpu.stats()["iterations"] == before
        # the last permitted sample renders, through every call
        for label, call in calls.items():
            call(LAST_SAMPLE, 1)
            before += 1
            assert gpu.stats()["iterations"] >= before, label
            before = gpu.stats()["iterations"]
        sums, squares, counts, depths = buffers.read() + (gpu.download_device_words(depth, np.zeros(PIXELS, dtype=U)),)
        assert (sums != pristine[0]).any(axis=1).sum() > PIXELS // 4 and (counts != pristine[2]).sum() == n_list and (depths != pristine[3]).any()
    finally:
        buffers.free()
        gpu.free_device_buffer(depth)


def test_too_many_work_units_in_one_pass_is_refused_before_anything_is_allocated():
    """1024 x 1024 pixels x 4 096 one-sample units in one pass (chunks_per_pass = 4096, spp_count = 4096) are 2^32 units, more
    than a pass can number.  The check comes before the pass allocates its partial sums (they would be 64 GB): the call
    returns -1, launches nothing and leaves the pattern."""
    import torch
    from pathed_amd.integrator import HipScene, PathedError
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene("scenes/cornell.json", 1024, 1024)
    gpu = HipScene(scene.desc, device=0, chunks_per_pass=4096)
    image = torch.full((3 * 1024 * 1024,), SUM_BITS, dtype=torch.int32, device="cuda:0")
    squares = torch.full((3 * 1024 * 1024,), SQUARE_BITS, dtype=torch.int32, device="cuda:0")
    free_before = torch.cuda.mem_get_info()[0]
    with pytest.raises(PathedError, match=r"\(-1\).*too many work units in one pass"):
        gpu.render_device(1, 0, 4096, *WINDOW, image.data_ptr())
    with pytest.raises(PathedError, match=r"\(-1\).*too many work units in one pass"):
        gpu.render_moments_device(1, 0, 4096, *WINDOW, image.data_ptr(), squares.data_ptr())
    torch.cuda.synchronize()
    assert gpu.stats()["iterations"] == 0
    assert free_before - torch.cuda.mem_get_info()[0] < (1 << 30)                 # nothing of the 64 GB was asked for
    assert bool((image == SUM_BITS).all()) and bool((squares == SQUARE_BITS).all())
    gpu.render_device(1, 0, 1, *WINDOW, image.data_ptr())                          # one sample of the same scene renders
    torch.cuda.synchronize()
    assert gpu.stats()["iterations"] >= 1 and bool((image != SUM_BITS).any())


def test_an_image_of_more_than_2_to_the_28_pixels_is_refused():
    """16385 x 16384 is 2^28 + 16384 pixels: scene creation returns -1, "image too large"; 2^28 itself is within the range
    (not created here: its buffers are not a test's to allocate)."""
    from pathed_amd.integrator import HipScene, PathedError
    from pathed_amd.scene import LoadedScene
    scene = LoadedScene("scenes/cornell.json", 16385, 16384)
    with pytest.raises(PathedError, match=r"\(-1\).*image too large"):
        HipScene(scene.desc, device=0)
