"""Henyey-Greenstein media on the BasicVolumeIntegrator (k_path_aniso / k_path_aniso_grid, DESIGN.md §4.4g;
pathed_hip_scene_set_medium_phase).

  1  identities, bit for bit: a Henyey-Greenstein slot that no surface references selects the anisotropic kernels
     (path_kernel 11) and the image is the isotropic kernels' (path_kernel 9); isotropic slots stay on 9; split calls, the
     8-row and 22-row forms and render_moments agree with one render call;
  2  image means against the float64 walk of tests/anisotropic_scattering_reference.py under tests/test_gpu_basic_volume.py's
     rule, 7.5 x the walk's deviation x sqrt(1 / (128 x 128 x 64) + 1 / 10^6).  No pixel and no window is left out;
  3  the two functions through their hook against the float64 formulas on the same fp32 inputs, under the bounds
     pathed_amd/csrc/volume.h derives;
  4  refusals and argument errors, by code and by name, with nothing launched;
  5  both launchers on jobs/cornell-smoke-hg.json.

The walk's camera sits on +z and its back-lit environment is 2 on directions with z < 0.  The device's environment map has its
pole on +y, so the device scene is the walk's under (x, y, z) -> (x, z, -y): the camera on +y looking down, up = -z, and the
map's lower half (theta >= pi / 2, rows 16..31 of 32) at 2 -- the split is a texel row's edge."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anisotropic_scattering_reference as reference

pytestmark = pytest.mark.gpu

SIZE, SPP = 128, 64
EPS = 2.0 ** -24
E_INVALID, E_UNSUPPORTED = "(-1)", "(-4)"


def _tolerance(deviation):
    return 7.5 * deviation * np.sqrt(1.0 / (SIZE * SIZE * SPP) + 1.0 / reference.WALKS)


def _basic(desc, **options):
    from pathed_amd.integrator import HipScene
    gpu = HipScene(desc, device=0, **options)
    gpu.set_integrator("BasicVolumeIntegrator")
    return gpu


def _render(gpu, kernel, *window):
    image = gpu.render(*window)
    stats = gpu.stats()
    assert np.isfinite(image).all() and stats["dropped_samples"] == 0 and stats["path_kernel"] == kernel, stats
    return image


# ---------------------------------------------------------------------------------------------- 1: identities
GRID_BOX = (-1.0, 0.2, -1.0, 1.0, 2.2, 1.0)      # the gas scene's container


def _grid():
    rng = np.random.default_rng(11)
    return dict(data=rng.random((5, 6, 7), dtype=np.float32), bounds=GRID_BOX, albedo=0.9, scale=4.0)


def _identity_scene(kind, idle):
    """the gas scene of tests/test_gpu_basic_volume.py (sigma = 2, slot 0) as `kind`, with one more medium slot that no surface
    references where `idle`: (scene, idle slot)"""
    from test_gpu_basic_volume import _gas_scene
    built = _gas_scene(2.0)
    slot = built.medium((1.0, 1.0, 1.0), (0.5, 0.5, 0.5)) if idle else None
    gpu = _basic(built.finish(), **({"intersector": "bvh"} if kind == "tree" else {}))
    if kind == "grid":
        gpu.set_grid_medium(0, **_grid())
    return gpu, slot


@pytest.mark.parametrize("kind", ["gas", "grid", "tree"])
def test_an_unreferenced_slot_selects_the_kernels_and_changes_no_bit(kind):
    window = (4, 0, 8, 0, 12)
    plain, _ = _identity_scene(kind, False)
    expected = _render(plain, 9, *window)
    assert expected.any()
    gpu, idle = _identity_scene(kind, True)
    assert np.array_equal(_render(gpu, 9, *window), expected)      # the slot alone, never given a phase function
    for g, type_ in ((0.8, "isotropic"), (0.0, "henyey-greenstein"), (5e-4, "henyey-greenstein"), (-9.9e-4, "henyey-greenstein")):
        gpu.set_medium_phase(idle, g, type_)
        assert np.array_equal(_render(gpu, 9, *window), expected), (g, type_)
    gpu.set_medium_phase(idle, 0.8)
    assert np.array_equal(_render(gpu, 11, *window), expected)
    assert np.array_equal(_render(gpu, 11, 4, 0, 5, 2, 6), _render(plain, 9, 4, 0, 5, 2, 6))      # a bounce window
    gpu.set_medium_phase(0, 0.0)      # the referenced slot at g = 0, the other still at 0.8: today's bits inside the new kernels
    assert np.array_equal(_render(gpu, 11, *window), expected)
    gpu.set_medium_phase(idle, -0.8)      # calling it again replaces the entry
    assert np.array_equal(_render(gpu, 11, *window), expected)
    gpu.set_medium_phase(idle, 0.0)
    assert np.array_equal(_render(gpu, 9, *window), expected)


@pytest.mark.parametrize("kind", ["gas", "grid"])
def test_split_calls_row_counts_and_moments_change_nothing(kind):
    """... on a medium that does scatter forward: g = 0.8 on the gas itself"""
    import torch
    from pathed_amd.integrator import HipScene
    from test_gpu_basic_volume import _gas_scene
    desc = _gas_scene(2.0).finish()

    def scene(**options):
        gpu = _basic(desc, phases=[(0, 0.8)], **options)
        if kind == "grid":
            gpu.set_grid_medium(0, **_grid())
        return gpu
    gpu = scene()
    image = _render(gpu, 11, 4, 0, 8, 0, 12)
    isotropic = scene()
    isotropic.set_medium_phase(0, 0.8, "isotropic")
    assert image.any() and not np.array_equal(_render(isotropic, 9, 4, 0, 8, 0, 12), image)      # g does change the image
    parts = torch.zeros((40, 48, 3), dtype=torch.float32, device="cuda:0")      # 3 + 5 samples are the 8 of one call
    gpu.render_device(4, 0, 3, 0, 12, parts.data_ptr())
    gpu.render_device(4, 3, 5, 0, 12, parts.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(parts.cpu().numpy(), image)
    sums, squares = gpu.render_moments(4, 0, 8, 0, 12)
    assert np.array_equal(sums, image) and squares.any() and gpu.stats()["path_kernel"] == 11
    for rows in (8, 16, 22):      # the tree walk: one 22-row form, whatever the scene's own row count
        walked = scene(stack_rows=rows, intersector="bvh")
        assert np.array_equal(_render(walked, 11, 4, 0, 8, 0, 12), image), rows
    late = HipScene(desc, device=0)      # the constructor's `phases` and a later call are the same thing
    late.set_integrator("BasicVolumeIntegrator")
    if kind == "grid":
        late.set_grid_medium(0, **_grid())
    late.set_medium_phase(0, 0.8)
    assert np.array_equal(_render(late, 11, 4, 0, 8, 0, 12), image)


# ---------------------------------------------------------------------------------------------- 2: means against the walk
def _device_box(box):
    (x0, y0, z0), (x1, y1, z1) = box      # walk (x, y, z) -> device (x, z, -y)
    return (x0, z0, -y1), (x1, z1, -y0)


def _built(albedo=1.0, box=None, environment="back-lit"):
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    from test_gpu_basic_volume import _sphere_mesh
    built = BuiltScene(SIZE, SIZE, (0, reference.DISTANCE, 0), (0, 0, 0), up=(0, 0, -1), fov_degrees=reference.FOV)
    passthrough = built.material(type_=_capi.MAT_PASSTHROUGH)
    gas = built.medium((2.0,) * 3, (2.0 * albedo,) * 3)
    if box is not None:
        built.box(*_device_box(box), passthrough, medium=gas)
    else:
        built.mesh(*_sphere_mesh(1.0), passthrough, medium=gas)
    rgba = np.ones((reference.BACK_LIT_ROWS, 64, 4), dtype=np.float32)
    if environment == "back-lit":
        rgba[..., :3] = reference.back_lit_map()[..., None]
    built.environment(rgba, scale=1.0)
    return built, gas


def _gpu_mean(gpu, last_bounce):
    image = _render(gpu, 11, 7, 0, SPP, 0, last_bounce)
    assert np.array_equal(image[..., 0], image[..., 1]) and np.array_equal(image[..., 0], image[..., 2])      # a grey world
    return float(image[..., 0].mean(dtype=np.float64)) / SPP


def _compare(gpu, walked, windows):
    for last in windows:
        mean, deviation = walked[last]
        found = _gpu_mean(gpu, last)
        print("window (0, %d): gpu %.5f  walk %.5f  tolerance %.5f" % (last, found, mean, _tolerance(deviation)))
        assert abs(found - mean) <= _tolerance(deviation), (last, found, mean, _tolerance(deviation))


def _assert_back_lit(gpu):
    """env_emit takes lightWo, the direction from the light towards the point: a ray that leaves along d reads emit(-d)"""
    leaving = np.array([[0.3, 0.9, 0.1], [0.0, 1.0, 0.0], [1.0, 1e-3, 0.0], [-0.6, 0.02, 0.8],
                        [0.3, -0.9, 0.1], [0.0, -1.0, 0.0], [1.0, -1e-3, 0.0], [-0.6, -0.02, 0.8]])
    leaving /= np.linalg.norm(leaving, axis=1, keepdims=True)
    found = gpu.shading_queries("env_emit", "All", -leaving)
    assert np.array_equal(found[:4], np.zeros((4, 3))) and np.array_equal(found[4:], np.full((4, 3), 2.0)), found      # front 0, back 2


SERIES = (2, 3, 5, 12)


@pytest.mark.parametrize("albedo", [1.0, 0.8])
@pytest.mark.parametrize("g", [0.7, -0.7])
def test_back_lit_scattering_series(g, albedo):
    """the sphere container, sigma_t = 2, lit from behind: the walk gives 1.009 .. 1.681 at g = +0.7 and 0.749 .. 1.022 at
    g = -0.7 (albedo 1, windows (0, 2) and (0, 12)); the isotropic values lie eight tolerances from either"""
    walked = reference.shared_walk(SERIES, g, "back-lit", albedo=albedo)
    other = reference.shared_walk(SERIES, -g, "back-lit", albedo=albedo)
    for last in SERIES:      # the comparison tells the two signs of g apart
        assert abs(walked[last][0] - other[last][0]) >= 10.0 * _tolerance(max(walked[last][1], other[last][1])), (last, walked, other)
    built, gas = _built(albedo=albedo)
    gpu = _basic(built.finish(), phases=[(gas, g)])
    _assert_back_lit(gpu)
    _compare(gpu, walked, SERIES)


@pytest.mark.parametrize("g", [0.7, -0.7])
def test_white_furnace(g):
    """a constant environment, albedo 1, window (0, 60): every order of scattering counted, the mean is the walk's (and 1)"""
    walked = reference.shared_walk((60,), g)
    built, gas = _built(environment="constant")
    _compare(_basic(built.finish(), phases=[(gas, g)]), walked, (60,))


BOX = ((-0.8, -0.7, -0.6), (0.8, 0.7, 0.6))


def test_grid_medium_against_the_walk_over_its_box():
    """a box container equal to the grid's bounds, constant density 0.5 x scale 4 = 2, albedo 1, g = 0.7, lit from behind:
    k_path_aniso_grid, the all-triangles form and the tree walk"""
    windows = (3, 12)
    walked = reference.shared_walk(windows, 0.7, "back-lit", box=BOX)
    isotropic = reference.shared_walk(windows, 0.0, "back-lit", box=BOX)
    for last in windows:
        assert abs(walked[last][0] - isotropic[last][0]) >= 5.0 * _tolerance(max(walked[last][1], isotropic[last][1])), (walked, isotropic)
    built, gas = _built(box=BOX)
    lo, hi = _device_box(BOX)
    grid = dict(data=np.full((5, 6, 7), 0.5, dtype=np.float32), bounds=lo + hi, albedo=1.0, scale=4.0)
    desc = built.finish()
    gpu = _basic(desc, phases=[(gas, 0.7)])
    gpu.set_grid_medium(gas, **grid)
    _assert_back_lit(gpu)
    _compare(gpu, walked, windows)
    image = _render(gpu, 11, 7, 0, 4, 0, 12)
    walked_tree = _basic(desc, phases=[(gas, 0.7)], intersector="bvh")
    walked_tree.set_grid_medium(gas, **grid)
    assert np.array_equal(_render(walked_tree, 11, 7, 0, 4, 0, 12), image)


# ---------------------------------------------------------------------------------------------- 3: the hook
def _hook_scene():
    from test_gpu_basic_volume import _gas_scene
    return _basic(_gas_scene(1.0, 8, 8).finish())


def _unit(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)


def _records(g, seed):
    """4 096 records (g, w, u1, u2, wi): the ends of [0, 1] and their neighbours, the frame's two branches and its axes,
    wi along and against w, then random ones"""
    rng = np.random.default_rng(seed)
    n = 4096
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    special = np.array([0.0, np.nextafter(np.float32(0.0), np.float32(1.0)), 1e-7, 0.25, 0.5, 0.75, np.nextafter(below_one, np.float32(0.0)), below_one, 1.0], dtype=np.float32)
    u = rng.random((n, 2), dtype=np.float32)
    pairs = np.array([(a, b) for a in special for b in special], dtype=np.float32)
    u[:len(pairs)] = pairs
    w = _unit(rng.normal(size=(n, 3)))
    axes = _unit([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1, 0], [1, -1, 1], [0.5, 0.5, 0.70710678]])
    w[100:100 + len(axes)] = axes
    wi = _unit(rng.normal(size=(n, 3)))
    wi[200:232] = w[200:232]
    wi[232:264] = -w[232:264]
    return np.concatenate([np.full((n, 1), g, dtype=np.float32), w, u, wi], axis=1)


@pytest.mark.parametrize("g", [0.05, -0.05, 0.3, -0.3, 0.7, -0.7, 0.9, -0.9, 0.99, -0.99])
def test_the_hook_against_the_float64_formulas(g):
    """The bounds are pathed_amd/csrc/volume.h's, first order in eps = 2^-24 with 0.1 % for the higher orders.
    c:  eps { [1 + 2 g^2 + s^2 (2 rho + 1)] / (2 |g|) + 2 },  rho = 1 / (1 - g^2) + kappa + 2,
        kappa = (|1 - g| + |2 g u1|) / |(1 - g) + 2 g u1|; read back as w . direction, which adds the frame: 24 eps (the two
        axes are orthogonal to w within 4 and 7 eps, |w|^2 is 1 within 2, the three products and two sums of toWorld 5, then
        the rounding of the direction itself).
    p:  relative eps { 1.5 (1 + 2 g^2 + 8 |g|) / x + 1 / (1 - g^2) + 5.5 } -- the dot product's three roundings times 2 |g|, the
        roundings of 1 + g^2, 2 g c and the difference, against x = 1 + g^2 - 2 g c; then x sqrt(x), 1 - g^2 and two divisions."""
    gpu = _hook_scene()
    records = _records(g, 17)
    found = gpu.phase_hg(records).astype(np.float64)
    assert found.shape == (4096, 4) and np.isfinite(found).all()
    g64 = float(np.float32(g))
    w, wi = records[:, 1:4].astype(np.float64), records[:, 6:9].astype(np.float64)
    u1, u2 = records[:, 4].astype(np.float64), records[:, 5].astype(np.float64)
    direction = found[:, :3]

    # unit length
    assert np.abs(np.linalg.norm(direction, axis=1) - 1.0).max() <= 1e-6
    # the cosine
    cosine, s = reference.hg_cosine(g64, u1)
    kappa = (abs(1.0 - g64) + np.abs(2.0 * g64 * u1)) / np.abs((1.0 - g64) + 2.0 * g64 * u1)
    rho = 1.0 / (1.0 - g64 * g64) + kappa + 2.0
    bound = 1.001 * EPS * ((1.0 + 2.0 * g64 * g64 + s * s * (2.0 * rho + 1.0)) / (2.0 * abs(g64)) + 2.0) + 24.0 * EPS
    deviation = np.abs(np.einsum("ij,ij->i", w, direction) - cosine)
    worst = int(np.argmax(deviation / bound))
    print("g %+.2f: largest deviation of c %.3e (bound there %.3e), largest share of the bound %.3f" % (g, deviation.max(), bound[int(np.argmax(deviation))], (deviation / bound).max()))
    assert (deviation <= bound).all(), (records[worst], deviation[worst], bound[worst])
    # the azimuth, in the frame normalToWorldSpace1(w): the part across w points along (cos phi, sin phi)
    x_axis, z_axis = reference.frame(w)
    phi = (2.0 * np.pi * u2).astype(np.float32).astype(np.float64)      # twoPiTimes: narrowed once
    across_x, across_z = np.einsum("ij,ij->i", x_axis, direction), np.einsum("ij,ij->i", z_axis, direction)
    assert np.abs(across_x * np.sin(phi) - across_z * np.cos(phi)).max() <= 2e-6
    assert (across_x * np.cos(phi) + across_z * np.sin(phi) >= -2e-6).all()
    # the value
    four_pi = float(np.float32(4.0 * np.pi))
    c = np.einsum("ij,ij->i", w, wi)
    x = (1.0 + g64 * g64) - 2.0 * g64 * c
    expected = (1.0 - g64 * g64) / (x * np.sqrt(x)) / four_pi
    relative = 1.001 * EPS * (1.5 * (1.0 + 2.0 * g64 * g64 + 8.0 * abs(g64)) / x + 1.0 / (1.0 - g64 * g64) + 5.5)
    error = np.abs(found[:, 3] - expected) / expected
    print("g %+.2f: largest relative error of p %.3e, largest share of its bound %.3f" % (g, error.max(), (error / relative).max()))
    assert (error <= relative).all(), float((error / relative).max())


def test_below_the_threshold_the_hook_is_the_isotropic_pair():
    gpu = _hook_scene()
    isotropic = None
    for g in (0.0, 5e-4, -9.9e-4):
        records = _records(g, 23)
        found = gpu.phase_hg(records)
        if isotropic is None:
            isotropic = gpu.phase_samples(records[:, 4:6])
        assert np.array_equal(found[:, :3], isotropic), g      # pathed_hip_debug_phase_samples' bits
        assert (found[:, 3] == np.float32(1.0) / np.float32(4.0 * np.pi)).all()      # 1.f / fourPi
    at = gpu.phase_hg(_records(1e-3, 23))      # at the threshold the function is Henyey-Greenstein
    assert not np.array_equal(at[:, :3], isotropic)


# ---------------------------------------------------------------------------------------------- 4: refusals, argument errors
def _nothing_ran(gpu):
    stats = gpu.stats()
    return stats["trace_launches_all"] == 0 and stats["camera_samples"] == 0 and stats["iterations"] == 0


def test_single_scattering_and_pixel_lists_are_refused_by_name():
    import torch
    from pathed_amd.integrator import PathedError
    from test_gpu_basic_volume import _gas_scene
    built = _gas_scene(2.0)
    idle = built.medium((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    gpu = _basic(built.finish(), phases=[(idle, 0.8)])      # an unreferenced slot is enough
    pixels = torch.tensor([3, 17, 400], dtype=torch.int32, device="cuda:0")
    sums = torch.zeros((40, 48, 3), dtype=torch.float32, device="cuda:0")
    squares, counts = torch.zeros_like(sums), torch.zeros((40, 48), dtype=torch.int32, device="cuda:0")
    listed = lambda: gpu.render_pixels(1, 0, 2, 0, 8, pixels.data_ptr(), 3, sums.data_ptr(), squares.data_ptr(), counts.data_ptr())
    assert _nothing_ran(gpu)
    with pytest.raises(PathedError) as error:
        listed()
    assert E_UNSUPPORTED in str(error.value) and "Henyey-Greenstein" in str(error.value) and "pixel lists" in str(error.value), str(error.value)
    gpu.set_integrator("VolumePathTracer")
    for call in (lambda: gpu.render(1, 0, 2, 0, 8), lambda: gpu.render_moments(1, 0, 2, 0, 8), listed):
        with pytest.raises(PathedError) as error:
            call()
        assert E_UNSUPPORTED in str(error.value) and "Henyey-Greenstein" in str(error.value) and "VolumePathTracer" in str(error.value), str(error.value)
    torch.cuda.synchronize()
    assert _nothing_ran(gpu) and not sums.any() and not squares.any() and not counts.any()
    gpu.set_medium_phase(idle, 0.8, "isotropic")      # without the slot both render as ever
    assert gpu.render(1, 0, 2, 0, 8).any() and gpu.stats()["path_kernel"] == 4
    gpu.set_integrator("BasicVolumeIntegrator")
    listed()
    assert gpu.stats()["path_kernel"] == 9 and int(counts.sum().item()) == 6


def test_argument_errors_leave_the_scene_as_it_was():
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError
    from test_gpu_basic_volume import _gas_scene
    built = _gas_scene(2.0)
    idle = built.medium((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    gpu = _basic(built.finish())
    lib = gpu._lib

    def refused(name, call):
        with pytest.raises(PathedError) as error:
            call()
        assert E_INVALID in str(error.value) and name in str(error.value), str(error.value)

    def raw(scene, index, phase):
        code = lib.pathed_hip_scene_set_medium_phase(scene, index, phase)
        if code != 0:
            raise PathedError("pathed_hip_scene_set_medium_phase failed (%d): %s" % (code, lib.pathed_hip_last_error().decode()))

    def phase(type_=_capi.PHASE_HENYEY_GREENSTEIN, g=0.5, size=None):
        record = _capi.PathedPhaseFunction()
        record.struct_size = C.sizeof(_capi.PathedPhaseFunction) if size is None else size
        record.type, record.g = type_, g
        return C.byref(record)

    def all_errors():
        refused("null", lambda: raw(None, idle, phase()))
        refused("null", lambda: raw(gpu._handle, idle, None))
        refused("struct_size", lambda: raw(gpu._handle, idle, phase(size=8)))
        for index in (-1, idle + 1, 1 << 20):
            refused("out of range", lambda: raw(gpu._handle, index, phase()))
        for type_ in (2, -1):
            refused("unknown phase function type", lambda: raw(gpu._handle, idle, phase(type_=type_)))
        for g in (float("nan"), float("inf"), -float("inf"), 0.995, -1.0):
            refused("|g| <= 0.99", lambda: raw(gpu._handle, idle, phase(g=g)))
            refused("|g| <= 0.99", lambda: raw(gpu._handle, idle, phase(type_=_capi.PHASE_ISOTROPIC, g=g)))

    all_errors()
    assert _nothing_ran(gpu)
    expected = _render(gpu, 9, 4, 0, 4, 0, 8)      # no table was made
    gpu.set_medium_phase(idle, 0.99)      # the largest g there is
    gpu.set_medium_phase(0, -0.5)
    image = _render(gpu, 11, 4, 0, 4, 0, 8)
    assert not np.array_equal(image, expected)
    all_errors()
    assert np.array_equal(_render(gpu, 11, 4, 0, 4, 0, 8), image)      # ... and the one there is stays

    from pathed_amd.scene import LoadedScene
    loaded = LoadedScene("scenes/cornell.json", 16, 16)      # a scene without media has no slot to set
    no_media = _basic(loaded.desc)
    with pytest.raises(PathedError) as error:
        no_media.set_medium_phase(0, 0.5)
    assert E_INVALID in str(error.value) and "out of range" in str(error.value)

    # the hook
    record = _records(0.5, 1)[:4]
    for column, value, name in ((0, 0.995, "|g| <= 0.99"), (0, np.nan, "|g| <= 0.99"), (4, 1.5, "[0, 1]"), (5, -0.1, "[0, 1]"), (2, np.inf, "finite")):
        bad = record.copy()
        bad[2, column] = value
        refused(name, lambda: gpu.phase_hg(bad))
    assert gpu.phase_hg(np.zeros((0, 9), dtype=np.float32)).shape == (0, 4)


# ---------------------------------------------------------------------------------------------- 5: the launchers
def _launch(name, job, tmp_path):
    from pathed_amd import _capi
    job_path = str(tmp_path / (name + ".json"))
    json.dump(job, open(job_path, "w"))
    command = ([os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")] if name == "cpp" else [sys.executable, "-m", "pathed_amd.run_job"]) + [job_path, _capi.REPO_ROOT]
    return subprocess.run(command, capture_output=True, text=True, cwd=_capi.REPO_ROOT)


def _job(tmp_path, name, **changes):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-smoke-hg.json")))
    assert job["scene"] == "scenes/cornell-smoke-hg.json" and job["integrator"] == "BasicVolumeIntegrator"
    job.update(width=64, height=48, spp=8, output_directory=str(tmp_path / name), **changes)
    return job


def test_both_launchers_write_the_same_bytes(tmp_path):
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    from test_gpu_job import _read_exr
    files = {}
    for name in ("cpp", "py"):
        job = _job(tmp_path, name)
        result = _launch(name, job, tmp_path)
        assert result.returncode == 0, result.stdout + result.stderr
        assert "sample: 8/8" in result.stdout
        files[name] = {f: open(os.path.join(job["output_directory"], f), "rb").read() for f in ("auto.exr", "auto-00008spp.exr", "auto-00004spp.exr")}
    assert files["cpp"] == files["py"]
    # ... of the anisotropic kernels' image: the mean of samples [0, 8), HALF precision in the file, rows flipped
    scene = LoadedScene("scenes/cornell-smoke-hg.json", 64, 48)
    gpu = HipScene(scene.desc, device=0, grids=scene.grids, phases=scene.phases)
    gpu.set_integrator("BasicVolumeIntegrator")
    job = _job(tmp_path, "cpp")
    mean = _render(gpu, 11, job.get("seed", 1), 0, 8, job["startBounce"], job["lastBounce"]) / 8.0
    half = mean[::-1].astype(np.float16).astype(np.float32)
    written = _read_exr(os.path.join(job["output_directory"], "auto-00008spp.exr"))[..., :3]
    assert np.allclose(written, half, rtol=2e-3, atol=2e-3)
    plain = HipScene(scene.desc, device=0, grids=scene.grids)
    plain.set_integrator("BasicVolumeIntegrator")
    assert not np.array_equal(_render(plain, 9, job.get("seed", 1), 0, 8, job["startBounce"], job["lastBounce"]) / 8.0, mean)


def test_both_launchers_stop_what_the_library_refuses_by_name(tmp_path):
    for name in ("cpp", "py"):
        result = _launch(name, _job(tmp_path, name + "-single", integrator="VolumePathTracer"), tmp_path)
        text = result.stdout + result.stderr
        assert result.returncode != 0 and "VolumePathTracer" in text and "henyey-greenstein" in text, text
        result = _launch(name, _job(tmp_path, name + "-adaptive", adaptive=True, target_noise=0.05), tmp_path)
        text = result.stdout + result.stderr
        assert result.returncode != 0 and "adaptive" in text, text
        for run in ("-single", "-adaptive"):      # stopped before anything was rendered
            directory = str(tmp_path / (name + run))
            assert not os.path.isdir(directory) or not [f for f in os.listdir(directory) if f.endswith(".exr")]
    result = _launch("cpp", _job(tmp_path, "cpp-adaptive", adaptive=True, target_noise=0.05), tmp_path)
    assert "henyey-greenstein" in result.stdout + result.stderr
