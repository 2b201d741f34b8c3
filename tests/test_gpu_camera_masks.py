"""The per-pixel candidate masks of the camera rays (pathed_amd/csrc/camera_masks.h): the fused kernel's camera-queue refill
reads a pixel's mask instead of running phase 1 over every record.  A mask must hold every triangle phase 2 can accept for any
ray through the pixel's footprint (superset), must not be the whole scene where the answer is plain (tightness), and the
renders must be the bytes of the old refill -- which the counting instantiations keep -- and of the per-slot kernels."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def libs():
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    return HipScene, LoadedScene


def _frame(camera):
    """buildCamera in float32: origin, the rows of cameraToWorld, film width and height."""
    def normalized(v):
        return (v / np.sqrt((v * v).sum(dtype=F), dtype=F)).astype(F)
    origin, target, up = (np.array(list(v), dtype=F) for v in (camera.origin, camera.target, camera.up))
    direction = normalized(origin - target)
    x_axis = normalized(np.cross(normalized(up), direction).astype(F))
    y_axis = np.cross(direction, x_axis).astype(F)
    sign = F(-1.0) if camera.flip_handedness else F(1.0)
    film_height = F(2.0) * np.tan(F(camera.vertical_fov) / F(2.0), dtype=F) * F(0.01)
    film_width = F(film_height * F(camera.width) / F(camera.height))
    return origin, sign * x_axis, y_axis, direction, film_width, film_height


def _camera_rays(camera, jitters):
    """cameraRay's expressions (shading.h) in float32 for every pixel and every jitter (jx, jy): (pixels, jitters, 10) rays for
    pathed_hip_debug_small_candidates, the second direction a copy of the first."""
    width, height = camera.width, camera.height
    origin, x_axis, y_axis, direction, film_width, film_height = _frame(camera)
    jitters = np.asarray(jitters, dtype=F)
    rows, cols = np.meshgrid(np.arange(height, dtype=F), np.arange(width, dtype=F), indexing="ij")
    col = (cols.reshape(-1, 1) + jitters[None, :, 0]).astype(F)
    row = (rows.reshape(-1, 1) + jitters[None, :, 1]).astype(F)
    x = (film_width * (col + F(0.5)) / F(width) - film_width / F(2.0)).astype(F)
    y = (film_height * (row + F(0.5)) / F(height) - film_height / F(2.0)).astype(F)
    z = np.full_like(x, -0.01, dtype=F)
    norm = np.sqrt(x * x + y * y + z * z, dtype=F)
    x, y, z = x / norm, y / norm, z / norm
    world = np.stack([x_axis[a] * x + y_axis[a] * y + direction[a] * z for a in range(3)], axis=-1).astype(F)
    rays = np.zeros(world.shape[:2] + (10,), dtype=F)
    rays[..., 0:3] = origin
    rays[..., 3:6] = world
    rays[..., 6:9] = world
    rays[..., 9] = 1e5
    return rays


def _item_words(words, order):
    """Words of the candidates hook (bit p = original primitive p) in the masks' layout (bit 63 - k = item-order triangle k)."""
    out = np.zeros(words.shape, dtype=np.uint64)
    for k, prim in enumerate(order):
        out |= ((words >> np.uint64(prim)) & np.uint64(1)) << np.uint64(63 - k)
    return out


def _grazing_scene(width, height):
    """The camera a hair (4 tnear) in front of a quad it looks at, a triangle that crosses the camera's plane, a light behind."""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(width, height, (0.1, 0.2, 4e-3), (0.1, 0.2, -1.0), fov_degrees=90.0)
    grey = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.6, 0.6, 0.6))
    light = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0, 0, 0), emit=(6.0, 6.0, 6.0))
    built.quad([(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)], grey)
    built.mesh(np.array([(-0.3, -0.2, -1.0), (0.6, -0.1, -1.0), (0.2, 0.1, 1.0)]), [(0, 1, 2)], grey)
    built.mesh(np.array([(0.1, 0.2, 3e-3), (0.4, 0.2, 5e-3), (0.1, 0.5, 5e-3)]), [(0, 1, 2)], grey)   # through the plane, at the origin's feet
    built.quad([(-2.0, -2.0, 3.0), (-2.0, 2.0, 3.0), (2.0, 2.0, 3.0), (2.0, -2.0, 3.0)], light)
    return built


def _scene(libs, name, width, height):
    HipScene, LoadedScene = libs
    if name == "grazing":
        keep = _grazing_scene(width, height)
        desc = keep.finish()
    else:
        keep = LoadedScene(name, width, height)
        desc = keep.desc
    return keep, desc, HipScene(desc, device=0)


def _footprint_jitters(seed):
    half = 0.5
    fixed = [(0.0, 0.0)] + [(sx * half, sy * half) for sx in (-1, 1) for sy in (-1, 1)] + [(-half, 0.0), (half, 0.0), (0.0, -half), (0.0, half)]
    random = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(8, 2))
    return np.concatenate([np.array(fixed), random]).astype(F)


@pytest.mark.parametrize("width,height", [(48, 32), (7, 5), (1, 1)])
@pytest.mark.parametrize("name", ["scenes/cornell.json", "scenes/mis-pbrt.json", "grazing"])
def test_masks_hold_everything_phase_2_accepts(libs, name, width, height):
    keep, desc, gpu = _scene(libs, name, width, height)
    assert gpu.stats()["path_kernel"] == 3
    n_tris = int(desc.contents.n_triangles)
    order = gpu.item_order(n_tris)
    assert sorted(order.tolist()) == list(range(n_tris))
    masks = gpu.camera_masks().reshape(-1)
    scene_bits = np.uint64(0)
    for k in range(n_tris):
        scene_bits |= np.uint64(1) << np.uint64(63 - k)
    assert not (masks & ~scene_bits).any()          # no bit beyond the scene's triangles
    rays = _camera_rays(desc.contents.camera, _footprint_jitters(width * 100 + height))
    out = gpu.small_candidates(rays.reshape(-1, 10)).reshape(rays.shape[0], rays.shape[1], 8)
    accepted = _item_words(out[:, :, 4], order)
    assert accepted.any()
    lost = accepted & ~masks[:, None]
    assert not lost.any(), (int(np.count_nonzero(lost)), np.argwhere(lost)[:4].tolist())


def test_masks_are_tight_inside_faces(libs):
    """Cornell 64 x 64: where a pixel's centre ray and its eight neighbours' have one and the same phase-1 candidate set, the
    pixel's footprint lies inside that set's faces and the mask must be exactly that set (an all-ones table fails)."""
    width = height = 64
    keep, desc, gpu = _scene(libs, "scenes/cornell.json", width, height)
    n_tris = int(desc.contents.n_triangles)
    order = gpu.item_order(n_tris)
    rays = _camera_rays(desc.contents.camera, [(0.0, 0.0)])
    out = gpu.small_candidates(rays.reshape(-1, 10))
    centre = _item_words(out[:, 6], order).reshape(height, width)
    masks = gpu.camera_masks()
    inner = centre[1:-1, 1:-1]
    uniform = np.ones(inner.shape, dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            uniform &= centre[1 + dy:height - 1 + dy, 1 + dx:width - 1 + dx] == inner
    print("pixels with uniform neighbourhoods: %d of %d" % (int(uniform.sum()), width * height))
    assert uniform.sum() * 2 >= width * height
    differing = uniform & (masks[1:-1, 1:-1] != inner)
    assert not differing.any(), (int(differing.sum()), np.argwhere(differing)[:4].tolist())


def _moved(camera):
    moved = copy.copy(camera)
    moved.origin = (C.c_float * 3)(camera.origin[0] + 0.35, camera.origin[1] - 0.2, camera.origin[2] * 0.8)
    return moved


@pytest.mark.parametrize("name,width,height,spp", [
    ("scenes/cornell.json", 13, 5, 1), ("scenes/cornell.json", 40, 24, 6), ("scenes/cornell.json", 256, 256, 4),
    ("scenes/mis-pbrt.json", 32, 24, 4),
])
def test_renders_are_the_bytes_of_the_old_refill(libs, name, width, height, spp):
    HipScene, LoadedScene = libs
    scene = LoadedScene(name, width, height)
    fused = HipScene(scene.desc, device=0)
    counting = HipScene(scene.desc, device=0)
    counting.set_stats_mode(count=True)            # the counting instantiations keep phase 1 in the refill
    per_slot = HipScene(scene.desc, device=0, shade_kernel="per-slot")
    first = fused.render(5, 0, spp, 0, 10)
    assert np.isfinite(first).all() and first.any()
    assert np.array_equal(counting.render(5, 0, spp, 0, 10), first)
    assert np.array_equal(per_slot.render(5, 0, spp, 0, 10), first)

    original = copy.copy(scene.desc.contents.camera)
    moved = _moved(original)
    fused.set_camera(moved)
    after = fused.render(5, 0, spp, 0, 10)
    elsewhere = LoadedScene(name, width, height)
    elsewhere.desc.contents.camera = moved
    assert np.array_equal(HipScene(elsewhere.desc, device=0).render(5, 0, spp, 0, 10), after)
    assert not np.array_equal(after, first)
    fused.set_camera(original)
    assert np.array_equal(fused.render(5, 0, spp, 0, 10), first)
