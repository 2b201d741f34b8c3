"""First-hit feature images (pathed_hip_render_features, k_features) and the AlbedoIntegrator against expectations derived
from the oracle's pieces: the counter stream, the camera ray, the closest hit.  Material, interpolated uv and normal come from
this file's own scene arrays in fp32 numpy (fmaf written out through float64, whose product of two floats is exact).

hit_count and depth_sum are bit-identical (the intersector contract is bit-exact, t is the oracle's t), albedo_sum is on
constant-albedo materials; checkerboard / texture albedo and normal_sum agree within the project's function-level tolerance
per sample, spp x (1e-6 relative + 2e-7 absolute).  No pixel is excluded anywhere."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
WIDTH, HEIGHT, SPP, SEED = 48, 32, 8, 7
DIFFUSE_KINDS = (0, 1, 3)   # Lambertian, OrenNayar, Plastic


def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _normalized(v):
    norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F)).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v / norm[:, None]).astype(F)


def _xcross(a, b):
    return np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1]).astype(F)),
                     _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2]).astype(F)),
                     _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]).astype(F))], axis=1)


def _camera_rays(camera, seed, spp_begin, spp_count):
    """(H * W, spp, 8) rays of startCameraSample: dimensions 0, 1 of the counter stream, X jitter first, cameraRay(row + jy, col + jx)"""
    import oracle_lib
    width, height = camera.width, camera.height
    head = list(camera.origin) + list(camera.target) + list(camera.up) + [camera.vertical_fov, width, height, camera.flip_handedness]
    rays = np.zeros((height * width, spp_count, 8), dtype=F)
    for pixel in range(height * width):
        row, col = divmod(pixel, width)
        for k in range(spp_count):
            jx = F(oracle_lib.rng(seed, pixel, spp_begin + k, 0)) - F(0.5)
            jy = F(oracle_lib.rng(seed, pixel, spp_begin + k, 1)) - F(0.5)
            ray = oracle_lib.evaluate("camera_ray", head + [F(row) + jy, F(col) + jx])
            rays[pixel, k] = (ray[0], ray[1], ray[2], 1e-3, ray[3], ray[4], ray[5], 1e5)
    return rays


class Expectation:
    """What the feature kernel and the albedo integrator must produce for `built`, per sample, from the oracle's hits."""

    def __init__(self, built, desc, seed=SEED, spp_begin=0, spp_count=SPP, camera=None, positions=None):
        import oracle_lib
        camera = camera if camera is not None else desc.contents.camera
        self.width, self.height, self.count = camera.width, camera.height, spp_count
        self.oracle = oracle_lib.OracleScene(desc)
        rays = _camera_rays(camera, seed, spp_begin, spp_count)
        flat = rays.reshape(-1, 8)
        hits = self.oracle.trace(flat)
        n = flat.shape[0]
        t, u, v = hits[:, 0].copy(), hits[:, 1].copy(), hits[:, 2].copy()
        prim = hits[:, 3].copy().view(np.int32)
        self.hit = prim >= 0
        self.t = t
        origin, direction = flat[:, 0:3], flat[:, 4:7]
        self.direction = direction

        positions = np.asarray(built.positions if positions is None else positions, dtype=F).reshape(-1, 3)
        normals = np.asarray(built.normals, dtype=F).reshape(-1, 3)
        uvs = np.asarray(built.uvs, dtype=F).reshape(-1, 2)
        indices = np.asarray(built.indices, dtype=np.int64).reshape(-1, 3)
        n_tris = len(indices)
        triangle = self.hit & (prim < n_tris)
        sphere = self.hit & (prim >= n_tris)

        self.material = np.full(n, -1, dtype=np.int64)
        self.shading = np.zeros((n, 3), dtype=F)
        self.geometric = np.zeros((n, 3), dtype=F)
        self.uv = np.zeros((n, 2), dtype=F)
        if triangle.any():
            # makeIsect: rtcInterpolate0 with weights (1 - u - v, u, v), the geometric normal where no normal is stored
            corner = indices[prim[triangle]]
            tu, tv = u[triangle], v[triangle]
            w = (F(1) - tu - tv).astype(F)
            interpolate = lambda a0, a1, a2: _fma(w, a0, _fma(tu, a1, (tv * a2).astype(F)))
            self.uv[triangle] = np.stack([interpolate(uvs[corner[:, 0], c], uvs[corner[:, 1], c], uvs[corner[:, 2], c]) for c in range(2)], axis=1)
            shading = np.stack([interpolate(normals[corner[:, 0], c], normals[corner[:, 1], c], normals[corner[:, 2], c]) for c in range(3)], axis=1)
            p0, p1, p2 = positions[corner[:, 0]], positions[corner[:, 1]], positions[corner[:, 2]]
            geometric = _normalized(_xcross((p1 - p0).astype(F), (p2 - p0).astype(F)))
            length = np.sqrt((shading[:, 0] * shading[:, 0] + shading[:, 1] * shading[:, 1] + shading[:, 2] * shading[:, 2]).astype(F))
            shading = np.where((length == 0)[:, None], geometric, shading)
            self.shading[triangle] = _normalized(shading)
            self.geometric[triangle] = geometric
            self.material[triangle] = np.asarray(built.tri_material, dtype=np.int64)[prim[triangle]]
        if sphere.any():
            which = prim[sphere] - n_tris
            centers = np.array([list(built.spheres[i].center_world) for i in which], dtype=F)
            point = (origin[sphere] + (direction[sphere] * t[sphere][:, None]).astype(F)).astype(F)
            geometric = _normalized((point - centers).astype(F))
            self.geometric[sphere] = geometric
            self.shading[sphere] = _normalized(geometric)
            self.material[sphere] = [built.spheres[i].material for i in which]

        # the albedo lookup of every hit whose material has one, and which samples read a varying albedo
        self.kind = np.array([m.type for m in built.materials], dtype=np.int64)
        self.lookup = np.zeros((n, 3), dtype=F)
        self.varying = np.zeros(n, dtype=bool)
        for i in np.nonzero(self.hit)[0]:
            m = built.materials[self.material[i]]
            if m.albedo_type == 0:
                self.lookup[i] = list(m.diffuse)
                continue
            self.varying[i] = True
            if m.albedo_type == 1:   # checkerboard: lambertian f x pi, looked at along the normal
                record = [0, 1] + list(m.diffuse) + [0, 0, 0] + list(m.checker_on) + list(m.checker_off) + list(m.checker_res) + [0, 0, 0, 0]
                f = oracle_lib.evaluate("material_f", record + [0, 0, 1, 0, 0, 1, 0, 0, 1, self.uv[i, 0], self.uv[i, 1]] + [0, 0, 1])
                self.lookup[i] = (f[:3] * F(np.pi)).astype(F)
            else:
                texture = built.textures[m.texture]
                texels = np.ctypeslib.as_array(texture.rgb, shape=(3 * texture.width * texture.height,)).astype(F)
                self.lookup[i] = oracle_lib.evaluate("texture_lookup", np.concatenate([[texture.width, texture.height, self.uv[i, 0], self.uv[i, 1]], texels]))[:3]
        self.built = built

    def _sum(self, per_sample):
        """sequential fp32 adds in sample order: (pixels * spp, c) -> (H, W, c)"""
        per_sample = per_sample.reshape(self.height * self.width, self.count, -1).astype(F)
        total = np.zeros((self.height * self.width, per_sample.shape[2]), dtype=F)
        for k in range(self.count):
            total = (total + per_sample[:, k]).astype(F)
        return total.reshape(self.height, self.width, -1)

    def _any(self, flag):
        return flag.reshape(self.height * self.width, self.count).any(axis=1).reshape(self.height, self.width)

    def features(self):
        diffuse = self.hit & np.isin(self.kind[np.maximum(self.material, 0)], DIFFUSE_KINDS)
        albedo = np.where(diffuse[:, None], self.lookup, F(1))
        albedo = np.where(self.hit[:, None], albedo, F(0)).astype(F)
        return {"albedo": self._sum(albedo), "normal": self._sum(np.where(self.hit[:, None], self.shading, F(0))),
                "depth": self._sum(np.where(self.hit, self.t, F(0))[:, None])[..., 0], "hits": self._sum(self.hit.astype(F)[:, None])[..., 0],
                "varying": self._any(self.varying & diffuse)}

    def reference(self, start_bounce):
        """SampleIntegrator::samplePixel with AlbedoIntegrator::L: rgb sums, and the pixels whose samples are not all constants"""
        lambertian = self.hit & (self.kind[np.maximum(self.material, 0)] == 0)
        color = np.where(lambertian[:, None], self.lookup, np.array([1, 0, 0], dtype=F)[None, :]).astype(F)
        emit = np.array([list(m.emit) for m in self.built.materials], dtype=F)[np.maximum(self.material, 0)]
        wo = (-self.direction).astype(F)
        facing = ((self.geometric[:, 0] * wo[:, 0]).astype(F) + (self.geometric[:, 1] * wo[:, 1]).astype(F) + (self.geometric[:, 2] * wo[:, 2]).astype(F)).astype(F)
        adds_emit = self.hit & (start_bounce <= 0) & (emit != 0).any(axis=1) & ~(facing < 0)
        color = np.where(adds_emit[:, None], (emit + color).astype(F), color)
        color = np.where(self.hit[:, None], color, F(0)).astype(F)
        inexact = self.varying & lambertian
        if self.built.env is not None:
            for i in np.nonzero(~self.hit)[0]:
                color[i] = self.oracle.env_eval("env_emit", -self.direction[i], 3)
            inexact = inexact | ~self.hit
        return self._sum(color), self._any(inexact)


def _assert_features(gpu_images, expected, spp=SPP):
    albedo, normal, depth, hits = gpu_images
    print("feature check: hits mismatches %d, depth mismatches %d, max |albedo diff| %.3g, max |normal diff| %.3g" % (
        int((hits != expected["hits"]).sum()), int((depth != expected["depth"]).sum()),
        float(np.abs(albedo - expected["albedo"]).max()), float(np.abs(normal - expected["normal"]).max())))
    assert np.array_equal(hits, expected["hits"])
    assert np.array_equal(depth, expected["depth"])
    exact = ~expected["varying"]
    assert np.array_equal(albedo[exact], expected["albedo"][exact])
    tolerance = lambda reference: spp * (1e-6 * np.abs(reference) + 2e-7)
    assert np.all(np.abs(albedo - expected["albedo"]) <= tolerance(expected["albedo"]))
    assert np.all(np.abs(normal - expected["normal"]) <= tolerance(expected["normal"]))


# ------------------------------------------------------------------------------------------------------------- scenes

def _material_box():
    """<= 64 triangles: an open room with an emitter and all six material kinds"""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(WIDTH, HEIGHT, origin=(0, 1, 4.5), target=(0, 1, 0), fov_degrees=45.0)
    white = built.material(diffuse=(0.7, 0.6, 0.5))
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], white)                                   # floor
    built.quad([(-2, 0, -2), (-2, 2.4, -2), (2, 2.4, -2), (2, 0, -2)], built.material(type_=_capi.MAT_OREN_NAYAR, diffuse=(0.2, 0.5, 0.3), sigma=0.4))
    built.quad([(-2, 0, 2), (-2, 2.4, 2), (-2, 2.4, -2), (-2, 0, -2)], built.material(type_=_capi.MAT_PLASTIC, diffuse=(0.6, 0.1, 0.1), alpha=0.2))
    built.quad([(2, 0, -2), (2, 2.4, -2), (2, 2.4, 2), (2, 0, 2)], built.material(type_=_capi.MAT_MICROFACET, alpha=0.3))
    built.quad([(-0.5, 2.2, -0.5), (0.5, 2.2, -0.5), (0.5, 2.2, 0.5), (-0.5, 2.2, 0.5)], built.material(diffuse=(0.3, 0.3, 0.3), emit=(5, 4, 3)))
    built.quad([(-0.4, 0.9, -1.9), (0.4, 0.9, -1.9), (0.4, 1.7, -1.9), (-0.4, 1.7, -1.9)], built.material(diffuse=(0.1, 0.1, 0.1), emit=(2, 2, 2)))   # faces the camera
    built.box((-1.2, 0, -0.6), (-0.4, 0.9, 0.2), built.material(type_=_capi.MAT_GLASS, ior=1.5))
    built.box((0.4, 0, -0.4), (1.1, 1.3, 0.3), built.material(type_=_capi.MAT_MIRROR))
    assert len(built.indices) <= 64
    return built, built.finish()


def _grid_vertices(n, phase=0.0):
    ys, xs = np.mgrid[0:n + 1, 0:n + 1]
    x = (xs / n * 4 - 2).astype(F)
    z = (ys / n * 4 - 2).astype(F)
    y = (0.25 * np.sin(2.5 * x + phase) * np.cos(2.0 * z)).astype(F)
    normals = np.stack([(-0.625 * np.cos(2.5 * x + phase) * np.cos(2.0 * z)), np.ones_like(x), (0.5 * np.sin(2.5 * x + phase) * np.sin(2.0 * z))], axis=-1)
    normals = (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(F)
    uvs = np.stack([xs / n * 3.0 - 0.5, ys / n * 2.0], axis=-1).astype(F)
    return np.stack([x, y, z], axis=-1).reshape(-1, 3), normals.reshape(-1, 3), uvs.reshape(-1, 2)


def _bvh_scene(n=48, environment=False, phase=0.0):
    """a wavy grid of 2 n^2 > 4096 triangles with vertex normals and uvs, one half checkerboard, one half textured"""
    from scene_builder import BuiltScene
    built = BuiltScene(WIDTH, HEIGHT, origin=(0.3, 2.2, 3.6), target=(0, 0, 0), fov_degrees=50.0)
    positions, normals, uvs = _grid_vertices(n, phase)
    texels = (np.random.default_rng(5).integers(0, 256, size=(16, 24, 3))).astype(np.uint8)
    checker = built.material(checker=((0.9, 0.8, 0.1), (0.1, 0.2, 0.7), (6.0, 5.0)))
    textured = built.material(texture=built.texture(texels))
    faces = [[], []]
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            faces[0 if i < n // 2 else 1] += [(a, c, b), (a, d, c)]
    built.mesh(positions, faces[0], checker, normals=normals, uvs=uvs)
    built.mesh(positions, faces[1], textured, normals=normals, uvs=uvs)
    if environment:
        rgba = np.random.default_rng(11).random((16, 32, 4)).astype(F)
        built.environment(rgba, scale=1.5)
    else:
        built.quad([(-0.5, 3.0, -0.5), (-0.5, 3.0, 0.5), (0.5, 3.0, 0.5), (0.5, 3.0, -0.5)], built.material(emit=(8, 8, 8)))
    assert len(built.indices) > 4096
    return built, built.finish()


def _sphere_scene():
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(WIDTH, HEIGHT, origin=(0, 1.2, 4.0), target=(0, 0.8, 0), fov_degrees=45.0)
    built.quad([(-3, 0, -3), (3, 0, -3), (3, 0, 3), (-3, 0, 3)], built.material(diffuse=(0.5, 0.5, 0.5)))
    built.sphere((-0.8, 0.8, 0.0), 0.8, built.material(diffuse=(0.2, 0.7, 0.9)))
    built.sphere((0.9, 0.6, 0.4), 0.6, built.material(type_=_capi.MAT_GLASS, ior=1.5))
    built.quad([(-0.5, 3.0, -0.5), (-0.5, 3.0, 0.5), (0.5, 3.0, 0.5), (0.5, 3.0, -0.5)], built.material(emit=(8, 8, 8)))
    return built, built.finish()


SCENES = {"materials": _material_box, "bvh": _bvh_scene, "sphere": _sphere_scene, "environment": lambda: _bvh_scene(environment=True)}


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# -------------------------------------------------------------------------------------------------------------- tests

# beside the values every other test here uses: a seed whose high word matters and eight samples across 2^24, the first
# sample index a float no longer holds (ids of the first rows stay the scene names)
LATE_SEED, LATE_BEGIN = (1 << 63) + 5, (1 << 24) - 3
FEATURE_CASES = [(name, SEED, 0) for name in sorted(SCENES)] + [(name, LATE_SEED, LATE_BEGIN) for name in sorted(SCENES)]


@pytest.mark.parametrize("name, seed, begin", FEATURE_CASES, ids=[name if begin == 0 else name + "-seed-2^63+5-from-sample-2^24-3" for name, _, begin in FEATURE_CASES])
def test_feature_sums_match_the_oracle_derived_expectation(name, seed, begin):
    from pathed_amd.integrator import HipScene
    built, desc = SCENES[name]()
    gpu = HipScene(desc, device=0)
    images = gpu.render_features(seed, begin, SPP)
    expected = Expectation(built, desc, seed=seed, spp_begin=begin).features()
    assert expected["hits"].max() == SPP and (name in ("materials",) or expected["hits"].min() == 0)   # hits and misses both occur
    _assert_features(images, expected)
    stats = gpu.stats()
    assert stats["path_kernel"] == 8 and stats["camera_samples"] == WIDTH * HEIGHT * SPP and stats["closest_rays"] == WIDTH * HEIGHT * SPP
    if begin:
        # the inputs can tell: the low word alone, or the sample index cut to a float's 24 bits, jitter the camera otherwise
        import oracle_lib
        jitter = lambda s, k: [oracle_lib.rng(s, pixel, k, d) for pixel in (0, 1, WIDTH * HEIGHT - 1) for d in (0, 1)]
        assert jitter(seed, begin + 4) != jitter(seed & 0xFFFFFFFF, begin + 4) and jitter(seed, begin + 4) != jitter(seed, begin + 3)   # (2^24 + 1 rounds to 2^24)

    # 3 + 5 samples in two calls are the 8 of one call, bit for bit
    split = gpu.render_features(seed, begin, 3)
    gpu.render_features(seed, begin + 3, 5, *split)
    assert _equal(split, images)

    # a subset of the buffers: the same floats, and the others keep their bits
    albedo, normal, depth, hits = gpu.render_features(seed, begin, SPP, normal=np.zeros((HEIGHT, WIDTH, 3), dtype=F), hits=np.zeros((HEIGHT, WIDTH), dtype=F))
    assert albedo is None and depth is None and np.array_equal(hits, images[3]) and np.array_equal(normal, images[1])


def test_device_buffers_continue_and_untouched_ones_keep_their_bits():
    import torch
    from pathed_amd.integrator import HipScene
    built, desc = _sphere_scene()
    gpu = HipScene(desc, device=0)
    expected = gpu.render_features(SEED, 0, SPP)
    buffers = {name: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
               for name, shape in (("albedo", (HEIGHT, WIDTH, 3)), ("normal", (HEIGHT, WIDTH, 3)), ("depth", (HEIGHT, WIDTH)), ("hits", (HEIGHT, WIDTH)))}
    gpu.render_features_device(SEED, 0, 3, **{k: v.data_ptr() for k, v in buffers.items()})
    gpu.render_features_device(SEED, 3, 5, **{k: v.data_ptr() for k, v in buffers.items()})
    assert _equal([buffers[k].cpu().numpy() for k in ("albedo", "normal", "depth", "hits")], expected)
    before = buffers["albedo"].clone()
    gpu.render_features_device(SEED, 8, 2, depth=buffers["depth"].data_ptr())
    assert torch.equal(buffers["albedo"], before) and not np.array_equal(buffers["depth"].cpu().numpy(), expected[2])


def test_features_follow_the_camera_and_a_refit():
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene
    built, desc = _bvh_scene()
    gpu = HipScene(desc, device=0, refittable=1)
    first = gpu.render_features(SEED, 0, SPP)

    moved = _capi.PathedCamera.from_buffer_copy(desc.contents.camera)
    moved.origin[:] = (-1.5, 1.6, 3.0)
    gpu.set_camera(moved)
    other, other_desc = _bvh_scene()
    other_desc.contents.camera = moved
    fresh = HipScene(other_desc, device=0).render_features(SEED, 0, SPP)
    after = gpu.render_features(SEED, 0, SPP)
    assert _equal(after, fresh) and not np.array_equal(after[2], first[2])
    _assert_features(after, Expectation(other, other_desc).features())

    positions, normals, _ = _grid_vertices(48, phase=0.9)
    quad = slice(2 * len(positions), None)   # the two halves carry the grid's vertices each; the emitter quad keeps its place
    gpu.refit(np.concatenate([positions, positions, np.asarray(built.positions, dtype=F)[quad]]),
              np.concatenate([normals, normals, np.asarray(built.normals, dtype=F)[quad]]))
    bent, bent_desc = _bvh_scene(phase=0.9)
    bent_desc.contents.camera = moved
    fresh = HipScene(bent_desc, device=0).render_features(SEED, 0, SPP)
    refitted = gpu.render_features(SEED, 0, SPP)
    assert _equal(refitted, fresh) and not np.array_equal(refitted[2], after[2])


def test_the_three_builders_give_identical_feature_images():
    from pathed_amd.integrator import HipScene
    built, desc = _bvh_scene()
    images = {builder: HipScene(desc, device=0, bvh_builder=builder).render_features(SEED, 0, SPP) for builder in ("sah", "lbvh", "ploc")}
    assert _equal(images["lbvh"], images["sah"]) and _equal(images["ploc"], images["sah"])


def _assert_reference(image, expected, inexact, spp=SPP):
    print("albedo integrator: max |diff| %.3g over %d inexact pixels, %d exact pixels differ" % (
        float(np.abs(image - expected).max()), int(inexact.sum()), int((image[~inexact] != expected[~inexact]).any(axis=-1).sum())))
    assert np.array_equal(image[~inexact], expected[~inexact])
    assert np.all(np.abs(image - expected) <= spp * (1e-6 * np.abs(expected) + 2e-7))


def test_albedo_integrator_is_the_references():
    """set_integrator("AlbedoIntegrator") + render: emission at bounce 0 when the window counts it, the Lambertian albedo,
    (1, 0, 0) for every other material, the environment on a miss; PathTracer afterwards renders the path tracer's bits."""
    from pathed_amd.integrator import HipScene
    built, desc = _material_box()
    gpu = HipScene(desc, device=0)
    beauty = gpu.render(SEED, 0, SPP, 0, 3)
    expectation = Expectation(built, desc)

    gpu.set_integrator("AlbedoIntegrator")
    with_emission = gpu.render(SEED, 0, SPP, 0, 3)            # an emitter in view, window 0..3
    expected, inexact = expectation.reference(start_bounce=0)
    _assert_reference(with_emission, expected, inexact)
    assert gpu.stats()["path_kernel"] == 8
    without = gpu.render(SEED, 0, SPP, 1, 3)                  # a window that starts at 1: no emission
    expected_without, inexact = expectation.reference(start_bounce=1)
    _assert_reference(without, expected_without, inexact)
    assert np.array_equal(gpu.render(SEED, 0, SPP, 1, -1), without)   # last_bounce is ignored
    assert (with_emission != without).any() and with_emission.max() > 4.0
    # glass answers (1, 0, 0): some pixel sees nothing but the glass box, sample after sample
    glass = [i for i, m in enumerate(built.materials) if m.type == 4][0]
    only_glass = (expectation.material.reshape(-1, SPP) == glass).all(axis=1).reshape(HEIGHT, WIDTH)
    assert only_glass.any() and np.array_equal(without[only_glass], np.tile(np.array([SPP, 0, 0], dtype=F), (int(only_glass.sum()), 1)))
    # 3 + 5 samples onto a device buffer continue like 8 (pathed_hip_render adds a call's own sum on the host instead)
    import torch
    sums = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
    gpu.render_device(SEED, 0, 3, 0, 3, sums.data_ptr())
    gpu.render_device(SEED, 3, 5, 0, 3, sums.data_ptr())
    assert np.array_equal(sums.cpu().numpy(), with_emission)

    gpu.set_integrator("PathTracer")
    assert np.array_equal(gpu.render(SEED, 0, SPP, 0, 3), beauty)
    assert gpu.stats()["path_kernel"] != 8

    # environment misses: within the env_emit tolerance
    built, desc = _bvh_scene(environment=True)
    gpu = HipScene(desc, device=0)
    gpu.set_integrator("AlbedoIntegrator")
    expected, inexact = Expectation(built, desc).reference(start_bounce=0)
    assert inexact.any()
    _assert_reference(gpu.render(SEED, 0, SPP, 0, 3), expected, inexact)


def _stack_rungs(bound):
    """the LDS row counts that hold a stack of `bound` entries without a spill: the default (the rule of configureTrace) and up"""
    default = 8 if bound <= 8 else 16 if bound <= 16 else 22
    return [rows for rows in (8, 16, 22) if rows >= default]


def _shallow_room():
    """8 triangles under intersector="bvh": leaves of <= 2 triangles make <= 7 leaves, which two 4-wide levels always hold"""
    from scene_builder import BuiltScene
    built = BuiltScene(16, 12, origin=(0, 1, 4.5), target=(0, 1, 0), fov_degrees=45.0)
    built.quad([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)], built.material(diffuse=(0.7, 0.6, 0.5)))
    built.quad([(-2, 0, -2), (-2, 2.4, -2), (2, 2.4, -2), (2, 0, -2)], built.material(checker=((0.9, 0.8, 0.1), (0.1, 0.2, 0.7), (6.0, 5.0))))
    built.quad([(-2, 0, 2), (-2, 2.4, 2), (-2, 2.4, -2), (-2, 0, -2)], built.material(diffuse=(0.6, 0.1, 0.1)))
    built.quad([(-0.5, 2.2, -0.5), (0.5, 2.2, -0.5), (0.5, 2.2, 0.5), (-0.5, 2.2, 0.5)], built.material(diffuse=(0.3, 0.3, 0.3), emit=(5, 4, 3)))
    assert len(built.indices) == 8
    return built, built.finish()


@pytest.mark.parametrize("reference", [False, True], ids=["features", "albedo-integrator"])
def test_every_stack_row_count_gives_the_same_bits(reference):
    """k_features<8 | 16 | 22, REFERENCE> (launchFeatures): the row count the scene takes by default and every larger one"""
    from pathed_amd.integrator import HipScene
    built, desc = _shallow_room()   # (`built` owns the arrays `desc` points to)

    def images(rows):
        gpu = HipScene(desc, device=0, stack_rows=rows, intersector="bvh")
        assert 3 * gpu.stats()["bvh_max_depth"] + 1 <= 8   # the default is 8 rows: all three rungs run, none spills
        if not reference:
            return gpu.render_features(SEED, 0, 4)
        gpu.set_integrator("AlbedoIntegrator")
        image = gpu.render(SEED, 0, 4, 0, 3)
        assert gpu.stats()["path_kernel"] == 8
        return [image]

    default = images(0)
    assert all(image.any() for image in default)
    for rows in _stack_rungs(8):
        assert _equal(images(rows), default), rows


def test_argument_errors():
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene
    from scene_builder import BuiltScene
    lib = _capi.load_hip()
    built = BuiltScene(WIDTH, HEIGHT, origin=(0, 1, 5), target=(0, 1, 0))
    built.quad([(-3, 0, -3), (3, 0, -3), (3, 0, 3), (-3, 0, 3)], built.material())
    built.box((-1, 0.2, -1), (1, 2.2, 1), built.material(type_=_capi.MAT_PASSTHROUGH), medium=built.medium((0.5, 0.5, 0.5), (0.4, 0.4, 0.4)))
    built.quad([(-0.5, 3.0, -0.5), (-0.5, 3.0, 0.5), (0.5, 3.0, 0.5), (0.5, 3.0, -0.5)], built.material(emit=(8, 8, 8)))
    gpu = HipScene(built.finish(), device=0)
    depth = np.zeros((HEIGHT, WIDTH), dtype=F)
    pointer = depth.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.pathed_hip_render_features(gpu._handle, 1, 0, 1, None, None, pointer, None) == -4   # PATHED_E_UNSUPPORTED
    assert b"passthrough" in lib.pathed_hip_last_error()
    gpu.set_integrator("AlbedoIntegrator")
    rgb = np.zeros((HEIGHT, WIDTH, 3), dtype=F)
    assert lib.pathed_hip_render(gpu._handle, 1, 0, 1, 0, 3, rgb.ctypes.data_as(C.POINTER(C.c_float))) == -4

    plain, desc = _sphere_scene()
    gpu = HipScene(desc, device=0)
    assert lib.pathed_hip_render_features(gpu._handle, 1, 0, 1, None, None, None, None) == -1   # PATHED_E_INVALID
    assert lib.pathed_hip_render_features_device(gpu._handle, 1, 0, 1, C.byref(_capi.PathedFeatureBuffers()), None) == -1
    assert lib.pathed_hip_render_features_device(gpu._handle, 1, 0, 1, None, None) == -1
    assert lib.pathed_hip_render_features(None, 1, 0, 1, None, None, pointer, None) == -1
    assert lib.pathed_hip_render_features(gpu._handle, 1, 0, 0, None, None, pointer, None) == 0 and not depth.any()   # spp_count == 0: nothing to do


# --------------------------------------------------------------------------------------------------------------- host

def _read_exr(path):
    from pathed_amd import _capi
    host = _capi.load_host()
    w, h = C.c_int(), C.c_int()
    assert host.pathed_host_read_exr_rgba(path.encode(), C.byref(w), C.byref(h), None, 0) == 0, host.pathed_host_last_error()
    data = np.zeros((h.value, w.value, 4), dtype=F)
    assert host.pathed_host_read_exr_rgba(path.encode(), C.byref(w), C.byref(h), data.ctypes.data_as(C.POINTER(C.c_float)), data.size) == 0
    return data


def _run_job(tmp_path, name, job, runner="cpp"):
    from pathed_amd import _capi
    out_dir = str(tmp_path / name)
    job = dict(job, output_directory=out_dir)
    job_path = str(tmp_path / (name + ".json"))
    json.dump(job, open(job_path, "w"))
    if runner == "cpp":
        command = [os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed"), job_path, _capi.REPO_ROOT]
    else:
        command = [sys.executable, "-m", "pathed_amd.run_job", job_path, _capi.REPO_ROOT]
    result = subprocess.run(command, capture_output=True, text=True, cwd=_capi.REPO_ROOT)
    return out_dir, result


FEATURE_FILES = ["auto-%s%s.exr" % (name, suffix) for name in ("albedo", "normal", "depth") for suffix in ("", "-00008spp", "-00016spp")]


def test_executable_writes_the_feature_images(tmp_path):
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(width=72, height=56, spp=16, features=["depth", "albedo", "normal"])
    straight_dir, result = _run_job(tmp_path, "straight", job)
    assert result.returncode == 0, result.stdout + result.stderr
    for name in FEATURE_FILES:
        assert os.path.exists(os.path.join(straight_dir, name)), name

    scene = LoadedScene(job["scene"], 72, 56)
    albedo, normal, depth, hits = HipScene(scene.desc, device=0).render_features(int(job.get("seed", 1)), 0, 16)
    half = lambda image: image[::-1].astype(np.float16).astype(F)   # Image::set flips; the writer rounds to HALF
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_depth = np.where(hits > 0, depth / hits, F(0)).astype(F)
    assert np.array_equal(_read_exr(os.path.join(straight_dir, "auto-albedo-00016spp.exr"))[..., :3], half(albedo / F(16)))
    assert np.array_equal(_read_exr(os.path.join(straight_dir, "auto-normal.exr"))[..., :3], half(normal / F(16)))
    assert np.array_equal(_read_exr(os.path.join(straight_dir, "auto-depth-00016spp.exr"))[..., :3], half(np.repeat(mean_depth[..., None], 3, axis=2)))

    # without the key nothing changes: no feature file, the same auto.exr
    plain_dir, result = _run_job(tmp_path, "plain", {k: v for k, v in job.items() if k != "features"})
    assert result.returncode == 0 and not [f for f in os.listdir(plain_dir) if f.startswith("auto-albedo")]
    assert open(os.path.join(plain_dir, "auto.exr"), "rb").read() == open(os.path.join(straight_dir, "auto.exr"), "rb").read()

    # a resumed job's feature files are the straight run's; so are those of two replicas
    _, result = _run_job(tmp_path, "resumed", dict(job, spp=8))
    assert result.returncode == 0, result.stdout + result.stderr
    resumed_dir, result = _run_job(tmp_path, "resumed", dict(job, resume=True))
    assert result.returncode == 0 and "resuming at sample 8/16" in result.stdout, result.stdout + result.stderr
    two_dir, result = _run_job(tmp_path, "two", dict(job, gpus=[0, 0]))
    assert result.returncode == 0, result.stdout + result.stderr
    for name in FEATURE_FILES:
        blob = open(os.path.join(straight_dir, name), "rb").read()
        assert open(os.path.join(resumed_dir, name), "rb").read() == blob, name
        assert open(os.path.join(two_dir, name), "rb").read() == blob, name

    _, result = _run_job(tmp_path, "unknown", dict(job, features=["albedo", "roughness"]))
    assert result.returncode != 0 and "roughness" in result.stderr


def test_albedo_integrator_through_both_launchers(tmp_path):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(width=64, height=48, spp=8, integrator="AlbedoIntegrator", features=["albedo"])
    images = {}
    for runner in ("cpp", "py"):
        out_dir, result = _run_job(tmp_path, runner, job, runner)
        assert result.returncode == 0, result.stdout + result.stderr
        images[runner] = (open(os.path.join(out_dir, "auto.exr"), "rb").read(), open(os.path.join(out_dir, "auto-albedo-00008spp.exr"), "rb").read())
    assert images["cpp"] == images["py"]
    image = _read_exr(os.path.join(str(tmp_path / "cpp"), "auto.exr"))[..., :3]
    assert image.max() > 0.5 and np.isfinite(image).all()
