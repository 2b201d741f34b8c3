"""The fused path kernel's pass over all items leaves out the triangles that are bit-for-bit copies of a triangle with a lower
primitive id (pathed_amd/csrc/small_items.h: NEVER-HIT; kernels.h: kSmallPassList): the Cornell file's two "Bottom Face" lines
name an earlier side face again.  A copy can change no hit -- same bits, same t, u, v on every ray, and of two equal hits the
lower id wins whatever the order -- so: the default render is the bytes of the library's own full pass (the counting
instantiation) and of the per-slot wavefront path, before and after a camera move; on ray pairs built the way sampleLightsTerm
builds them, a quarter leaving or grazing a copied face, the lowest-id member of the class of everything phase 2 accepts is a
candidate of the pass and no left-out primitive ever is; Cornell reports the layout the host test derives, and a scene without
copies a pass layout equal to its item layout."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP, BOUNCES = 16, (0, 5)


def room(built, material):
    """Five walls of an axis-aligned room open towards +z."""
    (x0, y0, z0), (x1, y1, z1) = (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0)
    for corners in ([(x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0)], [(x0, y1, z1), (x0, y1, z0), (x1, y1, z0), (x1, y1, z1)],
                    [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], [(x0, y0, z1), (x0, y0, z0), (x0, y1, z0), (x0, y1, z1)],
                    [(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)]):
        built.quad(corners, material)


BOX_LO, BOX_HI = (-0.6, 0.0, -0.5), (-0.1, 0.6, 0.0)
# the box's front face (z = hi) as scene_builder's box() lists its corners: quad() splits it into the same two triangles
BOX_FRONT = [(BOX_LO[0], BOX_LO[1], BOX_HI[2]), (BOX_HI[0], BOX_LO[1], BOX_HI[2]), (BOX_HI[0], BOX_HI[1], BOX_HI[2]), (BOX_LO[0], BOX_HI[1], BOX_HI[2])]
LIGHT = [(-0.25, 1.9, 0.25), (-0.25, 1.9, -0.25), (0.25, 1.9, -0.25), (0.25, 1.9, 0.25)]
LONE = [(0.2, 0.3, 0.4), (0.7, 0.3, 0.4), (0.7, 0.8, 0.1)]


def build(kind):
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.7, 0.7, 0.7))
    blue = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.2, 0.5, 0.7))
    red = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.7, 0.2, 0.1))
    light = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0, 0, 0), emit=(12.0, 11.0, 9.0))
    surface = blue
    if kind == "ggx":        # the rough-over-GGX rung of the launch ladder
        surface = built.material(_capi.MAT_MICROFACET, diffuse=(0.6, 0.6, 0.3), alpha=0.3)
        built.materials[surface].distribution = 1
    elif kind == "beckmann":  # the rough-over-Beckmann rung
        surface = built.material(_capi.MAT_MICROFACET, diffuse=(0.6, 0.6, 0.3), alpha=0.3)
    elif kind == "glass":    # the smooth rung
        surface = built.material(_capi.MAT_GLASS, ior=1.5)
    elif kind == "checker":  # a varying albedo: the generic instantiation
        surface = built.material(_capi.MAT_LAMBERTIAN, checker=((0.8, 0.8, 0.8), (0.1, 0.1, 0.1), (4.0, 4.0)))
    room(built, grey)
    if kind == "sphere-light":
        built.sphere((0.1, 1.5, 0.0), 0.15, light)
    else:
        built.quad(LIGHT, light)
    built.box(BOX_LO, BOX_HI, surface)
    built.mesh(LONE, [(0, 1, 2)], blue)
    if kind in ("copy", "ggx", "beckmann", "glass", "checker", "sphere-light"):
        built.quad(BOX_FRONT, surface)
    elif kind == "copy-material":
        built.quad(BOX_FRONT, red)
    elif kind == "copy-emitter":
        built.quad(LIGHT, light)
    elif kind == "triple":
        built.quad(BOX_FRONT, surface)
        built.quad(BOX_FRONT, red)
    elif kind == "copy-lone":
        built.mesh(LONE, [(0, 1, 2)], red)
    else:
        assert kind == "plain"
    emitters = {k for k, m in enumerate(built.tri_material) if any(built.materials[m].emit)}
    sphere_lights = [(s.center_sample[0], s.center_sample[1], s.center_sample[2], s.radius) for s in built.spheres]
    return built.finish(), built, emitters, sphere_lights


KINDS = ["copy", "copy-material", "copy-emitter", "triple", "copy-lone", "plain", "sphere-light", "ggx", "beckmann", "glass", "checker"]
NAMES = ["cornell"] + KINDS
# primitives left out of the pass: the copies were added last (room 10, light 2 -- none with the sphere --, box 12, lone 1)
EXPECTED_NEVER_HIT = {
    "cornell": 3 << 20 | 3 << 32, "copy": 3 << 25, "copy-material": 3 << 25, "copy-emitter": 3 << 25, "triple": 15 << 25, "copy-lone": 1 << 25,
    "plain": 0, "sphere-light": 3 << 23, "ggx": 3 << 25, "beckmann": 3 << 25, "glass": 3 << 25, "checker": 3 << 25,
}


@pytest.fixture(scope="module")
def built_scenes():
    from pathed_amd.scene import LoadedScene
    loaded = LoadedScene("scenes/cornell.json", 48, 32)
    out = {"cornell": (loaded.desc, loaded, {34, 35}, [])}
    for kind in KINDS:
        out[kind] = build(kind)
    return out


def classes_of(tris):
    """keeper[p] = the lowest primitive id among the triangles whose (v0, e1, e2) are p's bit for bit."""
    prims = tris[:, 3].copy().view(np.int32)
    keys = [tris[k, [0, 1, 2, 4, 5, 6, 8, 9, 10]].tobytes() for k in range(len(tris))]
    lowest = {}
    for k, key in enumerate(keys):
        lowest[key] = min(lowest.get(key, 1 << 30), int(prims[k]))
    return {int(prims[k]): lowest[keys[k]] for k in range(len(tris))}


@pytest.mark.parametrize("name", NAMES)
def test_renders_without_the_copies_are_the_bytes_of_the_full_pass_and_of_the_wavefront_path(built_scenes, name):
    from pathed_amd.integrator import HipScene
    desc, _, _, _ = built_scenes[name]
    gpu = HipScene(desc, device=0)
    assert gpu.stats()["path_kernel"] == 3, gpu.stats()["path_kernel"]    # the fused kernel
    _, tris = gpu.export_bvh()
    n = len(tris)
    empty = np.zeros((0, 10), dtype=np.float32)
    _, order, counts, never_hit = gpu.pass_candidates(empty, n)
    print(name, counts, hex(never_hit), order.tolist())
    assert never_hit == EXPECTED_NEVER_HIT[name], hex(never_hit)
    keeper = classes_of(tris)
    assert never_hit == sum(1 << p for p, k in keeper.items() if k != p)
    kept = sorted(p for p, k in keeper.items() if k == p)
    assert counts["triangles"] == len(kept) and 2 * counts["quads"] + counts["lone"] == len(kept)
    assert sorted(order[:len(kept)].tolist()) == kept and (order[len(kept):] == -1).all()
    if name == "plain":
        # no copies: the pass list is the item list
        _, item_counts, _ = gpu.shadow_candidates(empty)
        assert {key: counts[key] for key in item_counts} == item_counts and counts["triangles"] == n
        assert np.array_equal(order, gpu.item_order(n))
    image = gpu.render(5, 0, SPP, *BOUNCES)
    assert image.any()
    counting = HipScene(desc, device=0)
    counting.set_stats_mode(count=True)                                    # the counting instantiation: the full list for both rays
    assert np.array_equal(counting.render(5, 0, SPP, *BOUNCES), image)
    per_slot = HipScene(desc, device=0, shade_kernel="per-slot")
    assert np.array_equal(per_slot.render(5, 0, SPP, *BOUNCES), image)
    # another view: both lists, their records and the camera masks are rebuilt
    camera = copy.copy(desc.contents.camera)
    camera.origin = (C.c_float * 3)(0.6, 1.4, 5.0)
    for scene in (gpu, counting, per_slot):
        scene.set_camera(camera)
    _, _, moved_counts, moved_never_hit = gpu.pass_candidates(empty, n)
    assert moved_never_hit == never_hit and moved_counts["triangles"] == counts["triangles"]
    moved = gpu.render(6, 0, SPP, *BOUNCES)
    assert moved.any() and not np.array_equal(moved, image)
    assert np.array_equal(counting.render(6, 0, SPP, *BOUNCES), moved)
    assert np.array_equal(per_slot.render(6, 0, SPP, *BOUNCES), moved)


def ray_pairs(tris, emitters, sphere_lights, faces, rng, n):
    """Ray pairs as a path vertex has them: an origin on a scene triangle, a continuation direction, and sampleLightsTerm's shadow
    ray -- float32 direction to a point on an emitter, normalised, tfar = distance - 1e-3.  A quarter of the origins lie on a
    triangle of `faces` (inside, on an edge, on a corner), displaced along its normal by 0, +-1, +-4 ulps of the scene's size; half
    of those continue within the face's plane (grazing it), the others leave it.  Returns (rays (m, 10) float32, special (m,) bool)."""
    corners = np.stack([tris[:, 0:3], tris[:, 0:3] + tris[:, 4:7], tris[:, 0:3] + tris[:, 8:11]], axis=1).astype(np.float64)   # (T, 3, 3)
    prims = tris[:, 3].copy().view(np.int32)
    extent = float(np.linalg.norm(corners.reshape(-1, 3).max(axis=0) - corners.reshape(-1, 3).min(axis=0)))
    ulp = float(np.spacing(np.float32(extent)))

    def barycentric(count, kinds):
        a, b = rng.random(count), rng.random(count)
        flip = a + b > 1.0
        a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
        which = rng.integers(0, 3, count)
        edge, corner = kinds == 1, kinds == 2
        b[edge & (which == 0)] = 0.0
        a[edge & (which == 1)] = 0.0
        b[edge & (which == 2)] = 1.0 - a[edge & (which == 2)]
        a[corner], b[corner] = (which[corner] == 1).astype(np.float64), (which[corner] == 2).astype(np.float64)
        return a, b

    def points(index, a, b):
        c = corners[index]
        return c[:, 0] + a[:, None] * (c[:, 1] - c[:, 0]) + b[:, None] * (c[:, 2] - c[:, 0])

    def unit(count):
        v = rng.normal(size=(count, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n_special = n // 4
    face_rows = np.array([k for k in range(len(tris)) if int(prims[k]) in faces], dtype=np.int64)
    index = np.concatenate([rng.integers(0, len(tris), n - n_special), face_rows[rng.integers(0, len(face_rows), n_special)]])
    special = np.arange(n) >= n - n_special
    kinds = np.where(special, rng.integers(0, 3, n), 0)
    origins = points(index, *barycentric(n, kinds))
    normal = np.cross(corners[index, 1] - corners[index, 0], corners[index, 2] - corners[index, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    steps = np.where(special, np.array([0.0, 1.0, -1.0, 4.0, -4.0])[rng.integers(0, 5, n)], 0.0)
    origins = origins + normal * (steps * ulp)[:, None]
    # continuation: any direction; grazing: towards another point of the face's plane (inside the face or beyond its edges)
    direction = unit(n)
    grazing = special & (rng.random(n) < 0.5)
    a, b = rng.uniform(-0.5, 1.5, n), rng.uniform(-0.5, 1.5, n)
    within = points(index, a, b) - points(index, *barycentric(n, np.zeros(n, dtype=np.int64)))
    within /= np.maximum(np.linalg.norm(within, axis=1, keepdims=True), 1e-30)
    direction[grazing] = within[grazing]
    # ... and a sixth of the other rays aim at a point of those triangles: the faces are small, the rays have to meet them
    aimed = ~special & (rng.random(n) < 1.0 / 6.0)
    towards = points(face_rows[rng.integers(0, len(face_rows), n)], *barycentric(n, rng.integers(0, 3, n))) - origins
    towards /= np.maximum(np.linalg.norm(towards, axis=1, keepdims=True), 1e-30)
    direction[aimed] = towards[aimed]
    # the light sample
    if sphere_lights:
        sphere = np.array(sphere_lights, dtype=np.float64)[rng.integers(0, len(sphere_lights), n)]
        targets = sphere[:, 0:3] + sphere[:, 3:4] * unit(n)
    else:
        lights = np.array([k for k in range(len(tris)) if int(prims[k]) in emitters], dtype=np.int64)
        targets = points(lights[rng.integers(0, len(lights), n)], *barycentric(n, rng.integers(0, 3, n)))
    origins32, targets32 = origins.astype(np.float32), targets.astype(np.float32)
    delta = targets32 - origins32
    distance = np.sqrt((delta * delta).sum(axis=1, dtype=np.float32), dtype=np.float32)
    keep = distance > np.float32(2e-3)
    shadow = (delta / np.maximum(distance, np.float32(1e-30))[:, None]).astype(np.float32)
    rays = np.concatenate([origins32, direction.astype(np.float32), shadow, (distance - np.float32(1e-3))[:, None]], axis=1).astype(np.float32)
    return rays[keep], special[keep]


@pytest.mark.parametrize("name", NAMES)
def test_what_phase_two_accepts_is_a_candidate_of_the_pass_through_its_lowest_copy(built_scenes, name):
    from pathed_amd.integrator import HipScene
    desc, _, emitters, sphere_lights = built_scenes[name]
    gpu = HipScene(desc, device=0)
    _, tris = gpu.export_bvh()
    keeper = classes_of(tris)
    copied = {k for p, k in keeper.items() if k != p}
    faces = copied if copied else {12, 13}    # (the room without copies: a box face stands in)
    rays, special = ray_pairs(tris, emitters, sphere_lights, faces, np.random.default_rng(21), 20000)
    assert len(rays) > 19000 and special.mean() > 0.2
    out, _, counts, never_hit = gpu.pass_candidates(rays, len(tris))
    assert never_hit == EXPECTED_NEVER_HIT[name]
    full = gpu.small_candidates(rays)
    for ray, (candidates, accepted) in enumerate(((out[:, 0], full[:, 4]), (out[:, 1], full[:, 5]))):
        # every accepted primitive, through the lowest id of its class
        through = accepted.copy()
        for p, k in keeper.items():
            if k != p:
                has = (accepted >> np.uint64(p) & np.uint64(1)) != 0
                through[has] = (through[has] & ~np.uint64(1 << p)) | np.uint64(1 << k)
        lost = through & ~candidates
        on_classes = np.count_nonzero(through & np.uint64(sum(1 << k for k in copied)))
        print(name, "path ray" if ray == 0 else "shadow ray", "rays", len(rays), "accept something %.3f" % (np.count_nonzero(accepted) / len(rays)),
              "a copied triangle %.3f" % (on_classes / len(rays)), "candidates per ray %.2f" % np.mean([bin(int(c)).count("1") for c in candidates[:2000]]))
        # the check is not vacuous: a quarter of the path rays and a twentieth of the shadow rays meet something (half of the
        # continuation directions leave the room through the surface they start on; most light samples are visible) ...
        assert np.count_nonzero(accepted) >= (0.25 if ray == 0 else 0.05) * len(rays)
        if copied and ray == 0:
            assert on_classes >= 0.02 * len(rays)                        # ... and the path rays do meet the copied triangles
        assert not lost.any(), (int(np.count_nonzero(lost)), hex(int(lost[np.flatnonzero(lost)[0]])))
        assert not (candidates & np.uint64(never_hit)).any()


def test_cornell_reports_the_pass_layout_of_the_host_rule(built_scenes):
    from pathed_amd.integrator import HipScene
    desc, _, _, _ = built_scenes["cornell"]
    gpu = HipScene(desc, device=0)
    _, order, counts, never_hit = gpu.pass_candidates(np.zeros((0, 10), dtype=np.float32), 36)
    assert counts == {"quads": 15, "lone": 2, "shadow_quad_pairs": 6, "shadow_lone_pairs": 0, "triangles": 32}, counts
    assert never_hit == (3 << 20 | 3 << 32), hex(never_hit)
    assert not {20, 21, 32, 33} & set(order.tolist()) and (order[32:] == -1).all()
    # what the existing hooks report is what it was
    _, item_counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
    assert item_counts == {"quads": 17, "lone": 2, "shadow_quad_pairs": 7, "shadow_lone_pairs": 0} and never == 0x3F3
    assert sorted(gpu.item_order(36).tolist()) == list(range(36))
