"""Shadow rays of the fused path kernel skip the items that can never occlude a light sample (pathed_amd/csrc/small_items.h:
NEVER-OCCLUDERS; kernels.h: smallCandidatesItems<PRUNE>): the walls of a room go last in item order and the shadow ray's half of
phase 1 stops before them.  Three checks: the renders are the bytes of the library's own full pass (the counting instantiation)
and of the per-slot wavefront path; on rays built the way sampleLightsTerm builds them, everything phase 2 accepts is among the
pruned candidates; the Cornell box reports the layout the host test derives."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CORNELL_NEVER = 0x3F3   # floor (0, 1), back wall (4, 5), right wall (6, 7), the left wall's two triangles (8, 9)


def popcount(word):
    return bin(int(word)).count("1")


def room(built, materials, skip=(), lo=(-1.0, 0.0, -1.0), hi=(1.0, 2.0, 1.0)):
    """Five (or fewer) walls of an axis-aligned room open towards +z: floor, ceiling, back, left, right."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    walls = {
        "floor": [(x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0)],
        "ceiling": [(x0, y1, z1), (x0, y1, z0), (x1, y1, z0), (x1, y1, z1)],
        "back": [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)],
        "left": [(x0, y0, z1), (x0, y0, z0), (x0, y1, z0), (x0, y1, z1)],
        "right": [(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)],
    }
    for name, corners in walls.items():
        if name not in skip:
            built.quad(corners, materials[name] if isinstance(materials, dict) else materials)


def cornell_with_light_at(height):
    """The Cornell file's geometry with the light moved to y = height (Lambertian greys: the layout is what matters)."""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    built = BuiltScene(48, 32, (0.0, 1.0, 6.8), (0.0, 1.0, 0.0), fov_degrees=19.5)
    grey = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.7, 0.7, 0.7))
    red = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.6, 0.1, 0.1))
    light = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.78, 0.78, 0.78), emit=(17.0, 12.0, 4.0))
    vertices, name = [], ""
    import os
    for line in open(os.path.join(_capi.REPO_ROOT, "scenes", "CornellBox-Original.obj")):
        words = line.split()
        if not words:
            continue
        if words[0] == "v":
            vertices.append([float(w) for w in words[1:4]])
        elif words[0] == "usemtl":
            name = words[1]
        elif words[0] == "f":
            corners = np.array([vertices[int(w)] for w in words[1:]], dtype=np.float64)
            if name == "light":
                corners[:, 1] = height
            built.quad(corners, light if name == "light" else red if name == "leftWall" else grey)
    return built.finish(), built


def scenes():
    """name -> (descriptor pointer, keep-alive, what the layout must show)"""
    from pathed_amd import _capi
    from pathed_amd.scene import LoadedScene
    from scene_builder import BuiltScene
    out = {}
    loaded = LoadedScene("scenes/cornell.json", 48, 32)
    out["cornell"] = (loaded.desc, loaded, lambda counts, never: never == CORNELL_NEVER and counts["shadow_quad_pairs"] == 7 and counts["shadow_lone_pairs"] == 0)
    desc, keep = cornell_with_light_at(1.2)
    out["cornell-low-light"] = (desc, keep, lambda counts, never: never == CORNELL_NEVER | 0xC and counts["shadow_quad_pairs"] == 7)

    def lambertians(built):
        return (built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.7, 0.7, 0.7)), built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.2, 0.5, 0.7)),
                built.material(_capi.MAT_LAMBERTIAN, diffuse=(0, 0, 0), emit=(12.0, 11.0, 9.0)))

    built = BuiltScene(48, 32, (0.5, 5.0, 5.0), (0, 0.5, 0), fov_degrees=35.0)
    grey, blue, light = lambertians(built)
    built.quad([(-1, 1.0, 1), (1, 1.0, 1), (1, 0.0, -1), (-1, 0.0, -1)], grey)      # two quads that cross each other in the open, facing up
    built.quad([(-1, 0.0, 1), (1, 0.0, 1), (1, 1.0, -1), (-1, 1.0, -1)], blue)
    built.quad([(-0.5, 2.5, 0.5), (-0.5, 2.5, -0.5), (0.5, 2.5, -0.5), (0.5, 2.5, 0.5)], light)
    out["open"] = (built.finish(), built, lambda counts, never: never == 0 and counts["shadow_quad_pairs"] == (counts["quads"] + 1) // 2)

    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey, blue, light = lambertians(built)
    room(built, grey)
    built.quad([(-0.25, 1.1, 0.25), (-0.25, 1.1, -0.25), (0.25, 1.1, -0.25), (0.25, 1.1, 0.25)], light)
    built.box((-0.6, 0.0, -0.5), (-0.1, 0.6, 0.0), blue)                                # six faces; the bottom one lies in the floor
    built.quad([(0.2, 0.3, 0.4), (0.7, 0.3, 0.4), (0.7, 0.8, 0.1), (0.2, 0.8, 0.1)], blue)   # a loose plate
    # occluders: the light, the plate and the box faces but the bottom one -- an odd count, whatever becomes of the bottom face
    out["odd"] = (built.finish(), built, lambda counts, never: popcount(never) >= 10 and (counts["quads"] - popcount(never) // 2) % 2 == 1
                  and counts["shadow_quad_pairs"] == (counts["quads"] - popcount(never) // 2 + 1) // 2)

    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey, blue, light = lambertians(built)
    # walls of two triangles that share one corner only (a sliver apart along the diagonal): they find no partner
    built.mesh([(-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, -1.0), (0.9, 0.0, -1.0), (-1.0, 0.0, -1.0)], [(0, 1, 2), (0, 3, 4)], grey)     # floor
    built.mesh([(-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (1.0, 2.0, -1.0), (0.9, 2.0, -1.0), (-1.0, 2.0, -1.0)], [(0, 1, 2), (0, 3, 4)], grey)   # back wall
    built.quad([(-0.25, 1.1, 0.5), (-0.25, 1.1, 0.0), (0.25, 1.1, 0.0), (0.25, 1.1, 0.5)], light)
    built.box((-0.3, 0.05, -0.4), (0.2, 0.5, 0.1), blue)                                 # (off the floor: its bottom face is no never-occluder)
    out["lone"] = (built.finish(), built, lambda counts, never: never == 0xF and counts["lone"] == 4 and counts["shadow_lone_pairs"] < (counts["lone"] + 1) // 2)

    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey, blue, light = lambertians(built)
    glass = built.material(_capi.MAT_GLASS, ior=1.5)
    mirror = built.material(_capi.MAT_MIRROR)
    room(built, {"floor": grey, "ceiling": grey, "back": mirror, "left": blue, "right": grey})
    built.quad([(-0.25, 1.1, 0.25), (-0.25, 1.1, -0.25), (0.25, 1.1, -0.25), (0.25, 1.1, 0.25)], light)
    built.box((-0.5, 0.0, -0.3), (0.3, 0.7, 0.4), glass)                                 # paths run inside the glass
    # (only the Cornell-like instantiation prunes -- kernels.h kSmallPrunes -- so in this scene and the two sphere-lit ones the
    # render's equality says little; their layout checks judge the host rule, and the hook
    # always prunes: test_origins_on_and_inside_glass_lose_no_hit_to_the_pruning feeds it origins on the glass box)
    out["glass"] = (built.finish(), built, lambda counts, never: popcount(never) >= 10)

    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey, blue, light = lambertians(built)
    room(built, grey)
    built.sphere((0.1, 1.0, 0.0), 0.15, light)
    built.box((-0.6, 0.0, -0.5), (-0.1, 0.6, 0.0), blue)
    out["sphere-light"] = (built.finish(), built, lambda counts, never: popcount(never) >= 10)

    # a transformed sphere light has two centres: it is met about center_world and SAMPLED about center_sample (sphereSample),
    # here below the floor: the shadow rays cross the floor, which therefore has to stay an occluder
    built = BuiltScene(48, 32, (0.0, 1.0, 5.5), (0, 1, 0), fov_degrees=30.0)
    grey, blue, light = lambertians(built)
    room(built, grey)
    built.sphere((0.1, 1.0, 0.0), 0.15, light)
    built.spheres[-1].center_sample[:] = (0.1, -0.5, 0.0)
    built.box((-0.6, 0.0, -0.5), (-0.1, 0.6, 0.0), blue)
    out["sphere-light-moved"] = (built.finish(), built, lambda counts, never: never & 0x3 == 0 and popcount(never) >= 8)
    return out


@pytest.fixture(scope="module")
def built_scenes():
    return scenes()


NAMES = ["cornell", "cornell-low-light", "open", "odd", "lone", "glass", "sphere-light", "sphere-light-moved"]


@pytest.mark.parametrize("name", NAMES)
def test_pruned_renders_are_the_bytes_of_the_full_pass_and_of_the_wavefront_path(built_scenes, name):
    from pathed_amd.integrator import HipScene
    desc, _, expected = built_scenes[name]
    gpu = HipScene(desc, device=0)
    assert gpu.stats()["path_kernel"] == 3, gpu.stats()["path_kernel"]    # the fused kernel
    _, counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
    print(name, counts, hex(never))
    assert expected(counts, never), (counts, hex(never))
    image = gpu.render(5, 0, 16, 0, 10)
    assert image.any()
    counting = HipScene(desc, device=0)
    counting.set_stats_mode(count=True)                                    # the counting instantiation: every turn for both rays
    assert np.array_equal(counting.render(5, 0, 16, 0, 10), image)
    per_slot = HipScene(desc, device=0, shade_kernel="per-slot")
    assert np.array_equal(per_slot.render(5, 0, 16, 0, 10), image)
    if name == "cornell":
        # another view: the order, the records and the camera masks are rebuilt
        camera = copy.copy(desc.contents.camera)
        camera.origin = (C.c_float * 3)(0.6, 1.4, 5.0)
        for scene in (gpu, counting, per_slot):
            scene.set_camera(camera)
        _, counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
        assert never == CORNELL_NEVER and counts["shadow_quad_pairs"] == 7, (counts, hex(never))
        moved = gpu.render(6, 0, 16, 0, 10)
        assert moved.any() and not np.array_equal(moved, image)
        assert np.array_equal(counting.render(6, 0, 16, 0, 10), moved)
        assert np.array_equal(per_slot.render(6, 0, 16, 0, 10), moved)


def light_rays(tris, emitters, never, rng, n_uniform):
    """Rays as sampleLightsTerm builds them: origin on a scene triangle, target on the front of an emitter triangle, float32
    direction normalised, tfar = distance - 1e-3.  Returns (rays (n, 10) float32, on_border (n,) bool)."""
    corners = np.stack([tris[:, 0:3], tris[:, 0:3] + tris[:, 4:7], tris[:, 0:3] + tris[:, 8:11]], axis=1).astype(np.float64)   # (T, 3, 3)
    prims = tris[:, 3].copy().view(np.int32)
    extent = float(np.linalg.norm(corners.reshape(-1, 3).max(axis=0) - corners.reshape(-1, 3).min(axis=0)))
    ulp = float(np.spacing(np.float32(extent)))

    def points(tri_index, a, b):
        c = corners[tri_index]
        return c[:, 0] + a[:, None] * (c[:, 1] - c[:, 0]) + b[:, None] * (c[:, 2] - c[:, 0])

    def barycentric(n, kind):
        a, b = rng.random(n), rng.random(n)
        flip = a + b > 1.0
        a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
        if kind == "edge":
            which = rng.integers(0, 3, n)
            b[which == 0] = 0.0
            a[which == 1] = 0.0
            b[which == 2] = 1.0 - a[which == 2]
        elif kind == "corner":
            which = rng.integers(0, 3, n)
            a, b = (which == 1).astype(np.float64), (which == 2).astype(np.float64)
        return a, b

    walls = np.array([k for k in range(len(tris)) if never >> int(prims[k]) & 1], dtype=np.int64)
    lights = np.array([k for k in range(len(tris)) if int(prims[k]) in emitters], dtype=np.int64)
    origins, border = [], []
    # anywhere on the scene
    index = rng.integers(0, len(tris), n_uniform)
    origins.append(points(index, *barycentric(n_uniform, "inside")))
    border.append(np.zeros(n_uniform, dtype=bool))
    # on the edges and corners of the never-occluders (the walls share them with their neighbours), displaced along the wall's
    # normal by 0, +-1, +-4, +-16 ulps of the scene's size
    for kind, count in (("edge", n_uniform // 4), ("corner", n_uniform // 8)):
        index = walls[rng.integers(0, len(walls), count)]
        on = points(index, *barycentric(count, kind))
        normal = np.cross(corners[index, 1] - corners[index, 0], corners[index, 2] - corners[index, 0])
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        steps = np.array([0.0, 1.0, -1.0, 4.0, -4.0, 16.0, -16.0])[rng.integers(0, 7, count)]
        origins.append(on + normal * (steps * ulp)[:, None])
        border.append(np.ones(count, dtype=bool))
    origins, border = np.concatenate(origins), np.concatenate(border)
    n = len(origins)
    # targets: a third inside the light, a third on its edges, a third on its corners
    target_kind = rng.integers(0, 3, n)
    index = lights[rng.integers(0, len(lights), n)]
    targets = np.empty((n, 3))
    for k, kind in enumerate(("inside", "edge", "corner")):
        chosen = target_kind == k
        targets[chosen] = points(index[chosen], *barycentric(int(chosen.sum()), kind))
    light_normal = np.cross(corners[index, 1] - corners[index, 0], corners[index, 2] - corners[index, 0])
    origins32, targets32 = origins.astype(np.float32), targets.astype(np.float32)
    delta = targets32 - origins32
    distance = np.sqrt((delta * delta).sum(axis=1, dtype=np.float32), dtype=np.float32)
    keep = (distance > np.float32(2e-3)) & ((light_normal * delta).sum(axis=1) < 0.0)    # the light's front
    direction = (delta / np.maximum(distance, np.float32(1e-30))[:, None]).astype(np.float32)
    rays = np.concatenate([origins32, direction, direction, (distance - np.float32(1e-3))[:, None]], axis=1).astype(np.float32)
    return rays[keep], border[keep]


def test_everything_phase_two_accepts_is_a_pruned_candidate(built_scenes):
    from pathed_amd.integrator import HipScene
    desc, _, _ = built_scenes["cornell"]
    gpu = HipScene(desc, device=0)
    _, tris = gpu.export_bvh()
    _, counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
    assert never == CORNELL_NEVER
    rays, border = light_rays(tris, {34, 35}, never, np.random.default_rng(11), 40000)
    out, _, _ = gpu.shadow_candidates(rays)
    candidates, accepted = out[:, 0], out[:, 1]
    occluded = float(np.count_nonzero(accepted)) / len(rays)
    print("rays %d occluded %.3f on a never-occluder's border %.3f" % (len(rays), occluded, border.mean()))
    assert len(rays) > 30000
    assert occluded >= 0.2                     # the check is not vacuous: a fifth of the rays meet something
    assert border.mean() >= 0.1                # ... and a tenth leave the border of a never-occluder
    assert not (candidates & np.uint64(never)).any()        # the pruned turns contribute no candidate
    lost = accepted & ~candidates
    assert not lost.any(), (int(np.count_nonzero(lost)), hex(int(lost[np.flatnonzero(lost)[0]])))
    # the full pass sees the same rays: what it keeps beyond the pruned word are never-occluders only
    full = gpu.small_candidates(rays)[:, 7]
    assert not ((full ^ candidates) & ~np.uint64(never)).any()


def test_origins_on_and_inside_glass_lose_no_hit_to_the_pruning(built_scenes):
    """The Lambertian + glass + mirror room: paths run inside the glass box, so shadow rays leave its faces from either side.
    The hook prunes whatever instantiation the scene renders with."""
    from pathed_amd.integrator import HipScene
    desc, _, _ = built_scenes["glass"]
    gpu = HipScene(desc, device=0)
    _, tris = gpu.export_bvh()
    _, counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
    assert popcount(never) >= 10 and counts["shadow_quad_pairs"] < (counts["quads"] + 1) // 2, (counts, hex(never))
    rays, _ = light_rays(tris, {10, 11}, never, np.random.default_rng(12), 20000)
    # (half of the scene's 24 triangles are the glass box's faces, primitives 12 .. 23: half of the uniform origins lie on them)
    out, _, _ = gpu.shadow_candidates(rays)
    candidates, accepted = out[:, 0], out[:, 1]
    print("rays %d occluded %.3f" % (len(rays), float(np.count_nonzero(accepted)) / len(rays)))
    assert len(rays) > 15000 and accepted.any()
    assert not (candidates & np.uint64(never)).any()
    lost = accepted & ~candidates
    assert not lost.any(), (int(np.count_nonzero(lost)), hex(int(lost[np.flatnonzero(lost)[0]])))


def test_cornell_reports_the_layout_of_the_host_rule(built_scenes):
    from pathed_amd.integrator import HipScene
    desc, _, _ = built_scenes["cornell"]
    gpu = HipScene(desc, device=0)
    _, counts, never = gpu.shadow_candidates(np.zeros((0, 10), dtype=np.float32))
    assert counts == {"quads": 17, "lone": 2, "shadow_quad_pairs": 7, "shadow_lone_pairs": 0}, counts
    assert never == CORNELL_NEVER, hex(never)
    # the never-occluders are the tail of both sections of the item order
    order = gpu.item_order(36)
    flags = [never >> int(p) & 1 for p in order]
    assert flags[:28] == [0] * 28 and flags[28:] == [1] * 8, flags
