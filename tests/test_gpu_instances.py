"""Instanced geometry (include/pathed_hip.h: PathedInstanceDesc): the two-level tree, k_trace_instanced
and k_shade_instanced against the FLATTENED form of the same scene (pathed_amd.flatten_instances), which the unchanged
kernels render.

1. exact class   placements by the identity and uniform power-of-two scales: every quantity of the intersector is an exact
                 power-of-two multiple of the flattened scene's, so hits and images are equal bit for bit
2. general class rotation, non-uniform scale, translation, mirror, a placement 1 000 units away: the primitive of a float64
                 brute force on every ray that is not a knife-edge case, t within 4 x the flattened form's own deviation
3. image         against the CPU oracle's render of the flattened scene at the project's contract
4. memory        4 096 placements store one tree of the prototype
5. refusals      by code and by name, nothing launched
"""
import ctypes as C

import numpy as np
import pytest

from pathed_amd import _capi, flatten_instances
from pathed_amd.instances import flatten_points
from pathed_amd.integrator import HipScene, PathedError

import instances_scene as S

pytestmark = pytest.mark.gpu

EXACT_SIZE = (48, 32)
IMAGE_SIZE = (64, 48)


class Pair:
    """An instanced scene and its flattened form on the GPU, with what both were made from."""

    def __init__(self, placements, size):
        self.built, self.pointer, self.prototypes, self.placements = S.build(placements, *size)
        self.flat = flatten_instances(self.pointer, self.prototypes, self.placements)
        self.instanced_gpu = HipScene(self.pointer, device=0, prototypes=self.prototypes, instances=self.placements)
        self.flat_gpu = HipScene(self.flat.desc, device=0)


@pytest.fixture(scope="module")
def exact():
    return Pair(S.EXACT_PLACEMENTS, EXACT_SIZE)


@pytest.fixture(scope="module")
def general():
    return Pair(S.GENERAL_PLACEMENTS, IMAGE_SIZE)


def bits(array):
    return np.ascontiguousarray(array).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- 1. exact class

def test_exact_class_hits_are_the_flattened_scenes_bits(exact):
    rays, shadow = S.exact_rays(exact.flat, 20000, seed=11)
    instanced, flat = exact.instanced_gpu.trace(rays), exact.flat_gpu.trace(rays)
    assert (bits(instanced[:, 3]).view(np.int32) >= 0).mean() > 0.5          # the rays do hit things
    hit_instance = bits(instanced[:, 3]).view(np.int32) >= int(exact.flat.bases[0])
    assert hit_instance.mean() > 0.2                                         # ... placements among them
    assert np.array_equal(bits(instanced), bits(flat))
    occluded, expected = exact.instanced_gpu.trace(shadow, any_hit=True), exact.flat_gpu.trace(shadow, any_hit=True)
    assert 0.05 < expected.mean() < 0.95
    assert np.array_equal(occluded, expected)


@pytest.mark.parametrize("last_bounce", [0, 1, 2, 3])
def test_exact_class_render_is_the_flattened_scenes_bits(exact, last_bounce):
    sums, squares = exact.instanced_gpu.render_moments(5, 0, 4, 0, last_bounce)
    flat_sums, flat_squares = exact.flat_gpu.render_moments(5, 0, 4, 0, last_bounce)
    assert last_bounce == 0 or float(flat_sums.sum()) > 0.0   # (bounce 0 alone is the emitter seen directly: it is out of view)
    assert np.array_equal(bits(sums), bits(flat_sums))
    assert np.array_equal(bits(squares), bits(flat_squares))
    assert exact.instanced_gpu.stats()["path_kernel"] == 10


@pytest.mark.parametrize("listed", [1, 65, EXACT_SIZE[0] * EXACT_SIZE[1]])
def test_exact_class_list_pass(exact, listed):
    width, height = EXACT_SIZE
    pixels = width * height
    full_sums, full_squares = exact.flat_gpu.render_moments(5, 0, 4, 0, 3)
    chosen = np.sort(np.random.default_rng(listed).choice(pixels, listed, replace=False)).astype(np.uint32)
    gpu = exact.instanced_gpu
    pattern = np.full(3 * pixels, 0.375, dtype=np.float32)
    buffers = [gpu.device_buffer(3 * pixels, pattern), gpu.device_buffer(3 * pixels, pattern),
               gpu.device_words(pixels, np.full(pixels, 7, dtype=np.uint32)), gpu.device_words(listed, chosen)]
    try:
        # the listed pixels start from zero sums, the others keep the pattern
        start = pattern.reshape(pixels, 3).copy()
        start[chosen] = 0.0
        for pointer in buffers[:2]:
            gpu._lib.pathed_hip_accum_upload(gpu._handle, C.c_void_p(pointer), 3 * pixels, start.ctypes.data_as(C.POINTER(C.c_float)))
        gpu.render_pixels(5, 0, 4, 0, 3, buffers[3], listed, buffers[0], buffers[1], buffers[2])
        sums = gpu.download_device_buffer(buffers[0], np.zeros((pixels, 3), dtype=np.float32))
        squares = gpu.download_device_buffer(buffers[1], np.zeros((pixels, 3), dtype=np.float32))
        counts = gpu.download_device_words(buffers[2], np.zeros(pixels, dtype=np.uint32))
    finally:
        for pointer in buffers:
            gpu.free_device_buffer(pointer)
    others = np.ones(pixels, dtype=bool)
    others[chosen] = False
    assert np.array_equal(bits(sums[chosen]), bits(full_sums.reshape(pixels, 3)[chosen]))
    assert np.array_equal(bits(squares[chosen]), bits(full_squares.reshape(pixels, 3)[chosen]))
    assert np.all(sums[others] == np.float32(0.375)) and np.all(squares[others] == np.float32(0.375))
    assert np.all(counts[chosen] == 11) and np.all(counts[others] == 7)


def instanced_stack_rungs(depth):
    """The LDS row counts that hold a two-level stack without a spill, for bvh_max_depth = the top tree's levels + the deepest
    prototype's: the bound is (3 top + 1) + (3 deepest + 1) + 1 entries; the default is the first of 8, 16, 22 that holds it"""
    bound = 3 * depth + 3
    default = 8 if bound <= 8 else 16 if bound <= 16 else 22
    return [rows for rows in (8, 16, 22) if rows >= default]


@pytest.mark.parametrize("count", [False, True], ids=["plain", "counting"])
def test_every_stack_row_count_renders_the_same_bits(count):
    """k_trace_instanced<8 | 16 | 22, COUNT> in a render: the row count the scene takes by default and every larger one"""
    _, pointer, prototypes, placements = S.build(S.EXACT_PLACEMENTS, 16, 12)

    def render(rows):
        gpu = HipScene(pointer, device=0, prototypes=prototypes, instances=placements, stack_rows=rows)
        gpu.set_stats_mode(count=count)
        sums, squares = gpu.render_moments(5, 0, 4, 0, 3)
        stats = gpu.stats()
        assert stats["path_kernel"] == 10 and (stats["nodes_visited"] > 0 or not count)
        return sums, squares, stats["bvh_max_depth"], stats["nodes_visited"]

    sums, squares, depth, visited = render(0)
    assert float(sums.sum()) > 0.0
    rungs = instanced_stack_rungs(depth)
    assert rungs   # (22 always is one)
    for rows in rungs:
        again = render(rows)
        assert np.array_equal(bits(again[0]), bits(sums)) and np.array_equal(bits(again[1]), bits(squares)), rows
        assert again[3] == visited, rows


# -------------------------------------------------------------------------------------------------------- 2. general class

GENERAL_SEED = 3
GENERAL_RAYS = 6000


@pytest.fixture(scope="module")
def general_reference(general):
    rays = S.general_rays(general.flat, GENERAL_RAYS, GENERAL_SEED)
    nearest, prim, margin, second = S.brute_force(S.triangles_of(general.flat), rays)
    return rays, nearest, prim, S.keep_mask(nearest, prim, margin, second)


def test_general_class_hits(general, general_reference):
    """The bound on |t - t64| / t64 is 4 x the flattened form's own largest deviation on the same rays (unchanged code): evaluation
    in object space adds the roundings of the inverse transform applied to origin and direction to the intersector's own, and
    both forms cancel alike in o - v0.  Measured on MI355X: 5 592 of 6 000 rays kept; flattened max 2.449e-05 (mean 8.0e-08),
    instanced max 6.251e-05 (mean 1.7e-07): a factor 2.6."""
    import oracle_lib
    rays, nearest, prim, keep = general_reference
    assert keep.mean() >= 0.9, keep.mean()
    # the oracle's intersector (bit-identical to the GPU's) names the float64 primitive on every kept ray of the flattened scene
    oracle = oracle_lib.OracleScene(general.flat.desc).trace(rays)
    assert np.array_equal(bits(oracle[:, 3]).view(np.int32)[keep], prim[keep])
    # every placement is hit by kept rays
    for k in range(len(general.placements)):
        assert ((prim[keep] >= general.flat.bases[k]) & (prim[keep] < general.flat.bases[k + 1])).sum() > 50, k

    flat = general.flat_gpu.trace(rays)
    instanced = general.instanced_gpu.trace(rays)
    flat_deviation = np.abs(flat[keep, 0].astype(np.float64) - nearest[keep]) / nearest[keep]
    deviation = np.abs(instanced[keep, 0].astype(np.float64) - nearest[keep]) / nearest[keep]
    print("general class: %d of %d rays kept; |t - t64| / t64: flattened max %.3e mean %.3e, instanced max %.3e mean %.3e"
          % (keep.sum(), len(keep), flat_deviation.max(), flat_deviation.mean(), deviation.max(), deviation.mean()))
    assert np.array_equal(bits(flat[:, 3]).view(np.int32)[keep], prim[keep])
    assert np.array_equal(bits(instanced[:, 3]).view(np.int32)[keep], prim[keep])
    assert deviation.max() <= 4.0 * flat_deviation.max()

    # occlusion: a segment that ends at half the nearest hit is free, one that reaches twice as far is blocked
    shadow = rays[keep].copy()
    blocked = np.arange(len(shadow)) % 2 == 1
    shadow[:, 7] = (nearest[keep] * np.where(blocked, 2.0, 0.5)).astype(np.float32)
    assert np.array_equal(general.instanced_gpu.trace(shadow, any_hit=True), blocked.astype(np.int32))
    assert np.array_equal(general.flat_gpu.trace(shadow, any_hit=True), blocked.astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- 3. image

def test_general_class_image_against_the_oracle(general):
    """64 x 48 x 8 spp, bounces 0..4, against the oracle's render of the FLATTENED scene: relL2 <= 2e-3 (the project's contract)
    and at most 1 % of the pixels off by more than 1 % (a cap).  Every placement covers at least 5 % of the pixels, so a wrong
    transform or normal cannot hide under the cap."""
    import oracle_lib
    width, height = IMAGE_SIZE
    oracle = oracle_lib.OracleScene(general.flat.desc)
    camera = general.built.desc.camera
    first = bits(oracle.trace(S.camera_rays(width, height, tuple(camera.origin), tuple(camera.target)))[:, 3]).view(np.int32)
    for k in range(len(general.placements)):
        share = ((first >= general.flat.bases[k]) & (first < general.flat.bases[k + 1])).mean()
        assert share >= 0.05, (k, share)
    expected, _ = oracle.render(width, height, 9, 0, 8, 0, 4, threads=16)
    image = general.instanced_gpu.render(9, 0, 8, 0, 4)
    rel = float(np.linalg.norm(image - expected) / np.linalg.norm(expected))
    scale = np.maximum(np.abs(expected).max(axis=2), 1e-3 * float(np.abs(expected).max()))
    off = (np.abs(image - expected).max(axis=2) > 0.01 * scale).mean()
    print("general class image: relL2 %.3e, pixels off by more than 1 %%: %.4f" % (rel, off))
    assert rel <= 2e-3
    assert off <= 0.01


# --------------------------------------------------------------------------------------------------------------- 4. memory

def top_tree_nodes(nodes):
    """nodes reachable from the root without entering an instance: the top tree"""
    refs = nodes[:, 24:28].view(np.int32)
    seen, work = 0, [0]
    while work:
        node = work.pop()
        seen += 1
        work += [int(r) for r in refs[node] if r >= 0]
    return seen


def test_many_placements_store_one_tree():
    count = 4096
    placements = []
    for k in range(count):
        row, col = divmod(k, 64)
        placements.append((S.P, S.affine(S.rotation((0.1, 1.0, 0.2), 7.0 * k) * 0.12, (-9.0 + 0.28 * col, 0.3, -9.0 + 0.28 * row))))
    built, pointer, prototypes, placements = S.build(placements, 32, 24)
    gpu = HipScene(pointer, device=0, prototypes=prototypes, instances=placements)
    nodes, tris = gpu.export_bvh()
    world = int(built.desc.geoms[prototypes[0][0]].first)
    stored = int(built.desc.n_triangles)
    assert len(tris) == stored                                  # world + ONE copy of P (+ the unused Q), not 4 096 copies
    one = HipScene(pointer, device=0, prototypes=prototypes, instances=placements[:1])
    one_nodes, _ = one.export_bvh()
    prototype_nodes = len(one_nodes) - top_tree_nodes(one_nodes)
    assert len(nodes) - top_tree_nodes(nodes) == prototype_nodes   # the prototypes' trees are there once, whatever the placements
    assert top_tree_nodes(nodes) <= world + count
    image = gpu.render(1, 0, 2, 0, 3)
    assert np.isfinite(image).all() and float(image.sum()) > 0.0
    # a ray down onto a placement reports a virtual id inside that placement's range
    flat_first = world + 320 * 2080
    centre = flatten_points(placements[2080][1], np.array([[3.0, 2.0, 1.0]], dtype=np.float32))[0]
    ray = np.array([[centre[0], 8.0, centre[2], 1e-3, 0.0, -1.0, 0.0, 1e5]], dtype=np.float32)
    hit = gpu.trace(ray)
    assert flat_first <= int(bits(hit[:, 3]).view(np.int32)[0]) < flat_first + 320


# ------------------------------------------------------------------------------------------------------------- 5. refusals

UNSUPPORTED, INVALID = -4, -1


def create_error(pointer, prototypes, placements, **options):
    with pytest.raises(PathedError) as caught:
        HipScene(pointer, device=0, prototypes=None if hasattr(placements, "desc") else prototypes, instances=placements, **options)
    return str(caught.value)


def test_creation_refusals_name_their_reason():
    one = [(S.P, S.affine())]
    built, pointer, prototypes, _ = S.build(one, 16, 16)
    assert "(%d)" % UNSUPPORTED in create_error(pointer, prototypes, one, refittable=1) and "refittable" in create_error(pointer, prototypes, one, refittable=1)
    for builder in ("lbvh", "ploc"):
        message = create_error(pointer, prototypes, one, bvh_builder=builder)
        assert "(%d)" % UNSUPPORTED in message and "device builders" in message
    message = create_error(pointer, prototypes, one, shade_kernel="wave")
    assert "(%d)" % UNSUPPORTED in message and "shade_kernel" in message
    # the virtual ids: 2^31 / 320 placements are one too many
    message = create_error(pointer, prototypes, many_copies(prototypes, one[0], 2 ** 31 // 320 + 1))
    assert "(%d)" % INVALID in message and "2^31" in message
    message = create_error(pointer, prototypes, [(S.P, np.zeros(12, dtype=np.float32))])
    assert "(%d)" % INVALID in message and "invertible" in message

    # spheres, media, containers, an emitter in a prototype
    scene = S.BuiltScene(16, 16, origin=(0, 2, 8), target=(0, 1, 0))
    grey = scene.material()
    scene.medium((0.5, 0.5, 0.5))
    scene.quad([(-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)], grey)
    scene.box((1, 1, 1), (2, 2, 2), grey)
    message = create_error(scene.finish(), [(1, 1)], [(0, S.affine())])
    assert "(%d)" % UNSUPPORTED in message and "media" in message

    scene = S.BuiltScene(16, 16, origin=(0, 2, 8), target=(0, 1, 0))
    grey = scene.material()
    scene.sphere((0, 1, 0), 0.5, grey)
    scene.box((1, 1, 1), (2, 2, 2), grey)
    message = create_error(scene.finish(), [(1, 1)], [(0, S.affine())])
    assert "(%d)" % UNSUPPORTED in message and "sphere" in message

    scene = S.BuiltScene(16, 16, origin=(0, 2, 8), target=(0, 1, 0))
    shell = scene.material(_capi.MAT_PASSTHROUGH)
    scene.box((1, 1, 1), (2, 2, 2), shell)
    message = create_error(scene.finish(), [(0, 1)], [(0, S.affine())])
    assert "(%d)" % UNSUPPORTED in message and "containers" in message

    scene = S.BuiltScene(16, 16, origin=(0, 2, 8), target=(0, 1, 0))
    glow = scene.material(emit=(1, 1, 1))
    scene.box((1, 1, 1), (2, 2, 2), glow)
    message = create_error(scene.finish(), [(0, 1)], [(0, S.affine())])
    assert "(%d)" % UNSUPPORTED in message and "emissive" in message


def many_copies(prototypes, placement, count):
    """an InstanceSet of `count` copies of one placement, without a Python object per copy"""
    from pathed_amd.instances import InstanceSet
    instance_set = InstanceSet(prototypes, [placement])
    record = np.frombuffer(bytes(instance_set._instance_array), dtype=np.uint8)
    copies = np.ascontiguousarray(np.tile(record, count))
    instance_set._copies = copies
    instance_set.desc.n_instances = count
    instance_set.desc.instances = C.cast(copies.ctypes.data, C.POINTER(_capi.PathedInstance))
    return instance_set


def test_refusals_on_a_created_scene_launch_nothing(exact):
    gpu = exact.instanced_gpu
    gpu.reset_stats()

    def refused(call, word):
        with pytest.raises(PathedError) as caught:
            call()
        assert "(%d)" % UNSUPPORTED in str(caught.value) and word in str(caught.value), str(caught.value)

    positions = np.zeros((int(exact.built.desc.n_vertices), 3), dtype=np.float32)
    refused(lambda: gpu.refit(positions), "refit")
    refused(lambda: gpu.render_features(1, 0, 1), "feature")
    refused(lambda: gpu.small_candidates(np.zeros((1, 10), dtype=np.float32)), "instances")
    refused(lambda: gpu.light_records(int(exact.built.desc.n_triangles), 8), "instances")
    try:
        for name in ("VolumePathTracer", "BasicVolumeIntegrator", "AlbedoIntegrator"):
            gpu.set_integrator(name)
            refused(lambda: gpu.render(1, 0, 1, 0, 2), "integrator")
    finally:
        gpu.set_integrator("PathTracer")
    stats = gpu.stats()
    assert stats["trace_launches_all"] == 0 and stats["camera_samples"] == 0 and stats["iterations"] == 0
