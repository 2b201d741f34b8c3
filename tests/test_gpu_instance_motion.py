"""Moving placements (include/pathed_hip.h: pathed_hip_scene_set_instance_transforms[_device]; DESIGN.md section 4.6d;
instance_kernels.h: k_instance_records, k_refit_top_pass).  The yardstick throughout is a scene CREATED with the same placements: a
moved scene answers with its bits.

1. moved equals fresh   traces (closest and any hit), moments at bounces 0..3, and back again without residue
2. exact class          moved onto the exact placements: the flattened scene's bits
3. tree                 one instance leaf per placement with the fresh scene's box, inner boxes contain their nodes, prototypes
                        and leaf triangles untouched
4. depth                4 096 placements shuffled over a grid: a top tree of several levels, every box jumps
5. device entry         a torch tensor on the device
6. lists                render_pixels after a move
7. refusals             by code and by name; the scene stays as it was
"""
import ctypes as C

import numpy as np
import pytest

from pathed_amd import _capi, flatten_instances
from pathed_amd import instances as I
from pathed_amd.integrator import HipScene, PathedError, _check

import instances_scene as S

pytestmark = pytest.mark.gpu

SIZE = (48, 32)
UNSUPPORTED, INVALID = -4, -1
INSTANCE_BIT = 1 << 30
EMPTY = -(1 << 31)


def bits(array):
    return np.ascontiguousarray(array).view(np.uint32)


def linear_of(transform):
    return np.asarray(transform, dtype=np.float64).reshape(3, 4)[:, :3]


def moved_placements():
    """M1: every transform composed with a rotation and a translation of its own, except: the placement 1 000 units away comes
    close, a near one goes far, one determinant changes its sign, one transform stays."""
    g = S.GENERAL_PLACEMENTS
    return [
        (S.P, S.placed(S.rotation((0.3, 1.0, 0.1), 52.0) @ linear_of(g[0][1]), (-2.9, 2.4, 3.2), S.P_CENTRE)),
        (S.P, S.placed(np.diag([-1.0, 1.0, 1.0]) @ S.rotation((1.0, 0.2, 0.4), 33.0) @ linear_of(g[1][1]), (-5.2, 2.2, -1.0), S.P_CENTRE)),   # det < 0 now
        (S.Q, g[2][1].copy()),                                                                                                              # untouched
        (S.P, S.placed(90.0 * S.rotation((0.1, 0.3, 1.0), 64.0) @ linear_of(g[3][1]), (150.0, 260.0, -930.0), S.P_CENTRE)),                  # near -> far
        (S.P, S.placed(0.01 * S.rotation((1.0, 0.1, 0.7), 115.0) @ linear_of(g[4][1]), (4.4, 3.3, 1.5), S.P_CENTRE)),                        # far -> near
    ]


def transforms_of(placements):
    return np.stack([np.asarray(t, dtype=np.float32).reshape(12) for _, t in placements])


class Scene:
    """An instanced scene on the GPU with what it was made from."""

    def __init__(self, placements, size=SIZE):
        self.built, self.pointer, self.prototypes, self.placements = S.build(placements, *size)
        self.gpu = HipScene(self.pointer, device=0, prototypes=self.prototypes, instances=self.placements)

    def flat(self):
        return flatten_instances(self.pointer, None, self.gpu.instance_set)


def query_rays(flat, seed):
    """6 000 closest-hit rays onto the flattened triangles plus the 64 x 48 camera rays, and 6 000 any-hit segments that end at
    half or at twice the target's distance"""
    closest = np.concatenate([S.general_rays(flat, 6000, seed), S.camera_rays(64, 48, S.CAMERA["origin"], S.CAMERA["target"])])
    shadow = S.general_rays(flat, 6000, seed + 1)
    shadow[:, 7] = np.where(np.arange(len(shadow)) % 2 == 1, 2.0, 0.5).astype(np.float32)
    return closest, shadow


def assert_same_answers(moved, fresh, closest, shadow):
    a, b = moved.trace(closest), fresh.trace(closest)
    assert (bits(b[:, 3]).view(np.int32) >= 0).mean() > 0.5
    assert np.array_equal(bits(a), bits(b))
    occluded, expected = moved.trace(shadow, any_hit=True), fresh.trace(shadow, any_hit=True)
    assert 0.05 < expected.mean() < 0.95
    assert np.array_equal(occluded, expected)


def assert_same_moments(moved, fresh):
    for last_bounce in (0, 1, 2, 3):
        sums, squares = moved.render_moments(5, 0, 4, 0, last_bounce)
        fresh_sums, fresh_squares = fresh.render_moments(5, 0, 4, 0, last_bounce)
        assert last_bounce == 0 or float(fresh_sums.sum()) > 0.0
        assert np.array_equal(bits(sums), bits(fresh_sums)), last_bounce
        assert np.array_equal(bits(squares), bits(fresh_squares)), last_bounce


@pytest.fixture(scope="module")
def fresh_moved():
    """scene B: created with M1, never moved"""
    return Scene(moved_placements())


@pytest.fixture(scope="module")
def fresh_general():
    return Scene(S.GENERAL_PLACEMENTS)


@pytest.fixture(scope="module")
def moved():
    """scene A: created with the general placements, moved to M1 through the host entry; with its tree before the move"""
    scene = Scene(S.GENERAL_PLACEMENTS)
    scene.before = scene.gpu.export_bvh()
    scene.ms = scene.gpu.set_instance_transforms(transforms_of(moved_placements()))
    return scene


# --------------------------------------------------------------------------------------------------- 1. moved equals fresh

def test_moved_equals_fresh_and_back(fresh_moved, fresh_general):
    scene = Scene(S.GENERAL_PLACEMENTS)
    ms = scene.gpu.set_instance_transforms(transforms_of(moved_placements()).reshape(-1, 3, 4))
    assert ms > 0.0
    flat = scene.flat()   # the set followed the move: this is M1 flattened
    assert np.array_equal(bits(flat.positions), bits(fresh_moved.flat().positions))
    closest, shadow = query_rays(flat, seed=17)
    # every placement of M1 is hit
    prim = bits(fresh_moved.gpu.trace(closest)[:, 3]).view(np.int32)
    for k in range(len(scene.placements)):
        assert ((prim >= flat.bases[k]) & (prim < flat.bases[k + 1])).sum() > 50, k
    assert_same_answers(scene.gpu, fresh_moved.gpu, closest, shadow)
    assert_same_moments(scene.gpu, fresh_moved.gpu)
    assert scene.gpu.stats()["path_kernel"] == 10
    # and back: no residue of M1
    scene.gpu.set_instance_transforms(transforms_of(S.GENERAL_PLACEMENTS))
    closest, shadow = query_rays(fresh_general.flat(), seed=23)
    assert_same_answers(scene.gpu, fresh_general.gpu, closest, shadow)
    assert_same_moments(scene.gpu, fresh_general.gpu)
    for mine, theirs in zip(scene.gpu.instance_records(), fresh_general.gpu.instance_records()):
        assert np.array_equal(bits(mine), bits(theirs))


# ------------------------------------------------------------------------------------------------------------ 2. exact class

def test_moved_onto_the_exact_class_is_the_flattened_scenes_bits():
    # (six placements there, five here: the general set with one more, then moved)
    start = list(S.GENERAL_PLACEMENTS) + [(S.Q, S.placed(1.5 * S.rotation((0.0, 1.0, 0.3), 12.0), (3.0, 0.9, 5.0), S.Q_CENTRE))]
    start = [(exact[0], general[1]) for exact, general in zip(S.EXACT_PLACEMENTS, start)]   # the prototypes of the exact set
    scene = Scene(start)
    scene.gpu.set_instance_transforms(transforms_of(S.EXACT_PLACEMENTS))
    flat = flatten_instances(scene.pointer, scene.prototypes, S.EXACT_PLACEMENTS)
    flat_gpu = HipScene(flat.desc, device=0)
    rays, shadow = S.exact_rays(flat, 6000, seed=11)
    instanced, expected = scene.gpu.trace(rays), flat_gpu.trace(rays)
    assert (bits(expected[:, 3]).view(np.int32) >= int(flat.bases[0])).mean() > 0.2
    assert np.array_equal(bits(instanced), bits(expected))
    assert np.array_equal(scene.gpu.trace(shadow, any_hit=True), flat_gpu.trace(shadow, any_hit=True))
    sums, squares = scene.gpu.render_moments(5, 0, 4, 0, 3)
    flat_sums, flat_squares = flat_gpu.render_moments(5, 0, 4, 0, 3)
    assert float(flat_sums.sum()) > 0.0
    assert np.array_equal(bits(sums), bits(flat_sums)) and np.array_equal(bits(squares), bits(flat_squares))


# ------------------------------------------------------------------------------------------------------------------ 3. tree

def top_tree(nodes):
    """(nodes of the top tree in visiting order, {placement: [(node, slot), ...]}), walking from node 0 without entering an instance"""
    refs = nodes[:, 24:28].view(np.int32)
    seen, leaves, work = [], {}, [0]
    while work:
        node = work.pop()
        seen.append(node)
        for slot in range(4):
            ref = int(refs[node, slot])
            if ref >= 0:
                work.append(ref)
            elif ref != EMPTY and ((-ref - 1) & INSTANCE_BIT):
                leaves.setdefault((-ref - 1) & (INSTANCE_BIT - 1), []).append((node, slot))
    return seen, leaves


def child_box(nodes, node, slot):
    return nodes[node, 0:12].reshape(3, 4)[:, slot].copy(), nodes[node, 12:24].reshape(3, 4)[:, slot].copy()


def test_the_refitted_top_tree(moved, fresh_moved):
    nodes, tris = moved.gpu.export_bvh()
    before_nodes, before_tris = moved.before
    fresh_nodes, _ = fresh_moved.gpu.export_bvh()
    seen, leaves = top_tree(nodes)
    _, fresh_leaves = top_tree(fresh_nodes)
    top = len(seen)
    assert sorted(seen) == list(range(top))   # the top tree is the head of the node array
    assert sorted(top_tree(before_nodes)[0]) == list(range(top))
    desc = moved.built.desc
    for k, (prototype, transform) in enumerate(moved_placements()):
        assert len(leaves.get(k, [])) == 1 and len(fresh_leaves.get(k, [])) == 1, k
        lo, hi = child_box(nodes, *leaves[k][0])
        fresh_lo, fresh_hi = child_box(fresh_nodes, *fresh_leaves[k][0])
        assert np.array_equal(bits(lo), bits(fresh_lo)) and np.array_equal(bits(hi), bits(fresh_hi)), k
        # ... which is the numpy statement of the rule (pathed_amd.instances)
        geom = desc.geoms[moved.prototypes[prototype][0]]
        corners = np.ctypeslib.as_array(desc.indices, shape=(int(desc.n_triangles), 3))[geom.first:geom.first + geom.count].reshape(-1)
        positions = np.ctypeslib.as_array(desc.positions, shape=(int(desc.n_vertices), 3))[corners]
        rule_lo, rule_hi = I.pad_box(*I.placement_box(transform, *I.prototype_box(positions)))
        assert np.array_equal(bits(lo), bits(rule_lo)) and np.array_equal(bits(hi), bits(rule_hi)), k
    refs = nodes[:, 24:28].view(np.int32)
    inner = 0
    for node in seen:
        for slot in range(4):
            ref = int(refs[node, slot])
            if ref < 0:
                continue
            inner += 1
            lo, hi = child_box(nodes, node, slot)
            for below in range(4):
                if int(refs[ref, below]) == EMPTY:
                    continue
                below_lo, below_hi = child_box(nodes, ref, below)
                assert np.all(lo <= below_lo) and np.all(hi >= below_hi), (node, slot, below)
    assert inner >= 1
    # something did move up there, and nothing below
    assert not np.array_equal(bits(nodes[:top]), bits(before_nodes[:top]))
    assert np.array_equal(bits(nodes[:top, 24:32]), bits(before_nodes[:top, 24:32]))   # the topology
    assert len(nodes) > top and np.array_equal(bits(nodes[top:]), bits(before_nodes[top:]))
    assert np.array_equal(bits(tris), bits(before_tris))


# ----------------------------------------------------------------------------------------------------------------- 4. depth

def test_a_shuffled_grid_of_4096_placements():
    count, side = 4096, 64
    rng = np.random.default_rng(2024)
    spots = [(-11.8 + 0.375 * (k % side), 0.35 + 0.5 * ((k * 7) % 5), -11.8 + 0.375 * (k // side)) for k in range(count)]
    linears = [0.22 * S.rotation((0.2, 1.0, 0.1 + 0.001 * k), 11.0 * k) for k in range(count)]
    order = rng.permutation(count)
    start = [(S.Q, S.placed(linears[k], spots[k], S.Q_CENTRE)) for k in range(count)]
    shuffled = [(S.Q, S.placed(linears[k], spots[int(order[k])], S.Q_CENTRE)) for k in range(count)]
    scene = Scene(start, (32, 24))
    fresh = Scene(shuffled, (32, 24))
    assert scene.gpu.stats()["bvh_max_depth"] >= 4
    ids_before = scene.gpu.instance_records()[2]
    scene.gpu.set_instance_transforms(transforms_of(shuffled))
    rays = S.camera_rays(64, 48, S.CAMERA["origin"], S.CAMERA["target"])
    mine, theirs = scene.gpu.trace(rays), fresh.gpu.trace(rays)
    prim = bits(theirs[:, 3]).view(np.int32)
    assert len(np.unique((prim[prim >= 4] - 4) // 12)) > 100   # many placements are seen (world: 4 triangles; Q: 12 each)
    assert np.array_equal(bits(mine), bits(theirs))
    transforms, inverses, ids = scene.gpu.instance_records()
    expected = np.stack([I.instance_inverse(t) for _, t in shuffled])
    assert np.array_equal(bits(transforms), bits(transforms_of(shuffled)))
    assert np.array_equal(bits(inverses), bits(expected))
    fresh_records = fresh.gpu.instance_records()
    assert np.array_equal(bits(inverses), bits(fresh_records[1]))
    # quad 6 is the scene's own from before the move; the fresh scene's differs only in where its (other) top tree ends
    assert np.array_equal(ids, ids_before) and np.array_equal(ids[:, [0, 1, 3]], fresh_records[2][:, [0, 1, 3]])


# ---------------------------------------------------------------------------------------------------------- 5. device entry

def test_the_device_entry_takes_a_tensor(moved, fresh_moved):
    import torch
    scene = Scene(S.GENERAL_PLACEMENTS)
    tensor = torch.from_numpy(transforms_of(moved_placements())).to("cuda:0")
    torch.cuda.synchronize()
    ms = scene.gpu.set_instance_transforms(tensor)
    assert ms > 0.0
    for mine, theirs in zip(scene.gpu.instance_records(), moved.gpu.instance_records()):
        assert np.array_equal(bits(mine), bits(theirs))
    closest, shadow = query_rays(fresh_moved.flat(), seed=29)
    assert_same_answers(scene.gpu, fresh_moved.gpu, closest, shadow)
    with pytest.raises(ValueError):
        scene.gpu.set_instance_transforms(tensor.cpu())
    with pytest.raises(ValueError):
        scene.gpu.set_instance_transforms(tensor.double())


# ----------------------------------------------------------------------------------------------------------------- 6. lists

def test_a_list_pass_after_a_move(moved, fresh_moved):
    width, height = SIZE
    pixels, listed = width * height, 65
    full_sums, full_squares = fresh_moved.gpu.render_moments(5, 0, 4, 0, 3)
    chosen = np.sort(np.random.default_rng(listed).choice(pixels, listed, replace=False)).astype(np.uint32)
    gpu = moved.gpu
    pattern = np.full(3 * pixels, 0.375, dtype=np.float32)
    buffers = [gpu.device_buffer(3 * pixels, pattern), gpu.device_buffer(3 * pixels, pattern),
               gpu.device_words(pixels, np.full(pixels, 7, dtype=np.uint32)), gpu.device_words(listed, chosen)]
    try:
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
    assert float(full_sums.reshape(pixels, 3)[chosen].sum()) > 0.0
    assert np.array_equal(bits(sums[chosen]), bits(full_sums.reshape(pixels, 3)[chosen]))
    assert np.array_equal(bits(squares[chosen]), bits(full_squares.reshape(pixels, 3)[chosen]))
    assert np.all(sums[others] == np.float32(0.375)) and np.all(squares[others] == np.float32(0.375))
    assert np.all(counts[chosen] == 11) and np.all(counts[others] == 7)


# -------------------------------------------------------------------------------------------------------------- 7. refusals

def refused(call, code, word):
    with pytest.raises(PathedError) as caught:
        call()
    assert "(%d)" % code in str(caught.value) and word in str(caught.value), str(caught.value)


def test_refusals_leave_the_scene_as_it_was(fresh_general):
    scene = Scene(S.GENERAL_PLACEMENTS)
    gpu = scene.gpu
    good = transforms_of(S.GENERAL_PLACEMENTS)
    closest, shadow = query_rays(fresh_general.flat(), seed=31)
    records_before = gpu.instance_records()
    hits_before, occluded_before = gpu.trace(closest), gpu.trace(shadow, any_hit=True)

    flat = flatten_instances(scene.pointer, scene.prototypes, scene.placements)
    plain = HipScene(flat.desc, device=0)
    refused(lambda: plain.set_instance_transforms(good), UNSUPPORTED, "no instances")
    refused(lambda: plain.instance_records(), UNSUPPORTED, "no instances")
    refused(lambda: gpu.set_instance_transforms(good[:4]), INVALID, "count")
    refused(lambda: gpu.set_instance_transforms(np.concatenate([good, good[:1]])), INVALID, "count")
    lib = gpu._lib
    refused(lambda: _check(lib, lib.pathed_hip_scene_set_instance_transforms(gpu._handle, None, len(good), None), "set"), INVALID, "null")
    refused(lambda: _check(lib, lib.pathed_hip_scene_set_instance_transforms_device(gpu._handle, None, len(good), None), "set"), INVALID, "null")
    refused(lambda: _check(lib, lib.pathed_hip_debug_instance_records(gpu._handle, None, len(good)), "records"), INVALID, "null")

    # a NaN in placement 3, a singular matrix (two equal rows) in placement 2: each is named; both: the lower index
    moved = transforms_of(moved_placements())
    nan = moved.copy()
    nan[3, 5] = np.nan
    refused(lambda: gpu.set_instance_transforms(nan), INVALID, "instance transform 3 ")
    singular = moved.copy()
    singular[2, 4:8] = singular[2, 0:4]
    refused(lambda: gpu.set_instance_transforms(singular), INVALID, "instance transform 2 ")
    both = nan.copy()
    both[2] = singular[2]
    refused(lambda: gpu.set_instance_transforms(both), INVALID, "instance transform 2 ")
    infinite = moved.copy()
    infinite[4, 11] = np.inf
    refused(lambda: gpu.set_instance_transforms(infinite), INVALID, "instance transform 4 ")

    for mine, theirs in zip(gpu.instance_records(), records_before):
        assert np.array_equal(bits(mine), bits(theirs))
    for mine, theirs in zip(gpu.instance_set.instances, S.GENERAL_PLACEMENTS):
        assert np.array_equal(bits(mine[1]), bits(theirs[1]))
    assert np.array_equal(bits(gpu.trace(closest)), bits(hits_before))
    assert np.array_equal(gpu.trace(shadow, any_hit=True), occluded_before)
    assert_same_answers(gpu, fresh_general.gpu, closest, shadow)
    # and the scene still moves afterwards
    gpu.set_instance_transforms(moved)
    assert np.array_equal(bits(gpu.instance_records()[0]), bits(moved))


def test_an_empty_world_and_no_placements_pass_through():
    """the empty-world root (one node, four empty children) under a move of nothing; a lone placement in an empty world"""
    built = S.BuiltScene(16, 16, origin=(0, 2, 8), target=(0, 1, 0))
    grey = built.material()
    built.box((1, 1, 1), (2, 2, 2), grey)
    pointer = built.finish()
    none = HipScene(pointer, device=0, prototypes=[(0, 1)], instances=[])
    none.set_instance_transforms(np.zeros((0, 12), dtype=np.float32))
    nodes, _ = none.export_bvh()
    assert np.all(nodes[0, 24:28].view(np.int32) == EMPTY)
    ray = np.array([[1.5, 1.5, 8.0, 1e-3, 0.0, 0.0, -1.0, 1e5]], dtype=np.float32)
    assert bits(none.trace(ray)[:, 3]).view(np.int32)[0] < 0
    one = HipScene(pointer, device=0, prototypes=[(0, 1)], instances=[(0, S.affine())])
    assert bits(one.trace(ray)[:, 3]).view(np.int32)[0] >= 0
    one.set_instance_transforms(S.affine(np.eye(3), (10.0, 0.0, 0.0)).reshape(1, 12))
    assert bits(one.trace(ray)[:, 3]).view(np.int32)[0] < 0
    far = ray.copy()
    far[0, 0] += 10.0
    fresh = HipScene(pointer, device=0, prototypes=[(0, 1)], instances=[(0, S.affine(np.eye(3), (10.0, 0.0, 0.0)))])
    assert np.array_equal(bits(one.trace(far)), bits(fresh.trace(far))) and bits(fresh.trace(far)[:, 3]).view(np.int32)[0] >= 0
