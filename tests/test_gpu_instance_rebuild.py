"""Rebuilding the top tree of an instanced scene on the device (include/pathed_hip.h: pathed_hip_scene_rebuild_top; DESIGN.md
section 4.6d; lbvh.hip: buildTopBvhOnDevice; instance_kernels.h: k_placement_boxes, k_rebase_prototype_nodes, k_rebase_instance_roots).
The yardstick throughout is a scene CREATED with the same placements: hits do not depend on the tree (DESIGN.md "Intersector
specification"), so a rebuilt scene answers with the fresh scene's bits although its top tree is another one.  Every case runs
for both device builders.

1. rebuilt equals fresh   traces (closest and any hit), moments at bounces 0..3; without a move; and back without residue
2. tree                   the exported arrays: the top tree is the head, one instance leaf per placement with the rule's box,
                          boxes contain what is below, world triangles permuted, prototypes rebased, records rebased
3. edges                  0 / 4 / 32 world triangles, 2 / 5 / 300 coincident placements, fewer than two primitives
4. depth                  4 096 placements shuffled over a grid: the stack's bound is restated, then a refit of the rebuilt tree
5. lists                  render_pixels after a rebuild
6. refusals               by code and by name; the scene stays as it was
"""
import ctypes as C

import numpy as np
import pytest

from pathed_amd import flatten_instances
from pathed_amd import instances as I
from pathed_amd.integrator import HipScene, _check

import instances_scene as S
from test_gpu_instance_motion import (EMPTY, INSTANCE_BIT, INVALID, SIZE, UNSUPPORTED, Scene, assert_same_answers, assert_same_moments, bits,
                                      child_box, moved_placements, query_rays, refused, top_tree, transforms_of)

pytestmark = pytest.mark.gpu

BUILDERS = ("lbvh", "ploc")


@pytest.fixture(scope="module")
def fresh_moved():
    """created with M1, never touched"""
    return Scene(moved_placements())


@pytest.fixture(scope="module")
def fresh_general():
    return Scene(S.GENERAL_PLACEMENTS)


# --------------------------------------------------------------------------------------------------- 1. rebuilt equals fresh

@pytest.mark.parametrize("builder", BUILDERS)
def test_rebuilt_equals_fresh_and_back(builder, fresh_moved, fresh_general):
    scene = Scene(S.GENERAL_PLACEMENTS)
    # a rebuild with no move before it
    assert scene.gpu.rebuild_top(builder) > 0.0
    closest, shadow = query_rays(fresh_general.flat(), seed=41)
    assert_same_answers(scene.gpu, fresh_general.gpu, closest, shadow)
    # moved to M1, then rebuilt
    scene.gpu.set_instance_transforms(transforms_of(moved_placements()))
    assert scene.gpu.rebuild_top(builder) > 0.0
    flat = scene.flat()
    closest, shadow = query_rays(flat, seed=17)
    prim = bits(fresh_moved.gpu.trace(closest)[:, 3]).view(np.int32)
    for k in range(len(scene.placements)):
        assert ((prim >= flat.bases[k]) & (prim < flat.bases[k + 1])).sum() > 50, k
    assert_same_answers(scene.gpu, fresh_moved.gpu, closest, shadow)
    assert_same_moments(scene.gpu, fresh_moved.gpu)
    stats = scene.gpu.stats()
    assert stats["path_kernel"] == 10 and stats["bvh_builder"] == 0   # (what the scene was created with)
    # and back, rebuilt again: no residue of M1
    scene.gpu.set_instance_transforms(transforms_of(S.GENERAL_PLACEMENTS))
    scene.gpu.rebuild_top(builder)
    closest, shadow = query_rays(fresh_general.flat(), seed=23)
    assert_same_answers(scene.gpu, fresh_general.gpu, closest, shadow)
    assert_same_moments(scene.gpu, fresh_general.gpu)
    mine, theirs = scene.gpu.instance_records(), fresh_general.gpu.instance_records()
    assert np.array_equal(bits(mine[0]), bits(theirs[0])) and np.array_equal(bits(mine[1]), bits(theirs[1]))
    assert np.array_equal(mine[2][:, [0, 1, 3]], theirs[2][:, [0, 1, 3]])


# ------------------------------------------------------------------------------------------------------------------ 2. tree

def levels(refs, root):
    """4-wide levels below and including `root`, following inner references only"""
    depth, frontier = 0, [root]
    while frontier:
        depth += 1
        frontier = [int(r) for node in frontier for r in refs[node] if r >= 0]
    return depth


def deepest_prototype(refs, top):
    """levels of the deepest prototype tree behind the top tree: their roots are the nodes no inner reference names (a
    prototype no placement uses counts as well, as it does for the traversal stack's bound)"""
    roots = set(range(top, len(refs))) - set(int(r) for r in refs.reshape(-1) if r >= 0)
    return max(levels(refs, root) for root in roots)


def assert_boxes_contain_what_is_below(nodes, tris, seen):
    """every inner child box contains the child node's boxes; every triangle leaf's box the real-valued corners of its triangles"""
    refs = nodes[:, 24:28].view(np.int32)
    for node in seen:
        for slot in range(4):
            ref = int(refs[node, slot])
            if ref == EMPTY:
                continue
            lo, hi = child_box(nodes, node, slot)
            if ref >= 0:
                for below in range(4):
                    if int(refs[ref, below]) == EMPTY:
                        continue
                    below_lo, below_hi = child_box(nodes, ref, below)
                    assert np.all(lo <= below_lo) and np.all(hi >= below_hi), (node, slot, below)
            elif not ((-ref - 1) & INSTANCE_BIT):
                first, count = (-ref - 1) >> 3, (-ref - 1) & 7
                for record in tris[first:first + count].astype(np.float64):   # (float64 sums of two float32 are exact enough: 29 spare bits)
                    for corner in (record[0:3], record[0:3] + record[4:7], record[0:3] + record[8:11]):
                        assert np.all(lo <= corner) and np.all(hi >= corner), (node, slot)


@pytest.mark.parametrize("builder", BUILDERS)
def test_the_rebuilt_top_tree(builder, fresh_moved):
    scene = Scene(S.GENERAL_PLACEMENTS)
    gpu = scene.gpu
    gpu.set_instance_transforms(transforms_of(moved_placements()))
    before_nodes, before_tris = gpu.export_bvh()
    records_before = gpu.instance_records()
    old_top = len(top_tree(before_nodes)[0])
    world = 4   # the floor and the emitter

    gpu.rebuild_top(builder)
    nodes, tris = gpu.export_bvh()
    stats = gpu.stats()
    seen, leaves = top_tree(nodes)
    top = len(seen)
    assert sorted(seen) == list(range(top))   # the top tree is the head of the node array
    assert stats["bvh_nodes"] == len(nodes) == top + (len(before_nodes) - old_top)
    assert stats["bvh_bytes"] == 128 * len(nodes) + 48 * len(tris)
    delta = top - old_top

    fresh_nodes, _ = fresh_moved.gpu.export_bvh()
    _, fresh_leaves = top_tree(fresh_nodes)
    desc = scene.built.desc
    for k, (prototype, transform) in enumerate(moved_placements()):
        assert len(leaves.get(k, [])) == 1 and len(fresh_leaves.get(k, [])) == 1, k
        lo, hi = child_box(nodes, *leaves[k][0])
        fresh_lo, fresh_hi = child_box(fresh_nodes, *fresh_leaves[k][0])
        assert np.array_equal(bits(lo), bits(fresh_lo)) and np.array_equal(bits(hi), bits(fresh_hi)), k
        geom = desc.geoms[scene.prototypes[prototype][0]]
        corners = np.ctypeslib.as_array(desc.indices, shape=(int(desc.n_triangles), 3))[geom.first:geom.first + geom.count].reshape(-1)
        positions = np.ctypeslib.as_array(desc.positions, shape=(int(desc.n_vertices), 3))[corners]
        rule_lo, rule_hi = I.pad_box(*I.placement_box(transform, *I.prototype_box(positions)))
        assert np.array_equal(bits(lo), bits(rule_lo)) and np.array_equal(bits(hi), bits(rule_hi)), k
    assert sorted(leaves) == list(range(len(scene.placements)))
    assert_boxes_contain_what_is_below(nodes, tris, seen)

    # every world triangle once, with the bits it had, and referenced once by the top tree's triangle leaves
    assert sorted(map(bytes, bits(tris[:world]))) == sorted(map(bytes, bits(before_tris[:world])))
    assert len(set(map(bytes, bits(before_tris[:world])))) == world
    refs = nodes[:, 24:28].view(np.int32)
    covered = []
    for ref in refs[:top].reshape(-1):
        if ref < 0 and ref != EMPTY and not ((-int(ref) - 1) & INSTANCE_BIT):
            covered += list(range((-int(ref) - 1) >> 3, ((-int(ref) - 1) >> 3) + ((-int(ref) - 1) & 7)))
    assert sorted(covered) == list(range(world))
    # the prototypes: nodes moved by delta, inner references with them, triangles untouched
    expected = before_nodes[old_top:].copy()
    inner = expected[:, 24:28].view(np.int32)
    inner[inner >= 0] += delta
    assert len(nodes) > top and np.array_equal(bits(nodes[top:]), bits(expected))
    assert len(tris) == len(before_tris) and np.array_equal(bits(tris[world:]), bits(before_tris[world:]))
    # the records: only protoRoot, by the same delta
    records = gpu.instance_records()
    assert np.array_equal(bits(records[0]), bits(records_before[0])) and np.array_equal(bits(records[1]), bits(records_before[1]))
    assert np.array_equal(records[2][:, [0, 1, 3]], records_before[2][:, [0, 1, 3]])
    assert np.array_equal(records[2][:, 2], records_before[2][:, 2] + delta)
    assert np.all(records[2][:, 2] >= top)
    # the depth the statistics report is the new tree's
    assert set(int(root) for root in records[2][:, 2]) <= set(range(top, len(nodes)))
    assert stats["bvh_max_depth"] == levels(refs, 0) + deepest_prototype(refs, top)


# ----------------------------------------------------------------------------------------------------------------- 3. edges

def box_world(world):
    """(pointer, prototypes, keep-alive): a unit box as the one prototype behind `world` triangles of a floor"""
    built = S.BuiltScene(24, 16, origin=(0.0, 4.0, 14.0), target=(0.0, 0.5, 0.0), fov_degrees=50.0)
    grey = built.material()
    if world == 4:
        built.quad([(-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8)], grey)
        built.quad([(-2, 6, -2), (2, 6, -2), (2, 6, 2), (-2, 6, 2)], grey)
    elif world:
        side = int(round((world / 2) ** 0.5))
        assert 2 * side * side == world
        grid = [(-8.0 + 16.0 * i / side, 0.0, -8.0 + 16.0 * j / side) for j in range(side + 1) for i in range(side + 1)]
        faces = []
        for j in range(side):
            for i in range(side):
                a, b, c, d = j * (side + 1) + i, j * (side + 1) + i + 1, (j + 1) * (side + 1) + i + 1, (j + 1) * (side + 1) + i
                faces += [(a, d, c), (a, c, b)]
        built.mesh(grid, faces, grey)
    first = len(built.geoms)
    built.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), grey)
    return built.finish(), [(first, 1)], built


def spread(count, seed):
    rng = np.random.default_rng(seed)
    return [(0, S.affine(rng.uniform(0.6, 1.4) * S.rotation((0.2, 1.0, 0.1), rng.uniform(0, 360)), rng.uniform((-6, 0, -6), (6, 2, 6)))) for _ in range(count)]


EDGES = {
    "no world, two placements": (0, lambda: spread(2, 1), lambda: spread(2, 2)),
    "four world triangles": (4, lambda: spread(3, 3), lambda: spread(3, 4)),
    "a floor of 32 triangles, five placements": (32, lambda: spread(5, 5), lambda: spread(5, 6)),
    "300 placements, one transform": (4, lambda: spread(300, 7), lambda: 300 * spread(1, 8)),
}


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_the_builders_edges(edge, builder):
    world, start, end = EDGES[edge]
    pointer, prototypes, keep = box_world(world)
    start, end = start(), end()
    scene = HipScene(pointer, device=0, prototypes=prototypes, instances=start)
    fresh = HipScene(pointer, device=0, prototypes=prototypes, instances=end)
    scene.set_instance_transforms(transforms_of(end))
    assert scene.rebuild_top(builder) > 0.0
    flat = flatten_instances(pointer, prototypes, end)
    closest = np.concatenate([S.general_rays(flat, 1500, 3), S.camera_rays(32, 24, (0.0, 4.0, 14.0), (0.0, 0.5, 0.0))])
    shadow = S.general_rays(flat, 1500, 4)
    shadow[:, 7] = np.where(np.arange(len(shadow)) % 2 == 1, 2.0, 0.5).astype(np.float32)
    assert_same_answers(scene, fresh, closest, shadow)
    nodes, tris = scene.export_bvh()
    seen, leaves = top_tree(nodes)
    assert sorted(seen) == list(range(len(seen))) and sorted(leaves) == list(range(len(end))) and all(len(v) == 1 for v in leaves.values())
    assert scene.stats()["bvh_nodes"] == len(nodes)
    assert_boxes_contain_what_is_below(nodes, tris, seen)
    assert sorted(map(bytes, bits(tris[:world]))) == sorted(map(bytes, bits(fresh.export_bvh()[1][:world])))


@pytest.mark.parametrize("builder", BUILDERS)
def test_fewer_than_two_primitives_leave_the_tree_alone(builder):
    pointer, prototypes, keep = box_world(0)
    ray = np.array([[0.0, 0.5, 8.0, 1e-3, 0.0, 0.0, -1.0, 1e5]], dtype=np.float32)
    none = HipScene(pointer, device=0, prototypes=prototypes, instances=[])
    before = none.export_bvh()
    assert none.rebuild_top(builder) == 0.0
    after = none.export_bvh()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
    assert np.all(after[0][0, 24:28].view(np.int32) == EMPTY)   # the empty root: node 0 is never a prototype's
    assert bits(none.trace(ray)[:, 3]).view(np.int32)[0] < 0
    one = HipScene(pointer, device=0, prototypes=prototypes, instances=[(0, S.affine())])
    before, hit = one.export_bvh(), one.trace(ray)
    assert bits(hit[:, 3]).view(np.int32)[0] >= 0
    assert one.rebuild_top(builder) == 0.0
    after = one.export_bvh()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
    assert np.array_equal(bits(one.trace(ray)), bits(hit))


# ----------------------------------------------------------------------------------------------------------------- 4. depth

GRID = 4096


def grid_placements(which):
    side = 64
    spots = [(-11.8 + 0.375 * (k % side), 0.35 + 0.5 * ((k * 7) % 5), -11.8 + 0.375 * (k // side)) for k in range(GRID)]
    linears = [0.22 * S.rotation((0.2, 1.0, 0.1 + 0.001 * k), 11.0 * k) for k in range(GRID)]
    order = np.random.default_rng(2024).permutation(GRID)
    if which == "start":
        return [(S.Q, S.placed(linears[k], spots[k], S.Q_CENTRE)) for k in range(GRID)]
    lift = (0.0, 0.0, 0.0) if which == "shuffled" else (0.05, 0.02, -0.03)   # "nudged": the shuffled set after a small move
    return [(S.Q, S.placed(linears[k], np.add(spots[int(order[k])], lift), S.Q_CENTRE)) for k in range(GRID)]


@pytest.fixture(scope="module")
def fresh_grids():
    return {which: Scene(grid_placements(which), (32, 24)) for which in ("shuffled", "nudged")}


@pytest.mark.parametrize("builder", BUILDERS)
def test_a_shuffled_grid_of_4096_placements(builder, fresh_grids):
    scene = Scene(grid_placements("start"), (32, 24))
    fresh = fresh_grids["shuffled"]
    scene.gpu.set_instance_transforms(transforms_of(grid_placements("shuffled")))
    scene.gpu.rebuild_top(builder)
    rays = S.camera_rays(64, 48, S.CAMERA["origin"], S.CAMERA["target"])
    mine, theirs = scene.gpu.trace(rays), fresh.gpu.trace(rays)
    prim = bits(theirs[:, 3]).view(np.int32)
    assert len(np.unique((prim[prim >= 4] - 4) // 12)) > 100   # many placements are seen (world: 4 triangles; Q: 12 each)
    assert np.array_equal(bits(mine), bits(theirs))
    # the statistics are the new tree's
    nodes, _ = scene.gpu.export_bvh()
    refs = nodes[:, 24:28].view(np.int32)
    stats = scene.gpu.stats()
    seen, leaves = top_tree(nodes)
    top_levels = levels(refs, 0)
    assert top_levels >= 4
    assert stats["bvh_max_depth"] == top_levels + deepest_prototype(refs, len(seen))
    assert stats["bvh_nodes"] == len(nodes)
    assert sorted(seen) == list(range(len(seen))) and sorted(leaves) == list(range(GRID)) and all(len(v) == 1 for v in leaves.values())
    # a render walks it under the restated stack bound
    sums, squares = scene.gpu.render_moments(5, 0, 4, 0, 3)
    fresh_sums, fresh_squares = fresh.gpu.render_moments(5, 0, 4, 0, 3)
    assert float(fresh_sums.sum()) > 0.0
    assert np.array_equal(bits(sums), bits(fresh_sums)) and np.array_equal(bits(squares), bits(fresh_squares))
    # a further small move refits the REBUILT tree
    scene.gpu.set_instance_transforms(transforms_of(grid_placements("nudged")))
    nudged = fresh_grids["nudged"]
    assert np.array_equal(bits(scene.gpu.trace(rays)), bits(nudged.gpu.trace(rays)))
    sums, squares = scene.gpu.render_moments(5, 0, 4, 0, 3)
    fresh_sums, fresh_squares = nudged.gpu.render_moments(5, 0, 4, 0, 3)
    assert np.array_equal(bits(sums), bits(fresh_sums)) and np.array_equal(bits(squares), bits(fresh_squares))
    assert np.array_equal(bits(scene.gpu.export_bvh()[0][:, 24:28]), bits(nodes[:, 24:28]))   # the refit kept the rebuilt shape


# ----------------------------------------------------------------------------------------------------------------- 5. lists

@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("listed", (1, 65, SIZE[0] * SIZE[1]))
def test_a_list_pass_after_a_rebuild(listed, builder, fresh_moved):
    width, height = SIZE
    pixels = width * height
    full_sums, full_squares = fresh_moved.gpu.render_moments(5, 0, 4, 0, 3)
    chosen = np.sort(np.random.default_rng(listed).choice(pixels, listed, replace=False)).astype(np.uint32)
    scene = Scene(S.GENERAL_PLACEMENTS)
    gpu = scene.gpu
    gpu.set_instance_transforms(transforms_of(moved_placements()))
    gpu.rebuild_top(builder)
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
    assert listed == 1 or float(full_sums.reshape(pixels, 3)[chosen].sum()) > 0.0
    assert np.array_equal(bits(sums[chosen]), bits(full_sums.reshape(pixels, 3)[chosen]))
    assert np.array_equal(bits(squares[chosen]), bits(full_squares.reshape(pixels, 3)[chosen]))
    assert np.all(sums[others] == np.float32(0.375)) and np.all(squares[others] == np.float32(0.375))
    assert np.all(counts[chosen] == 11) and np.all(counts[others] == 7)


# -------------------------------------------------------------------------------------------------------------- 6. refusals

def test_refusals_leave_the_scene_as_it_was(fresh_general):
    scene = Scene(S.GENERAL_PLACEMENTS)
    gpu = scene.gpu
    closest, shadow = query_rays(fresh_general.flat(), seed=31)
    tree_before = gpu.export_bvh()
    records_before = gpu.instance_records()
    hits_before, occluded_before = gpu.trace(closest), gpu.trace(shadow, any_hit=True)

    def unchanged():
        tree = gpu.export_bvh()
        assert np.array_equal(bits(tree[0]), bits(tree_before[0])) and np.array_equal(bits(tree[1]), bits(tree_before[1]))
        for mine, theirs in zip(gpu.instance_records(), records_before):
            assert np.array_equal(bits(mine), bits(theirs))
        assert np.array_equal(bits(gpu.trace(closest)), bits(hits_before))
        assert np.array_equal(gpu.trace(shadow, any_hit=True), occluded_before)

    flat = flatten_instances(scene.pointer, scene.prototypes, scene.placements)
    plain = HipScene(flat.desc, device=0)
    plain_hits = plain.trace(closest)
    refused(lambda: plain.rebuild_top("ploc"), UNSUPPORTED, "no instances")
    assert np.array_equal(bits(plain.trace(closest)), bits(plain_hits))
    lib = gpu._lib
    refused(lambda: _check(lib, lib.pathed_hip_scene_rebuild_top(None, 2, None), "rebuild"), INVALID, "null")
    unchanged()
    refused(lambda: gpu.rebuild_top("sah"), UNSUPPORTED, "host builder")
    unchanged()
    for unknown in (3, -1, 1 << 20):
        refused(lambda: gpu.rebuild_top(unknown), UNSUPPORTED, "host builder")
    unchanged()
    assert gpu.stats()["bvh_nodes"] == len(tree_before[0])
    # and the scene still rebuilds afterwards
    assert gpu.rebuild_top("lbvh") > 0.0
    assert_same_answers(gpu, fresh_general.gpu, closest, shadow)
