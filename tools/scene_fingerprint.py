"""What scene creation leaves on the device, as one SHA-256 per section per scene, so that a change of the host code that
builds a scene (pathed_amd/csrc/pathed_hip.hip: createScene and its stages, scene_tables.h) shows up as the section it moved.

    python tools/scene_fingerprint.py --commit <id> --out fingerprints.json

Sections: the tree's nodes and leaf triangles (export_bvh), the per-triangle and per-light constants (light_records), the item
order and the camera masks of the fused kernel, the placements' records, the statistics that name the kernel choice, and the
radiance sums of a 48 x 32 render (4 spp, seed 2^32 + 1, bounces 0..5).  A hook that does not apply to a scene (camera masks
on a tree-walked scene, say) is recorded by its error text: which scenes a hook serves is part of the fingerprint.  Refused
creations are recorded by the code and the text of pathed_hip_last_error().  The device builders' trees are fingerprinted
only when two builds in a row give the same tree (`tree_repeats`); their render sums always are: hits are bit-identical over
any tree.  tests/test_gpu_scene_fingerprint.py compares against tests/golden/scene_fingerprints.json.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (REPO_ROOT, os.path.join(REPO_ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

WIDTH, HEIGHT, SPP, SEED, BOUNCES = 48, 32, 4, (1 << 32) + 1, (0, 5)


def sha(*arrays):
    digest = hashlib.sha256()
    for array in arrays:
        array = np.ascontiguousarray(array)
        digest.update(("%s%s" % (array.dtype.str, array.shape)).encode())
        digest.update(array.tobytes())
    return digest.hexdigest()


def mesh_scene(with_sphere=False):
    """A textured, environment-lit icosphere (vertex normals, uvs) over two adjacent plain meshes (a large floor, a small box):
    gamma texels, the environment tables (one black row, one bright texel), plain ranges, the env-only shade kernel and the
    local set (the floor's two triangles are large, the rest is not)."""
    from pathed_amd import _capi
    from scene_builder import BuiltScene
    from instances_scene import icosphere
    rng = np.random.default_rng(11)
    built = BuiltScene(WIDTH, HEIGHT, (0.5, 2.5, 7.0), (0.0, 1.0, 0.0), fov_degrees=40.0)
    texture = built.texture(rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8))
    skin = built.material(_capi.MAT_LAMBERTIAN, texture=texture)
    grey = built.material(_capi.MAT_LAMBERTIAN, diffuse=(0.6, 0.6, 0.55))
    blue = built.material(_capi.MAT_PLASTIC, diffuse=(0.2, 0.3, 0.6), alpha=0.15)
    positions, faces, normals, uvs = icosphere((0.0, 1.2, 0.0), 1.0)
    built.mesh(positions, faces, skin, normals=normals, uvs=uvs)
    built.mesh([(-9, 0, -9), (-9, 0, 9), (9, 0, 9), (9, 0, -9)], [(0, 1, 2), (0, 2, 3)], grey)     # plain: no normals, no uvs
    built.box((1.5, 0.0, -0.5), (2.2, 0.7, 0.2), blue)                                               # plain, adjacent
    if with_sphere:
        built.sphere((-1.8, 0.5, 0.6), 0.5, built.material(_capi.MAT_MIRROR))
    rgba = rng.uniform(0.05, 1.0, size=(6, 9, 4)).astype(np.float32)
    rgba[2, :, :3] = 0.0                     # an all-black row
    rgba[1, 4, :3] = (40.0, 35.0, 30.0)      # one bright texel
    built.environment(rgba, scale=1.5)
    return built, built.finish()


def describe(make_scene, integrator=None, refit=False, tree="always", **options):
    """The sections of one scene.  tree: "always" | "if-repeatable" (the device builders)."""
    from pathed_amd.integrator import HipScene, PathedError
    keep, desc, extra = make_scene()
    n_triangles, n_spheres = int(desc.contents.n_triangles), int(desc.contents.n_spheres)

    def hook(call, pack):
        try:
            return pack(call())
        except PathedError as error:
            return "refused: %s" % error

    def create():
        scene = HipScene(desc, device=0, **extra, **options)
        if integrator:
            scene.set_integrator(integrator)
        return scene

    scene = create()
    out = {}
    nodes, tris = scene.export_bvh()
    repeats = True
    if tree == "if-repeatable":
        again = create()
        nodes2, tris2 = again.export_bvh()
        repeats = np.array_equal(nodes.view(np.uint32), nodes2.view(np.uint32)) and np.array_equal(tris.view(np.uint32), tris2.view(np.uint32))
        again.close()
        out["tree_repeats"] = bool(repeats)
    if repeats:
        out["nodes"] = sha(nodes.view(np.uint32))
        out["leaf_triangles"] = sha(tris.view(np.uint32))
    out["light_records"] = hook(lambda: scene.light_records(n_triangles, n_triangles + n_spheres + 1), lambda r: sha(r[0].view(np.uint32), r[1].view(np.uint32)))
    out["item_order"] = hook(lambda: scene.item_order(n_triangles), sha)
    out["camera_masks"] = hook(scene.camera_masks, sha)
    out["instance_records"] = hook(scene.instance_records, lambda r: sha(r[0].view(np.uint32), r[1].view(np.uint32), r[2]))
    image = scene.render(SEED, 0, SPP, BOUNCES[0], BOUNCES[1])
    out["render"] = sha(image.view(np.uint32))
    stats = scene.stats()
    names = ("path_kernel", "scene_in_lds", "bvh_nodes", "bvh_max_depth", "bvh_builder") if repeats else ("path_kernel", "scene_in_lds", "bvh_builder")
    out["stats"] = {name: int(stats[name]) for name in names}
    if refit:
        positions = np.ctypeslib.as_array(desc.contents.positions, shape=(int(desc.contents.n_vertices), 3)).copy()
        scene.refit(positions)
        out["render_after_refit"] = sha(scene.render(SEED, 0, SPP, BOUNCES[0], BOUNCES[1]).view(np.uint32))
    scene.close()
    return out


def refusal(make_scene, **options):
    from pathed_amd.integrator import HipScene, PathedError
    keep, desc, extra = make_scene()
    try:
        HipScene(desc, **{"device": 0, **extra, **options}).close()
    except PathedError as error:
        return {"refused": str(error)}
    return {"refused": None}


def cornell():
    from pathed_amd.scene import LoadedScene
    loaded = LoadedScene("scenes/cornell.json", WIDTH, HEIGHT)     # scenes/CornellBox-Original.obj
    return loaded, loaded.desc, {}


def sphere_room():
    from test_gpu_shadow_pruning import scenes
    desc, keep, _ = scenes()["sphere-light-moved"]
    return keep, desc, {}


def mesh():
    built, desc = mesh_scene()
    return built, desc, {}


def mesh_and_sphere():
    built, desc = mesh_scene(with_sphere=True)
    return built, desc, {}


def hybrid_soup():
    from test_gpu_hybrid import _soup
    built, desc = _soup(2, 100, 12, True)
    desc.contents.camera.width, desc.contents.camera.height = WIDTH, HEIGHT
    return built, desc, {}


def gas_room():
    import volume_scenes
    built = volume_scenes.gas_room(width=WIDTH, height=HEIGHT)
    return built, built.finish(), {}


def instanced():
    import instances_scene
    built, desc, prototypes, placements = instances_scene.build(instances_scene.GENERAL_PLACEMENTS, WIDTH, HEIGHT)
    return built, desc, {"prototypes": prototypes, "instances": placements}


# name -> (function, arguments): insertion order is the order of the file
SCENES = {
    "cornell": (describe, dict(make_scene=cornell)),
    "sphere-light-moved": (describe, dict(make_scene=sphere_room)),
    # (by default the hybrid kernel takes a mesh of this size; the per-slot wavefront is where k_shade_env and the local set run)
    "mesh-env": (describe, dict(make_scene=mesh, shade_kernel="per-slot")),
    "mesh-env-no-local-rays": (describe, dict(make_scene=mesh, shade_kernel="per-slot", local_rays=1)),
    "mesh-env-hybrid": (describe, dict(make_scene=mesh)),
    "hybrid-soup": (describe, dict(make_scene=hybrid_soup)),
    "hybrid-soup-refittable": (describe, dict(make_scene=hybrid_soup, refittable=1, refit=True)),
    "gas-room-volume": (describe, dict(make_scene=gas_room, integrator="VolumePathTracer")),
    "instanced": (describe, dict(make_scene=instanced)),
    "mesh-sphere-lbvh": (describe, dict(make_scene=mesh_and_sphere, bvh_builder="lbvh", tree="if-repeatable")),
    "mesh-sphere-ploc": (describe, dict(make_scene=mesh_and_sphere, bvh_builder="ploc", tree="if-repeatable")),
    "cornell-generic": (describe, dict(make_scene=cornell, generic_kernels=1)),
    "refused-fused-on-mesh": (refusal, dict(make_scene=mesh, shade_kernel="fused")),
    "refused-wave-on-cornell": (refusal, dict(make_scene=cornell, shade_kernel="wave")),
    "refused-hybrid-on-cornell": (refusal, dict(make_scene=cornell, shade_kernel="hybrid")),
    "refused-compressed-nodes": (refusal, dict(make_scene=mesh, node_format="compressed")),
    "refused-hybrid-with-sphere": (refusal, dict(make_scene=mesh_and_sphere, shade_kernel="hybrid")),
    "refused-device-id": (refusal, dict(make_scene=cornell, device=4096)),
}


def fingerprint(name):
    function, arguments = SCENES[name]
    return function(**arguments)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--commit", default="", help="the commit the library was built from (stored in the file)")
    parser.add_argument("--out", default="-")
    args = parser.parse_args()
    os.chdir(REPO_ROOT)
    record = {"recorded_on": args.commit, "scenes": {}}
    for name in SCENES:
        record["scenes"][name] = fingerprint(name)
        print(name, json.dumps(record["scenes"][name]), file=sys.stderr, flush=True)
    text = json.dumps(record, indent=1, sort_keys=False) + "\n"
    if args.out == "-":
        sys.stdout.write(text)
    else:
        with open(args.out, "w") as handle:
            handle.write(text)


if __name__ == "__main__":
    main()
