"""The scene loader's "instance" / "instanced" models (reference src/scene_parser.cpp:231-249, 279-285, 449-492): what the C++
host hands pathed_hip_scene_create_instanced -- a ONE-level list of placements with nesting composed in double and rounded
once, transforms read column-major, emissive faces baked into world triangles and lights once per placement -- and that
pathed_amd.flatten_instances writes the triangles out in the order of the virtual primitive ids.  CPU only."""
import json

import numpy as np
import pytest

from pathed_amd import flatten_instances
from pathed_amd.instances import flatten_points
from pathed_amd.scene import LoadedScene


def column_major(linear, translation):
    matrix = np.eye(4)
    matrix[:3, :3] = linear
    matrix[:3, 3] = translation
    return ["%.9g" % float(np.float32(x)) for x in matrix.T.reshape(-1)]


def quad(diffuse, translate, emit=None, scale=("1", "1", "1")):
    bsdf = {"type": "lambertian", "diffuseReflectance": diffuse}
    if emit is not None:
        bsdf["emit"] = emit
    return {"type": "quad", "bsdf": bsdf, "transform": {"scale": list(scale), "translate": list(translate)}}


def turn(degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


INNER = (0.5 * turn(30.0), (0.25, 1.5, -0.75))       # "leaf" inside "branch"
OUTER = [(turn(40.0), (3.0, 0.5, 1.0)), (np.diag([2.0, 1.0, -1.5]), (-4.0, 0.25, 2.0))]   # "branch" in the world, twice


def scene_file(tmp_path, models=None, **extra):
    scene = {
        "sensor": {"lookAt": {"origin": ["0", "3", "12"], "target": ["0", "1", "0"], "up": ["0", "1", "0"]}, "fov": "40"},
        "models": models if models is not None else [
            quad(["0.5", "0.5", "0.5"], ("0", "0", "0"), scale=("10", "1", "10")),
            {"type": "instance", "name": "leaf", "models": [quad(["0.2", "0.7", "0.2"], ("0.5", "2", "0.5"))]},
            {"type": "instance", "name": "branch", "models": [
                quad(["0.6", "0.4", "0.2"], ("1", "1", "1")),
                quad(["0", "0", "0"], ("1", "3", "1"), emit=["5", "4", "3"]),
                {"type": "instanced", "instance_name": "leaf", "transform": column_major(*INNER)},
            ]},
            {"type": "instanced", "instance_name": "branch", "transform": column_major(*OUTER[0])},
            {"type": "instanced", "instance_name": "branch", "transform": column_major(*OUTER[1])},
        ],
    }
    scene.update(extra)
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(scene))
    return str(path)


def arrays(desc):
    d = desc.contents
    positions = np.ctypeslib.as_array(d.positions, shape=(d.n_vertices, 3)).copy()
    indices = np.ctypeslib.as_array(d.indices, shape=(d.n_triangles, 3)).copy()
    materials = np.ctypeslib.as_array(d.tri_material, shape=(d.n_triangles,)).copy()
    return d, positions, indices, materials


def as_float32(linear, translation):
    """the floats of the file: what the loader parsed"""
    return np.asarray(linear, dtype=np.float32).astype(np.float64), np.asarray(translation, dtype=np.float32).astype(np.float64)


def test_the_loader_hands_the_abi_a_one_level_list(tmp_path):
    scene = LoadedScene(scene_file(tmp_path), 32, 24, "")
    d, positions, indices, materials = arrays(scene.desc)
    emissive = [i for i in range(d.n_triangles) if tuple(d.materials[materials[i]].emit) != (0.0, 0.0, 0.0)]

    # geoms: the floor, the emissive quad baked once per placement of "branch", then the prototypes "leaf" and "branch"
    assert d.n_geoms == 5 and [d.geoms[g].count for g in range(5)] == [2, 2, 2, 2, 2]
    assert emissive == [2, 3, 4, 5]
    assert scene.prototypes == [(3, 1), (4, 1)]

    # one level: per placement of "branch" the prototype itself, then "leaf" under the composed transform
    assert [prototype for prototype, _ in scene.instances] == [1, 0, 1, 0]
    inner_linear, inner_translation = as_float32(*INNER)
    for k, outer in enumerate(OUTER):
        linear, translation = as_float32(*outer)
        expected = np.hstack([linear, translation[:, None]]).astype(np.float32).reshape(12)
        assert np.array_equal(np.asarray(scene.instances[2 * k][1], dtype=np.float32), expected)
        # a translation is read from elements 12..14 of the column-major array
        assert np.array_equal(np.asarray(scene.instances[2 * k][1], dtype=np.float32).reshape(3, 4)[:, 3], np.asarray(outer[1], dtype=np.float32))
        # the composed transform: the float64 product of the two parsed transforms, rounded once to float32
        composed = np.hstack([linear @ inner_linear, (linear @ inner_translation + translation)[:, None]]).astype(np.float32).reshape(12)
        assert np.array_equal(np.asarray(scene.instances[2 * k + 1][1], dtype=np.float32), composed)

    # the emissive quad: world triangles through the flatten routine, once per placement, and ordinary lights
    branch_first = d.geoms[4].first
    model = LoadedScene(scene_file(tmp_path, models=[quad(["0", "0", "0"], ("1", "3", "1"), emit=["5", "4", "3"])]), 32, 24, "")
    _, model_positions, model_indices, _ = arrays(model.desc)
    for k in range(2):
        baked = positions[indices[2 + 2 * k: 4 + 2 * k]].reshape(-1, 3)
        expected = flatten_points(scene.instances[2 * k][1], model_positions[model_indices].reshape(-1, 3))
        assert np.array_equal(baked.view(np.uint32), expected.view(np.uint32))
    # ... and the rest of "branch" stays a prototype, in its own space
    kept = LoadedScene(scene_file(tmp_path, models=[quad(["0.6", "0.4", "0.2"], ("1", "1", "1"))]), 32, 24, "")
    _, kept_positions, kept_indices, _ = arrays(kept.desc)
    assert np.array_equal(positions[indices[branch_first:branch_first + 2]], kept_positions[kept_indices])


def test_flatten_instances_orders_the_triangles_by_virtual_id(tmp_path):
    scene = LoadedScene(scene_file(tmp_path), 32, 24, "")
    d, positions, indices, materials = arrays(scene.desc)
    flat = flatten_instances(scene.desc, scene.prototypes, scene.instances)
    f, flat_positions, flat_indices, flat_materials = arrays(flat.desc)
    world = d.geoms[3].first
    assert world == 6 and f.n_triangles == world + 2 * 4
    assert flat.bases.tolist() == [6, 8, 10, 12, 14]
    assert np.array_equal(flat_positions[flat_indices[:world]], positions[indices[:world]])
    for k, (prototype, transform) in enumerate(scene.instances):
        first = d.geoms[scene.prototypes[prototype][0]].first
        expected = flatten_points(transform, positions[indices[first:first + 2]].reshape(-1, 3)).reshape(2, 3, 3)
        assert np.array_equal(flat_positions[flat_indices[flat.bases[k]:flat.bases[k + 1]]].view(np.uint32), expected.view(np.uint32))
        assert np.array_equal(flat_materials[flat.bases[k]:flat.bases[k + 1]], materials[first:first + 2])
    assert [f.geoms[g].first for g in range(f.n_geoms)] == [0, 2, 4, 6, 8, 10, 12]


def test_the_loaders_refusals_name_the_thing(tmp_path):
    floor = quad(["0.5", "0.5", "0.5"], ("0", "0", "0"))
    leaf = {"type": "instance", "name": "leaf", "models": [quad(["0.2", "0.7", "0.2"], ("0", "1", "0"))]}
    identity = column_major(np.eye(3), (0, 0, 0))

    def refused(models, *words):
        with pytest.raises(RuntimeError) as caught:
            LoadedScene(scene_file(tmp_path, models=models), 16, 16, "")
        for word in words:
            assert word in str(caught.value), str(caught.value)

    refused([floor, {"type": "instanced", "instance_name": "twig", "transform": identity}], "unknown instance_name", "twig")
    refused([floor, leaf, {"type": "instanced", "instance_name": "leaf", "transform": identity[:12]}], "16 numbers")
    branch = {"type": "instance", "name": "branch", "models": [{"type": "instanced", "instance_name": "leaf", "transform": identity}]}
    tree = {"type": "instance", "name": "tree", "models": [{"type": "instanced", "instance_name": "branch", "transform": identity}]}
    refused([floor, leaf, branch, tree], "two levels", "branch")
    # a cycle cannot be written down: a name is known only once its instance is complete
    loop = {"type": "instance", "name": "loop", "models": [{"type": "instanced", "instance_name": "loop", "transform": identity}]}
    refused([floor, loop], "unknown instance_name", "loop")
    ball = {"type": "sphere", "center": ["0", "1", "0"], "radius": "0.5", "bsdf": {"type": "lambertian", "diffuseReflectance": ["0.5", "0.5", "0.5"]}}
    refused([floor, {"type": "instance", "name": "ball", "models": [ball]}], "sphere inside an instance")
    refused([floor, {"type": "instance", "models": [floor]}], "name")


@pytest.mark.parametrize("change, words", [
    ({"bvh_builder": "ploc"}, ["bvh_builder", "ploc", "instances"]),
    ({"bvh_builder": "lbvh"}, ["bvh_builder", "lbvh", "instances"]),
    ({"features": ["albedo"]}, ["features", "instances"]),
    ({"integrator": "AlbedoIntegrator"}, ["AlbedoIntegrator", "instances"]),
    ({"integrator": "VolumePathTracer"}, ["VolumePathTracer", "instances"]),
    ({"integrator": "BasicVolumeIntegrator"}, ["BasicVolumeIntegrator", "instances"]),
])
def test_the_job_runner_refuses_by_name_beside_instances(tmp_path, change, words):
    """What the library refuses beside instances stops a job in the C++ host once the scene is read: before a tree is built or
    a device is touched (no GPU is needed to get this far)."""
    import os
    import subprocess
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update({"scene": scene_file(tmp_path), "output_directory": str(tmp_path / "out"), "width": 16, "height": 16, "spp": 1})
    job.update(change)
    job_path = tmp_path / "job.json"
    job_path.write_text(json.dumps(job))
    result = subprocess.run([os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed"), str(job_path), ""], capture_output=True, text=True, timeout=120)
    assert result.returncode != 0
    for word in words:
        assert word in result.stderr + result.stdout, result.stderr + result.stdout
