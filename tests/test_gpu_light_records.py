"""The records of per-light and per-triangle constants (pathed_amd/csrc/device_scene.h: the light sampling records, q7 of the
shading records, the second half of the plain-triangle records) hold, bit for bit, what the per-vertex functions compute for the
same triangles (triangleSample, trianglePdfSolidAngle, makeIsect: src/triangle.cpp:16-62, src/scene.cpp:121-218 in the
reference), and a refit rebuilds them: an emitter that moved is sampled where it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.int32)


def test_records_equal_what_the_per_vertex_functions_compute():
    from pathed_amd import _capi
    from pathed_amd.integrator import HipScene
    from scene_builder import BuiltScene
    built = BuiltScene(32, 32, (0.2, 0.4, 5.0), (0, 0, 0), fov_degrees=45.0)
    grey = built.material(diffuse=(0.6, 0.6, 0.6))
    lamp = built.material(diffuse=(0, 0, 0), emit=(9, 8, 7))
    second_lamp = built.material(diffuse=(0, 0, 0), emit=(1, 2, 3))
    rng = np.random.default_rng(11)
    built.box((-2, -2, -2), (2, 2, 2), grey)                                                     # plain triangles
    built.mesh(rng.normal(size=(12, 3)) * 1.5, [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(4)], grey)   # ... of any shape
    built.mesh([(-0.5, 1.9, -0.5), (0.5, 1.9, -0.5), (0.5, 1.9, 0.5), (-0.5, 1.9, 0.5)], [(0, 2, 1), (0, 3, 2)], lamp)   # a plain emitter
    built.quad([(-1.0, -1.9, 0.3), (0.1, -1.7, 0.2), (0.3, -1.8, 1.1), (-0.9, -1.9, 1.3)], second_lamp)   # an emitter with uvs
    slanted = rng.normal(size=(3, 3))
    built.mesh(slanted, [(0, 1, 2)], second_lamp, normals=rng.normal(size=(3, 3)))               # an emitter with vertex normals
    # zero-area emitters: three collinear corners, and one point three times (area 0, normal 0 / 0)
    built.mesh([(0, 0, 0), (1, 1, 1), (2, 2, 2)], [(0, 1, 2)], lamp)
    built.mesh([(0.25, 0.5, 0.75)] * 3, [(0, 1, 2)], lamp)
    built.sphere((1.0, 1.0, 1.0), 0.25, lamp)                                                    # a light that is not a triangle
    desc = built.finish()
    n_triangles = desc.contents.n_triangles
    gpu = HipScene(desc, device=0)
    triangles, lights = gpu.light_records(n_triangles, n_triangles + 2)

    positions = np.asarray(built.positions, dtype=np.float32)
    indices = np.asarray(built.indices)
    materials = np.asarray(built.tri_material)
    emissive = [i for i in range(n_triangles) if materials[i] in (lamp, second_lamp)]
    assert lights.shape[0] == len(emissive) + 1
    assert triangles.shape == (n_triangles, 20)

    # every triangle: (normal, 1 / area) of the shading record, the stored shading normal
    assert np.array_equal(_bits(triangles[:, 12:15]), _bits(triangles[:, 0:3]))
    assert np.array_equal(_bits(triangles[:, 15]), _bits(triangles[:, 4]))
    assert np.array_equal(_bits(triangles[:, 16:19]), _bits(triangles[:, 8:11]))
    regular = [i for i in range(n_triangles) if i not in emissive[-2:]]
    assert np.all(np.isfinite(triangles[regular, :12])) and np.all(triangles[regular, 3] > 0)
    assert np.allclose(np.linalg.norm(triangles[regular, 0:3], axis=1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(triangles[regular, 8:11], axis=1), 1.0, atol=1e-6)

    # every light, in model order: corners, material, and the constants of triangleSample and sampleLightsTerm
    for row, prim in zip(lights[:-1], emissive):
        assert (row[0], row[1]) == (0.0, float(prim))
        record = row[2:].reshape(4, 4)
        assert np.array_equal(_bits(record[0:3, 0:3]), _bits(positions[indices[prim]]))
        assert int(_bits(record[0, 3:4])[0]) == materials[prim]
        assert _bits(record[1, 3:4])[0] == _bits(triangles[prim, 3:4])[0]        # area
        assert _bits(record[2, 3:4])[0] == _bits(triangles[prim, 5:6])[0]        # invPDF
        assert np.array_equal(_bits(record[3, 0:3]), _bits(triangles[prim, 0:3]))   # normal
        assert _bits(record[3, 3:4])[0] == _bits(triangles[prim, 6:7])[0]        # 1 / invPDF
    # invPDF is the area times the light count
    light_count = np.float32(lights.shape[0])
    first = emissive[0]
    assert lights[0, 2 + 11] == np.float32(triangles[first, 3] * (np.float32(1) / (np.float32(1) / light_count)))
    # the sphere light's record is empty
    assert lights[-1, 0] == 1.0 and not np.any(_bits(lights[-1, 2:]))
    # the zero-area emitters: the old code's area 0, 1 / 0 and 0 / 0, and the very same bits in the records (compared above)
    for prim in emissive[-2:]:
        assert triangles[prim, 3] == 0.0 and np.isinf(triangles[prim, 4]) and np.isinf(triangles[prim, 6])
        assert np.all(np.isnan(triangles[prim, 0:3])) and np.all(np.isnan(triangles[prim, 8:11]))


def _lamp_scene():
    from scene_builder import BuiltScene
    built = BuiltScene(48, 48, (0.0, 1.0, 6.0), (0, 0, 0), fov_degrees=45.0)
    grey = built.material(diffuse=(0.7, 0.6, 0.5))
    lamp = built.material(diffuse=(0, 0, 0), emit=(12, 12, 12))
    # a floor of 10 x 10 cells (200 triangles: the scene has a tree, which a refit needs), a box on it, a lamp above
    n = 10
    xs = np.linspace(-3, 3, n + 1)
    vertices = [(x, -1.0 + 0.05 * np.sin(3 * x + z), z) for z in xs for x in xs]
    faces = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            faces += [(a, a + n + 1, a + 1), (a + 1, a + n + 1, a + n + 2)]
    built.mesh(vertices, faces, grey)
    built.box((-0.5, -1.0, -0.5), (0.5, 0.0, 0.5), grey)
    first_lamp_vertex = len(built.positions)
    built.mesh([(-0.6, 2.0, -0.6), (0.6, 2.0, -0.6), (0.6, 2.0, 0.6), (-0.6, 2.0, 0.6)], [(0, 1, 2), (0, 2, 3)], lamp)
    return built, first_lamp_vertex


def test_a_refitted_emitter_renders_like_a_fresh_scene_at_the_new_position():
    from pathed_amd.integrator import HipScene
    built, first_lamp_vertex = _lamp_scene()
    desc = built.finish()
    n_vertices = desc.contents.n_vertices
    live = np.ctypeslib.as_array(desc.contents.positions, shape=(n_vertices, 3))   # a VIEW of the descriptor's vertex array
    original = live.copy()
    gpu = HipScene(desc, device=0, refittable=1)
    before = gpu.render(5, 0, 8, 0, 6)
    assert before.sum() > 0

    moved = original.copy()
    lamp = moved[first_lamp_vertex:first_lamp_vertex + 4]
    lamp[:] = lamp * np.float32(1.7) + np.array([1.1, -0.4, 0.3], dtype=np.float32)   # elsewhere, and larger: another area, another pdf
    lamp[1, 1] += np.float32(0.5)                                                     # tilted: another normal
    gpu.refit(moved)
    live[:] = moved
    fresh = HipScene(desc, device=0)
    after = gpu.render(5, 0, 8, 0, 6)
    assert not np.array_equal(after, before)
    assert np.array_equal(_bits(after), _bits(fresh.render(5, 0, 8, 0, 6)))
    n_triangles = desc.contents.n_triangles
    refit_triangles, refit_lights = gpu.light_records(n_triangles, n_triangles)
    fresh_triangles, fresh_lights = fresh.light_records(n_triangles, n_triangles)
    assert refit_lights.shape[0] == 2
    assert np.array_equal(_bits(refit_lights), _bits(fresh_lights)) and np.array_equal(_bits(refit_triangles), _bits(fresh_triangles))
    assert np.array_equal(_bits(refit_lights[0, 2:5]), _bits(moved[first_lamp_vertex]))
