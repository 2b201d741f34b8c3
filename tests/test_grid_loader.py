"""Loading voxel-grid media: the .vol reader (pathed_amd/host/scene_loader.cpp: readVolFile, after the reference's
src/vol_parser.cpp, with the checks it lacks) and "heterogeneous" entries of a scene file's "media"
(src/scene_parser.cpp:202-220).  No GPU: the scene is loaded by the C++ host, which is also how Python loads scenes
(pathed_amd.scene.LoadedScene); the grid it hands on is compared with what this file wrote and with a float64 restatement
of the reference's parseTransform."""
import json
import struct

import numpy as np
import pytest

from pathed_amd import _capi
from pathed_amd.scene import LoadedScene

SCENE = {
    "sensor": {"lookAt": {"origin": ["0", "1", "6"], "target": ["0", "1", "0"], "up": ["0", "1", "0"]}, "fov": "30"},
    "media": [
        {"name": "thin", "type": "homogeneous", "sigma_t": ["0.5", "0.5", "0.5"], "sigma_s": ["0.25", "0.25", "0.25"]},
        {"name": "smoke", "type": "heterogeneous", "filename": "plume.vol", "albedo": "0.75", "scale": "2.5",
         "transform": {"scale": ["2", "1", "0.5"], "rotate": ["10", "25", "-40"], "translate": ["0.5", "1.0", "-0.25"]}},
        {"name": "plain", "type": "heterogeneous", "filename": "plume.vol", "albedo": "0.5"},
    ],
    "models": [
        {"type": "sphere", "radius": "0.5", "center": ["0", "1", "0"], "internal_medium": "smoke", "bsdf": {"type": "passthrough"}},
        {"type": "sphere", "radius": "0.25", "center": ["1", "1", "0"], "internal_medium": "plain", "bsdf": {"type": "passthrough"}},
        {"type": "sphere", "radius": "0.25", "center": ["-1", "1", "0"], "internal_medium": "thin", "bsdf": {"type": "passthrough"}},
    ],
}
BOUNDS = (-0.5, -0.25, -1.0, 0.75, 0.5, 1.5)


def vol_bytes(data, bounds=BOUNDS, header=b"VOL", channels=1):
    """the layout vol_parser.cpp reads; data: (cells_z, cells_y, cells_x)"""
    data = np.ascontiguousarray(data, dtype="<f4")
    return (header + struct.pack("<B", 3) + struct.pack("<5I", 1, data.shape[2], data.shape[1], data.shape[0], channels)
            + struct.pack("<6f", *bounds) + data.tobytes())


def write_scene(root, vol):
    (root / "plume.vol").write_bytes(vol)
    (root / "scene.json").write_text(json.dumps(SCENE))
    return str(root)


def grid_data():
    return np.random.default_rng(6).uniform(0.0, 2.0, (5, 4, 3)).astype(np.float32)


def reference_transform(entry):
    """parseTransform, src/scene_parser.cpp:690-793, in float64: scale, then rotate z, x, y (y negated), then translate"""
    sx, sy, sz = [float(v) for v in entry.get("scale", ["1", "1", "1"])]
    rx, ry, rz = [np.radians(float(v)) for v in entry.get("rotate", ["0", "0", "0"])]
    ry = -ry
    tx, ty, tz = [float(v) for v in entry.get("translate", ["0", "0", "0"])]

    def rotation(axis, angle):
        c, s = np.cos(angle), np.sin(angle)
        m = np.eye(4)
        i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    translate = np.eye(4)
    translate[:3, 3] = (tx, ty, tz)
    return translate @ rotation("y", ry) @ rotation("x", rx) @ rotation("z", rz) @ np.diag([sx, sy, sz, 1.0])


def test_a_scene_with_a_heterogeneous_medium_loads(tmp_path):
    data = grid_data()
    scene = LoadedScene("scene.json", 16, 12, asset_root=write_scene(tmp_path, vol_bytes(data)))
    desc = scene.desc.contents
    # every medium has a slot, in file order; the grids' slots are placeholders with zero sigmas
    assert desc.n_media == 3
    assert list(desc.media[0].sigma_t) == [0.5, 0.5, 0.5] and list(desc.media[0].sigma_s) == [0.25, 0.25, 0.25]
    assert list(desc.media[1].sigma_t) == [0.0, 0.0, 0.0] and list(desc.media[2].sigma_t) == [0.0, 0.0, 0.0]
    assert [desc.geoms[i].medium for i in range(3)] == [1, 2, 0]
    assert [slot for slot, _ in scene.grids] == [1, 2]

    slot, grid = scene.grids[0]
    assert grid.struct_size == __import__("ctypes").sizeof(_capi.PathedGridMedium)
    assert (grid.cells_x, grid.cells_y, grid.cells_z) == (3, 4, 5)
    assert tuple(grid.bounds) == BOUNDS
    assert np.array_equal(np.ctypeslib.as_array(grid.data, shape=(5, 4, 3)), data)
    assert grid.albedo == np.float32(0.75) and grid.scale == 2.5
    # the medium gets the INVERSE of the parsed transform (VolParser::parse passes transform.inversed())
    model_to_world = reference_transform(SCENE["media"][1]["transform"])
    assert np.allclose(np.array(grid.model_to_world).reshape(4, 4), model_to_world, rtol=0, atol=2e-6)
    assert np.allclose(np.array(grid.world_to_model).reshape(4, 4), np.linalg.inv(model_to_world), rtol=0, atol=2e-6)
    product = np.array(grid.world_to_model, dtype=np.float64).reshape(4, 4) @ np.array(grid.model_to_world, dtype=np.float64).reshape(4, 4)
    assert np.allclose(product, np.eye(4), rtol=0, atol=2e-6)

    _, plain = scene.grids[1]   # "scale" defaults to 1, "transform" to the identity
    assert plain.albedo == 0.5 and plain.scale == 1.0
    assert np.array_equal(np.array(plain.world_to_model).reshape(4, 4), np.eye(4)) and np.array_equal(np.array(plain.model_to_world).reshape(4, 4), np.eye(4))
    assert np.array_equal(np.ctypeslib.as_array(plain.data, shape=(5, 4, 3)), data)


@pytest.mark.parametrize("what, vol, message", [
    ("header", vol_bytes(grid_data(), header=b"VOX"), 'does not start with "VOL"'),
    ("channels", vol_bytes(grid_data(), channels=3), "has 3 channels"),
    ("truncated", vol_bytes(grid_data())[:-8], "288 bytes"),
    ("too long", vol_bytes(grid_data()) + b"\0\0\0\0", "288 bytes"),
    ("short header", vol_bytes(grid_data())[:20], "shorter than the 48-byte header"),
])
def test_a_bad_vol_file_is_refused_with_a_message(tmp_path, what, vol, message):
    with pytest.raises(RuntimeError) as error:
        LoadedScene("scene.json", 16, 12, asset_root=write_scene(tmp_path, vol))
    assert "plume.vol" in str(error.value) and message in str(error.value), str(error.value)


def test_a_missing_vol_file_or_key_is_refused(tmp_path):
    (tmp_path / "scene.json").write_text(json.dumps(SCENE))
    with pytest.raises(RuntimeError, match="cannot open"):
        LoadedScene("scene.json", 16, 12, asset_root=str(tmp_path))
    broken = json.loads(json.dumps(SCENE))
    del broken["media"][1]["albedo"]
    (tmp_path / "plume.vol").write_bytes(vol_bytes(grid_data()))
    (tmp_path / "scene.json").write_text(json.dumps(broken))
    with pytest.raises(RuntimeError, match="albedo"):
        LoadedScene("scene.json", 16, 12, asset_root=str(tmp_path))


def test_the_shipped_smoke_scene_loads():
    """scenes/cornell-smoke.json with the synthetic plume of tools/make_assets.py"""
    scene = LoadedScene("scenes/cornell-smoke.json", 32, 32)
    (slot, grid), = scene.grids
    assert slot == 0 and (grid.cells_x, grid.cells_y, grid.cells_z) == (32, 32, 32)
    data = np.ctypeslib.as_array(grid.data, shape=(32, 32, 32))
    assert data.min() == 0.0 and 0.5 < data.max() <= 1.0 and 0.1 < (data > 0.05).mean() < 0.5
    assert data[0].max() == data[-1].max() == data[:, 0].max() == data[:, -1].max() == data[:, :, 0].max() == data[:, :, -1].max() == 0.0
