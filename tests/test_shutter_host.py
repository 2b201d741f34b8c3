"""The shutter over instanced scenes (include/pathed_hip.h: pathed_hip_scene_set_instance_motion; DESIGN.md section 4.6d
"Shutter"), the part that needs no GPU.  tests/shutter_host.cpp includes pathed_amd/csrc/instances.h alone and is built
twice, plainly and with -fsanitize=address,undefined, and run as its own program; every comparison runs on both builds.

1. interpolateTransform and sampleTime are pathed_amd.instances.interpolate_transforms / sample_time, bit for bit
2. the stream at the time's dimension is not the stream of any dimension a render draws
3. movingPlacementBox is the numpy mirror's box, and it holds every corner of the prototype's box at every time of the shutter
4. the entry points are declared, bound and exported; the ABI version stays
5. the per-sample test's condition holds by the CPU oracle alone: the second placement set changes the first hit of at
   least a quarter of the pixels
6. the loader reads "transform_close", the job "shutter"; the three refusals by name; the moving field's files
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pathed_amd import _capi
from pathed_amd import instances as I

import instances_scene as S
import shutter_scene as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pathed_hip_scene_set_instance_motion", "pathed_hip_scene_set_instance_motion_device", "pathed_hip_trace_timed")


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    compiler = shutil.which("g++") or shutil.which("c++")
    if compiler is None:
        pytest.skip("no host compiler")
    folder = tmp_path_factory.mktemp("shutter_" + request.param)
    binary = folder / "shutter_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    built = subprocess.run([compiler, "-std=c++17", "-O2", "-ffp-contract=off", "-march=x86-64-v3", "-Wall", "-Wextra"] + flags
                           + ["-iquote", os.path.join(ROOT, "pathed_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                              os.path.join(ROOT, "tests", "shutter_host.cpp"), "-o", str(binary), "-lpthread"], capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-2000:]

    def run(what, records):
        result = subprocess.run([str(binary), what], input=np.ascontiguousarray(records).tobytes(), capture_output=True, timeout=120)
        assert result.returncode == 0, result.stderr[-2000:]
        return np.frombuffer(result.stdout, dtype=np.float32)
    return run


def random_transforms(rng, count):
    """rotations, shears and mirrors over seven decades of scale, translations from 1e-2 to 1e4"""
    out = np.zeros((count, 12), dtype=np.float32)
    for k in range(count):
        out[k] = S.affine(rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3), rng.normal(size=3) * 10.0 ** rng.uniform(-2, 4))
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the rule

def test_interpolate_transform_is_the_numpy_mirror(program):
    """10 000 random cases.  t = 0 and t = 1 (a fifth of the cases each) give the endpoints' bits apart from the sign of a
    zero: (1 * a) + (0 * b) is +0 where a is -0 and b is positive or +0."""
    rng = np.random.default_rng(7)
    n = 10000
    a, b = random_transforms(rng, n), random_transforms(rng, n)
    a[::50, 3] = -0.0          # signed zeros at both ends
    b[::75, 7] = 0.0
    t = rng.random(n).astype(np.float32)
    t[0::5], t[1::5] = 0.0, 1.0
    records = np.concatenate([a, b, t[:, None]], axis=1).astype(np.float32)
    out = program("interp", records).reshape(n, 12)
    expected = np.stack([I.interpolate_transforms(a[k], b[k], t[k]) for k in range(n)])
    assert np.array_equal(bits(out), bits(expected))
    assert np.array_equal(bits(I.interpolate_transforms(a, b, np.float32(0.25))), bits(np.stack([I.interpolate_transforms(a[k], b[k], 0.25) for k in range(n)])))
    # the endpoints: equal as numbers everywhere, equal in bits wherever the endpoint is not a zero
    for end, rows in ((a, slice(0, None, 5)), (b, slice(1, None, 5))):
        assert np.array_equal(out[rows], end[rows])
        nonzero = end[rows] != 0
        assert np.array_equal(bits(out[rows])[nonzero], bits(end[rows])[nonzero])
    assert np.signbit(a[0, 3]) and not np.signbit(out[0, 3])   # ... and the sign of a zero is indeed not kept


def test_sample_time_is_the_numpy_mirror(program):
    rng = np.random.default_rng(8)
    n = 10000
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    seeds[:4] = [0, 1, 2 ** 32, 2 ** 64 - 1]
    pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sample = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    pixel[:3], sample[:3] = [0, 2 ** 32 - 1, 7], [0, 2 ** 32 - 1, 2 ** 31]
    shutter = np.sort(rng.random((n, 2)).astype(np.float32), axis=1)
    shutter[0::7] = (0.0, 1.0)
    shutter[1::7, 1] = shutter[1::7, 0]          # a frozen shutter
    records = np.zeros((n, 6), dtype=np.uint32)
    records[:, 0], records[:, 1] = (seeds & np.uint64(0xFFFFFFFF)).astype(np.uint32), (seeds >> np.uint64(32)).astype(np.uint32)
    records[:, 2], records[:, 3] = pixel, sample
    records[:, 4:6] = bits(shutter)
    out = program("time", records)
    expected = np.array([I.sample_time(int(seeds[k]), pixel[k], sample[k], shutter[k, 0], shutter[k, 1]) for k in range(n)], dtype=np.float32)
    assert np.array_equal(bits(out), bits(expected))
    assert np.all((out >= shutter[:, 0]) & (out <= shutter[:, 1]))
    assert np.array_equal(out[1::7], shutter[1::7, 0])
    # the vectorised form the GPU tests use
    assert np.array_equal(bits(I.sample_time(9, pixel[:64], sample[:64], 0.25, 0.75)),
                          bits(np.array([I.sample_time(9, pixel[k], sample[k], 0.25, 0.75) for k in range(64)], dtype=np.float32)))


def test_the_time_dimension_is_nobodys(program):
    """u at dimension 0xFFFFFFFF against dimensions 0 and 1 (the camera jitter) and every vertex row up to vertex 12
    (vertexBase(v) = 2 + 8 (v - 1), eight dimensions each), on a few keys: another number everywhere, by the program's stream
    and by numpy's, which are the same stream."""
    assert I.DIM_TIME == 0xFFFFFFFF and I.DIM_TIME > 2 + 8 * 12
    drawn = np.arange(0, 2 + 8 * 12, dtype=np.uint32)
    for seed, pixel, sample in ((1, 0, 0), (5, 1535, 3), (2 ** 40 + 17, 48 * 32 - 1, 255), (2 ** 64 - 1, 2 ** 31, 2 ** 20)):
        dimensions = np.concatenate([drawn, np.array([I.DIM_TIME], dtype=np.uint32)])
        records = np.zeros((len(dimensions), 5), dtype=np.uint32)
        records[:, 0], records[:, 1], records[:, 2], records[:, 3], records[:, 4] = seed & 0xFFFFFFFF, seed >> 32, pixel, sample, dimensions
        out = program("stream", records)
        assert np.array_equal(bits(out), bits(I.stream_value(seed, pixel, sample, dimensions)))
        assert not np.any(out[:-1] == out[-1]), (seed, pixel, sample)
        assert np.array_equal(bits(out[-1:]), bits(I.sample_time(seed, pixel, sample, 0.0, 1.0).reshape(1)))


# ------------------------------------------------------------------------------------------------------------- 3. the box

def test_the_moving_box_holds_the_placement_at_every_time(program):
    """200 random endpoint pairs over small and large coordinates, the placements of the GPU tests and a placement 1 000 units
    away: the box is numpy's bit for bit, and it holds the float32 image of all eight corners of the prototype's box under
    M(t) at 257 times of the shutter, both ends included."""
    rng = np.random.default_rng(9)
    pairs = [(a, b) for a, b in zip(random_transforms(rng, 200), random_transforms(rng, 200))]
    pairs += list(zip(M.transforms(M.OPEN_PLACEMENTS), M.transforms(M.CLOSE_PLACEMENTS)))
    pairs.append((S.affine(np.eye(3), (1000.0, -1000.0, 1000.0)), S.affine(1.5 * S.rotation((1, 1, 0), 170.0), (1003.0, -998.0, 1001.0))))
    pairs.append((S.affine(np.eye(3)), S.affine(S.rotation((0, 0, 1), 180.0))))   # singular at t = 0.5: the box does not mind
    protos = [I.prototype_box(S.icosphere(centre, radius, subdivisions=1)[0])
              for centre, radius in (((3.0, 2.0, 1.0), 1.0), ((0.0, 0.0, 0.0), 1.0), ((500.0, -0.25, 1e-3), 0.01))]
    shutters = [(0.0, 1.0), (0.25, 0.75), (0.5, 0.5), (0.0, 0.0), (0.9, 1.0)]
    cases = [(a, b, shutters[k % len(shutters)], protos[k % len(protos)]) for k, (a, b) in enumerate(pairs)]
    records = np.stack([np.concatenate([a, b, np.float32(shutter), lo, hi]) for a, b, shutter, (lo, hi) in cases]).astype(np.float32)
    out = program("box", records).reshape(len(cases), 6)
    for (a, b, (shutter_open, shutter_close), (proto_lo, proto_hi)), row in zip(cases, out):
        lo, hi = I.moving_placement_box(a, b, shutter_open, shutter_close, proto_lo, proto_hi)
        assert np.array_equal(bits(lo), bits(row[0:3])) and np.array_equal(bits(hi), bits(row[3:6])), (a, b)
        corners = np.array([[(proto_hi if corner & (1 << axis) else proto_lo)[axis] for axis in range(3)] for corner in range(8)], dtype=np.float32)
        times = (np.float32(shutter_open) + (np.float32(shutter_close) - np.float32(shutter_open)) * np.linspace(0.0, 1.0, 257).astype(np.float32)).astype(np.float32)
        times[-1] = shutter_close
        for t in times:
            world = I.flatten_points(I.interpolate_transforms(a, b, t), corners)
            assert np.all(world >= lo) and np.all(world <= hi), (a, b, t)
        # ... and the static boxes of both ends, whose pads the walk of a static scene relies on
        for t in (shutter_open, shutter_close):
            end_lo, end_hi = I.placement_box(I.interpolate_transforms(a, b, t), proto_lo, proto_hi)
            assert np.all(end_lo >= lo) and np.all(end_hi <= hi)


# ------------------------------------------------------------------------------------------------------------- 4. the ABI

def test_the_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pathed_hip.h")).read()
    assert re.search(r"int pathed_hip_scene_set_instance_motion\(PathedScene \*scene, const float \*transforms_close, uint32_t n_instances,\s*"
                     r"float shutter_open, float shutter_close, float \*device_ms\);", header)
    assert re.search(r"int pathed_hip_scene_set_instance_motion_device\(PathedScene \*scene, const float \*d_transforms_close, uint32_t n_instances,\s*"
                     r"float shutter_open, float shutter_close, float \*device_ms\);", header)
    assert re.search(r"int pathed_hip_trace_timed\(PathedScene \*scene, const float \*rays, const float \*times, size_t n,\s*int any_hit, void \*hits\);", header)
    assert re.search(r"#define PATHED_ABI_VERSION 4\b", header)   # functions only, no struct changes: the version stays
    for phrase in ("SKIPS that placement", "0xFFFFFFFF", "does not move"):   # the rule is stated where the functions are declared
        assert phrase in header, phrase
    lib = C.CDLL(_capi.hip_library_path())
    for name in NEW_SYMBOLS:
        assert name in _capi.HIP_SYMBOLS and hasattr(lib, name), name
    blob = open(_capi.hip_library_path(), "rb").read()
    for name in (b"24k_trace_instanced_motionILi8ELb0E", b"24k_shade_instanced_motionILb1ELb0E", b"29k_trace_rays_instanced_motionILi22E", b"14k_motion_boxes"):
        assert name in blob, name


# ----------------------------------------------------------------------------------------- 5. the per-sample test's condition

def test_the_second_placement_set_changes_a_quarter_of_the_first_hits():
    """by the CPU oracle's trace over the flattened scenes of t = 0 and t = 1, at the resolutions the GPU tests render"""
    for width, height in ((8, 6), (48, 32)):
        assert M.first_hit_change(width, height) >= 0.25
    a, b = M.transforms(M.OPEN_PLACEMENTS), M.transforms(M.CLOSE_PLACEMENTS)
    moving = [k for k in range(len(a)) if not np.array_equal(bits(a[k]), bits(b[k]))]
    assert moving == [k for k in range(len(a)) if k != M.STILL]
    # the still placement under the plain interpolation at the frozen-shutter test's times: its own bits, so the static scenes
    # of those times are interpolate_transforms(a, b, t) itself, entry for entry
    for t in (0.0, 0.25, 1.0):
        assert np.array_equal(bits(I.interpolate_transforms(a, b, t)), bits(M.transforms(M.placements_at(t)))), t


# ------------------------------------------------------------------------------------------------- 6. scene files and job files

def test_the_loader_reads_transform_close(tmp_path):
    """"transform_close" on a top-level "instanced" model: 16 numbers, column-major like "transform".  What the outer placement
    holds inside moves with it (the composition in double, rounded once, as at time 0); a placement without the key carries its
    transform twice; a scene where nothing moves carries nothing."""
    from pathed_amd.scene import LoadedScene
    import test_instances_host as H
    floor = H.quad(["0.5", "0.5", "0.5"], ("0", "0", "0"), scale=("10", "1", "10"))
    leaf = {"type": "instance", "name": "leaf", "models": [H.quad(["0.2", "0.7", "0.2"], ("0.5", "2", "0.5"))]}
    branch = {"type": "instance", "name": "branch", "models": [H.quad(["0.6", "0.4", "0.2"], ("1", "1", "1")),
                                                              {"type": "instanced", "instance_name": "leaf", "transform": H.column_major(*H.INNER)}]}
    close = (H.turn(110.0) @ np.diag([1.5, 0.5, 2.0]), (2.0, 3.5, -1.0))
    models = [floor, leaf, branch,
              {"type": "instanced", "instance_name": "branch", "transform": H.column_major(*H.OUTER[0]), "transform_close": H.column_major(*close)},
              {"type": "instanced", "instance_name": "branch", "transform": H.column_major(*H.OUTER[1])}]
    scene = LoadedScene(H.scene_file(tmp_path, models=models), 32, 24, "")
    assert [prototype for prototype, _ in scene.instances] == [1, 0, 1, 0]
    assert scene.instances_close is not None and scene.instances_close.shape == (4, 12)
    linear, translation = H.as_float32(*close)
    inner_linear, inner_translation = H.as_float32(*H.INNER)
    assert np.array_equal(bits(scene.instances_close[0]), bits(np.hstack([linear, translation[:, None]]).astype(np.float32).reshape(12)))
    composed = np.hstack([linear @ inner_linear, (linear @ inner_translation + translation)[:, None]]).astype(np.float32).reshape(12)
    assert np.array_equal(bits(scene.instances_close[1]), bits(composed))
    for k in (2, 3):
        assert np.array_equal(bits(scene.instances_close[k]), bits(np.asarray(scene.instances[k][1], dtype=np.float32)))
    still = LoadedScene(H.scene_file(tmp_path, models=models[:3] + [dict(models[3], transform_close=None)] + models[4:]), 32, 24, "")
    assert still.instances_close is None and len(still.instances) == 4

    def refused(bad, *words):
        with pytest.raises(RuntimeError) as caught:
            LoadedScene(H.scene_file(tmp_path, models=bad), 16, 16, "")
        for word in words:
            assert word in str(caught.value), str(caught.value)

    # on a nested "instanced" model
    nested = {"type": "instance", "name": "branch", "models": [
        {"type": "instanced", "instance_name": "leaf", "transform": H.column_major(*H.INNER), "transform_close": H.column_major(*close)}]}
    refused([floor, leaf, nested, models[4]], "transform_close", "nested")
    # on a placement of a prototype that holds an emitter, directly or inside
    lamp = {"type": "instance", "name": "lamp", "models": [H.quad(["0.6", "0.4", "0.2"], ("1", "1", "1")), H.quad(["0", "0", "0"], ("1", "3", "1"), emit=["5", "4", "3"])]}
    moving_lamp = {"type": "instanced", "instance_name": "lamp", "transform": H.column_major(*H.OUTER[0]), "transform_close": H.column_major(*close)}
    refused([floor, lamp, moving_lamp], "transform_close", "emitter", "lamp")
    LoadedScene(H.scene_file(tmp_path, models=[floor, lamp, dict(moving_lamp, transform_close=None)]), 16, 16, "")   # ... which may stand still
    refused([floor, leaf, dict(models[4], instance_name="leaf", transform_close=H.column_major(*close)[:12])], "transform_close", "16 numbers")


@pytest.mark.parametrize("moves, shutter, words", [
    (False, [0.0, 1.0], ["shutter", "nothing moves"]),
    (True, [0.5], ["shutter", "[open, close]"]),
    (True, [0.6, 0.5], ["shutter", "0 <= open <= close <= 1"]),
    (True, [0.0, 1.5], ["shutter", "0 <= open <= close <= 1"]),
    (True, "open", ["shutter", "[open, close]"]),
])
def test_the_job_runner_refuses_a_shutter_by_name(tmp_path, moves, shutter, words):
    """"shutter" on a scene where nothing moves, or outside its rule, stops a job in the C++ host once the scene is read: before a
    tree is built or a device is touched (no GPU is needed to get this far)."""
    import json
    import test_instances_host as H
    floor = H.quad(["0.5", "0.5", "0.5"], ("0", "0", "0"), scale=("10", "1", "10"))
    leaf = {"type": "instance", "name": "leaf", "models": [H.quad(["0.2", "0.7", "0.2"], ("0.5", "2", "0.5"))]}
    placed = {"type": "instanced", "instance_name": "leaf", "transform": H.column_major(*H.OUTER[0])}
    if moves:
        placed["transform_close"] = H.column_major(*H.OUTER[1])
    job = json.load(open(os.path.join(ROOT, "jobs", "cornell-c1.json")))
    job.update({"scene": H.scene_file(tmp_path, models=[floor, leaf, placed]), "output_directory": str(tmp_path / "out"), "width": 16, "height": 16, "spp": 1,
                "shutter": shutter})
    job_path = tmp_path / "job.json"
    job_path.write_text(json.dumps(job))
    result = subprocess.run([os.path.join(ROOT, "pathed_amd", "bin", "pathed"), str(job_path), ""], capture_output=True, text=True, timeout=120)
    assert result.returncode != 0
    for word in words:
        assert word in result.stderr + result.stdout, result.stderr + result.stdout


def test_the_job_and_scene_files_of_the_moving_field():
    import json
    job = json.load(open(os.path.join(ROOT, "jobs", "instances-field-motion.json")))
    still = json.load(open(os.path.join(ROOT, "jobs", "instances-field.json")))
    assert job["scene"] == "scenes/instances-field-motion.json" and job["shutter"] == [0.0, 1.0]
    assert {k: v for k, v in job.items() if k not in ("scene", "shutter", "output_directory")} == {k: v for k, v in still.items() if k not in ("scene", "output_directory")}
    scene = json.load(open(os.path.join(ROOT, job["scene"])))
    field = json.load(open(os.path.join(ROOT, still["scene"])))
    assert len(scene["models"]) == len(field["models"])
    movers = [k for k, model in enumerate(scene["models"]) if "transform_close" in model]
    assert 3 <= len(movers) <= 8 and all(scene["models"][k]["type"] == "instanced" and len(scene["models"][k]["transform_close"]) == 16 for k in movers)
    for k, (mine, theirs) in enumerate(zip(scene["models"], field["models"])):
        assert {key: value for key, value in mine.items() if key != "transform_close"} == theirs, k
