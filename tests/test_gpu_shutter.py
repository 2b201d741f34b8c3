"""The shutter over instanced scenes (include/pathed_hip.h: pathed_hip_scene_set_instance_motion, pathed_hip_trace_timed;
DESIGN.md section 4.6d "Shutter"; instance_motion.h: k_trace_instanced_motion, k_shade_instanced_motion,
k_trace_rays_instanced_motion, k_motion_boxes).  The yardstick throughout is a STATIC instanced scene created with the
placements of one time, pathed_amd.instances.interpolate_transforms of the two sets: a scene with motion answers with its bits
for every ray and every sample of that time.

1. frozen shutter     [t, t] is the static scene of t: moments at bounces 0..3
2. timed hits         trace_timed, eight times: closest and any hit of the static scene of each time
3. per-sample times   every (pixel, sample) of a 2 spp render is the static scene of ITS time, instances.sample_time
4. clear / replace    clear_instance_motion, set_instance_transforms and rebuild_top on a scene with motion; the device entry
5. stack rows         every rung, plain and counting
6. lists              render_pixels over 1, 65 and all pixels
7. two calls are one  3 + 5 samples onto a device buffer
8. refusals           by code and by word, nothing launched
9. executable         a job with "transform_close" through both launchers, resumed, and with a frozen "shutter"
"""
import ctypes as C

import numpy as np
import pytest

from pathed_amd import flatten_instances
from pathed_amd import instances as I
from pathed_amd.integrator import HipScene, PathedError, _check

import instances_scene as S
import shutter_scene as M
from test_gpu_instances import instanced_stack_rungs

pytestmark = pytest.mark.gpu

SIZE = (48, 32)
UNSUPPORTED, INVALID = -4, -1
CLOSE = M.transforms(M.CLOSE_PLACEMENTS)
TIMES = [0.0, 1.0, 0.125, 0.3, 0.5, 0.62, 0.875, 0.99]


def bits(array):
    return np.ascontiguousarray(array).view(np.uint32)


class Scene:
    """An instanced scene on the GPU with what it was made from."""

    def __init__(self, placements, size=SIZE, **options):
        self.built, self.pointer, self.prototypes, self.placements = S.build(placements, *size)
        self.gpu = HipScene(self.pointer, device=0, prototypes=self.prototypes, instances=self.placements, **options)

    def flat(self):
        return flatten_instances(self.pointer, None, self.gpu.instance_set)


def moving_scene(size=SIZE, shutter=(0.0, 1.0), **options):
    scene = Scene(M.OPEN_PLACEMENTS, size, **options)
    scene.ms = scene.gpu.set_instance_motion(CLOSE, shutter=shutter)
    return scene


def moments(gpu):
    return [gpu.render_moments(5, 0, 4, 0, last) for last in (0, 1, 2, 3)]


def assert_moments_equal(mine, theirs):
    for last, ((sums, squares), (expected_sums, expected_squares)) in enumerate(zip(mine, theirs)):
        assert last == 0 or float(expected_sums.sum()) > 0.0
        assert np.array_equal(bits(sums), bits(expected_sums)), last
        assert np.array_equal(bits(squares), bits(expected_squares)), last


@pytest.fixture(scope="module")
def static_moments():
    """the moments of the static scenes of t = 0, 0.25 and 1, rendered once"""
    out = {}
    for t in (0.0, 0.25, 1.0):
        scene = Scene(M.placements_at(t))
        out[t] = moments(scene.gpu)
        assert scene.gpu.stats()["path_kernel"] == 10
    return out


@pytest.fixture(scope="module")
def moving():
    return moving_scene()


@pytest.fixture(scope="module")
def moving_moments(moving):
    """the full render of the open shutter, (sums, squares) at bounces 0..3: what the list pass is judged against"""
    return moving.gpu.render_moments(5, 0, 4, 0, 3)


# ----------------------------------------------------------------------------------------------------------- 1. frozen shutter

@pytest.mark.parametrize("t", [0.0, 0.25, 1.0])
def test_a_frozen_shutter_is_the_static_scene(static_moments, t):
    scene = moving_scene(shutter=(t, t))
    assert scene.ms > 0.0
    assert_moments_equal(moments(scene.gpu), static_moments[t])
    assert scene.gpu.stats()["path_kernel"] == 11
    # ... and the three times are three images
    assert not np.array_equal(bits(static_moments[0.0][3][0]), bits(static_moments[1.0][3][0]))
    assert not np.array_equal(bits(static_moments[0.0][3][0]), bits(static_moments[0.25][3][0]))


# --------------------------------------------------------------------------------------------------------------- 2. timed hits

def test_timed_hits_are_the_static_scenes_of_their_times(moving):
    """6 000 rays, 750 at each of eight times (both ends and six in between), aimed at the flattened triangles of their own time;
    as many any-hit segments that end at half or at twice the target's distance"""
    per_time = 6000 // len(TIMES)
    closest, shadow, times, expected, expected_occluded, bases = [], [], [], [], [], None
    for k, t in enumerate(TIMES):
        static = Scene(M.placements_at(t))
        flat = static.flat()
        bases = flat.bases
        rays = S.general_rays(flat, per_time, 40 + k)
        segments = S.general_rays(flat, per_time, 60 + k)
        segments[:, 7] = np.where(np.arange(per_time) % 2 == 1, 2.0, 0.5).astype(np.float32)
        closest.append(rays)
        shadow.append(segments)
        times.append(np.full(per_time, t, dtype=np.float32))
        expected.append(static.gpu.trace(rays))
        expected_occluded.append(static.gpu.trace(segments, any_hit=True))
    closest, shadow, times = np.concatenate(closest), np.concatenate(shadow), np.concatenate(times)
    expected, expected_occluded = np.concatenate(expected), np.concatenate(expected_occluded)
    # interleaved, so that the lanes of a wave hold different times
    order = np.random.default_rng(3).permutation(len(times))
    hits = moving.gpu.trace_timed(closest[order], times[order])
    occluded = moving.gpu.trace_timed(shadow[order], times[order], any_hit=True)
    prim = bits(expected[:, 3]).view(np.int32)
    assert (prim >= 0).mean() > 0.5
    for k in range(len(M.OPEN_PLACEMENTS)):
        assert ((prim >= bases[k]) & (prim < bases[k + 1])).sum() > 50, k
    for t in TIMES:
        at = times[order] == np.float32(t)
        assert np.array_equal(bits(hits[at]), bits(expected[order][at])), t
        assert np.array_equal(occluded[at], expected_occluded[order][at]), t
    assert 0.05 < expected_occluded.mean() < 0.95
    # the time matters: the same rays at time 0 are other hits
    assert not np.array_equal(bits(moving.gpu.trace_timed(closest, np.zeros(len(closest), dtype=np.float32))), bits(expected))


# --------------------------------------------------------------------------------------------------------- 3. per-sample times

def test_every_sample_sees_the_placements_at_its_own_time():
    """8 x 6 pixels x 2 spp, shutter [0, 1], bounces 0..2: for each of the 96 (pixel, sample) a static scene created at
    sample_time(seed, pixel, sample) renders that one sample; a pixel's two values are added in sample order in float32.  That
    the time matters here is checked without a GPU (test_shutter_host.py: the second placement set changes the first hit of
    more than a quarter of these pixels)."""
    width, height, seed, spp = 8, 6, 5, 2
    scene = moving_scene((width, height))
    image = scene.gpu.render(seed, 0, spp, 0, 2)
    assert scene.gpu.stats()["path_kernel"] == 11
    expected = np.zeros((height * width, 3), dtype=np.float32)
    times = []
    for sample in range(spp):
        for pixel in range(width * height):
            t = I.sample_time(seed, pixel, sample, 0.0, 1.0)
            times.append(float(t))
            static = Scene(M.placements_at(t), (width, height))
            one = static.gpu.render(seed, sample, 1, 0, 2).reshape(-1, 3)
            expected[pixel] = expected[pixel] + one[pixel]
    assert len(set(times)) == len(times) and min(times) < 0.05 and max(times) > 0.95
    assert float(expected.sum()) > 0.0
    assert np.array_equal(bits(image.reshape(-1, 3)), bits(expected))
    # neither end's static scene renders this image
    for t in (0.0, 1.0):
        assert not np.array_equal(bits(Scene(M.placements_at(t), (width, height)).gpu.render(seed, 0, spp, 0, 2)), bits(image))


# ------------------------------------------------------------------------------------------------------- 4. clear and replace

def test_clearing_and_replacing_the_motion(static_moments, moving_moments):
    scene = moving_scene()
    gpu = scene.gpu
    with_motion = gpu.render_moments(5, 0, 4, 0, 3)
    assert np.array_equal(bits(with_motion[0]), bits(moving_moments[0])) and gpu.stats()["path_kernel"] == 11
    assert not np.array_equal(bits(with_motion[0]), bits(static_moments[0.0][3][0]))
    # a new top tree over the moving boxes: the same bits
    gpu.rebuild_top("ploc")
    rebuilt = gpu.render_moments(5, 0, 4, 0, 3)
    assert np.array_equal(bits(rebuilt[0]), bits(with_motion[0])) and np.array_equal(bits(rebuilt[1]), bits(with_motion[1]))
    assert gpu.stats()["path_kernel"] == 11
    # cleared: the static scene of time 0 again (the open placements themselves: no interpolation took place)
    fresh = Scene(M.OPEN_PLACEMENTS)
    fresh_moments = moments(fresh.gpu)
    gpu.clear_instance_motion()
    assert_moments_equal(moments(gpu), fresh_moments)
    assert gpu.stats()["path_kernel"] == 10
    gpu.clear_instance_motion()   # nothing to remove: fine
    with pytest.raises(PathedError):
        gpu.trace_timed(np.zeros((1, 8), dtype=np.float32), np.zeros(1, dtype=np.float32))
    # set again, then new time-0 transforms: the motion goes, the new static scene's bits
    gpu.set_instance_motion(CLOSE)
    assert gpu.stats()["path_kernel"] == 11
    gpu.set_instance_transforms(CLOSE)
    replaced = Scene(M.CLOSE_PLACEMENTS)
    assert_moments_equal(moments(gpu), moments(replaced.gpu))
    assert gpu.stats()["path_kernel"] == 10
    # ... and a motion from there back to the open placements is the reversed motion: M(t) of (b, a) at a frozen shutter
    gpu.set_instance_motion(M.transforms(M.OPEN_PLACEMENTS), shutter=(0.25, 0.25))
    reverse = [(prototype, row) for (prototype, _), row in
               zip(M.OPEN_PLACEMENTS, I.interpolate_transforms(CLOSE, M.transforms(M.OPEN_PLACEMENTS), 0.25))]
    assert_moments_equal(moments(gpu), moments(Scene(reverse).gpu))


def test_the_device_entry_takes_a_tensor(moving_moments):
    import torch
    scene = Scene(M.OPEN_PLACEMENTS)
    tensor = torch.from_numpy(CLOSE).to("cuda:0")
    torch.cuda.synchronize()
    assert scene.gpu.set_instance_motion(tensor) > 0.0
    sums, squares = scene.gpu.render_moments(5, 0, 4, 0, 3)
    assert np.array_equal(bits(sums), bits(moving_moments[0])) and np.array_equal(bits(squares), bits(moving_moments[1]))
    with pytest.raises(ValueError):
        scene.gpu.set_instance_motion(tensor.cpu())
    # a bad transform is found on the device and named; the scene keeps the motion it had
    bad = CLOSE.copy()
    bad[3, 5] = np.nan
    with pytest.raises(PathedError) as caught:
        scene.gpu.set_instance_motion(torch.from_numpy(bad).to("cuda:0"))
    assert "(%d)" % INVALID in str(caught.value) and "instance transform 3 " in str(caught.value)
    again = scene.gpu.render_moments(5, 0, 4, 0, 3)
    assert np.array_equal(bits(again[0]), bits(sums)) and scene.gpu.stats()["path_kernel"] == 11


# ---------------------------------------------------------------------------------------------------------------- 5. stack rows

@pytest.mark.parametrize("count", [False, True], ids=["plain", "counting"])
def test_every_stack_row_count_renders_the_same_bits(count):
    """k_trace_instanced_motion<8 | 16 | 22, COUNT> in a render: the row count the scene takes by default and every larger one"""
    def render(rows):
        scene = moving_scene((16, 12), stack_rows=rows)
        scene.gpu.set_stats_mode(count=count)
        sums, squares = scene.gpu.render_moments(5, 0, 4, 0, 3)
        stats = scene.gpu.stats()
        assert stats["path_kernel"] == 11 and (stats["nodes_visited"] > 0 or not count)
        return sums, squares, stats["bvh_max_depth"], stats["nodes_visited"]

    sums, squares, depth, visited = render(0)
    assert float(sums.sum()) > 0.0
    rungs = instanced_stack_rungs(depth)
    assert rungs
    for rows in rungs:
        again = render(rows)
        assert np.array_equal(bits(again[0]), bits(sums)) and np.array_equal(bits(again[1]), bits(squares)), rows
        assert again[3] == visited, rows


# --------------------------------------------------------------------------------------------------------------------- 6. lists

@pytest.mark.parametrize("listed", [1, 65, SIZE[0] * SIZE[1]])
def test_a_list_pass_holds_the_full_renders_bits(moving, moving_moments, listed):
    width, height = SIZE
    pixels = width * height
    full_sums, full_squares = moving_moments
    chosen = np.sort(np.random.default_rng(listed).choice(pixels, listed, replace=False)).astype(np.uint32)
    gpu = moving.gpu
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
    assert np.array_equal(bits(sums[chosen]), bits(full_sums.reshape(pixels, 3)[chosen]))
    assert np.array_equal(bits(squares[chosen]), bits(full_squares.reshape(pixels, 3)[chosen]))
    assert np.all(sums[others] == np.float32(0.375)) and np.all(squares[others] == np.float32(0.375))
    assert np.all(counts[chosen] == 11) and np.all(counts[others] == 7)


# --------------------------------------------------------------------------------------------------------- 7. two calls are one

def test_two_calls_are_one(moving):
    width, height = SIZE
    gpu = moving.gpu
    one = gpu.render_moments(5, 0, 8, 0, 3)
    buffers = [gpu.device_buffer(3 * width * height), gpu.device_buffer(3 * width * height)]
    try:
        gpu.render_moments_device(5, 0, 3, 0, 3, buffers[0], buffers[1])
        gpu.render_moments_device(5, 3, 5, 0, 3, buffers[0], buffers[1])
        sums = gpu.download_device_buffer(buffers[0], np.zeros((height, width, 3), dtype=np.float32))
        squares = gpu.download_device_buffer(buffers[1], np.zeros((height, width, 3), dtype=np.float32))
    finally:
        for pointer in buffers:
            gpu.free_device_buffer(pointer)
    assert float(one[0].sum()) > 0.0
    assert np.array_equal(bits(sums), bits(one[0])) and np.array_equal(bits(squares), bits(one[1]))


# ------------------------------------------------------------------------------------------------------------------ 8. refusals

def refused(call, code, word):
    with pytest.raises(PathedError) as caught:
        call()
    assert "(%d)" % code in str(caught.value) and word in str(caught.value), str(caught.value)


def test_refusals_launch_nothing():
    scene = Scene(M.OPEN_PLACEMENTS)
    gpu = scene.gpu
    flat = flatten_instances(scene.pointer, scene.prototypes, scene.placements)
    plain = HipScene(flat.desc, device=0)
    gpu.reset_stats()
    plain.reset_stats()
    ray, time = np.array([[0.0, 3.0, 12.0, 1e-3, 0.0, 0.0, -1.0, 1e5]], dtype=np.float32), np.zeros(1, dtype=np.float32)
    refused(lambda: plain.set_instance_motion(CLOSE), UNSUPPORTED, "no instances")
    refused(lambda: plain.clear_instance_motion(), UNSUPPORTED, "no instances")
    refused(lambda: plain.trace_timed(ray, time), UNSUPPORTED, "no instances")
    refused(lambda: gpu.trace_timed(ray, time), INVALID, "no motion")
    refused(lambda: gpu.set_instance_motion(CLOSE[:4]), INVALID, "count")
    refused(lambda: gpu.set_instance_motion(np.concatenate([CLOSE, CLOSE[:1]])), INVALID, "count")
    lib = gpu._lib
    refused(lambda: _check(lib, lib.pathed_hip_scene_set_instance_motion(None, None, 0, 0.0, 1.0, None), "set"), INVALID, "null")
    for shutter in ((-0.1, 1.0), (0.0, 1.5), (0.6, 0.5), (float("nan"), 1.0), (0.0, float("nan"))):
        refused(lambda: gpu.set_instance_motion(CLOSE, shutter=shutter), INVALID, "shutter")
    nan = CLOSE.copy()
    nan[3, 5] = np.nan
    refused(lambda: gpu.set_instance_motion(nan), INVALID, "instance transform 3 ")
    infinite = CLOSE.copy()
    infinite[4, 11] = np.inf
    refused(lambda: gpu.set_instance_motion(infinite), INVALID, "not finite")
    singular = CLOSE.copy()
    singular[2, 4:8] = singular[2, 0:4]
    refused(lambda: gpu.set_instance_motion(singular), INVALID, "instance transform 2 ")
    refused(lambda: gpu.set_instance_motion(singular), INVALID, "not invertible")
    assert gpu.stats()["trace_launches_all"] == 0 and plain.stats()["trace_launches_all"] == 0
    assert gpu.stats()["path_kernel"] == 10
    # the scene is as it was, and a time outside the shutter is refused once there is one
    fresh = Scene(M.OPEN_PLACEMENTS)
    assert np.array_equal(bits(gpu.render(5, 0, 4, 0, 3)), bits(fresh.gpu.render(5, 0, 4, 0, 3)))
    gpu.set_instance_motion(CLOSE, shutter=(0.25, 0.75))
    refused(lambda: gpu.trace_timed(ray, np.array([0.8], dtype=np.float32)), INVALID, "outside the scene's shutter")
    gpu.trace_timed(ray, np.array([0.5], dtype=np.float32))


def test_a_placement_that_is_singular_in_between_is_skipped():
    """a half turn interpolated linearly: M(0.5) has no inverse, so rays of that time pass the placement by, and rays of
    other times meet it where the static scene of their time has it"""
    start = [(S.Q, S.affine(np.eye(3)))]
    turned = S.affine(S.rotation((0.0, 1.0, 0.0), 180.0))
    turned[[1, 4, 6, 9]] = 0.0            # an exact half turn about y: diag(-1, 1, -1)
    turned[[0, 5, 10]] = (-1.0, 1.0, -1.0)
    scene = Scene(start)
    scene.gpu.set_instance_motion(turned.reshape(1, 12))
    world = int(scene.flat().bases[0])
    for t in (0.0, 0.25, 0.75):
        static = Scene([(S.Q, I.interpolate_transforms(start[0][1], turned, t))])
        rays = S.general_rays(static.flat(), 500, 71)   # aimed at the world and at the placement where time t has it
        expected = static.gpu.trace(rays)
        assert (bits(expected[:, 3]).view(np.int32) >= world).sum() > 100, t
        assert np.array_equal(bits(scene.gpu.trace_timed(rays, np.full(len(rays), t, dtype=np.float32))), bits(expected)), t
        half = scene.gpu.trace_timed(rays, np.full(len(rays), 0.5, dtype=np.float32))
        assert np.all(bits(half[:, 3]).view(np.int32) < world), t


# --------------------------------------------------------------------------------------------------------------- 9. executable

def _shutter_scene_file(tmp_path, name, close=None, transform=None):
    """a floor with a glowing patch, a prototype of two quads above it, one placement -- with "transform_close" when `close` is given"""
    import json
    import test_instances_host as H
    # (time 0: low and near, between the camera and the patch, which the quads' unlit tops hide in part; by the CPU oracle the
    # flattened scenes of the two ends differ in a tenth of the 64 x 48 pixels)
    open_transform = (H.turn(20.0) @ np.diag([1.5, 1.0, 1.5]), (-1.0, 0.0, 5.0))
    models = [
        H.quad(["0.5", "0.5", "0.5"], ("0", "0", "0"), scale=("10", "1", "10")),
        H.quad(["0", "0", "0"], ("0", "0.02", "0"), emit=["9", "8", "7"], scale=("4", "1", "4")),   # (faces up: the camera sees its front)
        {"type": "instance", "name": "leaf", "models": [H.quad(["0.2", "0.7", "0.2"], ("0.5", "2", "0.5")), H.quad(["0.7", "0.3", "0.2"], ("0.2", "1", "0.4"))]},
        {"type": "instanced", "instance_name": "leaf", "transform": transform if transform is not None else H.column_major(*open_transform)},
    ]
    if close is not None:
        models[3]["transform_close"] = close
    scene = {"sensor": {"lookAt": {"origin": ["0", "3", "12"], "target": ["0", "1", "0"], "up": ["0", "1", "0"]}, "fov": "40"}, "models": models}
    path = tmp_path / (name + ".json")
    path.write_text(json.dumps(scene))
    return str(path), H.column_major(*open_transform)


def _run(launcher, name, job, tmp_path):
    import json
    import os
    import subprocess
    import sys
    from pathed_amd import _capi
    job = dict(job, output_directory=str(tmp_path / name))
    job_path = str(tmp_path / (name + "-job.json"))
    json.dump(job, open(job_path, "w"))
    command = ([os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")] if launcher == "cpp" else [sys.executable, "-m", "pathed_amd.run_job"]) + [job_path, _capi.REPO_ROOT]
    return subprocess.run(command, capture_output=True, text=True, cwd=_capi.REPO_ROOT), job


def _launch(launcher, name, job, tmp_path):
    import os
    result, job = _run(launcher, name, job, tmp_path)
    assert result.returncode == 0, result.stdout + result.stderr
    files = ["auto.exr", "auto-00004spp.exr"] + (["auto-00008spp.exr"] if job["spp"] >= 8 else [])
    return {f: open(os.path.join(job["output_directory"], f), "rb").read() for f in files}, job


def test_a_job_with_a_moving_placement_through_both_launchers(tmp_path):
    import json
    import os
    import test_instances_host as H
    from pathed_amd import _capi
    from test_gpu_job import _read_state
    close = H.column_major(H.turn(140.0) @ np.diag([1.0, 2.0, 0.8]), (2.5, 1.5, -1.0))
    moving, open_transform = _shutter_scene_file(tmp_path, "moving", close=close)
    still, _ = _shutter_scene_file(tmp_path, "still")
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(width=64, height=48, spp=8, scene=moving, force=True)
    cpp, cpp_job = _launch("cpp", "cpp", job, tmp_path)
    py, _ = _launch("py", "py", job, tmp_path)
    assert cpp == py
    # ... which is not the job without the key
    without, _ = _launch("cpp", "without", dict(job, scene=still), tmp_path)
    assert without["auto.exr"] != cpp["auto.exr"]
    # a resumed job equals the straight one
    _launch("cpp", "resumed", dict(job, spp=4), tmp_path)
    resumed, resumed_job = _launch("cpp", "resumed", dict(job, resume=True), tmp_path)
    assert resumed["auto-00008spp.exr"] == cpp["auto-00008spp.exr"]
    assert np.array_equal(_read_state(os.path.join(resumed_job["output_directory"], "auto.state"))[1], _read_state(os.path.join(cpp_job["output_directory"], "auto.state"))[1])
    # ... under the shutter it was started with: the state file of another shutter is another job's
    result, _ = _run("cpp", "resumed", dict(job, spp=16, resume=True, shutter=[0.0, 0.5]), tmp_path)
    assert result.returncode != 0 and "state file was rendered from another scene" in result.stdout + result.stderr, result.stdout + result.stderr
    result, _ = _run("cpp", "resumed", dict(job, spp=16, resume=True, shutter=[0.0, 1.0]), tmp_path)   # the default, written out
    assert result.returncode == 0 and "resuming at sample 8/16" in result.stdout, result.stdout + result.stderr
    # a frozen shutter is the scene file with the interpolated transform written out (9 digits round-trip float32)
    to_rows = lambda column_major: np.array([float(x) for x in column_major], dtype=np.float32).reshape(4, 4).T[:3].reshape(12)
    halfway = I.interpolate_transforms(to_rows(open_transform), to_rows(close), 0.5).reshape(3, 4)
    written = ["%.9g" % float(x) for x in np.vstack([halfway, np.array([[0, 0, 0, 1]], dtype=np.float32)]).T.reshape(-1)]
    assert np.array_equal(bits(to_rows(written)), bits(halfway.reshape(12)))
    frozen, _ = _launch("cpp", "frozen", dict(job, shutter=[0.5, 0.5]), tmp_path)
    static_file, _ = _shutter_scene_file(tmp_path, "halfway", transform=written)
    static, _ = _launch("cpp", "static", dict(job, scene=static_file), tmp_path)
    assert frozen == static
    frozen_py, _ = _launch("py", "frozen-py", dict(job, shutter=[0.5, 0.5]), tmp_path)
    assert frozen_py == static
    assert frozen["auto.exr"] != cpp["auto.exr"] and frozen["auto.exr"] != without["auto.exr"]


@pytest.mark.parametrize("launcher", ["cpp", "py"])
def test_both_launchers_refuse_a_shutter_by_name(tmp_path, launcher):
    """"shutter" on a scene where nothing moves, or outside its rule: refused by name once the scene file is read, before a tree
    is built (the Python launcher needs a GPU to start at all, so its refusals are checked here)"""
    import json
    import os
    from pathed_amd import _capi
    close = ["%.9g" % x for x in (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2, 1, 0, 1)]
    moving, _ = _shutter_scene_file(tmp_path, "moving", close=close)
    still, _ = _shutter_scene_file(tmp_path, "still")
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(width=16, height=16, spp=1, force=True)
    for scene, shutter, words in ((still, [0.0, 1.0], ["shutter", "nothing moves"]), (moving, [0.6, 0.5], ["shutter", "0 <= open <= close <= 1"]),
                                  (moving, [0.5], ["shutter", "[open, close]"]), (moving, "open", ["shutter", "[open, close]"])):
        result, _ = _run(launcher, "refused", dict(job, scene=scene, shutter=shutter), tmp_path)
        assert result.returncode != 0
        for word in words:
            assert word in result.stdout + result.stderr, result.stdout + result.stderr
        assert "sample:" not in result.stdout
