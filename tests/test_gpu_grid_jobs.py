"""jobs/cornell-smoke.json (scenes/cornell-smoke.json: a voxel-grid medium from a .vol file under a transform) at a reduced
size through both job runners -- the C++ host `pathed` and pathed_amd.run_job -- and a resumed run of the C++ host, whose
state file's digest covers the .vol bytes."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from pathed_amd import _capi

pytestmark = pytest.mark.gpu


def smoke_job(**changes):
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-smoke.json")))
    assert job["scene"] == "scenes/cornell-smoke.json" and job["integrator"] == "VolumePathTracer"
    job.update(width=48, height=40, spp=8, spp_per_launch=4)
    job.update(changes)
    return job


def run(tmp_path, name, job, runner="cpp", asset_root=_capi.REPO_ROOT):
    out_dir = str(tmp_path / name)
    job = dict(job, output_directory=out_dir)
    job_path = str(tmp_path / (name + ".json"))
    json.dump(job, open(job_path, "w"))
    if runner == "cpp":
        command = [os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed"), job_path, asset_root]
    else:
        command = [sys.executable, "-m", "pathed_amd.run_job", job_path, asset_root]
    environment = dict(os.environ, PYTHONPATH=_capi.REPO_ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return out_dir, subprocess.run(command, capture_output=True, text=True, cwd=str(tmp_path), env=environment)


def test_smoke_job_through_both_runners(tmp_path):
    outputs = {}
    for runner in ("cpp", "py"):
        out_dir, result = run(tmp_path, runner, smoke_job(), runner)
        assert result.returncode == 0, result.stdout + result.stderr
        outputs[runner] = {name: open(os.path.join(out_dir, name), "rb").read() for name in ("auto-00004spp.exr", "auto-00008spp.exr", "auto.exr")}
    assert outputs["cpp"] == outputs["py"]
    # the smoke is in the picture: the same job with the grid's density scaled to nothing is another image
    scene = json.load(open(os.path.join(_capi.REPO_ROOT, "scenes", "cornell-smoke.json")))
    scene["media"][0]["scale"] = "0.0"
    clear_path = str(tmp_path / "clear-scene.json")
    json.dump(scene, open(clear_path, "w"))
    out_dir, result = run(tmp_path, "clear", smoke_job(scene=clear_path))
    assert result.returncode == 0, result.stdout + result.stderr
    assert open(os.path.join(out_dir, "auto-00008spp.exr"), "rb").read() != outputs["cpp"]["auto-00008spp.exr"]
    # any other integrator is refused
    _, result = run(tmp_path, "refused", smoke_job(integrator="PathTracer"))
    assert result.returncode != 0 and "VolumePathTracer" in (result.stdout + result.stderr)


def test_resumed_smoke_job_equals_the_straight_run(tmp_path):
    straight_dir, result = run(tmp_path, "straight", smoke_job(spp=8))
    assert result.returncode == 0, result.stdout + result.stderr
    _, result = run(tmp_path, "resumed", smoke_job(spp=4))
    assert result.returncode == 0, result.stdout + result.stderr
    resumed_dir, result = run(tmp_path, "resumed", smoke_job(spp=8, resume=True))
    assert result.returncode == 0 and "resuming at sample 4/8" in result.stdout, result.stdout + result.stderr
    for name in ("auto-00008spp.exr", "auto.state"):
        assert open(os.path.join(resumed_dir, name), "rb").read() == open(os.path.join(straight_dir, name), "rb").read(), name


def test_a_changed_vol_file_is_another_scene_to_a_resumed_job(tmp_path):
    """the state file's digest covers the .vol bytes as it covers the scene file: the same scene over an edited grid does not
    continue the old sums"""
    root = tmp_path / "root"
    for directory in ("scenes", "assets/cornell-volume-caustic"):
        os.makedirs(str(root / directory))
    for name in ("scenes/cornell-smoke.json", "scenes/CornellBox-Original.mtl", "assets/smoke-plume.vol", "assets/cornell-volume-caustic/bounds.obj",
                 "assets/cornell-volume-caustic/CornellBox-Frame.obj"):
        shutil.copy(os.path.join(_capi.REPO_ROOT, name), str(root / name))
    _, result = run(tmp_path, "edited", smoke_job(spp=4), asset_root=str(root))
    assert result.returncode == 0, result.stdout + result.stderr
    with open(str(root / "assets" / "smoke-plume.vol"), "r+b") as handle:
        handle.seek(48 + 4 * (16 * 32 * 32 + 8 * 32 + 16))
        value = struct.unpack("<f", handle.read(4))[0]
        handle.seek(-4, 1)
        handle.write(struct.pack("<f", value + 0.25))
    _, result = run(tmp_path, "edited", smoke_job(spp=8, resume=True), asset_root=str(root))
    assert result.returncode != 0 and "another scene" in (result.stdout + result.stderr)
