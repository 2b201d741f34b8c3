"""Feature images and the AlbedoIntegrator, the parts that need no GPU: the job keys and the feature kernel's register budget."""
import json
import os
import subprocess

import pytest

from test_kernel_resources import resource_usage


def _job(tmp_path, **keys):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(keys)
    job["output_directory"] = str(tmp_path / "out")
    return job


def test_unknown_feature_name_is_rejected_by_name(tmp_path):
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError, features_from_job

    job = _job(tmp_path, features=["albedo", "roughness"])
    with pytest.raises(PathedError, match="roughness"):
        features_from_job(job)
    assert features_from_job(_job(tmp_path)) == []
    assert features_from_job(_job(tmp_path, features=["depth", "albedo"])) == ["albedo", "depth"]

    # the C++ host refuses the same job before it touches the output directory (and before any GPU call)
    job_path = str(tmp_path / "job.json")
    json.dump(job, open(job_path, "w"))
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode != 0 and "roughness" in result.stderr, result.stdout + result.stderr
    assert not os.path.exists(job["output_directory"])


def test_integrator_from_job_accepts_the_albedo_integrator(tmp_path):
    from pathed_amd.integrator import PathedError, PathTracer, integrator_from_job

    integrator = integrator_from_job(_job(tmp_path, integrator="AlbedoIntegrator", spp=4))
    assert isinstance(integrator, PathTracer) and integrator.spp == 4
    with pytest.raises(PathedError, match="Unimplemented"):
        integrator_from_job(_job(tmp_path, integrator="NoSuchIntegrator"))


def test_feature_kernel_register_budget(tmp_path):
    """k_features: no scratch and at most 128 VGPRs, i.e. four waves per SIMD at 256 threads per block (its state is a ray,
    eight sums and the traversal registers).  Compile-only, as tests/test_kernel_resources.py."""
    usage = resource_usage(tmp_path)
    features = {k: v for k, v in usage.items() if "10k_featuresI" in k}
    assert len(features) == 6, sorted(features)   # three stack heights x (feature, reference) mode
    assert all(v["ScratchSize"] == 0 and v["VGPRs"] <= 128 and v["Occupancy"] >= 4 for v in features.values()), features
