"""Adaptive sampling, the parts that need no GPU: the job key "adaptive" in both hosts (the per-GPU runner wants a GPU before it
reads a key: tests/test_gpu_adaptive.py), the numpy
restatement (tests/adaptive_reference.py) against cases worked out by hand."""
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference
import noise_reference

F = np.float32


def _job(tmp_path, **keys):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(keys)
    job["output_directory"] = str(tmp_path / "out")
    return job


def test_adaptive_key_defaults():
    from pathed_amd.integrator import adaptive_from_job
    assert adaptive_from_job({}) is False
    assert adaptive_from_job({"adaptive": False, "resume": True}) is False          # the key is off: nothing to refuse
    assert adaptive_from_job({"adaptive": True, "target_noise": 0.05}) is True
    assert adaptive_from_job({"adaptive": True, "target_noise": 0.05, "gpus": [0]}) is True


@pytest.mark.parametrize("keys, reason", [
    ({"adaptive": True}, "target_noise"),
    ({"adaptive": True, "target_noise": 0.1, "resume": True}, "resume"),
    ({"adaptive": True, "target_noise": 0.1, "gpus": 2}, "gpus"),
    ({"adaptive": True, "target_noise": 0.1, "gpus": [0, 0]}, "gpus"),
    ({"adaptive": True, "target_noise": 0.1, "integrator": "AlbedoIntegrator"}, "AlbedoIntegrator"),
    ({"adaptive": "yes", "target_noise": 0.1}, "true or false"),
])
def test_adaptive_is_refused_by_name_in_both_hosts(tmp_path, keys, reason):
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError, adaptive_from_job

    job = _job(tmp_path, **keys)
    with pytest.raises(PathedError, match=r'"adaptive".*' + reason):
        adaptive_from_job(job)

    # the C++ host refuses the same job before it touches the output directory (and before any GPU call)
    job_path = str(tmp_path / "job.json")
    json.dump(job, open(job_path, "w"))
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode != 0 and '"adaptive"' in result.stderr and reason in result.stderr, result.stdout + result.stderr
    assert not os.path.exists(job["output_directory"])


def test_path_tracer_arguments():
    from pathed_amd.integrator import BounceController, PathedError, PathTracer
    tracer = PathTracer(BounceController(0, 10), spp=64, target_noise=0.05, min_spp=4, adaptive=True)
    assert tracer.adaptive and tracer.sample_counts is None
    assert not PathTracer(BounceController(0, 10), target_noise=0.05).adaptive
    with pytest.raises(PathedError, match="target_noise"):
        PathTracer(BounceController(0, 10), adaptive=True)


def test_the_example_job_parses():
    from pathed_amd import _capi
    from pathed_amd.integrator import adaptive_from_job, noise_from_job
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-adaptive.json")))
    target, min_spp, floor, write_stderr = noise_from_job(job)
    assert adaptive_from_job(job) is True and target > 0 and 2 <= min_spp < job["spp"]
    plain = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-noise.json")))
    for key in ("scene", "integrator", "startBounce", "lastBounce", "width", "height"):
        assert job[key] == plain[key]                      # the same render, the stopping rule apart


# ------------------------------------------------------------------------------------------- the reference by hand

def test_errors_by_hand():
    """Grey pixels S = (s, s, s), Q = (q, q, q), floor 0.5, all values exact in float32:
      n = 2, s = 2, q = 4:  m = 1, d = 2 - 1 = 1, v = 1 * 2 = 2, e = sqrt(6 / 2) / 3.5 = sqrt(3) / 3.5
      n = 4, s = 4, q = 8:  m = 1, d = 1, v = 4 / 3 (rounded), e = sqrt((v + v + v) / 4) / 3.5
      n = 4, s = 4, q = 4:  d = 0: e = 0
      n = 1, n = 0:         no spread yet: e = 0, invalid, selected whatever the threshold
      n = 4, q = inf:       e is not finite: 0, invalid, not selected"""
    S = np.array([[2, 2, 2], [4, 4, 4], [4, 4, 4], [1, 1, 1], [0, 0, 0], [4, 4, 4]], dtype=F)
    Q = np.array([[4, 4, 4], [8, 8, 8], [4, 4, 4], [1, 1, 1], [0, 0, 0], [np.inf, 8, 8]], dtype=F)
    counts = np.array([2, 4, 4, 1, 0, 4], dtype=np.uint32)
    e, invalid, chosen = adaptive_reference.select(S, Q, counts, 0.5, 0.4)
    v = F(F(4) / F(3))
    expected1 = F(np.sqrt(F(F(F(v + v) + v) / F(4))) / F(3.5))
    assert e.dtype == F and e[0] == F(np.sqrt(F(3)) / F(3.5)) and e[1] == expected1
    assert abs(float(e[0]) - 3 ** 0.5 / 3.5) < 1e-7 and abs(float(e[1]) - 1 / 3.5) < 1e-7      # 0.4949, 0.2857
    assert list(e[2:]) == [0, 0, 0, 0] and list(invalid) == [False, False, False, True, True, True]
    assert chosen.dtype == np.uint32 and list(chosen) == [0, 3, 4]          # 0.4949 > 0.4 >= 0.2857; the two without a spread
    assert list(adaptive_reference.select(S, Q, counts, 0.5, 0.2)[2]) == [0, 1, 3, 4]
    assert list(adaptive_reference.select(S, Q, counts, 0.5, 1.0)[2]) == [3, 4]
    # one count everywhere: noise_reference's own figures
    uniform = np.full(6, 4, dtype=np.uint32)
    assert np.array_equal(adaptive_reference.errors(S, Q, uniform, 0.5)[0], noise_reference.noise(S, Q, 4, 0.5)[0])


def test_mean_by_hand():
    """257 pixels: a block of 256 and a block of one.  2^-30 added 256 times to nothing is exact, and the second block's 1.0
    is added to that sum: (1 + 2^-22) / 257 -- whereas adding the small values to 1.0 in float32 would lose them."""
    e = np.full(257, 2.0 ** -30, dtype=F)
    e[256] = 1.0
    assert adaptive_reference.mean_error(e) == (1.0 + 2.0 ** -22) / 257.0
    assert adaptive_reference.mean_error(np.array([0.5], dtype=F)) == 0.5
    # the same additions in the same order as the loop it restates, where the order matters: values over 12 decades
    rng = np.random.default_rng(3)
    for pixels in (1, 255, 256, 257, 1000, 8100 * 256 // 100 + 7):
        e = (rng.uniform(0.0, 1.0, pixels) * 10.0 ** rng.integers(-9, 3, pixels)).astype(F)
        total = 0.0
        for first in range(0, pixels, 256):
            partial = 0.0
            for value in e[first:first + 256]:
                partial += float(value)
            total += partial
        assert adaptive_reference.mean_error(e) == total / pixels, pixels


def test_replay_by_hand():
    """Three pixels, min_spp 2, cap 8, target 0.4, floor 0.5.  Sums made so that e is known:
      pixel 0 is constant (q = s^2 / n): e = 0 at every count: retires at 2;
      pixel 1 has e = sqrt(3) / 3.5 = 0.495 at 2 samples and 0 at 4: retires at 4;
      pixel 2 keeps m = 1, d = 1: e = sqrt(3 n / (n - 1) / n) / 3.5 = 0.495, 0.286 at 2 and 4 -- but a retired pixel stays retired,
      so its 0.286 at 4 retires it there too; with target 0.2 it goes on to the cap (0.187 at 8 would retire it; the cap ends the run).
    """
    def image(n, d):          # per pixel: S = n, Q = n (1 + d)
        S = np.full((3, 3), n, dtype=F)
        Q = np.array([[n * (1 + x)] * 3 for x in d], dtype=F)
        return S, Q
    uniform = {2: image(2, [0, 1, 1]), 4: image(4, [0, 0, 1]), 8: image(8, [0, 0, 1])}
    counts, rounds, rendered = adaptive_reference.replay(uniform, 2, 8, 0.4, 0.5)
    assert list(counts) == [2, 4, 4] and rounds == 1 and rendered == 3 * 2 + 2 * 2
    counts, rounds, rendered = adaptive_reference.replay(uniform, 2, 8, 0.2, 0.5)
    assert list(counts) == [2, 4, 8] and rounds == 2 and rendered == 3 * 2 + 2 * 2 + 1 * 4
    # a pixel whose error rises again after it retired is not taken up again
    uniform[4] = image(4, [5, 0, 1])
    assert list(adaptive_reference.replay(uniform, 2, 8, 0.2, 0.5)[0]) == [2, 4, 8]
    # min_spp beyond the cap: the cap's samples and no round
    counts, rounds, rendered = adaptive_reference.replay({8: image(8, [0, 0, 1])}, 16, 8, 0.01, 0.5)
    assert list(counts) == [8, 8, 8] and rounds == 0 and rendered == 24
