"""Second moments and noise-targeted stopping, the parts that need no GPU: the numpy restatement of the formulas against
float64, the job keys in both hosts, and the two new kernels' resources (compile-only)."""
import json
import os
import subprocess

import numpy as np
import pytest

import noise_reference
from test_kernel_resources import resource_usage

F = np.float32


def test_float32_restatement_against_float64():
    """tests/noise_reference.py against a float64 evaluation of the same formulas on the same fp32 sums, to the project's
    function-level tolerance (1e-6 relative + 2e-7 absolute, as tests/test_gpu_features.py).

    Inputs: per channel a mean m in [0.2, 4], a per-sample relative deviation r = sigma / m in [0.7, 3] and n out of
    {4, 5, 16, 64, 256, 1024}: S = n m, Q = n m^2 (1 + r^2), rounded to fp32; floors 0.01 and 0.1.  A pixel's relative noise
    is then at least (0.7 / sqrt(3 n)) (0.6 / 0.7) = 0.346 / sqrt(n) >= 0.0108 >= 0.01 (sqrt(sum m^2 r^2) >= 0.7 sum m / sqrt(3),
    and the floor is at most a seventh of the brightness), and d / (Q / n) = r^2 / (1 + r^2) >= 0.32: no case cancels below
    1e-3, none is excluded (both asserted).  Why the tolerance holds on these: with u = 2^-24, Q / n and m carry u each and
    m * m 3u, so d_c has the absolute error u m_c^2 (4 + r_c^2) + u d_c <= u (4 / 0.49 + 2) d_c; e goes with the square root
    of their sum: 5.1 u = 3.1e-7 relative, and the channel sums, the two divisions and the root add below 5 u = 3e-7."""
    rng = np.random.default_rng(17)
    for n in (4, 5, 16, 64, 256, 1024):
        m = rng.uniform(0.2, 4.0, size=(4096, 3))
        r = rng.uniform(0.7, 3.0, size=(4096, 3))
        S = (n * m).astype(F)
        Q = (n * m * m * (1.0 + r * r)).astype(F)
        for floor in (0.01, 0.1):
            expected, survives = noise_float64(S, Q, n, floor)
            assert survives.min() >= 1e-3            # the exclusion is a condition: nothing is excluded
            assert expected.min() >= 0.01            # relative noise of every pixel
            found, invalid = noise_reference.noise(S, Q, n, floor)
            assert found.dtype == F and not invalid.any()
            assert np.all(np.abs(found.astype(np.float64) - expected) <= 1e-6 * np.abs(expected) + 2e-7), (n, floor)
        # the standard error of the mean per channel (auto-stderr.exr) is the same v_c
        m64 = S.astype(np.float64) / n
        v64 = np.maximum(Q.astype(np.float64) / n - m64 * m64, 0.0) * (n / (n - 1.0))
        se = noise_reference.standard_error(S, Q, n)
        assert np.all(np.abs(se - np.sqrt(v64 / n)) <= 1e-6 * np.sqrt(v64 / n) + 2e-7)


noise_float64 = noise_reference.noise_float64


def test_square_sum_chain_against_float64():
    rng = np.random.default_rng(3)
    samples = rng.uniform(0.0, 6.0, size=(5, 384, 3)).astype(F)
    samples[2, 7] = 0.0                       # a dropped sample's entry is zero: adds zero
    start = rng.uniform(0.0, 2.0, size=(384, 3)).astype(F)
    q = noise_reference.square_sums(samples, start)
    exact = start.astype(np.float64) + (samples.astype(np.float64) ** 2).sum(axis=0)
    assert q.dtype == F and np.all(np.abs(q - exact) <= 1e-6 * exact + 2e-7)
    # continuation: 2 + 3 samples are the 5 of one chain, bit for bit
    assert np.array_equal(noise_reference.square_sums(samples[2:], noise_reference.square_sums(samples[:2], start)), q)
    s = noise_reference.sums(samples, start)
    assert np.all(np.abs(s - (start.astype(np.float64) + samples.astype(np.float64).sum(axis=0))) <= 1e-6 * s + 2e-7)


def test_degenerate_pixels():
    S = np.zeros((3, 3), dtype=F)
    Q = np.zeros((3, 3), dtype=F)
    S[1], Q[1] = 8.0, 4.0                     # Q / n < m^2: the variance is clamped at zero
    Q[2, 0] = np.inf                          # a square sum that overflowed: e is not finite, counts as 0 and as invalid
    e, invalid = noise_reference.noise(S, Q, 8, 0.01)
    assert e[0] == 0.0 and e[1] == 0.0 and e[2] == 0.0 and list(invalid) == [False, False, True]


def _job(tmp_path, **keys):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.update(keys)
    job["output_directory"] = str(tmp_path / "out")
    return job


def test_noise_keys_defaults():
    from pathed_amd.integrator import noise_from_job
    assert noise_from_job({}) == (None, 16, 0.01, False)
    assert noise_from_job({"stderr_image": True}) == (None, 16, 0.01, True)
    assert noise_from_job({"target_noise": 0.05, "min_spp": 4, "noise_floor": 0.1}) == (0.05, 4, 0.1, True)


@pytest.mark.parametrize("keys, name", [
    ({"target_noise": 0}, "target_noise"),
    ({"min_spp": 1, "target_noise": 0.1}, "min_spp"),
    ({"resume": True, "target_noise": 0.1}, "resume"),
    ({"resume": True, "stderr_image": True}, "resume"),
    ({"noise_floor": 0.0, "stderr_image": True}, "noise_floor"),
    ({"target_noise": "low"}, "target_noise"),
])
def test_bad_noise_keys_are_refused_by_name_in_both_hosts(tmp_path, keys, name):
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError, noise_from_job

    job = _job(tmp_path, **keys)
    with pytest.raises(PathedError, match=name):
        noise_from_job(job)

    # the C++ host refuses the same job before it touches the output directory (and before any GPU call)
    job_path = str(tmp_path / "job.json")
    json.dump(job, open(job_path, "w"))
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, job_path, _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode != 0 and ("\"%s\"" % name) in result.stderr, result.stdout + result.stderr
    assert not os.path.exists(job["output_directory"])


def test_path_tracer_arguments():
    from pathed_amd.integrator import BounceController, PathedError, PathTracer
    tracer = PathTracer(BounceController(0, 10), spp=64, target_noise=0.05, min_spp=4)
    assert tracer.target_noise == 0.05 and tracer.min_spp == 4 and tracer.noise_floor == 0.01 and tracer.noise_history == []
    assert PathTracer(BounceController(0, 10)).target_noise is None
    for bad in (dict(target_noise=0.0), dict(min_spp=1), dict(noise_floor=0.0)):
        with pytest.raises(PathedError):
            PathTracer(BounceController(0, 10), **bad)


def test_the_example_job_parses():
    from pathed_amd import _capi
    from pathed_amd.integrator import noise_from_job
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-noise.json")))
    target, min_spp, floor, write_stderr = noise_from_job(job)
    assert target > 0 and min_spp >= 2 and floor > 0 and write_stderr and job["spp"] >= min_spp


def test_noise_struct_matches_the_header(tmp_path):
    import ctypes as C
    from pathed_amd import _capi
    source = ('#include "pathed_hip.h"\n#include <stddef.h>\n#include <stdio.h>\n'
              'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(PathedNoise), offsetof(PathedNoise, mean_error),'
              ' offsetof(PathedNoise, max_error), offsetof(PathedNoise, pixels_above));return 0;}\n')
    c_file = str(tmp_path / "noise_size.c")
    open(c_file, "w").write(source)
    exe = str(tmp_path / "noise_size")
    subprocess.run(["gcc", "-I", os.path.join(_capi.REPO_ROOT, "include"), c_file, "-o", exe], check=True)
    found = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    noise = _capi.PathedNoise
    assert found == [C.sizeof(noise), noise.mean_error.offset, noise.max_error.offset, noise.pixels_above.offset]


def test_new_kernels_use_no_scratch(tmp_path):
    """k_resolve_moments and k_noise: no scratch (compile-only, as tests/test_kernel_resources.py)."""
    usage = resource_usage(tmp_path)
    moments = [v for k, v in usage.items() if "k_resolve_moments" in k]
    noise = [v for k, v in usage.items() if "7k_noise" in k]
    assert len(moments) == 1 and len(noise) == 1, sorted(usage)
    assert moments[0]["ScratchSize"] == 0 and noise[0]["ScratchSize"] == 0, (moments, noise)
