"""The seed as written, the parts that need no GPU: the job key "seed" in both hosts' readers (the per-GPU runner wants a GPU
before it reads a key, so its reader, seed_from_job, is called directly), the range check of the Python wrappers, and the
exact unsigned value a JSON number keeps beside its double.  The renders are in tests/test_gpu_job.py and
tests/test_gpu_argument_edges.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

# written as they would stand in a job file: the text is what matters, not what a float of it holds
EXACT = ["0", "1", "9007199254740992", "9007199254740993", "4294967297", "9223372036854775808", "18446744073709551615"]
REFUSED = ["-1", "1.5", "1.0", "1e3", "1E3", "18446744073709551616", "99999999999999999999999", "\"7\"", "true", "null", "[7]", "+7"]


def _job_text(seed_text, out_dir):
    from pathed_amd import _capi
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job["output_directory"] = out_dir
    job["seed"] = "@SEED@"
    text = json.dumps(job, indent=2).replace("\"@SEED@\"", seed_text)
    assert seed_text in text
    return text


@pytest.mark.parametrize("text", EXACT)
def test_both_readers_keep_the_seed_exactly(tmp_path, text):
    from pathed_amd import _capi
    from pathed_amd.integrator import seed_from_job
    host = _capi.load_host()
    job_path = tmp_path / "job.json"
    job_path.write_text(_job_text(text, str(tmp_path / "out")))
    value = C.c_uint64(12345)
    assert host.pathed_host_job_seed(str(job_path).encode(), C.byref(value)) == 0, host.pathed_host_last_error()
    assert value.value == int(text)
    assert seed_from_job(json.load(open(job_path))) == int(text)


def test_the_default_seed_is_one(tmp_path):
    from pathed_amd import _capi
    from pathed_amd.integrator import seed_from_job
    job = json.load(open(os.path.join(_capi.REPO_ROOT, "jobs", "cornell-c1.json")))
    job.pop("seed", None)
    job_path = tmp_path / "job.json"
    job_path.write_text(json.dumps(job))
    value = C.c_uint64(0)
    assert _capi.load_host().pathed_host_job_seed(str(job_path).encode(), C.byref(value)) == 0 and value.value == 1
    assert seed_from_job(job) == 1


@pytest.mark.parametrize("text", REFUSED)
def test_a_seed_that_cannot_be_read_exactly_is_refused_by_name_in_both_hosts(tmp_path, text):
    from pathed_amd import _capi
    from pathed_amd.integrator import PathedError, seed_from_job
    out_dir = str(tmp_path / "out")
    job_path = tmp_path / "job.json"
    job_path.write_text(_job_text(text, out_dir))
    wording = "job: \"seed\" must be an integer in [0, 2^64), written in plain digits"

    # the C++ host: before it touches the output directory (and before any GPU call)
    exe = os.path.join(_capi.REPO_ROOT, "pathed_amd", "bin", "pathed")
    result = subprocess.run([exe, str(job_path), _capi.REPO_ROOT], capture_output=True, text=True, cwd=str(tmp_path))
    assert result.returncode != 0 and wording in result.stderr, result.stdout + result.stderr
    assert not os.path.exists(out_dir)
    host = _capi.load_host()
    assert host.pathed_host_job_seed(str(job_path).encode(), None) == 1 and wording in host.pathed_host_last_error().decode()

    # run_job's reader: the same values, the same words ("+7" is no JSON to Python's parser: refused one step earlier)
    if text == "+7":
        with pytest.raises(ValueError):
            json.load(open(job_path))
        return
    with pytest.raises(PathedError) as caught:
        seed_from_job(json.load(open(job_path)))
    assert str(caught.value) == wording


@pytest.mark.parametrize("seed", [-1, 1 << 64, (1 << 64) + 1, -(1 << 63), 1.0, 1.5, "1", None, True])
def test_the_python_wrappers_refuse_a_seed_outside_the_range(seed):
    """_seed is what every HipScene.render* call, render_pixels and render_adaptive pass their seed through (on a scene:
    tests/test_gpu_argument_edges.py), and PathTracer checks its own at construction."""
    from pathed_amd import integrator
    with pytest.raises(integrator.PathedError, match=r"seed must be an integer in \[0, 2\^64\)"):
        integrator._seed(seed)
    with pytest.raises(integrator.PathedError, match=r"seed must be an integer in \[0, 2\^64\)"):
        integrator.PathTracer(integrator.BounceController(0, 4), seed=seed)


def test_the_python_wrappers_accept_the_whole_range():
    import numpy as np
    from pathed_amd import integrator
    for seed in (0, 1, (1 << 53) + 1, 1 << 63, (1 << 64) - 1, np.uint64((1 << 64) - 1), np.int32(7)):
        assert integrator._seed(seed) == int(seed)
    assert integrator.PathTracer(integrator.BounceController(0, 4), seed=(1 << 64) - 1).seed == (1 << 64) - 1


def test_json_numbers_keep_their_exact_unsigned_value():
    """Json::parse then Json::dump: report.json holds the seed as written.  A double holds 2^53 + 1 as 2^53 and 2^64 - 1 as
    2^64; numbers that are not plain digits keep going through the double, as before."""
    from pathed_amd import _capi
    host = _capi.load_host()

    def round_trip(text):
        out = C.create_string_buffer(4096)
        assert host.pathed_host_json_round_trip(text.encode(), out, len(out)) == 0, host.pathed_host_last_error()
        return out.value.decode()

    for text in ("18446744073709551615", "9007199254740993", "0"):
        assert round_trip(text) == text
        assert json.loads(round_trip("{\"seed\": %s, \"spp\": 16}" % text)) == {"seed": int(text), "spp": 16}
    assert round_trip("[9007199254740993, -3, 2.5, 1e3]").split() == ["[", "9007199254740993,", "-3,", "2.5,", "1000", "]"]
    assert float(round_trip("18446744073709551616")) == 2.0 ** 64      # over the range: a double, as before
