"""The budget of k_path_small_single (kernels.h), the launch the headline runs on: four waves per SIMD at 128 VGPRs, no more
scratch than the instantiation of k_path_small it stands in for had when it was split off (84 bytes per lane), and static LDS
that leaves room for four blocks per CU beside the material table of a scene that pairs triangles (64 materials).
Compile-only, device side only, of a translation unit that holds kernels.h alone: its non-template kernels are all it emits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_budget_of_the_single_sample_kernel(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    compiler = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    source = tmp_path / "probe.hip"
    source.write_text('#include "pathed_hip.h"\n#include "bvh_build.h"\n#include "kernels.h"\n')
    result = subprocess.run(
        [compiler, "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Iinclude", "-iquote", "pathed_amd/csrc",
         "-mllvm", "-instcombine-max-copied-from-constant-users=4000", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-c", str(source), "-o", str(tmp_path / "probe.o")],
        cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert result.returncode == 0, result.stderr[-2000:]
    usage = {}
    name = None
    for line in result.stderr.splitlines():
        found = re.search(r"Function Name: (\S+)", line)
        if found:
            name = found.group(1)
            usage[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            value = re.search(key + r": (\d+)", line)
            if value and name:
                usage[name][key.split(" ")[0]] = int(value.group(1))
    single = [v for k, v in usage.items() if "k_path_small_single" in k]
    assert len(single) == 1, sorted(usage)
    single = single[0]
    print(single)
    assert single["VGPRs"] <= 128 and single["Occupancy"] == 4, single
    assert single["ScratchSize"] <= 84, single
    assert single["LDS"] + 64 * 96 <= 160 * 1024 // 4, single
