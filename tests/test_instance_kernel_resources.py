"""The kernels of instanced scenes (kernels.h: k_trace_instanced, k_trace_rays_instanced, k_shade_instanced) exist beside the
persistent kernels, under names the symbol counts of test_kernel_resources.py do not see, and keep the resources they were
written down with.  Compile-only: a translation unit that instantiates just these kernels (and k_shade, for comparison), with
the library's flags; hipcc reports the usage per kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

PROBE = """
#include "pathed_hip.h"
#include "bvh_build.h"
#include "kernels.h"
namespace pathed {
template __global__ void k_trace_instanced<8, false>(RenderParams, DInstanceSet);
template __global__ void k_trace_instanced<16, false>(RenderParams, DInstanceSet);
template __global__ void k_trace_instanced<22, false>(RenderParams, DInstanceSet);
template __global__ void k_trace_instanced<8, true>(RenderParams, DInstanceSet);
template __global__ void k_trace_instanced<16, true>(RenderParams, DInstanceSet);
template __global__ void k_trace_instanced<22, true>(RenderParams, DInstanceSet);
template __global__ void k_trace_rays_instanced<8>(DScene, DInstanceSet, const float4 *, int, int, float4 *, int *, int *, int);
template __global__ void k_trace_rays_instanced<16>(DScene, DInstanceSet, const float4 *, int, int, float4 *, int *, int *, int);
template __global__ void k_trace_rays_instanced<22>(DScene, DInstanceSet, const float4 *, int, int, float4 *, int *, int *, int);
template __global__ void k_shade_instanced<true, false>(RenderParams, DInstanceSet);
template __global__ void k_shade_instanced<true, true>(RenderParams, DInstanceSet);
template __global__ void k_shade_instanced<false, false>(RenderParams, DInstanceSet);
template __global__ void k_shade_instanced<false, true>(RenderParams, DInstanceSet);
template __global__ void k_shade<true, false, TraitsAll>(RenderParams);
}
"""

# the patterns tests/test_kernel_resources.py selects and counts kernels with
EXISTING_PATTERNS = [r"k_shadeILb1", r"k_shade_env", r"k_traceILi\d+ELb[01]ELb0ELb[01]", r"k_trace_smallILb0",
                     r"12k_path_smallI", r"13k_path_volumeI", r"11k_path_waveI", r"7k_traceI", r"k_path_hybrid"]


def usage_of_the_probe(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    compiler = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    source = tmp_path / "instanced_probe.hip"
    source.write_text(PROBE)
    result = subprocess.run(
        [compiler, "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Iinclude", "-iquote", "pathed_amd/csrc",
         "-mllvm", "-instcombine-max-copied-from-constant-users=4000", "-Rpass-analysis=kernel-resource-usage",
         "-c", str(source), "-o", str(tmp_path / "instanced_probe.o")],
        cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert result.returncode == 0, result.stderr[-2000:]
    usage, name = {}, None
    for line in result.stderr.splitlines():
        found = re.search(r"Function Name: (\S+)", line)
        if found:
            name = found.group(1)
            usage[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]"):
            value = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if value and name:
                usage[name][key.split(" ")[0]] = int(value.group(1))
    return usage


def test_the_instanced_kernels_and_their_budgets(tmp_path):
    usage = usage_of_the_probe(tmp_path)
    trace = {k: v for k, v in usage.items() if "17k_trace_instancedI" in k}
    hook = {k: v for k, v in usage.items() if "22k_trace_rays_instancedI" in k}
    shade = {k: v for k, v in usage.items() if "17k_shade_instancedI" in k}
    assert len(trace) == 6 and len(hook) == 3 and len(shade) == 4, sorted(usage)
    # names the existing selections and symbol counts do not match
    for name in list(trace) + list(hook) + list(shade):
        assert not any(re.search(pattern, name) for pattern in EXISTING_PATTERNS), name
    # k_shade_instanced spills nothing, as k_shade does (its flatten branch costs registers, not scratch: 116 VGPRs against 104)
    plain = [v for k, v in usage.items() if "7k_shadeILb1ELb0E" in k]
    assert len(plain) == 1 and plain[0]["ScratchSize"] == 0 and plain[0]["VGPRs"] <= 104, plain
    assert all(v["ScratchSize"] == 0 and v["VGPRs"] <= 116 and v["Occupancy"] >= 4 for v in shade.values()), shade
    # the trace kernel as written down on the day it was added: 90 VGPRs (94 with the counters), no scratch, five waves per
    # SIMD -- 23.5 KiB of LDS stack rows per block allow six blocks per CU, so the registers bound the occupancy
    plain_trace = [v for k, v in trace.items() if k.endswith("ELb0EEEvNS_12RenderParamsENS_12DInstanceSetE")]
    counting = [v for k, v in trace.items() if k.endswith("ELb1EEEvNS_12RenderParamsENS_12DInstanceSetE")]
    assert len(plain_trace) == 3 and all(v["VGPRs"] <= 90 and v["ScratchSize"] == 0 and v["Occupancy"] >= 5 for v in plain_trace), trace
    assert len(counting) == 3 and all(v["VGPRs"] <= 94 and v["ScratchSize"] == 0 for v in counting), trace
    assert all(v["VGPRs"] <= 78 and v["ScratchSize"] == 0 for v in hook.values()), hook


def test_the_library_holds_the_instanced_kernels():
    from pathed_amd import _capi
    blob = open(_capi.hip_library_path(), "rb").read()
    for name in (b"17k_trace_instancedILi8ELb0E", b"17k_trace_instancedILi16ELb0E", b"17k_trace_instancedILi22ELb0E",
                 b"17k_trace_instancedILi22ELb1E", b"22k_trace_rays_instancedILi22E", b"17k_shade_instancedILb1ELb0E", b"17k_shade_instancedILb0ELb1E"):
        assert name in blob, name
