"""The kernels of the shutter (instance_motion.h: k_trace_instanced_motion, k_shade_instanced_motion,
k_trace_rays_instanced_motion, k_motion_boxes) exist with the expected instantiations, under names the symbol counts of
test_kernel_resources.py do not see.  Compile-only: a translation unit that instantiates just these kernels with the library's
flags; hipcc reports the usage per kernel.  The figures are printed and written down in DESIGN.md section 4.6d "Shutter"; what is
asserted is that every kernel runs (occupancy >= 1).

On the day they were written (ROCm 7, gfx950): k_trace_instanced_motion 107 VGPRs (111 counting), no scratch, 4 waves per SIMD
(k_trace_instanced: 90 / 94, 5 waves); k_shade_instanced_motion 106 VGPRs (104 environment-only), no scratch, 4 waves;
k_trace_rays_instanced_motion 95 VGPRs, 5 waves; k_motion_boxes 71 VGPRs, 7 waves."""
import os
import re
import shutil
import subprocess

import pytest

from test_instance_kernel_resources import EXISTING_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

PROBE = """
#include "pathed_hip.h"
#include "bvh_build.h"
#include "kernels.h"
namespace pathed {
template __global__ void k_trace_instanced_motion<8, false>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_instanced_motion<16, false>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_instanced_motion<22, false>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_instanced_motion<8, true>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_instanced_motion<16, true>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_instanced_motion<22, true>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_trace_rays_instanced_motion<8>(DScene, DInstanceSet, DMotionSet, const float4 *, const float *, int, int, float4 *, int *, int *, int);
template __global__ void k_trace_rays_instanced_motion<16>(DScene, DInstanceSet, DMotionSet, const float4 *, const float *, int, int, float4 *, int *, int *, int);
template __global__ void k_trace_rays_instanced_motion<22>(DScene, DInstanceSet, DMotionSet, const float4 *, const float *, int, int, float4 *, int *, int *, int);
template __global__ void k_shade_instanced_motion<true, false>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_shade_instanced_motion<true, true>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_shade_instanced_motion<false, false>(RenderParams, DInstanceSet, DMotionSet);
template __global__ void k_shade_instanced_motion<false, true>(RenderParams, DInstanceSet, DMotionSet);
void probe_launch(const float *close, int n, const float4 *live, const float4 *protoBoxes, float4 *rows, int *moving, float4 *records, float4 *table, unsigned int *bad)
{
    hipLaunchKernelGGL(k_motion_boxes, dim3(1), dim3(kBlock), 0, nullptr, close, n, live, protoBoxes, 1, 0.f, 1.f, rows, moving, records, table, bad);
}
}
"""


def test_the_shutter_kernels_and_their_resources(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    compiler = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    source = tmp_path / "shutter_probe.hip"
    source.write_text(PROBE)
    result = subprocess.run(
        [compiler, "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Iinclude", "-iquote", "pathed_amd/csrc",
         "-mllvm", "-instcombine-max-copied-from-constant-users=4000", "-Rpass-analysis=kernel-resource-usage",
         "-c", str(source), "-o", str(tmp_path / "shutter_probe.o")],
        cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert result.returncode == 0, result.stderr[-2000:]
    usage, name = {}, None
    for line in result.stderr.splitlines():
        found = re.search(r"Function Name: (\S+)", line)
        if found:
            name = found.group(1)
            usage[name] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            value = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if value and name:
                usage[name][key.split(" ")[0]] = int(value.group(1))
    trace = {k: v for k, v in usage.items() if "24k_trace_instanced_motionI" in k}
    hook = {k: v for k, v in usage.items() if "29k_trace_rays_instanced_motionI" in k}
    shade = {k: v for k, v in usage.items() if "24k_shade_instanced_motionI" in k}
    boxes = {k: v for k, v in usage.items() if "14k_motion_boxes" in k}
    assert len(trace) == 6 and len(hook) == 3 and len(shade) == 4 and len(boxes) == 1, sorted(usage)
    for kernel_name, figures in sorted({**trace, **hook, **shade, **boxes}.items()):
        print(kernel_name, figures)
        assert not any(re.search(pattern, kernel_name) for pattern in EXISTING_PATTERNS), kernel_name
        assert figures["Occupancy"] >= 1, (kernel_name, figures)


def test_the_library_holds_the_shutter_kernels():
    from pathed_amd import _capi
    blob = open(_capi.hip_library_path(), "rb").read()
    for name in (b"24k_trace_instanced_motionILi8ELb0E", b"24k_trace_instanced_motionILi16ELb0E", b"24k_trace_instanced_motionILi22ELb0E",
                 b"24k_trace_instanced_motionILi22ELb1E", b"29k_trace_rays_instanced_motionILi8E", b"29k_trace_rays_instanced_motionILi22E",
                 b"24k_shade_instanced_motionILb1ELb0E", b"24k_shade_instanced_motionILb0ELb1E", b"14k_motion_boxes"):
        assert name in blob, name
