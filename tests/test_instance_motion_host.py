"""Moving placements (include/pathed_hip.h: pathed_hip_scene_set_instance_transforms), the part that
needs no GPU:

1. the three entry points are declared, bound and exported
2. pathed_amd.instances.placement_box / prototype_box / pad_box are, bit for bit, the boxes scene creation hands the builder,
   and instance_inverse the inverse it stores -- through a small host program that calls the library's own placementBox and
   instanceInverse (instances.h) and the builder's Box and padBox (bvh_build.h) with the library's flags
3. InstanceSet.set_transforms keeps the set, and with it flatten_instances, in step
4. k_instance_records, k_refit_top_pass and k_placement_boxes: compile-only, no scratch, the registers written down on the day, names the
   symbol counts of test_kernel_resources.py do not see
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pathed_amd import _capi, flatten_instances
from pathed_amd import instances as I

import instances_scene as S
from test_instance_kernel_resources import EXISTING_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

NEW_SYMBOLS = ("pathed_hip_scene_set_instance_transforms", "pathed_hip_scene_set_instance_transforms_device", "pathed_hip_debug_instance_records")


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ 1. ABI

def test_the_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pathed_hip.h")).read()
    assert re.search(r"int pathed_hip_scene_set_instance_transforms\(PathedScene \*scene, const float \*transforms, uint32_t n_instances, float \*device_ms\);", header)
    assert re.search(r"int pathed_hip_scene_set_instance_transforms_device\(PathedScene \*scene, const float \*d_transforms, uint32_t n_instances, float \*device_ms\);", header)
    assert re.search(r"int pathed_hip_debug_instance_records\(PathedScene \*scene, float \*records[^,]*, size_t n_instances\);", header)
    assert re.search(r"#define PATHED_ABI_VERSION 4\b", header)   # two new functions, no struct changes: the version stays
    lib = C.CDLL(_capi.hip_library_path())
    for name in NEW_SYMBOLS:
        assert name in _capi.HIP_SYMBOLS and hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------------------- 2. box rule

BOX_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "instances.h"
using namespace pathed;
using namespace pathed::bvh_detail;
// stdin: int32 nPoints, nPoints * 3 floats (a prototype's corners), int32 nTransforms, nTransforms * 12 floats
// stdout: the prototype's padded box (6 floats), then per transform the placement's world box and the node's copy (12 floats),
// whether instanceInverse accepts the transform (one float, 1 or 0) and the inverse it wrote (12 floats)
int main()
{
    int nPoints = 0, nTransforms = 0;
    if (fread(&nPoints, 4, 1, stdin) != 1) { return 1; }
    std::vector<float> points((size_t)3 * nPoints);
    if (fread(points.data(), 4, points.size(), stdin) != points.size()) { return 1; }
    if (fread(&nTransforms, 4, 1, stdin) != 1) { return 1; }
    std::vector<float> transforms((size_t)12 * nTransforms);
    if (fread(transforms.data(), 4, transforms.size(), stdin) != transforms.size()) { return 1; }
    Box proto;
    proto.reset();
    for (int i = 0; i < nPoints; i++) { proto.grow(&points[(size_t)3 * i], &points[(size_t)3 * i]); }
    float lo[3], hi[3];
    padBox(proto, lo, hi);
    fwrite(lo, 4, 3, stdout);
    fwrite(hi, 4, 3, stdout);
    for (int k = 0; k < nTransforms; k++) {
        const float *m = &transforms[(size_t)12 * k];
        Box placed;
        placementBox(m, lo, hi, placed.lo, placed.hi);   // the statement the library and its kernels run
        float nodeLo[3], nodeHi[3];
        padBox(placed, nodeLo, nodeHi);
        fwrite(placed.lo, 4, 3, stdout);
        fwrite(placed.hi, 4, 3, stdout);
        fwrite(nodeLo, 4, 3, stdout);
        fwrite(nodeHi, 4, 3, stdout);
        float inverse[12] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        const float accepted = instanceInverse(m, inverse) ? 1.f : 0.f;
        fwrite(&accepted, 4, 1, stdout);
        fwrite(inverse, 4, 12, stdout);
    }
    return 0;
}
"""


def box_rule_transforms():
    """the placements of the instancing tests plus random rotations, shears, mirrors, tiny and huge scales, far translations"""
    rng = np.random.default_rng(41)
    out = [t for _, t in S.GENERAL_PLACEMENTS] + [t for _, t in S.EXACT_PLACEMENTS]
    for k in range(200):
        linear = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3)
        out.append(S.affine(linear, rng.normal(size=3) * 10.0 ** rng.uniform(-2, 4)))
    out.append(S.affine(np.eye(3), (0.0, 0.0, 0.0)))
    out.append(S.affine(-np.eye(3), (3.0, 2.0, 1.0)))     # corners that land on zero, with either sign
    return np.stack(out).astype(np.float32)


def test_the_numpy_box_rule_is_the_builders(tmp_path):
    compiler = shutil.which("g++") or shutil.which("c++")
    if compiler is None:
        pytest.skip("no host compiler")
    source = tmp_path / "box_rule.cpp"
    source.write_text(BOX_PROGRAM)
    program = tmp_path / "box_rule"
    built = subprocess.run([compiler, "-std=c++17", "-O2", "-ffp-contract=off", "-march=x86-64-v3", "-iquote", os.path.join(ROOT, "pathed_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "include"), str(source), "-o", str(program), "-lpthread"], capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-2000:]
    transforms = box_rule_transforms()
    for centre, radius in (((3.0, 2.0, 1.0), 1.0), ((-3.0, 1.0, 2.0), 0.7), ((0.0, 0.0, 0.0), 1.0), ((500.0, -0.25, 1e-3), 0.01)):
        points, _, _, _ = S.icosphere(centre, radius, subdivisions=1)
        payload = np.int32(len(points)).tobytes() + points.astype(np.float32).tobytes() + np.int32(len(transforms)).tobytes() + transforms.tobytes()
        result = subprocess.run([str(program)], input=payload, capture_output=True, timeout=60)
        assert result.returncode == 0
        words = np.frombuffer(result.stdout, dtype=np.float32)
        assert len(words) == 6 + 25 * len(transforms)
        proto_lo, proto_hi = I.prototype_box(points)
        assert np.array_equal(bits(proto_lo), bits(words[0:3])) and np.array_equal(bits(proto_hi), bits(words[3:6]))
        rows = words[6:].reshape(len(transforms), 25)
        for transform, row in zip(transforms, rows):
            lo, hi = I.placement_box(transform, proto_lo, proto_hi)
            assert np.array_equal(bits(lo), bits(row[0:3])) and np.array_equal(bits(hi), bits(row[3:6])), transform
            node_lo, node_hi = I.pad_box(lo, hi)
            assert np.array_equal(bits(node_lo), bits(row[6:9])) and np.array_equal(bits(node_hi), bits(row[9:12])), transform
            assert np.all(node_lo <= lo) and np.all(node_hi >= hi)
            # the inverse: numpy's is the library's bit for bit, and they refuse the same transforms
            try:
                inverse = I.instance_inverse(transform)
            except ValueError:
                inverse = None
            assert (inverse is not None) == (row[12] == 1.0), transform
            if inverse is not None:
                assert np.array_equal(bits(inverse), bits(row[13:25])), transform


# ------------------------------------------------------------------------------------------------------- 3. the Python set

def test_the_instance_set_follows_new_transforms():
    built, pointer, prototypes, placements = S.build(S.GENERAL_PLACEMENTS, 16, 16)
    moved = [(prototype, transform) for (prototype, _), (_, transform) in zip(S.GENERAL_PLACEMENTS, reversed(S.GENERAL_PLACEMENTS))]
    instance_set = I.InstanceSet(prototypes, placements)
    instance_set.set_transforms(np.stack([t for _, t in moved]).reshape(-1, 3, 4))
    assert [p for p, _ in instance_set.instances] == [p for p, _ in S.GENERAL_PLACEMENTS]
    for k, (_, transform) in enumerate(moved):
        assert np.array_equal(bits(instance_set.instances[k][1]), bits(transform))
        assert np.array_equal(bits(np.array(instance_set.desc.instances[k].transform[:], dtype=np.float32)), bits(transform))
        assert instance_set.desc.instances[k].prototype == moved[k][0]
    fresh = flatten_instances(pointer, prototypes, moved)
    again = flatten_instances(pointer, None, instance_set)
    assert np.array_equal(bits(fresh.positions), bits(again.positions)) and np.array_equal(fresh.indices, again.indices)
    with pytest.raises(ValueError):
        instance_set.set_transforms(np.zeros((2, 12), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------- 4. the new kernels

PROBE = """
#include "pathed_hip.h"
#include "bvh_build.h"
#include "kernels.h"
namespace pathed {
__global__ void probe_anchor(const float *t, int n, const float4 *live, float4 *staged, unsigned int *bad, float4 *nodes, int topNodes, const float4 *boxes,
                             float4 *lo, float4 *hi, const unsigned char *in, unsigned char *out)
{
}
void probe_launch(const float *t, int n, const float4 *live, float4 *staged, unsigned int *bad, float4 *nodes, int topNodes, const float4 *boxes,
                  float4 *lo, float4 *hi, const unsigned char *in, unsigned char *out)
{
    hipLaunchKernelGGL(k_instance_records, dim3(1), dim3(kBlock), 0, nullptr, t, n, live, staged, bad);
    hipLaunchKernelGGL(k_refit_top_pass, dim3(1), dim3(kBlock), 0, nullptr, nodes, topNodes, live, n, boxes, 1, lo, hi, in, out);
    hipLaunchKernelGGL(k_placement_boxes, dim3(1), dim3(kBlock), 0, nullptr, live, n, boxes, 1, lo);
}
}
"""

# what hipcc (ROCm 7, gfx950, the library's flags) reported on the day the kernels were written: see DESIGN.md section 4.6d
RECORDS_VGPRS, RECORDS_WAVES = 61, 8      # the double-precision cofactors and nine quotients
TOP_PASS_VGPRS, TOP_PASS_WAVES = 73, 6    # 24 box words, four children's records and corners in flight
BOXES_VGPRS, BOXES_WAVES = 39, 8          # one record's rows, one prototype box, the corners in flight


def test_the_new_kernels_and_their_budgets(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    compiler = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    source = tmp_path / "motion_probe.hip"
    source.write_text(PROBE)
    result = subprocess.run(
        [compiler, "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Iinclude", "-iquote", "pathed_amd/csrc",
         "-mllvm", "-instcombine-max-copied-from-constant-users=4000", "-Rpass-analysis=kernel-resource-usage",
         "-c", str(source), "-o", str(tmp_path / "motion_probe.o")],
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
    records = {k: v for k, v in usage.items() if "18k_instance_records" in k}
    top_pass = {k: v for k, v in usage.items() if "16k_refit_top_pass" in k}
    boxes = {k: v for k, v in usage.items() if "17k_placement_boxes" in k}
    assert len(records) == 1 and len(top_pass) == 1 and len(boxes) == 1, sorted(usage)
    for kernel_name in list(records) + list(top_pass) + list(boxes):
        assert not any(re.search(pattern, kernel_name) for pattern in EXISTING_PATTERNS), kernel_name
    print("k_instance_records %s, k_refit_top_pass %s, k_placement_boxes %s" % (list(records.values())[0], list(top_pass.values())[0], list(boxes.values())[0]))
    for found, cap, waves in ((records, RECORDS_VGPRS, RECORDS_WAVES), (top_pass, TOP_PASS_VGPRS, TOP_PASS_WAVES), (boxes, BOXES_VGPRS, BOXES_WAVES)):
        value = list(found.values())[0]
        assert value["ScratchSize"] == 0 and value["VGPRs"] <= cap and value["Occupancy"] >= waves, value


def test_the_library_holds_the_new_kernels():
    blob = open(_capi.hip_library_path(), "rb").read()
    for name in (b"18k_instance_records", b"16k_refit_top_pass"):
        assert name in blob, name
