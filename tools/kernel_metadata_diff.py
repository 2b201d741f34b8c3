#!/usr/bin/env python3
"""Compare the gfx950 code-object metadata of two builds of libpathed_hip.so, kernel by kernel: VGPRs, AGPRs, SGPRs, scratch
(private segment), LDS (group segment), spills and the waves-per-SIMD that follow from the registers.  A change that adds
kernels must leave every other kernel's row alone.

    tools/kernel_metadata_diff.py other/libpathed_hip.so [pathed_amd/lib/libpathed_hip.so]

Prints the kernels only one side has, then every kernel whose row differs; exit status 1 when a shared kernel differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def waves_per_simd(vgprs, agprs):
    """gfx950: 512 unified registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    total = max(1, -(-(vgprs + agprs) // 8) * 8)
    return min(8, 512 // total)


def metadata(library):
    kernels = {}
    with tempfile.TemporaryDirectory() as scratch:
        fat = os.path.join(scratch, "fatbin")
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", ".hip_fatbin=%s" % fat, library, os.path.join(scratch, "copy.so")], check=True)
        raw = open(fat, "rb").read()
        starts = [found.start() for found in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", raw)] + [len(raw)]
        for i in range(len(starts) - 1):
            bundle, code = os.path.join(scratch, "bundle%d" % i), os.path.join(scratch, "code%d.co" % i)
            open(bundle, "wb").write(raw[starts[i]:starts[i + 1]])
            subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--input=%s" % bundle, "--output=%s" % code], check=True)
            notes = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", code], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                block = ".agpr_count" + block
                symbol = re.search(r"\.symbol:\s+'?(\S+?)\.kd", block).group(1)
                row = {}
                for field in FIELDS:
                    found = re.search(r"\.%s:\s+(\d+)" % field, block)
                    row[field] = int(found.group(1)) if found else None
                row["waves_per_simd"] = waves_per_simd(row["vgpr_count"] or 0, row["agpr_count"] or 0)
                kernels[symbol] = row
    return kernels


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    other = metadata(sys.argv[1])
    this = metadata(sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "pathed_amd", "lib", "libpathed_hip.so"))
    print("kernels: %d there, %d here" % (len(other), len(this)))
    for name in sorted(set(other) - set(this)):
        print("only there: %s" % name)
    for name in sorted(set(this) - set(other)):
        print("only here:  %s %s" % (name, this[name]))
    changed = [name for name in sorted(set(this) & set(other)) if this[name] != other[name]]
    for name in changed:
        print("differs:    %s\n    there %s\n    here  %s" % (name, other[name], this[name]))
    print("%d shared kernels, %d differ" % (len(set(this) & set(other)), len(changed)))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
