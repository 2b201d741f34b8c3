"""The grid instantiations of the volume kernel (kernels.h: k_path_volume_grid) in the code object of the built library:
they exist, their registers and scratch are the figures DESIGN.md states (§4, "Voxel-grid media"), and grid support added no
instantiation of k_path_volume itself.  Read from the AMDGPU metadata notes of libpathed_hip.so's gfx950 code objects (what
the compiler reports as kernel-resource-usage, tests/test_kernel_resources.py, without compiling again)."""
import os
import re
import shutil
import subprocess

import pytest

from pathed_amd import _capi

LLVM_BIN = "/opt/rocm/llvm/bin"
GRID_KERNELS = {   # <STACK, SMALL>: (VGPRs, scratch bytes per lane), as in DESIGN.md
    "k_path_volume_gridILi8ELb1EE": (128, 448),
    "k_path_volume_gridILi8ELb0EE": (128, 464),
    "k_path_volume_gridILi16ELb0EE": (128, 464),
    "k_path_volume_gridILi22ELb0EE": (128, 464),
}


def tool(name):
    path = os.path.join(LLVM_BIN, name)
    if not os.path.exists(path):
        path = shutil.which(name)
    if not path:
        pytest.skip("no %s" % name)
    return path


def kernel_metadata(tmp_path):
    """{symbol: (vgpr_count, private_segment_fixed_size)} over every gfx950 code object of the library"""
    fat = tmp_path / "fatbin"
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=%s" % fat, _capi.hip_library_path(), str(tmp_path / "copy.so")], check=True)
    raw = fat.read_bytes()
    starts = [found.start() for found in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", raw)] + [len(raw)]   # one bundle per translation unit
    assert len(starts) >= 2
    kernels = {}
    for i in range(len(starts) - 1):
        bundle, code = tmp_path / ("bundle%d" % i), tmp_path / ("code%d.co" % i)
        bundle.write_bytes(raw[starts[i]:starts[i + 1]])
        subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=%s" % bundle, "--output=%s" % code], check=True)
        notes = subprocess.run([tool("llvm-readelf"), "--notes", str(code)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            symbol = re.search(r"\.symbol:\s+'?(\S+?)\.kd", block).group(1)
            kernels[symbol] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    return kernels


def test_grid_instantiations_and_their_resources(tmp_path):
    kernels = kernel_metadata(tmp_path)
    assert len(kernels) > 300
    grid = {name: usage for name, usage in kernels.items() if "18k_path_volume_gridI" in name}
    print(grid)
    assert len(grid) == len(GRID_KERNELS)
    for tag, expected in GRID_KERNELS.items():
        found = [usage for name, usage in grid.items() if tag in name]
        assert found == [expected], (tag, found, expected)
    # the kernel of scenes without a grid: the eleven instantiations the launch ladder had before grids (the count
    # tests/test_kernel_resources.py holds), none of them with grid code
    plain = [name for name in kernels if "13k_path_volumeI" in name]
    assert len(plain) == 11, plain
    assert any("14k_grid_queries" in name for name in kernels)
