"""The per-pixel cull rule of the camera-ray candidate masks (pathed_amd/csrc/camera_masks.h) on the host: a stand-alone
program (tests/camera_masks_host.cpp) drives the very function the device builder calls against a double-precision ray /
triangle test, on random cameras, pixels and triangles -- corners within 1e-6 of a side plane, edges whose plane passes within
1e-6 of a corner ray of the pixel, triangles behind the camera and across its plane.  Built plainly and with the address and undefined-behaviour sanitizers.  CPU only."""
import os
import subprocess

import pytest

from pathed_amd import _capi


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_cull_rule_never_loses_a_triangle_a_footprint_ray_meets(tmp_path, flags):
    exe = str(tmp_path / "camera_masks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                    "-iquote", os.path.join(_capi.REPO_ROOT, "pathed_amd", "csrc"),
                    os.path.join(_capi.REPO_ROOT, "tests", "camera_masks_host.cpp"), "-o", exe], check=True)
    result = subprocess.run([exe, "20000" if flags else "40000"], capture_output=True, text=True)
    print(result.stdout[-2000:], result.stderr[-2000:])
    assert result.returncode == 0
    assert "violations 0" in result.stdout
