"""The host arithmetic of instanced scenes (pathed_amd/csrc/instances.h) without a GPU: a stand-alone program
(tests/instances_host.cpp) checks every refusal of an instanced description (the code, the exact message, and with two things
wrong the message of the check that comes first), the inverse, the record and the box rule on hand-computed values, and the
two-level tree of four scenes -- two world triangles with a 20-triangle prototype under an identity, a turned and scaled and a
mirrored placement; an empty world with one placement; a world without prototypes; a 64 x 64 grid of a one-triangle prototype:
every reference inside its arrays, every placement and every world triangle in exactly one leaf, the prototypes inside their
own ranges behind the top tree, quad 6 of every record, the ascending bases, the stack bound, and every placed corner
(flattened in fp32, as the device does) inside the child box of its placement's leaf.  The header compiles on its own; the
program is built plainly and with the address and undefined-behaviour sanitizers.  CPU only."""
import os
import subprocess

import pytest

from pathed_amd import _capi

INCLUDES = ["-iquote", os.path.join(_capi.REPO_ROOT, "pathed_amd", "csrc"), "-I" + os.path.join(_capi.REPO_ROOT, "include")]


def test_the_header_compiles_on_its_own(tmp_path):
    unit = tmp_path / "only_the_header.cpp"
    unit.write_text('#include "instances.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *INCLUDES, "-fsyntax-only", str(unit)], check=True)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_arithmetic_of_instanced_scenes(tmp_path, flags):
    exe = str(tmp_path / "instances_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, *INCLUDES,
                    os.path.join(_capi.REPO_ROOT, "tests", "instances_host.cpp"), "-o", exe, "-lpthread"], check=True)
    result = subprocess.run([exe], capture_output=True, text=True)
    print(result.stdout[-3000:], result.stderr[-3000:])
    assert result.returncode == 0
    assert "failures 0" in result.stdout
