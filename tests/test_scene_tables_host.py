"""The host stages of scene creation (pathed_amd/csrc/scene_tables.h) without a GPU: a stand-alone program
(tests/scene_tables_host.cpp) checks the option validation (for every field the last accepted and the first refused value on
both ends, the exact message, and with two fields wrong the message of the one checked first), the environment tables on maps
of 1 x 1, 2 x 1, 3 x 2 and 8 x 4 texels with a black row, a black map, one bright texel and equal texels (CDFs non-decreasing
and ending at 1, guides and record windows against a linear search, the -1 marker exactly on the empty rows), the light list's
order, the plain ranges (merge, skip, the ninth dropped), the media tables, the gamma texels, the packed small-scene records
with both centres of a sphere light, and the large-triangle split on 200 random soups (areas and total against a plain double
recomputation, every vertex of the rest inside the padded box and sphere).  The header compiles on its own; the program is
built plainly and with the address and undefined-behaviour sanitizers.  CPU only."""
import os
import subprocess

import pytest

from pathed_amd import _capi

INCLUDES = ["-iquote", os.path.join(_capi.REPO_ROOT, "pathed_amd", "csrc"), "-I" + os.path.join(_capi.REPO_ROOT, "include")]


def test_the_header_compiles_on_its_own(tmp_path):
    unit = tmp_path / "only_the_header.cpp"
    unit.write_text('#include "scene_tables.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *INCLUDES, "-fsyntax-only", str(unit)], check=True)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_stages_of_scene_creation(tmp_path, flags):
    exe = str(tmp_path / "scene_tables_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, *INCLUDES,
                    os.path.join(_capi.REPO_ROOT, "tests", "scene_tables_host.cpp"), "-o", exe], check=True)
    result = subprocess.run([exe], capture_output=True, text=True)
    print(result.stdout[-3000:], result.stderr[-3000:])
    assert result.returncode == 0
    assert "failures 0" in result.stdout
