"""The never-hit rule of the fused kernel's pass over all items and the pass list it drives (pathed_amd/csrc/small_items.h:
smallNeverHit, buildSmallPassItems) on the host: a stand-alone program (tests/duplicate_items_host.cpp) builds random rooms in
which some triangles are copied bit for bit -- a triple, a copy with another material, an emitting copy of a non-emitting
triangle, a copy whose quad partner is not copied -- beside what is NOT a copy: rotated and reversed vertex order, one ulp off,
-0 for +0, records holding a NaN.  The triangles reach the rule in a shuffled order (the primitive id decides who stays).  Every
case is asserted on the marks; the pass list is a permutation of the kept triangles that keeps quads together and puts the
never-occluders last; and over 10^5 random rays per room plus rays through the copied triangles' corners and edges the closest
hit by the intersector's acceptance rule over ALL triangles equals the one over the pass list in (t, u, v, prim) bits, occlusion
likewise.  Then the Cornell file (exactly primitives 20, 21, 32, 33; 32 triangles as 15 parallelograms and 2 lone triangles, 6
shadow pair turns and no lone one), a scene without copies (byte-identical lists) and the emitter case (a wall with an emitting
copy of a triangle in its plane is no never-occluder of the pass).  Built plainly and with the address and undefined-behaviour
sanitizers.  CPU only."""
import os
import subprocess

import pytest

from pathed_amd import _capi


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_a_copy_changes_no_hit_and_the_pass_list_leaves_it_out(tmp_path, flags):
    exe = str(tmp_path / "duplicate_items_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                    "-iquote", os.path.join(_capi.REPO_ROOT, "pathed_amd", "csrc"),
                    os.path.join(_capi.REPO_ROOT, "tests", "duplicate_items_host.cpp"), "-o", exe], check=True)
    # (10^5 random rays per room in both builds; the sanitized one over fewer rooms)
    result = subprocess.run([exe, "3" if flags else "8", "100000", os.path.join(_capi.REPO_ROOT, "scenes", "CornellBox-Original.obj")],
                            capture_output=True, text=True)
    print(result.stdout[-3000:], result.stderr[-3000:])
    assert result.returncode == 0
    assert "failures 0 mismatches 0" in result.stdout
