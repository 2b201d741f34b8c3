"""The never-occluder rule of the fused kernel's shadow rays and the item order it drives (pathed_amd/csrc/small_items.h:
smallNeverOccluders, buildSmallItems) on the host: a stand-alone program (tests/never_occluders_host.cpp) builds random rooms --
walls exactly in, within eta of, or a little beyond a supporting plane of the scene, objects inside, emitters at distances
spread around Dmin (at least a third of the walls within a factor 2 of it, so the rule cannot pass by marking nothing) -- and
casts 10^5 segments per marked triangle, from points on the scene's triangles (corners and shared edges over-represented,
displaced by up to eta along the normal) to points on the emitters: in double precision none may meet the marked triangle at
t in (tnear / 2, distance - 1e-3 + 1e-5].  Then the Cornell file (exactly floor, back wall, right wall and the two left-wall
triangles), an environment light (nothing), an odd count of occluder quads (the straddling pair runs for both rays), and the
order as a permutation that keeps a quad's triangles adjacent.  Built plainly and with the address and undefined-behaviour
sanitizers.  CPU only."""
import os
import subprocess

import pytest

from pathed_amd import _capi


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_no_segment_to_a_light_meets_a_never_occluder(tmp_path, flags):
    exe = str(tmp_path / "never_occluders_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                    "-iquote", os.path.join(_capi.REPO_ROOT, "pathed_amd", "csrc"),
                    os.path.join(_capi.REPO_ROOT, "tests", "never_occluders_host.cpp"), "-o", exe], check=True)
    # (10^5 segments per marked triangle in both builds; the sanitized one over fewer rooms)
    result = subprocess.run([exe, "12" if flags else "60", "100000", os.path.join(_capi.REPO_ROOT, "scenes", "CornellBox-Original.obj")],
                            capture_output=True, text=True)
    print(result.stdout[-3000:], result.stderr[-3000:])
    assert result.returncode == 0
    assert "failures 0 violations 0" in result.stdout
