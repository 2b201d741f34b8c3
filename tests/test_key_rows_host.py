"""The inner keys of the random stream that k_path_small_single draws from (shading.h: fillKeyRow, drawFromRow, RowRng,
KeySlots) on the host: a stand-alone program (tests/key_rows_host.hip, host side only, no HIP call) checks a draw from a
filled row against Rng::next() bit for bit -- 10^6 random (k0, k1, vertex, column) and the corners --, a whole vertex's
sequence, the table layout and the two-table bookkeeping; once plain and once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")],
                         ids=["plain", "sanitized"])
def test_rows_draw_what_the_generator_draws(tmp_path, flags):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    compiler = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    exe = str(tmp_path / "key_rows_host")
    build = subprocess.run(
        [compiler, "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-Iinclude", "-iquote", "pathed_amd/csrc", *flags,
         os.path.join("tests", "key_rows_host.hip"), "-o", exe],
        cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "1000000 random draws, 0 failures" in run.stdout
