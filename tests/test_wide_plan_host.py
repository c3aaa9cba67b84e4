"""The wide path's host-side plan arithmetic, checked on the CPU: tests/host/wide_plan_check.cpp (a stand-alone program
with its own main) calls pc_plan over a sweep of one-block shapes and asserts that hk_pcond's LDS regions are ordered
and inside the carve, that d_cond_DCtd's integer bookkeeping (6 T + 2 ng2 ints at the start of LDS) stays below the
stage table, and that the deferred cross terms are on only where it also stays below the BAbt tile; three shapes are
pinned by hand, and make_layout's stage offsets are compared with the sums written out.  The program is compiled with
the address and undefined-behaviour sanitizers (host code only) and run; no GPU is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_wide_plan_check(tmp_path):
    exe = str(tmp_path / "wide_plan_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "host", "wide_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout, r.stdout
