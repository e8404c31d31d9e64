"""CPU: tests/native/ctx_check.hip -- the option table row by row and, where no device is present, every grow site's
behaviour when its allocation fails -- built into a temporary directory and run.  About a minute, all of it hipcc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")
def test_ctx_check(tmp_path):
    exe = str(tmp_path / "ctx_check")
    # (the flags of minbpe_amd/build.py: the program includes the library's host side, kernels and all)
    build = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-pthread",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "minbpe_amd", "csrc"),
                            os.path.join(ROOT, "tests", "native", "ctx_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "57 options" in run.stdout and "0 failures" in run.stdout, run.stdout
