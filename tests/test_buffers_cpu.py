"""The owning buffers' failure contract (csrc/rc_common.h: DevBuf / PinBuf), with host sanitizers.

tools/buffer_check.cpp is a stand-alone program: built here with AddressSanitizer and
UndefinedBehaviorSanitizer on its host code and run as a process of its own.  On a host without a
GPU every allocation fails, which is what the program expects: a failed reserve throws RC_ERR_OOM
and leaves an empty buffer, and a recorded workspace size reads 0.  The success paths are
test_buffers_gpu.py's.
"""
import os
import subprocess

import pytest

from conftest import PKG_NAME, REPO, gpu_available

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_buffer_check_under_sanitizers(tmp_path):
    if gpu_available():
        pytest.skip("buffer_check expects every allocation to fail: a host without a device")
    exe = str(tmp_path / "buffer_check")
    build = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-g", "-O1",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
             "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, PKG_NAME, "csrc"),
             os.path.join(REPO, "tools", "buffer_check.cpp"), "-o", exe]
    r = subprocess.run(build, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)  # its own process: the sanitizer runtime is linked in
    assert r.returncode == 0, r.stdout + r.stderr
    assert "buffer_check: ok" in r.stdout
