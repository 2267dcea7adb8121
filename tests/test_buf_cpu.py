"""The worker's owning buffer types (csrc/ifa_buf.h) as a stand-alone program under the address and undefined-behaviour
sanitizers: tests/buf_selftest.cc over malloc-backed spaces (moves, failed allocations, half-built pairs, nothing live at scope exit)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_buffer_types_selftest_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "inferflow_amd", "csrc"), os.path.join(ROOT, "tests", "buf_selftest.cc"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "buf_selftest ok" in r.stdout
