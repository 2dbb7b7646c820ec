"""AddressSanitizer + UBSan over the host side of the Swin2SR backend: csrc/sr_swin2sr_host.cpp (and csrc/sr_swinir_host.cpp, whose
ranges, reconstruction tables, extent rule and plan it reuses) is compiled with g++ -fsanitize=address,undefined
-fno-sanitize-recover=all together with the stand-alone tools/sanitize/swin2sr_driver.cpp, which takes the Swin2SR descriptions
and every refusal through the description check, the table list, the table check of a create, the plan and the two host tables
(the continuous position bias and the clamped logit scale) with exact-size buffers, and run as a program of its own: nothing is
preloaded, nothing loaded into Python is sanitised, nothing runs on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_swin2sr_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "super-resolution-system_amd", "csrc")
    exe = str(tmp_path / "swin2sr_driver")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-DSR_BUILD", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tools", "sanitize", "swin2sr_driver.cpp"),
           os.path.join(csrc, "sr_swin2sr_host.cpp"), os.path.join(csrc, "sr_swinir_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "swin2sr-driver-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
