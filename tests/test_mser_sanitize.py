"""AddressSanitizer + UBSan over the host side of MSER: csrc/sr_mser_host.cpp is compiled with g++
-fsanitize=address,undefined -fno-sanitize-recover=all together with the stand-alone tools/sanitize/mser_driver.cpp, which takes
the plan through sizes up to the largest an int holds and every refusal, checks the layout as the kernels use it, holds the
host tree of exact-size heap images (dense and strided, every channel count, both polarities) to a flood-fill evaluation of
the definition, checks the regions' order and short-buffer behaviour and the text-box filter at its edges, and run as a
program of its own: nothing is preloaded, nothing loaded into Python is sanitised, nothing runs on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_mser_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "super-resolution-system_amd", "csrc")
    exe = str(tmp_path / "mser_driver")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-DSR_BUILD", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tools", "sanitize", "mser_driver.cpp"), os.path.join(csrc, "sr_mser_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "mser-driver-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
