"""AddressSanitizer + UBSan over the host side of DISTS: csrc/sr_dists_host.cpp is compiled with g++
-fsanitize=address,undefined -fno-sanitize-recover=all together with the stand-alone tools/sanitize/dists_driver.cpp, which
takes seeded sums (dead, constant and equal channels included) through the sizes and the score with exact-size buffers and walks
the per-tile plans of csrc/sr_vgg_ranges.h (AlexNet, VGG16 and DISTS stacks, small and odd sizes, every tile), and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_dists_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "super-resolution-system_amd", "csrc")
    exe = str(tmp_path / "dists_driver")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-DSR_BUILD", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tools", "sanitize", "dists_driver.cpp"),
           os.path.join(csrc, "sr_dists_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "dists-driver-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
