"""AddressSanitizer + UBSan over the host side of VSI: csrc/sr_vsi_host.cpp and the two host units it calls
(sr_imresize_host.cpp, sr_fsim_host.cpp) are compiled with g++ -fsanitize=address,undefined -fno-sanitize-recover=all together
with the stand-alone tools/sanitize/vsi_driver.cpp, which takes plans, axis and band tables, LG / SD (exact-size buffers), the
values and the whole host metric through shapes on both sides of every threshold and every refusal, and checks each plan as
the kernels use it, and run as a program of its own: nothing is preloaded, nothing loaded into Python is sanitised, nothing
runs on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_vsi_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "super-resolution-system_amd", "csrc")
    exe = str(tmp_path / "vsi_driver")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-DSR_BUILD", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tools", "sanitize", "vsi_driver.cpp"), os.path.join(csrc, "sr_vsi_host.cpp"),
           os.path.join(csrc, "sr_imresize_host.cpp"), os.path.join(csrc, "sr_fsim_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "vsi-driver-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
