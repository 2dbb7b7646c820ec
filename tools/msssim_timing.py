#!/usr/bin/env python3
"""Device time of the 5-scale MS-SSIM (sr_ms_ssim_u8) against the single-scale Gaussian SSIM (sr_ssim_u8 mode 'gauss', the
unchanged fused assessment kernel) on one 200 MP pair (17320 x 11550 x 3): a noisy image resized on the device and its
bicubic partner (down to a quarter and back up), the pair stage 4 sees.  The two calls alternate in one run.  Warm-up 2, then
7 repetitions timed with HIP events (the library's own per-family event pairs: msssim_l0 .. msssim_l4 cover each level's
launch with its reduction, assess_all the single-scale call), median and minimum reported, and the wall time of both
synchronous calls.  Writes profiles/msssim_timing.json (or the path given as the third argument).
usage (GPU box): python tools/msssim_timing.py [W H [out.json]]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    sys.path.insert(0, p)
import numpy as np            # noqa: E402
import _native                # noqa: E402

WARM, RUNS = 2, 7
W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) >= 3 else (17320, 11550)
OUT = sys.argv[3] if len(sys.argv) >= 4 else os.path.join(ROOT, "profiles", "msssim_timing.json")
LEVELS = 5
ctx = _native.default_context(0)


def pair():
    rng = np.random.default_rng(1)
    h, w = max(H // 10, 8), max(W // 10, 8)
    yy, xx = np.mgrid[0:h, 0:w]
    small = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (h, w, 3)),
                    0, 255).astype(np.uint8)
    src, a, b = ctx.upload(small), ctx.alloc(H * W * 3), ctx.alloc(H * W * 3)
    q = ctx.alloc((H // 4) * (W // 4) * 3)
    ctx.resize_cubic_u8(src.ptr, w * 3, h, w, 3, a.ptr, W * 3, H, W)
    ctx.resize_cubic_u8(a.ptr, W * 3, H, W, 3, q.ptr, (W // 4) * 3, H // 4, W // 4)
    ctx.resize_cubic_u8(q.ptr, (W // 4) * 3, H // 4, W // 4, 3, b.ptr, W * 3, H, W)
    ctx.sync()
    src.free(); q.free()
    return a, b


def med_min(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}


a, b = pair()
box = {}


def run_ms():
    box["ms"] = ctx.ms_ssim_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, levels=LEVELS)


def run_ss():
    box["ss"] = ctx.ssim_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, "gauss")


for _ in range(WARM):
    run_ms(); run_ss()
ctx.sync()
names = [f"msssim_l{j}" for j in range(LEVELS)]
dev = {n: [] for n in names + ["ms_ssim_u8", "ssim_u8_gauss"]}
wall = {"ms_ssim_u8": [], "ssim_u8_gauss": []}
ctx.prof_enable(True)
for _ in range(RUNS):                                    # alternated: neither call always runs first or on a warmer chip
    ctx.prof_reset()
    t0 = time.perf_counter()
    run_ms()
    wall["ms_ssim_u8"].append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    run_ss()
    wall["ssim_u8_gauss"].append(1e3 * (time.perf_counter() - t0))
    ctx.sync()
    rec = ctx.prof_get()
    for n in names:
        dev[n].append(rec[n][0])
    dev["ms_ssim_u8"].append(sum(rec[n][0] for n in names))
    dev["ssim_u8_gauss"].append(rec["assess_all"][0])
ctx.prof_enable(False)
ms, (s1, n1) = box["ms"], box["ss"]
assert ms[0][2] == n1 and abs(ms[0][0] - s1) <= 1e-9 * abs(s1)          # level 0 is the single-scale sum
plan = _native.ms_ssim_plan(H, W, LEVELS)
pixels = [hh * ww for hh, ww in plan["sizes"]]
ratio = statistics.median(dev["ms_ssim_u8"]) / statistics.median(dev["ssim_u8_gauss"])
res = {"image": [H, W, 3], "levels": LEVELS, "level_sizes": plan["sizes"], "scratch_bytes": plan["scratch_bytes"],
       "value": _native.ms_ssim_value(ms), "s": [r[0] / r[2] for r in ms], "cs": [r[1] / r[2] for r in ms],
       "ms_ssim_u8": {"device": med_min(dev["ms_ssim_u8"]), "wall": med_min(wall["ms_ssim_u8"])},
       "per_level_device": {n: med_min(dev[n]) for n in names},
       "ssim_u8_gauss": {"device": med_min(dev["ssim_u8_gauss"]), "wall": med_min(wall["ssim_u8_gauss"])},
       "device_ratio_ms_over_single": round(ratio, 3),
       "level0_over_single": round(statistics.median(dev["msssim_l0"]) / statistics.median(dev["ssim_u8_gauss"]), 3),
       "structural_expectation": {"pixel_ratio": round(sum(pixels) / pixels[0], 4),
                                  "note": "4/3 of the pixels, one more accumulated map (cs), 4 bytes stored per level-1 pixel"},
       "method": f"warm-up {WARM}, {RUNS} alternated repetitions, HIP events (sr_prof) around each level's launch and reduction, "
                 "median and minimum; the whole call = the sum of its levels; wall = the synchronous call as the host sees it"}
a.free(); b.free()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
