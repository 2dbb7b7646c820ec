#!/usr/bin/env python3
"""Device time of HaarPSI (sr_haarpsi_u8: both conventions, with and without subsampling) beside the SR-benchmark PSNR / SSIM
(sr_bench_u8, SR_BENCH_Y) and GMSD (sr_gmsd_u8, SR_BENCH_Y) on the same buffers in the same process, on one 200 MP RGB pair
(17320 x 11550 x 3): a noisy image resized on the device and its bicubic partner (down to a quarter and back up), the pair
stage 4 sees; no crop.  The calls alternate in one run.  Warm-up 2, then 7 repetitions timed with HIP events (the library's own
per-family event pairs: each covers the call's launch and the reduction of its partials), median and minimum reported, and
the wall time of each synchronous call.  Writes profiles/haarpsi_timing.json (or the path given as the third argument).
usage (GPU box): python tools/haarpsi_timing.py [W H [out.json]]"""
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
OUT = sys.argv[3] if len(sys.argv) >= 4 else os.path.join(ROOT, "profiles", "haarpsi_timing.json")
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
Y = _native.BENCH_Y


def haarpsi(name, sub, conv):
    return (name, lambda: box.__setitem__(name, ctx.haarpsi(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, sub, conv)), "haarpsi")


CALLS = [haarpsi("haarpsi", True, "matlab"), haarpsi("haarpsi_python", True, "python"), haarpsi("haarpsi_full", False, "matlab"),
         ("gmsd", lambda: box.__setitem__("gmsd", ctx.gmsd_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, Y)), "gmsd"),
         ("bench_y", lambda: box.__setitem__("bench_y", ctx.bench_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, Y)), "srbench")]
for _ in range(WARM):
    for _, fn, _ in CALLS:
        fn()
ctx.sync()
dev = {n: [] for n, _, _ in CALLS}
wall = {n: [] for n, _, _ in CALLS}
ctx.prof_enable(True)
for r in range(RUNS):                                    # rotated: no call always runs first or after the same neighbour
    for k in range(len(CALLS)):
        name, fn, family = CALLS[(k + r) % len(CALLS)]
        ctx.prof_reset()
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
        ctx.sync()
        dev[name].append(ctx.prof_get()[family][0])
ctx.prof_enable(False)
bench, gmsd = statistics.median(dev["bench_y"]), statistics.median(dev["gmsd"])
HP = [n for n in dev if n.startswith("haarpsi")]
res = {"image": [H, W, 3], "crop_border": 0,
       "plan": {n: _native.haarpsi_plan(H, W, 3, 0, n != "haarpsi_full") for n in ("haarpsi", "haarpsi_full")},
       "values": {**{n: _native.haarpsi_value(box[n]) for n in HP}, "gmsd": _native.gmsd_value(box["gmsd"]),
                  "bench_y": dict(zip(("psnr", "ssim"), _native.bench_values(box["bench_y"])))},
       "device": {n: med_min(dev[n]) for n in dev}, "wall": {n: med_min(wall[n]) for n in wall},
       "ratio_over_bench_y": {n: round(statistics.median(dev[n]) / bench, 3) for n in HP + ["gmsd"]},
       "ratio_over_gmsd": {n: round(statistics.median(dev[n]) / gmsd, 3) for n in HP},
       "input_gb_per_s": {n: round(2 * H * W * 3 / (statistics.median(dev[n]) * 1e-3) / 1e9, 1) for n in dev},
       "method": f"warm-up {WARM}, {RUNS} rotated repetitions, HIP events (sr_prof) around each call's launch and reduction, "
                 "median and minimum; wall = the synchronous call as the host sees it; input_gb_per_s = both images' bytes once "
                 "over the median device time"}
a.free(); b.free()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
