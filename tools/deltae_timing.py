#!/usr/bin/env python3
"""Device time of the colour difference (sr_delta_e_u8: CIEDE2000 and CIE76 sums, each with and without the dense float64
map; sr_delta_e_cells_u8 at the pipeline's default cell of 256) beside the SR-benchmark PSNR / SSIM (sr_bench_u8 in
SR_BENCH_Y) on the same buffers in the same process, on one 200 MP RGB pair (17320 x 11550 x 3): a noisy image resized on the
device and its bicubic partner (down to a quarter and back up), the pair stage 4 sees; no crop.  The calls alternate in one
run.  Warm-up 2, then 7 repetitions timed with HIP events (the library's own per-family event pairs: deltae covers the
histogram clear, the sums launch and the finishing launch; deltae_cells the column launch and the cell launch; srbench its
launch and reduction), median and minimum reported, and the wall time of each synchronous call.  Writes
profiles/deltae_timing.json (or the path given as the third argument).
usage (GPU box): python tools/deltae_timing.py [W H [out.json]]"""
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
OUT = sys.argv[3] if len(sys.argv) >= 4 else os.path.join(ROOT, "profiles", "deltae_timing.json")
CELL = 256
ctx = _native.default_context(0)


def pair():
    rng = np.random.default_rng(1)
    h, w = max(H // 10, 8), max(W // 10, 8)
    yy, xx = np.mgrid[0:h, 0:w]
    small = np.clip(np.stack([128 + 64 * np.sin(xx / 37.0 + c) + 48 * np.cos(yy / 23.0 - c) for c in range(3)], -1)
                    + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
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
dmap = ctx.alloc(H * W * 8)
box = {}
XE, YE = list(range(0, W, CELL)) + [W], list(range(0, H, CELL)) + [H]


def sums(name, formula, with_map):
    def fn():
        box[name] = ctx.delta_e_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, formula, d_map=dmap.ptr if with_map else 0,
                                   map_stride=W * 8 if with_map else 0)
    return name, fn, "deltae"


CALLS = [sums("de00", _native.DELTA_E_2000, False), sums("de00_map", _native.DELTA_E_2000, True),
         sums("de76", _native.DELTA_E_76, False), sums("de76_map", _native.DELTA_E_76, True),
         ("de00_cells", lambda: box.__setitem__("de00_cells", ctx.delta_e_cells_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, XE, YE)),
          "deltae_cells"),
         ("bench_y", lambda: box.__setitem__("bench_y", ctx.bench_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, _native.BENCH_Y)),
          "srbench")]
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
bench = statistics.median(dev["bench_y"])
rec = box["de00"]
mean, rms = _native.delta_e_mean_rms(rec)
cells = box["de00_cells"]
res = {"image": [H, W, 3], "crop_border": 0, "cell": CELL, "grid": [len(YE) - 1, len(XE) - 1],
       "scratch_bytes": _native.delta_e_plan(H, W, 3)["scratch_bytes"], "blocks": _native.delta_e_plan(H, W, 3)["blocks"],
       "values": {"de00": {"mean": mean, "rms": rms, "max": rec["max"], "p50": _native.delta_e_percentile(rec, 50),
                           "p99": _native.delta_e_percentile(rec, 99), "frac_above_1": _native.delta_e_fraction(rec, 1.0),
                           "byte_equal_fraction_at_most": float(rec["hist"][0]) / rec["count"]},
                  "de76_mean": _native.delta_e_mean_rms(box["de76"])[0],
                  "cells_sum_over_sum": float(cells["sum"].sum()) / rec["sum"], "cells_max_equals_max": bool(cells["max"].max() == rec["max"]),
                  "map_changes_no_bit": bool(box["de00_map"]["sum"] == rec["sum"] and np.array_equal(box["de00_map"]["hist"], rec["hist"])),
                  "bench_y": dict(zip(("psnr", "ssim"), _native.bench_values(box["bench_y"])))},
       "device": {n: med_min(dev[n]) for n in dev}, "wall": {n: med_min(wall[n]) for n in wall},
       "ratio_over_bench_y": {n: round(statistics.median(dev[n]) / bench, 3) for n in dev if n != "bench_y"},
       "ns_per_pixel": {n: round(statistics.median(dev[n]) * 1e6 / (H * W), 4) for n in dev},
       "input_gb_per_s": {n: round(2 * H * W * 3 / (statistics.median(dev[n]) * 1e-3) / 1e9, 1) for n in dev},
       "method": f"warm-up {WARM}, {RUNS} rotated repetitions, HIP events (sr_prof) around each call's launches, median and "
                 "minimum; wall = the synchronous call as the host sees it; input_gb_per_s = both images' bytes once over the "
                 "median device time (the map variants also write 8 bytes per pixel)"}
a.free(); b.free(); dmap.free()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
