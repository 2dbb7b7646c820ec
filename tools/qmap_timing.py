#!/usr/bin/env python3
"""Device time of the per-cell quality map (sr_quality_map_u8, cell 256) against the fused global assessment
(sr_assess_u8, the unchanged yardstick) on one 200 MP pair (17320 x 11550 x 3) with the same flags -- SSE + UNIFORM7 +
GAUSS11 -- on the same buffers.  The pair is made on the device (two small noisy images through sr_resize_cubic_u8): the
times do not depend on the pixel values.  Warm-up 2, then 7 runs timed with HIP events (the library's own per-family event
pairs), median and minimum reported, and the wall time of the synchronous map call (workspace allocation, readback and free
included).  Writes profiles/qmap_timing.json.
usage (GPU box): python tools/qmap_timing.py [W H]"""
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
CELL = 256
FLAGS = _native.ASSESS_SSE | _native.ASSESS_UNIFORM7 | _native.ASSESS_GAUSS11
ctx = _native.default_context(0)


def big(seed):
    rng = np.random.default_rng(seed)
    h, w = max(H // 10, 8), max(W // 10, 8)
    yy, xx = np.mgrid[0:h, 0:w]
    small = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (h, w, 3)),
                    0, 255).astype(np.uint8)
    src, dst = ctx.upload(small), ctx.alloc(H * W * 3)
    ctx.resize_cubic_u8(src.ptr, w * 3, h, w, 3, dst.ptr, W * 3, H, W)
    ctx.sync()
    src.free()
    return dst


def events(fn, family):
    for _ in range(WARM):
        fn()
    ctx.sync()
    dev, wall = [], []
    ctx.prof_enable(True)
    ctx.prof_select(family)
    for _ in range(RUNS):
        ctx.prof_reset()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(ctx.prof_get()[family][0])
    ctx.prof_select(None)
    ctx.prof_enable(False)
    return dev, wall


def med_min(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}


a, b = big(1), big(2)
xe, ye = list(range(0, W, CELL)) + [W], list(range(0, H, CELL)) + [H]
box = {}


def run_map():
    box["map"] = ctx.quality_map_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, xe, ye, flags=FLAGS)


def run_assess():
    box["assess"] = ctx.assess_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, flags=FLAGS)


assess_dev, assess_wall = events(run_assess, "assess_all")
map_dev, map_wall = events(run_map, "qmap")
m, g = box["map"], box["assess"]
assert int(m["sse"].sum()) == int(round(g["sse"]))                       # the two computed the same thing
for k in ("ssim_uniform", "ssim_gauss"):
    assert abs(m[k].sum() - g[k]) <= 1e-9 * abs(g[k]), k
ratio = statistics.median(map_dev) / statistics.median(assess_dev)
res = {"image": [H, W, 3], "cell": CELL, "grid": [len(ye) - 1, len(xe) - 1], "flags": "SSE | UNIFORM7 | GAUSS11",
       "quality_map_u8": {"device": med_min(map_dev), "wall": med_min(map_wall)},
       "assess_u8": {"device": med_min(assess_dev), "wall": med_min(assess_wall)},
       "device_ratio_map_over_assess": round(ratio, 3),
       "method": f"warm-up {WARM}, {RUNS} runs, HIP events (sr_prof) around the kernels of each call, median and minimum; wall = "
                 "the synchronous call as the host sees it"}
a.free(); b.free()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "qmap_timing.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
