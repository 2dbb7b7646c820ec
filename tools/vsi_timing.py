#!/usr/bin/env python3
"""Device time of VSI (sr_vsi_u8) beside FSIM (sr_fsim_u8) and the SR-benchmark PSNR / SSIM (sr_bench_u8, SR_BENCH_Y) on the
same buffers in the same process, on one 200 MP RGB pair (17320 x 11550 x 3): a noisy coloured image resized on the device and
its bicubic partner (down to a quarter and back up), the pair stage 4 sees.  The three calls alternate in one run.  Warm-up 2,
then 7 repetitions timed with HIP events (the library's own per-family event pairs: vsi_shrink the antialiased resize of both
images to the 256 x 256 grid, vsi_sdsp Lab, the 24 dense transforms and the saliency, vsi_expand the up-resize with its min /
max over every sample and the pooled window sums, vsi_pool the one pass over the pair, vsi_score the score kernel and its
reduction), median and minimum reported, the wall time of each synchronous call, and the GB/s of the three full-resolution
passes beside the rate of a device-to-device copy of one image in the same process.  Writes profiles/vsi_timing.json (or the
path given as the third argument).
usage (GPU box): python tools/vsi_timing.py [W H [out.json]]"""
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
OUT = sys.argv[3] if len(sys.argv) >= 4 else os.path.join(ROOT, "profiles", "vsi_timing.json")
ctx = _native.default_context(0)


def pair():
    rng = np.random.default_rng(1)
    h, w = max(H // 10, 8), max(W // 10, 8)
    yy, xx = np.mgrid[0:h, 0:w]
    small = np.clip(np.stack([128 + 64 * np.sin(xx / 37.0), 120 + 48 * np.cos(yy / 23.0), 90 + 100.0 * xx / w], axis=2) +
                    rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
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
PARTS = ["vsi_shrink", "vsi_sdsp", "vsi_expand", "vsi_pool", "vsi_score"]
FPARTS = ["fsim_pool", "fsim_dft", "fsim_median", "fsim_rest"]
CALLS = [("vsi", lambda: box.__setitem__("vsi", ctx.vsi(a.ptr, W * 3, b.ptr, W * 3, H, W, 3)), PARTS),
         ("fsim", lambda: box.__setitem__("fsim", ctx.fsim_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3)), FPARTS),
         ("bench_y", lambda: box.__setitem__("bench_y", ctx.bench_u8(a.ptr, W * 3, b.ptr, W * 3, H, W, 3, 0, _native.BENCH_Y)),
          ["srbench"])]
for _ in range(WARM):
    for _, fn, _ in CALLS:
        fn()
ctx.sync()
dev = {}
wall = {n: [] for n, _, _ in CALLS}
ctx.prof_enable(True)
for r in range(RUNS):
    for k in range(len(CALLS)):
        name, fn, families = CALLS[(k + r) % len(CALLS)]
        ctx.prof_reset()
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
        ctx.sync()
        got = ctx.prof_get()
        if name == "bench_y":
            dev.setdefault("bench_y", []).append(got["srbench"][0])
            continue
        for fam in families:
            dev.setdefault(fam, []).append(got[fam][0])
        dev.setdefault(name, []).append(sum(got[fam][0] for fam in families))
ctx.prof_enable(False)
# the process's own copy rate: one image, device to device, read + written bytes over the wall time between two syncs
spare = ctx.alloc(H * W * 3)
copy_ms = []
for _ in range(WARM + RUNS):
    ctx.sync()
    t0 = time.perf_counter()
    ctx.copy_d2d(spare.ptr, a.ptr, H * W * 3)
    ctx.sync()
    copy_ms.append(1e3 * (time.perf_counter() - t0))
copy_ms = copy_ms[WARM:]
spare.free()
gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
bench = statistics.median(dev["bench_y"])
plan = _native.vsi_plan(H, W, 3)
img = H * W * 3
res = {"image": [H, W, 3], "F": plan["F"], "pooled": list(plan["size"]), "workspace_bytes": plan["workspace_bytes"],
       "values": {"vsi": _native.vsi_value(box["vsi"]), "fsim": _native.fsim_value(box["fsim"])[0],
                  "bench_y": dict(zip(("psnr", "ssim"), _native.bench_values(box["bench_y"])))},
       "device": {n: med_min(dev[n]) for n in dev}, "wall": {n: med_min(wall[n]) for n in wall},
       "ratio_over_bench_y": {n: round(statistics.median(dev[n]) / bench, 3) for n in ("vsi", "fsim")},
       "ratio_over_fsim": round(statistics.median(dev["vsi"]) / statistics.median(dev["fsim"]), 3),
       "gb_per_s": {"shrink_u8_read_twice": gbs(2 * 2 * img, statistics.median(dev["vsi_shrink"])),
                    "expand_samples_as_f64": gbs(2 * H * W * 8, statistics.median(dev["vsi_expand"])),
                    "pool_u8_read_once": gbs(2 * img, statistics.median(dev["vsi_pool"])),
                    "copy_d2d_read_plus_write": gbs(2 * img, statistics.median(copy_ms))},
       "method": f"warm-up {WARM}, {RUNS} alternating repetitions, HIP events (sr_prof) around each family's launches, median and "
                 "minimum; vsi / fsim = the sum of the call's families in each repetition; wall = the synchronous call as the "
                 "host sees it; shrink: both images' bytes twice (neighbouring windows overlap twofold) over the family's median; "
                 "expand: 8 bytes per full-resolution sample of both maps (formed in registers, never stored) over the family's "
                 "median, a rate of samples, not of memory traffic; pool: both images' bytes once; copy: one image read and "
                 "written, wall time between two syncs"}
a.free(); b.free()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
