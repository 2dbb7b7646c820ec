#!/usr/bin/env python3
"""Device time of MATLAB's bicubic imresize (sr_imresize_u8, U8 output) on a 200 MP RGB canvas (17320 x 11550 x 3) at 1/2, 1/4
and 1/8, and on a 12.5 MP image (4330 x 2887 x 3) at x 4, beside OpenCV's INTER_CUBIC resize (sr_resize_cubic_u8: four taps
per axis whatever the scale, no antialiasing -- less arithmetic, another result) on the same buffers to the same sizes, and
the device's copy rate (the copy_ of tools/hbm_rw_probe.py, 600 MB) in the same process.  Warm-up 2, then 7 repetitions with
the calls alternating, timed with HIP events (the library's own per-family pairs around the launch); median and minimum, and
GB/s of algorithmic bytes: the source read once plus the destination written once.  Writes profiles/imresize_timing.json (or
the path given as the first argument).
usage (GPU box): python tools/imresize_timing.py [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    sys.path.insert(0, p)
import numpy as np            # noqa: E402
import _native                # noqa: E402

WARM, RUNS = 2, 7
OUT = sys.argv[1] if len(sys.argv) >= 2 else os.path.join(ROOT, "profiles", "imresize_timing.json")
BIG, SMALL = (11550, 17320), (2887, 4330)
ctx = _native.default_context(0)


def noisy(h, w):
    """An h x w x 3 image in HBM: a smooth pattern with noise, resized up on the device from a tenth of the size."""
    rng = np.random.default_rng(1)
    sh, sw = max(h // 10, 8), max(w // 10, 8)
    yy, xx = np.mgrid[0:sh, 0:sw]
    small = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (sh, sw, 3)),
                    0, 255).astype(np.uint8)
    src, dst = ctx.upload(small), ctx.alloc(h * w * 3)
    ctx.resize_cubic_u8(src.ptr, sw * 3, sh, sw, 3, dst.ptr, w * 3, h, w)
    ctx.sync()
    src.free()
    return dst


def med_min(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}


def copy_rate():
    import torch
    n = 600 * 1000 * 1000 // 4
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    y.copy_(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 10
    del x, y
    torch.cuda.empty_cache()
    return {"bytes_each_way": n * 4, "ms": round(ms, 4), "gb_per_s_read_plus_write": round(2 * n * 4 / ms / 1e6, 1)}


cases = []
for name, (h, w), scale in (("200MP_half", BIG, 1 / 2), ("200MP_quarter", BIG, 1 / 4), ("200MP_eighth", BIG, 1 / 8), ("12.5MP_x4", SMALL, 4)):
    cases.append((name, h, w, scale, _native.imresize_size(h, scale), _native.imresize_size(w, scale)))
bufs = {BIG: noisy(*BIG), SMALL: noisy(*SMALL)}
res = {"copy": copy_rate(), "cases": {}}
for name, h, w, scale, dh, dw in cases:
    src, dst = bufs[(h, w)], ctx.alloc(dh * dw * 3)

    def run_imresize():
        ctx.imresize(src.ptr, w * 3, h, w, 3, scale, scale, dst.ptr, dw * 3, dh, dw)

    def run_cubic():
        ctx.resize_cubic_u8(src.ptr, w * 3, h, w, 3, dst.ptr, dw * 3, dh, dw)
        ctx.sync()

    calls = [("imresize", run_imresize, "imresize"), ("inter_cubic", run_cubic, "resize_cubic")]
    for _ in range(WARM):
        for _, fn, _ in calls:
            fn()
    ctx.sync()
    dev = {n: [] for n, _, _ in calls}
    ctx.prof_enable(True)
    for r in range(RUNS):
        for k in range(len(calls)):
            n, fn, family = calls[(k + r) % len(calls)]
            ctx.prof_reset()
            fn()
            ctx.sync()
            dev[n].append(ctx.prof_get()[family][0])
    ctx.prof_enable(False)
    nbytes = h * w * 3 + dh * dw * 3
    plan = _native.imresize_plan(h, w, 3, scale, scale, dh, dw)
    res["cases"][name] = {"source": [h, w, 3], "scale": scale, "destination": [dh, dw, 3], "algorithmic_bytes": nbytes, "plan": plan,
                          "device": {n: med_min(v) for n, v in dev.items()},
                          "gb_per_s": {n: round(nbytes / statistics.median(v) / 1e6, 1) for n, v in dev.items()}}
    dst.free()
for b in bufs.values():
    b.free()
res["method"] = (f"warm-up {WARM}, {RUNS} repetitions with the two calls alternating, HIP events (sr_prof) around each call's launch, "
                 "median and minimum; gb_per_s = (source bytes + destination bytes) over the median device time; copy = torch's "
                 "copy_ of 600 MB, 10 repetitions, bytes read plus bytes written over the mean time, in the same process")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
