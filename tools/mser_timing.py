#!/usr/bin/env python3
"""Time of MSER text-region detection (csrc/sr_mser.hip), both polarities, default parameters, on images resident in HBM:
the 1080 x 720 BASELINE source, and at 4096 x 4096 a smooth-plus-noise image, a flat image (the single-root atomic worst
case) and a two-level image.  Per input: the synchronous call (median of 7, after one warm-up; it holds the three host
synchronisations of each polarity), the device time of each kernel family from hipEvent pairs (sr_prof_*: sort = gray +
histogram + scatter; note / union / create / accum = the four launches of a level; select), the launches per call, the node
and region counts (the call is one execution of the detection whatever the count: the tool asserts four level launches per
non-empty level and polarity) and the workspace per pixel; beside them, in the same process, sr_mser_host_u8 on one
host thread and sr_saliency_u8 on the same image (what create_forbidden_zone_map already pays).
usage (GPU box): python tools/mser_timing.py > profiles/mser_timing.json"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np                       # noqa: E402
import _native                           # noqa: E402
from _mser_ref import baseline_source, gray_swapped    # noqa: E402

ctx = _native.default_context(0)
REPS = 7


def smooth_noise(n):
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    base = 128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0)
    return np.clip(base + rng.integers(-12, 13, size=(n, n)), 0, 255).astype(np.uint8)


def two_level(n):
    """Dark discs of radius 10 on a 32-pixel grid, jittered, over a bright page: many components that merge in one level."""
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:n, 0:n]
    cy = (yy // 32) * 32 + 16
    cx = (xx // 32) * 32 + 16
    jit = rng.integers(-4, 5, size=(n // 32 + 1, n // 32 + 1, 2))
    dy = yy - cy - jit[yy // 32, xx // 32, 0]
    dx = xx - cx - jit[yy // 32, xx // 32, 1]
    return np.where(dy * dy + dx * dx <= 100, 30, 220).astype(np.uint8)


def median_ms(fn):
    fn()
    ctx.sync()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(ts), 3)


def run(name, img):
    h, w = img.shape[:2]
    cn = img.shape[2] if img.ndim == 3 else 1
    d = ctx.upload(np.ascontiguousarray(img))
    call = lambda: ctx.mser(d.ptr, w * cn, h, w, cn)
    call_ms = median_ms(call)
    ctx.prof_enable(True)
    ctx.prof_reset()
    regs = call()
    ctx.sync()
    prof = ctx.prof_get()
    ctx.prof_enable(False)
    ctx.prof_reset()
    kern = {k: round(ms, 3) for k, (ms, _) in prof.items() if k.startswith("ms_")}
    level_launches = sum(n for k, (_, n) in prof.items() if k in ("ms_note", "ms_union", "ms_create", "ms_accum"))
    levels = len(np.unique(gray_swapped(img)))
    # one execution: four launches per non-empty level and polarity (Context.mser never runs the detection twice)
    assert level_launches == 2 * 4 * levels, (name, level_launches, levels)
    nodes = [len(ctx.mser_tree(d.ptr, w * cn, h, w, cn, pol)) for pol in (0, 1)]
    out = {"size": [h, w, cn], "call_ms_median7": call_ms, "device_ms_by_family": kern, "device_ms": round(sum(kern.values()), 3),
           # per polarity: gray + scatter, four per non-empty level, four selection kernels, one record kernel when regions exist
           "launches_per_call": int(level_launches + 2 * (2 + 4) + sum(1 for pol in (0, 1) if (regs["polarity"] == pol).any())),
           "level_launches": int(level_launches), "levels": int(levels), "nodes": nodes, "regions": int(len(regs)),
           "workspace_bytes_per_pixel": round(_native.mser_plan(h, w)["workspace_bytes"] / (h * w), 3)}
    if max(h, w) <= _native.load().sr_fft_max_len():
        d_sal = ctx.alloc(h * w)
        out["saliency_ms_median7"] = median_ms(lambda: ctx.saliency_u8(d.ptr, w * cn, h, w, cn, d_sal.ptr))
        d_sal.free()
    t0 = time.perf_counter()
    host = _native.mser_host(img)
    out["host_one_thread_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    out["equals_host"] = bool(host.tobytes() == regs.tobytes())
    d.free()
    print(f"{name}: {out}", file=sys.stderr, flush=True)
    return out


N = 4096
result = {"baseline_1080x720": run("baseline", baseline_source(720, 1080)),
          "smooth_noise_4096": run("smooth_noise", smooth_noise(N)),
          "flat_4096": run("flat", np.full((N, N), 128, np.uint8)),
          "two_level_4096": run("two_level", two_level(N)),
          "note": "MI355X; both polarities, default parameters; call_ms: the synchronous call on an image in HBM, median of 7 after "
                  "a warm-up; device_ms_by_family: hipEvent pairs around each launch of one further call"}
print(json.dumps(result, indent=1))
