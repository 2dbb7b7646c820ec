#!/usr/bin/env python3
"""Device time of BRISQUE's kernel families (brisque_half: the exact half plane; brisque_moments_1 / _2: the moment launch of
each scale; brisque_reduce: the two fixed-order reductions) on one 200 MP RGB canvas (17320 x 11550 x 3: a noisy image resized
on the device), beside sr_niqe_u8 on the same buffer in the same process as the comparison line.  The two calls alternate in
one run.  Warm-up 2, then 7 repetitions timed with HIP events (the library's own per-family event pairs), median and minimum
reported, the wall time of each synchronous call, and the host time of features + score on the records.  Writes
profiles/brisque_timing.json (or the path given as the third argument).
usage (GPU box): python tools/brisque_timing.py [W H [out.json]]"""
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
OUT = sys.argv[3] if len(sys.argv) >= 4 else os.path.join(ROOT, "profiles", "brisque_timing.json")
ctx = _native.default_context(0)


def canvas():
    rng = np.random.default_rng(1)
    h, w = max(H // 10, 8), max(W // 10, 8)
    yy, xx = np.mgrid[0:h, 0:w]
    small = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (h, w, 3)),
                    0, 255).astype(np.uint8)
    src, a = ctx.upload(small), ctx.alloc(H * W * 3)
    ctx.resize_cubic_u8(src.ptr, w * 3, h, w, 3, a.ptr, W * 3, H, W)
    ctx.sync()
    src.free()
    return a


def med_min(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}


a = canvas()
box = {}


def run_brisque():
    box["brisque"] = ctx.brisque_u8(a.ptr, W * 3, H, W, 3)


def run_niqe():
    box["niqe"] = ctx.niqe_u8(a.ptr, W * 3, H, W, 3)


BQ = ("brisque_half", "brisque_moments_1", "brisque_moments_2", "brisque_reduce")
CALLS = [("brisque", run_brisque, BQ), ("niqe", run_niqe, ("niqe_half", "niqe_blocks"))]
for _ in range(WARM):
    for _, fn, _ in CALLS:
        fn()
ctx.sync()
dev = {f: [] for _, _, fams in CALLS for f in fams}
wall = {n: [] for n, _, _ in CALLS}
ctx.prof_enable(True)
for r in range(RUNS):                                    # rotated: neither call always runs first
    for k in range(len(CALLS)):
        name, fn, fams = CALLS[(k + r) % len(CALLS)]
        ctx.prof_reset()
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
        ctx.sync()
        got = ctx.prof_get()
        for f in fams:
            dev[f].append(got[f][0])
ctx.prof_enable(False)
t0 = time.perf_counter()
feat = _native.brisque_features(box["brisque"])
t_feat = 1e3 * (time.perf_counter() - t0)
rng = np.random.default_rng(2)                           # any regressor of a published model's size times the score alike
model = {"sv": rng.uniform(-1, 1, (774, 36)), "sv_coef": rng.standard_normal(774), "gamma": 0.05, "rho": -150.0,
         "feature_min": feat - 1.0, "feature_max": feat + 1.0}
t0 = time.perf_counter()
score = _native.brisque_score(feat, model)
t_score = 1e3 * (time.perf_counter() - t0)
plan = _native.brisque_plan(H, W, 3, 0)
bq_dev = [sum(v) for v in zip(*(dev[f] for f in BQ))]
nq_dev = [x + y for x, y in zip(dev["niqe_half"], dev["niqe_blocks"])]
yard = statistics.median(nq_dev)
res = {"image": [H, W, 3], "half_size": list(plan["half_size"]), "scratch_bytes": plan["scratch_bytes"],
       "device": {**{f: med_min(v) for f, v in dev.items()}, "brisque_total": med_min(bq_dev), "niqe_total": med_min(nq_dev)},
       "wall": {n: med_min(v) for n, v in wall.items()},
       "host_ms": {"features": round(t_feat, 3), "score_774_sv": round(t_score, 3)},
       "ratio_over_niqe_total": {**{f: round(statistics.median(dev[f]) / yard, 3) for f in BQ},
                                 "brisque_total": round(statistics.median(bq_dev) / yard, 3)},
       "image_gb_per_s": {"brisque_total": round(H * W * 3 / (statistics.median(bq_dev) * 1e-3) / 1e9, 1),
                          "niqe_total": round(H * W * 3 / (yard * 1e-3) / 1e9, 1)},
       "features_finite": bool(np.isfinite(feat).all()), "score_finite": bool(np.isfinite(score)),
       "method": f"warm-up {WARM}, {RUNS} rotated repetitions, HIP events (sr_prof) around each kernel family, median and minimum; "
                 "brisque_reduce covers the reductions of both scales; wall = the synchronous call as the host sees it (the "
                 "records' download included); image_gb_per_s = the image's bytes once over the median device time"}
a.free()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
