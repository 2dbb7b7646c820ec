#!/usr/bin/env python3
"""Device time of the Poisson solver (sr_poisson_clone_u8) at 48 x 48, 1024 x 1536 and one 200 MP tile (4124 x 2970), with
per-kernel-family times, and of BlendingModule.repair_seams on a 2459 x 1640 canvas with about 200 planted seams; beside
each the SciPy float32 restatement (tests/_poisson_ref.py) on the same host.  Warm-up 2, then 7 runs timed with HIP events
(the library's own per-family event pairs; their sum is the device time of the call), median and minimum reported.
Writes profiles/poisson_timing.json.
usage (GPU box): python tools/poisson_timing.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np            # noqa: E402
import _native                # noqa: E402
import _poisson_ref as R      # noqa: E402
import blending_module as bm  # noqa: E402

WARM, RUNS = 2, 7
ctx = _native.default_context(0)


def events(fn):
    """-> ({family: [ms per run]}, [total ms per run]) from the library's HIP-event pairs."""
    for _ in range(WARM):
        fn()
    ctx.sync()
    fam, tot = {}, []
    ctx.prof_enable(True)
    for _ in range(RUNS):
        ctx.prof_reset()
        fn()
        ctx.sync()
        rec = {k: ms for k, (ms, _) in ctx.prof_get().items()}
        for k, ms in rec.items():
            fam.setdefault(k, []).append(ms)
        tot.append(sum(rec.values()))
    ctx.prof_enable(False)
    return fam, tot


def med_min(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}


def solver_case(h, w):
    dest, patch, mask = R.solver_inputs(h, w)
    bufs = [ctx.upload(dest), ctx.upload(patch), ctx.upload(mask), ctx.alloc(h * w * 3)]

    def run():
        ctx.poisson_clone_u8(bufs[0].ptr, w * 3, bufs[1].ptr, w * 3, bufs[2].ptr, w, h, w, R.MIXED, bufs[3].ptr, w * 3)

    fam, tot = events(run)
    t0 = time.perf_counter()
    R.clone(dest, patch, mask, R.MIXED, np.float32)
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    for b in bufs:
        b.free()
    wi, hi = w - 2, h - 2
    # algorithmic bytes: three u8 inputs + mask in, u8 out, and for each of the four transforms one read and one write of the
    # two complex planes at their natural (not odd-extended) length
    algo = h * w * (3 + 3 + 1 + 3) + 4 * 2 * (2 * wi * hi * 8)
    # moved by the glue kernels: eight passes over the odd-extended lines (rhs out, transpose in / out, eigenvalue pass
    # in / out, transpose in / out, final in), each 2 planes x hi lines x 2 (wi + 1) complex values, plus the u8 planes
    ext = 2 * hi * 2 * (wi + 1) * 8
    moved = h * w * (3 + 3 + 1 + 3 + 2) + 8 * ext
    out = {"roi": [h, w], "mode": "mixed", **med_min(tot), "kernel_ms": {k: med_min(v) for k, v in fam.items()},
           "scipy_float32_ms": round(cpu_ms, 2), "algorithmic_mb": round(algo / 1e6, 2),
           "moved_mb_glue_passes_only": round(moved / 1e6, 2),
           "note": "moved_mb counts the glue kernels (rhs, two transposes, eigenvalue pass, final) around the FFT line engine; "
                   "each sr_fft_lines call adds one read and one write of the extended lines per radix pass"}
    return out


def repair_case():
    H, W, n = 1640, 2459, 200
    rng = np.random.default_rng(4)
    img = R.synth(H, W, 3)
    tiles = [np.ascontiguousarray(img[:900, :1300]), np.ascontiguousarray(img[700:, 1100:])]
    seams = []
    for i in range(n):
        x, y = int(rng.integers(0, W - 48)), int(rng.integers(0, H - 48))
        seams.append(bm.Seam(x, y, int(rng.choice([16, 32, 48])), 16, 0.80 if i % 2 else 0.90))
    b = bm.BlendingModule()
    for _ in range(WARM):
        b.repair_seams(img, seams, tiles)
    wall = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        b.repair_seams(img, seams, tiles)
        wall.append(1e3 * (time.perf_counter() - t0))
    fam, tot = events(lambda: b.repair_seams(img, seams, tiles))
    t0 = time.perf_counter()
    R.repair_seams(img, seams, tiles, dtype=np.float32)
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    return {"canvas": [H, W], "seams": n, "poisson_seams": n // 2, "blur_seams": n - n // 2,
            "wall": med_min(wall), "device": med_min(tot), "kernel_ms": {k: med_min(v) for k, v in fam.items()},
            "restatement_float32_ms": round(cpu_ms, 1),
            "note": "wall includes one upload of image and tiles, one region-SSIM readback per (seam, tile) and one download"}


res = {"solver": [solver_case(h, w) for (h, w) in ((48, 48), (1024, 1536), (4124, 2970))], "repair_seams": repair_case(),
       "method": f"warm-up {WARM}, {RUNS} runs, HIP events (sr_prof), median and minimum"}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "poisson_timing.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
