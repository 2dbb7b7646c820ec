#!/usr/bin/env python3
"""Time of cascade detection (csrc/sr_cascade.hip), default parameters (factor 1.1), on images resident in HBM: the 1080 x 720
BASELINE source and a 4096 x 4096 smooth-plus-noise image, each with the OpenCV-trained LBP model of the fixtures
(tests/golden/lbpcascade_frontalface_opencv.xml, 20 stages, 139 stumps) and with a CONSTRUCTED 25-stage HAAR cascade of 2913
stumps (the stage sizes of OpenCV's frontal-face default; random balanced features -- a stand-in for the cost, not a
detector).  Per input: the synchronous call (median of 7 after a warm-up; it holds the two downloads), the device time of each
phase from hipEvent pairs (sr_prof_*, one pair per kernel launch: planes = gray + every scaled plane, with the model upload;
tables = row and column passes; dense = the leading stages on every window and the compaction; tail = the remaining stages on the survivors), the
kernel launches of that call counted from those pairs, the scales, positions and candidates, the fraction of scale-0 windows that pass stage 0 and the
dense stages (from the host stage map), and the workspace; beside them, in the same process on the same image,
sr_cascade_host_u8 on one host thread, sr_mser_u8 and sr_saliency_u8.
usage (GPU box): python tools/cascade_timing.py > profiles/cascade_timing.json"""
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
import tiling_module as tm               # noqa: E402
import _cascade_ref as R                 # noqa: E402

ctx = _native.default_context(0)
REPS = 7
HAAR_STAGES = (9, 16, 27, 32, 52, 53, 62, 72, 83, 91, 99, 115, 127, 135, 136, 137, 159, 155, 169, 196, 197, 181, 199, 211, 200)


def smooth_noise(n):
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    base = 128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0)
    return np.clip(base + rng.integers(-12, 13, size=(n, n)), 0, 255).astype(np.uint8)


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


def run(name, img, model, stage_counts, others):
    h, w = img.shape[:2]
    cn = img.shape[2] if img.ndim == 3 else 1
    d = ctx.upload(np.ascontiguousarray(img))
    call = lambda: ctx.cascade(model, d.ptr, w * cn, h, w, cn)                            # noqa: E731
    call_ms = median_ms(call)
    ctx.prof_enable(True)
    ctx.prof_reset()
    cands = call()
    ctx.sync()
    prof = ctx.prof_get()
    ctx.prof_enable(False)
    ctx.prof_reset()
    # the library opens one profiling scope per kernel launch: the launches of the call are counted, not assumed
    kern = {k[3:]: (ms, n) for k, (ms, n) in prof.items() if k.startswith("cc_")}
    launches = sum(n for _, n in kern.values())
    phases = {name: round(sum(kern[k][0] for k in parts if k in kern), 3)
              for name, parts in (("planes", ("gray", "planes")), ("tables", ("rows", "cols")), ("dense", ("dense",)), ("tail", ("tail",)))
              if any(k in kern for k in parts)}
    assert set(kern) <= {"gray", "planes", "rows", "cols", "dense", "tail"}, prof
    plan = model.plan(h, w)
    dense = 0                                # the leading stages the dense kernel takes: at most 64 stumps (and 64 stages)
    while dense < min(len(stage_counts), 64) and sum(stage_counts[:dense + 1]) <= 64:
        dense += 1
    out = {"size": [h, w, cn], "model": {"type": model.feature_type, "stages": model.n_stages, "stumps": model.n_stumps},
           "call_ms_median7": call_ms, "device_ms_by_phase": phases, "device_ms": round(sum(phases.values()), 3),
           # counted from the profile of this call (gray, planes, table rows, table columns, dense, tail; beside them one memset
           # of the counters, three small uploads and two downloads)
           "kernel_launches_per_call": int(launches), "launches_by_kernel": {k: int(n) for k, (_, n) in kern.items()},
           "scales": len(plan["scales"]), "positions": plan["positions"],
           "candidates": int(len(cands)), "boxes_min_neighbors_4": int(len(_native.cascade_group(cands, 4))),
           "workspace_bytes": plan["workspace_bytes"], "workspace_bytes_per_pixel": round(plan["workspace_bytes"] / (h * w), 2)}
    t0 = time.perf_counter()
    host = model.host(img)
    out["host_one_thread_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    smap = model.stage_map_host(img, 2)
    out["dense_stages"] = dense
    out["scale0_fraction_passing_stage0"] = round(float((smap >= 1).mean()), 5)
    out["scale0_fraction_passing_dense_stages"] = round(float((smap >= dense).mean()), 5)
    out["equals_host"] = bool(np.array_equal(host, cands))
    if others:
        out["mser_ms_median7"] = median_ms(lambda: ctx.mser(d.ptr, w * cn, h, w, cn))
        if max(h, w) <= _native.load().sr_fft_max_len():
            d_sal = ctx.alloc(h * w)
            out["saliency_ms_median7"] = median_ms(lambda: ctx.saliency_u8(d.ptr, w * cn, h, w, cn, d_sal.ptr))
            d_sal.free()
    d.free()
    print(f"{name}: {out}", file=sys.stderr, flush=True)
    return out


lbp_t = tm.load_cascade(R.LBP_XML)
lbp, lbp_n = _native.CascadeModel(lbp_t), [int(v) for v in lbp_t["stage_counts"]]
haar_t = R.random_haar(window=(24, 24), seed=21, stages=HAAR_STAGES, n_feats=1500)
haar_t["stage_thresholds"] = np.zeros(len(HAAR_STAGES), np.float32)      # random leaves: about half of the windows leave per stage
haar, haar_n = _native.CascadeModel(haar_t), list(HAAR_STAGES)
base, big = R.baseline_source(720, 1080), smooth_noise(4096)
result = {"baseline_1080x720_lbp": run("baseline lbp", base, lbp, lbp_n, True),
          "baseline_1080x720_haar2913": run("baseline haar", base, haar, haar_n, False),
          "smooth_noise_4096_lbp": run("4096 lbp", big, lbp, lbp_n, True),
          "smooth_noise_4096_haar2913": run("4096 haar", big, haar, haar_n, False),
          "note": "MI355X; scale_factor 1.1; call_ms: the synchronous call on an image in HBM, median of 7 after a warm-up; "
                  "device_ms_by_phase: hipEvent pairs around each phase of one further call; the HAAR model is constructed "
                  "(random balanced features, OpenCV's frontal-face stage sizes): it measures cost, it detects nothing"}
print(json.dumps(result, indent=1))
