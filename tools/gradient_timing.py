#!/usr/bin/env python3
"""Device time of BlendingModule.gradient_domain_fusion (sr_gradient_fusion: row pass + column pass) and of
compute_blend_quality's device part (sr_tile_ssim_sums_u8 + sr_gradient_stats_u8) on the 200 MP BASELINE grid (25 tiles
of 4124 x 2970 on 17320 x 11550), tiles already in HBM.
usage (GPU box): python tools/gradient_timing.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    sys.path.insert(0, p)
import torch                  # noqa: E402
import _native                # noqa: E402
import bench                  # noqa: E402
import device_pipeline as dp  # noqa: E402

geo = dp.workload_geometry("200MP")
H, W, cn = geo.canvas_h, geo.canvas_w, 3
dev = torch.device("cuda", 0)
pipe = dp.DevicePipeline(geo, 0, 1, 0)
src = bench.synthetic_source()
t = torch.from_numpy(src).to(dev)
image = torch.empty((H, W * cn), dtype=torch.uint8, device=dev)
pipe.ctx.resize_cubic_u8(t.data_ptr(), src.shape[1] * cn, src.shape[0], src.shape[1], cn, image.data_ptr(), W * cn, H, W)
pipe.step(image, image)
torch.cuda.synchronize()
ctx = pipe.ctx
ptrs = [pipe.local_tiles[i].data_ptr() for i in range(len(geo.rects))]
strides = [pipe.local_tiles[i].stride(0) for i in range(len(geo.rects))]
out = torch.empty((H, W * cn), dtype=torch.uint8, device=dev)
work = torch.empty((H, W * cn), dtype=torch.float32, device=dev)


def fusion():
    ctx.gradient_fusion(_native.SR_U8, ptrs, strides, geo.rects, cn, H, W, out.data_ptr(), W * cn, work.data_ptr())
    ctx.sync()


def quality():
    ctx.tile_ssim_sums_u8(out.data_ptr(), W * cn, H, W, cn, geo.rects, ptrs, strides)
    ctx.gradient_stats_u8(out.data_ptr(), W * cn, H, W, cn)


def timed(fn, reps=3):
    fn()
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    kern = {k: round(ms, 3) for k, (ms, _) in ctx.prof_get().items()}
    ctx.prof_enable(False)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3), kern


f_ms, f_kern = timed(fusion)
q_ms, q_kern = timed(quality)
tile_bytes = sum(w * h * cn for (_, _, w, h) in geo.rects)
floor_gb = (tile_bytes * 2 + H * W * cn * (4 + 4 + 1)) / 1e9       # tiles read by each pass, cx out and in, u8 out
print(json.dumps({"gradient_fusion_ms": f_ms, "gradient_fusion_kernel_ms": f_kern, "fusion_floor_gb": round(floor_gb, 2),
                  "blend_quality_ms": q_ms, "blend_quality_kernel_ms": q_kern,
                  "note": "wall time of the synchronous calls (quality: incl. the small result downloads)"}))
