#!/usr/bin/env python3
"""Device time of the content analysis (csrc/sr_content.hip) on an RGB image resident in HBM: saliency (per stage),
local entropy (window 64), forbidden map + per-tile counts, and the whole create_forbidden_zone_map device form followed
by tile_flags -- at the source-image size of the 200MP-kd workload (17320 x 11550) and at 4 MP (2459 x 1640).
Kernel times come from hipEvent pairs around each kernel family (sr_prof_*), after a warm-up call; the wall time of the
whole form is the mean of `reps` synchronised calls.  The byte floor of a stage is the bytes it must read and write once.
usage (GPU box): python tools/content_timing.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    sys.path.insert(0, p)
import torch                             # noqa: E402
import _native                           # noqa: E402
import tiling_module as tm               # noqa: E402

an = tm.ContentAnalyzer()
ctx = an._ctx()
STREAM_TBS = 5.2                         # what a plain device copy moves (read + write) on this part


def image(h, w):
    yy = torch.arange(h, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(w, device="cuda", dtype=torch.float32)[None, :]
    base = 110 + 50 * torch.sin(xx / 37.0) + 35 * torch.cos(yy / 23.0)
    blob = 90 * torch.exp(-(((yy - 0.37 * h) / (0.04 * h)) ** 2 + ((xx - 0.61 * w) / (0.04 * w)) ** 2))
    noise = torch.randint(-12, 13, (h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    return ((base + blob)[..., None] + noise).clamp(0, 255).to(torch.uint8).contiguous()


def kernel_ms(fn):
    fn()
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    ctx.sync()
    kern = {k: round(ms, 3) for k, (ms, _) in ctx.prof_get().items()}
    ctx.prof_enable(False)
    return kern


def wall_ms(fn, reps=3):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


def run(h, w, block):
    img = image(h, w)
    torch.cuda.synchronize()
    shape, px = (h, w, 3), h * w
    positions = _native.tile_plan(w, h, block, int(block * 0.2))
    d_sal, d_ent, d_map = ctx.alloc(px), ctx.alloc(px * 4), ctx.alloc(px)
    sal = kernel_ms(lambda: ctx.saliency_u8(img.data_ptr(), w * 3, h, w, 3, d_sal.ptr))
    ent = kernel_ms(lambda: ctx.local_entropy_u8(img.data_ptr(), w * 3, h, w, 3, 64, d_ent.ptr))
    mc = kernel_ms(lambda: (ctx.forbidden_map(d_sal.ptr, h, w, 178, [(w // 3, h // 3, w // 10, h // 10)], d_map.ptr),
                            ctx.rect_counts_u8(d_map.ptr, w, h, w, positions)))
    for b in (d_sal, d_ent, d_map):
        b.free()

    def whole():
        fm = an.create_forbidden_zone_map_device(img.data_ptr(), shape, protect_text=False)
        flags = an.tile_flags(fm, positions)
        fm.free()
        return flags

    whole_ms = wall_ms(whole)
    flags = whole()
    gb = 1e-9
    floors = {                            # bytes read + written once, over the streaming rate
        "ct_fft_fwd": (3 * px + 8 * px) * gb, "ct_residual": (8 * px + 8 * px) * gb, "ct_fft_inv": (8 * px + 8 * px) * gb,
        "ct_blur_norm": (8 * px + px) * gb, "ct_entropy": (3 * px + 4 * px) * gb, "ct_map": (px + px) * gb,
        "ct_count": sum(pw * ph for _, _, pw, ph in positions) * gb}
    floor_ms = {k: round(v / STREAM_TBS, 3) for k, v in floors.items()}
    del img
    torch.cuda.empty_cache()
    return {"size": [h, w], "tiles": len(positions), "saliency_kernel_ms": sal, "saliency_ms": round(sum(sal.values()), 3),
            "entropy_kernel_ms": ent, "map_counts_kernel_ms": mc, "forbidden_map_device_plus_flags_wall_ms": whole_ms,
            "byte_floor_ms": floor_ms, "tiles_with_forbidden_zone": sum(f["has_forbidden_zone"] for f in flags)}


out = {"image_200mp": run(11550, 17320, 4096), "image_4mp": run(1640, 2459, 1024),
       "note": "kernel ms from hipEvent pairs around each kernel family after one warm-up call; wall ms of the synchronous "
               "device form (saliency + map + counts, allocation included) as the mean of 3 calls"}
print(json.dumps(out))
