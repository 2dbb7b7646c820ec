#!/usr/bin/env python3
"""Local SR network (csrc/sr_srnet.hip) on the GPU: ms per 2048 x 2048 input tile and achieved TFLOP/s for the two usual
shapes, (F 64, D 16, s 2) and (F 64, D 32, s 4); the per-kernel split head / body / tail (HIP events, a run of its own);
and the sr_net stage of SuperResolutionPipeline.process() at the 200 MP scale.  Seeded synthetic weights (none ship with the
repository): timing does not depend on their values.  Useful FLOPs are those of the unstreamed forward, computed from the
shapes: per input pixel 2 * 27 F (head) + 2 * 9 F^2 D (body) + 2 * 9 F 3 s^2 (tail; the zero-padded couts are not counted).
usage: tools/srnet_timing.py [--side 2048] [--reps 5] [--tiles 0,1024] [--no-process] [--out profiles/srnet_timing.json]"""
import argparse
import asyncio
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3
EXPECTED_TFLOPS = 121.0          # what the README quotes for the LPIPS kernel of the same tiling (derived expectation)


def synthetic_state(F, D, s, seed=20260313):
    rng = np.random.default_rng(seed)
    st, chans = {}, [3] + [F] * (D + 1) + [3 * s * s]
    for k in range(D + 2):
        cin, cout = chans[k], chans[k + 1]
        st[f"body.{2 * k}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * (0.1 if k == D + 1 else 1.0)).astype(np.float32)
        st[f"body.{2 * k}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
        if k <= D:
            st[f"body.{2 * k + 1}.weight"] = rng.uniform(0.05, 0.3, cout).astype(np.float32)
    return st


def flops(F, D, s, h, w):
    px = float(h) * w
    return {"head": 2.0 * 27 * F * px, "body": 2.0 * 9 * F * F * D * px, "tail": 2.0 * 9 * F * 3 * s * s * px}


def time_net(ctx, F, D, s, side, reps, tiles):
    import sr_network
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    net = sr_network.CompactSRNet(synthetic_state(F, D, s))
    m = net.model(ctx)
    d_src, d_dst = ctx.upload(img), ctx.alloc(side * s * side * s * 3)
    fl = flops(F, D, s, side, side)
    total = sum(fl.values())
    out = {"n_feat": F, "n_body": D, "scale": s, "input": f"{side}x{side}", "useful_TFLOP": round(total / 1e12, 4), "by_tile": {}}
    try:
        for tile in tiles:
            halo, n, ws = m.plan(side, side, tile)
            for _ in range(2):                                   # warm-up: code objects, the activation buffers
                m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * s * 3, tile)
            ctx.sync()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * s * 3, tile)
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            # per-kernel split in a run of its own (the event pairs cost host time)
            ctx.prof_enable(True)
            ctx.prof_reset()
            m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * s * 3, tile)
            ctx.sync()
            prof = ctx.prof_get()
            ctx.prof_enable(False)
            ms = float(np.median(ts))
            kern = {k.replace("srnet_", ""): {"ms": round(v[0], 3), "launches": v[1],
                                               "useful_TFLOPs_per_s": round(fl[k.replace("srnet_", "")] / 1e12 / (v[0] / 1e3), 2)}
                    for k, v in prof.items() if k.startswith("srnet_")}
            out["by_tile"][str(tile)] = {
                "sub_tiles": n, "halo": halo, "workspace_MB": round(ws / 2 ** 20, 1),
                "ms_per_tile_median": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "reps": reps,
                "useful_TFLOPs_per_s": round(total / 1e12 / (ms / 1e3), 2),
                "frac_of_f32_matrix_peak": round(total / 1e12 / (ms / 1e3) / F32_MATRIX_PEAK_TFLOPS, 4),
                "expected_ms_at_121_TFLOPs": round(total / 1e12 / EXPECTED_TFLOPS * 1e3, 2),
                "kernels": kern}
    finally:
        ctx.sync()
        d_src.free(); d_dst.free()
        net.close()
    return out


def time_process(width, height, F, D, s):
    """One process() run at the 200 MP scale with the network as stage 2 (QA off: the stage of interest is sr_net)."""
    import main as sr_main
    import _native
    rng = np.random.default_rng(20260313)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    img = np.stack([128 + 64 * np.sin(xx / 37.0 + 0.7 * c) + 48 * np.cos(yy / 23.0 + 1.3 * c) for c in range(3)], axis=-1)
    img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
    del yy, xx
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        src, wpath = os.path.join(d, "in.png"), os.path.join(d, "net.npz")
        _native.write_image(img, src)
        np.savez(wpath, **synthetic_state(F, D, s))
        cfg = sr_main.PipelineConfig(block_size=2048, overlap_ratio=0.2, sr_scale=s, sr_weights=wpath, enable_qa=False)
        pipe = sr_main.SuperResolutionPipeline(cfg)
        pipe.tiling_module.l2_cache_dir = type(pipe.tiling_module.l2_cache_dir)(d)
        pipe.sr_net.model(pipe.quality_module._ctx())           # weights resident before the timed run
        t0 = time.perf_counter()
        res = asyncio.run(pipe.process(src, os.path.join(d, "out.tif"), prompt=""))
        dt = time.perf_counter() - t0
        assert res.success, res.error_message
        return {"source": f"{width}x{height}", "canvas_MP": round(width * s * height * s / 1e6, 1), "n_feat": F, "n_body": D,
                "scale": s, "blocks": res.total_blocks, "seconds": round(dt, 3),
                "stages_s": {k: round(v, 4) for k, v in pipe.stage_times.items()},
                "sr_net_ms_per_block": round(pipe.stage_times["sr_net"] * 1e3 / res.total_blocks, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", default="0,1024", help="sub-tile sizes to time (0: the library's choice)")
    ap.add_argument("--no-process", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srnet_timing.json"))
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    tiles = [int(t) for t in args.tiles.split(",")]
    out = {"nets": [time_net(ctx, 64, 16, 2, args.side, args.reps, tiles), time_net(ctx, 64, 32, 4, args.side, args.reps, tiles)]}
    if not args.no_process:
        out["process_200MP"] = time_process(8660, 5774, 64, 16, 2)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
