#!/usr/bin/env python3
"""Residual SR networks (csrc/sr_resnet.hip) on the GPU: ms per input tile and achieved TFLOP/s for MSRResNet (F 64, B 16, x4)
and EDSR baseline (F 64, B 16, x2), with the per-kernel split head / body / up / hr / last (HIP events, a run of its own).
Seeded synthetic weights (none ship with the repository): timing does not depend on their values.  Useful FLOPs are those of
the unstreamed forward, computed from the shapes: per input pixel 2 * 27 F (head) + 2 * 9 F^2 per body convolution, per
upsampling stage 2 * 9 F^2 r^2 at its own resolution, 2 * 9 F^2 s^2 (HR conv) and 2 * 9 F 3 s^2 (last; the zero-padded couts
are not counted).
usage: tools/resnet_timing.py [--side 512] [--reps 5] [--tiles 0,128] [--out profiles/resnet_timing.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3
EXPECTED_TFLOPS = 121.0          # what the README quotes for the LPIPS kernel of the same tiling (derived expectation)
STAGES = {1: [], 2: [2], 3: [3], 4: [2, 2]}


def synthetic_state(preset, F, B, s, seed=20260313):
    rng = np.random.default_rng(seed)
    st = {}

    def conv(name, cout, cin, gain=1.0):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)

    conv("conv_first", F, 3)
    for i in range(B):
        conv(f"body.{i}.conv1", F, F)
        conv(f"body.{i}.conv2", F, F, 0.1)
    if preset == "edsr":
        conv("conv_after_body", F, F)
    for k, r in enumerate(STAGES[s]):
        conv(f"upsample.{2 * k}" if preset == "edsr" else f"upconv{k + 1}", F * r * r, F)
    if preset == "msr":
        conv("conv_hr", F, F)
    conv("conv_last", 3, F, 0.1)
    return st


def flops(preset, F, B, s, h, w):
    px = float(h) * w
    fl = {"head": 2.0 * 27 * F * px, "body": 2.0 * 9 * F * F * (2 * B + (preset == "edsr")) * px, "up": 0.0,
          "hr": 2.0 * 9 * F * F * s * s * px if preset == "msr" else 0.0, "last": 2.0 * 9 * F * 3 * s * s * px}
    m = 1
    for r in STAGES[s]:
        fl["up"] += 2.0 * 9 * F * F * r * r * m * m * px
        m *= r
    return fl


def time_net(ctx, preset, F, B, s, side, reps, tiles):
    import sr_network
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    net = sr_network.ResidualSRNet(synthetic_state(preset, F, B, s))
    m = net.model(ctx)
    d_src, d_dst = ctx.upload(img), ctx.alloc(side * s * side * s * 3)
    fl = flops(preset, F, B, s, side, side)
    total = sum(fl.values())
    out = {"preset": preset, "n_feat": F, "n_blocks": B, "scale": s, "input": f"{side}x{side}", "useful_TFLOP": round(total / 1e12, 4),
           "by_tile": {}}
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
            kern = {k.replace("resnet_", ""): {"ms": round(v[0], 3), "launches": v[1],
                                                "useful_TFLOPs_per_s": round(fl[k.replace("resnet_", "")] / 1e12 / (v[0] / 1e3), 2)}
                    for k, v in prof.items() if k.startswith("resnet_")}
            out["by_tile"][str(tile)] = {
                "sub_tiles": n, "halo": halo, "workspace_MB": round(ws / 2 ** 20, 1),
                "ms_median": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "reps": reps,
                "useful_TFLOPs_per_s": round(total / 1e12 / (ms / 1e3), 2),
                "frac_of_f32_matrix_peak": round(total / 1e12 / (ms / 1e3) / F32_MATRIX_PEAK_TFLOPS, 4),
                "expected_ms_at_121_TFLOPs": round(total / 1e12 / EXPECTED_TFLOPS * 1e3, 2),
                "kernels": kern}
    finally:
        ctx.sync()
        d_src.free(); d_dst.free()
        net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", default="0,128", help="sub-tile sizes to time (0: the library's choice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_timing.json"))
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    tiles = [int(t) for t in args.tiles.split(",")]
    out = {"nets": [time_net(ctx, "msr", 64, 16, 4, args.side, args.reps, tiles), time_net(ctx, "edsr", 64, 16, 2, args.side, args.reps, tiles)]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
