#!/usr/bin/env python3
"""RRDB networks (csrc/sr_rrdb.hip) on the GPU: ms per input tile and achieved TFLOP/s for RealESRGAN_x4plus's shape (F 64, G 32,
B 23) and the anime model's (F 64, G 32, B 6), with the per-kernel split head / dense (the G-output convolutions) / blockout (the
F-output conv5 of a dense block) / bodyup (conv_body, conv_up1, conv_up2) / hr / last (HIP events, a run of its own).
Seeded synthetic weights (none ship with the repository): timing does not depend on their values.  Useful FLOPs are those of
the unstreamed forward, computed from the shapes: per input pixel 2 * 27 F (head), per dense block 2 * 9 G (F + (k - 1) G) for
k = 1 .. 4 and 2 * 9 F (F + 4 G), 2 * 9 F^2 for conv_body, 4 and 16 times that for conv_up1 and conv_up2, 16 times for conv_hr
and 2 * 9 F 3 * 16 for conv_last (the zero-padded couts are not counted).
Run it in the same GPU visit as tools/resnet_timing.py: the EDSR body TFLOP/s of that run is the yardstick for the dense
convolutions.
usage: tools/rrdb_timing.py [--side 512] [--reps 5] [--tiles 0,128] [--out profiles/rrdb_timing.json]"""
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
NAMES = ("head", "dense", "blockout", "bodyup", "hr", "last")


def synthetic_state(F, G, B, seed=20260313):
    rng = np.random.default_rng(seed)
    st = {}

    def conv(name, cout, cin, gain=1.0):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)

    conv("conv_first", F, 3)
    for i in range(B):
        for d in (1, 2, 3):
            for k in range(1, 5):
                conv(f"body.{i}.rdb{d}.conv{k}", G, F + (k - 1) * G)
            conv(f"body.{i}.rdb{d}.conv5", F, F + 4 * G, 0.1)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, F, F)
    conv("conv_last", 3, F, 0.1)
    return st


def flops(F, G, B, h, w):
    px = float(h) * w
    return {"head": 2.0 * 27 * F * px,
            "dense": 2.0 * 9 * G * sum(F + k * G for k in range(4)) * 3 * B * px,
            "blockout": 2.0 * 9 * F * (F + 4 * G) * 3 * B * px,
            "bodyup": 2.0 * 9 * F * F * (1 + 4 + 16) * px,
            "hr": 2.0 * 9 * F * F * 16 * px,
            "last": 2.0 * 9 * F * 3 * 16 * px}


def time_net(ctx, F, G, B, side, reps, tiles):
    import sr_network
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    net = sr_network.RRDBSRNet(synthetic_state(F, G, B))
    m = net.model(ctx)
    d_src, d_dst = ctx.upload(img), ctx.alloc(side * 4 * side * 4 * 3)
    fl = flops(F, G, B, side, side)
    total = sum(fl.values())
    out = {"n_feat": F, "n_grow": G, "n_blocks": B, "scale": 4, "input": f"{side}x{side}", "useful_TFLOP": round(total / 1e12, 4), "by_tile": {}}
    run = lambda tile: m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * 4 * 3, tile, 0)
    try:
        for tile in tiles:
            halo, n, nt, ws = m.plan(side, side, tile, 0)
            for _ in range(2):                                   # warm-up: code objects, the activation buffers
                run(tile)
            ctx.sync()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                run(tile)
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            # per-kernel split in a run of its own (the event pairs cost host time)
            ctx.prof_enable(True)
            ctx.prof_reset()
            run(tile)
            ctx.sync()
            prof = ctx.prof_get()
            ctx.prof_enable(False)
            ms = float(np.median(ts))
            kern = {k: {"ms": round(prof[f"rrdb_{k}"][0], 3), "launches": prof[f"rrdb_{k}"][1],
                        "useful_TFLOPs_per_s": round(fl[k] / 1e12 / (prof[f"rrdb_{k}"][0] / 1e3), 2)} for k in NAMES if f"rrdb_{k}" in prof}
            out["by_tile"][str(tile)] = {
                "trunk_pieces": n, "tail_pieces": nt, "halo": halo, "workspace_MB": round(ws / 2 ** 20, 1),
                "ms_median": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "reps": reps,
                "useful_TFLOPs_per_s": round(total / 1e12 / (ms / 1e3), 2),
                "frac_of_f32_matrix_peak": round(total / 1e12 / (ms / 1e3) / F32_MATRIX_PEAK_TFLOPS, 4),
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
    ap.add_argument("--tiles", default="0,128", help="trunk piece sizes to time (0: the library's choice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrdb_timing.json"))
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    tiles = [int(t) for t in args.tiles.split(",")]
    out = {"nets": [time_net(ctx, 64, 32, 23, args.side, args.reps, tiles), time_net(ctx, 64, 32, 6, args.side, args.reps, tiles)]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
