#!/usr/bin/env python3
"""Swin2SR (csrc/sr_swin2sr.hip) on the GPU beside SwinIR of the same configuration, in the same process: C 180, 6 heads, hidden
360, L 6, D 6, x4 pixelshuffle on a 512 x 512 input.  Per family: the host-timed median (a host clock around a forward that ends
in a synchronise), the device time (the sum of the HIP-event intervals of a profiled run, in runs of their own, median of 7) and
the split head / ln (LayerNorm, for Swin2SR with its skip) / linear (qkv, proj, fc1, fc2 and Swin2SR's 1 x 1 projections) /
attention / conv (the trunk's 3 x 3 convolutions) / tail (the reconstruction).  SwinIR's figures are tools/swinir_timing.py's
(time_net); the two families are timed in alternation (SwinIR, Swin2SR, SwinIR, Swin2SR) and the spread is reported, so that the
ratio is not a difference between two moments of a shared machine.
Seeded synthetic weights (none ship with the repository): timing does not depend on their values.  Useful FLOPs per pixel of the
padded image: SwinIR's (tools/swinir_timing.flops) plus 2 C^2 for each of the L + 1 projections; the normalisation of q and k,
the LayerNorm, the softmax and the GELU count as none.
usage: tools/swin2sr_timing.py [--side 512] [--reps 7] [--out profiles/swin2sr_timing.json]"""
import argparse
import datetime
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import swinir_timing  # noqa: E402

NAMES = swinir_timing.NAMES
STAGES = swinir_timing.STAGES


def synthetic_state(C, heads, hidden, L, D, scale, seed=20261020):
    """The `transformers` package's key layout, pixelshuffle only (the shape this tool times)."""
    rng = np.random.default_rng(seed)
    st = {}

    def conv(name, cout, cin, k=3, gain=0.5):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (k * k * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)

    def lin(name, cout, cin, bias=True):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin)) * 0.5 / np.sqrt(cin)).astype(np.float32)
        if bias:
            st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)

    def norm(name):
        st[f"{name}.weight"] = rng.uniform(0.5, 1.5, C).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(C) * 0.1).astype(np.float32)

    conv("swin2sr.first_convolution", C, 3)
    conv("swin2sr.embeddings.patch_embeddings.projection", C, C, 1)
    norm("swin2sr.embeddings.patch_embeddings.layernorm")
    for i in range(L):
        for j in range(D):
            b = f"swin2sr.encoder.stages.{i}.layers.{j}"
            a = f"{b}.attention.self"
            st[f"{a}.logit_scale"] = rng.uniform(math.log(3.0), math.log(200.0), (heads, 1, 1)).astype(np.float32)
            lin(f"{a}.continuous_position_bias_mlp.0", 512, 2)
            lin(f"{a}.continuous_position_bias_mlp.2", heads, 512, bias=False)
            lin(f"{a}.query", C, C)
            lin(f"{a}.key", C, C, bias=False)
            lin(f"{a}.value", C, C)
            lin(f"{b}.attention.output.dense", C, C)
            norm(f"{b}.layernorm_before")
            lin(f"{b}.intermediate.dense", hidden, C)
            lin(f"{b}.output.dense", C, hidden)
            norm(f"{b}.layernorm_after")
        conv(f"swin2sr.encoder.stages.{i}.conv", C, C)
        conv(f"swin2sr.encoder.stages.{i}.patch_embed.projection", C, C, 1)
    norm("swin2sr.layernorm")
    conv("swin2sr.conv_after_body", C, C)
    conv("upsample.conv_before_upsample", 64, C)
    for k, r in enumerate(STAGES[scale]):
        conv(f"upsample.upsample.convolution_{k}" if scale != 3 else "upsample.upsample.convolution", 64 * r * r, 64)
    conv("upsample.final_convolution", 3, 64, 3, 0.1)
    return st


def flops(C, hidden, L, D, scale, hp, wp):
    fl = swinir_timing.flops(C, hidden, L, D, scale, hp, wp)
    fl["linear"] += 2.0 * C * C * (L + 1) * float(hp) * wp
    return fl


def time_net(ctx, C, heads, hidden, L, D, scale, side, reps):
    import sr_network
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    net = sr_network.Swin2SRNet(synthetic_state(C, heads, hidden, L, D, scale))
    m = net.model(ctx)
    d_src, d_dst = ctx.upload(img), ctx.alloc(side * scale * side * scale * 3)
    run = lambda: m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * scale * 3, 0)  # noqa: E731
    try:
        hp, wp, halo, nt, ws = m.plan(side, side, 0)
        fl = flops(C, hidden, L, D, scale, hp, wp)
        total = sum(fl.values())
        for _ in range(2):                                       # warm-up: code objects, the activation buffers
            run()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        ctx.prof_enable(True)                                    # device time and the split, in runs of their own
        profs = []
        for _ in range(reps):
            ctx.prof_reset()
            run()
            ctx.sync()
            profs.append(ctx.prof_get())
        ctx.prof_enable(False)
    finally:
        ctx.sync()
        d_src.free(); d_dst.free()
        net.close()
    dev = [sum(p[f"swin2sr_{k}"][0] for k in NAMES if f"swin2sr_{k}" in p) for p in profs]
    prof = profs[int(np.argsort(dev)[len(dev) // 2])]            # the run whose device time is the median
    ms, dev_ms = float(np.median(ts)), float(np.median(dev))
    kern = {}
    for k in NAMES:
        if f"swin2sr_{k}" in prof:
            t, n = prof[f"swin2sr_{k}"]
            kern[k] = {"ms": round(t, 3), "launches": n, "share": round(t / dev_ms, 4)}
            if k in fl and t > 0:
                kern[k]["useful_TFLOPs_per_s"] = round(fl[k] / 1e12 / (t / 1e3), 2)
    return {"n_feat": C, "n_heads": heads, "n_hidden": hidden, "n_groups": L, "depth": D, "scale": scale, "upsampler": "pixelshuffle",
            "mask_value": net.mask_value, "input": f"{side}x{side}", "padded": f"{wp}x{hp}", "useful_TFLOP": round(total / 1e12, 4),
            "tail_pieces": nt, "tail_halo": halo, "workspace_MB": round(ws / 2 ** 20, 1), "reps": reps,
            "host_ms_median": round(ms, 3), "host_ms_min": round(min(ts), 3), "host_ms_max": round(max(ts), 3),
            "device_ms_median": round(dev_ms, 3), "device_ms_min": round(min(dev), 3), "device_ms_max": round(max(dev), 3),
            "useful_TFLOPs_per_s": round(total / 1e12 / (dev_ms / 1e3), 2),
            "frac_of_f32_matrix_peak": round(total / 1e12 / (dev_ms / 1e3) / swinir_timing.F32_MATRIX_PEAK_TFLOPS, 4), "kernels": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin2sr_timing.json"))
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    cfg = (180, 6, 360, 6, 6, 4)
    rounds = []
    for _ in range(2):                                           # alternated: SwinIR, Swin2SR, SwinIR, Swin2SR
        rounds.append((swinir_timing.time_net(ctx, *cfg, args.side, args.reps), time_net(ctx, *cfg, args.side, args.reps)))
    ratios = [b["device_ms_median"] / a["device_ms_median"] for a, b in rounds]
    sw, s2 = rounds[-1]
    out = {"date": datetime.date.today().isoformat(), "what": "device time of one forward, median of %d; Swin2SR and SwinIR of the same configuration "
           "in the same process, alternated twice" % args.reps,
           "swin2sr": s2, "swinir": sw,
           "device_ms_median_by_round": {"swinir": [a["device_ms_median"] for a, _ in rounds], "swin2sr": [b["device_ms_median"] for _, b in rounds]},
           "swin2sr_over_swinir_device_time": [round(r, 4) for r in ratios]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
