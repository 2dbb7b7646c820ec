#!/usr/bin/env python3
"""HAT (csrc/sr_hat.hip) on the GPU: ms per input tile and achieved TFLOP/s for the HAT configuration (C 180, 6 heads, hidden
360, n_mid 60, squeeze 6, L 6, D 6, x4) on a 512 x 512 input: host-timed median, device time (the sum of the HIP-event intervals
of a profiled run, median of the same number of runs) and the split linear (qkv, proj, fc1, fc2) / attention (16 x 16 windows) /
oca (the overlapping cross-attention) / cab_conv (the CAB's two 3 x 3 convolutions) / cab_pool (channel mean + attention +
scale-and-skip) / ln (LayerNorm) / conv (the trunk's 3 x 3 convolutions) / tail (the reconstruction) / head.
Seeded synthetic weights (none ship with the repository): timing does not depend on their values.  Useful FLOPs are those of
the forward, computed from the shapes on the padded image: per pixel 2 * 27 C (head), per HAB and per OCAB 2 (4 C^2 + 2 C hidden)
(linear), per HAB 4 * 256 C (q k^T and p v of a 256-token window -- once; the kernel's recomputed scores count as none) and
2 * 9 * 2 C n_mid (CAB), per OCAB 4 * 576 C, 2 * 9 C^2 per trunk convolution (L + 1 of them), and the reconstruction's
convolutions at their own resolutions; zero-padded channels, the LayerNorm, the softmax, the GELU and the pooling count as none.
In the same process, as yardsticks: SwinIR's standard case (tools/swinir_timing.py) and the trunk-convolution rate of
tools/rcan_timing.py; and one run at HAT-L depth (L 12).
usage: tools/hat_timing.py [--side 512] [--reps 7] [--out profiles/hat_timing.json] [--no-yardstick] [--no-large]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import swinir_timing  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = swinir_timing.F32_MATRIX_PEAK_TFLOPS
STAGES = swinir_timing.STAGES
SPLIT = {"head": ("head",), "ln": ("ln",), "linear": ("linear",), "attention": ("attention",), "oca": ("oca",), "cab_conv": ("cab_conv",),
         "cab_pool": ("cab_reduce", "cab_attention", "cab_scale"), "conv": ("conv",), "tail": ("tail",)}


def synthetic_state(C, heads, hidden, mid, sq, L, D, scale, seed=20261020):
    rng = np.random.default_rng(seed)
    st = {}

    def conv(name, cout, cin, gain=0.5, k=3):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (k * k * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)

    def lin(name, cout, cin):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin)) * 0.5 / np.sqrt(cin)).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)

    def norm(name):
        st[f"{name}.weight"] = rng.uniform(0.5, 1.5, C).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(C) * 0.1).astype(np.float32)

    def mlp(b):
        norm(f"{b}.norm2")
        lin(f"{b}.mlp.fc1", hidden, C)
        lin(f"{b}.mlp.fc2", C, hidden)

    conv("conv_first", C, 3)
    norm("patch_embed.norm")
    for i in range(L):
        for j in range(D):
            b = f"layers.{i}.residual_group.blocks.{j}"
            norm(f"{b}.norm1")
            lin(f"{b}.attn.qkv", 3 * C, C)
            st[f"{b}.attn.relative_position_bias_table"] = (rng.standard_normal((961, heads)) * 0.5).astype(np.float32)
            lin(f"{b}.attn.proj", C, C)
            conv(f"{b}.conv_block.cab.0", mid, C)
            conv(f"{b}.conv_block.cab.2", C, mid)
            conv(f"{b}.conv_block.cab.3.attention.1", sq, C, 1.0, 1)
            conv(f"{b}.conv_block.cab.3.attention.3", C, sq, 1.0, 1)
            mlp(b)
        o = f"layers.{i}.residual_group.overlap_attn"
        norm(f"{o}.norm1")
        lin(f"{o}.qkv", 3 * C, C)
        st[f"{o}.relative_position_bias_table"] = (rng.standard_normal((1521, heads)) * 0.5).astype(np.float32)
        lin(f"{o}.proj", C, C)
        mlp(o)
        conv(f"layers.{i}.conv", C, C)
    norm("norm")
    conv("conv_after_body", C, C)
    conv("conv_before_upsample.0", 64, C)
    for k, r in enumerate(STAGES[scale]):
        conv(f"upsample.{2 * k}", 64 * r * r, 64)
    conv("conv_last", 3, 64, 0.1)
    return st


def flops(C, hidden, mid, L, D, scale, hp, wp):
    px = float(hp) * wp
    tail, m = 2.0 * 9 * C * 64 * px, 1
    for r in STAGES[scale]:
        tail += 2.0 * 9 * 64 * 64 * r * r * m * m * px
        m *= r
    tail += 2.0 * 9 * 64 * 3 * scale * scale * px
    return {"head": 2.0 * 27 * C * px, "linear": 2.0 * (4 * C * C + 2 * C * hidden) * L * (D + 1) * px, "attention": 4.0 * 256 * C * L * D * px,
            "oca": 4.0 * 576 * C * L * px, "cab_conv": 2.0 * 9 * 2 * C * mid * L * D * px, "conv": 2.0 * 9 * C * C * (L + 1) * px, "tail": tail}


def time_net(ctx, C, heads, hidden, mid, sq, L, D, scale, side, reps):
    import sr_network
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    net = sr_network.HATSRNet(synthetic_state(C, heads, hidden, mid, sq, L, D, scale))
    m = net.model(ctx)
    d_src, d_dst = ctx.upload(img), ctx.alloc(side * scale * side * scale * 3)
    run = lambda: m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, side * scale * 3, 0)
    try:
        hp, wp, halo, nt, ws = m.plan(side, side, 0)
        fl = flops(C, hidden, mid, L, D, scale, hp, wp)
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
    scopes = [f"hat_{s}" for parts in SPLIT.values() for s in parts]
    dev = [sum(p[s][0] for s in scopes if s in p) for p in profs]
    prof = profs[int(np.argsort(dev)[len(dev) // 2])]            # the run whose device time is the median
    ms, dev_ms = float(np.median(ts)), float(np.median(dev))
    kern = {}
    for k, parts in SPLIT.items():
        got = [prof[f"hat_{s}"] for s in parts if f"hat_{s}" in prof]
        if got:
            t, n = sum(g[0] for g in got), sum(g[1] for g in got)
            kern[k] = {"ms": round(t, 3), "launches": n, "share": round(t / dev_ms, 4)}
            if k in fl and t > 0:
                kern[k]["useful_TFLOPs_per_s"] = round(fl[k] / 1e12 / (t / 1e3), 2)
    return {"n_feat": C, "n_heads": heads, "n_hidden": hidden, "n_mid": mid, "n_squeeze": sq, "n_groups": L, "depth": D, "scale": scale,
            "input": f"{side}x{side}", "padded": f"{wp}x{hp}", "useful_TFLOP": round(total / 1e12, 4), "tail_pieces": nt, "tail_halo": halo,
            "workspace_MB": round(ws / 2 ** 20, 1), "reps": reps,
            "host_ms_median": round(ms, 3), "host_ms_min": round(min(ts), 3), "host_ms_max": round(max(ts), 3),
            "device_ms_median": round(dev_ms, 3), "device_ms_min": round(min(dev), 3), "device_ms_max": round(max(dev), 3),
            "useful_TFLOPs_per_s": round(total / 1e12 / (dev_ms / 1e3), 2),
            "frac_of_f32_matrix_peak": round(total / 1e12 / (dev_ms / 1e3) / F32_MATRIX_PEAK_TFLOPS, 4), "kernels": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hat_timing.json"))
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    out = {"nets": [time_net(ctx, 180, 6, 360, 60, 6, 6, 6, 4, args.side, args.reps)]}
    if not args.no_large:
        out["hat_l_depth"] = time_net(ctx, 180, 6, 360, 60, 6, 12, 6, 4, args.side, 1)
    if not args.no_yardstick:
        import rcan_timing
        s = swinir_timing.time_net(ctx, 180, 6, 360, 6, 6, 4, args.side, args.reps)
        out["yardstick_swinir"] = {"what": "tools/swinir_timing.py, C 180, 6 heads, hidden 360, L 6, D 6, x4, same process",
                                   "device_ms_median": s["device_ms_median"], "host_ms_median": s["host_ms_median"],
                                   "attention_ms": s["kernels"]["attention"]["ms"], "linear_useful_TFLOPs_per_s":
                                   s["kernels"]["linear"].get("useful_TFLOPs_per_s")}
        y = rcan_timing.time_net(ctx, 64, 4, 10, 20, 4, args.side, args.reps)
        out["yardstick_rcan_3x3"] = {"what": "tools/rcan_timing.py, F 64, G 10, B 20, x4, the trunk convolutions, same process",
                                     "conv_useful_TFLOPs_per_s": y["kernels"]["conv"].get("useful_TFLOPs_per_s"), "ms_median": y["ms_median"]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
