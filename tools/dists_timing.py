#!/usr/bin/env python3
"""DISTS against LPIPS-VGG on the same buffers at the same tile: device time of sr_dists_u8 and sr_lpips_u8 on one synthetic
pair (HIP events around the whole call, median of --reps), then one profiled call each for the split into convolutions, the L2
pooling and the per-channel sums, and the achieved GB/s of the two new kernels beside the device's copy rate measured in the
same process (the y.copy_(x) of tools/hbm_rw_probe.py).  Writes profiles/dists_timing.json and prints it.
usage: tools/dists_timing.py [--size HxW | --workload 200MP-kd] [--tile 4096] [--reps 7]
Synthetic seeded weights (no pretrained weights offline): timing does not depend on their values."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def new_kernel_bytes(sizes, channels):
    """Bytes the two new kernels move for both images, from the untiled geometry (tile halos of the pooling not counted):
    the pooling reads stage k's map and writes a quarter of it; the sums read every stage's two maps (stage 0: u8 HWC)."""
    pool = 0
    for k in range(1, 5):
        (h, w), (ho, wo) = sizes[k], sizes[k + 1]
        pool += 2 * channels[k] * (h * w + ho * wo) * 4
    stats = 2 * sizes[0][0] * sizes[0][1] * 3
    for k in range(1, 6):
        stats += 2 * channels[k] * sizes[k][0] * sizes[k][1] * 4
    return pool, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default=None)
    ap.add_argument("--workload", default="200MP-kd", help="take the canvas size of a bench workload")
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dists_timing.json"))
    args = ap.parse_args()
    import torch
    import _native
    import device_pipeline as dp
    if args.size:
        H, W = (int(v) for v in args.size.lower().split("x"))
    else:
        g = dp.workload_geometry(args.workload)
        H, W = g.canvas_h, g.canvas_w
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = _native.Context(0, stream=stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(1)
    a = torch.randint(0, 256, (H, W * 3), dtype=torch.uint8, device=dev, generator=gen)
    noise = torch.randint(-6, 7, (H, W * 3), dtype=torch.int16, device=dev, generator=gen)
    b = (a.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    del noise

    def timed(fn):
        fn()                                   # warm-up: allocates the activation buffers
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def profiled(fn):
        ctx.prof_enable(True)
        ctx.prof_reset()
        fn()
        torch.cuda.synchronize()
        prof = {k: round(v[0], 3) for k, v in ctx.prof_get().items()}
        ctx.prof_enable(False)
        return prof

    out = {"image": f"{W}x{H}", "megapixels": round(H * W / 1e6, 2), "tile": args.tile, "reps": args.reps}
    ap_, bp_ = a.data_ptr(), b.data_ptr()
    dists = _native.DistsModel(ctx, _native.dists_synthetic_weights())
    run_d = lambda: dists.sums(ap_, W * 3, bp_, W * 3, H, W, 3, args.tile)          # noqa: E731
    ms_d = timed(run_d)
    prof_d = profiled(run_d)
    sizes = dists.layer_sizes(H, W)
    dists.close()
    lpips = _native.LpipsModel(ctx, "vgg", _native.lpips_synthetic_weights("vgg"))
    run_l = lambda: lpips.layer_sums(ap_, W * 3, bp_, W * 3, H, W, 3, args.tile)     # noqa: E731
    ms_l = timed(run_l)
    prof_l = profiled(run_l)
    lpips.close()
    # the device's copy rate, in this process: 1 GiB y.copy_(x), read + write
    n = 2**30 // 4
    x = torch.empty(n, dtype=torch.float32, device=dev).fill_(1.0)
    y = torch.empty_like(x)
    copy_ms = statistics.median(timed(lambda: y.copy_(x)))
    copy_gbps = 2 * n * 4 / copy_ms / 1e6
    pool_b, stats_b = new_kernel_bytes(sizes, _native.DISTS_CHANNELS)
    med_d, med_l = statistics.median(ms_d), statistics.median(ms_l)
    conv_d = prof_d.get("dists_conv_mfma", 0.0) + prof_d.get("dists_conv_stem", 0.0)
    out.update({
        "dists_ms": {"median": round(med_d, 2), "min": round(min(ms_d), 2), "max": round(max(ms_d), 2)},
        "lpips_vgg_ms": {"median": round(med_l, 2), "min": round(min(ms_l), 2), "max": round(max(ms_l), 2)},
        "dists_over_lpips_vgg": round(med_d / med_l, 4),
        "dists_split_ms_profiled_call": {"convolutions": round(conv_d, 2), "l2pool": prof_d.get("dists_l2pool", 0.0),
                                         "stats": prof_d.get("dists_stats", 0.0)},
        "dists_kernel_ms": prof_d, "lpips_vgg_kernel_ms": prof_l,
        "copy_GBps_rw_1GiB": round(copy_gbps, 1),
        "l2pool": {"GB_untiled": round(pool_b / 1e9, 2),
                   "GBps": None if not prof_d.get("dists_l2pool") else round(pool_b / prof_d["dists_l2pool"] / 1e6, 1)},
        "stats": {"GB_untiled": round(stats_b / 1e9, 2), "includes": "the fixed-order accumulate launches",
                  "GBps": None if not prof_d.get("dists_stats") else round(stats_b / prof_d["dists_stats"] / 1e6, 1)},
    })
    for k in ("l2pool", "stats"):
        if out[k]["GBps"]:
            out[k]["frac_of_copy_rate"] = round(out[k]["GBps"] / copy_gbps, 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
