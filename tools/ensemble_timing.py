#!/usr/bin/env python3
"""Geometric self-ensemble (csrc/sr_ensemble.hip) on the GPU: for one side x side tile of each local SR family at its usual scale
-- the compact network (F 64, D 16, x2), MSRResNet (F 64, B 16, x4) and RRDBNet (F 64, G 32, B 23, x4) -- the plain u8 forward, the
ensemble at 2, 4 and 8 members, and per ensemble the time of its three bandwidth passes (HIP events, a run of its own) with the bytes
they move per second:
    d4      T_k of the u8 input                 reads and writes h w 3 bytes                      (n - 1 launches: T_0 is skipped)
    acc     acc = / += T_k^-1(forward output)   first: reads and writes 12 H W; add: reads 24 H W, writes 12 H W
    finish  acc / n -> u8                       reads 12 H W, writes 3 H W
tools/hbm_rw_probe.py is run in the same process afterwards and its copy rate recorded beside them: what a bandwidth pass can
hope for.  Nothing here is a pass / fail threshold.  Seeded synthetic weights: timing does not depend on their values.
usage: tools/ensemble_timing.py [--side 2048] [--rrdb-blocks 23] [--families compact,msrresnet,rrdb] [--out profiles/ensemble_timing.json]"""
import argparse
import contextlib
import io
import json
import os
import runpy
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

MASKS = {2: 0x03, 4: 0x0F, 8: 0xFF}


def make_net(family, rrdb_blocks):
    import sr_network
    if family == "compact":
        import srnet_timing
        return sr_network.CompactSRNet(srnet_timing.synthetic_state(64, 16, 2)), "F 64, D 16, x2"
    if family == "msrresnet":
        import resnet_timing
        return sr_network.ResidualSRNet(resnet_timing.synthetic_state("msr", 64, 16, 4)), "F 64, B 16, x4"
    import rrdb_timing
    return sr_network.RRDBSRNet(rrdb_timing.synthetic_state(64, 32, rrdb_blocks)), f"F 64, G 32, B {rrdb_blocks}, x4"


def wall_ms(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def time_family(ctx, family, side, rrdb_blocks):
    net, shape = make_net(family, rrdb_blocks)
    s = net.scale
    H = W = side * s
    img = np.random.default_rng(1).integers(0, 256, (side, side, 3), dtype=np.uint8)
    d_src, d_dst = ctx.upload(img), ctx.alloc(H * W * 3)
    m = net.model(ctx)
    plain = lambda: m.upscale_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, W * 3)
    out = {"family": family, "shape": shape, "input": f"{side}x{side}", "scale": s, "ensembles": {}}
    try:
        plain()                                                  # warm-up: code objects, the activation buffers
        out["plain_ms"] = round(min(wall_ms(ctx, plain) for _ in range(2)), 3)
        m.ensemble_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, W * 3, mask=0x10)      # warm-up: the ensemble's workspace at its largest
        for n, mask in MASKS.items():
            ens = lambda: m.ensemble_u8(d_src.ptr, side * 3, side, side, d_dst.ptr, W * 3, mask=mask)
            ms = wall_ms(ctx, ens)
            ctx.prof_enable(True)
            ctx.prof_reset()
            ens()
            ctx.sync()
            prof = ctx.prof_get()
            ctx.prof_enable(False)
            in_b, out_b = side * side * 3, H * W * 12
            moved = {"d4": 2 * in_b * (n - 1), "acc": 2 * out_b + 3 * out_b * (n - 1), "finish": out_b + H * W * 3}
            passes = {}
            for k, b in moved.items():
                t, launches = prof[f"ens_{k}"]
                passes[k] = {"ms": round(t, 4), "launches": launches, "ms_per_launch": round(t / launches, 4), "bytes": b,
                             "TB_per_s": round(b / (t / 1e3) / 1e12, 3)}
            pass_ms = sum(p["ms"] for p in passes.values())
            out["ensembles"][str(n)] = {
                "mask": mask, "ms": round(ms, 3), "ms_over_n_plain": round(ms / (n * out["plain_ms"]), 4),
                "passes_ms": round(pass_ms, 4), "passes_share_of_n_plain": round(pass_ms / (n * out["plain_ms"]), 5),
                "workspace_MB": round(__import__("_native").ens_plan(side, side, s, mask)[1] / 2 ** 20, 1), "passes": passes}
    finally:
        ctx.sync()
        d_src.free(); d_dst.free()
        net.close()
    return out


def hbm_probe():
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "tools", "hbm_rw_probe.py"))
    return json.loads(buf.getvalue().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--rrdb-blocks", type=int, default=23)
    ap.add_argument("--families", default="compact,msrresnet,rrdb")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_timing.json"))
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = {"families": []}

    def save():
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")

    for family in args.families.split(","):
        out["families"].append(time_family(ctx, family, args.side, args.rrdb_blocks))
        save()                                                   # a long run that is cut short keeps what it has
    out["hbm_rw_probe"] = hbm_probe()
    save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
