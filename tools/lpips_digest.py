#!/usr/bin/env python3
"""The float64 bit patterns of what LPIPS and DISTS return, for holding a change of their shared convolution
(csrc/sr_vgg_stream.h, csrc/sr_conv_mfma.h) against its parent bit for bit: the five layer sums of sr_lpips_u8 for VGG and
AlexNet on a seeded 300 x 420 pair, untiled and at tiles 64, 128 and 304 (float.hex of each), and the 1475 x 5 sums of
sr_dists_u8 on the same pair at tile 128 (SHA-256 of the array and float.hex of the five column totals).  Run it once per build,
each in a fresh process (SR_LIB_PATH names the other build's library), and compare the two outputs: equal code gives equal
lines.  usage: tools/lpips_digest.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

H, W = 300, 420
TILES = (0, 64, 128, 304)


def pair():
    rng = np.random.default_rng(20260313)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None]
    a = np.clip(base + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float32) + rng.normal(0, 9.0, (H, W, 3)), 0, 255).astype(np.uint8)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import _native
    ctx = _native.default_context(0)
    res = {"library": os.path.basename(os.path.dirname(os.path.abspath(_native.LIB_PATH))) + "/" + os.path.basename(_native.LIB_PATH),
           "source_digest": _native.load().sr_source_digest().decode()}
    a, b = pair()
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for net in ("vgg", "alex"):
            model = _native.LpipsModel(ctx, net, _native.lpips_synthetic_weights(net))
            for tile in TILES:
                sums = model.layer_sums(da.ptr, W * 3, db.ptr, W * 3, H, W, 3, tile)
                res[f"lpips {net} {H}x{W} tile {tile}"] = [float(s).hex() for s in sums]
            model.close()
        model = _native.DistsModel(ctx, _native.dists_synthetic_weights())
        sums = model.sums(da.ptr, W * 3, db.ptr, W * 3, H, W, 3, 128)
        res[f"dists {H}x{W} tile 128 sha256"] = hashlib.sha256(np.ascontiguousarray(sums).tobytes()).hexdigest()
        res[f"dists {H}x{W} tile 128 column totals"] = [float(s).hex() for s in sums.sum(axis=0)]
        model.close()
    finally:
        da.free(); db.free()
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
