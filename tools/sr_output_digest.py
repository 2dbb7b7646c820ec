#!/usr/bin/env python3
"""SHA-256 of what the two window-attention backends (SwinIR, HAT) put out, for holding a host-side refactor against its parent
bit for bit: the seeded synthetic networks of the GPU tests (tests/_swinir_ref.py and tests/_hat_ref.py, CASES + EDGE_CASES --
the small shapes, nothing larger), each at two ``tail`` values, the u8 and the fp32 output; one ensemble output per family (all
eight members, fp32 and u8); one call each of swinir_layernorm, swinir_attention, hat_attention and hat_oca on seeded tensors.
Run it once per build, each in a fresh process, and compare the two lists: equal code gives equal lines.
usage: tools/sr_output_digest.py [--root TREE] [--out FILE]     TREE: the checkout whose package (and library) is loaded; the
                                                                 default is this file's own."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAILS = (0, 7)                                                     # the library's choice (one sub-piece here) and many small ones


def sha(a) -> str:
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def forwards(ctx, net, img, ensemble: bool):
    """-> {label: digest} of the model's outputs on img at both tails."""
    import numpy as np
    h, w = img.shape[:2]
    s, m = net.scale, net.model(ctx)
    n = h * s * w * s * 3
    d_src, d_u8, d_f32 = ctx.upload(img), ctx.alloc(n), ctx.alloc(n * 4)
    out = {}
    try:
        for tail in TAILS:
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_u8.ptr, w * s * 3, tail)
            m.forward_f32(d_src.ptr, w * 3, h, w, d_f32.ptr, w * s * 3 * 4, tail)
            out[f"u8 tail {tail}"] = sha(ctx.download(d_u8.ptr, (h * s, w * s, 3), np.uint8))
            out[f"f32 tail {tail}"] = sha(ctx.download(d_f32.ptr, (h * s, w * s, 3), np.float32))
            if ensemble:
                m.ensemble_u8(d_src.ptr, w * 3, h, w, d_u8.ptr, w * s * 3, tail, mask=255)
                m.ensemble_f32(d_src.ptr, w * 3, h, w, d_f32.ptr, w * s * 3 * 4, tail, mask=255)
                out[f"ens u8 tail {tail}"] = sha(ctx.download(d_u8.ptr, (h * s, w * s, 3), np.uint8))
                out[f"ens f32 tail {tail}"] = sha(ctx.download(d_f32.ptr, (h * s, w * s, 3), np.float32))
    finally:
        for b in (d_src, d_u8, d_f32):
            b.free()
    return out


def planar_call(ctx, x, planes_out, call):
    """x (P, h, w) fp32 dense on the device -> the (planes_out, h, w) result of call(d_x, plane stride, row stride, d_out, ...)."""
    import numpy as np
    P, h, w = x.shape
    d_x, d_out = ctx.upload(np.ascontiguousarray(x, dtype=np.float32)), ctx.alloc(planes_out * h * w * 4)
    try:
        call(d_x.ptr, h * w * 4, w * 4, d_out.ptr, h * w * 4, w * 4)
        return sha(ctx.download(d_out.ptr, (planes_out, h, w), np.float32))
    finally:
        d_x.free(); d_out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (os.path.join(root, "tests"), os.path.join(root, "super-resolution-system_amd"), root):
        sys.path.insert(0, p)
    import numpy as np
    import _hat_ref as H
    import _native
    import _swinir_ref as S
    import sr_network
    ctx = _native.default_context(0)
    res = {"library": _native.load()._name}
    for i, c in enumerate(S.CASES + S.EDGE_CASES):
        st = S.synthetic_state(*c[:7])
        net = sr_network.SwinIRSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"])
        for k, v in forwards(ctx, net, S.make_image(c[7], c[8]), ensemble=i == 0).items():
            res[f"swinir {S.case_id(c)} {k}"] = v
        net.close()
    for i, c in enumerate(H.CASES + H.EDGE_CASES):
        st = H.synthetic_state(*c[:8])
        net = sr_network.HATSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"], conv_scale=float(st["conv_scale"]))
        for k, v in forwards(ctx, net, H.make_image(c[8], c[9]), ensemble=i == 0).items():
            res[f"hat {H.case_id(c)} {k}"] = v
        net.close()
    rng = np.random.default_rng(20261020)
    C, heads = 60, 6
    x = rng.standard_normal((C, 13, 21)).astype(np.float32)
    g, b = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    res["swinir_layernorm C60 13x21"] = planar_call(ctx, x, C, lambda dx, ps, rs, do, ops, ors: _native.swinir_layernorm(
        ctx, dx, ps, rs, C, 13, 21, g, b, do, ops, ors))
    qkv8, qkv16 = (rng.standard_normal((3 * C, hp, wp)).astype(np.float32) for hp, wp in ((16, 24), (32, 48)))
    t8, t16, toca = (rng.standard_normal((rows, heads)).astype(np.float32) for rows in (225, _native.HAT_REL_ROWS, _native.HAT_OCA_ROWS))
    res["swinir_attention C60 16x24 shift 4"] = planar_call(ctx, qkv8, C, lambda dx, ps, rs, do, ops, ors: _native.swinir_attention(
        ctx, dx, ps, rs, C, heads, 16, 24, 4, t8, do, ops, ors))
    res["hat_attention C60 32x48 shift 8"] = planar_call(ctx, qkv16, C, lambda dx, ps, rs, do, ops, ors: _native.hat_attention(
        ctx, dx, ps, rs, C, heads, 32, 48, 8, t16, do, ops, ors))
    res["hat_oca C60 32x48"] = planar_call(ctx, qkv16, C, lambda dx, ps, rs, do, ops, ors: _native.hat_oca(
        ctx, dx, ps, rs, C, heads, 32, 48, toca, None, do, ops, ors))
    res["library"] = os.path.relpath(res["library"], root)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
