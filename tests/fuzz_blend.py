#!/usr/bin/env python3
"""Randomised parity sweep (GPU box): random tile arrangements, sizes, levels, weight types, channel counts, dtypes and
row windows through the HIP blend against the CPU oracle, bit for bit.  Also the fused assessment on random shapes.
Test infrastructure (it drives the oracle); tests/test_gpu_fuzz.py runs a short sweep.
usage: python tests/fuzz_blend.py [cases] [seed]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-system_amd")):
    sys.path.insert(0, p)
import numpy as np            # noqa: E402
import _native                # noqa: E402
from oracle import oracle_c as oc   # noqa: E402  (checker only)



def run(cases: int = 200, seed: int = 1) -> int:
    rng = np.random.default_rng(seed)
    ctx = _native.default_context(0)
    bad = 0
    compared = rejected = strips = 0
    for it in range(cases):
        # both forms of the canvas gather: the march (forced: the default takes it from 90 MP of canvas up) and the block kernel
        os.environ["SR_MARCH"] = "2" if it % 3 else "1"
        # the remainder of a marched gather: rectangles of cells (default; every 7th case small ones)
        os.environ["SR_RECT_CELLS"] = "48" if it % 7 == 3 else "256"
        n = int(rng.integers(1, 7))
        cn = int(rng.choice([1, 3]))
        levels = int(rng.integers(1, 7))
        wt = str(rng.choice(["cosine", "linear", "sigmoid"]))
        f32 = bool(rng.integers(0, 4) == 0)
        tiles, pos = [], []
        for _ in range(n):
            h, w = int(rng.integers(9, 520)), int(rng.integers(9, 660))
            if rng.integers(0, 25) == 0:
                h, w = int(rng.integers(2, 9)), int(rng.integers(2, 12))       # tiny tiles: few levels
            shape = (h, w, 3) if cn == 3 else (h, w)
            base = rng.integers(0, 256, shape)
            t = base.astype(np.float32) * np.float32(0.93) + np.float32(1.7) if f32 else base.astype(np.uint8)
            tiles.append(t)
            pos.append((int(rng.integers(0, 400)), int(rng.integers(0, 520))))
        H = max(p[0] + t.shape[0] for p, t in zip(pos, tiles)) - int(rng.integers(0, 7))
        W = max(p[1] + t.shape[1] for p, t in zip(pos, tiles)) - int(rng.integers(0, 7))
        H, W = max(H, 2), max(W, 2)
        lap = bool(rng.integers(0, 5) != 0)
        try:
            if lap:
                want = oc.laplacian_fusion(tiles, pos, (H, W), levels, wt)
            else:
                want = oc.weighted_average_fusion(tiles, pos, (H, W), wt)
        except Exception as exc:                      # the oracle rejects what the reference rejects (e.g. 1-px tiles)
            want, oerr = None, exc
        try:
            got = ctx.fusion_np(tiles, pos, (H, W), levels, wt, laplacian=lap)
        except Exception as exc:
            got, gerr = None, exc
        if want is None or got is None:
            if (want is None) != (got is None):
                bad += 1
                print("MISMATCH in error behaviour", it, n, cn, levels, wt, f32, lap, [t.shape for t in tiles], pos, (H, W))
            rejected += 1
            continue
        compared += 1
        if not np.array_equal(got, want):
            bad += 1
            d = np.argwhere(got != want)
            print("MISMATCH", it, dict(n=n, cn=cn, levels=levels, wt=wt, f32=f32, lap=lap, shapes=[t.shape for t in tiles], pos=pos,
                                       canvas=(H, W)), "first diffs", d[:3].tolist(), "count", len(d))
        # the same canvas from two or three row-window plans (strip owners), u8 tiles
        if lap and not f32 and H >= 8 and rng.integers(0, 2) == 0:
            strips += 1
            rects = [(p[1], p[0], t.shape[1], t.shape[0]) for p, t in zip(pos, tiles)]
            bufs = [ctx.upload(np.ascontiguousarray(t)) for t in tiles]
            canvas = ctx.alloc(H * W * cn)
            ctx.memset(canvas.ptr, 0, H * W * cn)
            cuts = sorted(set([0, H] + [int(v) // 2 * 2 for v in rng.integers(1, H, int(rng.integers(1, 3)))]))
            for a_, b_ in zip(cuts[:-1], cuts[1:]):
                if b_ <= a_:
                    continue
                plan = _native.BlendPlan(ctx, rects, cn, H, W, levels, wt, a_, b_)
                plan.blend([bf.ptr for bf in bufs], [t.shape[1] * cn for t in tiles], canvas.ptr, W * cn)
                ctx.sync()
                plan.close()
            got2 = ctx.download(canvas.ptr, (H, W, 3) if cn == 3 else (H, W), np.uint8)
            if not np.array_equal(got2, want):
                bad += 1
                print("STRIP MISMATCH", it, dict(n=n, cn=cn, levels=levels, wt=wt, shapes=[t.shape for t in tiles], pos=pos,
                                                 canvas=(H, W), cuts=cuts))
            for bf in bufs:
                bf.free()
            canvas.free()
    # TilingModule.merge_tiles feather path: random tiles (resized or not), ramps, canvas crops
    from oracle import oracle_np as onp
    merges = 0
    for it in range(max(cases // 3, 10)):
        n = int(rng.integers(1, 7))
        Wc, Hc = int(rng.integers(40, 700)), int(rng.integers(30, 500))
        datas, metas, descs = [], [], []
        for _ in range(n):
            ow, oh = int(rng.integers(8, 300)), int(rng.integers(8, 240))
            if rng.integers(0, 2):
                sw, sh = ow, oh
            else:
                sw, sh = max(2, int(ow * rng.uniform(0.3, 1.6))), max(2, int(oh * rng.uniform(0.3, 1.6)))
            x, y = int(rng.integers(0, Wc)), int(rng.integers(0, Hc))
            ov = [int(rng.integers(0, max(1, min(oh, ow) // 2))) if rng.integers(0, 3) else 0 for _ in range(4)]
            ov[0], ov[1] = min(ov[0], oh), min(ov[1], oh)
            ov[2], ov[3] = min(ov[2], ow), min(ov[3], ow)
            datas.append(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8))
            metas.append(dict(global_x=x, global_y=y, output_w=ow, output_h=oh, overlap_top=ov[0], overlap_bottom=ov[1],
                              overlap_left=ov[2], overlap_right=ov[3]))
            descs.append(dict(x=x, y=y, src_w=sw, src_h=sh, out_w=ow, out_h=oh, ov_t=ov[0], ov_b=ov[1], ov_l=ov[2], ov_r=ov[3]))
        blending = bool(rng.integers(0, 4) != 0)
        want = onp.merge_tiles(datas, metas, Wc, Hc, 1.0, blending)
        got = ctx.feather_merge_np(datas, descs, Wc, Hc, blending)
        merges += 1
        if not np.array_equal(got, want):
            bad += 1
            d = np.argwhere(got != want)
            print("MERGE MISMATCH", it, metas, (Hc, Wc), blending, "first diffs", d[:3].tolist(), "count", len(d))
    # strip partitions: every rank of a random world over a random (grid or k-d) geometry, rehearsed with only the rows
    # its exchange plan delivers, reproduces its rows of the monolithic canvas and the metric sums add up
    import torch
    import device_pipeline as dp
    worlds = 0
    for it in range(max(cases // 20, 3)):
        if rng.integers(0, 2):
            geo = dp.kd_geometry(int(rng.integers(500, 1500)), int(rng.integers(400, 1200)), leaves=int(rng.integers(3, 14)),
                                 overlap=float(rng.uniform(0.10, 0.2)), seed=int(rng.integers(0, 1 << 30)))
        else:
            tw, th = int(rng.integers(120, 420)), int(rng.integers(100, 380))
            geo = dp.grid_geometry(tile_w=tw, tile_h=th, rows=int(rng.integers(1, 5)), cols=int(rng.integers(1, 5)),
                                   ov_x=int(tw * rng.uniform(0.1, 0.3)), ov_y=int(th * rng.uniform(0.1, 0.3)))
        if geo.canvas_h < 64:
            continue
        world = int(rng.integers(2, 9))
        Hc, Wc = geo.canvas_h, geo.canvas_w
        image = torch.from_numpy(rng.integers(0, 256, (Hc, Wc * 3), dtype=np.uint8)).cuda()
        reference = torch.from_numpy(rng.integers(0, 256, (Hc, Wc * 3), dtype=np.uint8)).cuda()
        mono = dp.DevicePipeline(geo, 0, 1, 0)
        mono.step(image, reference)
        torch.cuda.synchronize()
        full = {t: mono.local_tiles[t] for t in range(len(geo.rects))}
        sums = torch.zeros_like(mono.results)
        ok = True
        for r in range(world):
            pr = dp.DevicePipeline(geo, r, world, 0)
            pr.rehearse_fill(full)
            pr.rehearse_step(reference, staged=bool(rng.integers(0, 2)))
            torch.cuda.synchronize()
            a_, b_ = pr.strip
            ok = ok and torch.equal(pr.canvas[a_:b_], mono.canvas[a_:b_])
            sums += pr.results
            pr.close()
        ok = ok and float(sums[0]) == float(mono.results[0]) and bool(torch.allclose(sums[1:], mono.results[1:], rtol=1e-12, atol=0))
        worlds += 1
        if not ok:
            bad += 1
            print("WORLD MISMATCH", it, world, (Hc, Wc), geo.rects)
        mono.close()
    # bicubic resize (cv2.INTER_CUBIC semantics), up and down, 1 and 3 channels
    resizes = 0
    for it in range(max(cases // 4, 10)):
        h, w = int(rng.integers(2, 200)), int(rng.integers(2, 260))
        dh, dw = max(1, int(h * rng.uniform(0.1, 6.0))), max(1, int(w * rng.uniform(0.1, 6.0)))
        cn = int(rng.choice([1, 3]))
        a = rng.integers(0, 256, (h, w, 3) if cn == 3 else (h, w), dtype=np.uint8)
        da = ctx.upload(a)
        dd = ctx.alloc(dh * dw * cn)
        ctx.resize_cubic_u8(da.ptr, w * cn, h, w, cn, dd.ptr, dw * cn, dh, dw)
        got = ctx.download(dd.ptr, (dh, dw, 3) if cn == 3 else (dh, dw), np.uint8)
        resizes += 1
        if not np.array_equal(got, oc.resize_cubic_u8(a, dw, dh)):
            bad += 1
            print("RESIZE MISMATCH", it, a.shape, (dh, dw))
        da.free(); dd.free()
    # fused assessment on random shapes
    for it in range(max(cases // 4, 10)):
        h, w = int(rng.integers(7, 400)), int(rng.integers(7, 700))
        cn = int(rng.choice([1, 3]))
        shape = (h, w, 3) if cn == 3 else (h, w)
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
        da, db = ctx.upload(a), ctx.upload(b)
        r = ctx.assess_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn)
        g0 = oc.rgb2gray_u8(a) if cn == 3 else a
        g1 = oc.rgb2gray_u8(b) if cn == 3 else b
        ok = r["sse"] == float(np.sum((a.astype(np.int64) - b.astype(np.int64)) ** 2))
        for mode in ("uniform", "gauss", "simple"):
            cnt = _native.ssim_count(h, w, mode)
            if cnt:
                ok = ok and abs(r[f"ssim_{mode}"] / cnt - oc.ssim(g0, g1, mode)) <= 1e-9
        if not ok:
            bad += 1
            print("ASSESS MISMATCH", it, shape)
        da.free(); db.free()
    # resized assessment (the downsample comparison of evaluate_full_reference): sample both images with INTER_CUBIC, then
    # PSNR-SSE + SSIM on the resized pair -- against resize-then-assess through the oracle
    rs = 0
    for it in range(max(cases // 4, 10)):
        h, w = int(rng.integers(12, 400)), int(rng.integers(12, 600))
        dh, dw = max(7, int(h * rng.uniform(0.08, 1.3))), max(7, int(w * rng.uniform(0.08, 1.3)))
        cn = int(rng.choice([1, 3]))
        shape = (h, w, 3) if cn == 3 else (h, w)
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-25, 26, shape), 0, 255).astype(np.uint8)
        da, db = ctx.upload(a), ctx.upload(b)
        r = ctx.assess_resized_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, dh, dw, flags=_native.ASSESS_ALL)
        ra, rb = oc.resize_cubic_u8(a, dw, dh), oc.resize_cubic_u8(b, dw, dh)
        g0 = oc.rgb2gray_u8(ra) if cn == 3 else ra
        g1 = oc.rgb2gray_u8(rb) if cn == 3 else rb
        ok = r["sse"] == float(np.sum((ra.astype(np.int64) - rb.astype(np.int64)) ** 2))
        for mode in ("uniform", "gauss", "simple"):
            cnt = _native.ssim_count(dh, dw, mode)
            if cnt:
                ok = ok and abs(r[f"ssim_{mode}"] / cnt - oc.ssim(g0, g1, mode)) <= 1e-9
        rs += 1
        if not ok:
            bad += 1
            print("RESIZED ASSESS MISMATCH", it, shape, (dh, dw))
        da.free(); db.free()
    print(f"fuzz: {rs} resized assessments; ", end="")
    print(f"fuzz: {cases} blend cases ({compared} compared, {rejected} rejected by both, {strips} also as strips) + "
          f"{merges} feather merges + {worlds} strip worlds + {resizes} resizes + {max(cases // 4, 10)} assessment cases, {bad} mismatches")
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
