"""GPU: every strided entry point of include/sr_hip.h on padded, offset, guarded views (tests/_views.py).

(sr_weighted_blend_custom included: tiles, fp32 weight maps and the canvas are three kinds of views.)

Each test lays its inputs and outputs into parents full of a fill byte -- base residues 0..3, 7, 12 mod 16, stride residues
0..3 mod 4 and a 64-byte gap, input and output layouts chosen independently -- and asserts (a) the result: the reference and
tolerance of the entry point's own test where that is a few lines (the C oracle, oracle_np, the tests/_*_ref.py
restatements, plain NumPy), and equality with the same call on dense aligned buffers where both forms run the same kernels
(documented as "equal inputs give equal bytes / bits") -- for sr_commercial_u8, sr_saliency_u8,
sr_tile_ssim_sums_u8, sr_lpips_u8 and the magnitude sum of sr_gradient_stats_u8 the dense call is the ONLY reference here:
these tests show that the layout does not matter, the entry points' own test files hold the dense call against the
independent restatements; (b) check_guard on every output parent: not one byte outside the
view changed.  Two fills: a kernel that reads outside its rectangle gives different results under the two, one of which
then misses the reference.  Assertion messages name the layout.

The last section addresses rows through strides whose products with a row count pass 2^32."""
import numpy as np
import pytest

import _native
import _views as V
from oracle import oracle_c as oc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

NL = len(V.LAYOUTS_U8)
LAY_IDS = [V.layout_id(l) for l in V.LAYOUTS_U8]
FILL = pytest.mark.parametrize("fill", V.FILLS, ids=lambda f: f"fill{f:02x}")
LAYK = pytest.mark.parametrize("k", range(NL), ids=LAY_IDS)
MARCH_FORMS = [pytest.param("2", {}, id="2-env0"),
               pytest.param("2", {"SR_MARCH_TAIL": "0", "SR_MARCH_ROUNDS": "6,6,6", "SR_RECT_CELLS": "64"}, id="2-env2"),
               pytest.param("1", {}, id="1-env3")]


# input layout k goes with output layout _ok(k): k = 0 pairs the aligned dense input with a misaligned output (off3-pad2),
# k = 9 a misaligned input (off1-pad0) with the aligned dense output; every output layout occurs once
def _ok(k: int) -> int:
    return (5 * k + 3) % NL


def _lay(k: int, f32: bool = False):
    return V.pick(V.LAYOUTS_F32 if f32 else V.LAYOUTS_U8, k)


def _in(ctx, arr, k, fill):
    """-> (parent, ptr, stride, tag) of `arr` as a view in layout k of its type's list."""
    lay = _lay(k, arr.dtype != np.uint8)
    p, ptr, st = V.embed(ctx, arr, lay[0], lay[1], fill)
    return p, ptr, st, V.layout_id(lay)


def _out(ctx, h, rowbytes, k, fill, f32=False, dense=False):
    lay = _lay(k, f32)
    if dense:
        lay = (lay[0], 0)
    p, ptr, st = V.out_view(ctx, h, rowbytes, lay[0], lay[1], fill)
    return p, ptr, st, V.layout_id(lay)


def _free(*ps):
    for p in ps:
        p.free()


def _scene(rng, h, w, cn=3, i=0):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 64 * np.sin(xx / 37.0 + i) + 48 * np.cos(yy / 23.0 + 0.5 * i)
    img = np.clip(base[..., None] + rng.integers(-12, 13, (h, w, max(cn, 1))) + 7 * i, 0, 255).astype(np.uint8)
    return img if cn > 1 else img[..., 0]


def _pair(rng, h, w, cn=3):
    a = _scene(rng, h, w, cn)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _rb(a):
    return a.nbytes // a.shape[0]


# widths whose row length w * 3 is 1, 3, 15, 0, 6 and 1 mod 16; heights that are not multiples of 4, 8 or 16
SHAPES = [(37, 43), (50, 33), (41, 53), (64, 64), (131, 66), (19, 11)]


# ---- tile stage ---------------------------------------------------------------------------------------------------------
@FILL
@LAYK
def test_tile_extract(ctx, rng, k, fill):
    for cn in (3, 1):
        H, W = 90, 141
        img = rng.integers(0, 256, (H, W, cn), dtype=np.uint8)
        pi, ip, ist, itag = _in(ctx, img, k, fill)
        # row lengths 1, 3, 15, 0 mod 16 (cn 3: 43, 33, 37, 64 pixels), one tile on the image's right / bottom edge
        xywh = [(5, 3, 43, 37), (98, 40, 43, 50), (0, 0, 33, 19), (17, 9, 37, 41), (77, 26, 64, 64)]
        outs = [_out(ctx, h, w * cn, _ok(k) + 5 * j, fill) for j, (_, _, w, h) in enumerate(xywh)]
        ctx.tile_extract(ip, H, W, cn, ist, xywh, [o[1] for o in outs], [o[2] for o in outs])
        for (x, y, w, h), o in zip(xywh, outs):
            what = f"sr_tile_extract cn {cn} image {itag} tile {(x, y, w, h)} -> {o[3]}"
            got = V.check_guard(ctx, o[0], np.uint8, (h, w, cn), what=what)
            assert np.array_equal(got, img[y:y + h, x:x + w]), what
        _free(pi, *[o[0] for o in outs])


@FILL
@pytest.mark.parametrize("mode", ["mirror", "replicate", "reflect", "constant"])
def test_tile_extract_pad(ctx, rng, mode, fill):
    img = rng.integers(0, 256, (75, 107, 3), dtype=np.uint8)
    block, ov = 48, 10
    xywh = _native.tile_plan(107, 75, block, ov)
    for k in range(NL):
        pi, ip, ist, itag = _in(ctx, img, k, fill)
        po, op, _, otag = _out(ctx, len(xywh) * block, block * 3, _ok(k), fill, dense=True)       # d_tiles is contiguous by the ABI
        ctx.tile_extract_pad(ip, 75, 107, 3, ist, xywh, block, mode, op)
        what = f"sr_tile_extract_pad {mode} image {itag} -> tiles {otag}"
        got = V.check_guard(ctx, po, np.uint8, (len(xywh), block, block, 3), what=what)
        for i, (x, y, w, h) in enumerate(xywh):
            assert np.array_equal(got[i], oc.tile_extract_pad(img, x, y, w, h, block, mode)), (what, i)
        _free(pi, po)


@FILL
@LAYK
def test_gray_moments(ctx, rng, k, fill):
    n, h, w = 3, 37, 43
    tiles = rng.integers(0, 256, (n * h, w, 3), dtype=np.uint8)         # tile i = rows [i h, (i + 1) h) of one view
    pi, ip, ist, itag = _in(ctx, tiles, k, fill)
    dense = ctx.upload(tiles)
    for swap in (True, False):
        got = ctx.gray_moments_u8(ip, n, h * ist, ist, h, w, 15, swap)
        same = ctx.gray_moments_u8(dense.ptr, n, h * w * 3, w * 3, h, w, 15, swap)
        g = (onp.bgr2gray_on_rgb_u8(tiles) if swap else oc.rgb2gray_u8(tiles)).astype(np.int64).reshape(n, h * w)
        want = np.stack([g.sum(1), (g * g).sum(1)], axis=1).astype(np.uint64)
        assert np.array_equal(got, want) and np.array_equal(got, same), f"sr_gray_moments_u8 swap {swap} tiles {itag}"
    _free(pi, dense)


# ---- blend --------------------------------------------------------------------------------------------------------------
def _blend_case(rng, cn, f32):
    th, tw, ov_y, ov_x = 96, 131, 30, 31
    tiles = [_scene(rng, th, tw, cn, i) for i in range(4)]
    if f32:
        tiles = [t.astype(np.float32) * np.float32(0.75) + np.float32(3.25) for t in tiles]
    rects = [((i % 2) * (tw - ov_x), (i // 2) * (th - ov_y), tw, th) for i in range(4)]
    return tiles, rects, 2 * th - ov_y, 2 * tw - ov_x                  # canvas 162 x 231: ragged cells right and bottom


def _run_blend(ctx, plan, tiles, cn, k, fill, H, W, mode="lap", rows=None):
    """One blend with every tile and the canvas as views -> (u8 canvas, fp32 canvas, tag); guards checked."""
    f32 = tiles[0].dtype != np.uint8
    ins = [_in(ctx, t, k + 1 + 5 * j, fill) for j, t in enumerate(tiles)]
    pc, cp, cst, ctag = _out(ctx, H, W * cn, _ok(k), fill)
    pf, fp, _, ftag = _out(ctx, H, W * cn * 4, k, fill, f32=True, dense=True)      # the fp32 canvas is dense by the ABI
    ptrs, strides = [i[1] for i in ins], [i[2] for i in ins]
    dt = _native.SR_F32 if f32 else _native.SR_U8
    if mode == "staged":
        plan.pyramids(ptrs, strides, [3, 0], first=True, dtype=dt)
        plan.pyramids(ptrs, strides, [1, 2], first=False, dtype=dt)
        plan.gather(ptrs, strides, cp, cst, dtype=dt, d_canvas_f32=fp)
    else:
        plan.blend(ptrs, strides, cp, cst, dtype=dt, d_canvas_f32=fp, laplacian=mode != "weighted")
    tag = f"tiles {[i[3] for i in ins]} canvas {ctag} fp32 canvas {ftag}"
    shape = (H, W, cn) if cn > 1 else (H, W)
    u8 = V.check_guard(ctx, pc, np.uint8, shape, rows=rows, what=f"blend canvas ({tag})")
    fl = V.check_guard(ctx, pf, np.float32, shape, rows=rows, what=f"blend fp32 canvas ({tag})")
    _free(pc, pf, *[i[0] for i in ins])
    return u8, fl, tag


@FILL
@pytest.mark.parametrize("march,env", MARCH_FORMS)
@pytest.mark.parametrize("cn,f32,mode", [(3, False, "lap"), (1, False, "lap"), (3, True, "lap"), (1, True, "lap"),
                                         (3, False, "staged")])
def test_blend_views(ctx, rng, cn, f32, mode, march, env, fill, monkeypatch):
    """sr_laplacian_blend / sr_blend_pyramids + sr_blend_gather through _native.BlendPlan: one plan, the tile and canvas
    layouts change from call to call; canvases bit for bit the oracle's."""
    _check_blend(ctx, rng, cn, f32, mode, march, env, fill, monkeypatch)


@FILL
@pytest.mark.parametrize("cn,f32", [(3, False), (1, False), (3, True), (1, True)])
def test_weighted_blend_views(ctx, rng, cn, f32, fill, monkeypatch):
    """sr_weighted_blend (one gather kernel whatever SR_MARCH says)."""
    _check_blend(ctx, rng, cn, f32, "weighted", "2", {}, fill, monkeypatch)


def _check_blend(ctx, rng, cn, f32, mode, march, env, fill, monkeypatch):
    monkeypatch.setenv("SR_MARCH", march)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    tiles, rects, H, W = _blend_case(rng, cn, f32)
    pos = [(r[1], r[0]) for r in rects]
    if mode == "weighted":
        ref_u8, ref_f = oc.weighted_average_fusion(tiles, pos, (H, W), "cosine", return_float=True)
    else:
        ref_u8, ref_f = oc.laplacian_fusion(tiles, pos, (H, W), 6, "cosine", return_float=True)
    plan = _native.BlendPlan(ctx, rects, cn, H, W, 6, "cosine")
    try:
        for k in (range(NL) if march == "2" and not env else range(fill & 1, NL, 2)):
            u8, fl, tag = _run_blend(ctx, plan, tiles, cn, k, fill, H, W, mode)
            assert np.array_equal(fl, ref_f), f"{mode} fp32 canvas differs from the oracle: {tag}"
            assert np.array_equal(u8, ref_u8), f"{mode} u8 canvas differs from the oracle: {tag}"
    finally:
        plan.close()


@FILL
@pytest.mark.parametrize("march,env", MARCH_FORMS)
def test_blend_row_window_views(ctx, rng, march, env, fill, monkeypatch):
    """A row-window plan writes rows [row_begin, row_end) of the canvas view and nothing else: the other rows keep the fill."""
    monkeypatch.setenv("SR_MARCH", march)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    tiles, rects, H, W = _blend_case(rng, 3, False)
    ref_u8, ref_f = oc.laplacian_fusion(tiles, [(r[1], r[0]) for r in rects], (H, W), 6, "cosine", return_float=True)
    for n_win, (a, b) in enumerate([(0, 53), (53, 118), (118, H)]):
        plan = _native.BlendPlan(ctx, rects, 3, H, W, 6, "cosine", a, b)
        try:
            for k in range(n_win, NL, 3):
                u8, fl, tag = _run_blend(ctx, plan, tiles, 3, k, fill, H, W, "lap", rows=(a, b))
                assert np.array_equal(fl[a:b], ref_f[a:b]) and np.array_equal(u8[a:b], ref_u8[a:b]), f"rows [{a}, {b}): {tag}"
        finally:
            plan.close()


def _custom_case(rng, cn, f32):
    """Four tiles of 40 x 67 at overlaps 12 / 13 on a 68 x 121 canvas, weight maps uniform in [0.1, 1) with one box where every
    covering weight is 0 and one where the four weights sum to 3e-7, below the 1e-6 floor."""
    th, tw = 40, 67
    rects = [((i % 2) * (tw - 13), (i // 2) * (th - 12), tw, th) for i in range(4)]
    tiles = [_scene(rng, th, tw, cn, i) for i in range(4)]
    if f32:
        tiles = [t.astype(np.float32) * np.float32(0.75) + np.float32(3.25) for t in tiles]
    maps = [rng.uniform(0.1, 1.0, (th, tw)).astype(np.float32) for _ in range(4)]
    for m, (x, y, _, _) in zip(maps, rects):
        m[30 - y:34 - y, 56 - x:60 - x] = 0.0                          # canvas rows 30..33, columns 56..59: under all four tiles
        m[35 - y:38 - y, 58 - x:64 - x] = np.float32(7.5e-8)
    return tiles, maps, rects, 2 * th - 12, 2 * tw - 13


@FILL
@pytest.mark.parametrize("cn,f32", [(3, False), (1, True), (4, False), (3, True)], ids=["cn3-u8", "cn1-f32", "cn4-u8", "cn3-f32"])
def test_weighted_blend_custom_views(ctx, rng, cn, f32, fill):
    """sr_weighted_blend_custom takes three kinds of (pointer, stride) pairs: tiles (LAYOUTS_U8 / LAYOUTS_F32 by their type),
    fp32 weight maps (LAYOUTS_F32: base and stride multiples of 4, what a const float * needs) and the u8 canvas (a guarded
    view); the fp32 canvas is dense by the ABI.  Both canvases bit for bit oracle_np's AND the dense call's; one plan, the
    layouts change from call to call."""
    tiles, maps, rects, H, W = _custom_case(rng, cn, f32)
    ref_u8, ref_f = onp.weighted_average_fusion(tiles, [(r[1], r[0]) for r in rects], (H, W), weights=maps, return_float=True)
    shape = (H, W, cn) if cn > 1 else (H, W)
    dt = _native.SR_F32 if f32 else _native.SR_U8
    plan = _native.BlendPlan(ctx, rects, cn, H, W, 1, "linear")
    try:
        tb, wb = [ctx.upload(t) for t in tiles], [ctx.upload(m) for m in maps]
        cu, cf = ctx.alloc(H * W * cn), ctx.alloc(H * W * cn * 4)
        plan.blend_custom_weights([b.ptr for b in tb], [_rb(t) for t in tiles], [b.ptr for b in wb], [_rb(m) for m in maps],
                                  cu.ptr, W * cn, dtype=dt, d_canvas_f32=cf.ptr)
        dense_u8, dense_f = ctx.download(cu.ptr, shape, np.uint8), ctx.download(cf.ptr, shape, np.float32)
        _free(cu, cf, *tb, *wb)
        assert np.array_equal(dense_f, ref_f) and np.array_equal(dense_u8, ref_u8), "dense call differs from the oracle"
        for k in range(NL):
            ins = [_in(ctx, t, k + 1 + 5 * j, fill) for j, t in enumerate(tiles)]
            wts = [_in(ctx, m, k + 2 + j, fill) for j, m in enumerate(maps)]
            pc, cp, cst, ctag = _out(ctx, H, W * cn, _ok(k), fill)
            pf, fp, _, ftag = _out(ctx, H, W * cn * 4, k, fill, f32=True, dense=True)
            plan.blend_custom_weights([i[1] for i in ins], [i[2] for i in ins], [i[1] for i in wts], [i[2] for i in wts],
                                      cp, cst, dtype=dt, d_canvas_f32=fp)
            tag = f"tiles {[i[3] for i in ins]} weights {[i[3] for i in wts]} canvas {ctag} fp32 canvas {ftag}"
            u8 = V.check_guard(ctx, pc, np.uint8, shape, what=f"custom blend canvas ({tag})")
            fl = V.check_guard(ctx, pf, np.float32, shape, what=f"custom blend fp32 canvas ({tag})")
            _free(pc, pf, *[i[0] for i in ins], *[i[0] for i in wts])
            assert np.array_equal(fl, ref_f), f"fp32 canvas differs from the oracle: {tag}"
            assert np.array_equal(u8, ref_u8), f"u8 canvas differs from the oracle: {tag}"
            assert np.array_equal(fl.view(np.uint32), dense_f.view(np.uint32)) and np.array_equal(u8, dense_u8), f"differs from the dense call: {tag}"
    finally:
        plan.close()


def _merge_case(rng, f32):
    """2 x 2 grid of 60 x 75 output tiles, 12 px ramps; the last tile arrives at half size and is resized."""
    th, tw, ov = 60, 75, 12
    tiles, metas, descs = [], [], []
    for i in range(4):
        r, c = divmod(i, 2)
        t = _scene(rng, th // 2 if i == 3 else th, (tw + 1) // 2 if i == 3 else tw, 3, i)
        t = t.astype(np.float32) * np.float32(0.5) + np.float32(1.25) if f32 else t
        m = dict(global_x=c * (tw - ov), global_y=r * (th - ov), output_w=tw, output_h=th, overlap_top=ov if r else 0,
                 overlap_bottom=0 if r else ov, overlap_left=ov if c else 0, overlap_right=0 if c else ov)
        tiles.append(t)
        metas.append(m)
        descs.append(dict(x=m["global_x"], y=m["global_y"], src_w=t.shape[1], src_h=t.shape[0], out_w=tw, out_h=th,
                          ov_t=m["overlap_top"], ov_b=m["overlap_bottom"], ov_l=m["overlap_left"], ov_r=m["overlap_right"]))
    return tiles, metas, descs, 2 * th - ov, 2 * tw - ov


@FILL
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_feather_merge_views(ctx, rng, f32, fill):
    tiles, metas, descs, H, W = _merge_case(rng, f32)
    want = onp.merge_tiles(tiles, metas, W, H, 1.0, True)
    for k in range(NL):
        ins = [_in(ctx, t, k + 1 + 5 * j, fill) for j, t in enumerate(tiles)]
        pc, cp, cst, ctag = _out(ctx, H, W * 3, _ok(k), fill)
        ctx.feather_merge(_native.SR_F32 if f32 else _native.SR_U8, descs, [i[1] for i in ins], [i[2] for i in ins], True,
                          cp, cst, H, W)
        what = f"sr_feather_merge_dt tiles {[i[3] for i in ins]} -> canvas {ctag}"
        got = V.check_guard(ctx, pc, np.uint8, (H, W, 3), what=what)
        assert np.array_equal(got, want), what
        _free(pc, *[i[0] for i in ins])


@FILL
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_gradient_fusion_views(ctx, rng, f32, fill):
    import _gradient_ref as gref
    th, tw, ov = 41, 53, 12
    tiles = [_scene(rng, th, tw, 3, i) for i in range(4)]
    if f32:
        tiles = [t.astype(np.float32) for t in tiles]                      # whole numbers: byte-equal with the restatement
    pos = [(r * (th - ov), c * (tw - ov)) for r in range(2) for c in range(2)]
    H, W = 2 * th - ov, 2 * tw - ov
    want = gref.gradient_domain_fusion(tiles, pos, (H, W))
    rects = [(x, y, tw, th) for (y, x) in pos]
    work = ctx.alloc(H * W * 3 * 4)
    for k in range(NL):
        ins = [_in(ctx, t, k + 1 + 5 * j, fill) for j, t in enumerate(tiles)]
        pc, cp, cst, ctag = _out(ctx, H, W * 3, _ok(k), fill)
        ctx.gradient_fusion(_native.SR_F32 if f32 else _native.SR_U8, [i[1] for i in ins], [i[2] for i in ins], rects, 3, H, W,
                            cp, cst, work.ptr)
        what = f"sr_gradient_fusion tiles {[i[3] for i in ins]} -> canvas {ctag}"
        got = V.check_guard(ctx, pc, np.uint8, (H, W, 3), what=what)
        assert np.array_equal(got, want), what
        _free(pc, *[i[0] for i in ins])
    work.free()


@FILL
def test_gradient_stats_tile_ssim_and_seam_scan_views(ctx, rng, fill):
    """Input-only entry points of the blend-quality stage: exact integer sums, so the view call equals the dense call."""
    for cn in (3, 1):
        th, tw, ov = 50, 67, 14
        tiles = [_scene(rng, th, tw, cn, i) for i in range(4)]
        rects = [((i % 2) * (tw - ov), (i // 2) * (th - ov), tw, th) for i in range(4)]
        H, W = 2 * th - ov - 5, 2 * tw - ov - 3                              # the canvas clips the last row / column of tiles
        canvas = np.ascontiguousarray(oc.laplacian_fusion(tiles, [(r[1], r[0]) for r in rects], (H + 5, W + 3), 4, "cosine")[:H, :W])
        dc, dts = ctx.upload(canvas), [ctx.upload(t) for t in tiles]
        dense_stats = ctx.gradient_stats_u8(dc.ptr, W * cn, H, W, cn)
        dense_sums = ctx.tile_ssim_sums_u8(dc.ptr, W * cn, H, W, cn, rects, [d.ptr for d in dts], [tw * cn] * 4)
        dense_seams = {w: ctx.seam_scan(dc.ptr, W * cn, H, W, cn, rects, [d.ptr for d in dts], [tw * cn] * 4, w[0], w[1], 0.999)
                       for w in ((16, 8), (12, 6))}
        assert all(len(s) > 0 for s in dense_seams.values())
        # against plain NumPy: the Sobel sum of squares (reflect-101, exact integers)
        p = np.pad(canvas.reshape(H, W, cn).astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
        gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
        gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
        assert dense_stats[0] == int((gx * gx + gy * gy).sum())
        for k in range(NL):
            pc, cp, cst, ctag = _in(ctx, canvas, k, fill)
            ins = [_in(ctx, t, _ok(k) + 5 * j, fill) for j, t in enumerate(tiles)]
            tag = f"cn {cn} canvas {ctag} tiles {[i[3] for i in ins]}"
            sq, mag = ctx.gradient_stats_u8(cp, cst, H, W, cn)
            assert sq == dense_stats[0] and mag == pytest.approx(dense_stats[1], rel=1e-12), f"sr_gradient_stats_u8 {tag}"
            sums = ctx.tile_ssim_sums_u8(cp, cst, H, W, cn, rects, [i[1] for i in ins], [i[2] for i in ins])
            assert np.array_equal(sums, dense_sums), f"sr_tile_ssim_sums_u8 {tag}"
            for (win, st), want in dense_seams.items():
                got = ctx.seam_scan(cp, cst, H, W, cn, rects, [i[1] for i in ins], [i[2] for i in ins], win, st, 0.999)
                assert [g[:3] for g in got] == [w_[:3] for w_ in want], f"sr_seam_scan {win}/{st} {tag}"
                assert all(abs(g[3] - w_[3]) <= 1e-12 for g, w_ in zip(got, want)), f"sr_seam_scan {win}/{st} {tag}"
            _free(pc, *[i[0] for i in ins])
        # the dense seam scan against the oracle (the tolerance of test_seam_scan_cell_kernel_vs_oracle)
        for (win, st), got in dense_seams.items():
            want = []
            for t, (x, y, w_, h_) in enumerate(rects):
                tile, res = tiles[t].reshape(th, tw, cn), canvas.reshape(H, W, cn)
                gt = onp.bgr2gray_on_rgb_u8(tile) if cn == 3 else tile[..., 0]
                gr = onp.bgr2gray_on_rgb_u8(res) if cn == 3 else res[..., 0]
                rh, rw = min(y + h_, H) - y, min(x + w_, W) - x
                for wy in range(0, rh - win + 1, st):
                    for wx in range(0, rw - win + 1, st):
                        s = onp.window_ssim(gt[wy:wy + win, wx:wx + win], gr[y + wy:y + wy + win, x + wx:x + wx + win])
                        if s < 0.999:
                            want.append((t, x + wx, y + wy, s))
            assert [g[:3] for g in got] == [w_[:3] for w_ in want], (cn, win, st)
            assert all(g[3] == pytest.approx(w_[3], rel=1e-9, abs=1e-12) for g, w_ in zip(got, want))
        _free(dc, *dts)


# ---- metrics ------------------------------------------------------------------------------------------------------------
@FILL
@LAYK
def test_sse_views(ctx, rng, k, fill):
    """sr_sse_u8: k_sse_flat for a dense, 16-byte aligned pair, k_sse_rows for everything else (off4-pad0 is dense but
    misaligned by 4 bytes); exact integers either way.  sr_sse_f32: fp64 sum of fp32 squares, against NumPy."""
    for (h, w) in SHAPES:
        a, b = _pair(rng, h, w)
        want = int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
        pa, ap, ast, atag = _in(ctx, a, k, fill)
        for kb in (k, _ok(k)):                                   # the same layout on both sides, then two different ones
            pb, bp, bst, btag = _in(ctx, b, kb, fill)
            assert ctx.sse_u8(ap, ast, bp, bst, h, w * 3) == want, f"sr_sse_u8 {h}x{w} a {atag} b {btag}"
            pb.free()
        pa.free()
    fa = rng.uniform(0, 255, (37, 43, 3)).astype(np.float32)
    fb = (fa + rng.normal(0, 4, fa.shape)).astype(np.float32)
    d = (fa - fb).astype(np.float32)
    want = float((d * d).astype(np.float32).astype(np.float64).sum())
    pa, ap, ast, atag = _in(ctx, fa, k, fill)
    pb, bp, bst, btag = _in(ctx, fb, k + 2, fill)
    got = ctx.sse_f32(ap, ast, bp, bst, 37, 43 * 3)
    assert got == pytest.approx(want, rel=1e-12), f"sr_sse_f32 a {atag} b {btag}"
    _free(pa, pb)


@FILL
@LAYK
def test_ssim_and_assess_views(ctx, rng, k, fill):
    h, w = SHAPES[k % len(SHAPES)]
    h, w = max(h, 23), max(w, 23)
    for cn in (3, 1):
        a, b = _pair(rng, h, w, cn)
        ga, gb = (oc.rgb2gray_u8(a), oc.rgb2gray_u8(b)) if cn == 3 else (a, b)
        pa, ap, ast, atag = _in(ctx, a, k, fill)
        pb, bp, bst, btag = _in(ctx, b, _ok(k), fill)
        da, db = ctx.upload(a), ctx.upload(b)
        tag = f"{h}x{w}x{cn} a {atag} b {btag}"
        for mode in ("uniform", "gauss", "simple"):
            s, n = ctx.ssim_u8(ap, ast, bp, bst, h, w, cn, mode)
            ref = oc.ssim(ga, gb, mode)
            assert abs(s / n - ref) <= 1e-9 * abs(ref), f"sr_ssim_u8 {mode} {tag}"
            s0, n0 = ctx.ssim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, mode)
            assert n == n0 and s == pytest.approx(s0, rel=1e-13), f"sr_ssim_u8 {mode} {tag}: view != dense"
        got = ctx.assess_u8(ap, ast, bp, bst, h, w, cn)
        same = ctx.assess_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn)
        assert got["sse"] == float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()), f"sr_assess_u8 sse {tag}"
        for key, mode in (("ssim_uniform", "uniform"), ("ssim_gauss", "gauss"), ("ssim_simple", "simple")):
            assert got[key] == pytest.approx(same[key], rel=1e-13, abs=1e-300), f"sr_assess_u8 {key} {tag}: view != dense"
            assert got[key] / _native.ssim_count(h, w, mode) == pytest.approx(oc.ssim(ga, gb, mode), rel=1e-9), f"sr_assess_u8 {key} {tag}"
        _free(pa, pb, da, db)


@FILL
@pytest.mark.parametrize("dtype,cn", [(np.float32, 3), (np.float32, 1), (np.float64, 1)], ids=["f32c3", "f32c1", "f64c1"])
def test_ssim_float_views(ctx, rng, dtype, cn, fill):
    h, w = 37, 43
    a8, b8 = _pair(rng, h, w, cn)
    a = (a8.astype(dtype) * dtype(0.9) + dtype(3.5))
    b = (b8.astype(dtype) * dtype(0.9) + dtype(2.25))
    ga, gb = (onp.rgb2gray_f32(a), onp.rgb2gray_f32(b)) if cn == 3 else (a, b)
    code = _native.SR_F32 if dtype == np.float32 else _native.SR_F64
    step = 4 if dtype == np.float32 else 8
    lays = [l for l in V.LAYOUTS_F32 if l[0] % step == 0 and l[1] % step == 0]          # element-aligned views
    da, db = ctx.upload(a), ctx.upload(b)
    for i, la in enumerate(lays):
        lb = lays[(i + 2) % len(lays)]
        pa, ap, ast = V.embed(ctx, a, la[0], la[1], fill)
        pb, bp, bst = V.embed(ctx, b, lb[0], lb[1], fill)
        for mode in ("uniform", "gauss", "simple"):
            s, n = ctx.ssim_float(ap, ast, bp, bst, h, w, cn, code, mode)
            ref = onp.ssim(ga, gb, mode)
            tag = f"sr_ssim_float {mode} a {V.layout_id(la)} b {V.layout_id(lb)}"
            assert abs(s / n - ref) <= 1e-9 * abs(ref), tag
            s0, n0 = ctx.ssim_float(da.ptr, _rb(a), db.ptr, _rb(b), h, w, cn, code, mode)
            assert n == n0 and s == pytest.approx(s0, rel=1e-13), tag + ": view != dense"
        _free(pa, pb)
    _free(da, db)


# shapes of test_assess_resized_equals_resize_then_assess: plain, gentle down-sampling (the column march), windows further
# apart than four rows, a scale near 0.1
RESIZED = [((97, 83, 3), (97, 83)), ((193, 257, 3), (19, 25)), ((128, 640), (51, 256)), ((257, 300, 3), (129, 151)),
           ((70, 200, 3), (65, 66)), ((333, 90, 3), (100, 81)), ((400, 330, 3), (80, 66)), ((391, 345, 3), (100, 90)),
           ((410, 777, 3), (50, 90))]


@FILL
@pytest.mark.parametrize("shape,dst", RESIZED)
def test_assess_resized_views(ctx, rng, shape, dst, fill):
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, shape), 0, 255).astype(np.uint8)
    (h, w), cn, (dh, dw) = shape[:2], 3 if len(shape) == 3 else 1, dst
    oa, ob = oc.resize_cubic_u8(a, dw, dh), oc.resize_cubic_u8(b, dw, dh)
    want_sse = float(np.sum((oa.astype(np.int64) - ob.astype(np.int64)) ** 2))
    g0, g1 = (oc.rgb2gray_u8(oa), oc.rgb2gray_u8(ob)) if cn == 3 else (oa, ob)
    da, db = ctx.upload(a), ctx.upload(b)
    dense = ctx.assess_resized_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, dh, dw, flags=_native.ASSESS_ALL)
    k0 = RESIZED.index((shape, dst))
    for k in range(k0 % 4, NL, 4):
        pa, ap, ast, atag = _in(ctx, a, k, fill)
        pb, bp, bst, btag = _in(ctx, b, _ok(k), fill)
        got = ctx.assess_resized_u8(ap, ast, bp, bst, h, w, cn, dh, dw, flags=_native.ASSESS_ALL)
        tag = f"sr_assess_resized_u8 {shape} -> {dst} a {atag} b {btag}"
        assert got["sse"] == want_sse, tag
        assert got["ssim_uniform"] / _native.ssim_count(dh, dw, "uniform") == pytest.approx(oc.ssim(g0, g1, "uniform"), rel=1e-9), tag
        for key in ("ssim_uniform", "ssim_gauss", "ssim_simple"):
            assert got[key] == pytest.approx(dense[key], rel=1e-13, abs=1e-300), f"{tag} {key}: view != dense"
        _free(pa, pb)
    _free(da, db)


@FILL
@LAYK
def test_rgb2gray_resize_and_histogram_views(ctx, rng, k, fill):
    h, w = SHAPES[(k + 1) % len(SHAPES)]
    a = _scene(rng, h, w, 3, k)
    pi, ip, ist, itag = _in(ctx, a, k, fill)
    hist = ctx.histogram_u8(ip, ist, h, w, 3)
    assert np.array_equal(hist, np.stack([np.bincount(a[..., c].ravel(), minlength=256) for c in range(3)])), f"sr_histogram_u8 {itag}"
    for shift in (15, 14):
        po, op, ost, otag = _out(ctx, h, w, _ok(k) + shift, fill)
        ctx.rgb2gray_u8(ip, ist, h, w, op, ost, shift)
        what = f"sr_rgb2gray_u8 shift {shift} {h}x{w} {itag} -> {otag}"
        assert np.array_equal(V.check_guard(ctx, po, np.uint8, (h, w), what=what), oc.rgb2gray_u8(a, shift)), what
        po.free()
    for j, (dh, dw) in enumerate([(h // 3 + 1, w // 2 + 2), (2 * h + 1, 2 * w - 3), (h, w)]):
        ref = oc.resize_cubic_u8(a, dw, dh)
        po, op, ost, otag = _out(ctx, dh, dw * 3, _ok(k) + j, fill)
        ctx.resize_cubic_u8(ip, ist, h, w, 3, op, ost, dh, dw)
        what = f"sr_resize_cubic_u8 {h}x{w} -> {dh}x{dw} {itag} -> {otag}"
        assert np.array_equal(V.check_guard(ctx, po, np.uint8, (dh, dw, 3), what=what), ref), what
        po.free()
        x0, y0, ww, wh = dw // 3, dh // 4, max(dw // 2, 1), max(dh // 2, 1)
        po, op, ost, otag = _out(ctx, wh, ww * 3, _ok(k) + j + 1, fill)
        ctx.resize_cubic_window_u8(ip, ist, h, w, 3, dh, dw, x0, y0, ww, wh, op, ost)
        what = f"sr_resize_cubic_window_u8 {h}x{w} -> {dh}x{dw} window {(x0, y0, ww, wh)} {itag} -> {otag}"
        assert np.array_equal(V.check_guard(ctx, po, np.uint8, (wh, ww, 3), what=what), ref[y0:y0 + wh, x0:x0 + ww]), what
        po.free()
        ref = onp.resize_linear_u8(a, dw, dh)
        po, op, ost, otag = _out(ctx, dh, dw * 3, _ok(k) + j + 2, fill)
        ctx.resize_linear_u8(ip, ist, h, w, 3, op, ost, dh, dw)
        what = f"sr_resize_linear_u8 {h}x{w} -> {dh}x{dw} {itag} -> {otag}"
        assert np.array_equal(V.check_guard(ctx, po, np.uint8, (dh, dw, 3), what=what), ref), what
        po.free()
    pi.free()


# ---- colour correction ----------------------------------------------------------------------------------------------------
# radius 8 keeps its ids; 5 and 12 are an odd radius and an even one above the 64 KiB LDS threshold of the generic kernels
# (k_cc_coeff / k_cc_apply, k_gf_box / k_gf_out), which the radius-8 cases never launch
CC_CASES = [pytest.param(0, 8, id="lut"), pytest.param(1, 8, id="guided"), pytest.param(2, 8, id="ximgproc")] + \
           [pytest.param(lf, r, id=f"{name}-r{r}") for lf, name in ((1, "guided"), (2, "ximgproc")) for r in (5, 12)]


@FILL
@pytest.mark.parametrize("local_filter,radius", CC_CASES)
def test_color_correct_views(ctx, rng, local_filter, radius, fill):
    """Out of place and in place; an integer table (the fused kernels out of place at radius 8) and a float table (branches
    0 and 1; branch 2 away from radius 8, where no kernel depends on the table's class)."""
    h, w = 46, 75
    img = _scene(rng, h, w, 3)
    src = img.astype(np.float32)
    lut_i = np.tile(np.arange(256, dtype=np.float32), (3, 1))
    lut_i[1] = np.clip(np.arange(256) * 0.5 + 40, 0, 255).astype(np.int32)
    lut_f = (np.arange(256, dtype=np.float32)[None, :] - np.float32(140.25)) * np.float32(1.5) + np.float32(100.5)
    lut_f = np.ascontiguousarray(np.repeat(lut_f, 3, 0))
    for lut in ((lut_i,) if local_filter == 2 and radius == 8 else (lut_i, lut_f)):
        corrected = np.stack([lut[c][img[..., c]] for c in range(3)], axis=-1).astype(np.float32)
        if local_filter == 0:
            want = np.clip(corrected, 0, 255).astype(np.uint8)
        else:
            f = onp.simple_guided_filter if local_filter == 1 else onp.guided_filter_ximgproc
            want = np.clip(f(corrected, src, radius, 0.01), 0, 255).astype(np.uint8)
        for k in range(NL):
            pi, ip, ist, itag = _in(ctx, img, k, fill)
            po, op, ost, otag = _out(ctx, h, w * 3, _ok(k), fill)
            ctx.color_correct_u8(ip, ist, h, w, 3, lut, local_filter, radius, 0.01, op, ost)
            what = f"sr_color_correct_u8 filter {local_filter} radius {radius} {itag} -> {otag}"
            got = V.check_guard(ctx, po, np.uint8, (h, w, 3), what=what)
            assert np.array_equal(got, want), (what, int((got != want).sum()))
            ctx.color_correct_u8(ip, ist, h, w, 3, lut, local_filter, radius, 0.01, ip, ist)
            what = f"sr_color_correct_u8 filter {local_filter} radius {radius} in place {itag}"
            got = V.check_guard(ctx, pi, np.uint8, (h, w, 3), what=what)
            assert np.array_equal(got, want), (what, int((got != want).sum()))
            _free(pi, po)


# ---- commercial / content / Poisson -----------------------------------------------------------------------------------------
@FILL
def test_commercial_saliency_entropy_views(ctx, rng, fill):
    """sr_commercial_u8 (every metric bit, two ROIs), sr_saliency_u8, sr_local_entropy_u8: fixed summation orders, so a view
    gives the bits of the dense call (which tests/test_gpu_commercial.py and test_gpu_content.py hold against the
    restatements); the entropy also against the restatement's 2e-5.  The output planes are contiguous by the ABI: their
    base offset varies."""
    import _content_ref as CR
    for (h, w, cn) in ((67, 91, 3), (50, 64, 1)):
        img = CR.synthetic(h, w, cn, seed=5)
        img = img if cn > 1 else img.reshape(h, w)
        flags = (1 << 12) - 1 if cn == 3 else (1 | 2 | 4 | 8 | 16 | 256 | 512 | 1024 | 2048)
        rois = [(3, 5, 40, 33), (w - 31, h - 20, 31, 20)]
        rflags = [1 | 16 | (32 | 64 | 128 if cn == 3 else 0)] * 2
        d = ctx.upload(img)
        ints0, flts0 = ctx.commercial_u8(d.ptr, w * cn, h, w, cn, flags, rois, rflags)
        sal0, ent0 = ctx.alloc(h * w), ctx.alloc(h * w * 4)
        ctx.saliency_u8(d.ptr, w * cn, h, w, cn, sal0.ptr)
        ctx.local_entropy_u8(d.ptr, w * cn, h, w, cn, 16, ent0.ptr)
        sal_d, ent_d = ctx.download(sal0.ptr, (h, w), np.uint8), ctx.download(ent0.ptr, (h, w), np.float32)
        assert np.abs(ent_d.astype(np.float64) - CR.local_entropy(img, 16).astype(np.float64)).max() <= 2e-5
        for k in range(NL):
            pi, ip, ist, itag = _in(ctx, img, k, fill)
            ints, flts = ctx.commercial_u8(ip, ist, h, w, cn, flags, rois, rflags)
            assert np.array_equal(ints, ints0) and np.array_equal(flts, flts0), f"sr_commercial_u8 cn {cn} {itag}: view != dense"
            ps, sp, _, stag = _out(ctx, h, w, _ok(k), fill, dense=True)
            ctx.saliency_u8(ip, ist, h, w, cn, sp)
            what = f"sr_saliency_u8 cn {cn} {itag} -> {stag}"
            assert np.array_equal(V.check_guard(ctx, ps, np.uint8, (h, w), what=what), sal_d), what
            pe, ep, _, etag = _out(ctx, h, w * 4, k, fill, f32=True, dense=True)
            ctx.local_entropy_u8(ip, ist, h, w, cn, 16, ep)
            what = f"sr_local_entropy_u8 cn {cn} {itag} -> {etag}"
            assert np.array_equal(V.check_guard(ctx, pe, np.float32, (h, w), what=what), ent_d), what
            _free(pi, ps, pe)
        _free(d, sal0, ent0)


@FILL
@LAYK
def test_rect_counts_views(ctx, rng, k, fill):
    h, w = 61, 83
    plane = (rng.integers(0, 4, (h, w)) == 0).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    rects = [(0, 0, w, h), (5, 7, 33, 19), (w - 17, h - 9, 40, 40), (11, 0, 1, h), (0, 30, w, 1), (80, 2, 3, 3)]
    pi, ip, ist, itag = _in(ctx, plane, k, fill)
    want = [int(np.count_nonzero(plane[y:min(y + rh, h), x:min(x + rw, w)])) for (x, y, rw, rh) in rects]
    assert ctx.rect_counts_u8(ip, ist, h, w, rects) == want, f"sr_rect_counts_u8 {itag}"
    pi.free()


@FILL
@pytest.mark.parametrize("h,w,mode", [(37, 43, 1), (50, 33, 2), (41, 64, 3)])
def test_poisson_clone_views(ctx, h, w, mode, fill):
    """Destination, patch, mask and output in four different layouts; the bounds of test_solver_matches_restatement."""
    import _poisson_ref as R
    dest, patch, mask = R.solver_inputs(h, w)
    want, f32 = R.clone(dest, patch, mask, mode, np.float64), R.clone(dest, patch, mask, mode, np.float32)
    allowed = max(8.0 * int(np.count_nonzero(f32 != want)), 16.0)
    for k in range(NL):
        pd, dp, dst_, dtag = _in(ctx, dest, k, fill)
        pp, pptr, pst, ptag = _in(ctx, patch, k + 3, fill)
        pm, mp, mst, mtag = _in(ctx, mask, k + 7, fill)
        po, op, ost, otag = _out(ctx, h, w * 3, _ok(k), fill)
        ctx.poisson_clone_u8(dp, dst_, pptr, pst, mp, mst, h, w, mode, op, ost)
        what = f"sr_poisson_clone_u8 {h}x{w} mode {mode} dest {dtag} patch {ptag} mask {mtag} -> {otag}"
        got = V.check_guard(ctx, po, np.uint8, (h, w, 3), what=what)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert int(diff.max()) <= 1 and int(np.count_nonzero(diff)) <= allowed, (what, int(diff.max()), int(np.count_nonzero(diff)), allowed)
        assert np.array_equal(got[0], dest[0]) and np.array_equal(got[:, -1], dest[:, -1]), what
        _free(pd, pp, pm, po)


@FILL
@pytest.mark.parametrize("h,w,cn", [(37, 43, 3), (50, 33, 1), (19, 51, 4)])
def test_blur15_and_region_ssim_views(ctx, h, w, cn, fill):
    import _poisson_ref as R
    rng = np.random.default_rng(h * w)
    img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    img = img[..., 0] if cn == 1 else img
    want = R.gaussian_blur15(img)
    other = np.clip(img.astype(int) + rng.integers(-30, 31, img.shape), 0, 255).astype(np.uint8)
    for k in range(NL):
        pi, ip, ist, itag = _in(ctx, img, k, fill)
        po, op, ost, otag = _out(ctx, h, w * cn, _ok(k), fill)
        if cn != 4:
            pb, bp, bst, btag = _in(ctx, other, k + 4, fill)
            s = ctx.region_ssim_u8(ip, ist, bp, bst, h, w, cn)
            pb.free()
            assert abs(s - R.region_ssim(img, other)) <= 1e-12, f"sr_region_ssim_u8 cn {cn} a {itag} b {btag}"
        ctx.gaussian_blur15_u8(ip, ist, h, w, cn, op, ost)
        what = f"sr_gaussian_blur15_u8 cn {cn} {itag} -> {otag}"
        assert np.array_equal(V.check_guard(ctx, po, np.uint8, img.shape, what=what), want), what
        ctx.gaussian_blur15_u8(ip, ist, h, w, cn, ip, ist)
        what = f"sr_gaussian_blur15_u8 cn {cn} in place {itag}"
        assert np.array_equal(V.check_guard(ctx, pi, np.uint8, img.shape, what=what), want), what
        _free(pi, po)


# ---- LPIPS ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alex(ctx):
    from oracle import lpips_oracle as lo
    m = _native.LpipsModel(ctx, "alex", lo.synthetic_weights("alex"))
    yield m
    m.close()


@FILL
def test_lpips_views(ctx, rng, alex, fill):
    h, w = 97, 131
    a, b = _pair(rng, h, w)
    da, db = ctx.upload(a), ctx.upload(b)
    dense = {tile: alex.layer_sums(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, tile) for tile in (0, 64)}
    assert sum(dense[0]) > 0
    for k in range(NL):
        pa, ap, ast, atag = _in(ctx, a, k, fill)
        pb, bp, bst, btag = _in(ctx, b, _ok(k), fill)
        for tile, want in dense.items():
            got = alex.layer_sums(ap, ast, bp, bst, h, w, 3, tile)
            for g, x in zip(got, want):
                assert abs(g - x) <= 1e-9 * abs(x), f"sr_lpips_u8 tile {tile} a {atag} b {btag}: {got} != {want}"
        _free(pa, pb)
    _free(da, db)


# ---- strides whose products with a row count pass 2^32 -----------------------------------------------------------------------
def _wide_case(rng, th=64):
    """Two overlapping th x 96 tiles on a th x 160 canvas: an interior of both tiles and of their overlap that the marched
    kernels take (64 rows: cell rows 2 .. 27, canvas rows 4 .. 55; 152 rows: cell rows 2 .. 69, 68 steps)."""
    tw, ov = 96, 32
    tiles = [_scene(rng, th, tw, 3, i) for i in range(2)]
    rects = [(0, 0, tw, th), (tw - ov, 0, tw, th)]
    return tiles, rects, th, 2 * tw - ov


def _march_launches(ctx, plan, bufs, strides, canvas_ptr, canvas_stride):
    """Launches of the marched gather kernels in one blend (the per-kernel timing of the context counts them)."""
    ctx.prof_select(None)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        plan.blend(bufs, strides, canvas_ptr, canvas_stride)
        ctx.sync()
        return sum(v[1] for name, v in ctx.prof_get().items() if name.startswith("gather_march"))
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


def _strided_upload(ctx, arr, stride, fill=None):
    """arr's rows at `stride` bytes in a fresh allocation, written by per-row device copies (nothing of the size of the
    allocation is staged on the host); the gaps are set to `fill` on the device when given."""
    h, rowbytes = arr.shape[0], _rb(arr)
    total = V.GUARD + (h - 1) * stride + rowbytes + V.GUARD
    assert total < 8 << 30
    buf = ctx.alloc(total)
    if fill is not None:
        ctx.memset(buf.ptr, fill, total)
    dense = ctx.upload(arr)
    for r in range(h):
        ctx.copy_d2d(buf.ptr + V.GUARD + r * stride, dense.ptr + r * rowbytes, rowbytes)
    ctx.sync()
    dense.free()
    return buf, buf.ptr + V.GUARD


@pytest.mark.parametrize("march,env", MARCH_FORMS[:2])
def test_blend_tile_stride_past_32_bits(ctx, rng, march, env, monkeypatch):
    """One tile whose row offsets pass 2^32 inside the zone the marched gather takes: 64 rows of 88 MiB + 4099 bytes (a
    5.4 GiB allocation), so rows 47 .. 63 start beyond 4 GiB and the marched cells reach canvas row 55.  A gather that formed
    (unsigned)row * (unsigned)stride would read rows 47 .. 55 of that tile from the wrong place.  The canvas must be the
    oracle's (the library takes the block gather for such a blend)."""
    monkeypatch.setenv("SR_MARCH", march)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    tiles, rects, H, W = _wide_case(rng)
    ref = oc.laplacian_fusion(tiles, [(r[1], r[0]) for r in rects], (H, W), 6, "cosine")
    stride = (88 << 20) + 4099
    assert 48 * stride >= 1 << 32                   # a row the marched cells read
    wide, wide_ptr = _strided_upload(ctx, tiles[1], stride, V.FILLS[0])
    t0, t0p, t0s = V.embed(ctx, tiles[0], 1, 3, V.FILLS[0])
    pc, cp, cst = V.out_view(ctx, H, W * 3, 3, 2, V.FILLS[1])
    plan = _native.BlendPlan(ctx, rects, 3, H, W, 6, "cosine")
    try:
        small = ctx.upload(tiles[1])
        assert _march_launches(ctx, plan, [t0p, small.ptr], [t0s, 96 * 3], cp, cst) > 0, "this geometry was meant to march"
        small.free()
        ctx.memset(pc.buf.ptr, pc.fill, pc.nbytes)
        plan.blend([t0p, wide_ptr], [t0s, stride], cp, cst)
        got = V.check_guard(ctx, pc, np.uint8, (H, W, 3), what="canvas of the blend with an 88 MiB tile stride")
        bad = np.flatnonzero((got != ref).any(axis=(1, 2)))
        assert bad.size == 0, f"canvas rows {bad.tolist()} differ from the oracle ({int((got != ref).sum())} bytes)"
    finally:
        ctx.sync()
        plan.close()
        _free(wide, t0, pc)


def test_blend_canvas_stride_past_32_bits(ctx, rng, monkeypatch):
    """A canvas on which one item of the marched gather spans more than 2^32 bytes: 152 rows of 34 MiB + 7 bytes (a 5.0 GiB
    allocation set to a fill on the device), the planner told to cut full-length items (uniform segments, a fraction of a
    round: MARCH_SEG = 64 steps = 128 canvas rows of the 68 marchable steps), so the item's last rows lie 127 strides = 4.5e9
    bytes past its first.  A gather that advanced a 32-bit offset by 2 * stride per step would write those rows 4 GiB too
    low and leave the fill in their place.  Rows and the 64 bytes on either side of each are read back one by one."""
    monkeypatch.setenv("SR_MARCH", "2")
    monkeypatch.setenv("SR_MARCH_TAIL", "0")
    monkeypatch.setenv("SR_MARCH_ROUNDS", "0.0001")
    tiles, rects, H, W = _wide_case(rng, 152)
    ref = oc.laplacian_fusion(tiles, [(r[1], r[0]) for r in rects], (H, W), 6, "cosine")
    cstride, fill, lead = (34 << 20) + 7, V.FILLS[0], 256 + 3
    assert cstride * 127 > 1 << 32
    total = lead + (H - 1) * cstride + W * 3 + V.GUARD
    assert total < 8 << 30
    canvas = ctx.alloc(total)
    ctx.memset(canvas.ptr, fill, total)
    bufs = [ctx.upload(t) for t in tiles]
    plan = _native.BlendPlan(ctx, rects, 3, H, W, 6, "cosine")
    try:
        dense = ctx.alloc(H * W * 3)
        assert _march_launches(ctx, plan, [b.ptr for b in bufs], [96 * 3] * 2, dense.ptr, W * 3) > 0, "this geometry was meant to march"
        dense.free()
        plan.blend([b.ptr for b in bufs], [t.shape[1] * 3 for t in tiles], canvas.ptr + lead, cstride)
        bad = []
        for r in range(H):
            row = ctx.download(canvas.ptr + lead + r * cstride - 64, (64 + W * 3 + 64,), np.uint8)
            assert np.all(row[:64] == fill) and np.all(row[-64:] == fill), f"bytes beside canvas row {r} were written"
            if not np.array_equal(row[64:-64].reshape(W, 3), ref[r]):
                bad.append(r)
        assert not bad, f"canvas rows {bad} differ from the oracle"
    finally:
        ctx.sync()
        plan.close()
        _free(canvas, *bufs)


def test_feather_merge_strides_past_32_bits(ctx, rng):
    """sr_feather_merge_dt with a tile and a canvas whose row * stride passes 2^32 (its kernel forms 64-bit row addresses)."""
    tiles, metas, descs, H, W = _merge_case(rng, False)
    want = onp.merge_tiles(tiles, metas, W, H, 1.0, True)
    tstride = (72 << 20) + 5                                              # 60 rows: 4.2 GiB
    cstride, fill, lead = (40 << 20) + 3, V.FILLS[1], 256 + 1             # 108 rows: 4.2 GiB
    assert tstride * tiles[0].shape[0] > 1 << 32 and cstride * H > 1 << 32
    wide, wide_ptr = _strided_upload(ctx, tiles[0], tstride)
    bufs = [ctx.upload(t) for t in tiles[1:]]
    total = lead + (H - 1) * cstride + W * 3 + V.GUARD
    assert total < 8 << 30
    canvas = ctx.alloc(total)
    ctx.memset(canvas.ptr, fill, total)
    try:
        ctx.feather_merge(_native.SR_U8, descs, [wide_ptr] + [b.ptr for b in bufs], [tstride] + [_rb(t) for t in tiles[1:]],
                          True, canvas.ptr + lead, cstride, H, W)
        for r in range(H):
            row = ctx.download(canvas.ptr + lead + r * cstride - 64, (64 + W * 3 + 64,), np.uint8)
            assert np.all(row[:64] == fill) and np.all(row[-64:] == fill), f"bytes beside canvas row {r} were written"
            assert np.array_equal(row[64:-64].reshape(W, 3), want[r]), f"canvas row {r} differs from the oracle"
    finally:
        ctx.sync()
        _free(wide, canvas, *bufs)
