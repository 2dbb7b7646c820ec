"""GPU: level-1 Gaussian planes of u8 RGB tiles kept as 16-bit integers (256 * G_1, csrc/sr_down2.inc and G1<> in
csrc/sr_engine.hip).

256 * G_1 of a u8 tile is an exact integer below 2^16 and (float)n * (1 / 256) gives back the bits of the fp32 value, so
nothing may change: every case asserts that the fp32 canvas is bit-equal to the oracle's, the u8 canvas equal, both equal to the
same call on a plan made under SR_G1_U16=0 (fp32 planes), and that sr_blend_plan_g1_format names the format that is expected
-- which is what shows that the 16-bit kernels ran."""
import numpy as np
import pytest

import _native
import _views as V
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

F32, U16 = 0, 1
LEVELS, WEIGHT = 6, "cosine"


def _blend(ctx, tiles, rects, H, W, rows=None, layouts=None, fill=0x5B, plan=None):
    """One Laplacian blend through a plan -> (u8 canvas, fp32 canvas, format the plan reports for the tiles' dtype).  Rows
    outside `rows` come back as the zeros the canvases are cleared to.  layouts: (base_off, pad) per tile -- the tiles as
    padded, offset views inside guarded parents, the canvas as well (its guard is checked)."""
    dt = _native.SR_U8 if tiles[0].dtype == np.uint8 else _native.SR_F32
    own = plan is None
    if own:
        plan = _native.BlendPlan(ctx, rects, 3, H, W, LEVELS, WEIGHT, *(rows or (0, H)))
    keep = []
    try:
        if layouts is None:
            bufs = [ctx.upload(np.ascontiguousarray(t)) for t in tiles]
            keep += bufs
            ptrs, strides = [b.ptr for b in bufs], [t.shape[1] * 3 * t.itemsize for t in tiles]
            canvas = ctx.alloc(H * W * 3)
            keep.append(canvas)
            ctx.memset(canvas.ptr, 0, H * W * 3)
            cptr, cstride, cparent = canvas.ptr, W * 3, None
        else:
            ins = [V.embed(ctx, t, lay[0], lay[1], fill) for t, lay in zip(tiles, layouts)]
            keep += [i[0] for i in ins]
            ptrs, strides = [i[1] for i in ins], [i[2] for i in ins]
            cparent, cptr, cstride = V.out_view(ctx, H, W * 3, 3, 2, fill)
            keep.append(cparent)
        canvas_f = ctx.alloc(H * W * 3 * 4)
        keep.append(canvas_f)
        ctx.memset(canvas_f.ptr, 0, H * W * 3 * 4)
        fmt = plan.g1_format(dt)
        plan.blend(ptrs, strides, cptr, cstride, dt, canvas_f.ptr)
        ctx.sync()
        if cparent is None:
            u8 = ctx.download(cptr, (H, W, 3), np.uint8)
        else:
            u8 = V.check_guard(ctx, cparent, np.uint8, (H, W, 3), rows=rows, what="canvas of a blend with 16-bit G_1")
        fl = ctx.download(canvas_f.ptr, (H, W, 3), np.float32)
    finally:
        if own:
            plan.close()
        for b in keep:
            b.free()
    return u8, fl, fmt


def _check(ctx, monkeypatch, tiles, rects, H, W, want_fmt, **kw):
    """The four properties of one case (module docstring); -> the u8 canvas."""
    pos = [(r[1], r[0]) for r in rects]
    ref_u8, ref_f = oc.laplacian_fusion(tiles, pos, (H, W), LEVELS, WEIGHT, return_float=True)
    u8, fl, fmt = _blend(ctx, tiles, rects, H, W, **kw)
    assert fmt == want_fmt, f"sr_blend_plan_g1_format says {fmt}, expected {want_fmt}"
    assert np.array_equal(fl, ref_f), float(np.nanmax(np.abs(fl - ref_f)))
    assert np.array_equal(u8, ref_u8)
    monkeypatch.setenv("SR_G1_U16", "0")                   # read when the plan is made
    u8_0, fl_0, fmt_0 = _blend(ctx, tiles, rects, H, W, **kw)
    monkeypatch.delenv("SR_G1_U16")
    assert fmt_0 == F32, "SR_G1_U16=0 must select fp32 planes"
    assert np.array_equal(fl_0, fl) and np.array_equal(u8_0, u8)
    return u8


def _grid(rng, variant=None):
    """2 x 2 tiles of 96 x 130 with 30 px of overlap and a four-tile crossing; every origin has odd x and odd y."""
    th, tw, ov = 96, 130, 30
    tiles = []
    for i in range(4):
        yy, xx = np.mgrid[0:th, 0:tw]
        base = 128 + 64 * np.sin(xx / 37.0 + i) + 48 * np.cos(yy / 23.0 + 0.5 * i)
        tiles.append(np.clip(base[..., None] + rng.integers(-12, 13, (th, tw, 3)) + 7 * i, 0, 255).astype(np.uint8))
    if variant == "all255":
        tiles[2][:] = 255                                  # 256 * G_1 = 65280 everywhere: the largest 16-bit value
    elif variant == "all0":
        tiles[1][:] = 0
    rects = [(1 + (i % 2) * (tw - ov), 1 + (i // 2) * (th - ov), tw, th) for i in range(4)]
    assert all(x % 2 == 1 and y % 2 == 1 for (x, y, _, _) in rects)
    return tiles, rects, 1 + 2 * th - ov, 1 + 2 * tw - ov


@pytest.mark.parametrize("march", ["2", "0"])
@pytest.mark.parametrize("h,w", [(33, 18), (41, 27), (99, 51), (201, 404), (67, 805)])
def test_two_disagreeing_tiles(ctx, rng, h, w, march, monkeypatch):
    """Two overlapping tiles as in test_down2_march_shapes (one half saturated, one with a zero area) through the marches and
    rectangles (SR_MARCH=2) and through the block kernel (SR_MARCH=0)."""
    monkeypatch.setenv("SR_MARCH", march)
    tiles = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
    tiles[1][: h // 2] = 255
    tiles[0][h // 2:, : w // 3] = 0
    ov = max(w // 3, 4)
    rects = [(0, 0, w, h), (w - ov, 3, w, h)]
    _check(ctx, monkeypatch, tiles, rects, h + 3, 2 * w - ov, U16)


@pytest.mark.parametrize("variant", [None, "all255", "all0"])
def test_grid_with_crossing(ctx, rng, variant, monkeypatch):
    tiles, rects, H, W = _grid(rng, variant)
    _check(ctx, monkeypatch, tiles, rects, H, W, U16)


def test_row_windows(ctx, rng, monkeypatch):
    """The grid as three strips (row_begin / row_end): the strips' rows put together are the whole-canvas plan's bytes."""
    tiles, rects, H, W = _grid(rng)
    whole = _check(ctx, monkeypatch, tiles, rects, H, W, U16)
    parts_u8, parts_f = [], []
    for a, b in [(0, 53), (53, 118), (118, H)]:
        u8, fl, fmt = _blend(ctx, tiles, rects, H, W, rows=(a, b))
        assert fmt == U16, f"rows [{a}, {b})"
        parts_u8.append(u8[a:b])
        parts_f.append(fl[a:b])
    assert np.concatenate(parts_u8).tobytes() == whole.tobytes()
    ref_f = oc.laplacian_fusion(tiles, [(r[1], r[0]) for r in rects], (H, W), LEVELS, WEIGHT, return_float=True)[1]
    assert np.array_equal(np.concatenate(parts_f), ref_f)


def test_mixed_eligibility(ctx, rng, monkeypatch):
    """One tile the fused down march refuses -- 12 wide and 40 high: no interior column group (down2_takes) -- keeps the
    whole plan on fp32 planes; the results are the oracle's."""
    tiles, rects, H, W = _grid(rng)
    tiles.append(rng.integers(0, 256, (40, 12, 3), dtype=np.uint8))
    rects.append((61, 45, 12, 40))
    _check(ctx, monkeypatch, tiles, rects, H, W, F32)


def test_plan_reuse_across_dtypes(ctx, rng):
    """One plan: u8 tiles (16-bit planes), float32 tiles of the same values (fp32 planes in the same space), u8 again."""
    tiles, rects, H, W = _grid(rng)
    ftiles = [t.astype(np.float32) for t in tiles]
    pos = [(r[1], r[0]) for r in rects]
    plan = _native.BlendPlan(ctx, rects, 3, H, W, LEVELS, WEIGHT)
    try:
        for ts, want in ((tiles, U16), (ftiles, F32), (tiles, U16)):
            ref_u8, ref_f = oc.laplacian_fusion(ts, pos, (H, W), LEVELS, WEIGHT, return_float=True)
            u8, fl, fmt = _blend(ctx, ts, rects, H, W, plan=plan)
            assert fmt == want
            assert np.array_equal(fl, ref_f) and np.array_equal(u8, ref_u8), ts[0].dtype
    finally:
        plan.close()


@pytest.mark.parametrize("fill", V.FILLS, ids=lambda f: f"fill{f:02x}")
def test_padded_offset_views(ctx, rng, fill, monkeypatch):
    """Tiles as views with a row stride above the width and a base inside a larger buffer (tests/_views.py): every base
    residue mod 4 among the four tiles; nothing outside the canvas view is written."""
    tiles, rects, H, W = _grid(rng)
    _check(ctx, monkeypatch, tiles, rects, H, W, U16, layouts=[(1, 3), (7, 13), (2, 1), (12, 64)], fill=fill)
