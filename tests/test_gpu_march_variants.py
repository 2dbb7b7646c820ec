"""GPU: every specialised loop of the marched canvas gather, at small shapes, with tiles that disagree where they overlap.

tests/test_march_variants_host.py proves on the restatement (tests/_march_ref.py) that the geometries of tests/_march_geoms.py
reach all 66 loops of k_final_march1 / k_final_marchn<2|3|4> (csrc/sr_march.inc).  Here, for each geometry:
  * the planner's work lists (sr_blend_plan_march_items) are the restatement's, item for item, and together with the
    rectangles of k_final_rect they cover every cell of the canvas exactly once;
  * the launches are the non-empty lists' (per-kernel timing records of the context), and the loop keys computed from the
    planner's own items are the ones the host test counted;
  * the fp32 canvas is bit-equal and the u8 canvas equal to the oracle's, with 8-step items, without the fp32 canvas, with
    items of 64 steps and a tapered tail, with fp32 level-1 planes and with gray tiles."""
import functools

import numpy as np
import pytest

import _march_geoms as G
import _march_ref as R
import _native
import _views as V
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

NAMES = [g.name for g in G.GEOMETRIES]


@functools.lru_cache(maxsize=None)
def _case(name, cn=3):
    """-> (geometry, tiles, oracle u8 canvas, oracle fp32 canvas): computed once, shared by the forms, never written."""
    g = G.BY_NAME[name]
    tiles = G.make_tiles(g, cn)
    ref_u8, ref_f = oc.laplacian_fusion(tiles, [(y, x) for (x, y, _, _) in g.rects], (g.H, g.W), G.LEVELS, g.weight, return_float=True)
    for a in tiles + [ref_u8, ref_f]:
        a.setflags(write=False)
    return g, tiles, ref_u8, ref_f


def _lists(plan):
    """The accessor's lists -> ({nt: [Item]}, [(x, y, w, h)])."""
    items = {nt: R.items_from_flat(plan.march_items(nt), nt) for nt in range(1, R.MAX_TILES + 1)}
    return items, [tuple(int(v) for v in r) for r in plan.march_items(0)]


def _check_plan(ctx, g, plan, long_items=False):
    """Planner against restatement, the exact partition of the canvas' cells, the promised keys -> the planner's lists."""
    items, rects = _lists(plan)
    want = G.expected_items(g, ctx.num_cu(), long_items)
    for nt in want:
        assert items[nt] == want[nt], f"{g.name}: the {nt}-tile list differs from the restatement"
    cnt = R.marched_cell_counts(items, g.H, g.W, rects)
    assert cnt.shape == (-(-g.H // 2), -(-g.W // 4))
    assert np.all(cnt == 1), f"{g.name}: cells covered {np.unique(cnt).tolist()} times, first at {np.argwhere(cnt != 1)[:4].tolist()}"
    luts = G.luts(g, _native.weight_lut)
    assert R.keys_of(items, g.rects, luts) == G.expected_keys(g, _native.weight_lut, long_items=long_items)
    return items, rects


def _blend(ctx, g, tiles, plan, with_f=True, guarded_fill=None):
    """One blend -> (u8 canvas, fp32 canvas or None, {gather launch name: launches})."""
    cn = 1 if tiles[0].ndim == 2 else 3
    bufs = [ctx.upload(t) for t in tiles]
    keep = list(bufs)
    try:
        if guarded_fill is None:
            canvas = ctx.alloc(g.H * g.W * cn)
            keep.append(canvas)
            ctx.memset(canvas.ptr, 0, g.H * g.W * cn)
            cparent, cptr, cstride = None, canvas.ptr, g.W * cn
        else:
            cparent, cptr, cstride = V.out_view(ctx, g.H, g.W * cn, 3, 5, guarded_fill)
            keep.append(cparent)
        canvas_f = None
        if with_f:
            canvas_f = ctx.alloc(g.H * g.W * cn * 4)
            keep.append(canvas_f)
            ctx.memset(canvas_f.ptr, 0xFF, g.H * g.W * cn * 4)         # NaNs: a value nobody wrote is no oracle value
        ctx.prof_select(None)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            plan.blend([b.ptr for b in bufs], [t.shape[1] * cn for t in tiles], cptr, cstride, _native.SR_U8,
                       canvas_f.ptr if with_f else None)
            ctx.sync()
            launches = {k: v[1] for k, v in ctx.prof_get().items() if k.startswith("gather_")}
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
        shape = (g.H, g.W, 3) if cn == 3 else (g.H, g.W)
        if cparent is None:
            u8 = ctx.download(cptr, shape, np.uint8)
        else:
            u8 = V.check_guard(ctx, cparent, np.uint8, shape, what=f"canvas of {g.name}")
        fl = ctx.download(canvas_f.ptr, shape, np.float32) if with_f else None
        return u8, fl, launches
    finally:
        for b in keep:
            b.free()


def _expected_launches(items):
    return {**{f"gather_march{nt}": 1 for nt, lst in items.items() if lst}, "gather_rest": 1}


def _assert_canvases(g, u8, fl, ref_u8, ref_f, what):
    if fl is not None:
        same = fl.view(np.uint32) == ref_f.view(np.uint32)
        assert same.all(), f"{g.name} {what}: {int((~same).sum())} fp32 values differ, first at {np.argwhere(~same)[:4].tolist()}"
    bad = np.argwhere(u8 != ref_u8)
    assert bad.size == 0, f"{g.name} {what}: {len(bad)} bytes differ, first at {bad[:4].tolist()}"


def _run(ctx, name, what, cn=3, with_f=True, long_items=False, want_fmt=None, guarded_fill=None):
    g, tiles, ref_u8, ref_f = _case(name, cn)
    plan = _native.BlendPlan(ctx, g.rects, cn, g.H, g.W, G.LEVELS, g.weight)
    try:
        items, rects = _check_plan(ctx, g, plan, long_items)
        assert rects, "every geometry leaves border cells to the rectangles"
        if want_fmt is not None:
            assert plan.g1_format(_native.SR_U8) == want_fmt
        u8, fl, launches = _blend(ctx, g, tiles, plan, with_f, guarded_fill)
        assert launches == _expected_launches(items), f"{g.name} {what}"
        _assert_canvases(g, u8, fl, ref_u8, ref_f, what)
        return items
    finally:
        plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_default_segments(ctx, name):
    """(a) 8-step items with the fp32 canvas, (b) the same without it (the kernels get a zero-sized resource for it)."""
    items = _run(ctx, name, "8-step items", want_fmt=1)
    assert all(it.nstep <= R.MIN_STEPS for lst in items.values() for it in lst)
    _run(ctx, name, "8-step items, no fp32 canvas", with_f=False)


@pytest.mark.parametrize("name", NAMES)
def test_long_items(ctx, name, monkeypatch):
    """(c) one round per list, tapered tail: items as long as the bands allow.  On the grids (bands of about 150 steps) the
    one- and two-tile lists hold items of MARCH_SEG steps, the taper makes the lists longer than uniform segments do, and an
    item of 64 steps takes a unit-weight loop (not under sigmoid weights, whose table never reaches 1)."""
    monkeypatch.setenv("SR_MARCH_ROUNDS", G.LONG_ROUNDS)               # read when the plan is made
    monkeypatch.delenv("SR_MARCH_TAIL", raising=False)
    items = _run(ctx, name, "long items", long_items=True)
    if name not in G.GRIDS:
        return
    g = G.BY_NAME[name]
    monkeypatch.setenv("SR_MARCH_TAIL", "0")
    plan = _native.BlendPlan(ctx, g.rects, 3, g.H, g.W, G.LEVELS, g.weight)
    try:
        uniform, _ = _lists(plan)
    finally:
        plan.close()
    assert uniform == G.expected_items(g, ctx.num_cu(), long_items=True, taper=False)
    for nt in (1, 2):
        assert any(it.nstep == R.MAX_STEPS for it in items[nt]), f"no {R.MAX_STEPS}-step item in the {nt}-tile list"
        assert len(items[nt]) > len(uniform[nt]), f"the taper did not cut the {nt}-tile list's tail"
    luts = G.luts(g, _native.weight_lut)
    long_unit = [it for it in items[1] if it.nstep == R.MAX_STEPS and R.variant_keys(it, g.rects, luts)[0][1] == "unit1"]
    if float(luts[0][-1]) == 1.0:
        assert long_unit, "no unit-weight item of 64 steps"
    else:
        assert g.weight == "sigmoid" and not long_unit


@pytest.mark.parametrize("name", G.STORAGE_SUBSET)
def test_fp32_level1_planes(ctx, name, monkeypatch):
    """(d) SR_G1_U16=0: the fp32 form of G_1 (CN = 3) through the same lists."""
    monkeypatch.setenv("SR_G1_U16", "0")
    _run(ctx, name, "fp32 G_1", want_fmt=0)


@pytest.mark.parametrize("name", G.STORAGE_SUBSET)
def test_gray_tiles(ctx, name):
    """(e) one-channel tiles of the same rectangles (CN = 1: 4-byte pixel loads and stores, fp32 G_1)."""
    _run(ctx, name, "gray", cn=1, want_fmt=0)
    _run(ctx, name, "gray, no fp32 canvas", cn=1, with_f=False)


@pytest.mark.parametrize("fill", V.FILLS, ids=lambda f: f"fill{f:02x}")
@pytest.mark.parametrize("name", G.GUARDED)
def test_guarded_prefilled_canvas(ctx, name, fill):
    """The canvas as an offset, padded view of a parent full of `fill`: a cell no item wrote shows as fill (not as the zeros
    of a cleared canvas), a byte written outside the view as a guard violation."""
    _run(ctx, name, f"guarded view, fill {fill:#x}", guarded_fill=fill)
