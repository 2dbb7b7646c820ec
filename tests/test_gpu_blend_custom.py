"""GPU: sr_weighted_blend_custom (k_weighted_custom, csrc/sr_engine.hip) bit for bit against oracle_np.weighted_average_fusion
with caller-supplied weight maps -- fp32 canvas first, then the u8 canvas.

Bit equality follows from the kernel and the oracle doing the same thing in the same order: both accumulate
acc += fl32(pixel * w) and wacc += w in ascending tile order, take max(wacc, 1e-6), do one fp32 division, clip and truncate;
the library is compiled with -ffp-contract=off.

The plans are made the way BlendingModule.weighted_average_fusion makes them (levels 1, weight type "linear"), and every call
passes d_canvas_f32.  Covered here: u8 and float32 tiles with 1, 3 and 4 channels; a regular 2 x 2 arrangement whose canvas
spans two 64-pixel blocks and is ragged in both axes; an arrangement of unequal tiles with holes, a tile sticking out of the
canvas and one pixel under all four tiles; weights that are 0 under every covering tile, weights that sum to less than the
1e-6 floor, one map a thousand times the others; row-window plans (rows outside the window untouched, NULL pointers for the
tiles a window does not reach); padded weight maps; every refusal; the module path above the entry point.
tests/test_gpu_views.py::test_weighted_blend_custom_views runs the same entry point on padded, offset, guarded views."""
import ctypes as C

import numpy as np
import pytest

import _native
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

FILL = 0x5B
# four tiles of 40 x 67 at overlaps 12 (rows) / 13 (columns): a 68 x 121 canvas
REG_RECTS = [(0, 0, 67, 40), (54, 0, 67, 40), (0, 28, 67, 40), (54, 28, 67, 40)]          # (x, y, w, h)
REG_SHAPE = (68, 121)
# unequal tiles: holes (e.g. the top right corner and the bottom left), tile 3 sticks out on the right and at the bottom
# (rows 35..84, columns 55..114 of a 70 x 110 canvas), and exactly one pixel -- (35, 55) -- lies under all four tiles
RAG_RECTS = [(0, 0, 56, 36), (50, 5, 55, 45), (10, 30, 70, 36), (55, 35, 60, 50)]
RAG_SHAPE = (70, 110)
TYPES = [(cn, f32) for cn in (1, 3, 4) for f32 in (False, True)]
TYPE_IDS = [f"cn{cn}-{'f32' if f32 else 'u8'}" for cn, f32 in TYPES]


def _cover(rects, shape):
    """Number of tiles over every canvas pixel."""
    n = np.zeros(shape, np.int32)
    for (x, y, w, h) in rects:
        n[y:y + h, x:x + w] += 1                                   # slices clip at the canvas edge
    return n


def _paint(maps, rects, box, value):
    """Sets the weight of EVERY tile over the canvas box (y0, y1, x0, x1) to `value`."""
    y0, y1, x0, x1 = box
    for m, (x, y, w, h) in zip(maps, rects):
        a, b, c, d = max(y0 - y, 0), min(y1 - y, h), max(x0 - x, 0), min(x1 - x, w)
        if a < b and c < d:
            m[a:b, c:d] = value


def _tiles(rng, rects, cn, kind):
    out = []
    for i, (_, _, w, h) in enumerate(rects):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 64 * np.sin(xx / 17.0 + i) + 48 * np.cos(yy / 11.0 + 0.5 * i)
        t = np.clip(base[..., None] + rng.integers(-12, 13, (h, w, cn)) + 7 * i, 0, 255).astype(np.uint8)
        t = t if cn > 1 else t[..., 0]
        if kind == "f32":                                          # the suite's usual float form
            t = t.astype(np.float32) * np.float32(0.75) + np.float32(3.25)
        elif kind == "wide":                                       # -100 .. 410: the clip works on both sides
            t = t.astype(np.float32) * np.float32(2.0) - np.float32(100.0)
        out.append(np.ascontiguousarray(t))
    return out


def _maps(rng, rects, shape, zero_box, floor_box, floor_each):
    """uniform [0.1, 1); map 1 times 1000; then, in zero_box, every covering weight 0 (the floor gives 0 / 1e-6 = 0) and, in
    floor_box, every covering weight floor_each (their sum stays below the 1e-6 floor: the result is acc / 1e-6)."""
    maps = [rng.uniform(0.1, 1.0, (h, w)).astype(np.float32) for (_, _, w, h) in rects]
    maps[1] *= np.float32(1e3)
    _paint(maps, rects, zero_box, np.float32(0.0))
    _paint(maps, rects, floor_box, np.float32(floor_each))
    cover = _cover(rects, shape)
    for box in (zero_box, floor_box):
        assert cover[box[0]:box[1], box[2]:box[3]].min() >= 2, "the special weights belong into an overlap"
    return maps


def _case(rng, name, cn, kind):
    """-> tiles, rects, positions, canvas shape, weight maps."""
    if name == "regular":
        rects, shape = REG_RECTS, REG_SHAPE
        # both boxes inside the 12 x 13 rectangle all four tiles share (rows 28..39, columns 54..66): 4 x 7.5e-8 = 3e-7
        maps = _maps(rng, rects, shape, (30, 34, 56, 60), (35, 38, 58, 64), 7.5e-8)
    else:
        rects, shape = RAG_RECTS, RAG_SHAPE
        # rows 40..49, columns 85..104 lie under tiles 1 and 3 only: 2 x 1.5e-7 = 3e-7
        assert np.all(_cover(rects, shape)[40:48, 85:95] == 2)
        maps = _maps(rng, rects, shape, (40, 45, 85, 95), (45, 48, 85, 95), 1.5e-7)
    tiles = _tiles(rng, rects, cn, kind)
    pos = [(y, x) for (x, y, _, _) in rects]
    return tiles, rects, pos, shape, maps


def _reference(tiles, pos, shape, maps):
    u8, fl = onp.weighted_average_fusion(tiles, pos, shape, weights=maps, return_float=True)
    assert np.all(np.isfinite(fl))
    return u8, fl


class _Dev:
    """Tiles and weight maps in HBM (dense, or weight rows padded by `wpad` bytes) and two canvases full of the fill byte."""

    def __init__(self, ctx, tiles, maps, shape, cn, wpad=0):
        self.ctx, self.shape, self.cn = ctx, shape, cn
        self.cshape = shape if cn == 1 else shape + (cn,)
        self.f32 = tiles[0].dtype != np.uint8
        self.dtype = _native.SR_F32 if self.f32 else _native.SR_U8
        self.tb = [ctx.upload(t) for t in tiles]
        self.tstrides = [t.nbytes // t.shape[0] for t in tiles]
        padded = [np.concatenate([m, np.full((m.shape[0], wpad // 4), 7.0, np.float32)], axis=1) if wpad else m for m in maps]
        self.wb = [ctx.upload(m) for m in padded]
        self.wstrides = [m.shape[1] * 4 for m in padded]
        self.nb = shape[0] * shape[1] * cn
        self.canvas, self.canvas_f = ctx.alloc(self.nb), ctx.alloc(self.nb * 4)
        self.refill()

    def refill(self):
        self.ctx.memset(self.canvas.ptr, FILL, self.nb)
        self.ctx.memset(self.canvas_f.ptr, FILL, self.nb * 4)

    def run(self, plan, tile_ptrs=None, weight_ptrs=None, **kw):
        args = dict(d_tiles=tile_ptrs or [b.ptr for b in self.tb], strides=self.tstrides,
                    d_weights=weight_ptrs or [b.ptr for b in self.wb], weight_strides=self.wstrides,
                    d_canvas=self.canvas.ptr, canvas_stride=self.shape[1] * self.cn, dtype=self.dtype,
                    d_canvas_f32=self.canvas_f.ptr)
        args.update(kw)
        plan.blend_custom_weights(**args)

    def canvases(self):
        """-> (u8 canvas, fp32 canvas as its bytes' uint32 -- a fill pattern is a NaN as a float)."""
        self.ctx.sync()
        return (self.ctx.download(self.canvas.ptr, self.cshape, np.uint8),
                self.ctx.download(self.canvas_f.ptr, self.cshape, np.uint32))

    def untouched(self):
        u8, fl = self.canvases()
        return bool(np.all(u8 == FILL) and np.all(fl == FILL * 0x01010101))

    def free(self):
        for b in self.tb + self.wb + [self.canvas, self.canvas_f]:
            b.free()


def _plan(ctx, rects, cn, shape, rows=None):
    a, b = rows or (0, shape[0])
    return _native.BlendPlan(ctx, rects, cn, shape[0], shape[1], 1, "linear", a, b)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("cn,f32", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["regular", "ragged"])
def test_matches_oracle(ctx, rng, name, cn, f32):
    """Whole canvas, dense buffers, then the same call with weight rows padded by 20 bytes (the map's own stride counts)."""
    tiles, rects, pos, shape, maps = _case(rng, name, cn, "f32" if f32 else "u8")
    ref_u8, ref_f = _reference(tiles, pos, shape, maps)
    cover = _cover(rects, shape)
    assert (cover == 0).any() == (name == "ragged") and cover.max() == 4
    if name == "ragged":
        assert (cover == 4).sum() == 1 and cover[35, 55] == 4       # one pixel under all four tiles
        assert np.all(ref_f[cover == 0] == 0) and np.all(ref_u8[cover == 0] == 0)
    plan = _plan(ctx, rects, cn, shape)
    try:
        for wpad in (0, 20):
            dev = _Dev(ctx, tiles, maps, shape, cn, wpad)
            try:
                dev.run(plan)
                u8, fl = dev.canvases()
            finally:
                dev.free()
            assert np.array_equal(fl, _bits(ref_f).reshape(fl.shape)), (name, cn, f32, wpad, "fp32 canvas")
            assert np.array_equal(u8, ref_u8), (name, cn, f32, wpad, "u8 canvas")
            if name == "ragged":                                    # a hole is exactly 0 in both canvases
                assert np.all(u8[cover == 0] == 0) and np.all(fl[cover == 0] == 0)
    finally:
        plan.close()


def test_special_weights_do_what_they_claim(rng):
    """The reference on the regular case: the all-zero box gives exactly 0, the box below the floor acc / 1e-6 (not the
    weighted mean), and the floor is what decides it -- so a kernel with another floor cannot pass test_matches_oracle."""
    tiles, rects, pos, shape, maps = _case(rng, "regular", 3, "u8")
    _, fl = _reference(tiles, pos, shape, maps)
    assert np.all(fl[30:34, 56:60] == 0)
    acc = np.zeros((3, 6, 3), np.float32)
    wsum = np.zeros((3, 6), np.float32)
    for t, m, (x, y, w, h) in zip(tiles, maps, rects):
        acc += t[35 - y:38 - y, 58 - x:64 - x].astype(np.float32) * m[35 - y:38 - y, 58 - x:64 - x, None]
        wsum += m[35 - y:38 - y, 58 - x:64 - x]
    assert np.all(wsum > 0) and np.all(wsum < np.float32(1e-6))
    assert np.array_equal(fl[35:38, 58:64], acc / np.float32(1e-6))
    assert not np.array_equal(fl[35:38, 58:64], acc / np.maximum(wsum, np.float32(1e-5))[..., None])
    assert np.all(fl[35:38, 58:64] < 255) and np.all(fl[35:38, 58:64] > 0)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_values_outside_0_255_are_clipped(ctx, rng, cn):
    tiles, rects, pos, shape, maps = _case(rng, "regular", cn, "wide")
    ref_u8, ref_f = _reference(tiles, pos, shape, maps)
    assert ref_f.min() < -10 and ref_f.max() > 265 and (ref_u8 == 0).any() and (ref_u8 == 255).any()
    plan, dev = _plan(ctx, rects, cn, shape), _Dev(ctx, tiles, maps, shape, cn)
    try:
        dev.run(plan)
        u8, fl = dev.canvases()
    finally:
        plan.close()
        dev.free()
    assert np.array_equal(fl, _bits(ref_f).reshape(fl.shape)) and np.array_equal(u8, ref_u8)


@pytest.mark.parametrize("cn,f32", [(3, False), (1, True), (4, False), (3, True)], ids=["cn3-u8", "cn1-f32", "cn4-u8", "cn3-f32"])
@pytest.mark.parametrize("name", ["regular", "ragged"])
def test_row_windows(ctx, rng, name, cn, f32):
    """Plans over rows [0, 17), [17, 50), [50, H): each changes exactly its own rows of a canvas full of the fill byte, and
    the three strips together are the full-canvas result, bit for bit in both canvases.  A tile the window does not reach
    (plan.tile_rows(t) empty) is passed as a NULL tile pointer AND a NULL weight pointer -- include/sr_hip.h allows both;
    a NULL weight pointer for a tile that has rows is refused."""
    tiles, rects, pos, shape, maps = _case(rng, name, cn, "f32" if f32 else "u8")
    ref_u8, ref_f = _reference(tiles, pos, shape, maps)
    H = shape[0]
    dev = _Dev(ctx, tiles, maps, shape, cn)
    got_u8 = np.empty_like(ref_u8)
    got_f = np.empty(ref_f.shape, np.uint32)
    rowless_seen = 0
    try:
        for (a, b) in [(0, 17), (17, 50), (50, H)]:
            plan = _plan(ctx, rects, cn, shape, (a, b))
            try:
                has_rows = []
                for t, (x, y, w, h) in enumerate(rects):
                    r0, r1 = plan.tile_rows(t)
                    assert (r0 < r1) == (max(a, y) < min(b, y + h)), (t, a, b, r0, r1)
                    has_rows.append(r0 < r1)
                rowless_seen += has_rows.count(False)
                dev.refill()
                dev.run(plan, tile_ptrs=[p.ptr if ok else None for p, ok in zip(dev.tb, has_rows)],
                        weight_ptrs=[p.ptr if ok else None for p, ok in zip(dev.wb, has_rows)])
                u8, fl = dev.canvases()
                assert np.all(u8[:a] == FILL) and np.all(u8[b:] == FILL), f"rows outside [{a}, {b}) of the u8 canvas were written"
                assert np.all(fl[:a] == FILL * 0x01010101) and np.all(fl[b:] == FILL * 0x01010101), \
                    f"rows outside [{a}, {b}) of the fp32 canvas were written"
                got_u8[a:b], got_f[a:b] = u8[a:b], fl[a:b]
                t_live = has_rows.index(True)
                wp = [p.ptr for p in dev.wb]
                wp[t_live] = None
                dev.refill()
                with pytest.raises(ValueError):
                    dev.run(plan, weight_ptrs=wp)
                assert dev.untouched()
            finally:
                plan.close()
    finally:
        dev.free()
    assert rowless_seen >= 2, "the windows were meant to leave tiles without rows"
    assert np.array_equal(got_f, _bits(ref_f).reshape(got_f.shape)), "the strips' fp32 rows differ from the full canvas"
    assert np.array_equal(got_u8, ref_u8), "the strips' u8 rows differ from the full canvas"


def test_refusals_leave_the_canvas_untouched(ctx, rng):
    """No kernel runs in any of these: the binding's matching error, and both canvases keep the fill byte."""
    cn = 3
    tiles, rects, pos, shape, maps = _case(rng, "regular", cn, "u8")
    H, W = shape
    plan, dev = _plan(ctx, rects, cn, shape), _Dev(ctx, tiles, maps, shape, cn)
    try:
        wp = [b.ptr for b in dev.wb]
        with pytest.raises(ValueError, match="null"):                                       # a NULL map for a tile with rows
            dev.run(plan, weight_ptrs=[wp[0], None, wp[2], wp[3]])
        assert dev.untouched()
        with pytest.raises(_native.SrShapeError, match="weight map 2 stride"):              # a weight stride of w * 4 - 4
            dev.run(plan, weight_strides=[67 * 4, 67 * 4, 67 * 4 - 4, 67 * 4])
        assert dev.untouched()
        with pytest.raises(_native.SrShapeError, match="canvas stride"):                    # a canvas stride of W * cn - 1
            dev.run(plan, canvas_stride=W * cn - 1)
        assert dev.untouched()
        with pytest.raises(ValueError, match="dtype") as ei:                                # neither SR_U8 nor SR_F32
            dev.run(plan, dtype=_native.SR_F64)
        assert not isinstance(ei.value, _native.SrShapeError) and dev.untouched()
        # a NULL weight array: the binding always builds one, so this goes to the C ABI itself
        n = len(rects)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(b.ptr) for b in dev.tb])
        st = (C.c_int64 * n)(*dev.tstrides)
        ws = (C.c_int64 * n)(*dev.wstrides)
        with pytest.raises(ValueError, match="null"):
            _native.check(ctx.lib.sr_weighted_blend_custom(plan.handle, _native.SR_U8, ptrs, st, None, ws, C.c_void_p(dev.canvas.ptr),
                                                           W * cn, C.c_void_p(dev.canvas_f.ptr)))
        assert dev.untouched()
        wpa = (C.c_void_p * n)(*[C.c_void_p(p) for p in wp])
        with pytest.raises(ValueError, match="null"):                                       # ... and a NULL stride array
            _native.check(ctx.lib.sr_weighted_blend_custom(plan.handle, _native.SR_U8, ptrs, st, wpa, None, C.c_void_p(dev.canvas.ptr),
                                                           W * cn, C.c_void_p(dev.canvas_f.ptr)))
        assert dev.untouched()
        # a destroyed plan: the library keeps a registry of live plans, so the stale handle is recognised, not followed
        stale = C.c_void_p(plan.handle.value)
        plan.close()
        plan.handle = stale
        try:
            with pytest.raises(ValueError, match="destroyed plan"):
                dev.run(plan)
        finally:
            plan.handle = None
        assert dev.untouched()
    finally:
        plan.close()
        dev.free()


# ---- the module path above the entry point ------------------------------------------------------------------------------
def _module_case(rng, cn, kind):
    import blending_module as bm
    tiles, rects, pos, shape, maps = _case(rng, "regular", cn, kind)
    infos = [bm.TileInfo(t, x, y, i // 2, i % 2) for i, (t, (x, y, _, _)) in enumerate(zip(tiles, rects))]
    return bm, tiles, infos, pos, shape, maps


@pytest.mark.parametrize("cn,kind", [(1, "u8"), (3, "f32")], ids=["gray-u8", "rgb-f32"])
def test_module_weighted_average_fusion_with_weights(rng, cn, kind):
    """BlendingModule.weighted_average_fusion(infos, weights=...) with gray u8 tiles and float32 RGB tiles: len(weights) of 0
    (generated maps for every tile), 1 and n; the remaining tiles' maps come from oracle_np.distance_weight_map."""
    bm, tiles, infos, pos, shape, maps = _module_case(rng, cn, kind)
    b = bm.BlendingModule()
    gen = [onp.distance_weight_map(t.shape[0], t.shape[1], "cosine") for t in tiles]
    for k in (0, 1, len(tiles)):
        full = maps[:k] + gen[k:]
        got = b.weighted_average_fusion(infos, weights=maps[:k], weight_type=bm.WeightType.COSINE)
        want = onp.weighted_average_fusion(tiles, pos, shape, "cosine", weights=full)
        assert got.dtype == np.uint8 and got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want), (cn, kind, k, int((got != want).sum()))
    # a map given as (h, w, 1)
    got = b.weighted_average_fusion(infos, weights=[m[..., None] for m in maps], weight_type=bm.WeightType.COSINE)
    assert np.array_equal(got, onp.weighted_average_fusion(tiles, pos, shape, "cosine", weights=maps))
    # a map of the wrong shape
    with pytest.raises(ValueError, match="weight map 1"):
        b.weighted_average_fusion(infos, weights=[maps[0], maps[1][:-1]])
    with pytest.raises(ValueError, match="weight map 0"):
        b.weighted_average_fusion(infos, weights=[maps[0].T.copy()])
