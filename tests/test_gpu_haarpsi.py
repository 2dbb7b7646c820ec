"""GPU: HaarPSI, the Haar wavelet perceptual similarity index (sr_haarpsi_u8, sr_haarpsi_cells_u8, csrc/sr_haarpsi.hip).

* restatement: every per-channel num and den and the value against tests/_haarpsi_ref.py (the scripts' float form on
  scipy.signal.convolve2d) at 1e-9 relative, counts equal -- at the smallest sizes (2 x 2 up), around the kernel's tile
  (16 x 64 samples: 15 / 16 / 17 sample rows and 63 / 64 / 65 sample columns from odd and even input sides, with and without
  subsampling), one image of at least 3 x 3 blocks, and cn x crop border x convention x subsample on one odd shape;
* properties: identity and a flat pair give 1 within 1e-12, symmetry, a black pair is NaN, saturated pairs, a
  complementary-colour pair (red against cyan: the chroma coefficients are magnitudes, so sim(c_I) stays 1) and a red against
  gray pair that drives sim(c_I) far from 1, equal bits for equal inputs;
* cells: against the restatement's per-sample maps at 1e-9, adding up to the global record at 1e-9, with odd edges that fall
  inside a block, through the module methods and their device twins;
* memory: padded, offset, guarded views give the dense bits and nothing outside is written; rows that start beyond 2^32
  bytes, and a row stride that itself is beyond 2^32 bytes, for the sums and the cells;
* the pipeline: the hook at its smallest canvas, whole runs of the device-resident and the host-array path, and main.py
  --qa-haarpsi as two ranks against one (the sharded path and the command line).
parity: the 'python' convention is SciPy's own convolve2d(mode='same'); 'matlab' is unpinned (MATLAB, piq, pyiqa are not
available offline).  Largest relative distance from the restatement seen on an MI355X: see README.md."""
import functools
import math

import numpy as np
import pytest

import _haarpsi_ref as H
import _views as V

pytestmark = pytest.mark.gpu

TOL = 1e-9
CONVENTIONS = ("matlab", "python")


@functools.lru_cache(maxsize=None)
def _case(h, w, cn=3):
    """One image pair per shape, made once and shared (never modified): a smooth ramp with texture, and a noisy copy."""
    rng = np.random.default_rng(1000 * h + w + cn)
    y, x = np.mgrid[0:h, 0:w]
    base = (96 + 60 * np.sin(x / 5.0) * np.cos(y / 7.0))[..., None] + 40 * np.arange(cn)[None, None, :] / max(cn - 1, 1)
    a = np.clip(base + rng.normal(0, 25, (h, w, cn)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float64) + rng.normal(0, 12, a.shape) + 6 * np.sin(x / 3.0)[..., None], 0, 255).astype(np.uint8)
    if cn == 1:
        a, b = a[..., 0], b[..., 0]
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, cb, sub, conv):
    a, b = _case(h, w, cn)
    return H.haarpsi_ref(a, b, cb, sub, conv)


def _run(ctx, a, b, cb=0, sub=True, conv="matlab"):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.haarpsi(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, crop_border=cb, subsample=sub, convention=conv)
    finally:
        da.free(); db.free()


def _bits(rec):
    return (tuple(np.asarray(rec["num"], np.float64).view(np.uint64)), tuple(np.asarray(rec["den"], np.float64).view(np.uint64)),
            rec["channels"], rec["count"])


def _check(got, want, what):
    import _native
    value = _native.haarpsi_value(got)
    assert got["channels"] == want["channels"] == len(got["num"]) == len(got["den"]), what
    assert got["count"] == want["map_den"].size, what
    worst = 0.0
    for c in range(want["channels"]):
        for k in ("num", "den"):
            g, r = float(got[k][c]), float(want[k][c])
            assert r > 0, (what, k, c)
            worst = max(worst, abs(g - r) / r)
    worst = max(worst, abs(value - want["value"]) / want["value"])
    print(f"{what}: value {value!r} ref {want['value']!r} largest rel {worst:.2e}")
    for c in range(want["channels"]):
        assert got["num"][c] == pytest.approx(want["num"][c], rel=TOL, abs=0), (what, "num", c)
        assert got["den"][c] == pytest.approx(want["den"][c], rel=TOL, abs=0), (what, "den", c)
    assert value == pytest.approx(want["value"], rel=TOL, abs=0), what


SHAPES = [(2, 2), (2, 3), (3, 5), (7, 8), (16, 16), (17, 33), (33, 18), (65, 127)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_small_shapes_match_the_restatement(ctx, h, w):
    for cn in (3, 1):
        for conv in CONVENTIONS:
            for sub in (True, False):
                a, b = _case(h, w, cn)
                _check(_run(ctx, a, b, 0, sub, conv), _ref(h, w, cn, 0, sub, conv), f"{h}x{w} cn {cn} {conv} sub {sub}")


def test_anchors(ctx):
    """The cross-check input of the definition, both conventions, with and without subsampling, colour and gray."""
    a, b = H.anchor_pair()
    for (colour, conv, sub), want in H.ANCHORS.items():
        x, y = (a, b) if colour else (np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(b[..., 0]))
        import _native
        v = _native.haarpsi_value(_run(ctx, x, y, 0, sub, conv))
        print(colour, conv, sub, v, want, abs(v - want) / want)
        assert v == pytest.approx(want, rel=TOL, abs=0), (colour, conv, sub)
    rec = _run(ctx, a, b)
    assert rec["num"] == pytest.approx(H.ANCHOR_NUM, rel=TOL, abs=0) and rec["den"] == pytest.approx(H.ANCHOR_DEN, rel=TOL, abs=0)


# 15 / 16 / 17 sample rows and 63 / 64 / 65 sample columns: one tile less one, one tile, one tile and a sliver
TILE_SUB = [(29, 125), (30, 126), (31, 127), (32, 128), (33, 129), (34, 130)]
TILE_FULL = [(15, 63), (16, 64), (17, 65), (16, 65), (17, 64)]


@pytest.mark.parametrize("h,w", TILE_SUB, ids=[f"{h}x{w}" for h, w in TILE_SUB])
def test_around_the_tile_subsampled(ctx, h, w):
    import _native
    assert [_native.haarpsi_plan(s, s, 3)["size"][0] for s in (29, 30, 31, 32, 33, 34, 125, 126, 127, 128, 129, 130)] == \
        [15, 15, 16, 16, 17, 17, 63, 63, 64, 64, 65, 65]
    assert _native.haarpsi_plan(h, w, 3)["blocks"] == -(-((h + 1) // 2) // 16) * -(-((w + 1) // 2) // 64)
    for conv in CONVENTIONS:
        a, b = _case(h, w, 3)
        _check(_run(ctx, a, b, 0, True, conv), _ref(h, w, 3, 0, True, conv), f"{h}x{w} {conv}")


@pytest.mark.parametrize("h,w", TILE_FULL, ids=[f"{h}x{w}" for h, w in TILE_FULL])
def test_around_the_tile_not_subsampled(ctx, h, w):
    import _native
    assert _native.haarpsi_plan(h, w, 1, 0, False)["blocks"] == -(-h // 16) * -(-w // 64)
    for conv in CONVENTIONS:
        for cn in (3, 1):
            a, b = _case(h, w, cn)
            _check(_run(ctx, a, b, 0, False, conv), _ref(h, w, cn, 0, False, conv), f"{h}x{w} cn {cn} {conv} full")


def test_multi_block(ctx):
    """67 x 263: 34 x 132 samples in 3 x 3 blocks when subsampled, 5 x 5 blocks otherwise; the last of either axis partial."""
    import _native
    h, w = 67, 263
    assert _native.haarpsi_plan(h, w, 3)["blocks"] == 9 and _native.haarpsi_plan(h, w, 3, 0, False)["blocks"] == 25
    for conv in CONVENTIONS:
        for sub in (True, False):
            a, b = _case(h, w, 3)
            _check(_run(ctx, a, b, 0, sub, conv), _ref(h, w, 3, 0, sub, conv), f"{h}x{w} {conv} sub {sub}")


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_channels_crops_conventions_and_subsampling(ctx, cn):
    """37 x 43, odd sides: the crop changes the parity of both sides and the residue of the first byte."""
    h, w = 37, 43
    a, b = _case(h, w, cn)
    seen = set()
    for cb in (0, 1, 2, 3):
        for conv in CONVENTIONS:
            for sub in (True, False):
                got = _run(ctx, a, b, cb, sub, conv)
                want = _ref(h, w, cn, cb, sub, conv)
                _check(got, want, f"cn {cn} cb {cb} {conv} sub {sub}")
                seen.add(want["value"])
                if cb:
                    ac = np.ascontiguousarray(a[cb:h - cb, cb:w - cb])
                    bc = np.ascontiguousarray(b[cb:h - cb, cb:w - cb])
                    assert _bits(_run(ctx, ac, bc, 0, sub, conv)) == _bits(got), (cn, cb, conv, sub)
    assert len(seen) == 16                                                  # every switch is told apart
    if cn == 4:                                                             # alpha is ignored
        a2 = a.copy(); a2[..., 3] = 255 - a2[..., 3]
        assert _bits(_run(ctx, a2, b)) == _bits(_run(ctx, a, b)) == _bits(_run(ctx, np.ascontiguousarray(a[..., :3]),
                                                                                np.ascontiguousarray(b[..., :3])))


def test_properties(ctx):
    import _native
    val = _native.haarpsi_value
    for h, w, cn in ((2, 2, 3), (17, 33, 3), (33, 18, 1), (67, 263, 3)):
        a, b = _case(h, w, cn)
        for conv in CONVENTIONS:
            for sub in (True, False):
                kw = dict(sub=sub, conv=conv)
                same = val(_run(ctx, a, a, **kw))
                assert abs(same - 1.0) <= 1e-12, (h, w, cn, kw, same)
                ab, ba = _run(ctx, a, b, **kw), _run(ctx, b, a, **kw)
                assert abs(val(ab) - val(ba)) <= 1e-12 * val(ab), (h, w, cn, kw)
                assert np.allclose(ab["num"], ba["num"], rtol=1e-12, atol=0) and np.allclose(ab["den"], ba["den"], rtol=1e-12, atol=0)
                assert 0.0 < val(ab) < 1.0
                # a black pair: every weight is 0
                z = np.zeros_like(a)
                rec = _run(ctx, z, z, **kw)
                assert all(d == 0.0 for d in rec["den"]) and math.isnan(val(rec)), (h, w, cn, kw)
                # a flat pair: the zero border gives the rim a weight, every similarity is 1
                f = np.full_like(a, 77)
                rec = _run(ctx, f, f, **kw)
                assert all(d > 0.0 for d in rec["den"][:2]) and abs(val(rec) - 1.0) <= 1e-12, (h, w, cn, kw, val(rec))


def test_saturated_and_complementary_pairs(ctx):
    h, w = 33, 47
    rng = np.random.default_rng(5)
    # saturated: white against white with a few dark pixels, and the largest step there is (0 against 255 checkers)
    white = np.full((h, w, 3), 255, np.uint8)
    speck = white.copy()
    speck[rng.integers(0, h, 40), rng.integers(0, w, 40)] = 0
    chk = (((np.add.outer(np.arange(h), np.arange(w)) // 4) % 2) * 255).astype(np.uint8)
    chk = np.ascontiguousarray(np.repeat(chk[..., None], 3, 2))
    # complementary colours, red against cyan: I = 0.596 * 255 against -0.596 * 255 and the coefficient is a magnitude, so
    # sim(c_I) = sim(c_Q) = 1 and the chroma channel cannot tell them apart (the luma channels do).  Red against a gray of
    # about its luma is the pair that drives sim(c_I) far from 1.
    red = np.zeros((h, w, 3), np.uint8); red[..., 0] = 255
    cyan = 255 - red
    gray = np.full((h, w, 3), 76, np.uint8)
    for x, y, what in ((white, speck, "white / specks"), (chk, 255 - chk, "checkers"), (red, cyan, "red / cyan"),
                       (red, gray, "red / gray")):
        for conv in CONVENTIONS:
            for sub in (True, False):
                want = H.haarpsi_ref(x, y, 0, sub, conv)
                _check(_run(ctx, x, y, 0, sub, conv), want, f"{what} {conv} sub {sub}")
                if what == "red / cyan":                                    # LS_c = 1 everywhere: the channel sits at sigmoid(4.2)
                    assert want["num"][2] / want["den"][2] == pytest.approx(1.0 / (1.0 + math.exp(-4.2)), rel=1e-12, abs=0)
                if what == "red / gray":
                    # the pair is made for this: sim(c_I) = 30 / (152^2 + 30) = 0.001 and sim(c_Q) = 0.01 inside, so the chroma
                    # channel sits at sigmoid(4.2 * 0.006) = 0.51; in the rim's corners, where a quarter of the window is left,
                    # at sigmoid(4.2 * 0.08) = 0.58 -- against sigmoid(4.2) = 0.985 of the luma channels
                    ratio = want["num"][2] / want["den"][2]
                    assert 0.5 < ratio < 0.6 and want["num"][0] / want["den"][0] > 0.9, ratio


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    import _native
    h, w = 37, 43
    a, b = _case(h, w, 3)
    big_a, big_b = _case(67, 263, 3)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for sub in (True, False):
            first = ctx.haarpsi(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, sub)
            second = ctx.haarpsi(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, sub)
            ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
            assert _native.haarpsi_plan(67, 263, 3, 0, sub)["scratch_bytes"] >= _native.haarpsi_plan(h, w, 3, 2, sub)["scratch_bytes"]
            big = _run(ctx, big_a, big_b, 0, sub)                           # a larger shape through the scratch
            cells = ctx.haarpsi_cells(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, [0, 20, w], [0, h], subsample=sub)
            third = ctx.haarpsi(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, sub)
            assert _bits(first) == _bits(second) == _bits(third), sub
            assert _bits(big) == _bits(_run(ctx, big_a, big_b, 0, sub)), sub
            again = ctx.haarpsi_cells(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, [0, 20, w], [0, h], subsample=sub)
            assert all(np.array_equal(cells[k].view(np.uint64), again[k].view(np.uint64)) for k in ("num", "den"))
    finally:
        da.free(); db.free()


def _cells_ref(want, xe, ye, sub):
    """The restatement's per-sample maps added per cell: sample (i, j) belongs to the cell that holds pixel (2 i, 2 j)."""
    step = 2 if sub else 1
    mh, mw = want["map_den"].shape
    gi = np.searchsorted(np.asarray(ye), step * np.arange(mh), side="right") - 1
    gj = np.searchsorted(np.asarray(xe), step * np.arange(mw), side="right") - 1
    num, den = np.zeros((len(ye) - 1, len(xe) - 1)), np.zeros((len(ye) - 1, len(xe) - 1))
    np.add.at(num, (gi[:, None], gj[None, :]), want["map_num"])
    np.add.at(den, (gi[:, None], gj[None, :]), want["map_den"])
    return num, den


def test_cells_against_the_restatement_and_the_global_record(ctx):
    """67 x 263 (3 x 3 blocks subsampled): odd edges inside a block, a one-pixel cell at an odd pixel (no sample when
    subsampled), through the module methods and their device twins."""
    import _native
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    h, w = 67, 263
    xe, ye = [0, 37, 38, 101, 199, w], [0, 21, 22, 45, h]
    for cn in (3, 1):
        a, b = _case(h, w, cn)
        shape = a.shape
        da = ctx.upload(a)
        pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
        try:
            for conv in CONVENTIONS:
                for sub in (True, False):
                    want = _ref(h, w, cn, 0, sub, conv)
                    rnum, rden = _cells_ref(want, xe, ye, sub)
                    m = q.evaluate_haarpsi_map(a, b, x_edges=xe, y_edges=ye, subsample=sub, convention=conv)
                    md = q.evaluate_haarpsi_map_device(da.ptr, shape, ptr_b, shape, x_edges=xe, y_edges=ye, subsample=sub,
                                                       convention=conv, stride2=sb)
                    assert m["x_edges"] == xe and m["y_edges"] == ye and m["haarpsi"].shape == (4, 5)
                    for k in ("haarpsi", "num", "den"):
                        assert np.array_equal(m[k].view(np.uint64), md[k].view(np.uint64)), (k, conv, sub)
                    empty = rden == 0.0
                    assert empty.any() == sub                               # the cells [37, 38) and [21, 22) hold no even pixel
                    assert np.array_equal(m["den"] == 0.0, empty) and np.isnan(m["haarpsi"][empty]).all()
                    full = ~empty
                    rel = max(np.max(np.abs(m["num"][full] - rnum[full]) / rnum[full]), np.max(np.abs(m["den"][full] - rden[full]) / rden[full]))
                    print(f"cells cn {cn} {conv} sub {sub}: largest rel {rel:.2e}")
                    assert np.allclose(m["num"], rnum, rtol=TOL, atol=0) and np.allclose(m["den"], rden, rtol=TOL, atol=0)
                    for gy, gx in zip(*np.nonzero(full)):
                        x = rnum[gy, gx] / rden[gy, gx]
                        assert m["haarpsi"][gy, gx] == pytest.approx((math.log(x / (1 - x)) / 4.2) ** 2, rel=TOL, abs=0)
                    rec = q.calculate_haarpsi(a, b, subsample=sub, convention=conv, return_parts=True)
                    assert m["num"].sum() == pytest.approx(float(np.sum(rec["num"])), rel=TOL, abs=0)
                    assert m["den"].sum() == pytest.approx(float(np.sum(rec["den"])), rel=TOL, abs=0)
            # uniform cells, the default convention: one cell is the whole image
            one = q.evaluate_haarpsi_map(a, b, cell=512)
            assert one["haarpsi"].shape == (1, 1)
            assert one["haarpsi"][0, 0] == pytest.approx(_ref(h, w, cn, 0, True, "matlab")["value"], rel=TOL, abs=0)
            assert q.evaluate_haarpsi_map(a, b, cell=32)["haarpsi"].shape == (3, 9)
        finally:
            da.free(); pb.free()


@pytest.mark.parametrize("cn", [3, 1, 4])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 37, 43, 3
    a, b = _case(h, w, cn)
    for conv in CONVENTIONS:
        for sub in (True, False):
            dense = _run(ctx, a, b, cb, sub, conv)
            for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
                la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
                pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
                pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
                try:
                    got = ctx.haarpsi(ptr_a, sa, ptr_b, sb, h, w, cn, cb, sub, conv)
                    cells = ctx.haarpsi_cells(ptr_a, sa, ptr_b, sb, h, w, cn, [0, 5, w - 2 * cb], [0, 9, h - 2 * cb], cb, sub, conv)
                    # the calls only read: both parents are as they were, inside the views and outside
                    ra = V.check_guard(ctx, pa, what="image a")
                    rb = V.check_guard(ctx, pb, what="image b")
                finally:
                    pa.free(); pb.free()
                assert _bits(got) == _bits(dense), (conv, sub, V.layout_id(la), V.layout_id(lb))
                assert cells["num"].sum() == pytest.approx(float(np.sum(dense["num"])), rel=TOL, abs=0)
                assert np.array_equal(ra.reshape(a.shape), a) and np.array_equal(rb.reshape(b.shape), b)


def test_rows_beyond_4_gib(ctx):
    """166 rows at a stride of 25 MiB + 5 bytes: rows 164 and 165 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w, cb = 166, 48, 0
    a, b = _case(h, w, 3)
    stride = (25 << 20) + 5
    assert (h - 1 - cb) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    assert total < 8 << 30
    wide = ctx.alloc(total)
    da = ctx.upload(a)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 2, V.FILLS[1])
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, da.ptr + r * w * 3, w * 3)
        ctx.sync()
        for sub in (True, False):
            dense = _run(ctx, a, b, cb, sub)
            got = ctx.haarpsi(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, cb, sub)
            assert _bits(got) == _bits(dense), sub
            _check(got, _ref(h, w, 3, cb, sub, "matlab"), f"wide stride sub {sub}")
    finally:
        wide.free(); da.free(); pb.free()


def test_row_stride_beyond_32_bits(ctx):
    """Three rows 2^32 + 4100 bytes apart (one 8.0 GiB allocation): the stride itself does not fit 32 bits.  A stride cut to
    32 bits anywhere between the Python layer and the loader would read rows 1 and 2 at bytes 4100 and 8200, which hold other
    pixels.  As the first image of the sums and as the second image of the cells, every switch; bits equal to the dense run."""
    h, w = 3, 40
    a, b = _case(h, w, 3)
    stride, lead = (1 << 32) + 4100, 256
    total = lead + (h - 1) * stride + w * 3 + V.GUARD
    assert stride > 1 << 32 and total < 9 << 30
    big = ctx.alloc(total)
    base = big.ptr + lead
    da, db = ctx.upload(a), ctx.upload(b)
    decoy = ctx.upload(np.ascontiguousarray(255 - a))
    try:
        for r in range(h):
            ctx.copy_d2d(base + r * stride, da.ptr + r * w * 3, w * 3)
        for r in (1, 2):                                                    # where a 32-bit stride would look
            ctx.copy_d2d(base + r * 4100, decoy.ptr + r * w * 3, w * 3)
        ctx.sync()
        xe, ye = [0, 13, w], [0, 1, h]
        for conv in CONVENTIONS:
            for sub in (True, False):
                dense = ctx.haarpsi(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 0, sub, conv)
                got = ctx.haarpsi(base, stride, db.ptr, w * 3, h, w, 3, 0, sub, conv)
                assert _bits(got) == _bits(dense), (conv, sub)
                _check(got, _ref(h, w, 3, 0, sub, conv), f"stride 2^32 + 4100 {conv} sub {sub}")
                dense_c = ctx.haarpsi_cells(db.ptr, w * 3, da.ptr, w * 3, h, w, 3, xe, ye, 0, sub, conv)
                got_c = ctx.haarpsi_cells(db.ptr, w * 3, base, stride, h, w, 3, xe, ye, 0, sub, conv)
                for k in ("num", "den"):
                    assert np.array_equal(got_c[k].view(np.uint64), dense_c[k].view(np.uint64)), (k, conv, sub)
                assert got_c["den"].sum() == pytest.approx(float(np.sum(dense["den"])), rel=TOL, abs=0)
    finally:
        big.free(); da.free(); db.free(); decoy.free()


def test_module_methods(ctx):
    import _native
    import quality_assessment_module as qam
    a, b = _case(37, 43, 3)
    q = qam.QualityAssessmentModule()
    for kw in (dict(), dict(convention="python"), dict(subsample=False), dict(crop_border=3, convention="python", subsample=False)):
        want = _ref(37, 43, 3, kw.get("crop_border", 0), kw.get("subsample", True), kw.get("convention", "matlab"))
        v = q.calculate_haarpsi(a, b, **kw)
        assert isinstance(v, float) and v == pytest.approx(want["value"], rel=TOL, abs=0)
        parts = q.calculate_haarpsi(a, b, return_parts=True, **kw)
        assert parts["haarpsi"] == v and parts["channels"] == 3 and parts["count"] == want["map_den"].size
        assert parts["convention"] == kw.get("convention", "matlab") and parts["subsample"] == kw.get("subsample", True)
        assert parts["num"] == pytest.approx(want["num"], rel=TOL, abs=0) and parts["den"] == pytest.approx(want["den"], rel=TOL, abs=0)
        # the device form on resident images gives the same bits, dense and strided
        da = ctx.upload(a)
        pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
        try:
            assert q.calculate_haarpsi_device(da.ptr, a.shape, ptr_b, b.shape, stride2=sb, **kw) == v
            assert q.calculate_haarpsi_device(da.ptr, a.shape, ptr_b, b.shape, stride1=43 * 3, stride2=sb, **kw) == v
        finally:
            da.free(); pb.free()
    assert abs(q.calculate_haarpsi(a, a) - 1.0) <= 1e-12
    assert math.isnan(q.calculate_haarpsi(np.zeros_like(a), np.zeros_like(a)))
    ga, gb = _case(37, 43, 1)
    assert q.calculate_haarpsi(ga, gb, crop_border=1) == pytest.approx(_ref(37, 43, 1, 1, True, "matlab")["value"], rel=TOL, abs=0)


def test_pipeline_hook_at_its_smallest_canvas(ctx, rng):
    """The helper all three QA paths of main.py call, as they call it: a canvas of one row gives None and a note, two rows are
    enough; a black pair gives None and a note; qa_map_cell adds the per-cell entry; overall_score is not touched."""
    import main as sr_main
    src = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    canvas = np.ascontiguousarray(np.repeat(np.repeat(src, 2, 0), 2, 1))
    d_src, d_canvas = ctx.upload(src), ctx.upload(canvas)
    d_black = ctx.upload(np.zeros_like(canvas))
    try:
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_haarpsi=True))
        rep = {}
        pipe._haarpsi(ctx, rep, d_src.ptr, (1, 32, 3), d_canvas.ptr, (1, 64, 3))
        assert sorted(rep) == ["haarpsi", "haarpsi_note"] and rep["haarpsi"] is None and "at least 2" in rep["haarpsi_note"]
        rep = {}
        pipe._haarpsi(ctx, rep, d_src.ptr, (1, 32, 3), d_canvas.ptr, (2, 64, 3))
        assert sorted(rep) == ["haarpsi"] and isinstance(rep["haarpsi"], float) and 0.0 < rep["haarpsi"] <= 1.0
        ref = pipe.quality_module.upsample_bicubic(src[:1], (2, 64))
        assert rep["haarpsi"] == pytest.approx(H.haarpsi_ref(ref, canvas[:2])["value"], rel=TOL, abs=0)
        rep = {}
        pipe._haarpsi(ctx, rep, d_black.ptr, (24, 32, 3), d_black.ptr, (48, 64, 3))
        assert sorted(rep) == ["haarpsi", "haarpsi_note"] and rep["haarpsi"] is None and "black" in rep["haarpsi_note"]
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_haarpsi=True, qa_map_cell=32))
        rep = {}
        pipe._haarpsi(ctx, rep, d_src.ptr, (24, 32, 3), d_canvas.ptr, (48, 64, 3))
        assert sorted(rep) == ["haarpsi", "haarpsi_map"] and rep["haarpsi_map"]["grid"] == [2, 2] and rep["haarpsi_map"]["cell"] == 32
        ref = pipe.quality_module.upsample_bicubic(src, (48, 64))
        want = H.haarpsi_ref(ref, canvas)
        assert rep["haarpsi"] == pytest.approx(want["value"], rel=TOL, abs=0)
        rnum, rden = _cells_ref(want, rep["haarpsi_map"]["x_edges"], rep["haarpsi_map"]["y_edges"], True)
        x = rnum / rden
        assert np.asarray(rep["haarpsi_map"]["haarpsi"]) == pytest.approx((np.log(x / (1 - x)) / 4.2) ** 2, rel=TOL, abs=0)
        assert not sr_main.PipelineConfig().qa_haarpsi
    finally:
        d_src.free(); d_canvas.free(); d_black.free()


def test_pipeline_switch(ctx, rng, tmp_path):
    """Whole runs of the smallest pipeline: without the switch the report has the keys it had; with it, one new key on the
    device-resident path; with qa_map_cell the per-cell entry too, the same on the device-resident and the host-array path."""
    import asyncio
    import json

    import main as sr_main
    from PIL import Image
    import _msssim_ref as M
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("haarpsi", "haarpsi_map", "haarpsi_note")
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_map_cell=64, **kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # the switch alone, device-resident: one new key
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_haarpsi=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "hp" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"]              # takes no part in the overall score
    assert sorted(set(rep) - set(res0.quality_report)) == ["haarpsi"]
    fused = np.asarray(Image.open(out))
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (160, 192))
    assert rep["haarpsi"] == q.calculate_haarpsi(ref_img, fused)
    assert rep["haarpsi"] == pytest.approx(H.haarpsi_ref(ref_img, fused)["value"], rel=TOL, abs=0) and 0.0 < rep["haarpsi"] < 1.0
    assert json.load(open(str(tmp_path / "hp" / "result_qa_report.json")))["haarpsi"] == rep["haarpsi"]
    # with qa_map_cell: the per-cell map over the cells of quality_map; device-resident and host-array paths give the same bits
    reps = []
    for name, extra in (("hp_map", dict()), ("hp_map_host", dict(device_resident=False))):
        p = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_haarpsi=True, qa_map_cell=64, **extra, **kw))
        p.tiling_module.l2_cache_dir = tmp_path
        r = asyncio.run(p.process(src, str(tmp_path / name / "result.png")))
        assert r.success, r.error_message
        reps.append(r.quality_report)
        assert sorted(k for k in r.quality_report if k in keys) == ["haarpsi", "haarpsi_map"]
        assert r.quality_report["haarpsi"] == rep["haarpsi"]
    assert sorted(set(reps[0]) - set(res0.quality_report)) == ["haarpsi", "haarpsi_map"]
    hm = reps[0]["haarpsi_map"]
    assert hm == reps[1]["haarpsi_map"] and hm["cell"] == 64 and hm["grid"] == [3, 3] == reps[0]["quality_map"]["grid"]
    assert hm["x_edges"] == reps[0]["quality_map"]["x_edges"] and hm["y_edges"] == reps[0]["quality_map"]["y_edges"]
    want = q.evaluate_haarpsi_map(ref_img, fused, cell=64)
    assert np.array_equal(np.array(hm["haarpsi"]), want["haarpsi"])
    json.dumps(hm)


def test_sharded_path_and_command_line(tmp_path):
    """main.py --qa-haarpsi --qa-map-cell 128 as the launcher + 2 gloo ranks on the one GPU against the plain one-rank run, in
    the style of tests/test_main_sharded.py: the third QA path, where rank 0 computes the entry from the gathered canvas and
    the report is broadcast, and the command-line flags.  Same file bytes, same entries."""
    import json
    import os
    import subprocess
    import sys

    from PIL import Image
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:300, 0:420]
    img = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (300, 420, 3)), 0, 255)
    src = str(tmp_path / "in.png")
    Image.fromarray(img.astype(np.uint8)).save(src)
    main_py = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "super-resolution-system_amd", "main.py")

    def run(args, env=None, timeout=600):
        e = dict(os.environ)
        e.update(env or {})
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
            e.pop(k, None)
        return subprocess.run([sys.executable, main_py] + args, capture_output=True, text=True, timeout=timeout, env=e)

    flags = ["--block-size", "128", "--qa-haarpsi", "--qa-map-cell", "128"]
    out1, out2 = str(tmp_path / "one.png"), str(tmp_path / "two.png")
    r1 = run([src, out1] + flags)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = run([src, out2] + flags + ["--gpus", "2"], env={"SR_DIST_BACKEND": "gloo"}, timeout=900)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert open(out1, "rb").read() == open(out2, "rb").read()
    q1 = json.load(open(str(tmp_path / "one_qa_report.json")))
    q2 = json.load(open(str(tmp_path / "two_qa_report.json")))
    assert isinstance(q1["haarpsi"], float) and 0.0 < q1["haarpsi"] < 1.0 and "haarpsi_note" not in q1
    assert q2["haarpsi"] == q1["haarpsi"] and q2["haarpsi_map"] == q1["haarpsi_map"]
    assert q1["haarpsi_map"]["cell"] == 128 and q1["haarpsi_map"]["grid"] == q1["quality_map"]["grid"]
    fused = np.asarray(Image.open(out1))
    import quality_assessment_module as qam
    ref_img = qam.QualityAssessmentModule().upsample_bicubic(img.astype(np.uint8), fused.shape[:2])
    assert q1["haarpsi"] == pytest.approx(H.haarpsi_ref(ref_img, fused)["value"], rel=TOL, abs=0)
