"""GPU: the per-pixel colour difference, CIEDE2000 and CIE76 (sr_delta_e_u8, sr_delta_e_cells_u8, csrc/sr_deltae.hip).

* parity, PINNED: every case of tests/golden/deltae_skimage.npz (scikit-image 0.18.3's own rgb2lab and deltaE maps), both
  formulas: the dense map at 1e-9 absolute, sum / sum2 / max / mean at 1e-9 relative, the count and the whole histogram equal;
* restatement (tests/_deltae_ref.py, itself held to the fixture at 1e-12): 1 x 1, 1 x 7, 3 x 1 and both sides of every constant
  of the kernels -- DE_LANES = 64 and DE_RUN = 4 (a thread's 4 pixels are 64 columns apart: 63 .. 65, 127 .. 129, 191 .. 193
  columns), the tile of DE_TW = 256 columns (255 .. 257, 513) by DE_TH = 4 rows (3 .. 5), DE_MAX_BLOCKS = 2048 (2048 and 2049
  tiles: a block then takes a second tile) --, one multi-block image, cn = 1, 3, 4 and crop borders 0 .. 3 at every alignment;
* values: identical images give exactly 0 everywhere; swapped arguments agree; a constant pair gives the host function's value;
* cells: uniform cells, a one-pixel cell, uneven edges, both sides of DE_CELL_ROWS = 64 rows and of the 256 columns of a block:
  every cell sum against the restatement at 1e-9 relative; the cell maxima equal to the restatement's cell rule on the map the
  sums launch wrote (and within 1e-9 of the NumPy values, whose cbrt / atan2 / cos differ from the device's in the last bits);
  the cells add up to the global sum at 1e-12 relative and the largest cell max is the global max, exactly;
* bits: equal inputs give equal bits, also after the scratch has grown; padded, offset, guarded views (one with rows beyond
  2^32 bytes, for the inputs and for the map) give the dense bits and nothing outside is written;
* the module methods, their device twins and the pipeline switch on the device-resident and the host-array path; the sharded
  path and the command line (main.py --qa-delta-e [--qa-map-cell N]) as a two-rank gloo rehearsal on the one card against the
  one-rank run.
Where the issue asks for equality between device and host values (a constant pair's max, the cell maxima) the bar is 1e-9: the two
math libraries differ in the last bits.  Equality is asserted wherever both sides come from the device."""
import asyncio
import functools
import os

import numpy as np
import pytest

import _deltae_ref as R
import _views as V

pytestmark = pytest.mark.gpu

TOL = 1e-9
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deltae_skimage.npz")
FORMULAS = ((R.CIEDE2000, "de00"), (R.CIE76, "de76"))


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def _case(h, w, cn=3):
    """One image pair per shape, made once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, cb, formula):
    a, b = _case(h, w, cn)
    m = R.delta_e_map(a, b, formula, cb)
    m.setflags(write=False)
    return m


def _cn(a):
    return a.shape[2] if a.ndim == 3 else 1


def _run(ctx, a, b, cb=0, formula=R.CIEDE2000, want_map=True):
    """-> (record, dense map or None)"""
    cn, (h, w) = _cn(a), a.shape[:2]
    ch, cw = h - 2 * cb, w - 2 * cb
    da, db = ctx.upload(a), ctx.upload(b)
    dm = ctx.alloc(ch * cw * 8) if want_map else None
    try:
        rec = ctx.delta_e_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, crop_border=cb, formula=formula,
                             d_map=dm.ptr if dm else 0, map_stride=cw * 8 if dm else 0)
        return rec, (ctx.download(dm.ptr, (ch, cw), np.float64) if dm else None)
    finally:
        da.free(); db.free()
        if dm:
            dm.free()


def _bits(rec):
    return (rec["count"], np.float64(rec["sum"]).view(np.uint64), np.float64(rec["sum2"]).view(np.uint64),
            np.float64(rec["max"]).view(np.uint64), rec["hist"].tobytes())


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def _check(rec, dmap, want_map, what, exact_hist):
    """The map at 1e-9 absolute, the sums at 1e-9 relative, the histogram against the reference's (exact_hist: the fixture,
    whose values keep 1e-6 from every bin edge) and always against the map the same launch wrote.  -> largest distances."""
    import _native
    want = R.sums(want_map)
    d_map = float(np.abs(dmap - want_map).max())
    mean = _native.delta_e_mean_rms(rec)[0]
    rels = {k: _rel(rec[k], want[k]) for k in ("sum", "sum2", "max")}
    rels["mean"] = _rel(mean, want["sum"] / want["count"])
    print(f"{what}: map {d_map:.2e} abs; " + ", ".join(f"{k} {v:.2e}" for k, v in rels.items()) + " rel")
    assert dmap.shape == want_map.shape and d_map <= TOL, what
    assert rec["count"] == want["count"] == int(rec["hist"].sum()), what
    assert all(v <= TOL for v in rels.values()), (what, rels)
    assert np.array_equal(rec["hist"], R.histogram(dmap)), what           # the record and the map of one launch agree exactly
    assert rec["max"] == dmap.max(), what
    assert np.array_equal(dmap == 0.0, want_map == 0.0), what            # byte-equal pairs, and only they, are exactly 0
    if exact_hist:
        assert np.array_equal(rec["hist"], want["hist"]), what
    return d_map, max(rels.values())


def test_fixture_cases_match_scikit_image(ctx):
    g = _gold()
    worst_map = worst_rel = 0.0
    for name in (str(c) for c in g["cases"]):
        a, b = np.ascontiguousarray(g[f"{name}_a"]), np.ascontiguousarray(g[f"{name}_b"])
        for f, key in FORMULAS:
            rec, dmap = _run(ctx, a, b, 0, f)
            m, r = _check(rec, dmap, g[f"{name}_{key}"], f"{name} {key}", exact_hist=True)
            worst_map, worst_rel = max(worst_map, m), max(worst_rel, r)
            assert _bits(_run(ctx, a, b, 0, f, want_map=False)[0]) == _bits(rec), (name, key)     # the map changes no sum
    print(f"against scikit-image 0.18.3: largest distance of a map value {worst_map:.2e}, of a sum {worst_rel:.2e} relative")


# DE_LANES 64, DE_RUN 4, DE_TW 256, DE_TH 4: both sides of each, the smallest sizes first
SHAPES = [(1, 1), (1, 7), (3, 1), (3, 63), (4, 64), (5, 65), (3, 127), (4, 128), (5, 129), (4, 191), (3, 192), (5, 193),
          (3, 255), (4, 256), (5, 257), (9, 513)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes_match_the_restatement(ctx, h, w):
    import _native
    assert [_native.delta_e_plan(hh, ww, 3)["blocks"] for hh, ww in ((4, 256), (5, 256), (4, 257), (5, 257))] == [1, 2, 2, 4]
    a, b = _case(h, w, 3)
    for f, key in FORMULAS:
        rec, dmap = _run(ctx, a, b, 0, f)
        _check(rec, dmap, _ref(h, w, 3, 0, f), f"{h}x{w} {key}", exact_hist=False)


@pytest.mark.parametrize("h,w", [(41, 300), (4 * 2048, 5), (4 * 2048 + 1, 5), (4 * 2048 + 5, 3)], ids=lambda v: str(v))
def test_multi_block_and_the_block_cap(ctx, h, w):
    """41 x 300: 11 x 2 tiles, the last of either axis partial.  8192 x 5 is 2048 tiles, one per block; 8193 and 8197 rows are
    2049 and 2050: blocks 0 and 1 take a second tile."""
    import _native
    tiles = -(-h // 4) * -(-w // 256)
    assert _native.delta_e_plan(h, w, 3)["blocks"] == min(tiles, 2048)
    a, b = _case(h, w, 3)
    rec, dmap = _run(ctx, a, b, 0, R.CIEDE2000)
    _check(rec, dmap, _ref(h, w, 3, 0, R.CIEDE2000), f"{h}x{w} de00", exact_hist=False)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_channels_and_crop_borders_at_every_alignment(ctx, cn):
    """23 x 37: odd sides; cb * cn mod 4 walks every residue for cn = 1 and 3.  The crop is pointer arithmetic: the cropped
    call and the call on the cropped copy give the same bits.  Alpha is ignored."""
    h, w = 23, 37
    a, b = _case(h, w, cn)
    seen = set()
    for cb in (0, 1, 2, 3):
        for f, key in FORMULAS:
            rec, dmap = _run(ctx, a, b, cb, f)
            _check(rec, dmap, _ref(h, w, cn, cb, f), f"cn {cn} cb {cb} {key}", exact_hist=False)
            ac, bc = np.ascontiguousarray(R.crop(a, cb)), np.ascontiguousarray(R.crop(b, cb))
            rec_c, dmap_c = _run(ctx, ac, bc, 0, f)
            assert _bits(rec_c) == _bits(rec) and np.array_equal(dmap_c, dmap), (cn, cb, key)
        seen.add(rec["sum"])
    assert len(seen) == 4                                                   # the crops are told apart
    if cn == 4:
        a2 = a.copy(); a2[..., 3] ^= 0xFF
        assert _bits(_run(ctx, a2, b, 1, R.CIEDE2000, want_map=False)[0]) == _bits(_run(ctx, a, b, 1, R.CIEDE2000, want_map=False)[0])
    if cn == 1:                                                             # gray is R = G = B, as one plane or as h x w x 1
        rgb = np.ascontiguousarray(np.repeat(a[..., None], 3, 2)), np.ascontiguousarray(np.repeat(b[..., None], 3, 2))
        r1, m1 = _run(ctx, a, b, 2, R.CIEDE2000)
        r3, m3 = _run(ctx, rgb[0], rgb[1], 2, R.CIEDE2000)
        assert _bits(r1) == _bits(r3) and np.array_equal(m1, m3)
        assert _bits(_run(ctx, np.ascontiguousarray(a[..., None]), np.ascontiguousarray(b[..., None]), 2)[0]) == _bits(r1)


def test_identical_swapped_and_constant_pairs(ctx):
    import _native
    for (h, w), cn in (((5, 7), 3), ((9, 513), 3), ((23, 37), 1), ((23, 37), 4)):
        a = _case(h, w, cn)[0]
        for f, _ in FORMULAS:
            rec, dmap = _run(ctx, a, a, 0, f)
            assert rec["sum"] == 0.0 and rec["sum2"] == 0.0 and rec["max"] == 0.0 and not dmap.any(), (h, w, cn)
            assert rec["hist"][0] == rec["count"] == h * w and int(rec["hist"].sum()) == h * w
            assert [_native.delta_e_percentile(rec, p) for p in (50, 95, 99, 100)] == [0.0] * 4
            assert _native.delta_e_fraction(rec, 0.0625) == 0.0 and _native.delta_e_fraction(rec, 0) == 1.0
    a, b = _case(41, 300, 3)
    for f, key in FORMULAS:
        r1, m1 = _run(ctx, a, b, 1, f)
        r2, m2 = _run(ctx, b, a, 1, f)
        assert np.abs(m1 - m2).max() <= 1e-12 * m1.max(), key
        # dE(a, b) and dE(b, a) differ in the last bits, so a count may cross a bin edge: each histogram is held to its own map
        assert np.array_equal(r1["hist"], R.histogram(m1)) and np.array_equal(r2["hist"], R.histogram(m2)), key
        for k in ("sum", "sum2", "max"):
            assert r1[k] == pytest.approx(r2[k], rel=1e-12, abs=0), (key, k)
    # a constant pair of colours: the host function's value in max -- at 1e-9 relative, not bit for bit: the host's and the
    # device's cbrt / atan2 / cos differ in the last bits (the values are printed) --, every map value equal to max, and the
    # mean within 1e-12 of it
    for c1, c2 in (((200, 30, 40), (190, 45, 30)), ((0, 0, 0), (255, 255, 255)), ((0, 0, 255), (255, 255, 0)), ((10, 10, 10), (0, 0, 0))):
        x = np.empty((13, 70, 3), np.uint8); x[:] = c1
        y = np.empty((13, 70, 3), np.uint8); y[:] = c2
        for f, key in FORMULAS:
            want = _native.delta_e_pair(_native.delta_e_lab(*c1), _native.delta_e_lab(*c2), f)
            rec, dmap = _run(ctx, x, y, 0, f)
            print(f"{c1} / {c2} {key}: host {want!r} device {rec['max']!r}")
            assert rec["max"] == pytest.approx(want, rel=TOL, abs=0) and (dmap == rec["max"]).all()
            assert _native.delta_e_mean_rms(rec)[0] == pytest.approx(rec["max"], rel=1e-12, abs=0)
            assert rec["hist"][min(int(16 * rec["max"]), 2047)] == 13 * 70
    assert _run(ctx, x, y, 0, R.CIEDE2000)[0]["max"] > 1.0


def _cells(ctx, a, b, xe, ye, cb=0, formula=R.CIEDE2000):
    cn, (h, w) = _cn(a), a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.delta_e_cells_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, xe, ye, crop_border=cb, formula=formula)
    finally:
        da.free(); db.free()


def _uniform(n, cell):
    return list(range(0, n, cell)) + [n]


# (h, w, cb, x_edges, y_edges): uniform cells, a one-pixel cell, uneven edges; DE_CELL_ROWS = 64: cell rows of 63, 64, 65 and 129
# rows (one, one, two and three chunks); 255 .. 257 and 513 columns: one, one, two and three column blocks
CELL_CASES = [
    ("uniform 8", 23, 37, 0, _uniform(37, 8), _uniform(23, 8)),
    ("one cell", 5, 7, 0, [0, 7], [0, 5]),
    ("1 x 1 image", 1, 1, 0, [0, 1], [0, 1]),
    ("one-pixel cells, uneven", 23, 37, 1, [0, 1, 2, 20, 34, 35], [0, 1, 9, 10, 21]),
    ("cropped uniform", 41, 300, 3, _uniform(294, 100), _uniform(35, 16)),
    ("rows 63 | 64 | 65 | 129", 63 + 64 + 65 + 129, 9, 0, [0, 4, 9], [0, 63, 127, 192, 321]),
    ("columns 255", 3, 255, 0, [0, 255], [0, 3]),
    ("columns 256", 3, 256, 0, [0, 100, 256], [0, 3]),
    ("columns 257", 3, 257, 0, [0, 256, 257], [0, 1, 3]),
    ("columns 513", 9, 513, 0, [0, 255, 257, 512, 513], [0, 4, 9]),
]


@pytest.mark.parametrize("name,h,w,cb,xe,ye", CELL_CASES, ids=[c[0] for c in CELL_CASES])
def test_cells(ctx, name, h, w, cb, xe, ye):
    a, b = _case(h, w, 3)
    for f, key in FORMULAS:
        want_s, want_m = R.cells(_ref(h, w, 3, cb, f), xe, ye)
        got = _cells(ctx, a, b, xe, ye, cb, f)
        rec, dmap = _run(ctx, a, b, cb, f)
        assert got["sum"].shape == got["max"].shape == (len(ye) - 1, len(xe) - 1)
        rel = np.abs(got["sum"] - want_s) / np.where(want_s == 0, 1.0, want_s)
        print(f"{name} {key}: cell sums {rel.max():.2e} rel, cells summed against sum {_rel(float(got['sum'].sum()), rec['sum']):.2e}")
        assert rel.max() <= TOL and np.array_equal(got["sum"] == 0, want_s == 0)
        assert np.abs(got["max"] - want_m).max() <= TOL                     # against the restatement: its own rounding
        assert np.array_equal(got["max"], R.cells(dmap, xe, ye)[1])         # against the map of the sums launch: equal
        assert float(got["sum"].sum()) == pytest.approx(rec["sum"], rel=1e-12, abs=0)
        assert got["max"].max() == rec["max"]


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    import _native
    h, w = 41, 300
    a, b = _case(h, w, 3)
    big_a, big_b = _case(4 * 2048 + 1, 5, 3)
    xe, ye = _uniform(w - 4, 64), _uniform(h - 4, 16)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for f, _ in FORMULAS:
            first = ctx.delta_e_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, f)
            second = ctx.delta_e_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, f)
            c1 = ctx.delta_e_cells_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye, 2, f)
            ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
            assert _native.delta_e_plan(4 * 2048 + 1, 5, 3)["scratch_bytes"] > _native.delta_e_plan(h, w, 3, 2)["scratch_bytes"]
            big = _run(ctx, big_a, big_b, 0, f, want_map=False)[0]          # larger launches through the scratch: the table moves
            _cells(ctx, big_a, big_b, [0, 5], _uniform(4 * 2048 + 1, 100), 0, f)
            third = ctx.delta_e_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, f)
            c2 = ctx.delta_e_cells_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye, 2, f)
            assert _bits(first) == _bits(second) == _bits(third), f
            assert c1["sum"].tobytes() == c2["sum"].tobytes() and c1["max"].tobytes() == c2["max"].tobytes(), f
            assert _bits(big) == _bits(_run(ctx, big_a, big_b, 0, f, want_map=False)[0]), f
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("cn", [3, 1, 4])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 23, 37, 3
    ch, cw = h - 2 * cb, w - 2 * cb
    a, b = _case(h, w, cn)
    xe, ye = [0, 1, 20, cw], [0, 9, ch]
    for f, key in FORMULAS:
        dense, dense_map = _run(ctx, a, b, cb, f)
        dense_cells = _cells(ctx, a, b, xe, ye, cb, f)
        for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
            la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
            lm = V.pick(V.LAYOUTS_F32, k)
            pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
            pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
            pm, ptr_m, sm = V.out_view(ctx, ch, cw * 8, 2 * lm[0], 2 * lm[1], fill)     # offsets and pads in multiples of 8
            try:
                got = ctx.delta_e_u8(ptr_a, sa, ptr_b, sb, h, w, cn, cb, f, d_map=ptr_m, map_stride=sm)
                cells = ctx.delta_e_cells_u8(ptr_a, sa, ptr_b, sb, h, w, cn, xe, ye, cb, f)
                # the inputs are only read; of the map's parent only the view is written
                ra = V.check_guard(ctx, pa, what="image a")
                rb = V.check_guard(ctx, pb, what="image b")
                gm = V.check_guard(ctx, pm, dtype=np.float64, shape=(ch, cw), what="the map")
            finally:
                pa.free(); pb.free(); pm.free()
            assert _bits(got) == _bits(dense), (key, V.layout_id(la), V.layout_id(lb))
            assert gm.tobytes() == dense_map.tobytes(), (key, V.layout_id(lm))
            assert cells["sum"].tobytes() == dense_cells["sum"].tobytes() and cells["max"].tobytes() == dense_cells["max"].tobytes()
            assert np.array_equal(ra.reshape(a.shape), a) and np.array_equal(rb.reshape(b.shape), b)


def test_rows_beyond_4_gib(ctx):
    """166 rows at a stride of 25 MiB + 5 bytes (inputs) and 25 MiB + 8 (the map): rows 164 and 165 start beyond 2^32 bytes.  A
    kernel that formed a 32-bit row * stride would read, or write, them in the wrong place."""
    h, w, cb = 166, 48, 0
    a, b = _case(h, w, 3)
    stride, mstride = (25 << 20) + 5, (25 << 20) + 8
    assert (h - 1 - cb) * stride >= 1 << 32
    total, mtotal = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD, V.GUARD + (h - 1) * mstride + w * 8 + V.GUARD
    assert total < 8 << 30 and mtotal < 8 << 30
    wide, wmap = ctx.alloc(total), ctx.alloc(mtotal)
    da, rows = ctx.upload(a), ctx.alloc(h * w * 8)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 2, V.FILLS[1])
    xe, ye = [0, 20, w], [0, 100, 165, h]
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, da.ptr + r * w * 3, w * 3)
        ctx.sync()
        for f, key in FORMULAS:
            dense, dense_map = _run(ctx, a, b, cb, f)
            got = ctx.delta_e_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, cb, f, d_map=wmap.ptr + V.GUARD, map_stride=mstride)
            assert _bits(got) == _bits(dense), key
            for r in range(h):
                ctx.copy_d2d(rows.ptr + r * w * 8, wmap.ptr + V.GUARD + r * mstride, w * 8)
            ctx.sync()
            assert ctx.download(rows.ptr, (h, w), np.float64).tobytes() == dense_map.tobytes(), key
            cells = ctx.delta_e_cells_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, xe, ye, cb, f)
            dc = _cells(ctx, a, b, xe, ye, cb, f)
            assert cells["sum"].tobytes() == dc["sum"].tobytes() and cells["max"].tobytes() == dc["max"].tobytes(), key
            _check(got, dense_map, _ref(h, w, 3, cb, f), f"wide stride {key}", exact_hist=False)
    finally:
        wide.free(); wmap.free(); da.free(); rows.free(); pb.free()


def test_module_methods(ctx):
    import _native
    import quality_assessment_module as qam
    a, b = _case(41, 300, 3)
    q = qam.QualityAssessmentModule()
    KEYS = ['count', 'formula', 'frac_above_1', 'frac_above_3', 'frac_above_5', 'level', 'max', 'mean', 'p50', 'p95', 'p99', 'rms']
    for formula, f in (("ciede2000", R.CIEDE2000), ("cie76", R.CIE76)):
        rec, dmap = _run(ctx, a, b, 2, f)
        want = R.sums(_ref(41, 300, 3, 2, f))
        r = q.calculate_delta_e(a, b, formula=formula, crop_border=2)
        assert sorted(r) == KEYS and r["formula"] == formula and r["count"] == 37 * 296
        assert (r["mean"], r["rms"]) == _native.delta_e_mean_rms(rec) and r["max"] == rec["max"]
        assert r["mean"] == pytest.approx(want["sum"] / want["count"], rel=TOL, abs=0)
        assert r["rms"] == pytest.approx((want["sum2"] / want["count"]) ** 0.5, rel=TOL, abs=0)
        for p in (50, 95, 99):
            assert r[f"p{p}"] == _native.delta_e_percentile(rec, p) == R.percentile(rec["hist"], rec["count"], p)
            true = np.sort(dmap.ravel())[max(1, -(-p * dmap.size // 100)) - 1]                 # the k-th smallest value
            assert r[f"p{p}"] <= true < r[f"p{p}"] + 1 / 16.0
        for t in (1, 3, 5):
            assert r[f"frac_above_{t}"] == float((dmap >= t).sum()) / dmap.size
        assert r["level"] == q._assess_delta_e(r["mean"]) and r["level"] in ("excellent", "good", "fair", "poor")
        rm = q.calculate_delta_e(a, b, formula=formula, crop_border=2, percentiles=(10, 99.9), return_map=True)
        assert sorted(rm) == sorted([k for k in KEYS if k[0] != "p"] + ["p10", "p99.9", "map"])
        assert rm["map"].dtype == np.float64 and rm["map"].tobytes() == dmap.tobytes() and rm["mean"] == r["mean"]
        # the device form on resident images gives the same bits, dense and strided
        da = ctx.upload(a)
        pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
        try:
            assert q.calculate_delta_e_device(da.ptr, a.shape, ptr_b, b.shape, formula=formula, crop_border=2, stride2=sb) == r
            rd = q.calculate_delta_e_device(da.ptr, a.shape, ptr_b, b.shape, formula=formula, crop_border=2, stride1=300 * 3,
                                            stride2=sb, return_map=True)
            assert rd["map"].tobytes() == dmap.tobytes()
            m = q.evaluate_delta_e_map(a, b, cell=64, formula=formula)
            md = q.evaluate_delta_e_map_device(da.ptr, a.shape, ptr_b, b.shape, cell=64, formula=formula, stride2=sb)
        finally:
            da.free(); pb.free()
        assert m["x_edges"] == [0, 64, 128, 192, 256, 300] and m["y_edges"] == [0, 41] and m["mean"].shape == (1, 5)
        assert all(np.array_equal(m[k], md[k]) for k in ("mean", "max")) and md["x_edges"] == m["x_edges"]
        ws, wm = R.cells(_ref(41, 300, 3, 0, f), m["x_edges"], m["y_edges"])
        area = np.outer(np.diff(m["y_edges"]), np.diff(m["x_edges"]))
        assert np.abs(m["mean"] - ws / area).max() <= TOL * (ws / area).max() and np.abs(m["max"] - wm).max() <= TOL
        full = q.calculate_delta_e(a, b, formula=formula)
        assert float((m["mean"] * area).sum()) / area.sum() == pytest.approx(full["mean"], rel=1e-12, abs=0)
        assert m["max"].max() == full["max"]
        e = q.evaluate_delta_e_map(a, b, x_edges=[0, 1, 300], y_edges=[0, 40, 41], formula=formula)
        assert e["mean"].shape == (2, 2) and e["max"][0, 0] == _run(ctx, np.ascontiguousarray(a[:40, :1]), np.ascontiguousarray(b[:40, :1]), 0, f)[0]["max"]
    # defaults: CIEDE2000, no crop; identical images; a gray and an RGBA pair
    assert q.calculate_delta_e(a, b) == q.calculate_delta_e(a, b, formula="ciede2000", crop_border=0, percentiles=(50, 95, 99))
    same = q.calculate_delta_e(a, a)
    assert same["mean"] == same["max"] == same["p99"] == same["frac_above_1"] == 0.0 and same["level"] == "excellent"
    for cn in (1, 4):
        x, y = _case(23, 37, cn)
        assert q.calculate_delta_e(x, y, crop_border=1)["mean"] == pytest.approx(float(_ref(23, 37, cn, 1, R.CIEDE2000).mean()), rel=TOL, abs=0)


def test_pipeline_switch(ctx, rng, tmp_path):
    import json

    import main as sr_main
    from PIL import Image
    import _msssim_ref as M
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("delta_e", "delta_e_map", "delta_e_note")
    # default: the report has exactly the keys it had
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    pipe0m = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_map_cell=64, **kw))
    pipe0m.tiling_module.l2_cache_dir = tmp_path
    res0m = asyncio.run(pipe0m.process(src, str(tmp_path / "plain_map" / "result.png")))
    assert res0m.success and sorted(set(res0m.quality_report) - set(res0.quality_report)) == ["quality_map"]
    # the switch alone, device-resident: one new key
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_delta_e=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "de" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"]              # takes no part in the overall score
    assert sorted(set(rep) - set(res0.quality_report)) == ["delta_e"]
    fused = np.asarray(Image.open(out))
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (160, 192))
    assert rep["delta_e"] == q.calculate_delta_e(ref_img, fused) and rep["delta_e"]["formula"] == "ciede2000"
    assert rep["delta_e"]["mean"] == pytest.approx(float(R.delta_e_map(ref_img, fused).mean()), rel=TOL, abs=0)
    assert rep["delta_e"]["count"] == 160 * 192 and rep["delta_e"]["max"] > 0.0
    assert json.load(open(str(tmp_path / "de" / "result_qa_report.json")))["delta_e"] == rep["delta_e"]
    # with qa_map_cell: the per-cell map over the cells of quality_map; device-resident and host-array paths give the same bits
    reps = []
    for name, extra in (("de_map", dict()), ("de_map_host", dict(device_resident=False))):
        p = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_delta_e=True, qa_map_cell=64, **extra, **kw))
        p.tiling_module.l2_cache_dir = tmp_path
        r = asyncio.run(p.process(src, str(tmp_path / name / "result.png")))
        assert r.success, r.error_message
        reps.append(r.quality_report)
        assert sorted(k for k in r.quality_report if k in keys) == ["delta_e", "delta_e_map"]
        assert r.quality_report["delta_e"] == rep["delta_e"]
    assert sorted(set(reps[0]) - set(res0m.quality_report)) == ["delta_e", "delta_e_map"]
    dm = reps[0]["delta_e_map"]
    assert dm == reps[1]["delta_e_map"] and dm["cell"] == 64 and dm["grid"] == [3, 3] == reps[0]["quality_map"]["grid"]
    assert dm["x_edges"] == reps[0]["quality_map"]["x_edges"] and dm["y_edges"] == reps[0]["quality_map"]["y_edges"]
    want = q.evaluate_delta_e_map(ref_img, fused, cell=64)
    assert np.array_equal(np.array(dm["mean"]), want["mean"]) and np.array_equal(np.array(dm["max"]), want["max"])
    assert np.array(dm["max"]).max() == rep["delta_e"]["max"]
    json.dumps(reps[0]["delta_e_map"])
    # the one helper all three QA paths call, as they call it (the sharded path: test_sharded_path_and_command_line): keys
    # already in the report stay, and a refusal gives None and a note, not an error
    d_src, d_canvas = ctx.upload(img), ctx.upload(np.ascontiguousarray(fused))
    try:
        rep_s = {"kept": 1}
        pipe._delta_e(ctx, rep_s, d_src.ptr, (80, 96, 3), d_canvas.ptr, (160, 192, 3))
        assert rep_s == {"kept": 1, "delta_e": rep["delta_e"]}
        rep_t = {}
        pipe._delta_e(ctx, rep_t, d_src.ptr, (80, 96, 2), d_canvas.ptr, (160, 192, 2))
        assert rep_t == {"delta_e": None, "delta_e_note": rep_t["delta_e_note"]} and "channels" in rep_t["delta_e_note"]
    finally:
        d_src.free(); d_canvas.free()


def _main(args, env=None, timeout=600):
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env or {})
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    main_py = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "super-resolution-system_amd", "main.py")
    return subprocess.run([sys.executable, main_py] + args, capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("cell", [0, 128], ids=["no-map", "map-cell-128"])
def test_sharded_path_and_command_line(tmp_path, cell):
    """main.py --qa-delta-e (with and without --qa-map-cell) as the launcher + 2 gloo ranks on the one GPU against the plain
    one-rank run, in the style of tests/test_main_sharded.py: the third QA path, where rank 0 computes the entry from the
    gathered canvas and the report is broadcast, and the command-line flags.  Same file bytes, same report; without the
    flags the report has neither key."""
    import json

    from PIL import Image
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:300, 0:420]
    img = np.clip((128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None] + rng.integers(-12, 13, (300, 420, 3)), 0, 255)
    src = str(tmp_path / "in.png")
    Image.fromarray(img.astype(np.uint8)).save(src)
    flags = ["--block-size", "128", "--qa-delta-e"] + (["--qa-map-cell", str(cell)] if cell else [])
    out1, out2 = str(tmp_path / "one.png"), str(tmp_path / "two.png")
    r1 = _main([src, out1] + flags)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = _main([src, out2] + flags + ["--gpus", "2"], env={"SR_DIST_BACKEND": "gloo"}, timeout=900)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert open(out1, "rb").read() == open(out2, "rb").read()
    q1 = json.load(open(str(tmp_path / "one_qa_report.json")))
    q2 = json.load(open(str(tmp_path / "two_qa_report.json")))
    for q in (q1, q2):
        q.pop("timestamp")
        if cell:
            q["quality_map"].pop("image")                                   # named after the output file
    assert q1 == q2
    de = q1["delta_e"]
    assert de is not None and "delta_e_note" not in q1 and de["formula"] == "ciede2000" and de["count"] == 600 * 840
    assert 0.0 < de["mean"] <= de["rms"] <= de["max"] and de["p50"] <= de["p95"] <= de["p99"] <= de["max"]
    fused = np.asarray(Image.open(out2))
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    want = q.calculate_delta_e(q.upsample_bicubic(img.astype(np.uint8), (600, 840)), fused)
    assert de == want
    if cell:
        dm = q1["delta_e_map"]
        assert dm["cell"] == 128 and dm["grid"] == [5, 7] == q1["quality_map"]["grid"] and dm["x_edges"] == q1["quality_map"]["x_edges"]
        assert np.array(dm["max"]).max() == de["max"]
    else:
        assert "delta_e_map" not in q1 and "quality_map" not in q1
        r0 = _main([src, str(tmp_path / "plain.png"), "--block-size", "128"])
        assert r0.returncode == 0, r0.stdout[-2000:] + r0.stderr[-2000:]
        q0 = json.load(open(str(tmp_path / "plain_qa_report.json")))
        q0.pop("timestamp")
        assert sorted(set(q1) - set(q0)) == ["delta_e"] and set(q0) <= set(q1)
