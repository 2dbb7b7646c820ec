"""GPU: the gradient magnitude similarity deviation (sr_gmsd_u8, csrc/sr_gmsd.hip).

* restatement: the sums of d and d^2 and the score of every mode against tests/_gmsd_ref.py (MATLAB's q, np.std(ddof=1) in two
  passes) at 1e-9 relative, counts equal -- at the smallest sizes (4 x 4; 5 x 7, where the zero row and column enter the 2 x 2
  mean), odd and even sides around the kernel's tile (16 x 64 samples of the half-size map: 31 .. 34 rows, 127 .. 130
  columns), one multi-block image and crop borders at every alignment;
* values: identical images give exactly 0;
* bits: equal inputs give equal bits, also after the scratch has grown; padded, offset, guarded views (one with rows beyond
  2^32 bytes) give the dense bits and nothing outside is written;
* the module methods and their device twins (the pipeline switches: tests/test_gpu_vif.py).
parity: unpinned (MATLAB, piq, pyiqa are not available offline); pinned by the restatement alone."""
import functools

import numpy as np
import pytest

import _gmsd_ref as G
import _views as V
import _vif_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
MODES = ((R.Y, "y", 3), (R.Y_ROUND, "y_round", 3), (R.CHANNELS, "gray", 1))


@functools.lru_cache(maxsize=None)
def _case(h, w, cn=3):
    """One image pair per shape, made once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn, noise=20.0)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, cb, mode):
    a, b = _case(h, w, cn)
    r = G.gmsd(a, b, cb, mode)
    return {k: r[k] for k in ("score", "sum_d", "sum_d2", "count")}


def _run(ctx, a, b, cb=0, mode=R.Y):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.gmsd_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, crop_border=cb, mode=mode)
    finally:
        da.free(); db.free()


def _bits(rec):
    return (np.float64(rec["sum_d"]).view(np.uint64), np.float64(rec["sum_d2"]).view(np.uint64), rec["count"])


def _check(got, want, what):
    import _native
    score = _native.gmsd_value(got)
    for k, g in (("sum_d", got["sum_d"]), ("sum_d2", got["sum_d2"]), ("score", score)):
        print(f"{what}: {k} {g!r} ref {want[k]!r} rel {abs(g - want[k]) / abs(want[k]):.2e}")
    assert got["count"] == want["count"], what
    assert want["sum_d"] > 0 and want["score"] > 0, what
    assert got["sum_d"] == pytest.approx(want["sum_d"], rel=TOL, abs=0), what
    assert got["sum_d2"] == pytest.approx(want["sum_d2"], rel=TOL, abs=0), what
    assert score == pytest.approx(want["score"], rel=TOL, abs=0), what


SHAPES = [(4, 4), (5, 7), (8, 5), (31, 127), (32, 128), (33, 129), (34, 130), (97, 130)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_modes_match_the_restatement(ctx, h, w):
    import _native
    assert [_native.gmsd_plan(s, s, 3)["size"][0] for s in (31, 32, 33, 127, 128, 129)] == [16, 16, 17, 64, 64, 65]
    for mode, name, cn in MODES:
        a, b = _case(h, w, cn)
        _check(_run(ctx, a, b, 0, mode), _ref(h, w, cn, 0, mode), f"{h}x{w} {name}")


@pytest.mark.parametrize("cb", [0, 1, 2, 3])
def test_crop_borders_at_every_alignment(ctx, cb):
    """53 x 67: odd sides, cb * 3 mod 4 is 0, 3, 2, 1; the crop changes the parity of both sides' halves."""
    h, w = 53, 67
    for mode, name, cn in MODES:
        a, b = _case(h, w, cn)
        got = _run(ctx, a, b, cb, mode)
        _check(got, _ref(h, w, cn, cb, mode), f"cb {cb} {name}")
        ac, bc = np.ascontiguousarray(R.crop(a, cb)), np.ascontiguousarray(R.crop(b, cb))
        assert _bits(_run(ctx, ac, bc, 0, mode)) == _bits(got), (cb, name)
    assert len({_ref(h, w, 3, c, R.Y)["score"] for c in (0, 1, 2, 3)}) == 4      # the crops are told apart


def test_multi_block(ctx):
    """603 x 701: a 302 x 351 map, 19 x 6 tiles, the last of either axis partial."""
    h, w = 603, 701
    a, b = _case(h, w, 3)
    _check(_run(ctx, a, b, 1, R.Y), _ref(h, w, 3, 1, R.Y), "603x701 y cb 1")


def test_identical_images_give_exactly_0(ctx):
    import _native
    for h, w in ((5, 7), (33, 129), (97, 130)):
        for mode, name, cn in MODES:
            a = _case(h, w, cn)[0]
            rec = _run(ctx, a, a, 0, mode)
            assert rec["sum_d"] == 0.0 and rec["sum_d2"] == 0.0 and _native.gmsd_value(rec) == 0.0, (h, w, name)


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    import _native
    h, w = 97, 130
    a, b = _case(h, w, 3)
    big_a, big_b = _case(603, 701, 3)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for mode, _, cn in MODES[:2]:
            first = ctx.gmsd_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            second = ctx.gmsd_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
            assert _native.gmsd_plan(603, 701, 3)["scratch_bytes"] > _native.gmsd_plan(h, w, 3, 2)["scratch_bytes"]
            big = _run(ctx, big_a, big_b, 0, mode)                          # a larger shape through the scratch
            third = ctx.gmsd_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            assert _bits(first) == _bits(second) == _bits(third), mode
            assert _bits(big) == _bits(_run(ctx, big_a, big_b, 0, mode)), mode
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 53, 67, 3
    a, b = _case(h, w, cn)
    for mode, name, mcn in MODES:
        if mcn != cn:
            continue
        dense = _run(ctx, a, b, cb, mode)
        for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
            la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
            pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
            pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
            try:
                got = ctx.gmsd_u8(ptr_a, sa, ptr_b, sb, h, w, cn, cb, mode)
                # the call only reads: both parents are as they were, inside the views and outside
                ra = V.check_guard(ctx, pa, what="image a")
                rb = V.check_guard(ctx, pb, what="image b")
            finally:
                pa.free(); pb.free()
            assert _bits(got) == _bits(dense), (name, V.layout_id(la), V.layout_id(lb))
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
        for mode, name, _ in MODES[:2]:
            dense = _run(ctx, a, b, cb, mode)
            got = ctx.gmsd_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, cb, mode)
            assert _bits(got) == _bits(dense), name
            _check(got, _ref(h, w, 3, cb, mode), f"wide stride {name}")
    finally:
        wide.free(); da.free(); pb.free()


def test_module_methods(ctx):
    import _native
    import quality_assessment_module as qam
    a, b = _case(53, 67, 3)
    q = qam.QualityAssessmentModule()
    for kw, mode in ((dict(), R.Y), (dict(y_round=True), R.Y_ROUND)):
        want = _native.gmsd_value(_run(ctx, a, b, 3, mode))
        v = q.calculate_gmsd(a, b, crop_border=3, **kw)
        assert isinstance(v, float) and v == want
        assert v == pytest.approx(_ref(53, 67, 3, 3, mode)["score"], rel=TOL, abs=0)
        # the device form on resident images gives the same bits, dense and strided
        da = ctx.upload(a)
        pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
        try:
            assert q.calculate_gmsd_device(da.ptr, a.shape, ptr_b, b.shape, crop_border=3, stride2=sb, **kw) == v
            assert q.calculate_gmsd_device(da.ptr, a.shape, ptr_b, b.shape, crop_border=3, stride1=67 * 3, stride2=sb, **kw) == v
        finally:
            da.free(); pb.free()
    # defaults: the exact luma, no crop; symmetric
    assert q.calculate_gmsd(a, b) == pytest.approx(_ref(53, 67, 3, 0, R.Y)["score"], rel=TOL, abs=0)
    assert q.calculate_gmsd(b, a) == q.calculate_gmsd(a, b)
    assert q.calculate_gmsd(a, a) == 0.0
    # a gray pair: the plane as it is
    ga, gb = _case(53, 67, 1)
    assert q.calculate_gmsd(ga, gb, crop_border=1) == pytest.approx(_ref(53, 67, 1, 1, R.CHANNELS)["score"], rel=TOL, abs=0)


def test_pipeline_note_on_a_tiny_canvas(ctx, rng):
    """The helper all three QA paths of main.py call, as they call it: a canvas below 4 rows gives None and a note; the switch
    alone decides which keys appear (whole runs: tests/test_gpu_vif.py)."""
    import main as sr_main
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_gmsd=True))
    src = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    d_src, d_canvas = ctx.upload(src), ctx.upload(np.ascontiguousarray(np.repeat(np.repeat(src, 2, 0), 2, 1)))
    try:
        rep = {}
        pipe._vif_gmsd(ctx, rep, d_src.ptr, (2, 32, 3), d_canvas.ptr, (3, 64, 3))
        assert sorted(rep) == ["gmsd", "gmsd_note"] and rep["gmsd"] is None and "at least 4" in rep["gmsd_note"]
        rep = {}
        pipe._vif_gmsd(ctx, rep, d_src.ptr, (24, 32, 3), d_canvas.ptr, (48, 64, 3))
        assert sorted(rep) == ["gmsd"] and isinstance(rep["gmsd"], float)
        ref = pipe.quality_module.upsample_bicubic(src, (48, 64))
        canvas = np.ascontiguousarray(np.repeat(np.repeat(src, 2, 0), 2, 1))
        assert rep["gmsd"] == pytest.approx(G.gmsd(ref, canvas)["score"], rel=TOL, abs=0)
    finally:
        d_src.free(); d_canvas.free()
