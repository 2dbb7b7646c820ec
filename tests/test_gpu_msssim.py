"""GPU: multi-scale SSIM (sr_ms_ssim_u8, csrc/sr_msssim.hip).

* restatement: every per-level S_j, CS_j and the value against tests/_msssim_ref.py at 1e-9 (relative: the bar the suite holds
  for SSIM sums), on inputs that separate the levels (asserted on the restatement's own numbers);
* scikit-image: L = 1 against the three *_ssim_gauss fixtures and sr_ssim_u8 mode 'gauss', S_j against msssim_skimage.npz;
* identical images give 1, b = 255 - a gives exactly 0.0;
* the pooled planes are bit-equal to the exact integer sums;
* reproducibility: equal inputs give equal bits; strided, offset, guarded views (one with rows beyond 2^32 bytes) too;
* the module methods and the pipeline hook (default off).
parity: S_j pinned by scikit-image 0.18.3 on exactly pooled planes; CS_j and the value rest on the restatement (scikit-image
does not expose cs); pytorch-msssim / TensorFlow parity is unpinned."""
import asyncio
import functools
import os

import numpy as np
import pytest

import _msssim_ref as R
import _views as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _case(h, w, cn):
    """One image pair per shape, made once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, levels=5, data_range=255.0, shift=15):
    a, b = _case(h, w, cn)
    return R.ms_ssim(a, b, levels=levels, data_range=data_range, shift=shift)


def _run(ctx, a, b, levels=5, **kw):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.ms_ssim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, levels=levels, **kw)
    finally:
        da.free(); db.free()


def _check(recs, want, what, weights=None):
    import _native
    v, s, cs = want
    assert len(recs) == len(s)
    gs, gcs = [r[0] / r[2] for r in recs], [r[1] / r[2] for r in recs]
    gv = _native.ms_ssim_value(recs, weights)
    for j in range(len(s)):
        print(f"{what} level {j}: S {gs[j]!r} ref {s[j]!r} rel {abs(gs[j] - s[j]) / abs(s[j]):.2e}   "
              f"CS {gcs[j]!r} ref {cs[j]!r} rel {abs(gcs[j] - cs[j]) / abs(cs[j]):.2e}")
    print(f"{what} value {gv!r} ref {v!r}")
    for j in range(len(s)):
        assert gs[j] == pytest.approx(s[j], rel=TOL, abs=0), (what, "S", j)
        assert gcs[j] == pytest.approx(cs[j], rel=TOL, abs=0), (what, "CS", j)
    assert gv == pytest.approx(v, rel=TOL, abs=0), what


def _separates(s, cs):
    """The inputs must keep telling the levels, and S from CS, apart."""
    assert all(1 - c >= 0.05 for c in cs), cs
    assert all(abs(x - y) >= 1e-5 for x, y in zip(s, cs)), (s, cs)


# 176 x 176: level 4 is 11 x 11, one sample.  177 x 191: odd sides at levels 0-3.  300 x 600 x 3: more than one block wide and
# more than one chunk tall at level 0, and a block edge inside level 1.
SHAPES = [(176, 176, 1), (177, 191, 1), (177, 191, 3), (191, 353, 1), (300, 600, 3)]


@pytest.mark.parametrize("h,w,cn", SHAPES, ids=[f"{h}x{w}x{cn}" for h, w, cn in SHAPES])
def test_levels_match_the_restatement(ctx, h, w, cn):
    import _native
    a, b = _case(h, w, cn)
    want = _ref(h, w, cn)
    _separates(want[1], want[2])
    recs = _run(ctx, a, b)
    assert [r[2] for r in recs] == _native.ms_ssim_plan(h, w, 5)["counts"] == R.plan(h, w, 5)[1]
    _check(recs, want, f"{h}x{w}x{cn}")
    if (h, w) == (176, 176):
        assert recs[4][2] == 1


@pytest.mark.parametrize("shift,data_range", [(14, 255.0), (15, 200.0), (14, 200.0)])
def test_gray_shift_and_data_range(ctx, shift, data_range):
    a, b = _case(177, 191, 3)
    want = _ref(177, 191, 3, 5, data_range, shift)
    base = _ref(177, 191, 3)
    assert want[0] != base[0]
    _check(_run(ctx, a, b, gray_shift=shift, data_range=data_range), want, f"shift {shift} range {data_range}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_level_counts_with_their_own_weights(ctx, levels):
    a, b = _case(191, 353, 1)
    wt = (0.7, 0.15, 0.4, 0.05, 0.3)[:levels]
    v, s, cs = _ref(191, 353, 1, levels)
    _check(_run(ctx, a, b, levels=levels), (R.value(s, cs, wt), s, cs), f"{levels} levels", weights=wt)
    # fewer levels see the same first levels
    full = _ref(191, 353, 1)
    assert s == full[1][:levels] and cs == full[2][:levels]


def test_one_level_is_the_skimage_gaussian_ssim(ctx):
    import _native
    z = np.load(os.path.join(GOLD, "metrics_skimage.npz"))
    for name in z["cases"]:
        a, b = np.ascontiguousarray(z[f"{name}_a"][..., 1]), np.ascontiguousarray(z[f"{name}_b"][..., 1])
        h, w = a.shape
        da, db = ctx.upload(a), ctx.upload(b)
        try:
            recs = ctx.ms_ssim_u8(da.ptr, w, db.ptr, w, h, w, 1, levels=1)
            s1, n1 = ctx.ssim_u8(da.ptr, w, db.ptr, w, h, w, 1, "gauss")
        finally:
            da.free(); db.free()
        v = _native.ms_ssim_value(recs, (1.0,))
        want = float(z[f"{name}_ssim_gauss"])
        print(name, v, want, s1 / n1)
        assert recs[0][2] == n1
        assert v == recs[0][0] / recs[0][2]
        assert v == pytest.approx(want, rel=TOL, abs=0)
        assert v == pytest.approx(s1 / n1, rel=TOL, abs=0)


def test_levels_match_skimage_on_the_pooled_planes(ctx):
    z = np.load(os.path.join(GOLD, "msssim_skimage.npz"))
    recs = _run(ctx, z["a"], z["b"])
    for j in range(5):
        got = recs[j][0] / recs[j][2]
        print("level", j, got, float(z["s"][j]))
        assert got == pytest.approx(float(z["s"][j]), rel=TOL, abs=0), j


def test_identical_images_give_one(ctx):
    import _native
    for h, w, cn in ((177, 191, 3), (300, 600, 3)):
        a = _case(h, w, cn)[0]
        recs = _run(ctx, a, a)
        for j, r in enumerate(recs):
            assert r[0] / r[2] == pytest.approx(1.0, abs=1e-12), j
            assert r[1] / r[2] == pytest.approx(1.0, abs=1e-12), j
        assert _native.ms_ssim_value(recs) == pytest.approx(1.0, abs=1e-12)


def test_inverted_image_gives_exactly_zero(ctx):
    import _native
    a = _case(177, 191, 1)[0]
    b = (255 - a).astype(np.uint8)
    v, s, cs = R.ms_ssim(a, b)
    assert v == 0.0 and min(cs[:4]) < 0
    recs = _run(ctx, a, b)
    assert _native.ms_ssim_value(recs) == 0.0
    for j in range(5):
        print("level", j, recs[j][0] / recs[j][2], s[j], recs[j][1] / recs[j][2], cs[j])
        assert recs[j][0] / recs[j][2] == pytest.approx(s[j], rel=TOL, abs=0), j
        assert recs[j][1] / recs[j][2] == pytest.approx(cs[j], rel=TOL, abs=0), j
    assert any(r[1] < 0 for r in recs[:4])


@pytest.mark.parametrize("h,w,cn", [(177, 191, 1), (300, 600, 3)])
def test_pooled_planes_are_the_exact_sums(ctx, h, w, cn):
    import _native
    a, b = _case(h, w, cn)
    sa, sb = R.pool_sums(R.gray_u8(a), 5), R.pool_sums(R.gray_u8(b), 5)
    sizes = _native.ms_ssim_plan(h, w, 5)["sizes"]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        ctx.ms_ssim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn)
        for level in range(1, 5):
            x, y = ctx.ms_ssim_planes(level, sizes[level])
            assert x.dtype == np.uint16 and x.shape == sa[level].shape
            assert np.array_equal(x.astype(np.int64), sa[level]), level
            assert np.array_equal(y.astype(np.int64), sb[level]), level
        with pytest.raises(ValueError):
            ctx.ms_ssim_planes(0, sizes[0])
        with pytest.raises(ValueError):
            ctx.ms_ssim_planes(5, sizes[4])
        # a call with fewer levels keeps only its own planes
        ctx.ms_ssim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, levels=2)
        x, _ = ctx.ms_ssim_planes(1, sizes[1])
        assert np.array_equal(x.astype(np.int64), sa[1])
        with pytest.raises(ValueError):
            ctx.ms_ssim_planes(2, sizes[2])
    finally:
        da.free(); db.free()


def test_equal_inputs_give_equal_bits(ctx):
    a, b = _case(300, 600, 3)
    h, w = 300, 600
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        first = ctx.ms_ssim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        second = ctx.ms_ssim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream and scratch
        ctx.ms_ssim_u8(db.ptr, w * 3, da.ptr, w * 3, 200, 500, 3, levels=3, data_range=100.0)
        tmp = ctx.alloc(200 * 300 * 3)
        ctx.resize_cubic_u8(da.ptr, w * 3, h, w, 3, tmp.ptr, 300 * 3, 200, 300)
        third = ctx.ms_ssim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        tmp.free()
    finally:
        da.free(); db.free()
    bits = lambda recs: [(np.float64(r[0]).view(np.uint64), np.float64(r[1]).view(np.uint64), r[2]) for r in recs]
    assert bits(first) == bits(second) == bits(third)


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    a, b = _case(177, 191, cn)
    dense = _run(ctx, a, b)
    for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
        la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
        pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
        pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
        try:
            got = ctx.ms_ssim_u8(ptr_a, sa, ptr_b, sb, 177, 191, cn)
        finally:
            pa.free(); pb.free()
        assert got == dense, (V.layout_id(la), V.layout_id(lb))


def test_rows_beyond_4_gib(ctx):
    """176 rows at a stride of 25 MiB + 5 bytes: rows 164 .. 175 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w = 176, 180
    a, b = _case(h, w, 3)
    dense = _run(ctx, a, b)
    stride = (25 << 20) + 5
    assert (h - 1) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    assert total < 8 << 30
    wide = ctx.alloc(total)
    da = ctx.upload(a)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 2, V.FILLS[1])
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, da.ptr + r * w * 3, w * 3)
        ctx.sync()
        got = ctx.ms_ssim_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3)
        swapped = ctx.ms_ssim_u8(ptr_b, sb, wide.ptr + V.GUARD, stride, h, w, 3)
    finally:
        wide.free(); da.free(); pb.free()
    assert got == dense
    # SSIM is symmetric in its two images up to the order of a few products
    for g, d in zip(swapped, dense):
        assert g[0] == pytest.approx(d[0], rel=1e-12) and g[1] == pytest.approx(d[1], rel=1e-12)


def test_module_methods(ctx):
    import quality_assessment_module as qam
    a, b = _case(300, 600, 3)
    want = _ref(300, 600, 3)
    q = qam.QualityAssessmentModule()
    v = q.calculate_ms_ssim(a, b)
    assert isinstance(v, float) and v == pytest.approx(want[0], rel=TOL, abs=0)
    v2, lv = q.calculate_ms_ssim(a, b, return_levels=True)
    assert v2 == v and lv["weights"] == list(R.WEIGHTS)
    assert lv["s"] == pytest.approx(want[1], rel=TOL, abs=0) and lv["cs"] == pytest.approx(want[2], rel=TOL, abs=0)
    # levels, weights and data_range reach the kernel
    wt = (0.2, 0.3, 0.5)
    r3 = R.ms_ssim(a, b, levels=3, weights=wt, data_range=200.0)
    assert q.calculate_ms_ssim(a, b, data_range=200.0, levels=3, weights=wt) == pytest.approx(r3[0], rel=TOL, abs=0)
    # the device form on resident images gives the same bits
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        d, dlv = q.calculate_ms_ssim_device(da.ptr, a.shape, db.ptr, b.shape, return_levels=True)
    finally:
        da.free(); db.free()
    assert d == v and dlv == lv
    # differently sized inputs: the common top-left rectangle, like calculate_ssim
    a2, b2 = a[:250, :400], b[:280, :380]
    ac, bc = np.ascontiguousarray(a[:250, :380]), np.ascontiguousarray(b[:250, :380])
    assert q.calculate_ms_ssim(a2, b2) == q.calculate_ms_ssim(ac, bc)
    # gray_shift follows the module; the single-scale keys are untouched by all this
    q14 = qam.QualityAssessmentModule(gray_shift=14)
    assert q14.calculate_ms_ssim(a, b) == pytest.approx(R.ms_ssim(a, b, shift=14)[0], rel=TOL, abs=0)
    full = q.evaluate_full_reference(a, b)
    assert full["ms_ssim"] == pytest.approx(q.calculate_ssim(a, b, multiscale=True), rel=1e-12) and "ms_ssim_5scale" not in full
    assert abs(full["ms_ssim"] - v) > 1e-3


def test_pipeline_hook(rng, tmp_path):
    import json

    import main as sr_main
    from PIL import Image
    img = R.base_image(rng, 200, 300, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=128, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("ms_ssim_5scale", "ms_ssim_5scale_levels", "ms_ssim_5scale_note")
    # default: no key
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # with the option: the device-resident path
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_ms_ssim=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "ms" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"] and "ms_ssim_5scale_note" not in rep
    fused = np.asarray(Image.open(out))
    assert fused.shape == (400, 600, 3)
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (400, 600))
    v, lv = q.calculate_ms_ssim(ref_img, fused, return_levels=True)
    assert rep["ms_ssim_5scale"] == v and rep["ms_ssim_5scale_levels"] == lv
    rv, rs, rcs = R.ms_ssim(ref_img, fused)
    assert v == pytest.approx(rv, rel=TOL, abs=0) and lv["s"] == pytest.approx(rs, rel=TOL, abs=0)
    assert 0.0 < v < 1.0
    on_disk = json.load(open(str(tmp_path / "ms" / "result_qa_report.json")))
    assert on_disk["ms_ssim_5scale"] == v and on_disk["ms_ssim_5scale_levels"] == lv
    # the host-array path agrees bit for bit
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_ms_ssim=True, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report["ms_ssim_5scale"] == v and res_h.quality_report["ms_ssim_5scale_levels"] == lv
    # a canvas below 176 on a side: None and a note, the run succeeds
    small = str(tmp_path / "small.png")
    Image.fromarray(img[:80, :96]).save(small)
    for resident in (True, False):
        pipe_s = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(block_size=64, sr_scale=2, num_pyramid_levels=4, qa_ms_ssim=True,
                                                                        device_resident=resident))
        pipe_s.tiling_module.l2_cache_dir = tmp_path
        res_s = asyncio.run(pipe_s.process(small, str(tmp_path / f"small{int(resident)}" / "result.png")))
        assert res_s.success, res_s.error_message
        rep_s = res_s.quality_report
        assert rep_s["ms_ssim_5scale"] is None and rep_s["ms_ssim_5scale_levels"] is None
        assert "at least 176" in rep_s["ms_ssim_5scale_note"]
