"""GPU: VIF in the pixel domain over four scales (sr_vif_u8, csrc/sr_vif.hip).

* restatement: every num_s and den_s of every mode against tests/_vif_ref.py (the 2-D window, so the separable kernel is held
  against the unseparated form) at 1e-9 relative, counts equal -- at the smallest sizes (41: one sample at scale 4), odd sizes,
  the parities of H - 8, one shape on each side of every column constant of the kernels (240 map columns per block at scale
  1; 124 decimated columns per block into scale 2; 120, 62, 124, 63, 126 at the float64 scales), several chunks of rows at
  every scale, one multi-block image, crop borders at every alignment and a saturated flat patch;
* values: the metric is not symmetric, identical noise gives 1 within 1e-9, a flat reference gives NaN;
* bits: equal inputs give equal bits, also after the scratch has grown; padded, offset, guarded views (one with rows beyond
  2^32 bytes) give the dense bits and nothing outside is written;
* the module methods, their device twins and the pipeline switches (default off).
* the chunk constants: two tall narrow pairs, 131100 x 41 (chunks of 128, 64, 32 and 16 rows at scales 1 .. 4, each scale at
  or over the 1024-block cut) and 130960 x 41 (one block short at every scale: 64, 32, 16, 16), against the restatement
  evaluated on three periods of a vertically periodic image (R.vifp_tall, held against the direct form on the CPU);
parity: unpinned (MATLAB, piq, pyiqa are not available offline); pinned by the restatement alone."""
import asyncio
import functools
import math

import numpy as np
import pytest

import _vif_ref as R
import _views as V

pytestmark = pytest.mark.gpu

TOL = 1e-9
MODES = ((R.Y, "y", 3), (R.Y_ROUND, "y_round", 3), (R.CHANNELS, "gray", 1))


@functools.lru_cache(maxsize=None)
def _case(h, w, cn=3, flat=None):
    """One image pair per shape, made once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn, flat=flat)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, cb, mode, flat=None):
    a, b = _case(h, w, cn, flat)
    return R.vifp(a, b, cb, mode)


def _run(ctx, a, b, cb=0, mode=R.Y):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.vif_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, crop_border=cb, mode=mode)
    finally:
        da.free(); db.free()


def _bits(rec):
    return [(np.float64(n).view(np.uint64), np.float64(d).view(np.uint64), c) for n, d, c in rec]


def _check(got, want, what):
    assert [c for _, _, c in got] == want["count"], what
    for s, (n, d, _) in enumerate(got):
        wn, wd = want["num"][s], want["den"][s]
        print(f"{what} scale {s + 1}: num {n!r} ref {wn!r} rel {abs(n - wn) / abs(wn):.2e}   den {d!r} ref {wd!r} "
              f"rel {abs(d - wd) / abs(wd):.2e}")
        assert wd > 0 and wn > 0, (what, s)                                  # no scale's sums vanish
        assert n == pytest.approx(wn, rel=TOL, abs=0), (what, s)
        assert d == pytest.approx(wd, rel=TOL, abs=0), (what, s)


# cropped sizes (h, w).  41: one sample at scale 4; 57 x 58: two chunks of rows at scale 2; 97 x 130: three.  Columns, from the
# kernels' constants (csrc/sr_vif.h): 256 | 257 = 240 | 241 map columns at scale 1 and 124 | 125 columns of scale 2;
# 264 | 265 = 120 | 121 map columns at scale 2 and 62 | 63 columns of scale 3; 528 | 529 = 124 | 125 map columns at scale 3 and
# 63 | 64 columns of scale 4; 1048 | 1049 = 126 | 127 map columns at scale 4.
SHAPES = [(41, 41), (41, 57), (42, 43), (57, 58), (64, 64), (97, 130), (41, 256), (42, 257), (43, 264), (41, 265), (42, 528),
          (41, 529), (41, 1048), (43, 1049)]


def test_the_shapes_sit_on_the_kernels_constants():
    import _native
    w = lambda cw: [s[1] for s in _native.vif_plan(41, cw, 3)["sizes"]]
    assert (w(256)[0] - 16, w(257)[0] - 16) == (240, 241) and (w(256)[1], w(257)[1]) == (124, 125)
    assert (w(264)[1] - 8, w(265)[1] - 8) == (120, 121) and (w(264)[2], w(265)[2]) == (62, 63)
    assert (w(528)[2] - 4, w(529)[2] - 4) == (124, 125) and (w(528)[3], w(529)[3]) == (63, 64)
    assert (w(1048)[3] - 2, w(1049)[3] - 2) == (126, 127)


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_modes_match_the_restatement(ctx, h, w):
    for mode, name, cn in MODES:
        a, b = _case(h, w, cn)
        _check(_run(ctx, a, b, 0, mode), _ref(h, w, cn, 0, mode), f"{h}x{w} {name}")


@pytest.mark.parametrize("cb", [0, 1, 2, 3])
def test_crop_borders_at_every_alignment(ctx, cb):
    """53 x 67: odd sides; cb * 3 mod 4 is 0, 3, 2, 1.  The crop on the full image gives the bits of crop_border = 0 on a
    contiguous copy of the crop."""
    h, w = 53, 67
    for mode, name, cn in MODES:
        a, b = _case(h, w, cn)
        got = _run(ctx, a, b, cb, mode)
        _check(got, _ref(h, w, cn, cb, mode), f"cb {cb} {name}")
        ac, bc = np.ascontiguousarray(R.crop(a, cb)), np.ascontiguousarray(R.crop(b, cb))
        assert _bits(_run(ctx, ac, bc, 0, mode)) == _bits(got), (cb, name)
    assert len({_ref(h, w, 3, c, R.Y)["value"] for c in (0, 1, 2, 3)}) == 4      # the crops are told apart


def test_saturated_flat_patch(ctx):
    """A saturated patch wider than the largest window inside a noisy image: s1 and s2 vanish there up to rounding of either
    sign, and the thresholds of the definition take over."""
    h, w, flat = 90, 110, (12, 60, 20, 85)
    for mode, name, cn in MODES:
        a, b = _case(h, w, cn, flat)
        assert a[12:60, 20:85].min() == 255 and b[12:60, 20:85].min() == 255
        _check(_run(ctx, a, b, 0, mode), _ref(h, w, cn, 0, mode, flat), f"flat patch {name}")


def test_multi_block(ctx):
    """603 x 701: three column blocks at scale 1, two and more at the others, dozens of chunks."""
    h, w = 603, 701
    a, b = _case(h, w, 3)
    _check(_run(ctx, a, b, 1, R.Y), _ref(h, w, 3, 1, R.Y), "603x701 y cb 1")


@functools.lru_cache(maxsize=None)
def _tall_blocks(cn):
    """One period (104 rows: a multiple of 8, no divisor of a chunk length) of the tall images."""
    a, b = R.img_pair(np.random.default_rng(104 + cn), 104, 41, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("h", [131100, 130960])
def test_tall_images_walk_every_chunk_length(ctx, h):
    """One column block, so the chunk cut alone decides the block count: 131100 rows take chunks of 128 | 64 | 32 | 16 rows at
    scales 1 | 2 | 3 | 4 (1025, 1025, 1024, 1024 blocks), 130960 rows fall one block short of 1024 at every scale and take
    64 | 32 | 16 | 16 (tools/sanitize/vif_gmsd_driver.cpp pins both cuts).  A period of 104 rows meets the chunk borders at
    every phase; one map row lost or counted twice moves a sum by about 1e-5."""
    for mode, name, cn in (MODES[2], MODES[0]):
        blk_a, blk_b = _tall_blocks(cn)
        a, b = R.tile_rows(blk_a, h), R.tile_rows(blk_b, h)
        _check(_run(ctx, a, b, 0, mode), R.vifp_tall(blk_a, blk_b, h, mode), f"{h}x41 {name}")


def test_asymmetry_identity_and_a_flat_reference(ctx):
    import _native
    a, b = _case(97, 130, 3)
    v_ab, v_ba = _native.vif_value(_run(ctx, a, b)), _native.vif_value(_run(ctx, b, a))
    want = _ref(97, 130, 3, 0, R.Y)["value"]
    assert v_ab == pytest.approx(want, rel=TOL, abs=0) and 0.05 < v_ab < 0.95
    assert v_ba == pytest.approx(R.vifp(b, a)["value"], rel=TOL, abs=0) and abs(v_ab - v_ba) > 1e-5
    noise = np.random.default_rng(4).integers(0, 256, (64, 80, 3), dtype=np.uint8)
    for mode, name, cn in MODES:
        n = noise if cn == 3 else np.ascontiguousarray(noise[..., 0])
        v = _native.vif_value(_run(ctx, n, n, 0, mode))
        print(name, v)
        assert abs(v - 1.0) <= 1e-9, name
    flat = np.full((64, 80, 3), 200, np.uint8)
    rec = _run(ctx, flat, noise)
    assert [d for _, d, _ in rec] == [0.0] * 4 and math.isnan(_native.vif_value(rec))


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    import _native
    h, w = 97, 130
    a, b = _case(h, w, 3)
    big_a, big_b = _case(603, 701, 3)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for mode, _, cn in MODES[:2]:
            first = ctx.vif_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            second = ctx.vif_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
            assert _native.vif_plan(603, 701, 3)["scratch_bytes"] > 16 * _native.vif_plan(h, w, 3, 2)["scratch_bytes"]
            big = _run(ctx, big_a, big_b, 0, mode)                          # a larger shape: the scratch grows, the planes move
            third = ctx.vif_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
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
                got = ctx.vif_u8(ptr_a, sa, ptr_b, sb, h, w, cn, cb, mode)
                # the call only reads: both parents are as they were, inside the views and outside
                ra = V.check_guard(ctx, pa, what="reference")
                rb = V.check_guard(ctx, pb, what="distorted")
            finally:
                pa.free(); pb.free()
            assert _bits(got) == _bits(dense), (name, V.layout_id(la), V.layout_id(lb))
            assert np.array_equal(ra.reshape(a.shape), a) and np.array_equal(rb.reshape(b.shape), b)


def test_rows_beyond_4_gib(ctx):
    """166 rows at a stride of 25 MiB + 5 bytes: rows 164 and 165 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w, cb = 166, 48, 1
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
            got = ctx.vif_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, cb, mode)
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
        rec = _run(ctx, a, b, 3, mode)
        v, scales = q.calculate_vif(a, b, crop_border=3, return_scales=True, **kw)
        assert isinstance(v, float) and _bits(scales) == _bits(rec) and v == _native.vif_value(rec)
        assert q.calculate_vif(a, b, crop_border=3, **kw) == v
        assert v == pytest.approx(_ref(53, 67, 3, 3, mode)["value"], rel=TOL, abs=0)
        # the device form on resident images gives the same bits, dense and strided
        da = ctx.upload(a)
        pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
        try:
            assert q.calculate_vif_device(da.ptr, a.shape, ptr_b, b.shape, crop_border=3, stride2=sb, **kw) == v
            dv, ds = q.calculate_vif_device(da.ptr, a.shape, ptr_b, b.shape, crop_border=3, return_scales=True, stride1=67 * 3,
                                            stride2=sb, **kw)
            assert dv == v and _bits(ds) == _bits(rec)
        finally:
            da.free(); pb.free()
    # defaults: the exact luma, no crop, the first argument is the reference
    assert q.calculate_vif(a, b) == pytest.approx(_ref(53, 67, 3, 0, R.Y)["value"], rel=TOL, abs=0)
    assert q.calculate_vif(b, a) != q.calculate_vif(a, b)
    # a gray pair: the plane as it is
    ga, gb = _case(53, 67, 1)
    assert q.calculate_vif(ga, gb, crop_border=1) == pytest.approx(_ref(53, 67, 1, 1, R.CHANNELS)["value"], rel=TOL, abs=0)
    assert q.calculate_vif(ga[..., None], gb[..., None], crop_border=1) == q.calculate_vif(ga, gb, crop_border=1)


def test_pipeline_switches(ctx, rng, tmp_path):
    import json

    import main as sr_main
    from PIL import Image
    import _gmsd_ref as G
    import _msssim_ref as M
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("vifp", "vifp_scales", "vifp_note", "gmsd", "gmsd_note")
    # default: no key
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # both switches: the device-resident path
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_vif=True, qa_gmsd=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "both" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"]
    assert sorted(set(rep) - set(res0.quality_report)) == ["gmsd", "vifp", "vifp_scales"]
    fused = np.asarray(Image.open(out))
    assert fused.shape == (160, 192, 3)
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (160, 192))
    v, scales = q.calculate_vif(ref_img, fused, return_scales=True)            # the resize is the reference
    assert rep["vifp"] == v and rep["vifp_scales"] == [{"num": n, "den": d, "count": c} for n, d, c in scales]
    assert rep["gmsd"] == q.calculate_gmsd(ref_img, fused)
    assert rep["vifp"] == pytest.approx(R.vifp(ref_img, fused)["value"], rel=TOL, abs=0) and 0.0 < rep["vifp"] < 1.5
    assert rep["gmsd"] == pytest.approx(G.gmsd(ref_img, fused)["score"], rel=TOL, abs=0) and 0.0 < rep["gmsd"] < 0.5
    on_disk = json.load(open(str(tmp_path / "both" / "result_qa_report.json")))
    assert on_disk["vifp"] == rep["vifp"] and on_disk["vifp_scales"] == rep["vifp_scales"] and on_disk["gmsd"] == rep["gmsd"]
    # one switch each on the host-array path: only its keys, the same bits
    for sw, mine in (("qa_vif", ["vifp", "vifp_scales"]), ("qa_gmsd", ["gmsd"])):
        pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(device_resident=False, **{sw: True}, **kw))
        res_h = asyncio.run(pipe_h.process(src, str(tmp_path / sw / "result.png")))
        assert res_h.success, res_h.error_message
        assert sorted(k for k in res_h.quality_report if k in keys) == mine
        assert all(res_h.quality_report[k] == rep[k] for k in mine)
    # A canvas of 40 rows is below VIF's minimum and one of 3 rows below GMSD's: None and a note, no error.  (Stage 4's other
    # metrics need more rows than that, so no whole run gets here; the one helper all three paths call is called as they do.)
    d_src, d_canvas = ctx.upload(np.ascontiguousarray(img[:20, :48])), ctx.upload(np.ascontiguousarray(ref_img[:40, :96]))
    try:
        rep_s = {"kept": 1}
        pipe._vif_gmsd(ctx, rep_s, d_src.ptr, (20, 48, 3), d_canvas.ptr, (40, 96, 3))
        assert rep_s["vifp"] is None and rep_s["vifp_scales"] is None and "at least 41" in rep_s["vifp_note"]
        assert isinstance(rep_s["gmsd"], float) and "gmsd_note" not in rep_s and rep_s["kept"] == 1
        rep_t = {}
        pipe._vif_gmsd(ctx, rep_t, d_src.ptr, (2, 48, 3), d_canvas.ptr, (3, 96, 3))
        assert rep_t == {"vifp": None, "vifp_scales": None, "vifp_note": rep_t["vifp_note"], "gmsd": None, "gmsd_note": rep_t["gmsd_note"]}
        assert "at least 4" in rep_t["gmsd_note"]
        json.dumps(rep_s); json.dumps(rep_t)
    finally:
        d_src.free(); d_canvas.free()
    # a flat source: VIF is 0 / 0 -- None and a note, with the per-scale sums kept
    flat = ctx.upload(np.full((30, 48, 3), 90, np.uint8))
    d_canvas = ctx.upload(np.ascontiguousarray(fused[:60, :96]))
    try:
        rep_f = {}
        pipe._vif_gmsd(ctx, rep_f, flat.ptr, (30, 48, 3), d_canvas.ptr, (60, 96, 3))
        assert rep_f["vifp"] is None and "flat" in rep_f["vifp_note"] and [s["den"] for s in rep_f["vifp_scales"]] == [0.0] * 4
        assert isinstance(rep_f["gmsd"], float)
    finally:
        flat.free(); d_canvas.free()
