"""GPU: MATLAB's bicubic imresize (sr_imresize_u8, csrc/sr_imresize.hip) against the NumPy restatement tests/_imresize_ref.py.

* F64 output at 1e-10 absolute in gray levels: |v| < 300 and at most 132 float64 multiply-adds give an error below 5e-12; the
  bar leaves 20 x for a different but fixed association.  Scales 1/2 .. 1/16, 3/4, 1, 1.5 .. 4, per-axis scales in both pass
  orders, antialiasing off, 1 / 3 / 4 channels, every residue of n mod 4 at 1/4, sizes at the kernel's own tile constants (one
  tile, one output more and one less in each axis, three tiles; the plan says what the tile is), sides shorter than the kernel;
* U8 output byte-equal to the restatement's rounding wherever the restatement is farther than 1e-9 from a half (at most 0.01 %
  of a case's pixels may be left out); F32 equal to np.float32 of the F64 output;
* exact probes: scale 1, constant images, a one-hot pixel against the outer product of the two weight columns, a step image;
* 65536 x the F64 output at scale 1/2 equals NIQE's shipped int32 half plane;
* bits: equal inputs give equal bits; padded, offset, guarded views on source and destination (one source with rows beyond
  2^32 bytes) give the dense bits and nothing outside is written; the table scratch regrows between calls;
* evaluate_sr_network equals the composition of the public methods, and the pipeline's benchmark_degrade switch.
parity: unpinned with MATLAB and BasicSR (neither is available offline); the anchors are in include/sr_hip.h."""
import asyncio
import functools
import json

import numpy as np
import pytest

import _imresize_ref as R
import _native
import _views as V

pytestmark = pytest.mark.gpu

TOL = 1e-10
HALF_EPS = 1e-9
F64, F32, U8 = _native.IMRESIZE_F64, _native.IMRESIZE_F32, _native.IMRESIZE_U8


@functools.lru_cache(maxsize=None)
def _img(h, w, cn=3):
    """One seeded random u8 image per shape, made once and shared (never modified)."""
    shape = (h, w, cn) if cn > 1 else (h, w)
    a = np.random.default_rng(7919 * h + 31 * w + cn).integers(0, 256, shape).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, scale=None, output_shape=None, aa=True):
    v = R.imresize_f64(_img(h, w, cn), scale, output_shape, aa)
    v.setflags(write=False)
    return v


def _run(ctx, img, scale=None, output_shape=None, aa=True, out=F64):
    cn = img.shape[2] if img.ndim == 3 else 1
    h, w = img.shape[:2]
    sy, sx, dh, dw = _native.imresize_geometry(h, w, scale, output_shape)
    dtype = _native.IMRESIZE_DTYPES[out]
    item = np.dtype(dtype).itemsize
    d_src, d_dst = ctx.upload(img), ctx.alloc(dh * dw * cn * item)
    try:
        ctx.imresize(d_src.ptr, w * cn, h, w, cn, sy, sx, d_dst.ptr, dw * cn * item, dh, dw, antialias=aa, out_type=out)
        return ctx.download(d_dst.ptr, (dh, dw, cn) if img.ndim == 3 else (dh, dw), dtype)
    finally:
        d_src.free(); d_dst.free()


def _check_f64(ctx, h, w, cn, scale=None, output_shape=None, aa=True):
    got = _run(ctx, _img(h, w, cn), scale, output_shape, aa)
    want = _ref(h, w, cn, scale, output_shape, aa)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.abs(got - want).max())
    print(f"imresize {h}x{w}x{cn} scale {scale} shape {output_shape} aa {aa}: max err {err:.3e}")
    assert err <= TOL, (h, w, cn, scale, output_shape, aa, err)
    return got


@pytest.mark.parametrize("scale", R.SCALES, ids=[f"{s:.4g}" for s in R.SCALES])
def test_f64_every_scale(ctx, scale):
    _check_f64(ctx, 97, 131, 3, scale)


@pytest.mark.parametrize("cn", [1, 4])
def test_f64_other_channel_counts(ctx, cn):
    for scale in (1 / 2, 1 / 3, 1 / 16, 1.5, 4):
        _check_f64(ctx, 83, 101, cn, scale)


def test_f64_per_axis_scales_in_both_pass_orders(ctx):
    for shape, first in (((40, 100), "vertical"), ((80, 45), "horizontal"), ((150, 60), "horizontal"), ((30, 300), "vertical"),
                         ((97, 40), "horizontal"), ((7, 9), "horizontal")):
        assert _native.imresize_plan(97, 131, 3, shape[0] / 97, shape[1] / 131, shape[0], shape[1])["first"] == first
        _check_f64(ctx, 97, 131, 3, output_shape=shape)
    _check_f64(ctx, 97, 131, 1, output_shape=(80, 45))


def test_f64_antialiasing_off(ctx):
    for scale in (1 / 3, 1 / 4, 3 / 4):
        got = _check_f64(ctx, 97, 131, 3, scale, aa=False)
        # another image than the antialiased one
        assert np.abs(got - _ref(97, 131, 3, scale)).max() > 1.0


def test_f64_every_residue_mod_4(ctx):
    for h, w in ((96, 131), (97, 130), (98, 129), (99, 128)):
        _check_f64(ctx, h, w, 3, 1 / 4)


@pytest.mark.parametrize("scale,cn", [(1 / 2, 3), (1 / 16, 3), (2, 1)], ids=["half-rgb", "sixteenth-rgb", "double-gray"])
def test_f64_at_the_tile_constants(ctx, scale, cn):
    """The plan says which output tile one workgroup owns; the sizes here are exactly one tile, one output more and one less
    in each axis, and three tiles (the input is the output over the scale, so the scalar form gives these sizes)."""
    inv = round(1 / scale) if scale < 1 else None

    def src(n_out):
        return n_out * inv if inv else -(-n_out // int(scale))

    probe = _native.imresize_plan(src(100), src(100), cn, scale, scale, R.out_size(src(100), scale), R.out_size(src(100), scale))
    th, tw = probe["tile"]
    for dh, dw in ((th, tw), (th + 1, tw + 1), (max(th - 1, 1), tw - 1), (3 * th, 3 * tw), (th + 1, tw), (th, tw + 1)):
        h, w = src(dh), src(dw)
        if scale > 1:
            dh, dw = R.out_size(h, scale), R.out_size(w, scale)
        assert _native.imresize_plan(h, w, cn, scale, scale, dh, dw)["tile"] == (th, tw)
        got = _check_f64(ctx, h, w, cn, scale)
        assert got.shape[:2] == (dh, dw)
    # the other pass order: the tile's roles swap
    p = _native.imresize_plan(4 * 40, 2 * 70, cn, 1 / 4, 1 / 2, 40, 70)
    q = _native.imresize_plan(2 * 70, 4 * 40, cn, 1 / 2, 1 / 4, 70, 40)
    assert p["first"] == "vertical" and q["first"] == "horizontal"
    _check_f64(ctx, 160, 140, cn, output_shape=(40, 70))
    _check_f64(ctx, 140, 160, cn, output_shape=(70, 40))


def test_f64_sides_shorter_than_the_kernel(ctx):
    _check_f64(ctx, 5, 7, 3, 1 / 4)
    _check_f64(ctx, 1, 40, 1, 1 / 4)
    _check_f64(ctx, 40, 1, 3, 1 / 4)
    _check_f64(ctx, 1, 1, 4, 1 / 16)
    _check_f64(ctx, 3, 2, 3, 4)


@pytest.mark.parametrize("scale", [1 / 2, 1 / 3, 1 / 4, 1 / 8, 1 / 16, 3 / 4, 2, 3, 4], ids=lambda s: f"{s:.4g}")
def test_u8_and_f32_outputs(ctx, scale):
    """Scale 1.5 is left to the F64 tests: there a phase with dyadic weights on one axis meets thirds on the other, true ties
    come out of inexact arithmetic, and the restatement alone has 9 of 86286 values (0.0104 %) within 1e-9 of a half, more
    than the budget, whatever the kernel does.  At the scales here the restatement leaves out none (measured on the CPU)."""
    img = _img(97, 131, 3)
    want = _ref(97, 131, 3, scale)
    got = _run(ctx, img, scale, out=U8)
    assert got.dtype == np.uint8 and got.shape == want.shape
    # An output whose weights are all dyadic (multiples of 2^-20: products with a byte and sums of at most 32 x 32 of them stay
    # far below 2^53) is computed exactly on both sides, ties included: it is never left out.
    dh, dw = want.shape[:2]
    dyadic = [np.all(np.mod(R.weights(n, m, scale)[0] * 2.0 ** 20, 1.0) == 0.0, axis=1) for n, m in ((97, dh), (131, dw))]
    keep = (R.half_distance(want) > HALF_EPS) | np.outer(dyadic[0], dyadic[1])[:, :, None]
    print(f"imresize u8 scale {scale}: closest to a half {float(R.half_distance(want).min()):.3e}, exact outputs "
          f"{int(np.outer(dyadic[0], dyadic[1]).sum())} of {dh * dw}, left out {int((~keep).sum())} of {keep.size}")
    assert (~keep).sum() <= 1e-4 * keep.size
    assert np.array_equal(got[keep], R.to_u8(want)[keep])
    f64 = _run(ctx, img, scale, out=F64)
    f32 = _run(ctx, img, scale, out=F32)
    assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32))


def test_u8_exact_halves_at_dyadic_scales(ctx):
    """At scale 1/2 every weight is a multiple of 1/256 and every value a multiple of 1/65536: both sides compute exactly, so
    ties round the same way and nothing is left out."""
    img = _img(96, 130, 3)
    want = R.imresize_f64(img, 0.5)
    assert np.array_equal(_run(ctx, img, 0.5, out=F64), want)
    assert np.array_equal(_run(ctx, img, 0.5, out=U8), R.to_u8(want))
    flat = np.full((40, 44), 7, np.uint8)
    flat[::2] = 8                                                                  # rows alternate 7 / 8: the half plane is 7.5
    got = _run(ctx, flat, 0.5, out=U8)
    assert np.all(_run(ctx, flat, 0.5, out=F64)[2:-2] == 7.5) and np.all(got[2:-2] == 8)


def test_scale_one_returns_the_input(ctx):
    for cn in (1, 3, 4):
        img = _img(37, 53, cn)
        assert np.array_equal(_run(ctx, img, 1, out=U8), img)
        assert np.array_equal(_run(ctx, img, 1.0, out=F64), img.astype(np.float64))


def test_constant_images_stay_constant(ctx):
    for value in (0, 255):
        img = np.full((45, 61, 3), value, np.uint8)
        for scale in R.SCALES:
            got = _run(ctx, img, scale, out=U8)
            assert got.shape[:2] == (R.out_size(45, scale), R.out_size(61, scale))
            assert np.all(got == value), (value, scale)
            assert np.abs(_run(ctx, img, scale, out=F64) - value).max() <= TOL


def test_one_hot_pixel_is_the_outer_product_of_the_weight_columns(ctx):
    h, w = 41, 57
    for scale in (1 / 2, 1 / 3, 1 / 8, 1.5, 3):
        dh, dw = R.out_size(h, scale), R.out_size(w, scale)
        wy, iy = _native.imresize_weights(h, dh, scale)
        wx, ix = _native.imresize_weights(w, dw, scale)
        for py, px in ((20, 30), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (1, w - 2)):
            img = np.zeros((h, w), np.uint8)
            img[py, px] = 255
            col_y = np.zeros(dh)
            for k in range(wy.shape[1]):                                          # ascending taps, as the kernel adds them
                col_y = col_y + np.where(iy[:, k] == py, wy[:, k], 0.0)
            col_x = np.zeros(dw)
            for k in range(wx.shape[1]):
                col_x = col_x + np.where(ix[:, k] == px, wx[:, k], 0.0)
            got = _run(ctx, img, scale)
            err = np.abs(got - 255.0 * np.outer(col_y, col_x)).max()
            assert err <= TOL, (scale, py, px, err)
            assert np.abs(got - R.imresize_f64(img, scale)).max() <= TOL


def test_step_image_saturates(ctx):
    img = np.zeros((48, 64, 3), np.uint8)
    img[:, 32:] = 255
    img[24:, :, 1] = 255 - img[24:, :, 1]
    for scale in (1 / 2, 1 / 3, 2, 3):
        f64 = _run(ctx, img, scale)
        u8 = _run(ctx, img, scale, out=U8)
        assert f64.min() < -1.0 and f64.max() > 256.0                              # the kernel's lobes overshoot a step
        assert np.all(u8[f64 <= 0.0] == 0) and np.all(u8[f64 >= 255.0] == 255)
        assert np.array_equal(u8, R.to_u8(f64))
        assert np.array_equal(_run(ctx, img, scale, out=F32), f64.astype(np.float32))   # not clamped


def test_half_scale_is_the_half_plane_of_niqe(ctx):
    plane = _img(96, 192, 1)
    d = ctx.upload(plane)
    try:
        ctx.niqe_u8(d.ptr, 192, 96, 192, 1)
        half = ctx.niqe_half_plane((48, 96))
    finally:
        d.free()
    got = _run(ctx, plane, 0.5)
    assert np.array_equal(65536.0 * got, half.astype(np.float64))


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    small, large = _img(20, 24, 3), _img(97, 131, 3)
    first = _run(ctx, small, 0.5)
    big = _run(ctx, large, 4)                                                      # far larger tables: the scratch regrows
    assert _native.imresize_plan(97, 131, 3, 4, 4, 388, 524)["scratch_bytes"] > 4 * _native.imresize_plan(20, 24, 3, .5, .5, 10, 12)["scratch_bytes"]
    second = _run(ctx, small, 0.5)
    assert first.tobytes() == second.tobytes() == R.imresize_f64(small, 0.5).tobytes()
    assert big.tobytes() == _run(ctx, large, 4).tobytes()
    d = ctx.upload(large)
    try:
        ctx.assess_u8(d.ptr, 131 * 3, d.ptr, 131 * 3, 97, 131, 3)                  # unrelated work on the same stream
    finally:
        d.free()
    assert _run(ctx, large, 1 / 3, out=U8).tobytes() == _run(ctx, large, 1 / 3, out=U8).tobytes()


@pytest.mark.parametrize("out,layouts", [(U8, V.LAYOUTS_U8), (F32, V.LAYOUTS_F32), (F64, [(0, 0), (8, 16), (16, 64), (24, 8)])],
                         ids=["u8", "f32", "f64"])
def test_strided_guarded_views_give_the_dense_bits(ctx, out, layouts):
    dtype = _native.IMRESIZE_DTYPES[out]
    item = np.dtype(dtype).itemsize
    for cn, (h, w), kw in ((3, (61, 83), dict(scale=1 / 3)), (1, (61, 83), dict(output_shape=(70, 40))), (4, (33, 47), dict(scale=2))):
        img = _img(h, w, cn)
        dense = _run(ctx, img, out=out, **kw)
        sy, sx, dh, dw = _native.imresize_geometry(h, w, kw.get("scale"), kw.get("output_shape"))
        for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (5, V.FILLS[0])):
            ls, ld = V.pick(V.LAYOUTS_U8, k), V.pick(layouts, k + 1)
            ps, ptr_s, ss = V.embed(ctx, img, ls[0], ls[1], fill)
            pd, ptr_d, sd = V.out_view(ctx, dh, dw * cn * item, ld[0], ld[1], fill ^ 0xFF)
            try:
                ctx.imresize(ptr_s, ss, h, w, cn, sy, sx, ptr_d, sd, dh, dw, out_type=out)
                got = V.check_guard(ctx, pd, dtype=dtype, shape=dense.shape, what="destination")
                back = V.check_guard(ctx, ps, what="source")
            finally:
                ps.free(); pd.free()
            assert got.tobytes() == dense.tobytes(), (cn, kw, V.layout_id(ls), V.layout_id(ld))
            assert np.array_equal(back.reshape(img.shape), img)


def test_source_rows_beyond_4_gib(ctx):
    """166 rows at a stride of 25 MiB + 5 bytes: rows 164 and 165 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w = 166, 40
    img = _img(h, w, 3)
    stride = (25 << 20) + 5
    assert (h - 2) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    assert total < 8 << 30
    wide, d_img = ctx.alloc(total), ctx.upload(img)
    pd, ptr_d, sd = V.out_view(ctx, 83, 20 * 3 * 8, 8, 16, V.FILLS[1])
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, d_img.ptr + r * w * 3, w * 3)
        ctx.sync()
        ctx.imresize(wide.ptr + V.GUARD, stride, h, w, 3, 0.5, 0.5, ptr_d, sd, 83, 20, out_type=F64)
        got = V.check_guard(ctx, pd, dtype=np.float64, shape=(83, 20, 3), what="destination")
    finally:
        wide.free(); d_img.free(); pd.free()
    assert got.tobytes() == _run(ctx, img, 0.5).tobytes()
    assert np.abs(got - _ref(h, w, 3, 0.5)).max() <= TOL
    # the last output rows read the rows beyond 2^32 bytes
    assert np.abs(got[-1] - _ref(h, w, 3, 0.5)[-1]).max() <= TOL and got[-1].std() > 1.0


def test_module_methods(ctx):
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    img = _img(61, 83, 3)
    assert np.array_equal(q.imresize(img, 1 / 3), _run(ctx, img, 1 / 3, out=U8))
    assert np.array_equal(q.imresize(img, output_shape=(70, 40), dtype=np.float64), _run(ctx, img, output_shape=(70, 40)))
    assert np.array_equal(q.imresize(img, 2, antialiasing=False, dtype=np.float32), _run(ctx, img, 2, aa=False, out=F32))
    gray = _img(61, 83, 1)
    assert q.imresize(gray, 0.5).shape == (31, 42)
    # not the INTER_CUBIC resize that keeps the name downsample_bicubic
    assert not np.array_equal(q.imresize(img, 0.5)[:30, :41], q.downsample_bicubic(img, 0.5)[:30, :41])
    # the device form, on a view: the mod-crop of a resident image is its address with the full stride
    crop = qam.mod_crop(img, 4)
    d_src, d_dst = ctx.upload(img), ctx.alloc(15 * 20 * 3)
    try:
        shape = q.imresize_device(d_src.ptr, crop.shape, d_dst.ptr, scale=1 / 4, src_stride=83 * 3)
        got = ctx.download(d_dst.ptr, shape, np.uint8)
    finally:
        d_src.free(); d_dst.free()
    assert shape == (15, 20, 3) and np.array_equal(got, q.imresize(np.ascontiguousarray(crop), 1 / 4))


def test_evaluate_sr_network_is_the_composition_of_the_public_methods(ctx):
    import quality_assessment_module as qam
    import sr_network
    import _srnet_ref as ref
    q = qam.QualityAssessmentModule()
    net = sr_network.CompactSRNet(ref.synthetic_state(64, 1, 2))
    try:
        hr = _img(45, 62, 3)                                                       # 45 is odd: the mod-crop drops a row
        got = q.evaluate_sr_network(net, hr, return_sr=True)
        crop = np.ascontiguousarray(qam.mod_crop(hr, 2))
        lr = q.imresize(crop, 1 / 2)
        sr = net.upscale(lr)
        y = q.evaluate_sr_benchmark(sr, crop, crop_border=2)
        rgb = q.evaluate_sr_benchmark(sr, crop, crop_border=2, test_y_channel=False)
        assert np.array_equal(got.pop("sr"), sr)
        assert got == {"psnr_y": y["psnr"], "ssim_y": y["ssim"], "psnr_rgb": rgb["psnr"], "ssim_rgb": rgb["ssim"], "crop_border": 2,
                       "scale": 2, "hr_shape": (44, 62, 3), "lr_shape": (22, 31, 3)}
        # the options reach the parts: another border, MATLAB's rounded luma, the ensemble
        opt = q.evaluate_sr_network(net, hr, crop_border=5, ensemble=2, y_round=True)
        sr2 = net.upscale(lr, ensemble=2)
        y2 = q.evaluate_sr_benchmark(sr2, crop, crop_border=5, y_round=True)
        assert "sr" not in opt and (opt["psnr_y"], opt["ssim_y"], opt["crop_border"]) == (y2["psnr"], y2["ssim"], 5)
        with pytest.raises(ValueError):
            q.evaluate_sr_network(net, hr[:, :, 0])
        with pytest.raises(ValueError):
            q.evaluate_sr_network(net, hr[:20, :20], crop_border=5)                # 10 x 10 after the crop: below the window
    finally:
        net.close()


def _pipeline_case(tmp_path, h, w, scale_factors):
    """One ground-truth run against a plain run on the low-resolution image.  scale_factors: the downsample comparison of the
    full-reference section (ScaleConfig), None for the default; both runs get the same."""
    import main as sr_main
    import quality_assessment_module as qam
    from PIL import Image
    import _msssim_ref as M
    hr = M.base_image(np.random.default_rng(1000 * h + w), h, w, 3)
    src = str(tmp_path / "hr.png")
    Image.fromarray(hr).save(src)
    kw = dict(block_size=32, overlap_ratio=0.25, sr_scale=2, num_pyramid_levels=3)

    def make(**extra):
        p = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**extra, **kw))
        p.tiling_module.l2_cache_dir = tmp_path
        if scale_factors is not None:
            p.quality_module.scale_config = qam.ScaleConfig(scale_factors=list(scale_factors))
        return p

    pipe = make(benchmark_degrade=True)
    out = str(tmp_path / "degrade" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert "degrade" in pipe.stage_times and "benchmark_hr_note" not in rep
    # the canvas against the mod-cropped ground truth
    q = pipe.quality_module
    fused = np.asarray(Image.open(out))
    crop = np.ascontiguousarray(qam.mod_crop(hr, 2))
    H, W = h - h % 2, w - w % 2
    assert fused.shape == crop.shape == (H, W, 3)
    y = q.evaluate_sr_benchmark(fused, crop, crop_border=2)
    rgb = q.evaluate_sr_benchmark(fused, crop, crop_border=2, test_y_channel=False)
    assert rep["benchmark_hr"] == {"psnr_y": y["psnr"], "ssim_y": y["ssim"], "psnr_rgb": rgb["psnr"], "ssim_rgb": rgb["ssim"],
                                   "crop_border": 2, "scale": 2, "hr_shape": [H, W, 3], "lr_shape": [H // 2, W // 2, 3]}
    assert rep["benchmark_hr"]["psnr_y"] > 15.0 and 0.0 < rep["benchmark_hr"]["ssim_y"] <= 1.0
    assert json.load(open(str(tmp_path / "degrade" / "result_qa_report.json")))["benchmark_hr"] == rep["benchmark_hr"]
    # every other key is that of a plain run on the low-resolution image
    lr = q.imresize(crop, 1 / 2)
    lr_path = str(tmp_path / "lr.png")
    Image.fromarray(lr).save(lr_path)
    plain = make()
    out0 = str(tmp_path / "plain" / "result.png")
    res0 = asyncio.run(plain.process(lr_path, out0))
    assert res0.success, res0.error_message
    rep0 = res0.quality_report
    assert "benchmark_hr" not in rep0 and "degrade" not in plain.stage_times      # default off
    assert sorted(set(rep) - set(rep0)) == ["benchmark_hr"]
    for key in rep0:
        if key != "timestamp":
            assert rep[key] == rep0[key], key
    assert np.array_equal(np.asarray(Image.open(out0)), fused)
    assert (res.total_blocks, res.quality_score) == (res0.total_blocks, res0.quality_score)
    return pipe, hr


def test_pipeline_benchmark_degrade(ctx, tmp_path):
    """The stub backend on a 97 x 130 PNG at sr_scale 2.  Its low-resolution image is 48 x 65, and the full-reference section's
    default downsample comparison at 0.1 would compare 4 x 6 images, below its 7-tap window, in the plain run as well: both
    runs compare at 0.2 and 0.4 instead.  test_pipeline_benchmark_degrade_default_scales runs a size the defaults take."""
    pipe, hr = _pipeline_case(tmp_path, 97, 130, (0.2, 0.4))
    # A 12 x 12 ground truth leaves 8 x 8 after the crop, below the SSIM window: None and a note, no error.  (Stage 4's other
    # metrics need far more than 12 rows, so no whole run gets here; the helper is called as the pipeline calls it.)
    tiny = np.ascontiguousarray(hr[:12, :12])
    d_hr, stride, shape, lr_tiny = pipe._degrade(ctx, tiny)
    d_canvas = ctx.upload(tiny)
    try:
        assert (stride, shape, lr_tiny.shape) == (36, (12, 12, 3), (6, 6, 3))
        rep_s = {"kept": 1}
        pipe._benchmark_hr(ctx, rep_s, d_hr.ptr, stride, d_canvas.ptr, (12, 12, 3), lr_tiny.shape)
    finally:
        d_hr.free(); d_canvas.free()
    assert rep_s["benchmark_hr"] is None and "at least 11" in rep_s["benchmark_hr_note"] and rep_s["kept"] == 1
    json.dumps(rep_s)


def test_pipeline_benchmark_degrade_default_scales(tmp_path):
    _pipeline_case(tmp_path, 161, 150, None)
