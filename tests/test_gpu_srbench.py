"""GPU: the SR-benchmark PSNR / SSIM (sr_bench_u8, csrc/sr_srbench.hip).

* restatement: every mode against tests/_srbench_ref.py -- the SSIM mean at 1e-9 (relative: the bar the suite holds for SSIM
  sums), sse equal as an integer in CHANNELS / Y_ROUND and at 1e-12 in Y (every thread's sum is an exact integer; only the
  fp64 additions of the block tree and of the partials round, log2(n) * 2^-53 each way) -- at the shapes where the
  ownership of map columns, map rows and squared differences can go wrong (from the kernel's constants: 246 map columns per
  block, chunks of 16 map rows in a small image), and with crop borders that put crop_border * cn at every residue mod 4;
* scikit-image: all six values of tests/golden/srbench_skimage.npz at both crop borders at 1e-9;
* values: identical images, a gray image through Y_ROUND, the crop against a contiguous copy of the crop;
* bits: equal inputs give equal bits; padded, offset, guarded views (one with rows beyond 2^32 bytes) give the dense bits and
  nothing outside is written;
* the module methods and the pipeline hook (default off).
parity: pinned by scikit-image 0.18.3 and the restatement; BasicSR parity is unpinned (its float32 Y moves PSNR by ~1e-6 dB
and SSIM by ~1e-8)."""
import asyncio
import functools
import math
import os

import numpy as np
import pytest

import _srbench_ref as R
import _views as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-9
SSE_TOL_Y = 1e-12
MODES = ((R.Y, "y"), (R.Y_ROUND, "y_round"), (R.CHANNELS, "channels"))


@functools.lru_cache(maxsize=None)
def _case(h, w, cn=3):
    """One image pair per shape, made once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn, cb, mode, data_range=255.0):
    a, b = _case(h, w, cn)
    return R.bench(a, b, cb, mode, data_range)


def _run(ctx, a, b, cb=0, mode=R.Y, **kw):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.bench_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, crop_border=cb, mode=mode, **kw)
    finally:
        da.free(); db.free()


def _bits(rec):
    return (np.float64(rec["sse"]).view(np.uint64), np.float64(rec["ssim_sum"]).view(np.uint64), rec["n_elems"], rec["n_map"])


def _check(got, want, mode, what):
    g_ssim, w_ssim = got["ssim_sum"] / got["n_map"], want["ssim"]
    print(f"{what}: ssim {g_ssim!r} ref {w_ssim!r} rel {abs(g_ssim - w_ssim) / abs(w_ssim):.2e}   sse {got['sse']!r} ref "
          f"{want['sse']!r} rel {abs(got['sse'] - want['sse']) / max(abs(want['sse']), 1e-300):.2e}")
    assert (got["n_elems"], got["n_map"]) == (want["n_elems"], want["n_map"]), what
    assert g_ssim == pytest.approx(w_ssim, rel=TOL, abs=0), what
    if mode == R.Y:
        assert got["sse"] == pytest.approx(want["sse"], rel=SSE_TOL_Y, abs=0), what
    else:
        assert got["sse"] == float(want["sse"]) and int(got["sse"]) == want["sse_int"], what


# cropped sizes (h, w).  Columns: 11 = one map column; 256 = exactly one column block (246 map columns), 257 and 258 one and
# two columns more; 521 = three blocks.  Rows: 11 = one map row; 26 = exactly one chunk (16 map rows), 27 one row more (two
# chunks of 9 and 8); 45 = three chunks.
SHAPES = [(11, 11), (37, 11), (11, 300), (26, 256), (27, 257), (26, 258), (45, 521)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_modes_match_the_restatement(ctx, h, w):
    assert R.blocks(26, 256) == (1, 1) and R.blocks(27, 257) == (2, 2) and R.blocks(26, 258) == (1, 2) and R.blocks(45, 521) == (3, 3)
    for cn, modes in ((3, MODES), (1, MODES[2:])):
        a, b = _case(h, w, cn)
        for mode, name in modes:
            want = _ref(h, w, cn, 0, mode)
            assert 0.05 < want["ssim"] < 0.95 and want["sse_int"] > 100 * h * w, (name, want)
            _check(_run(ctx, a, b, 0, mode), want, mode, f"{h}x{w}x{cn} {name}")


@pytest.mark.parametrize("cb", [0, 1, 3, 4])
def test_crop_borders_at_every_alignment(ctx, cb):
    """61 x 83: odd sides; cb * 3 mod 4 is 0, 3, 1, 0 and cb * 1 mod 4 is 0, 1, 3, 0.  The crop on the full image gives the bits
    of crop_border = 0 on a contiguous copy of the crop."""
    h, w = 61, 83
    for cn, modes in ((3, MODES), (1, MODES[2:])):
        a, b = _case(h, w, cn)
        for mode, name in modes:
            got = _run(ctx, a, b, cb, mode)
            _check(got, _ref(h, w, cn, cb, mode), mode, f"cb {cb} cn {cn} {name}")
            ac, bc = np.ascontiguousarray(R.crop(a, cb)), np.ascontiguousarray(R.crop(b, cb))
            assert _bits(_run(ctx, ac, bc, 0, mode)) == _bits(got), (cb, cn, name)
    # the crops are told apart
    assert len({_ref(h, w, 3, c, R.Y)["ssim"] for c in (0, 1, 3, 4)}) == 4


@pytest.mark.parametrize("data_range", [200.0, 100.0])
def test_data_range(ctx, data_range):
    a, b = _case(61, 83, 3)
    for mode, name in MODES:
        want = _ref(61, 83, 3, 3, mode, data_range)
        assert want["ssim"] != _ref(61, 83, 3, 3, mode)["ssim"]
        _check(_run(ctx, a, b, 3, mode, data_range=data_range), want, mode, f"range {data_range} {name}")


def test_against_skimage(ctx):
    import _native
    z = np.load(os.path.join(GOLD, "srbench_skimage.npz"))
    a, b = z["a"], z["b"]
    for i, cb in enumerate(z["crop_borders"].tolist()):
        for mode, name in ((R.Y, "y"), (R.Y_ROUND, "y_round"), (R.CHANNELS, "rgb")):
            psnr, ssim = _native.bench_values(_run(ctx, a, b, cb, mode))
            wp, ws = float(z["psnr_" + name][i]), float(z["ssim_" + name][i])
            print(cb, name, psnr, wp, abs(psnr - wp) / wp, ssim, ws, abs(ssim - ws) / ws)
            assert psnr == pytest.approx(wp, rel=TOL, abs=0), (cb, name)
            assert ssim == pytest.approx(ws, rel=TOL, abs=0), (cb, name)


def test_identical_images(ctx):
    import _native
    for h, w in ((27, 257), (61, 83)):
        a = _case(h, w, 3)[0]
        for mode, name in MODES:
            rec = _run(ctx, a, a, 1, mode)
            psnr, ssim = _native.bench_values(rec)
            assert rec["sse"] == 0.0 and psnr == math.inf, name
            assert ssim == pytest.approx(1.0, abs=1e-12), name


def test_gray_through_y_round_is_channels_on_the_mapped_plane(ctx):
    """R = G = B = v: X = 219000 v + 4080000, so Y_ROUND sees the plane floor((2 X + 255000) / 510000), computed here on the
    host and fed as one channel: bit for bit."""
    va, vb = _case(45, 521, 1)
    rgb_a, rgb_b = (np.ascontiguousarray(np.stack([v, v, v], -1)) for v in (va, vb))
    ya, yb = R.gray_as_y_round(va), R.gray_as_y_round(vb)
    assert ya.min() >= 16 and ya.max() <= 235 and not np.array_equal(ya, va)
    for cb in (0, 3):
        got = _run(ctx, rgb_a, rgb_b, cb, R.Y_ROUND)
        want = _run(ctx, ya, yb, cb, R.CHANNELS)
        assert _bits(got) == _bits(want), cb
        assert got["sse"] == R.bench(ya, yb, cb, R.CHANNELS)["sse_int"]


def test_equal_inputs_give_equal_bits(ctx):
    h, w = 45, 521
    a, b = _case(h, w, 3)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for mode, _ in MODES:
            first = ctx.bench_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            second = ctx.bench_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
            ctx.bench_u8(db.ptr, w * 3, da.ptr, w * 3, 30, 400, 3, 0, R.CHANNELS, 100.0)     # another shape through the scratch
            third = ctx.bench_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, 2, mode)
            assert _bits(first) == _bits(second) == _bits(third), mode
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 61, 83, 3
    a, b = _case(h, w, cn)
    for mode, name in (MODES if cn == 3 else MODES[2:]):
        dense = _run(ctx, a, b, cb, mode)
        for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
            la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
            pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
            pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
            try:
                got = ctx.bench_u8(ptr_a, sa, ptr_b, sb, h, w, cn, cb, mode)
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
    h, w, cb = 166, 40, 1
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
        for mode, name in MODES:
            dense = _run(ctx, a, b, cb, mode)
            got = ctx.bench_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3, cb, mode)
            assert _bits(got) == _bits(dense), name
            _check(got, _ref(h, w, 3, cb, mode), mode, f"wide stride {name}")
    finally:
        wide.free(); da.free(); pb.free()


def test_module_methods(ctx):
    import quality_assessment_module as qam
    a, b = _case(61, 83, 3)
    q = qam.QualityAssessmentModule()
    for kw, mode, channel in ((dict(), R.Y, "y"), (dict(y_round=True), R.Y_ROUND, "y_round"), (dict(test_y_channel=False), R.CHANNELS, "rgb")):
        want = _ref(61, 83, 3, 4, mode)
        got = q.evaluate_sr_benchmark(a, b, crop_border=4, **kw)
        assert sorted(got) == ["channel", "crop_border", "psnr", "ssim"] and got["channel"] == channel and got["crop_border"] == 4
        assert isinstance(got["psnr"], float) and isinstance(got["ssim"], float)
        assert got["psnr"] == pytest.approx(want["psnr"], rel=TOL, abs=0) and got["ssim"] == pytest.approx(want["ssim"], rel=TOL, abs=0)
        # the device form on resident images gives the same bits
        da, db = ctx.upload(a), ctx.upload(b)
        try:
            dev = q.evaluate_sr_benchmark_device(da.ptr, a.shape, db.ptr, b.shape, crop_border=4, **kw)
        finally:
            da.free(); db.free()
        assert dev == got
    # defaults: Y channel, no crop; data_range reaches the kernel and the PSNR
    assert q.evaluate_sr_benchmark(a, b)["ssim"] == pytest.approx(_ref(61, 83, 3, 0, R.Y)["ssim"], rel=TOL, abs=0)
    r200 = _ref(61, 83, 3, 4, R.Y, 200.0)
    g200 = q.evaluate_sr_benchmark(a, b, crop_border=4, data_range=200.0)
    assert g200["psnr"] == pytest.approx(r200["psnr"], rel=TOL, abs=0) and g200["ssim"] == pytest.approx(r200["ssim"], rel=TOL, abs=0)
    # a gray pair: the channel as it is
    ga, gb = _case(61, 83, 1)
    gg = q.evaluate_sr_benchmark(ga, gb, crop_border=1, test_y_channel=False)
    assert gg["channel"] == "gray" and gg["ssim"] == pytest.approx(_ref(61, 83, 1, 1, R.CHANNELS)["ssim"], rel=TOL, abs=0)
    assert q.evaluate_sr_benchmark(a, a)["psnr"] == math.inf
    # the existing PSNR (over all RGB elements, no crop) is another number
    assert abs(q.calculate_psnr(a, b) - q.evaluate_sr_benchmark(a, b)["psnr"]) > 0.1


def test_pipeline_hook(ctx, rng, tmp_path):
    import json

    import main as sr_main
    from PIL import Image
    import _msssim_ref as M
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("sr_benchmark", "sr_benchmark_note")
    # default: no key
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # with the option: the device-resident path
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_benchmark=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "bench" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"] and "sr_benchmark_note" not in rep
    assert sorted(set(rep) - set(res0.quality_report)) == ["sr_benchmark"]
    sec = rep["sr_benchmark"]
    assert sorted(sec) == ["crop_border", "psnr_rgb", "psnr_y", "ssim_rgb", "ssim_y"] and sec["crop_border"] == 2
    fused = np.asarray(Image.open(out))
    assert fused.shape == (160, 192, 3)
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (160, 192))
    y = q.evaluate_sr_benchmark(ref_img, fused, crop_border=2)
    rgb = q.evaluate_sr_benchmark(ref_img, fused, crop_border=2, test_y_channel=False)
    assert (sec["psnr_y"], sec["ssim_y"], sec["psnr_rgb"], sec["ssim_rgb"]) == (y["psnr"], y["ssim"], rgb["psnr"], rgb["ssim"])
    want = R.bench(ref_img, fused, 2, R.Y)
    assert sec["ssim_y"] == pytest.approx(want["ssim"], rel=TOL, abs=0) and sec["psnr_y"] == pytest.approx(want["psnr"], rel=TOL, abs=0)
    assert 0.0 < sec["ssim_y"] <= 1.0 and 0.0 < sec["ssim_rgb"] <= 1.0 and sec["psnr_y"] > 10.0
    on_disk = json.load(open(str(tmp_path / "bench" / "result_qa_report.json")))
    assert on_disk["sr_benchmark"] == sec
    # the host-array path agrees bit for bit
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_benchmark=True, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report["sr_benchmark"] == sec and "sr_benchmark_note" not in res_h.quality_report
    # A canvas of 12 rows has 8 after the crop, below the window: None entries and a note, no error.  (Stage 4's other metrics
    # need far more than 12 rows, so no whole run gets here; the one helper all three paths call is called as they call it.)
    d_src, d_canvas = ctx.upload(np.ascontiguousarray(img[:6, :48])), ctx.upload(np.ascontiguousarray(ref_img[:12, :96]))
    try:
        for p in (pipe, pipe_h):
            rep_s = {"kept": 1}
            p._sr_benchmark(ctx, rep_s, d_src.ptr, (6, 48, 3), d_canvas.ptr, (12, 96, 3))
            assert rep_s["sr_benchmark"] == {"psnr_y": None, "ssim_y": None, "psnr_rgb": None, "ssim_rgb": None, "crop_border": 2}
            assert "at least 11" in rep_s["sr_benchmark_note"] and rep_s["kept"] == 1
            json.dumps(rep_s)
    finally:
        d_src.free(); d_canvas.free()
    # 15 rows leave exactly 11: values, no note
    d_src, d_canvas = ctx.upload(np.ascontiguousarray(img[:8, :48])), ctx.upload(np.ascontiguousarray(fused[:15, :96]))
    try:
        rep_ok = {}
        pipe._sr_benchmark(ctx, rep_ok, d_src.ptr, (8, 48, 3), d_canvas.ptr, (15, 96, 3))
    finally:
        d_src.free(); d_canvas.free()
    assert "sr_benchmark_note" not in rep_ok and all(isinstance(rep_ok["sr_benchmark"][k], float) for k in ("psnr_y", "ssim_y", "psnr_rgb", "ssim_rgb"))
    ref15 = q.upsample_bicubic(np.ascontiguousarray(img[:8, :48]), (15, 96))
    assert rep_ok["sr_benchmark"]["ssim_y"] == pytest.approx(R.bench(ref15, np.ascontiguousarray(fused[:15, :96]), 2, R.Y)["ssim"], rel=TOL, abs=0)
