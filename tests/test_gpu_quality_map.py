"""GPU: the per-cell PSNR / SSIM quality map (sr_quality_map_u8, csrc/sr_qmap.hip).

* restatement: every cell against tests/_qmap_ref.py (the algebra of oracle_np.ssim before its mean, binned) -- the squared
  error exactly, every SSIM sum at the 1e-9 the suite holds between the HIP SSIM and this oracle;
* recombination: the cells add up to sr_sse_u8 (exactly), to sr_assess_u8 (1e-10: a reordered fp64 sum of n <= 4e5 terms of
  magnitude <= 1 is bounded by n 2^-53 ~ 5e-11) and to the scikit-image fixtures (the tolerance of test_gpu_metrics.py);
* reproducibility: equal inputs give equal bits;
* strided, offset, guarded views (one with rows beyond 2^32 bytes) give the bits of the dense call;
* the module methods and the pipeline hook (default off).
parity: pinned through the recombination with the scikit-image fixtures; the per-cell split itself is checked against this
repository's restatement."""
import asyncio
import functools
import os

import numpy as np
import pytest

import _qmap_ref as R
import _views as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "metrics_skimage.npz")
FIELDS = ("ssim_uniform", "ssim_gauss", "ssim_simple")


@functools.lru_cache(maxsize=None)
def _case(h, w, cn, shift=15):
    """One image pair per shape and its reference maps, computed once and shared (never modified)."""
    a, b = R.img_pair(np.random.default_rng(1000 * h + w + cn), h, w, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b, R.Reference(a, b, shift)


def _run(ctx, a, b, xe, ye, **kw):
    cn = a.shape[2] if a.ndim == 3 else 1
    h, w = a.shape[:2]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.quality_map_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, xe, ye, **kw)
    finally:
        da.free(); db.free()


def _check(got, want, what):
    print(what, "cells", got["sse"].shape)
    assert got["sse"].dtype == np.uint64 and np.array_equal(got["sse"], want["sse"]), what
    for k in FIELDS:
        g, r = got[k], want[k]
        err = np.abs(g - r) / np.maximum(np.abs(r), 1e-300)
        print(f"  {k}: largest relative error {np.where(r != 0, err, 0).max():.3e}")
        assert g.shape == r.shape and g.dtype == np.float64
        for i in range(g.size):
            assert g.flat[i] == pytest.approx(r.flat[i], rel=1e-9, abs=1e-12), (what, k, np.unravel_index(i, g.shape))
        empty = want["count_" + k[5:]] == 0
        assert np.all(g[empty] == 0.0), (what, k)                   # a cell without a valid sample: exactly 0


GRIDS = [(97, 131, 3, c) for c in (4, 16, 37, 64, 200)] + [(97, 131, 1, c) for c in (4, 16, 37, 64, 200)] + \
        [(23, 29, 3, c) for c in (1, 4, 16, 37, 64)] + [(523, 771, 3, c) for c in (16, 37, 64, 1000)]


@pytest.mark.parametrize("h,w,cn,cell", GRIDS, ids=[f"{g[0]}x{g[1]}x{g[2]}-cell{g[3]}" for g in GRIDS])
def test_uniform_cells_match_the_restatement(ctx, h, w, cn, cell):
    a, b, ref = _case(h, w, cn)
    xe, ye = R.uniform_edges(w, cell), R.uniform_edges(h, cell)
    got = _run(ctx, a, b, xe, ye)
    want = ref.cells(xe, ye)
    _check(got, want, f"{h}x{w}x{cn} cell {cell}")
    if cell == 4:
        # the top / left cell rows lie wholly inside the gauss crop: count 0, sum exactly 0
        assert np.all(want["count_gauss"][0] == 0) and np.all(got["ssim_gauss"][0] == 0.0) and np.all(got["ssim_gauss"][:, 0] == 0.0)
    if cell == 1:
        # the map is then the S map itself (0 outside the valid region)
        assert got["ssim_simple"].shape == (h, w)
        assert np.all(got["ssim_gauss"][:5] == 0) and np.all(got["ssim_uniform"][:, -3:] == 0)
        assert np.all(got["ssim_gauss"][5:-5, 5:-5] != 0)


def test_non_uniform_grid(ctx):
    a, b, ref = _case(97, 131, 3)
    xe, ye = [0, 5, 6, 70, 131], [0, 1, 50, 97]
    _check(_run(ctx, a, b, xe, ye), ref.cells(xe, ye), "non-uniform")


def test_gray_shift_14_and_flag_selection(ctx):
    a, b = _case(97, 131, 3)[:2]
    ref14 = R.Reference(a, b, 14)
    xe, ye = R.uniform_edges(131, 37), R.uniform_edges(97, 37)
    _check(_run(ctx, a, b, xe, ye, gray_shift=14), ref14.cells(xe, ye), "gray_shift 14")
    # unselected fields are 0, selected ones do not depend on what else is selected
    import _native
    full = _run(ctx, a, b, xe, ye)
    for flags, keep in ((_native.ASSESS_SSE, ("sse",)), (_native.ASSESS_GAUSS11, ("ssim_gauss",)),
                        (_native.ASSESS_SSE | _native.ASSESS_UNIFORM7, ("sse", "ssim_uniform")),
                        (_native.ASSESS_SIMPLE, ("ssim_simple",)), (0, ())):
        part = _run(ctx, a, b, xe, ye, flags=flags)
        for k in ("sse",) + FIELDS:
            if k in keep:
                assert np.array_equal(part[k].view(np.uint64), full[k].view(np.uint64)), (flags, k)
            else:
                assert not part[k].any(), (flags, k)
    # another data_range: the cropped variants take its constants, simple keeps those of 255
    dr = _run(ctx, a, b, xe, ye, data_range=510.0)
    want = R.Reference(a, b, 15, 510.0).cells(xe, ye)
    _check(dr, want, "data_range 510")
    assert not np.array_equal(dr["ssim_gauss"], full["ssim_gauss"]) and dr["ssim_simple"] == pytest.approx(full["ssim_simple"], rel=1e-12)


def test_cells_recombine_to_the_global_metrics(ctx):
    import _native
    a, b, _ = _case(523, 771, 3)
    h, w = 523, 771
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        sse = ctx.sse_u8(da.ptr, w * 3, db.ptr, w * 3, h, w * 3)
        glob = ctx.assess_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, flags=_native.ASSESS_ALL)
        for xe, ye in ((R.uniform_edges(w, 64), R.uniform_edges(h, 64)), (R.uniform_edges(w, 37), R.uniform_edges(h, 16)),
                       ([0, 5, 6, 700, w], [0, 1, 300, h])):
            m = ctx.quality_map_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye)
            assert int(m["sse"].sum()) == sse == int(round(glob["sse"]))
            for k in FIELDS:
                print(k, m[k].sum(), glob[k], abs(m[k].sum() - glob[k]) / abs(glob[k]))
                assert m[k].sum() == pytest.approx(glob[k], rel=1e-10)
                cnt = _native.quality_map_counts(h, w, k[5:], xe, ye)
                assert int(cnt.sum()) == _native.ssim_count(h, w, k[5:])
    finally:
        da.free(); db.free()


def test_cells_recombine_to_the_skimage_fixtures(ctx):
    import _native
    z = np.load(GOLD)
    pairs = [(z[f"{name}_a"], z[f"{name}_b"], 1, float(z[f"{name}_psnr"]), float(z[f"{name}_ssim_uniform"]),
              float(z[f"{name}_ssim_gauss"])) for name in z["cases"]]
    np.random.seed(42)                                  # the 512 x 512 pair of the fixture file is generated, not stored
    o = np.random.randint(0, 256, (512, 512, 3), dtype=np.uint8)
    u = np.clip(o.astype(np.float32) + np.random.randn(512, 512, 3) * 5, 0, 255).astype(np.uint8)
    pairs.append((o, u, 0, float(z["ex_psnr"]), float(z["ex_ssim_uniform_ch0"]), float(z["ex_ssim_gauss_ch0"])))
    assert {(64, 64), (193, 257), (512, 512)} <= {p[0].shape[:2] for p in pairs}
    for a, b, ch, psnr, s_uniform, s_gauss in pairs:
        h, w = a.shape[:2]
        xe, ye = R.uniform_edges(w, 48), R.uniform_edges(h, 48)
        m = _run(ctx, a, b, xe, ye, flags=_native.ASSESS_SSE)
        assert _native.psnr_from_sse(int(m["sse"].sum()), a.size, 255.0) == pytest.approx(psnr, rel=1e-12)
        ga, gb = np.ascontiguousarray(a[..., ch]), np.ascontiguousarray(b[..., ch])
        m = _run(ctx, ga, gb, xe, ye)
        for mode, want in (("uniform", s_uniform), ("gauss", s_gauss)):
            n = _native.quality_map_counts(h, w, mode, xe, ye)
            assert int(n.sum()) == _native.ssim_count(h, w, mode)
            assert m[f"ssim_{mode}"].sum() / n.sum() == pytest.approx(want, rel=1e-9)


def test_equal_inputs_give_equal_bits(ctx):
    a, b, _ = _case(523, 771, 3)
    h, w = 523, 771
    xe, ye = R.uniform_edges(w, 64), R.uniform_edges(h, 64)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        first = ctx.quality_map_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye)
        second = ctx.quality_map_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye)
        ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)            # unrelated work on the same stream and scratch
        tmp = ctx.alloc(200 * 300 * 3)
        ctx.resize_cubic_u8(da.ptr, w * 3, h, w, 3, tmp.ptr, 300 * 3, 200, 300)
        third = ctx.quality_map_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, xe, ye)
        tmp.free()
        for k in ("sse",) + FIELDS:
            assert np.array_equal(first[k].view(np.uint64), second[k].view(np.uint64)), k
            assert np.array_equal(first[k].view(np.uint64), third[k].view(np.uint64)), k
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    a, b, _ = _case(97, 131, cn)
    xe, ye = R.uniform_edges(131, 37), [0, 1, 50, 97]
    dense = _run(ctx, a, b, xe, ye)
    for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
        la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
        pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
        pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
        try:
            got = ctx.quality_map_u8(ptr_a, sa, ptr_b, sb, 97, 131, cn, xe, ye)
        finally:
            pa.free(); pb.free()
        for f in ("sse",) + FIELDS:
            assert np.array_equal(got[f].view(np.uint64), dense[f].view(np.uint64)), (V.layout_id(la), V.layout_id(lb), f)


def test_rows_beyond_4_gib(ctx):
    """64 rows at a stride of 72 MiB + 5 bytes: rows 60 .. 63 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    a, b = R.img_pair(np.random.default_rng(77), 64, 96)
    xe, ye = R.uniform_edges(96, 37), R.uniform_edges(64, 16)
    dense = _run(ctx, a, b, xe, ye)
    stride = (72 << 20) + 5
    assert 60 * stride >= 1 << 32
    total = V.GUARD + 63 * stride + 96 * 3 + V.GUARD
    assert total < 8 << 30
    wide = ctx.alloc(total)
    da = ctx.upload(a)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 2, V.FILLS[1])
    try:
        for r in range(64):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, da.ptr + r * 96 * 3, 96 * 3)
        ctx.sync()
        got = ctx.quality_map_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, 64, 96, 3, xe, ye)
        swapped = ctx.quality_map_u8(ptr_b, sb, wide.ptr + V.GUARD, stride, 64, 96, 3, xe, ye)
    finally:
        wide.free(); da.free(); pb.free()
    for f in ("sse",) + FIELDS:
        assert np.array_equal(got[f].view(np.uint64), dense[f].view(np.uint64)), f
    assert np.array_equal(swapped["sse"], dense["sse"])


def test_module_methods(ctx):
    import _native
    import quality_assessment_module as qam
    a, b, ref = _case(97, 131, 3)
    q = qam.QualityAssessmentModule()
    m = q.evaluate_quality_map(a, b, cell=37)
    xe, ye = R.uniform_edges(131, 37), R.uniform_edges(97, 37)
    want = ref.cells(xe, ye)
    assert m["x_edges"] == xe and m["y_edges"] == ye
    elems = np.outer(np.diff(ye), np.diff(xe)) * 3
    assert np.array_equal(m["mse"], want["sse"].astype(np.float64) / elems)
    assert np.allclose(m["psnr"], 10 * np.log10(255.0 ** 2 / m["mse"]), rtol=1e-15)
    assert np.array_equal(m["ssim_count"].astype(np.int64), want["count_uniform"])
    assert np.array_equal(m["ms_ssim_count"].astype(np.int64), want["count_gauss"])
    assert m["ssim"] == pytest.approx(want["ssim_uniform"] / want["count_uniform"], rel=1e-9)
    assert m["ms_ssim"] == pytest.approx(want["ssim_gauss"] / want["count_gauss"], rel=1e-9)
    # the device form on resident images gives the same arrays
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        d = q.evaluate_quality_map_device(da.ptr, a.shape, db.ptr, b.shape, cell=37)
    finally:
        da.free(); db.free()
    assert d.keys() == m.keys()
    for k in m:
        assert np.array_equal(np.asarray(d[k]), np.asarray(m[k]), equal_nan=(np.asarray(m[k]).dtype.kind == "f")), k
    # a cell without a valid sample has mean nan; identical images have psnr inf and ssim 1
    m4 = q.evaluate_quality_map(a, b, cell=4)
    assert np.all(np.isnan(m4["ms_ssim"][0])) and np.all(np.isnan(m4["ms_ssim"][:, 0])) and not np.isnan(m4["ms_ssim"][2:-2, 2:-2]).any()
    assert not np.isnan(m4["ssim"][1:-1, 1:-1]).any() and m4["ssim_count"][0, 0] == 1 and np.isnan(m4["ssim"][-1, -1])
    same = q.evaluate_quality_map(a, a, x_edges=[0, 5, 6, 70, 131], y_edges=[0, 1, 50, 97])
    assert np.all(np.isinf(same["psnr"])) and np.all(same["mse"] == 0)
    ok = ~np.isnan(same["ms_ssim"])
    assert ok.any() and same["ms_ssim"][ok] == pytest.approx(1.0, rel=1e-12)
    # branch 'B': the simple variant in both keys
    qb = qam.QualityAssessmentModule(ssim_branch='B')
    mb = qb.evaluate_quality_map(a, b, cell=37)
    assert np.array_equal(mb["ssim"], mb["ms_ssim"]) and np.array_equal(mb["ssim_count"], mb["ms_ssim_count"])
    assert mb["ssim"] == pytest.approx(want["ssim_simple"] / want["count_simple"], rel=1e-9)
    assert int(mb["ssim_count"].sum()) == 97 * 131
    # differently sized inputs: the common top-left rectangle, like calculate_psnr
    a2, b2 = _case(97, 131, 3)[0], _case(523, 771, 3)[1][:90, :140]
    mc = q.evaluate_quality_map(a2, b2, cell=64)
    assert mc["x_edges"] == [0, 64, 128, 131] and mc["y_edges"] == [0, 64, 90]
    ac, bc = np.ascontiguousarray(a2[:90, :131]), np.ascontiguousarray(b2[:90, :131])
    md = q.evaluate_quality_map(ac, bc, cell=64)
    for k in ("sse", "ssim", "ms_ssim"):
        assert np.array_equal(mc[k], md[k], equal_nan=True), k
    assert _native.psnr_from_sse(int(mc["sse"].sum()), 90 * 131 * 3) == q.calculate_psnr(a2, b2)


def _decode_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_pipeline_hook(rng, tmp_path):
    import _native
    import main as sr_main
    from PIL import Image
    img = R.img_pair(rng, 200, 300)[0]
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=128, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    # default: no key, no file
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert 'quality_map' not in res0.quality_report
    assert sorted(os.listdir(tmp_path / "plain")) == ["result.png", "result_qa_report.json"]
    # with the map
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_map_cell=64, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "map" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    fused = _decode_png(out)
    H, W = 400, 600
    assert fused.shape == (H, W, 3) and np.array_equal(fused, _decode_png(str(tmp_path / "plain" / "result.png")))
    assert {k: v for k, v in res.quality_report['full_reference'].items()} == res0.quality_report['full_reference']
    sec = res.quality_report['quality_map']
    gh, gw = 7, 10
    assert sec["cell"] == 64 and sec["grid"] == [gh, gw]
    assert sec["x_edges"] == R.uniform_edges(W, 64) and sec["y_edges"] == R.uniform_edges(H, 64)
    for k in ("psnr", "ssim", "ms_ssim", "sse"):
        assert len(sec[k]) == gh and all(len(r) == gw for r in sec[k]), k
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, (H, W))
    total = sum(sum(r) for r in sec["sse"])
    assert _native.psnr_from_sse(total, H * W * 3) == q.calculate_psnr(ref_img, fused)
    direct = q.evaluate_quality_map(ref_img, fused, cell=64)
    assert np.array_equal(np.array(sec["ms_ssim"], dtype=np.float64), direct["ms_ssim"])
    assert np.array_equal(np.array(sec["psnr"], dtype=np.float64), direct["psnr"])
    # the five worst cells by ms_ssim, with their rectangles
    flat = sorted((v, gy, gx) for gy, r in enumerate(sec["ms_ssim"]) for gx, v in enumerate(r))
    assert [(c["ms_ssim"], c["gy"], c["gx"]) for c in sec["worst_cells"]] == flat[:5]
    c = sec["worst_cells"][0]
    assert c["rect"] == [64 * c["gx"], 64 * c["gy"], min(64, W - 64 * c["gx"]), min(64, H - 64 * c["gy"])]
    # one entry per tile: its ownership region (cuts at 2 * 103 + 25 = 231 and 437)
    assert len(sec["tiles"]) == res.total_blocks == 6
    assert sorted(t["rect"] for t in sec["tiles"]) == sorted([x0, y0, x1 - x0, y1 - y0] for (y0, y1) in ((0, 231), (231, 400))
                                                           for (x0, x1) in ((0, 231), (231, 437), (437, 600)))
    per_tile = q.evaluate_quality_map(ref_img, fused, x_edges=[0, 231, 437, 600], y_edges=[0, 231, 400])
    for t in sec["tiles"]:
        assert t["ms_ssim"] == per_tile["ms_ssim"][t["row"], t["col"]] and t["psnr"] == per_tile["psnr"][t["row"], t["col"]]
    # the PNG: gh x gw gray, floor(255 * clip(ms_ssim, 0, 1))
    png = _decode_png(str(tmp_path / "map" / "result_qa_map.png"))
    assert png.shape == (gh, gw) and png.dtype == np.uint8
    assert np.array_equal(png, np.floor(255.0 * np.clip(direct["ms_ssim"], 0, 1)).astype(np.uint8))
    assert sec["image"] == "result_qa_map.png"
    assert sorted(os.listdir(tmp_path / "map")) == ["result.png", "result_qa_map.png", "result_qa_report.json"]
    # the host-array path gives the same section
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_map_cell=64, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report['quality_map'] == sec
    assert np.array_equal(_decode_png(str(tmp_path / "host" / "result_qa_map.png")), png)
