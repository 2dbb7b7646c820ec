"""GPU: FSIM / FSIMc (sr_fsim_u8, csrc/sr_fsim.hip) and its inspection entries.

* pooling: sr_fsim_pool_u8 equals the restatement's integer window sums exactly, F in {1, 2, 3, 4, 5, 8} on 13 x 19, 16 x 16 and
  17 x 23 with 1, 3 and 4 channels, and on both sides of the kernel's row-segment constant (a block holds floor(256 / F)
  windows: widths 255 .. 258 put the last window of a row on either side of a block's end for every F of the list), plus
  F = 200 (one window per block, idle lanes) and F = 256 (the largest);
* phase congruency: sr_fsim_pc_f64 against the restatement (numpy.fft) at 1e-9 absolute, medians at 1e-12 relative, on planes
  with odd and even element counts, odd and even sides;
* the pair: the three sums and both values at 1e-9 relative on the seven shapes of the issue's table (F = 1, 2, 3), the
  distorted image being the reference plus bounded noise plus one flat patch;
* probes: complementary colours (a negative S_i S_q), identity, symmetry, a flat pair;
* equal bits for equal inputs (also after the workspace has grown), padded, offset, guarded views (one with rows beyond 2^32
  bytes), nothing written outside a view;
* the module methods, their device twin and the pipeline switch (default off).
parity: unpinned (MATLAB, piq, pyiqa are not available offline); pinned by the restatement tests/_fsim_ref.py alone."""
import asyncio
import functools
import math

import numpy as np
import pytest

import _fsim_ref as R
import _views as V

pytestmark = pytest.mark.gpu

TOL = 1e-9
# (h, w, cn) of the issue's table: F = 1 (five shapes, 383 the last short side of F = 1), 2, 3
PAIRS = [(16, 16, 1), (17, 23, 3), (32, 45, 3), (64, 64, 1), (383, 200, 3), (384, 385, 3), (640, 641, 1)]


@functools.lru_cache(maxsize=None)
def _case(h, w, cn):
    """One structured image and its distorted copy (noise within +-20 and a flat patch) per shape, shared, never modified."""
    a, b = R.case(h, w, cn)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(h, w, cn):
    a, b = _case(h, w, cn)
    r = R.fsim(a, b)
    assert r["an_all_min"] >= 1e-3, (h, w, cn, r["an_all_min"])        # the guard of the definition's 0 / 0
    return r


def _cn(a):
    return a.shape[2] if a.ndim == 3 else 1


def _run(ctx, a, b):
    h, w = a.shape[:2]
    cn = _cn(a)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.fsim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn)
    finally:
        da.free(); db.free()


def _bits(rec):
    return tuple(np.float64(rec[k]).view(np.uint64) for k in ("sum_s", "sum_sc", "sum_pcm")) + (rec["count"], rec["F"], rec["size"])


def _check(got, want, what):
    import _native
    assert got["F"] == want["F"] and tuple(got["size"]) == tuple(want["size"]), what
    assert got["count"] == want["size"][0] * want["size"][1], what
    v, vc = _native.fsim_value(got)
    for k, g, wv in (("sum_s", got["sum_s"], want["sum_s"]), ("sum_sc", got["sum_sc"], want["sum_sc"]),
                     ("sum_pcm", got["sum_pcm"], want["sum_pcm"]), ("fsim", v, want["fsim"]), ("fsimc", vc, want["fsimc"])):
        print(f"{what} {k}: {g!r} ref {wv!r} rel {abs(g - wv) / abs(wv):.2e}")
        assert g == pytest.approx(wv, rel=TOL, abs=0), (what, k)


# ---- pooling -------------------------------------------------------------------------------------------------------------------
def _pool(ctx, a, b, F):
    h, w = a.shape[:2]
    cn = _cn(a)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return ctx.fsim_pool_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, F)
    finally:
        da.free(); db.free()


def _pool_pair(h, w, cn, seed):
    rnd = np.random.default_rng(seed)
    shape = (h, w) if cn == 1 else (h, w, cn)
    return rnd.integers(0, 256, shape, dtype=np.uint8), rnd.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_pooling_is_exact_at_small_shapes(ctx, cn):
    for h, w in ((13, 19), (16, 16), (17, 23)):
        a, b = _pool_pair(h, w, cn, 100 * h + w + cn)
        for F in (1, 2, 3, 4, 5, 8):
            got = _pool(ctx, a, b, F)
            want = np.stack([R.pooled_int(a, F), R.pooled_int(b, F)])
            assert got.shape == want.shape == (2, 3, -(-h // F), -(-w // F))
            assert np.array_equal(got, want), (h, w, cn, F)
    if cn == 1:
        assert not got[:, 1:].any()                     # a gray image's I and Q records are 0


@pytest.mark.parametrize("w", [255, 256, 257, 258])
def test_pooling_on_both_sides_of_the_row_segment(ctx, w):
    """A block holds floor(256 / F) windows: 256, 128, 85, 64, 51, 32 for the F of the list.  The pooled widths of 255 .. 258
    columns are 128 | 129 (F = 2), 85 | 86 (3), 64 | 65 (4), 51 | 52 (5) and 32 | 33 (8), and 256 | 257 at F = 1."""
    import _native
    h = 11
    a, b = _pool_pair(h, w, 3, w)
    for F in (1, 2, 3, 4, 5, 8):
        assert np.array_equal(_pool(ctx, a, b, F), np.stack([R.pooled_int(a, F), R.pooled_int(b, F)])), (w, F)
    widths = {F: sorted({-(-v // F) for v in (255, 256, 257, 258)}) for F in (1, 2, 3, 4, 5, 8)}
    assert all(256 // F in ws and 256 // F + 1 in ws for F, ws in widths.items())
    with pytest.raises(ValueError):
        _pool(ctx, a, b, 257)
    assert "256" in _native.last_error()


def test_pooling_with_large_windows(ctx):
    """F = 200: one window per block and 56 idle lanes; F = 256: the largest, every lane a column.  The windows hang over the
    top, the left and (partly) the bottom and right edges."""
    a, b = _pool_pair(300, 610, 3, 5)
    for F in (200, 256):
        assert np.array_equal(_pool(ctx, a, b, F), np.stack([R.pooled_int(a, F), R.pooled_int(b, F)])), F


# ---- phase congruency ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(16, 16), (17, 23), (32, 45), (33, 47), (50, 17)],
                         ids=lambda v: str(v))
def test_phase_congruency_matches_the_restatement(ctx, rows, cols):
    """16 x 16, 32 x 45, 50 x 17: even counts (the mean of the two middle values); 17 x 23, 33 x 47: odd counts.  More than one
    transform tile on both axes from 17 up, sides that are no multiple of the tile."""
    img = R.structured(rows, cols, 1, rows * cols)
    plane = img.astype(np.float64) * (1000.0 / 1003.0) + 0.125            # no integers: as a pooled plane is
    want = R.phasecong(plane)
    assert want["an_all"].min() >= 1e-3
    d_in, d_out = ctx.upload(plane), ctx.alloc(rows * cols * 8)
    try:
        got = ctx.fsim_pc_f64(d_in.ptr, rows, cols, d_out.ptr)
        pc = ctx.download(d_out.ptr, (rows, cols), np.float64)
    finally:
        d_in.free(); d_out.free()
    worst = float(np.abs(pc - want["pc"]).max())
    rel_med = float(np.abs(got["median"] / want["median"] - 1).max())
    rel_t = float(np.abs(got["T"] / want["T"] - 1).max())
    print(f"{rows}x{cols}: max |dPC| {worst:.2e}   medians rel {rel_med:.2e}   T rel {rel_t:.2e}   PC in [{pc.min():.3f}, {pc.max():.3f}]")
    assert worst <= 1e-9
    assert rel_med <= 1e-12
    assert rel_t <= 1e-9
    assert pc.max() > 0.2 and (pc >= 0).all()


def test_phase_congruency_writes_its_plane_only_and_refuses_on_the_host(ctx):
    import _native
    rows, cols = 17, 23
    plane = R.structured(rows, cols, 1, 3).astype(np.float64)
    d_in = ctx.upload(plane)
    out, ptr, stride = V.out_view(ctx, rows, cols * 8, 0, 0, V.FILLS[0])
    try:
        ctx.fsim_pc_f64(d_in.ptr, rows, cols, ptr)
        pc = V.check_guard(ctx, out, np.float64, (rows, cols), what="pc")
        assert np.abs(pc - R.phasecong(plane)["pc"]).max() <= 1e-9
        with pytest.raises(_native.SrShapeError):
            ctx.fsim_pc_f64(d_in.ptr, 15, 23, ptr)
        with pytest.raises(_native.SrNativeError):
            ctx.fsim_pc_f64(d_in.ptr, 16, 2049, ptr)
        assert "2048" in _native.last_error()
    finally:
        d_in.free(); out.free()


# ---- the pair --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,cn", PAIRS, ids=[f"{h}x{w}x{c}" for h, w, c in PAIRS])
def test_the_pair_matches_the_restatement(ctx, h, w, cn):
    a, b = _case(h, w, cn)
    want = _ref(h, w, cn)
    got = _run(ctx, a, b)
    _check(got, want, f"{h}x{w}x{cn}")
    assert 0.5 < want["fsim"] < 0.9999
    if cn == 1:
        assert got["sum_sc"] == got["sum_s"]


def test_four_channels_ignore_alpha(ctx):
    a, b = _case(32, 45, 3)
    rnd = np.random.default_rng(9)
    a4 = np.dstack([a, rnd.integers(0, 256, a.shape[:2], dtype=np.uint8)])
    b4 = np.dstack([b, rnd.integers(0, 256, a.shape[:2], dtype=np.uint8)])
    assert _bits(_run(ctx, a4, b4)) == _bits(_run(ctx, a, b))


def test_complementary_colours_take_the_negative_branch(ctx):
    """Red against blue: I changes sign and Q does not, so S_i S_q is negative there and the weight is |z|^0.03 cos(0.03 pi)."""
    a, b = (v.copy() for v in _case(32, 45, 3))
    a[6:20, 8:30] = (255, 0, 0)
    b[6:20, 8:30] = (0, 0, 255)
    want = R.fsim(a, b)
    assert want["min_siq"] < -0.1 and want["an_all_min"] >= 1e-3
    assert abs(R.fsim(a, b, mut="abs_pow")["fsimc"] - want["fsimc"]) > 1e-6
    _check(_run(ctx, a, b), want, "red | blue")


def test_identity_symmetry_and_a_flat_pair(ctx):
    import _native
    for h, w, cn in ((17, 23, 3), (384, 385, 3), (64, 64, 1)):
        a, b = _case(h, w, cn)
        v, vc = _native.fsim_value(_run(ctx, a, a))
        print(f"{h}x{w}x{cn} self: {v!r} {vc!r}")
        assert abs(v - 1.0) <= 1e-12 and abs(vc - 1.0) <= 1e-12
        ab, ba = _native.fsim_value(_run(ctx, a, b)), _native.fsim_value(_run(ctx, b, a))
        assert ab[0] == pytest.approx(ba[0], rel=1e-12, abs=0) and ab[1] == pytest.approx(ba[1], rel=1e-12, abs=0)
    for cn, value in ((3, 128), (1, 77), (3, 0)):
        flat = np.full((24, 31, 3) if cn == 3 else (24, 31), value, np.uint8)
        rec = _run(ctx, flat, flat)
        v, vc = _native.fsim_value(rec)
        assert math.isnan(v) and math.isnan(vc), (cn, value, rec)


# ---- bits and views --------------------------------------------------------------------------------------------------------------
def test_equal_inputs_give_equal_bits_and_the_workspace_regrows(ctx):
    import _native
    h, w = 32, 45
    a, b = _case(h, w, 3)
    big_a, big_b = _case(384, 385, 3)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        first = ctx.fsim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        second = ctx.fsim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        ctx.assess_u8(db.ptr, w * 3, da.ptr, w * 3, h, w, 3)                # unrelated work on the same stream
        assert _native.fsim_plan(384, 385, 3)["workspace_bytes"] > 8 * _native.fsim_plan(h, w, 3)["workspace_bytes"]
        big = _run(ctx, big_a, big_b)                                       # another pooled size: new filters, maybe a new buffer
        third = ctx.fsim_u8(da.ptr, w * 3, db.ptr, w * 3, h, w, 3)
        assert _bits(first) == _bits(second) == _bits(third)
        assert _bits(big) == _bits(_run(ctx, big_a, big_b))
    finally:
        da.free(); db.free()


@pytest.mark.parametrize("cn", [3, 1, 4])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w = 37, 53
    a, b = _case(h, w, cn)
    dense = _run(ctx, a, b)
    dense_pool = _pool(ctx, a, b, 3)
    for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
        la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, k + 3)
        pa, ptr_a, sa = V.embed(ctx, a, la[0], la[1], fill)
        pb, ptr_b, sb = V.embed(ctx, b, lb[0], lb[1], fill ^ 0xFF)
        try:
            got = ctx.fsim_u8(ptr_a, sa, ptr_b, sb, h, w, cn)
            got_pool = ctx.fsim_pool_u8(ptr_a, sa, ptr_b, sb, h, w, cn, 3)
            # the calls only read: both parents are as they were, inside the views and outside
            ra = V.check_guard(ctx, pa, what="first")
            rb = V.check_guard(ctx, pb, what="second")
        finally:
            pa.free(); pb.free()
        assert _bits(got) == _bits(dense), (V.layout_id(la), V.layout_id(lb))
        assert np.array_equal(got_pool, dense_pool)
        assert np.array_equal(ra.reshape(a.shape), a) and np.array_equal(rb.reshape(b.shape), b)


def test_rows_beyond_4_gib(ctx):
    """166 rows at a stride of 25 MiB + 5 bytes: rows 164 and 165 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w = 166, 48
    a, b = _case(h, w, 3)
    stride = (25 << 20) + 5
    assert (h - 1) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    wide = ctx.alloc(total)
    da = ctx.upload(a)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 2, V.FILLS[1])
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, da.ptr + r * w * 3, w * 3)
        ctx.sync()
        got = ctx.fsim_u8(wide.ptr + V.GUARD, stride, ptr_b, sb, h, w, 3)
        assert _bits(got) == _bits(_run(ctx, a, b))
        _check(got, R.fsim(a, b), "wide stride")
    finally:
        wide.free(); da.free(); pb.free()


def test_refusals_come_before_the_device(ctx):
    import _native
    a, b = _case(17, 23, 3)
    da = ctx.upload(a)
    try:
        with pytest.raises(_native.SrShapeError):
            ctx.fsim_u8(da.ptr, 23 * 3, da.ptr, 23 * 3, 15, 23, 3)
        assert "at least 16" in _native.last_error()
        with pytest.raises(_native.SrShapeError):
            ctx.fsim_u8(da.ptr, 23 * 3 - 1, da.ptr, 23 * 3, 17, 23, 3)
        with pytest.raises(ValueError):
            ctx.fsim_u8(da.ptr, 23 * 2, da.ptr, 23 * 2, 17, 23, 2)
        with pytest.raises(ValueError):
            ctx.fsim_u8(0, 23 * 3, da.ptr, 23 * 3, 17, 23, 3)
        with pytest.raises(_native.SrNativeError):
            ctx.fsim_u8(da.ptr, 2100 * 3, da.ptr, 2100 * 3, 100, 2100, 3)      # refused on the host: nothing is read
        assert "2048" in _native.last_error()
    finally:
        da.free()


# ---- the surface -----------------------------------------------------------------------------------------------------------------
def test_module_methods(ctx):
    import _native
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    a, b = _case(32, 45, 3)
    rec = _run(ctx, a, b)
    out = q.calculate_fsim(a, b, return_parts=True)
    assert sorted(out) == ["fsim", "fsimc", "parts"] and _bits(out["parts"]) == _bits(rec)
    assert (out["fsim"], out["fsimc"]) == _native.fsim_value(rec)
    plain = q.calculate_fsim(a, b)
    assert plain == {"fsim": out["fsim"], "fsimc": out["fsimc"]} and isinstance(plain["fsim"], float)
    want = _ref(32, 45, 3)
    assert plain["fsim"] == pytest.approx(want["fsim"], rel=TOL, abs=0) and plain["fsimc"] == pytest.approx(want["fsimc"], rel=TOL, abs=0)
    da = ctx.upload(a)
    pb, ptr_b, sb = V.embed(ctx, b, 3, 13, V.FILLS[0])
    try:
        assert q.calculate_fsim_device(da.ptr, a.shape, ptr_b, b.shape, stride2=sb) == plain
        dev = q.calculate_fsim_device(da.ptr, a.shape, ptr_b, b.shape, return_parts=True, stride1=45 * 3, stride2=sb)
        assert _bits(dev["parts"]) == _bits(rec)
        with pytest.raises(_native.SrShapeError):
            q.calculate_fsim_device(da.ptr, a.shape, ptr_b, b.shape, stride2=45 * 3 - 1)
    finally:
        da.free(); pb.free()
    ga, gb = _case(64, 64, 1)
    g = q.calculate_fsim(ga, gb)
    assert g["fsim"] == g["fsimc"] == pytest.approx(_ref(64, 64, 1)["fsim"], rel=TOL, abs=0)
    assert q.calculate_fsim(ga[..., None], gb[..., None]) == g
    with pytest.raises(ValueError):
        q.calculate_fsim(a, b[:, :44])
    with pytest.raises(NotImplementedError):
        q.calculate_fsim(a.astype(np.float32), b.astype(np.float32))


def test_pipeline_switch(ctx, rng, tmp_path):
    import json

    import main as sr_main
    from PIL import Image
    import _msssim_ref as M
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("fsim", "fsimc", "fsim_note")
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)                  # default off
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_fsim=True, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "fsim" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert sorted(set(rep) - set(res0.quality_report)) == ["fsim", "fsimc"]
    assert rep["full_reference"] == res0.quality_report["full_reference"]
    assert rep.get("overall_score") == res0.quality_report.get("overall_score")
    fused = np.asarray(Image.open(out))
    q = pipe.quality_module
    ref_img = q.upsample_bicubic(img, fused.shape[:2])
    v = q.calculate_fsim(ref_img, fused)
    assert (rep["fsim"], rep["fsimc"]) == (v["fsim"], v["fsimc"])
    want = R.fsim(ref_img, fused)
    assert rep["fsim"] == pytest.approx(want["fsim"], rel=TOL, abs=0) and rep["fsimc"] == pytest.approx(want["fsimc"], rel=TOL, abs=0)
    assert 0.5 < rep["fsim"] <= 1.0
    on_disk = json.load(open(str(tmp_path / "fsim" / "result_qa_report.json")))
    assert on_disk["fsim"] == rep["fsim"] and on_disk["fsimc"] == rep["fsimc"]
    # the host-array path: the same bits
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(device_resident=False, qa_fsim=True, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert (res_h.quality_report["fsim"], res_h.quality_report["fsimc"]) == (rep["fsim"], rep["fsimc"])
    # refusals and a flat pair: None and a note, no error (the one helper all three paths call, called as they do)
    d_src, d_canvas = ctx.upload(np.ascontiguousarray(img[:6, :48])), ctx.upload(np.ascontiguousarray(ref_img[:12, :96]))
    flat = ctx.upload(np.full((20, 48, 3), 90, np.uint8))
    flat2 = ctx.upload(np.full((40, 96, 3), 90, np.uint8))
    try:
        rep_s = {"kept": 1}
        pipe._fsim(ctx, rep_s, d_src.ptr, (6, 48, 3), d_canvas.ptr, (12, 96, 3))
        assert rep_s["fsim"] is None and rep_s["fsimc"] is None and "at least 16" in rep_s["fsim_note"] and rep_s["kept"] == 1
        rep_w = {}
        pipe._fsim(ctx, rep_w, d_src.ptr, (6, 48, 3), d_canvas.ptr, (100, 2100, 3))     # refused before anything is read
        assert rep_w["fsim"] is None and "2048" in rep_w["fsim_note"]
        rep_f = {}
        pipe._fsim(ctx, rep_f, flat.ptr, (20, 48, 3), flat2.ptr, (40, 96, 3))
        assert rep_f["fsim"] is None and rep_f["fsimc"] is None and "flat" in rep_f["fsim_note"]
        json.dumps(rep_s); json.dumps(rep_w); json.dumps(rep_f)
    finally:
        d_src.free(); d_canvas.free(); flat.free(); flat2.free()
