"""GPU: BRISQUE (sr_brisque_u8, sr_brisque_half_plane; csrc/sr_brisque.hip) against the NumPy / SciPy restatement
tests/_brisque_ref.py.  T = 64 is the moment kernel's tile side.

* shapes (each with 1 and 3 channels): 16 x 16 -- the minimum: one partial tile owns every wrap and every window touches the
  padding; 64 x 64 -- one full tile; 65 x 127 -- 2 x 2 tiles with one-pixel and T - 1 remainders, odd sides (H2, W2 round up,
  both reflect sides of the 8-tap pass); 192 x 192 -- an interior tile with no wrap and no padding; 200 x 301 with crop_border
  3 -- an odd byte offset and an odd width;
* the half plane is equal as integers, and equal to NIQE's on shapes that are multiples of 96 after the crop (one kernel, two
  instantiations);
* per scale and per X the ten counts are equal and the sums are within 1e-9 relative (all-positive fp64 sums: the suite's bar,
  the one of tests/test_gpu_niqe.py); a failure names scale and shift;
* a wrap probe: an image whose last row and column are far from the first ones; the restatement's counts for the shifts
  (1, 0), (1, 1), (1, -1) differ from those of a replicate-border and a zero-border roll (asserted here), so a wrong wrap
  cannot pass;
* features from the GPU's records: alpha equal (no fit of the restatement lies within 1e-9 relative of a table midpoint:
  asserted, so nothing is exempt), the others at 1e-8 relative;
* the score under the committed libsvm fit (tests/golden/brisque_svr_sklearn.npz) under the bar measured on the restatement
  (_brisque_ref.score_bar: the change of its score under a relative 1e-9 on its moments, times 100, printed); the cases'
  scores lie more than 100 bars apart;
* bits: equal inputs give equal bits across an unrelated call and another shape through the scratch; small -> large -> small
  gives the first bytes again; a padded, offset view inside a guarded parent (and one whose rows start beyond 2^32 bytes)
  gives the dense records and nothing outside is written; the crop equals the contiguous copy of the crop and its margin is
  not read;
* the module methods, save -> load -> score, and the pipeline hook (default off; a note on a 12-pixel canvas).
parity: MATLAB / pyiqa / piq parity is unpinned (none of them is available offline)."""
import asyncio
import json

import numpy as np
import pytest

import _brisque_ref as R
import _views as V

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-9
FEAT_TOL = 1e-8
MID_TOL = 1e-9
SHIFT_NAMES = ("X0 = m", "shift (0, 1)", "shift (1, 0)", "shift (1, 1)", "shift (1, -1)")
CASES = [(h, w, cb, cn) for (h, w, cb) in R.SHAPES for cn in (1, 3)]
IDS = [f"{h}x{w}-cb{cb}-cn{cn}" for h, w, cb, cn in CASES]


def _run(ctx, img, cb=0):
    cn = img.shape[2] if img.ndim == 3 else 1
    h, w = img.shape[:2]
    d = ctx.upload(img)
    try:
        return ctx.brisque_u8(d.ptr, w * cn, h, w, cn, crop_border=cb)
    finally:
        d.free()


def _check_records(got, want, what):
    assert got.shape == want.shape == (2,) and got.dtype == want.dtype, what
    worst = 0.0
    for s in range(2):
        assert int(got[s]["n"]) == int(want[s]["n"]), f"{what}: scale {s + 1}: n"
        for i, name in enumerate(SHIFT_NAMES):
            where = f"{what}: scale {s + 1}, {name}"
            g, w = got[s]["x"][i], want[s]["x"][i]
            assert (int(g["n_neg"]), int(g["n_pos"])) == (int(w["n_neg"]), int(w["n_pos"])), \
                f"{where}: counts {int(g['n_neg'])}, {int(g['n_pos'])} ref {int(w['n_neg'])}, {int(w['n_pos'])}"
            for f in ("ssq_neg", "ssq_pos", "sabs"):
                rel = abs(g[f] - w[f]) / abs(w[f])
                worst = max(worst, rel)
                assert rel < SUM_TOL, f"{where}: {f} {g[f]!r} ref {w[f]!r} rel {rel:.2e}"
    print(f"{what}: largest relative difference of a sum {worst:.2e}")


@pytest.mark.parametrize("h,w,cb,cn", CASES, ids=IDS)
def test_half_plane_records_and_features_match_the_restatement(ctx, h, w, cb, cn):
    import _native
    img, want, half, want_feat, mids, least = R.case(h, w, cb, cn)
    assert least.min() > 0.0 and mids.min() > MID_TOL                   # no X at 0, no fit at a midpoint: nothing is exempt
    plan = _native.brisque_plan(h, w, cn, cb)
    assert plan["size"] == (h - 2 * cb, w - 2 * cb) and plan["half_size"] == half.shape
    got = _run(ctx, img, cb)
    got_half = ctx.brisque_half_plane(plan["half_size"])
    bad = np.argwhere(got_half != half)
    assert bad.size == 0, f"half plane differs at {bad[:4].tolist()}: {got_half[tuple(bad[0])]} ref {half[tuple(bad[0])]}"
    _check_records(got, want, f"{h}x{w} cb {cb} cn {cn}")
    feat = _native.brisque_features(got)
    a = R.ALPHA_SLOTS
    assert np.array_equal(feat[a], want_feat[a]), (feat[a], want_feat[a])
    rel = np.abs(feat - want_feat) / np.abs(want_feat)
    print(f"largest relative difference of a feature {rel.max():.2e}")
    assert rel.max() < FEAT_TOL, int(rel.argmax())


def test_the_roll_wraps_over_the_whole_plane(ctx):
    img, want, replicate, zero = R.wrap_probe()
    for s in range(2):
        for i in (2, 3, 4):                                              # the shifts that read the row above
            counts = [(int(r[s]["x"][i]["n_neg"]), int(r[s]["x"][i]["n_pos"])) for r in (want, replicate, zero)]
            assert counts[0] != counts[1] and counts[0] != counts[2], (s, i, counts)
    _check_records(_run(ctx, img), want, "wrap probe")


@pytest.mark.parametrize("cn", [1, 3])
def test_niqe_and_brisque_keep_the_same_half_plane(ctx, cn):
    """One half-plane kernel (k_mscn_half) serves both metrics: NIQE's instantiation without the clamp and the store guard,
    BRISQUE's with them.  On shapes that are multiples of 96 after the crop both keep the same plane: equal integers.
    (200 x 301 with crop_border 3 is not among them: NIQE trims it to 192 x 288 and reflects at another edge.)"""
    import _niqe_ref
    for h, w, cb in ((96, 96, 0), (96, 192, 0), (288, 288, 0), (102, 198, 3)):
        img = _niqe_ref.image(_niqe_ref.case_seed(h, w, cn), h, w, cn)
        shape = ((h - 2 * cb) // 2, (w - 2 * cb) // 2)
        d = ctx.upload(img)
        try:
            ctx.niqe_u8(d.ptr, w * cn, h, w, cn, crop_border=cb)
            ctx.brisque_u8(d.ptr, w * cn, h, w, cn, crop_border=cb)
        finally:
            d.free()
        niqe_half, brisque_half = ctx.niqe_half_plane(shape), ctx.brisque_half_plane(shape)
        assert niqe_half.dtype == brisque_half.dtype == np.int32 and niqe_half.any()
        bad = np.argwhere(niqe_half != brisque_half)
        assert bad.size == 0, f"{h}x{w} cb {cb}: half planes differ at {bad[:4].tolist()}"


def test_score_matches_the_restatement(ctx):
    import _native
    model = R.fixture_model()
    change, bar = R.score_bar()
    print(f"restated score under a relative 1e-9 on its moments moves by {change:.3e}; bar {bar:.3e}")
    seen = []
    for h, w, cb, cn in CASES:
        img, _, _, want_feat, *_ = R.case(h, w, cb, cn)
        got = _native.brisque_score(_native.brisque_features(_run(ctx, img, cb)), model)
        want = R.score(want_feat, model)
        print(f"{h}x{w} cb {cb} cn {cn}: {got!r} ref {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) < bar, (h, w, cb, cn)
        seen.append(got)
    assert min(abs(p - q) for k, p in enumerate(seen) for q in seen[k + 1:]) > 100 * bar        # told apart


def test_the_crop_is_the_contiguous_copy_of_the_crop(ctx):
    for cn in (1, 3):
        img = R.case(200, 301, 3, cn)[0]
        got = _run(ctx, img, 3)
        assert _run(ctx, np.ascontiguousarray(img[3:-3, 3:-3]), 0).tobytes() == got.tobytes()
        other = img.copy()                                               # the margin is not read
        other[197:, :] ^= 0xFF
        other[:, 298:] ^= 0xFF
        other[:3, :] ^= 0xFF
        other[:, :3] ^= 0xFF
        assert _run(ctx, other, 3).tobytes() == got.tobytes()


def test_equal_inputs_give_equal_bits_and_the_scratch_regrows(ctx):
    import _native
    h, w = 192, 192
    img, small = R.case(h, w, 0, 3)[0], R.case(16, 16, 0, 1)[0]
    fresh = _native.Context(0)                                           # its scratch starts empty: small -> large -> small
    d, ds = fresh.upload(img), fresh.upload(small)
    try:
        s1 = fresh.brisque_u8(ds.ptr, 16, 16, 16, 1)
        hs1 = fresh.brisque_half_plane((8, 8))
        first = fresh.brisque_u8(d.ptr, w * 3, h, w, 3)
        half1 = fresh.brisque_half_plane((96, 96))
        second = fresh.brisque_u8(d.ptr, w * 3, h, w, 3)
        fresh.assess_u8(d.ptr, w * 3, d.ptr, w * 3, h, w, 3)            # unrelated work on the same stream
        s2 = fresh.brisque_u8(ds.ptr, 16, 16, 16, 1)                    # another shape through the scratch
        hs2 = fresh.brisque_half_plane((8, 8))
        third = fresh.brisque_u8(d.ptr, w * 3, h, w, 3)
        half3 = fresh.brisque_half_plane((96, 96))
    finally:
        d.free(); ds.free()
        fresh.close()
    assert first.tobytes() == second.tobytes() == third.tobytes() and np.array_equal(half1, half3)
    assert s1.tobytes() == s2.tobytes() and np.array_equal(hs1, hs2)
    assert first.tobytes() == _run(ctx, img).tobytes()                  # and on another context


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 200, 301, 3
    img = R.case(h, w, cb, cn)[0]
    dense = _run(ctx, img, cb)
    for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
        lay = V.pick(V.LAYOUTS_U8, k)
        p, ptr, stride = V.embed(ctx, img, lay[0], lay[1], fill)
        try:
            got = ctx.brisque_u8(ptr, stride, h, w, cn, crop_border=cb)
            back = V.check_guard(ctx, p, what="image")                  # the call only reads: the parent is as it was
        finally:
            p.free()
        assert got.tobytes() == dense.tobytes(), V.layout_id(lay)
        assert np.array_equal(back.reshape(img.shape), img)


def test_rows_beyond_4_gib(ctx):
    """65 rows at a stride of 65 MiB + 5 bytes: rows 64 on start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w = 65, 127
    img, want, *_ = R.case(h, w, 0, 3)
    stride = (65 << 20) + 5
    assert (h - 1) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    assert total < 8 << 30
    wide, d = ctx.alloc(total), ctx.upload(img)
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, d.ptr + r * w * 3, w * 3)
        ctx.sync()
        got = ctx.brisque_u8(wide.ptr + V.GUARD, stride, h, w, 3)
        dense = ctx.brisque_u8(d.ptr, w * 3, h, w, 3)
    finally:
        wide.free(); d.free()
    assert got.tobytes() == dense.tobytes()
    _check_records(got, want, "wide stride")


def test_module_methods_and_the_model_round_trip(ctx, tmp_path):
    import _native
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    model = R.fixture_model()
    _, bar = R.score_bar()
    img, _, _, want_feat, *_ = R.case(200, 301, 3, 3)
    feat = q.brisque_features(img, crop_border=3)
    assert feat.shape == (36,) and np.array_equal(feat, _native.brisque_features(_run(ctx, img, 3)))
    v = q.calculate_brisque_model(img, model, crop_border=3)
    assert isinstance(v, float) and abs(v - R.score(want_feat, model)) < bar
    d = ctx.upload(img)
    try:
        assert q.calculate_brisque_model_device(d.ptr, img.shape, model, crop_border=3) == v
    finally:
        d.free()
    gray = R.case(65, 127, 0, 1)
    assert abs(q.calculate_brisque_model(gray[0], model) - R.score(gray[3], model)) < bar
    # the stand-in keeps its name and its value: another number
    assert abs(q.calculate_brisque(img) - v) > 1e-3
    # a flat image has no m on either side of 0: a NaN feature, no score
    with pytest.raises(ValueError, match="NaN"):
        q.calculate_brisque_model(np.full((32, 32), 255, np.uint8)[:, :], model)
    path = str(tmp_path / "svr.npz")
    qam.save_brisque_model(path, model)
    loaded = qam.load_brisque_model(path)
    assert np.array_equal(loaded["sv"], model["sv"]) and loaded["rho"] == model["rho"]
    assert q.calculate_brisque_model(img, loaded, crop_border=3) == v


def test_pipeline_hook(ctx, tmp_path):
    import main as sr_main
    import quality_assessment_module as qam
    from PIL import Image
    import _niqe_ref
    path = str(tmp_path / "svr.npz")
    qam.save_brisque_model(path, R.fixture_model())
    img = _niqe_ref.image(4242, 100, 120, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("brisque_model", "brisque_model_note")
    # default: no key
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # with the option: the device-resident path
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_brisque_model=path, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "brisque" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert sorted(set(rep) - set(res0.quality_report)) == ["brisque_model"]
    assert rep["full_reference"] == res0.quality_report["full_reference"]
    fused = np.asarray(Image.open(out))
    assert fused.shape == (200, 240, 3)
    # The canvas is not held against the restatement (it may hold exactly flat 7 x 7 neighbourhoods, where the sign of m is
    # rounding noise): the module method is what is pinned above; the pipeline must hand its canvas to it unchanged.
    want = pipe.quality_module.calculate_brisque_model(fused, qam.load_brisque_model(path))
    assert isinstance(rep["brisque_model"], float) and rep["brisque_model"] == want and np.isfinite(want)
    assert json.load(open(str(tmp_path / "brisque" / "result_qa_report.json")))["brisque_model"] == want
    # the host-array path agrees bit for bit
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_brisque_model=path, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report["brisque_model"] == want and "brisque_model_note" not in res_h.quality_report
    # a 12-pixel canvas: None and a note, no error (the helper all three paths call)
    shape = (12, 240, 3)
    d = ctx.upload(np.ascontiguousarray(fused[:shape[0], :shape[1]]))
    try:
        for p in (pipe, pipe_h):
            rep_s = {"kept": 1}
            p._brisque_model_entry(ctx, rep_s, d.ptr, shape)
            assert rep_s["brisque_model"] is None and "at least 16" in rep_s["brisque_model_note"] and rep_s["kept"] == 1
            json.dumps(rep_s)
    finally:
        d.free()
