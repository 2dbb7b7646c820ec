"""GPU: NIQE (sr_niqe_u8, sr_niqe_half_plane; csrc/sr_niqe.hip) against the NumPy / SciPy restatement tests/_niqe_ref.py.

* shapes (each with 1 and 3 channels): 96 x 96 -- one block, with both reflect sides of the 8-tap pass and all four replicate
  borders in it; 96 x 192 -- the smallest scoreable shape; 288 x 288 -- an interior block whose halo is neighbour pixels;
  200 x 301 with crop_border 3 -- 194 x 295 becomes 192 x 288, an odd byte offset and unused right / bottom margins;
* the half plane is equal as integers;
* records: the ten counts equal, the fifteen sums and sum_sigma at 1e-9 relative (all-positive fp64 sums of at most 9216 terms:
  the suite's bar for fp64 reductions); a failure names the block, scale and shift;
* features from the GPU's records: alpha equal (a fit whose restated R lies within 1e-9 relative of a table midpoint would be
  exempt, at most 1 % of fits; tests/test_niqe_host.py shows there is none), the others at 1e-8 relative;
* the score with parameters the restatement fitted from three other seeded images, under the bar measured on the restatement
  (_niqe_ref.score_bar: the change of its score under a relative 1e-9 on its moments, times 100);
* bits: equal inputs give equal bits; a padded, offset view inside a guarded parent (and one whose rows start beyond 2^32
  bytes) gives the dense records and nothing outside the scratch is written;
* the module methods, fit -> save -> load -> score, and the pipeline hook (default off).
parity: BasicSR / pyiqa / MATLAB parity is unpinned (none of them is available offline)."""
import asyncio
import json

import numpy as np
import pytest

import _niqe_ref as R
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
        return ctx.niqe_u8(d.ptr, w * cn, h, w, cn, crop_border=cb)
    finally:
        d.free()


def _check_records(got, want, nbx, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    worst = 0.0
    for s in range(2):
        for b in range(got.shape[1]):
            where = f"{what}: scale {s + 1}, block ({b // nbx}, {b % nbx})"
            for i, name in enumerate(SHIFT_NAMES):
                g, w = got[s, b]["x"][i], want[s, b]["x"][i]
                assert (int(g["n_neg"]), int(g["n_pos"])) == (int(w["n_neg"]), int(w["n_pos"])), f"{where}, {name}: counts"
                for f in ("ssq_neg", "ssq_pos", "sabs"):
                    rel = abs(g[f] - w[f]) / abs(w[f])
                    worst = max(worst, rel)
                    assert rel < SUM_TOL, f"{where}, {name}: {f} {g[f]!r} ref {w[f]!r} rel {rel:.2e}"
            rel = abs(got[s, b]["sum_sigma"] - want[s, b]["sum_sigma"]) / want[s, b]["sum_sigma"]
            worst = max(worst, rel)
            assert rel < SUM_TOL, f"{where}: sum_sigma rel {rel:.2e}"
    print(f"{what}: largest relative difference of a sum {worst:.2e}")


@pytest.mark.parametrize("h,w,cb,cn", CASES, ids=IDS)
def test_half_plane_records_and_features_match_the_restatement(ctx, h, w, cb, cn):
    import _native
    img, want, half, (H, W, nby, nbx), want_feat, fits, _ = R.case(h, w, cb, cn)
    assert _native.niqe_plan(h, w, cn, cb)["size"] == (H, W)
    got = _run(ctx, img, cb)
    got_half = ctx.niqe_half_plane((H // 2, W // 2))
    bad = np.argwhere(got_half != half)
    assert bad.size == 0, f"half plane differs at {bad[:4].tolist()}: {got_half[tuple(bad[0])]} ref {half[tuple(bad[0])]}"
    _check_records(got, want, nbx, f"{h}x{w} cb {cb} cn {cn}")
    # features from the GPU's records
    feat = _native.niqe_features(got)
    a = R.alpha_slots()
    near = (R.midpoint_distance(fits) < MID_TOL).reshape(2, nby * nbx, 5)      # fits in the order scale, block, X
    exempt = np.zeros(feat.shape, dtype=bool)
    exempt[:, a[:5]], exempt[:, a[5:]] = near[0], near[1]
    assert exempt.sum() <= fits.size // 100
    diff_alpha = (feat != want_feat) & ~exempt
    assert not diff_alpha[:, a].any(), (np.argwhere(diff_alpha[:, a])[:4].tolist(), feat[:, a][diff_alpha[:, a]][:4])
    rel = np.abs(feat - want_feat) / np.abs(want_feat)
    rel[:, a] = 0.0
    print(f"largest relative difference of a feature {rel.max():.2e}")
    assert rel.max() < FEAT_TOL, np.unravel_index(rel.argmax(), rel.shape)


def test_score_matches_the_restatement(ctx):
    import _native
    mu, cov = R.pristine()[:2]
    change, bar = R.score_bar()
    print(f"restated score under a relative 1e-9 on its moments moves by {change:.3e}; bar {bar:.3e}")
    seen = []
    for h, w, cb, cn in CASES:
        img, _, _, _, want_feat, *_ = R.case(h, w, cb, cn)
        feat = _native.niqe_features(_run(ctx, img, cb))
        got, want = _native.niqe_score(feat, mu, cov), R.score(want_feat, mu, cov)
        print(f"{h}x{w} cb {cb} cn {cn}: {got!r} ref {want!r} diff {abs(got - want):.3e}")
        if feat.shape[0] < 2:
            assert got != got and want != want
            continue
        assert abs(got - want) < bar, (h, w, cb, cn)
        seen.append(got)
    assert len(seen) == 6 and min(abs(p - q) for k, p in enumerate(seen) for q in seen[k + 1:]) > 100 * bar   # told apart


def test_the_crop_is_the_contiguous_copy_of_the_crop(ctx):
    for cn in (1, 3):
        img = R.case(200, 301, 3, cn)[0]
        got = _run(ctx, img, 3)
        assert _run(ctx, np.ascontiguousarray(img[3:-3, 3:-3]), 0).tobytes() == got.tobytes()
        assert _run(ctx, np.ascontiguousarray(img[3:195, 3:291]), 0).tobytes() == got.tobytes()      # the margins are not read
        other = img.copy()
        other[195:, :] ^= 0xFF
        other[:, 291:] ^= 0xFF
        other[:3, :] ^= 0xFF
        other[:, :3] ^= 0xFF
        assert _run(ctx, other, 3).tobytes() == got.tobytes()


def test_equal_inputs_give_equal_bits(ctx):
    h, w = 288, 288
    img, small = R.case(h, w, 0, 3)[0], R.case(96, 192, 0, 1)[0]
    d, ds = ctx.upload(img), ctx.upload(small)
    try:
        first = ctx.niqe_u8(d.ptr, w * 3, h, w, 3)
        half1 = ctx.niqe_half_plane((144, 144))
        second = ctx.niqe_u8(d.ptr, w * 3, h, w, 3)
        ctx.assess_u8(d.ptr, w * 3, d.ptr, w * 3, h, w, 3)               # unrelated work on the same stream
        ctx.niqe_u8(ds.ptr, 192, 96, 192, 1)                             # another shape through the scratch
        third = ctx.niqe_u8(d.ptr, w * 3, h, w, 3)
        half3 = ctx.niqe_half_plane((144, 144))
    finally:
        d.free(); ds.free()
    assert first.tobytes() == second.tobytes() == third.tobytes() and np.array_equal(half1, half3)


@pytest.mark.parametrize("cn", [3, 1])
def test_strided_guarded_views_give_the_dense_bits(ctx, cn):
    h, w, cb = 200, 301, 3
    img = R.case(h, w, cb, cn)[0]
    dense = _run(ctx, img, cb)
    for k, fill in ((1, V.FILLS[0]), (4, V.FILLS[1]), (6, V.FILLS[0])):
        lay = V.pick(V.LAYOUTS_U8, k)
        p, ptr, stride = V.embed(ctx, img, lay[0], lay[1], fill)
        try:
            got = ctx.niqe_u8(ptr, stride, h, w, cn, crop_border=cb)
            back = V.check_guard(ctx, p, what="image")                  # the call only reads: the parent is as it was
        finally:
            p.free()
        assert got.tobytes() == dense.tobytes(), V.layout_id(lay)
        assert np.array_equal(back.reshape(img.shape), img)


def test_rows_beyond_4_gib(ctx):
    """96 rows at a stride of 44 MiB + 5 bytes: rows 93 to 95 start beyond 2^32 bytes.  A kernel that formed a 32-bit
    row * stride would read them from the wrong place."""
    h, w = 96, 192
    img, want, *_ = R.case(h, w, 0, 3)
    stride = (44 << 20) + 5
    assert (h - 1) * stride >= 1 << 32
    total = V.GUARD + (h - 1) * stride + w * 3 + V.GUARD
    assert total < 8 << 30
    wide, d = ctx.alloc(total), ctx.upload(img)
    try:
        for r in range(h):
            ctx.copy_d2d(wide.ptr + V.GUARD + r * stride, d.ptr + r * w * 3, w * 3)
        ctx.sync()
        got = ctx.niqe_u8(wide.ptr + V.GUARD, stride, h, w, 3)
        dense = ctx.niqe_u8(d.ptr, w * 3, h, w, 3)
    finally:
        wide.free(); d.free()
    assert got.tobytes() == dense.tobytes()
    _check_records(got, want, 2, "wide stride")


def test_module_methods_and_the_parameter_round_trip(ctx, tmp_path):
    import _native
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    mu, cov = R.pristine()[:2]
    params = {"mu_pris_param": mu, "cov_pris_param": cov}
    _, bar = R.score_bar()
    img, _, _, _, want_feat, *_ = R.case(200, 301, 3, 3)
    feat, sharp = q.niqe_features(img, crop_border=3)
    rec = _run(ctx, img, 3)
    assert np.array_equal(feat, _native.niqe_features(rec)) and np.array_equal(sharp, R.sharpness(rec)) and sharp.shape == (6,)
    v = q.calculate_niqe_model(img, params, crop_border=3)
    assert isinstance(v, float) and abs(v - R.score(want_feat, mu, cov)) < bar
    d = ctx.upload(img)
    try:
        assert q.calculate_niqe_model_device(d.ptr, img.shape, params, crop_border=3) == v
    finally:
        d.free()
    assert q.calculate_niqe_model(img, {"mu_pris_param": mu.reshape(1, 36), "cov_pris_param": cov}, crop_border=3) == v
    gray = R.case(288, 288, 0, 1)[0]
    assert abs(q.calculate_niqe_model(gray, params) - R.score(R.case(288, 288, 0, 1)[4], mu, cov)) < bar
    with pytest.raises(ValueError, match="at least 2"):
        q.calculate_niqe_model(R.case(96, 96, 0, 1)[0], params)          # one block has no covariance
    # the stand-in keeps its name and its value: another number
    assert abs(q.calculate_niqe(img) - v) > 1.0
    # fit on the GPU's features -> save -> load -> score
    images = [R.image(seed, *R.FIT_SHAPE, 1) for seed in R.FIT_SEEDS]
    fitted = qam.fit_niqe_model(images)
    assert np.abs(fitted["mu_pris_param"] - mu).max() / np.abs(mu).max() < FEAT_TOL
    assert np.abs(fitted["cov_pris_param"] - cov).max() / np.abs(cov).max() < FEAT_TOL
    for name in ("pristine.npz", "pristine.mat"):
        path = str(tmp_path / name)
        qam.save_niqe_params(path, fitted)
        loaded = qam.load_niqe_params(path)
        assert np.array_equal(loaded["mu_pris_param"], fitted["mu_pris_param"])
        got = q.calculate_niqe_model(img, loaded, crop_border=3)
        assert got == q.calculate_niqe_model(img, fitted, crop_border=3) and abs(got - v) < bar
    with pytest.raises(ValueError, match=r"\b30 blocks"):
        qam.fit_niqe_model(images[:1])


def test_pipeline_hook(ctx, tmp_path):
    import main as sr_main
    import quality_assessment_module as qam
    from PIL import Image
    mu, cov = R.pristine()[:2]
    path = str(tmp_path / "pristine.npz")
    qam.save_niqe_params(path, {"mu_pris_param": mu, "cov_pris_param": cov})
    img = R.image(4242, 100, 120, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    keys = ("niqe_model", "niqe_model_note")
    # default: no key
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert not any(k in res0.quality_report for k in keys)
    # with the option: the device-resident path
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_niqe_params=path, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "niqe" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert sorted(set(rep) - set(res0.quality_report)) == ["niqe_model"]
    assert rep["full_reference"] == res0.quality_report["full_reference"]
    fused = np.asarray(Image.open(out))
    assert fused.shape == (200, 240, 3)
    want = pipe.quality_module.calculate_niqe_model(fused, qam.load_niqe_params(path))
    assert isinstance(rep["niqe_model"], float) and rep["niqe_model"] == want
    # The canvas is not held against the restatement: it has exactly flat (white) 7 x 7 neighbourhoods, where m is 0 up to the
    # rounding of mu and the sign counts follow the summation order -- the generator's guards exist to keep such values out of
    # the comparisons above.  The module method is what is pinned there; the pipeline must hand its canvas to it unchanged.
    assert np.isfinite(want) and want > 0.0
    assert json.load(open(str(tmp_path / "niqe" / "result_qa_report.json")))["niqe_model"] == want
    # the host-array path agrees bit for bit
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_niqe_params=path, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report["niqe_model"] == want and "niqe_model_note" not in res_h.quality_report
    # a canvas with a side below 96, and one with a single block: None and a note, no error (the helper all three paths call)
    for shape, word in (((90, 240, 3), "at least 96"), ((100, 120, 3), "at least 2")):
        d = ctx.upload(np.ascontiguousarray(fused[:shape[0], :shape[1]]))
        try:
            for p in (pipe, pipe_h):
                rep_s = {"kept": 1}
                p._niqe_model(ctx, rep_s, d.ptr, shape)
                assert rep_s["niqe_model"] is None and word in rep_s["niqe_model_note"] and rep_s["kept"] == 1
                json.dumps(rep_s)
        finally:
            d.free()
