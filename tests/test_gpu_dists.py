"""GPU: DISTS (csrc/sr_dists.hip + csrc/sr_dists_host.cpp) against the restatement of tests/_dists_ref.py on seeded SYNTHETIC
weights.

PARITY UNPINNED: DISTS_pytorch, piq, pyiqa, torchvision and the published alpha / beta do not exist offline.  What is checked:
the L2 pooling bit for bit against its NumPy fp32 restatement; the stage-0 sums as exact integers; every per-channel S1 / S2 of
stages 1 .. 5 and the score within 8 x the distance between the fp32 and the fp64 restatement (the project's standing margin
for an fp32 convolution stack with another summation order, tests/test_gpu_srnet.py); tiled == untiled; gray / RGBA; strided
views; the QualityAssessmentModule and pipeline surface.

Measured on an MI355X (max over channels of |S_gpu - S_f64| as a fraction of max over channels of |S_f32 - S_f64|, S1 / S2; the
bar is 8; every case prints its own line under -s): 131x77 5.9 / 2.4, 96x160 1.6 / 7.9, 33x47 0.9 / 0.9, 17x1 1.4 / 1.1, 1x1 1.8 /
exact, two textures 5.1 / 6.1, 37x70 gray 4.2 / 1.5 and 5.5 / 7.4, RGBA 7.1 / 2.4; the score moves by 0.004 of that distance at most.
The margin is thin: in the median over channels the matrix-core convolutions (one fp32 chain over all of cin x 9 per output,
csrc/sr_conv_mfma.h) are 3 x as far from fp64 as torch's blocked CPU GEMM, and the worst channel of either is a nearly dead
one of stage 4 or 5 whose mean^2 is of the order of c1.  DESIGN.md, "DISTS", has the whole record."""
import asyncio

import numpy as np
import pytest

import _dists_ref as dr
import _native
import _views as V

pytestmark = pytest.mark.gpu
MARGIN = 8.0
SHAPES = [(131, 77), (96, 160), (33, 47), (17, 1), (1, 1)]


@pytest.fixture(scope="module")
def weights():
    return _native.dists_synthetic_weights()


@pytest.fixture(scope="module")
def model(ctx, weights):
    m = _native.DistsModel(ctx, weights)
    yield m
    m.close()


@pytest.fixture(scope="module")
def refs(weights):
    """The fp32 and fp64 restatements per case, computed once: key -> (a, b, (score, s1, s2) fp64, (score, s1, s2) fp32)."""
    import torch
    cache = {}

    def get(key, make):
        if key not in cache:
            a, b = make()
            cache[key] = (a, b, dr.dists(a, b, weights, torch.float64), dr.dists(a, b, weights, torch.float32))
        return cache[key]
    return get


def _cn(a):
    return a.shape[2] if a.ndim == 3 else 1


def _sums(ctx, model, a, b, tile=0, lo=0, hi=-1):
    cn = _cn(a)
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        return model.sums(da.ptr, a.shape[1] * cn, db.ptr, b.shape[1] * cn, a.shape[0], a.shape[1], cn, tile, lo, hi)
    finally:
        da.free(); db.free()


def _value(ctx, model, a, b, tile=0):
    s = _sums(ctx, model, a, b, tile)
    return _native.dists_score(s, model.layer_sizes(*a.shape[:2]), model.alpha, model.beta, per_channel=True), s


def _stage0_exact(s, a, b):
    ua, ub = dr.to_rgb(a).astype(np.int64), dr.to_rgb(b).astype(np.int64)
    for c in range(3):
        p, q = ua[:, :, c], ub[:, :, c]
        want = [p.sum(), q.sum(), (p * p).sum(), (q * q).sum(), (p * q).sum()]
        assert s[c].tolist() == [float(x) for x in want], (c, s[c], want)


def _check_against_refs(got, f64, f32, what):
    """Every channel of stages 1 .. 5 and the score under the issue's bar; -> the measured ratios (S1, S2, score)."""
    (v, s1, s2), (v64, a1, a2), (v32, b1, b2) = got, f64, f32
    bar1, bar2 = MARGIN * np.max(np.abs(b1[3:] - a1[3:])), MARGIN * np.max(np.abs(b2[3:] - a2[3:]))
    e1, e2 = np.abs(s1[3:] - a1[3:]), np.abs(s2[3:] - a2[3:])
    ratios = (e1.max() / (bar1 / MARGIN) if bar1 else 0.0, e2.max() / (bar2 / MARGIN) if bar2 else 0.0,
              abs(v - v64) / (max(bar1, bar2) / MARGIN) if max(bar1, bar2) else 0.0)
    print(f"[dists] {what}: max|S1 err| {e1.max():.3e} (f32-f64 {bar1 / MARGIN:.3e}, ratio {ratios[0]:.3f}); "
          f"max|S2 err| {e2.max():.3e} (f32-f64 {bar2 / MARGIN:.3e}, ratio {ratios[1]:.3f}); "
          f"score {v:.9f} vs {v64:.9f} (ratio {ratios[2]:.3f})")
    # stage 0 is integer arithmetic: the same sums, the same float64 formula
    assert np.max(np.abs(s1[:3] - a1[:3])) <= 1e-12 and np.max(np.abs(s2[:3] - a2[:3])) <= 1e-12, what
    assert np.all(e1 <= bar1), (what, int(np.argmax(e1 - bar1)) + 3, e1.max(), bar1)
    assert np.all(e2 <= bar2), (what, int(np.argmax(e2 - bar2)) + 3, e2.max(), bar2)
    dead = (a1 == 1.0) & (a2 == 1.0)                   # dead in fp64 (all five sums zero): exactly 1 here too
    assert np.all(s1[dead] == 1.0) and np.all(s2[dead] == 1.0), what
    assert abs(v - v64) <= max(bar1, bar2), (what, v, v64)
    return ratios


# ---- the L2 pooling, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (7, 8), (65, 130)])
def test_l2pool_bit_for_bit(ctx, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    x = (rng.standard_normal((3, h, w)) * rng.choice([1e-3, 1.0, 30.0], (3, h, w))).astype(np.float32)
    x[rng.random((3, h, w)) < 0.2] = 0.0               # exact zeros ...
    x[1] = 0.0                                         # ... and a whole plane of them: the 1e-12 alone decides
    x[2, -1, :] = np.abs(x[2, -1, :]) + 1.0            # the last row and column are never all zero
    x[2, :, -1] = np.abs(x[2, :, -1]) + 1.0
    got = _native.dists_l2pool(ctx, x)
    want = dr.l2pool_np(x)
    assert got.shape == want.shape == (3, (h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert np.all(got[1] == np.sqrt(np.float32(1e-12)))


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matches_restatement(ctx, model, refs, shape):
    a, b, f64, f32 = refs(shape, lambda: dr.pair(np.random.default_rng(shape[0] * 1000 + shape[1]), *shape))
    got, s = _value(ctx, model, a, b)
    assert model.layer_sizes(*shape) == dr.layer_sizes(*shape)
    _stage0_exact(s, a, b)
    _check_against_refs(got, f64, f32, f"{shape[0]}x{shape[1]}")


def test_distance_between_two_textures_is_meaningful(ctx, model, refs):
    def make():
        rng = np.random.default_rng(77)
        yy, xx = np.mgrid[0:96, 0:128]
        a = np.clip(128 + 90 * np.sin(xx / 3.0) * np.cos(yy / 5.0) + rng.integers(-8, 9, (96, 128)), 0, 255)
        b = np.clip(rng.integers(40, 216, (96, 128)) + 30 * np.sin((xx + yy) / 11.0), 0, 255)
        return (np.repeat(a[..., None], 3, 2).astype(np.uint8) + np.uint8([0, 3, 7])[None, None],
                np.repeat(b[..., None], 3, 2).astype(np.uint8))
    a, b, f64, f32 = refs("textures", make)
    got, _ = _value(ctx, model, a, b)
    _check_against_refs(got, f64, f32, "two textures 96x128")
    assert got[0] > 1e-3 and f64[0] > 1e-3                 # not a sum of ones


# ---- tile streaming ------------------------------------------------------------------------------------------------------------
def test_tiled_equals_untiled(ctx, model):
    a, b = dr.pair(np.random.default_rng(300420), 300, 420)
    whole = _sums(ctx, model, a, b, 0)
    assert whole.shape == (1475, 5) and np.all(whole[:, :4].sum(axis=1) >= 0)
    _stage0_exact(whole, a, b)
    for tile in (64, 128, 304):
        got = _sums(ctx, model, a, b, tile)
        assert np.array_equal(got[:3], whole[:3]), tile                      # integers
        assert np.all(np.abs(got - whole) <= 1e-9 * np.abs(whole)), (tile, np.max(np.abs(got - whole) / np.maximum(np.abs(whole), 1e-300)))
    n = model.tile_count(300, 420, 128)
    assert n == 3 * 4
    parts = [_sums(ctx, model, a, b, 128, lo, hi) for lo, hi in ((0, 5), (5, 7), (7, n))]
    full = _sums(ctx, model, a, b, 128)
    assert np.all(np.abs(sum(parts) - full) <= 1e-12 * np.abs(full))
    assert np.array_equal(sum(parts)[:3], full[:3])


def test_tile_16_own_ranges_of_one_or_two_pixels(ctx, model, refs):
    shape = (131, 77)
    a, b, f64, f32 = refs(shape, lambda: dr.pair(np.random.default_rng(shape[0] * 1000 + shape[1]), *shape))
    assert model.tile_count(131, 77, 16) == 9 * 5
    whole, tiled = _sums(ctx, model, a, b, 0), _sums(ctx, model, a, b, 16)
    assert np.array_equal(tiled[:3], whole[:3])
    assert np.all(np.abs(tiled - whole) <= 1e-9 * np.abs(whole))
    got = _native.dists_score(tiled, model.layer_sizes(*shape), model.alpha, model.beta, per_channel=True)
    _check_against_refs(got, f64, f32, "131x77 tile 16")


# ---- layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [0, 1, 4], ids=["gray2d", "gray", "rgba"])
def test_gray_and_rgba(ctx, model, refs, cn):
    """Gray is repeated and alpha is dropped in the stem and in the stage-0 sums alone (a per-pixel channel select), so the
    smallest shape at which that can go wrong is one with odd sides and more than one 64-lane row.  Two checks: the sums equal,
    bit for bit, those of the same picture handed over as RGB (the same kernels on the same values); and the restatement, under
    the bar of the RGB cases."""
    h, w = 37, 70
    a, b, f64, f32 = refs(("layout", cn), lambda: dr.pair(np.random.default_rng(40 + cn), h, w, cn=cn))
    got, s = _value(ctx, model, a, b)
    _stage0_exact(s, a, b)
    assert np.array_equal(s, _sums(ctx, model, np.ascontiguousarray(dr.to_rgb(a)), np.ascontiguousarray(dr.to_rgb(b))))
    if cn == 4:                                            # the alpha plane is never read
        a2 = a.copy()
        a2[:, :, 3] = 255 - a2[:, :, 3]
        assert np.array_equal(_sums(ctx, model, a2, b), s)
    _check_against_refs(got, f64, f32, f"{h}x{w} cn {cn}")


def test_equal_images_and_equal_bits(ctx, model):
    a, b = dr.pair(np.random.default_rng(9), 70, 90)
    (v, s1, s2), _ = _value(ctx, model, a, a)
    assert np.all(s1 == 1.0) and np.all(s2 == 1.0)         # include/sr_hip.h: every term exactly 1 ...
    assert abs(v) <= 1e-12                                 # ... and the value 1 minus the rounded sum of the normalised weights
    for tile in (0, 64):
        assert np.array_equal(_sums(ctx, model, a, b, tile), _sums(ctx, model, a, b, tile))


@pytest.mark.parametrize("fill", V.FILLS, ids=lambda f: f"fill{f:02x}")
def test_strided_views(ctx, model, fill):
    h, w = 97, 131
    a, b = dr.pair(np.random.default_rng(97131), h, w)
    da, db = ctx.upload(a), ctx.upload(b)
    dense = {tile: model.sums(da.ptr, w * 3, db.ptr, w * 3, h, w, 3, tile) for tile in (0, 64)}
    assert np.all(dense[0][:, 0] >= 0) and dense[0][3:, 0].sum() > 0
    nl = len(V.LAYOUTS_U8)
    for k in range(nl):
        la, lb = V.pick(V.LAYOUTS_U8, k), V.pick(V.LAYOUTS_U8, 5 * k + 3)
        pa, ap, ast = V.embed(ctx, a, la[0], la[1], fill)
        pb, bp, bst = V.embed(ctx, b, lb[0], lb[1], fill)
        for tile, want in dense.items():
            got = model.sums(ap, ast, bp, bst, h, w, 3, tile)
            assert np.array_equal(got, want), f"sr_dists_u8 tile {tile} a {V.layout_id(la)} b {V.layout_id(lb)}"
        pa.free(); pb.free()
    da.free(); db.free()


# ---- module surface ------------------------------------------------------------------------------------------------------------
def test_quality_module_surface(ctx, model, weights, tmp_path, monkeypatch):
    from quality_assessment_module import QualityAssessmentModule
    monkeypatch.delenv("SR_DISTS_WEIGHTS", raising=False)
    a, b = dr.pair(np.random.default_rng(200240), 200, 240)
    plain = QualityAssessmentModule()
    assert plain.dists_model is None
    with pytest.raises(RuntimeError):
        plain.calculate_dists(a, b)
    base = plain.evaluate_full_reference(a, b)
    assert "dists" not in base
    path = tmp_path / "dists.npz"
    np.savez(path, **weights)
    q = QualityAssessmentModule(dists_weights=str(path), dists_tile=128)
    v = q.calculate_dists(a, b)
    (want, _, _), _ = _value(ctx, model, a, b, tile=128)
    assert isinstance(v, float) and v == want and v > 0
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        assert q.calculate_dists_device(da.ptr, a.shape, db.ptr, b.shape) == v
    finally:
        da.free(); db.free()
    with pytest.raises(ValueError):
        q.calculate_dists(a, b[:190])
    with pytest.raises(ValueError):
        q.calculate_dists(a, b[:, :, 0])
    with pytest.raises(NotImplementedError):
        q.calculate_dists(a.astype(np.float32), b.astype(np.float32))
    full = q.evaluate_full_reference(a, b)
    assert full["dists"] == v and sorted(set(full) - set(base)) == ["dists"]
    for k in base:
        assert full[k] == base[k], k                       # every existing key, the overall score included, bit for bit
    monkeypatch.setenv("SR_DISTS_WEIGHTS", str(path))
    env = QualityAssessmentModule()                        # the environment variable is the default
    assert env.dists_model is not None and abs(env.calculate_dists(a, b) - v) <= 1e-9 * v


def test_pipeline_hook(ctx, rng, weights, tmp_path, monkeypatch):
    import json

    import main as sr_main
    from PIL import Image
    import _msssim_ref as M
    monkeypatch.delenv("SR_DISTS_WEIGHTS", raising=False)
    img = M.base_image(rng, 80, 96, 3)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    wpath = str(tmp_path / "dists.npz")
    np.savez(wpath, **weights)
    kw = dict(block_size=64, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4)
    pipe0 = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw))
    pipe0.tiling_module.l2_cache_dir = tmp_path
    res0 = asyncio.run(pipe0.process(src, str(tmp_path / "plain" / "result.png")))
    assert res0.success, res0.error_message
    assert "dists" not in res0.quality_report and "dists" not in res0.quality_report["full_reference"]
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_dists_weights=wpath, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    out = str(tmp_path / "dists" / "result.png")
    res = asyncio.run(pipe.process(src, out))
    assert res.success, res.error_message
    rep = res.quality_report
    assert rep["full_reference"] == res0.quality_report["full_reference"] and rep["commercial"] == res0.quality_report["commercial"]
    assert sorted(set(rep) - set(res0.quality_report)) == ["dists"]
    fused = np.asarray(Image.open(out))
    assert fused.shape == (160, 192, 3)
    from quality_assessment_module import QualityAssessmentModule
    q = QualityAssessmentModule(dists_weights=wpath)
    ref_img = q.upsample_bicubic(img, (160, 192))
    assert isinstance(rep["dists"], float) and rep["dists"] == q.calculate_dists(ref_img, fused) and rep["dists"] > 0
    assert json.load(open(str(tmp_path / "dists" / "result_qa_report.json")))["dists"] == rep["dists"]
    # the host-array path agrees bit for bit
    pipe_h = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(qa_dists_weights=wpath, device_resident=False, **kw))
    res_h = asyncio.run(pipe_h.process(src, str(tmp_path / "host" / "result.png")))
    assert res_h.success, res_h.error_message
    assert res_h.quality_report["dists"] == rep["dists"]
