"""GPU: evaluate_commercial / evaluate_no_reference (csrc/sr_commercial.hip) against the NumPy restatement in
tests/_commercial_ref.py, the FFT line lengths of every path, Canny hysteresis stress, determinism and the pipeline's
commercial section."""
import asyncio
import json

import numpy as np
import pytest

import _commercial_ref as R

pytestmark = pytest.mark.gpu


def _qa(**kw):
    import quality_assessment_module as qam
    return qam.QualityAssessmentModule(**kw)


def _img(rng, h, w, cn=3):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(xx / 9.0) + 40 * np.cos(yy / 7.0) + 30 * ((xx // 16 + yy // 16) % 2)
    if cn == 1:
        return np.clip(base + rng.integers(-20, 21, (h, w)), 0, 255).astype(np.uint8)
    img = np.clip(base[..., None] + rng.integers(-40, 41, (h, w, cn)), 0, 255).astype(np.uint8)
    return img


def _close(got, want):
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        assert type(got[k]) in (float, str), (k, type(got[k]))
        if isinstance(want[k], str):
            assert got[k] == want[k], k
        else:
            assert got[k] == pytest.approx(want[k], rel=R.tolerance(k), abs=1e-9 if want[k] == 0 else 0), k


ROIS = [
    {'type': 'text', 'bbox': [3, 2, 40, 30]},
    {'type': 'product', 'bbox': [-5, -3, 50, 40]},                 # negative offset: not subtracted from w, h
    {'type': 'face', 'bbox': [20, 10, 10000, 10000]},              # overflowing
    {'type': 'brand', 'bbox': [1, 1, 17, 9], 'reference_color': (200, 30, 40)},
    {'type': 'brand', 'bbox': [1, 1, 17, 9]},                      # no reference colour: no keys
    {'type': 'face', 'bbox': [5, 5, 0, 10]},                       # zero area: skipped
    {'bbox': [0, 0, 8, 8]},                                        # default type roi_5
    {'type': 'text'},                                              # default bbox: the whole image
]


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (41, 1), (7, 5), (64, 64), (257, 193), (1021, 769)])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_commercial_matches_restatement(rng, h, w, cn):
    img = _img(rng, h, w, cn)
    q = _qa()
    got = q.evaluate_commercial(img, ROIS)
    _close(got, R.evaluate_commercial(img, ROIS))
    json.dumps(got)
    assert q.evaluate_commercial(img, ROIS) == got                 # bitwise reproducible


@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (64, 64), (257, 193)])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_no_reference_matches_restatement(rng, h, w, cn):
    img = _img(rng, h, w, cn)
    got = _qa().evaluate_no_reference(img)
    _close(got, R.evaluate_no_reference(img))
    f32 = R.evaluate_no_reference(img, fp64=False)                 # the reference's float32 reductions
    for k in ("niqe", "brisque"):
        assert got[k] == pytest.approx(f32[k], rel=1e-5), k
    json.dumps(got)


def test_gray_shift_14(rng):
    img = _img(rng, 96, 80)
    _close(_qa(gray_shift=14).evaluate_commercial(img, ROIS[:3]), R.evaluate_commercial(img, ROIS[:3], gray_shift=14))


def test_medium_canvas(rng):
    img = _img(rng, 2970, 4124)
    rois = [{'type': t, 'bbox': [100 * i, 50 * i, 700, 500], 'reference_color': (10, 200, 30)}
            for i, t in enumerate(('text', 'product', 'face', 'brand'))]
    _close(_qa().evaluate_commercial(img, rois), R.evaluate_commercial(img, rois))


def test_reference_helpers_on_device(rng):
    img = _img(rng, 120, 90)
    q = _qa()
    g = R.gray_of(img)
    assert q._calculate_sharpness(img) == pytest.approx(R.sharpness(g), rel=1e-12)
    assert q._calculate_contrast(img) == pytest.approx(R.contrast(g), rel=1e-12)
    assert q._calculate_colorfulness(img) == pytest.approx(R.colorfulness(img), rel=1e-12)
    assert q._calculate_hf_ratio(img) == pytest.approx(R.hf_ratio(g), rel=1e-4)
    assert q._detect_oversharpen(img) == pytest.approx(R.oversharpen(g), rel=1e-12)
    assert q._detect_artifacts(img) == pytest.approx(R.artifact_score(g), rel=1e-12)
    assert q._estimate_noise(img) == pytest.approx(R.noise_level(g), rel=1e-9)
    assert q._calculate_brightness_uniformity(img) == pytest.approx(R.brightness_uniformity(g), rel=1e-12)
    assert q._calculate_texture_score(img) == pytest.approx(R.texture(g), rel=1e-9)
    assert q._calculate_face_naturalness(img) == pytest.approx(R.face_naturalness(img), rel=1e-12)
    assert q._calculate_skin_tone_naturalness(img) == pytest.approx(R.skin_tone(img), rel=1e-12)
    assert q._calculate_delta_e(img, (90, 100, 110)) == pytest.approx(R.delta_e(img, (90, 100, 110)), rel=1e-12)
    assert q.calculate_niqe(img) == pytest.approx(R.niqe(g), rel=1e-9)
    assert q.calculate_brisque(img) == pytest.approx(R.brisque(g), rel=1e-9)


# ---- Canny ---------------------------------------------------------------------------------------------------------------

def _edge_count(img):
    import _native
    ctx = _native.default_context(0)
    d = ctx.upload(img)
    try:
        ints, _ = ctx.commercial_u8(d.ptr, img.shape[1] * (img.shape[2] if img.ndim == 3 else 1), img.shape[0], img.shape[1],
                                    img.shape[2] if img.ndim == 3 else 1, _native.CM_CANNY)
    finally:
        d.free()
    return int(ints[0, 36]), int(ints[0, 37])


def _spiral(n=600, step=12):
    """A one-pixel weak step edge along a square spiral over many 32 x 32 tiles; only its far (inner) end is strong."""
    img = np.full((n, n), 100, np.uint8)
    y0, x0, y1, x1 = 4, 4, n - 5, n - 5
    path = []
    while y1 - y0 > 2 * step and x1 - x0 > 2 * step:
        path += [(y0, x) for x in range(x0, x1)] + [(y, x1) for y in range(y0, y1)]
        path += [(y1, x) for x in range(x1, x0 + step, -1)] + [(y, x0 + step) for y in range(y1, y0 + step, -1)]
        y0, x0, y1, x1 = y0 + step, x0 + step, y1 - step, x1 - step
    for (y, x) in path:
        img[y, x] = 114                                             # weak: a ridge of 14 gives magnitudes 56..112
    ye, xe = path[-1]
    img[ye, xe] = 220                                               # strong at the far end only
    return img, len(path)


def test_canny_spiral_crosses_tiles():
    img, plen = _spiral()
    want = int(R.canny_edges(R.gray_of(img)).sum())
    got, sweeps = _edge_count(img)
    assert got == want and want > plen // 2                         # the whole spiral is reached from its end
    assert sweeps > 2


def test_canny_thresholds_ties_and_borders(rng):
    for k in range(4):
        img = (rng.integers(0, 4, (97, 131)) * (25 if k % 2 else 13)).astype(np.uint8)  # plateaus: NMS ties
        g = R.gray_of(img)
        got, _ = _edge_count(img)
        assert got == int(R.canny_edges(g).sum())
    img = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    g = R.gray_of(img)
    m = np.abs(R.sobel(g, True)[0]) + np.abs(R.sobel(g, True)[1])
    assert (m == 50).any() and (m == 150).any()                      # exactly the thresholds occur
    assert _edge_count(img)[0] == int(R.canny_edges(g).sum())
    ramp = np.tile(np.arange(40, dtype=np.uint8) * 6, (30, 1))       # edges touching every border
    assert _edge_count(ramp)[0] == int(R.canny_edges(R.gray_of(ramp)).sum())


# ---- FFT -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 11, 16, 97, 433, 1021, 4099, 11550, 17320, 32768])
def test_fft_line_lengths(rng, n):
    import _native
    ctx = _native.default_context(0)
    lines = max(1, min(4, 65536 // n))
    x = (rng.standard_normal((lines, n)) + 1j * rng.standard_normal((lines, n))).astype(np.complex64)
    d = ctx.upload(x)
    try:
        ctx.fft_c2c(d.ptr, d.ptr, lines, n)
        y = ctx.download(d.ptr, (lines, n), np.complex64)
    finally:
        d.free()
    want = np.fft.fft(x.astype(np.complex128), axis=1)
    err = np.abs(y - want).max() / np.abs(want).max()
    assert err < 2e-5, err


def test_fft_length_limit():
    import _native
    ctx = _native.default_context(0)
    assert ctx.lib.sr_fft_max_len() == 32768
    d = ctx.alloc(8 * 32769)
    try:
        with pytest.raises(_native.SrNativeError):
            ctx.fft_c2c(d.ptr, d.ptr, 1, 32769)
    finally:
        d.free()
    q = _qa()
    with pytest.raises(NotImplementedError):
        q.evaluate_commercial_device(d.ptr, (1, 32769, 3))          # refused before any device work


# ---- device entry, pipeline ------------------------------------------------------------------------------------------------

def test_device_entry_equals_host_entry(rng):
    import _native
    img = _img(rng, 150, 222)
    q = _qa()
    ctx = q._ctx()
    d = ctx.upload(img)
    h2d, d2h = ctx.h2d_bytes, ctx.d2h_bytes
    try:
        dev = q.evaluate_commercial_device(d.ptr, img.shape, ROIS)
    finally:
        d.free()
    assert (ctx.h2d_bytes, ctx.d2h_bytes) == (h2d, d2h)              # nothing staged through upload / download
    assert dev == q.evaluate_commercial(img, ROIS)


def test_pipeline_commercial_section(rng, tmp_path):
    import main as sr_main
    from PIL import Image
    img = _img(rng, 150, 200)
    src = str(tmp_path / "input.png")
    Image.fromarray(img).save(src)
    rois = [{'type': 'text', 'bbox': [10, 10, 100, 60]}, {'type': 'face', 'bbox': [50, 40, 90, 90]},
            {'type': 'brand', 'bbox': [0, 0, 30, 30], 'reference_color': [120, 130, 140]}]
    sections = []
    for resident in (True, False):
        cfg = sr_main.PipelineConfig(block_size=96, overlap_ratio=0.2, sr_scale=2, num_pyramid_levels=4,
                                     device_resident=resident)
        pipe = sr_main.SuperResolutionPipeline(cfg)
        pipe.tiling_module.l2_cache_dir = tmp_path
        res = asyncio.run(pipe.process(src, str(tmp_path / f"out{int(resident)}.png"), prompt="x", roi_regions=rois))
        assert res.success, res.error_message
        sections.append(res.quality_report['commercial'])
        if resident:
            tr = pipe.transfers
            assert tr["h2d_bytes"] == img.nbytes and tr["d2h_bytes"] <= tr["canvas_bytes"] + 4096
    dev, host = sections
    assert dev == host
    assert 'text_sharpness_0' in dev and 'face_naturalness_1' in dev and 'brand_color_delta_e_2' in dev
    fused = np.asarray(Image.open(str(tmp_path / "out1.png")))
    _close(dev, R.evaluate_commercial(fused, rois))


def test_full_canvas_200mp():
    import torch
    import _native
    h, w = 11550, 17320
    gen = torch.Generator(device="cuda").manual_seed(7)
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    q = _qa()
    ctx = _native.default_context(0)
    torch.cuda.synchronize()
    a = q.evaluate_commercial_device(img.data_ptr(), (h, w, 3), [{'type': 'text', 'bbox': [100, 200, 3000, 2000]}])
    b = q.evaluate_commercial_device(img.data_ptr(), (h, w, 3), [{'type': 'text', 'bbox': [100, 200, 3000, 2000]}])
    assert a == b
    r, gg, bb = (img[..., c].to(torch.int64) for c in range(3))
    g = (r * 9798 + gg * 19235 + bb * 3735 + (1 << 14)) >> 15
    del r, gg, bb
    gd = g.to(torch.float64)
    assert a['global_sharpness'] > 0
    var_g = float(gd.var(unbiased=False))
    # contrast is not a key of the commercial dict: check the Laplacian variance and the hf ratio instead
    P = torch.nn.functional.pad(gd[None, None], (1, 1, 1, 1), mode="reflect")[0, 0]
    lap = P[:-2, 1:-1] + P[2:, 1:-1] + P[1:-1, :-2] + P[1:-1, 2:] - 4 * gd
    assert a['global_sharpness'] == pytest.approx(float(lap.var(unbiased=False)), rel=1e-12)
    del P, lap
    F = torch.fft.fft2(gd).abs()
    F = torch.fft.fftshift(F)
    yy = (torch.arange(h, device="cuda", dtype=torch.int64) - h // 2) ** 2
    xx = (torch.arange(w, device="cuda", dtype=torch.int64) - w // 2) ** 2
    mask = (yy[:, None] + xx[None, :]) > (min(h, w) // 4) ** 2
    hf = float(F[mask].sum() / (F.sum() + 1e-10))
    assert a['high_frequency_ratio'] == pytest.approx(hf, rel=1e-4)
    assert var_g > 0
