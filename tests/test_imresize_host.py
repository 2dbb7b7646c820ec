"""CPU: the host side of MATLAB's bicubic imresize -- sr_imresize_size, sr_imresize_weights and sr_imresize_plan against the
NumPy restatement tests/_imresize_ref.py, the restatement against torch's float64 antialiased bicubic away from the border,
and every refusal of the entry point, the module methods and the pipeline switch before a device call."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _imresize_ref as R
import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    assert "enum sr_imresize_out { SR_IMRESIZE_U8 = 0, SR_IMRESIZE_F32 = 1, SR_IMRESIZE_F64 = 2 }" in text
    assert (_native.IMRESIZE_U8, _native.IMRESIZE_F32, _native.IMRESIZE_F64) == (0, 1, 2)
    assert "PARITY UNPINNED with MATLAB and BasicSR" in text and "+-1 level" in text and "INTER_CUBIC" in text


def test_sizes_are_ceil_in_double():
    assert _native.imresize_size(100, 0.07) == 8 == math.ceil(100 * 0.07)          # 100 * 0.07 = 7.000000000000001
    rnd = np.random.default_rng(11)
    cases = [(100, 0.5), (101, 0.5), (97, 1 / 3), (99, 1 / 3), (7, 1 / 16), (16, 1 / 16), (1, 1 / 16), (1, 16), (300, 4), (37, 1.5),
             (11550, 1 / 8), (17320, 0.25), (50, 1), (64, 0.75)]
    cases += [(int(rnd.integers(1, 20000)), float(rnd.uniform(1 / 16, 16))) for _ in range(300)]
    cases += [(int(rnd.integers(1, 3000)), k / 100) for k in range(7, 100)]         # decimal scales: the floating-point trap
    for n, s in cases:
        assert _native.imresize_size(n, s) == math.ceil(n * s) == R.out_size(n, s), (n, s)
    with pytest.raises(ValueError):
        _native.imresize_size(0, 0.5)
    for s in (1 / 16.5, 16.01, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_native.SrNativeError, match=r"\[1/16, 16\]"):
            _native.imresize_size(10, s)


AXES = [(100, 0.5, True), (101, 0.5, True), (97, 1 / 3, True), (97, 1 / 3, False), (98, 1 / 4, True), (97, 1 / 4, False), (130, 1 / 8, True),
        (97, 1 / 16, True), (64, 0.75, True), (64, 0.75, False), (40, 1, True), (37, 1.5, True), (20, 2, True), (20, 3, True), (20, 4, True),
        (9, 16, True), (5, 1 / 4, True), (1, 1 / 4, True), (1, 4, True), (2, 1 / 16, True), (100, 0.07, True)]


@pytest.mark.parametrize("n,scale,aa", AXES)
def test_weights_and_indices_against_the_restatement(n, scale, aa):
    m = R.out_size(n, scale)
    w, idx = _native.imresize_weights(n, m, scale, aa)
    rw, ridx = R.weights(n, m, scale, aa)
    assert w.shape == rw.shape and w.shape[1] <= _native.IMRESIZE_MAX_TAPS
    assert np.array_equal(idx, ridx)
    assert idx.min() >= 0 and idx.max() < n
    # + - x / floor only; 1e-14 covers another association of the normalising sum over <= 66 terms
    assert np.abs(w - rw).max() <= 1e-14
    sums = np.zeros(m)
    for k in range(w.shape[1]):
        sums = sums + w[:, k]
    assert np.abs(sums - 1.0).max() <= 1e-14


def test_weights_output_size_form_and_tap_count():
    # the axis scale of the output-size form is m / n in double
    for n, m in ((97, 31), (50, 75), (100, 7), (7, 100)):
        w, idx = _native.imresize_weights(n, m, m / n)
        rw, ridx = R.weights(n, m, m / n)
        assert np.array_equal(idx, ridx) and np.abs(w - rw).max() <= 1e-14
    # P = ceil(kw) + 2 bounds the kept taps; at 1/16 it is 66, of which the two outermost are zero for every output
    assert _native.imresize_weights(320, 20, 1 / 16)[0].shape == (20, 64)
    assert _native.imresize_weights(100, 34, 1 / 3)[0].shape[1] <= math.ceil(12) + 2


def test_short_axes_wrap_more_than_once():
    w, idx = _native.imresize_weights(5, 2, 1 / 4)
    rw, ridx = R.weights(5, 2, 1 / 4)
    assert np.array_equal(idx, ridx)
    # output 0: u = 2.5, left = floor(2.5 - 8) = -6, and |8.5 - k| < 8 keeps k = 1 .. 16: the 1-based indices -5 .. 10 over 5
    # samples fold three times, j = (idx - 1) mod 10, j >= 5 -> 9 - j
    assert idx[0].tolist() == [4, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    w1, idx1 = _native.imresize_weights(1, 1, 1 / 4)
    assert np.all(idx1 == 0) and abs(w1.sum() - 1.0) <= 1e-14


def test_identity_and_the_exact_half_taps():
    w, idx = _native.imresize_weights(40, 40, 1.0)
    assert w.shape == (40, 1) and np.all(w == 1.0) and idx[:, 0].tolist() == list(range(40))
    w, idx = _native.imresize_weights(100, 50, 0.5)
    assert w.shape == (50, 8)
    assert np.all(w == np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256)
    j = 2 * np.arange(50)[:, None] - 3 + np.arange(8)[None, :]
    assert np.array_equal(idx, np.where(j < 0, -j - 1, np.where(j >= 100, 199 - j, j)))


def test_weights_refusals():
    lib = _native.load()
    taps = C.c_int(0)
    assert lib.sr_imresize_weights(10, 5, 0.5, 1, 0, None, None, None) == _native.SR_ERR_INVALID_ARG
    buf = np.zeros(5 * 8)
    assert lib.sr_imresize_weights(10, 5, 0.5, 1, 8, C.byref(taps), buf.ctypes.data_as(C.c_void_p), None) == _native.SR_ERR_INVALID_ARG
    ibuf = np.zeros(5 * 8, dtype=np.int32)
    assert lib.sr_imresize_weights(10, 5, 0.5, 1, 7, C.byref(taps), buf.ctypes.data_as(C.c_void_p),
                                   ibuf.ctypes.data_as(C.c_void_p)) == _native.SR_ERR_INVALID_ARG
    assert taps.value == 8 and "8 needed" in _native.last_error()
    with pytest.raises(ValueError, match="neither"):
        _native.imresize_weights(10, 6, 0.5)                                        # neither ceil(n scale) nor m / n
    with pytest.raises(ValueError):
        _native.imresize_weights(0, 1, 0.5)
    with pytest.raises(_native.SrNativeError, match=r"\[1/16, 16\]"):
        _native.imresize_weights(100, 5, 0.05)


def _torch_bicubic(a: np.ndarray, dh: int, dw: int) -> np.ndarray:
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(a.astype(np.float64))[None, None]
    return F.interpolate(t, size=(dh, dw), mode="bicubic", antialias=True, align_corners=False)[0, 0].numpy()


@pytest.mark.parametrize("h,w,dh,dw", [(96, 120, 48, 60), (99, 120, 33, 40), (96, 120, 24, 30), (40, 50, 80, 100), (30, 40, 90, 120),
                                       (64, 96, 48, 72), (60, 80, 90, 120), (96, 80, 24, 40)])
def test_restatement_against_torch_float64_away_from_the_border(h, w, dh, dw):
    """An independent implementation: torch's antialiased bicubic (a = -0.5, float64 on the CPU) agrees with the definition
    away from the border, where torch clamps and MATLAB reflects.  The sizes divide so that torch's scale n / m is the
    intended one; the margin is 3 output pixels for a downscale and 2 s + 2 for an upscale by s."""
    a = np.random.default_rng(h * 1000 + dw).integers(0, 256, (h, w)).astype(np.uint8)
    ref = R.imresize_f64(a, output_shape=(dh, dw))
    got = _torch_bicubic(a, dh, dw)
    my = 3 if dh <= h else math.ceil(2 * dh / h + 2)
    mx = 3 if dw <= w else math.ceil(2 * dw / w + 2)
    assert np.abs(ref - got)[my:dh - my, mx:dw - mx].max() <= 1e-9


def test_restatement_equals_the_half_plane_of_niqe():
    import _niqe_ref as N
    p = np.random.default_rng(5).integers(0, 256, (96, 192)).astype(np.uint8)
    assert np.array_equal(R.imresize_f64(p, 0.5), N.half_plane(p.astype(np.float64)))


def test_plan_order_taps_and_tiles():
    P = _native.imresize_plan
    assert P(200, 300, 3, 0.5, 0.5, 100, 150)["first"] == "vertical"                # a tie: the vertical pass
    assert P(200, 300, 3, 0.25, 0.5, 50, 150)["first"] == "vertical"
    assert P(200, 300, 3, 0.5, 0.25, 100, 75)["first"] == "horizontal"              # the smaller scale first
    assert P(200, 300, 1, 2.0, 0.5, 400, 150)["first"] == "horizontal"
    assert P(200, 300, 4, 100 / 200, 301 / 300, 100, 301)["first"] == "vertical"
    for cn in (1, 3, 4):
        for s in R.SCALES:
            h, w = 97, 131
            dh, dw = R.out_size(h, s), R.out_size(w, s)
            p = P(h, w, cn, s, s, dh, dw)
            assert p["taps"] == (R.weights(h, dh, s)[0].shape[1], R.weights(w, dw, s)[0].shape[1])
            th, tw = p["tile"]
            assert th >= 1 and tw >= 1 and 0 < p["lds_bytes"] <= 48 * 1024, (cn, s, p)
            # the tables: weights (8 bytes), indices (4) and starts (4 per output) of both axes, each section a multiple of 256
            lo = sum(n * t * 12 + n * 4 for n, t in zip((dh, dw), p["taps"]))
            assert lo <= p["scratch_bytes"] <= lo + 6 * 256 and p["scratch_bytes"] % 256 == 0
    # the tile shrinks with the scale: the same LDS budget holds 16 input columns and the apron per output column at 1/16
    assert P(960, 960, 3, 1 / 16, 1 / 16, 60, 60)["tile"][0] < P(960, 960, 3, 0.5, 0.5, 480, 480)["tile"][0]
    lib = _native.load()
    assert lib.sr_imresize_plan(64, 64, 3, 0.5, 0.5, 32, 32, 1, None, None, None, None, None, None, None) == _native.SR_OK


def test_plan_refusals():
    P = _native.imresize_plan
    for cn in (0, 2, 5):
        with pytest.raises(ValueError, match="channels"):
            P(64, 64, cn, 0.5, 0.5, 32, 32)
    for bad in (dict(h=0), dict(w=0), dict(dh=0), dict(dw=-1)):
        kw = dict(h=64, w=64, cn=3, scale_y=0.5, scale_x=0.5, dh=32, dw=32)
        kw.update(bad)
        with pytest.raises(ValueError, match=">= 1"):
            P(**kw)
    with pytest.raises(_native.SrNativeError, match=r"vertical scale .* \[1/16, 16\]"):
        P(640, 64, 3, 1 / 32, 0.5, 20, 32)
    with pytest.raises(_native.SrNativeError, match=r"horizontal scale .* \[1/16, 16\]"):
        P(64, 4, 3, 0.5, 17.0, 32, 68)
    with pytest.raises(ValueError, match="neither"):
        P(64, 64, 3, 0.5, 0.5, 33, 32)


def test_entry_point_refuses_before_any_device_call():
    """No context exists here (the handle is null): a refusal that names anything but the context came first."""
    lib = _native.load()
    src, dst = C.c_void_p(4096), C.c_void_p(8192)

    def call(**kw):
        a = dict(src=src, ss=192, h=64, w=64, cn=3, sy=0.5, sx=0.5, aa=1, out=_native.IMRESIZE_U8, dst=dst, ds=96, dh=32, dw=32)
        a.update(kw)
        rc = lib.sr_imresize_u8(None, a["src"], a["ss"], a["h"], a["w"], a["cn"], a["sy"], a["sx"], a["aa"], a["out"], a["dst"], a["ds"],
                                a["dh"], a["dw"])
        return rc, _native.last_error()

    for kw, code, word in ((dict(src=None), _native.SR_ERR_INVALID_ARG, "null argument"),
                           (dict(dst=None), _native.SR_ERR_INVALID_ARG, "null argument"),
                           (dict(cn=2, ss=128, ds=64), _native.SR_ERR_INVALID_ARG, "channels"),
                           (dict(sy=1 / 17, h=640, ss=192, dh=38), _native.SR_ERR_UNSUPPORTED, "[1/16, 16]"),
                           (dict(sx=16.5), _native.SR_ERR_UNSUPPORTED, "[1/16, 16]"),
                           (dict(ss=191), _native.SR_ERR_SHAPE, "source stride"),
                           (dict(ds=95), _native.SR_ERR_SHAPE, "destination stride"),
                           (dict(out=_native.IMRESIZE_F32, ds=96 * 4 - 1), _native.SR_ERR_SHAPE, "destination stride"),
                           (dict(out=_native.IMRESIZE_F32, ds=96 * 4 + 2), _native.SR_ERR_INVALID_ARG, "multiples of 4"),
                           (dict(out=_native.IMRESIZE_F64, ds=96 * 8, dst=C.c_void_p(8196)), _native.SR_ERR_INVALID_ARG, "multiples of 8"),
                           (dict(out=3), _native.SR_ERR_INVALID_ARG, "out_type"),
                           (dict(dh=31), _native.SR_ERR_INVALID_ARG, "neither"),
                           (dict(h=0), _native.SR_ERR_INVALID_ARG, ">= 1")):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    rc, msg = call()                                                                # everything valid: only now the context is looked at
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg


def test_module_refusals_without_a_device():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()
    img = np.zeros((24, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="exactly one"):
        q.imresize(img)
    with pytest.raises(ValueError, match="exactly one"):
        q.imresize(img, scale=0.5, output_shape=(12, 16))
    with pytest.raises(_native.SrNativeError, match=r"\[1/16, 16\]"):
        q.imresize(img, scale=1 / 20)
    with pytest.raises(ValueError, match="channels"):
        q.imresize(np.zeros((24, 32, 2), np.uint8), scale=0.5)
    with pytest.raises(NotImplementedError):
        q.imresize(img.astype(np.float32), scale=0.5)
    with pytest.raises(ValueError, match="dtype"):
        q.imresize(img, scale=0.5, dtype=np.int16)
    with pytest.raises(ValueError, match="null"):
        q.imresize_device(0, img.shape, 4096, scale=0.5)
    with pytest.raises(ValueError, match="null"):
        q.imresize_device(4096, img.shape, 0, scale=0.5)
    with pytest.raises(ValueError, match="stride"):
        q.imresize_device(4096, img.shape, 8192, scale=0.5, src_stride=95)
    with pytest.raises(ValueError, match="stride"):
        q.imresize_device(4096, img.shape, 8192, scale=0.5, dst_stride=47)
    # mod_crop is a view of the top-left h - h % s by w - w % s
    v = qam.mod_crop(np.arange(7 * 9 * 3, dtype=np.uint8).reshape(7, 9, 3), 4)
    assert v.shape == (4, 8, 3) and v.base is not None
    assert qam.mod_crop(np.zeros((8, 12), np.uint8), 4).shape == (8, 12)
    with pytest.raises(ValueError):
        qam.mod_crop(img, 0)


def test_pipeline_switch_defaults_and_refusals(monkeypatch):
    import main
    assert main.PipelineConfig().benchmark_degrade is False
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    main.SuperResolutionPipeline(main.PipelineConfig(benchmark_degrade=True))      # the stub backend: accepted, no device call
    with pytest.raises(ValueError, match="sr_backend"):
        main.SuperResolutionPipeline(main.PipelineConfig(benchmark_degrade=True), sr_backend=lambda p, t, s: None)
    with pytest.raises(ValueError, match="device_resident"):
        main.SuperResolutionPipeline(main.PipelineConfig(benchmark_degrade=True, device_resident=False))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one GPU"):
        main.SuperResolutionPipeline(main.PipelineConfig(benchmark_degrade=True))
    main.SuperResolutionPipeline(main.PipelineConfig())                             # the switch off: several ranks stay allowed
