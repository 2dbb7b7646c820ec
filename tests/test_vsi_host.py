"""CPU: the host side of VSI (csrc/sr_vsi_host.cpp) against the NumPy / SciPy restatement tests/_vsi_ref.py, and the
restatement against its own mutants.

* the plan: F on both sides of 384 and 640, the pooled sizes;
* the triangle resize weights at 1e-15: rows sum to 1, scale 1 is the identity, 2000 -> 256 has 18 taps, 256 -> 16 has 34;
* LG and SD at 1e-15;
* sr_vsi_host_u8 (the kernels' formulation: composite pooling tables, no stored full-resolution map) against the restatement
  (the literal order) below 1e-11 relative on the shapes tests/test_gpu_vsi.py uses;
* sr_vsi_value (ratio, NaN) and sr_vsi_chroma_weight (the negative branch);
* identity, symmetry, a flat pair, every refusal;
* mutants: each deliberate mistake moves the restatement's value beyond the GPU test's bar (1e-9 relative), so that bar tells
  the definition from its near misses."""
import math

import numpy as np
import pytest

import _native
import _vsi_ref as R

BAR = 1e-9          # tests/test_gpu_vsi.py: TOL
HOST_BAR = 1e-11
SHAPES = [(16, 16), (17, 33), (16, 2000), (2000, 16), (255, 256), (256, 256), (256, 257), (257, 255), (383, 400), (384, 400), (640, 641)]


@pytest.mark.parametrize("side,F", [(383, 1), (384, 2), (639, 2), (640, 3), (16, 1), (128, 1)])
def test_f_and_the_pooled_size(side, F):
    for h, w in ((side, side + 301), (side + 77, side)):
        p = _native.vsi_plan(h, w, 3)
        assert p["F"] == F == R.auto_f(h, w)
        assert p["size"] == (-(-h // F), -(-w // F))
        assert p["workspace_bytes"] > 6 * 8 * p["size"][0] * p["size"][1] + 12 * 65536 * 8
        assert _native.vsi_plan(h, w, 4) == p


@pytest.mark.parametrize("n_in,n_out", [(2000, 256), (256, 2000), (256, 16), (16, 256), (255, 256), (256, 255), (257, 256), (256, 257),
                                        (256, 256), (14142, 256), (256, 641), (33, 256), (256, 17)], ids=lambda v: str(v))
def test_resize_weights_match_the_restatement(n_in, n_out):
    w, idx = _native.vsi_resize_weights(n_in, n_out)
    rw, ridx = R.axis_weights(n_in, n_out)
    assert w.shape == rw.shape and np.array_equal(idx, ridx)
    assert np.abs(w - rw).max() <= 1e-15
    # each weight is a quotient by the row's sum, rounded once (half an ulp of a value below 1), and numpy's sum rounds each
    # of its additions of a partial sum below 1: at most one ulp of 1 per tap
    assert np.abs(w.sum(axis=1) - 1).max() <= w.shape[1] * 2.3e-16 and (w >= 0).all()
    assert idx.min() >= 0 and idx.max() < n_in


def test_resize_tap_counts_and_the_identity():
    assert _native.vsi_resize_weights(2000, 256)[0].shape == (256, 18)
    assert _native.vsi_resize_weights(256, 16)[0].shape == (16, 34)
    assert _native.vsi_resize_weights(14142, 256)[0].shape[1] == math.ceil(2 * 14142 / 256) + 2      # P: no tap is trimmed
    w, idx = _native.vsi_resize_weights(256, 256)
    assert w.shape == (256, 4) and ((w == 1).sum(axis=1) == 1).all() and ((w == 0).sum(axis=1) == 3).all()
    assert np.array_equal(idx[w == 1], np.arange(256)) and np.array_equal(R.axis_matrix(256, 256), np.eye(256))
    # the dense matrix of the rule resizes a ramp to a ramp (away from the reflected border)
    m = R.axis_matrix(256, 641)
    ramp = m @ np.arange(256.0)
    assert np.abs(np.diff(ramp[5:-5]) - 256 / 641).max() <= 1e-12


def test_filter_planes_match_the_restatement():
    f = _native.vsi_filter()
    assert np.abs(f["lg"] - R.log_gabor()).max() <= 1e-15
    assert np.abs(f["sd"] - R.centre_prior()).max() <= 1e-15
    assert f["lg"][0, 0] == 0 and f["lg"].max() <= 1.0 and f["lg"].min() == 0.0
    assert f["lg"][128, 128] == 0                       # beyond the mask the radius is 0, the filter too
    assert f["sd"].max() == f["sd"][127, 127] == 1.0    # the 1-based centre 128


def test_value_and_chroma_weight():
    assert _native.vsi_value({"sum_s": 3.0, "sum_w": 4.0}) == 0.75
    assert math.isnan(_native.vsi_value({"sum_s": 0.0, "sum_w": 0.0}))
    assert math.isnan(_native.vsi_value({"sum_s": float("nan"), "sum_w": 1.0}))
    for z in (1.0, 0.27, -0.28, -1e-9, 0.0):
        assert _native.vsi_chroma_weight(z) == pytest.approx(float(np.real(complex(z) ** 0.02)), rel=1e-15, abs=0), z
    assert _native.vsi_chroma_weight(-0.28) == pytest.approx(0.28 ** 0.02 * math.cos(0.02 * math.pi), rel=1e-15)
    assert _native.vsi_chroma_weight(-0.28) < 0.28 ** 0.02 * 0.999


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_host_matches_the_restatement(h, w):
    a, b = R.case(h, w)
    want, got = R.vsi(a, b), _native.vsi_host(a, b)
    assert got["F"] == want["F"] and got["size"] == tuple(want["size"]) and got["count"] == want["size"][0] * want["size"][1]
    d = {k: _rel(got[k], want[k]) for k in ("sum_s", "sum_w", "a_range", "b_range", "vs_range")}
    d["value"] = _rel(_native.vsi_value(got), want["value"])
    print(h, w, {k: f"{v:.2e}" for k, v in d.items()})
    assert max(d.values()) < HOST_BAR, d
    # the a and b minima are not one pixel's (where SC would be 0 and the map's minimum with it)
    s = want["sdsp"][0]
    assert np.argmin(s["lab"][1]) != np.argmin(s["lab"][2])


def test_four_channels_and_strides_on_the_host():
    a, b = R.case(17, 33)
    a4, b4 = R.case(17, 33, 4)
    want = _native.vsi_host(a, b)
    got = _native.vsi_host(a4, b4)
    wide = np.zeros((17, 40, 3), np.uint8)
    wide[:, :33] = a
    view = _native.vsi_host(wide[:, :33], b)
    for k in ("sum_s", "sum_w"):
        assert got[k] == want[k] == view[k]


def test_identity_symmetry_and_a_flat_pair():
    for h, w in ((17, 33), (384, 400)):
        a, b = R.case(h, w)
        assert abs(_native.vsi_value(_native.vsi_host(a, a)) - 1.0) <= 1e-12
        assert abs(R.vsi(a, a)["value"] - 1.0) <= 1e-12
        ab, ba = _native.vsi_host(a, b), _native.vsi_host(b, a)
        assert _native.vsi_value(ab) == pytest.approx(_native.vsi_value(ba), rel=1e-12, abs=0)
    # black: every resized sample is exactly 0, so a and b are exactly flat and the value is 0 / 0
    flat = np.zeros((24, 31, 3), np.uint8)
    assert math.isnan(_native.vsi_value(_native.vsi_host(flat, flat))) and math.isnan(R.vsi(flat, flat)["value"])
    a, _ = R.case(24, 31)
    assert math.isnan(_native.vsi_value(_native.vsi_host(a, flat)))


def test_refusals():
    for cn in (0, 2, 5):
        with pytest.raises(ValueError):
            _native.vsi_plan(64, 64, cn)
    with pytest.raises(ValueError):
        _native.vsi_plan(0, 64, 3)
    with pytest.raises(_native.SrNativeError):
        _native.vsi_plan(64, 64, 1)
    assert "colour" in _native.last_error()
    for h, w in ((15, 64), (64, 15)):
        with pytest.raises(_native.SrShapeError):
            _native.vsi_plan(h, w, 3)
        assert "at least 16" in _native.last_error()
    with pytest.raises(_native.SrNativeError):
        _native.vsi_plan(65700, 70000, 3)               # F = 257
    assert "256" in _native.last_error()
    assert _native.vsi_plan(65600, 70000, 3)["F"] == 256
    with pytest.raises(_native.SrNativeError):
        _native.vsi_plan(64, (1 << 20) + 1, 3)
    with pytest.raises(ValueError):
        _native.vsi_resize_weights(0, 16)
    with pytest.raises(ValueError):
        _native.vsi_resize_weights(16, 0)
    a, b = R.case(17, 33)
    with pytest.raises(ValueError):
        _native.vsi_host(a, b[:, :32])
    with pytest.raises(_native.SrNativeError):
        _native.vsi_host(a[..., 0], b[..., 0])
    with pytest.raises(_native.SrShapeError):
        _native.vsi_host(a[:15], b[:15])
    with pytest.raises(ValueError):
        _native.vsi_host(a.astype(np.float32), b.astype(np.float32))
    if _native.device_count() == 0:                     # without a device the compute entries fail loudly
        with pytest.raises(_native.SrNativeError):
            _native.Context(0)


# py_pool shows at an even F only (for an odd F both conventions centre the window on the sample)
MUTANTS = [(m, s) for m in ("sigma_c", "no_mask", "centre", "no_mat2gray", "abs_pow", "no_antialias")
           for s in ((16, 16), (17, 33), (384, 400), (640, 641))] + [("py_pool", (384, 400)), ("py_pool", (512, 600))]


@pytest.mark.parametrize("mut,shape", MUTANTS, ids=[f"{m}-{s[0]}x{s[1]}" for m, s in MUTANTS])
def test_mutants_move_the_value_beyond_the_bar(mut, shape):
    a, b = R.case(*shape)
    good, bad = R.vsi(a, b), R.vsi(a, b, mut=mut)
    rel = abs(bad["value"] / good["value"] - 1)
    print(mut, shape, good["value"], bad["value"], rel)
    if mut == "abs_pow":
        assert good["min_sc"] < 0
    assert rel > BAR
