"""CPU: the host side of DISTS -- the feature-map sizes and the score of csrc/sr_dists_host.cpp against the NumPy restatement
(tests/_dists_ref.py), weight packing and loading, every refusal of the C ABI that happens before a device call, and the
Python surface without weights.  PARITY UNPINNED (no DISTS_pytorch / piq / pyiqa, no published alpha / beta offline)."""
import ctypes as C

import numpy as np
import pytest

import _dists_ref as dr
import _native

FAKE = 0x1000          # a handle that never was a model or a context: only compared against the live sets, never dereferenced


def _last():
    return _native.last_error()


@pytest.mark.parametrize("h,w", [(1, 1), (17, 1), (1, 17), (2, 3), (16, 16), (31, 33), (32, 48), (131, 77), (96, 160), (300, 420),
                                 (15, 18), (29, 30), (57, 58), (9, 10)])
def test_layer_sizes_are_ceil_halving(h, w):
    got = _native.dists_layer_sizes(h, w)
    want, hh, ww = [(h, w), (h, w)], h, w
    for _ in range(4):
        hh, ww = int(np.ceil(hh / 2)), int(np.ceil(ww / 2))
        want.append((hh, ww))
    assert got == want == dr.layer_sizes(h, w)


def test_layer_sizes_cover_both_parities_at_every_level():
    seen = set()
    for h in range(1, 70):
        for k, (hh, _) in enumerate(_native.dists_layer_sizes(h, 1)[1:5]):
            seen.add((k, hh % 2))                      # the side the next pooling halves
    assert seen == {(k, p) for k in range(4) for p in (0, 1)}


def test_layer_sizes_refusals():
    lib = _native.load()
    out = (C.c_int * 12)()
    assert lib.sr_dists_layer_sizes(0, 5, out) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_layer_sizes(5, -1, out) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_layer_sizes(5, 5, None) == _native.SR_ERR_INVALID_ARG


def _seeded_sums(rng, hw):
    """Sums of synthetic per-channel samples: consistent (variances >= 0) and with the special channels of the issue."""
    s = np.zeros((dr.TOTAL, 5))
    ch = 0
    for k, c in enumerate(dr.CHANNELS):
        n = hw[k][0] * hw[k][1]
        for _ in range(c):
            if k == 0:
                a, b = rng.integers(0, 256, n).astype(np.float64), rng.integers(0, 256, n).astype(np.float64)
            else:
                a = np.maximum(rng.normal(0.3, 1.0, n), 0)
                b = np.maximum(a + rng.normal(0, 0.3, n), 0)
            s[ch] = [a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()]
            ch += 1
    return s


def test_score_matches_numpy(rng):
    hw = dr.layer_sizes(40, 24)
    s = _seeded_sums(rng, hw)
    n1 = hw[1][0] * hw[1][1]
    dead, const, same = 3 + 5, 3 + 6, 3 + 64 + 7
    s[dead] = 0.0                                              # a dead channel: both terms are exactly 1
    s[const] = [0.5 * n1, 0.25 * n1, 0.25 * n1, 0.0625 * n1, 0.125 * n1]     # constants 0.5 and 0.25: zero variances
    s[same, 1], s[same, 3], s[same, 4] = s[same, 0], s[same, 2], s[same, 2]  # a == b on one channel
    alpha, beta = rng.uniform(0, 1, dr.TOTAL).astype(np.float32), rng.uniform(0, 1, dr.TOTAL).astype(np.float32)
    got, g1, g2 = _native.dists_score(s, hw, alpha, beta, per_channel=True)
    want, w1, w2 = dr.score(s, hw, alpha, beta)
    assert np.max(np.abs(g1 - w1)) <= 1e-12 and np.max(np.abs(g2 - w2)) <= 1e-12
    assert abs(got - want) <= 1e-12
    assert g1[dead] == 1.0 and g2[dead] == 1.0
    assert g2[const] == 1.0 and abs(g1[const] - (0.25 + 1e-6) / (0.3125 + 1e-6)) <= 1e-12
    assert g1[same] == 1.0 and g2[same] == 1.0
    assert _native.dists_score(s, hw, alpha, beta) == got      # without the per-channel outputs


def test_score_of_equal_images_is_what_the_header_says(rng):
    hw = dr.layer_sizes(33, 47)
    s = _seeded_sums(rng, hw)
    s[:, 1], s[:, 3], s[:, 4] = s[:, 0], s[:, 2], s[:, 2]
    alpha, beta = rng.uniform(0, 1, dr.TOTAL).astype(np.float32), rng.uniform(0, 1, dr.TOTAL).astype(np.float32)
    v, s1, s2 = _native.dists_score(s, hw, alpha, beta, per_channel=True)
    assert np.all(s1 == 1.0) and np.all(s2 == 1.0)
    assert abs(v) <= 1e-12


def test_score_refusals(rng):
    lib = _native.load()
    hw = np.asarray(dr.layer_sizes(8, 8), np.int32).reshape(-1)
    s = np.zeros((dr.TOTAL, 5))
    one = np.ones(dr.TOTAL, np.float32)
    out = C.c_double()
    args = [s.ctypes.data, hw.ctypes.data, one.ctypes.data, one.ctypes.data, C.byref(out), None, None]
    assert lib.sr_dists_score(*args) == _native.SR_OK
    for i in range(5):
        bad = list(args)
        bad[i] = None
        assert lib.sr_dists_score(*bad) == _native.SR_ERR_INVALID_ARG and "null" in _last()
    zero = np.zeros(dr.TOTAL, np.float32)
    assert lib.sr_dists_score(s.ctypes.data, hw.ctypes.data, zero.ctypes.data, zero.ctypes.data, C.byref(out), None, None) == _native.SR_ERR_INVALID_ARG
    assert "positive total" in _last()
    nan = one.copy()
    nan[3] = np.nan
    assert lib.sr_dists_score(s.ctypes.data, hw.ctypes.data, nan.ctypes.data, one.ctypes.data, C.byref(out), None, None) == _native.SR_ERR_INVALID_ARG
    hw0 = hw.copy()
    hw0[4] = 0
    assert lib.sr_dists_score(s.ctypes.data, hw0.ctypes.data, one.ctypes.data, one.ctypes.data, C.byref(out), None, None) == _native.SR_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        _native.dists_score(np.zeros((10, 5)), dr.layer_sizes(8, 8), one, one)
    with pytest.raises(ValueError):
        _native.dists_score(s, dr.layer_sizes(8, 8), one[:-1], one)


# ---- weights ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return _native.dists_synthetic_weights()


def test_pack_weights_shapes_and_names(weights):
    assert _native.DISTS_CONV_KEYS == dr.CONV_KEYS and _native.DISTS_TOTAL == 1475
    cw, cb, alpha, beta, mean, std = _native.dists_pack_weights(weights)
    assert len(cw) == len(cb) == 13 and mean is None and std is None
    for w, b, (co, ci, k) in zip(cw, cb, _native.DISTS_CONV_SHAPES):
        assert w.shape == (co, ci, k, k) and b.shape == (co,) and w.dtype == np.float32 and w.flags.c_contiguous
    assert alpha.shape == beta.shape == (1475,) and alpha.dtype == np.float32
    assert np.array_equal(alpha, weights["alpha"].reshape(-1))
    again = _native.dists_synthetic_weights()
    assert all(np.array_equal(weights[k], again[k]) for k in weights)          # seeded
    withms = dict(weights, mean=np.array([0.5, 0.5, 0.5]), std=np.array([[0.25, 0.25, 0.25]]))
    _, _, _, _, mean, std = _native.dists_pack_weights(withms)
    assert np.array_equal(mean, np.float32([0.5] * 3)) and np.array_equal(std, np.float32([0.25] * 3))


def test_pack_weights_names_every_missing_key(weights):
    for key in list(weights):
        missing = {k: v for k, v in weights.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            _native.dists_pack_weights(missing)


def test_pack_weights_names_every_wrong_shape(weights):
    for key, v in weights.items():
        bad = dict(weights)
        bad[key] = np.zeros(tuple(np.asarray(v.shape) + 1), np.float32) if key not in ("alpha", "beta") else v.reshape(-1)[:-1]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            _native.dists_pack_weights(bad)
    for name, v in (("mean", np.zeros(4)), ("std", np.zeros(3)), ("mean", np.array([0.1, np.nan, 0.2]))):
        with pytest.raises(ValueError, match=name):
            _native.dists_pack_weights(dict(weights, **{name: v}))


def test_pack_weights_filter_and_totals(weights):
    hann = np.outer([0.25, 0.5, 0.25], [0.25, 0.5, 0.25]).astype(np.float32)
    ok = dict(weights)
    ok["stage2.4.filter"] = np.tile(hann[None, None], (64, 1, 1, 1))
    _native.dists_pack_weights(ok)
    for bad in (np.full((64, 1, 3, 3), 1 / 9, np.float32), np.tile(hann[None, None], (64, 1, 1, 1))[:, :, :2], hann):
        with pytest.raises(ValueError, match=r"stage2\.4\.filter"):
            _native.dists_pack_weights(dict(weights, **{"stage2.4.filter": bad}))
    with pytest.raises(ValueError, match="positive"):
        _native.dists_pack_weights(dict(weights, alpha=np.zeros(1475, np.float32), beta=np.zeros(1475, np.float32)))
    with pytest.raises(ValueError, match="positive"):
        _native.dists_pack_weights(dict(weights, alpha=-weights["alpha"], beta=weights["alpha"]))
    inf = weights["beta"].copy()
    inf.reshape(-1)[7] = np.inf
    with pytest.raises(ValueError, match="beta"):
        _native.dists_pack_weights(dict(weights, beta=inf))


def test_pack_weights_features_fallback_and_npz_round_trip(weights, tmp_path):
    tv = {}
    for k, v in weights.items():
        if k.startswith("stage"):
            _, idx, kind = k.split(".")
            tv[f"features.{idx}.{kind}"] = v
        else:
            tv[k] = v
    a, b = _native.dists_pack_weights(weights), _native.dists_pack_weights(tv)
    for x, y in zip(a[0] + a[1] + [a[2], a[3]], b[0] + b[1] + [b[2], b[3]]):
        assert np.array_equal(x, y)
    mixed = dict(tv)
    mixed["stage1.0.weight"] = weights["stage1.0.weight"] * 2          # the DISTS name wins over the fallback
    assert np.array_equal(_native.dists_pack_weights(mixed)[0][0], weights["stage1.0.weight"] * 2)
    p = tmp_path / "dists.npz"
    np.savez(p, **weights)
    back = _native.load_dists_weights(str(p))
    assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)
    obj = tmp_path / "obj.npz"
    np.savez(obj, alpha=np.array([{"a": 1}], dtype=object))
    with pytest.raises(ValueError):
        _native.load_dists_weights(str(obj))


# ---- C ABI: refused on the host before any device call ---------------------------------------------------------------------
def test_tile_count_and_its_refusals():
    lib = _native.load()
    n = C.c_int(-1)
    assert lib.sr_dists_tile_count(300, 420, 128, C.byref(n)) == _native.SR_OK and n.value == 3 * 4
    assert lib.sr_dists_tile_count(300, 420, 0, C.byref(n)) == _native.SR_OK and n.value == 1
    assert lib.sr_dists_tile_count(300, 420, -5, C.byref(n)) == _native.SR_OK and n.value == 1
    assert lib.sr_dists_tile_count(131, 77, 16, C.byref(n)) == _native.SR_OK and n.value == 9 * 5
    assert lib.sr_dists_tile_count(300, 420, 100, C.byref(n)) == _native.SR_ERR_INVALID_ARG and "multiple of 16" in _last()
    assert lib.sr_dists_tile_count(0, 420, 128, C.byref(n)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_tile_count(300, 420, 128, None) == _native.SR_ERR_INVALID_ARG


def test_abi_refusals_before_any_device_call(weights):
    lib = _native.load()
    cw, cb, _, _, _, _ = _native.dists_pack_weights(weights)
    pw = (C.c_void_p * 13)(*[a.ctypes.data for a in cw])
    pb = (C.c_void_p * 13)(*[a.ctypes.data for a in cb])
    h = C.c_void_p()
    # create: null output, null tables, a null array, a bad std, then the context itself
    assert lib.sr_dists_create(FAKE, pw, pb, None, None, None) == _native.SR_ERR_INVALID_ARG and "null out" in _last()
    assert lib.sr_dists_create(FAKE, None, pb, None, None, C.byref(h)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_create(FAKE, pw, None, None, None, C.byref(h)) == _native.SR_ERR_INVALID_ARG
    hole = (C.c_void_p * 13)(*[a.ctypes.data for a in cw])
    hole[6] = None
    assert lib.sr_dists_create(FAKE, hole, pb, None, None, C.byref(h)) == _native.SR_ERR_INVALID_ARG and "6" in _last()
    zero_std = np.array([0.2, 0.0, 0.2], np.float32)
    assert lib.sr_dists_create(FAKE, pw, pb, None, zero_std.ctypes.data, C.byref(h)) == _native.SR_ERR_INVALID_ARG and "std" in _last()
    assert lib.sr_dists_create(None, pw, pb, None, None, C.byref(h)) == _native.SR_ERR_INVALID_ARG and "context" in _last()
    assert lib.sr_dists_create(FAKE, pw, pb, None, None, C.byref(h)) == _native.SR_ERR_INVALID_ARG and "context" in _last()
    assert not h.value
    # forward: every argument refusal, then the model handle (a pointer that is not a live model is never dereferenced)
    out = np.zeros((1475, 5))
    img = 0x2000

    def u8(model=FAKE, a=img, sa=40 * 3, b=img, sb=40 * 3, hh=30, ww=40, cn=3, tile=0, sums=out.ctypes.data):
        return lib.sr_dists_u8(model, a, sa, b, sb, hh, ww, cn, tile, 0, -1, sums)

    assert u8(a=None) == _native.SR_ERR_INVALID_ARG and "null argument" in _last()
    assert u8(b=None) == _native.SR_ERR_INVALID_ARG and "null argument" in _last()
    assert u8(sums=None) == _native.SR_ERR_INVALID_ARG and "null argument" in _last()
    assert u8(cn=2) == _native.SR_ERR_INVALID_ARG and "channels" in _last()
    assert u8(hh=0) == _native.SR_ERR_INVALID_ARG
    assert u8(tile=40) == _native.SR_ERR_INVALID_ARG and "multiple of 16" in _last()
    assert u8(sa=40 * 3 - 1) == _native.SR_ERR_SHAPE and "stride" in _last()
    assert u8(sb=40 * 3 - 1) == _native.SR_ERR_SHAPE and "stride" in _last()
    assert u8(cn=4, sa=40 * 4, sb=40 * 3) == _native.SR_ERR_SHAPE
    assert u8() == _native.SR_ERR_INVALID_ARG and "destroyed model" in _last()
    assert u8(model=None) == _native.SR_ERR_INVALID_ARG and "destroyed model" in _last()
    assert lib.sr_dists_destroy(None) == _native.SR_OK and lib.sr_dists_destroy(FAKE) == _native.SR_OK     # never live: a no-op
    # the pooling probe
    assert lib.sr_dists_l2pool_f32(FAKE, None, 3, 4, 4, img) == _native.SR_ERR_INVALID_ARG and "null argument" in _last()
    assert lib.sr_dists_l2pool_f32(FAKE, img, 3, 4, 4, None) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_l2pool_f32(FAKE, img, 0, 4, 4, img) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_l2pool_f32(FAKE, img, 3, 0, 4, img) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_dists_l2pool_f32(FAKE, img, 3, 4, 4, img) == _native.SR_ERR_INVALID_ARG and "context" in _last()
    assert not np.any(out)


# ---- Python surface without weights ------------------------------------------------------------------------------------------
def test_module_without_weights(monkeypatch):
    from quality_assessment_module import QualityAssessmentModule
    monkeypatch.delenv("SR_DISTS_WEIGHTS", raising=False)
    q = QualityAssessmentModule()
    assert q.dists_model is None and q.dists_tile == 4096
    a = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(RuntimeError):
        q.calculate_dists(a, a)
    with pytest.raises(RuntimeError):
        q.calculate_dists_device(0x1000, (8, 8, 3), 0x1000, (8, 8, 3))
    # (evaluate_full_reference runs on the GPU: tests/test_gpu_dists.py checks that it has no 'dists' key without weights)


def test_pipeline_config_default():
    from main import PipelineConfig
    assert PipelineConfig().qa_dists_weights == ""
