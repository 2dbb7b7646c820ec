"""CPU: the host side of BRISQUE (csrc/sr_brisque_host.cpp: sr_brisque_plan, sr_brisque_features, sr_brisque_score; every
refusal of sr_brisque_u8 and of the module methods before a device call; the model files; the pipeline option's default)
against the NumPy / SciPy restatement tests/_brisque_ref.py and against libsvm's own predictions
(tests/golden/brisque_svr_sklearn.npz, written by scikit-learn's SVR, which is libsvm).

Bars.  Features: 1e-12 relative (two Gamma implementations, a few ulp each, through at most two square roots and three
products).  Score against libsvm: 1e-10 relative.  NIQE's features keep the bits they had before the Gamma-ratio table moved
into a header (a digest of sr_niqe_features on a restated case, taken from the library before the move)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import _brisque_ref as R
import _native
import _niqe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(h, w, cb, cn) for (h, w, cb) in R.SHAPES for cn in (1, 3)]
NIQE_FEATURES_SHA256 = "e4e171982e30112178d45009b4727ef9cff9a4e0ce07d947ea4b88b66d1df22d"


def test_record_is_the_header_struct():
    assert _native.BRISQUE_RECORD.itemsize == 208 and _native.BRISQUE_RECORD == R.RECORD
    text = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    # the contract's words on parity stand in the header
    assert "PARITY UNPINNED with MATLAB, pyiqa and piq" in text and "allmodel / allrange" in text
    assert "the same multiset of products" in text


def test_plan_and_its_size_rule():
    for h, w in ((16, 16), (17, 31), (64, 64), (65, 127), (200, 301), (11550, 17320)):
        for cb in (0, 1, 3, 52):
            for cn in (1, 3):
                ch, cw = h - 2 * cb, w - 2 * cb
                if min(ch, cw) < 16:
                    with pytest.raises(_native.SrShapeError, match=r"at least 16\b"):
                        _native.brisque_plan(h, w, cn, cb)
                    continue
                p = _native.brisque_plan(h, w, cn, cb)
                h2, w2 = -(-ch // 2), -(-cw // 2)
                assert p["size"] == (ch, cw) and p["half_size"] == (h2, w2), (h, w, cb)
                tiles = lambda a, b: -(-a // 64) * -(-b // 64)               # noqa: E731
                need = h2 * w2 * 4 + (tiles(ch, cw) + tiles(h2, w2)) * 25 * 8
                assert need <= p["scratch_bytes"] <= need + 5 * 256 + 2 * (tiles(ch, cw) // 1024 + 2) * 200, (h, w, cb, p)
    assert _native.load().sr_brisque_plan(16, 16, 3, 0, None, None, None, None, None) == _native.SR_OK   # outputs may be NULL


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=0), "channels"), (dict(crop_border=-1), "crop_border"),
                     (dict(h=0), "h, w"), (dict(w=-5), "h, w")):
        args = dict(h=128, w=128, cn=3, crop_border=2)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.brisque_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    for h, w, cb in ((15, 128, 0), (128, 15, 0), (23, 128, 4), (128, 23, 4), (8, 8, 4), (128, 128, 400)):
        with pytest.raises(_native.SrShapeError, match=r"at least 16\b"):
            _native.brisque_plan(h, w, 3, cb)
    with pytest.raises(ValueError):
        _native.brisque_plan(128, 128, 3, 1.5)
    _native.brisque_plan(24, 24, 3, 4)                                      # exactly 16 left


def test_entry_points_refuse_before_any_device_call():
    """With a null context every valid argument list ends in 'null or destroyed context'; every refusal below comes first."""
    lib = _native.load()
    out = np.zeros(2, dtype=_native.BRISQUE_RECORD)
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, s=384, h=100, w=128, cn=3, cb=2, o=out.ctypes.data_as(C.c_void_p)):
        rc = lib.sr_brisque_u8(None, a, s, h, w, cn, cb, o)
        return rc, _native.last_error()

    rc, msg = call()
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    rc, msg = call(cn=1, s=128)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    for kw in (dict(a=None), dict(o=None)):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cb=-1), "crop_border"), (dict(h=0), "h, w")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
    for kw, word in ((dict(s=383), "stride"), (dict(cn=1, s=127), "stride"), (dict(h=19), "at least 16"), (dict(w=19, s=57), "at least 16"),
                     (dict(cb=43), "at least 16"), (dict(cb=1000), "at least 16")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
    assert lib.sr_brisque_half_plane(None, None) == _native.SR_ERR_INVALID_ARG and "null argument" in _native.last_error()
    assert lib.sr_brisque_half_plane(None, p) == _native.SR_ERR_INVALID_ARG and "context" in _native.last_error()
    # the host-only entry points
    feat = np.zeros(36)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
    assert lib.sr_brisque_features(None, vp(feat)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_brisque_features(vp(out), None) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_brisque_features(vp(out), vp(feat)) == _native.SR_ERR_INVALID_ARG and "no elements" in _native.last_error()
    sv, coef, lo, hi = np.zeros((3, 36)), np.ones(3), -np.ones(36), np.ones(36)
    good = [vp(feat), vp(sv), vp(coef), 3, 0.05, 0.0, vp(lo), vp(hi), -1.0, 1.0]
    assert lib.sr_brisque_score(*good) == 3.0                               # three kernels of 1 at distance 0
    for k in (0, 1, 2, 6, 7):
        args = list(good)
        args[k] = None
        v = lib.sr_brisque_score(*args)
        assert v != v and "null argument" in _native.last_error(), k
    for k, bad, word in ((3, 0, "support vector"), (3, -2, "support vector"), (4, 0.0, "gamma"), (4, -1.0, "gamma"),
                         (4, float("inf"), "gamma"), (4, float("nan"), "gamma")):
        args = list(good)
        args[k] = bad
        v = lib.sr_brisque_score(*args)
        assert v != v and word in _native.last_error(), (k, bad)


@pytest.mark.parametrize("h,w,cb,cn", CASES)
def test_features_match_the_restatement(h, w, cb, cn):
    _, rec, _, want, mids, least = R.case(h, w, cb, cn)
    assert least.min() > 1e-9 and mids.min() > 1e-9                          # what the device test's integer equalities rest on
    feat = _native.brisque_features(rec)
    a = R.ALPHA_SLOTS
    assert np.array_equal(feat[a], want[a])
    rel = np.abs(feat - want) / np.abs(want)
    assert rel.max() < 1e-12, int(rel.argmax())


def test_the_wrap_probe_tells_the_rolls_apart():
    _, want, replicate, zero = R.wrap_probe()
    for s in range(2):
        for i in (2, 3, 4):
            counts = [(int(r[s]["x"][i]["n_neg"]), int(r[s]["x"][i]["n_pos"])) for r in (want, replicate, zero)]
            assert counts[0] != counts[1] and counts[0] != counts[2], (s, i, counts)


def test_half_plane_sizes_round_up_and_are_integral():
    for h, w in ((16, 16), (17, 31), (65, 127)):
        _, half = R.records(_niqe_ref.image(11, h, w, 1))
        assert half.shape == (-(-h // 2), -(-w // 2)) and np.abs(half).max() < 2 ** 25


def test_features_of_degenerate_records():
    rec = R.case(64, 64, 0, 1)[1].copy()
    rec[0]["x"][0] = (0, 0, 0.0, 0.0, 0.0)                                   # a flat plane: no GGD
    rec[0]["x"][2]["n_neg"] = 0
    rec[1]["x"][4]["n_pos"] = 0
    feat, want = _native.brisque_features(rec), R.features(rec)
    nan = np.isnan(feat)
    assert np.array_equal(nan, np.isnan(want))
    assert nan[[0, 1]].all() and nan[6:10].all() and nan[18 + 14:18 + 18].all() and nan.sum() == 10
    assert np.abs(feat[~nan] - want[~nan]).max() < 1e-12
    # zeros count in n: a plane that is half zeros halves E and s2
    one = R.case(64, 64, 0, 1)[1].copy()
    two = one.copy()
    two["n"] *= 2
    f1, f2 = _native.brisque_features(one), _native.brisque_features(two)
    assert f2[1] == f1[1] / 2 and f2[0] != f1[0]
    assert np.abs(f2 - R.features(two)).max() < 1e-12
    assert np.isnan(_native.brisque_score(feat, R.fixture_model()))


def test_score_against_libsvm():
    model = R.fixture_model()
    with np.load(R.GOLDEN, allow_pickle=False) as z:
        probes, answers = z["probe_features"], z["probe_scores"]
    assert probes.shape == (12, 36) and np.ptp(answers) > 10.0
    for f, want in zip(probes, answers):
        got = _native.brisque_score(f, model)
        assert abs(got - want) <= 1e-10 * abs(want), (got, want)
        assert abs(R.score(f, model) - want) <= 1e-10 * abs(want)
    f = probes[0].copy()
    f[:] = np.nan
    assert np.isnan(_native.brisque_score(f, model))                         # all NaN
    f = probes[0].copy()
    f[17] = np.nan
    assert np.isnan(_native.brisque_score(f, model))                         # one NaN
    # a zero-range feature scales to 0 whatever its value
    flat = dict(model)
    flat["feature_min"], flat["feature_max"] = model["feature_min"].copy(), model["feature_max"].copy()
    flat["feature_min"][5] = flat["feature_max"][5] = 0.7
    a, b = probes[1].copy(), probes[1].copy()
    a[5], b[5] = -3.0, 99.0
    assert _native.brisque_score(a, flat) == _native.brisque_score(b, flat)
    k = np.exp(-model["gamma"] * ((model["sv"] - np.where(np.arange(36) == 5, 0.0, -1.0 + 2.0 * (a - model["feature_min"]) /
                                                         (model["feature_max"] - model["feature_min"]))) ** 2).sum(axis=1))
    want = float(model["sv_coef"] @ k - model["rho"])
    assert abs(_native.brisque_score(a, flat) - want) <= 1e-10 * abs(want)
    # the scaler does not clamp: a feature beyond its range moves the score
    c = probes[1].copy()
    c[0] = model["feature_max"][0] + 2.0 * (model["feature_max"][0] - model["feature_min"][0])
    d = c.copy()
    d[0] = model["feature_max"][0]
    assert _native.brisque_score(c, model) != _native.brisque_score(d, model)


def test_wrong_model_shapes():
    model = R.fixture_model()
    for key, bad in (("sv", model["sv"][:, :35]), ("sv", model["sv"][:0]), ("sv_coef", model["sv_coef"][:-1]), ("gamma", 0.0),
                     ("gamma", float("nan")), ("rho", float("inf")), ("feature_min", np.zeros(35)), ("feature_max", np.zeros((2, 18))),
                     ("lower", float("nan"))):
        m = dict(model)
        m[key] = bad
        with pytest.raises(ValueError, match=key):
            _native.check_brisque_model(m)
    for key in ("sv", "sv_coef", "gamma", "rho", "feature_min", "feature_max"):
        m = dict(model)
        del m[key]
        with pytest.raises(ValueError, match="needs the keys"):
            _native.check_brisque_model(m)
    m = dict(model)
    del m["lower"], m["upper"]
    assert _native.check_brisque_model(m)["lower"] == -1.0 and _native.check_brisque_model(m)["upper"] == 1.0
    m["sv_coef"] = model["sv_coef"].reshape(1, -1)                            # libsvm's dual_coef_ layout
    assert np.array_equal(_native.check_brisque_model(m)["sv_coef"], model["sv_coef"])
    with pytest.raises(ValueError, match="features"):
        _native.brisque_score(np.zeros(35), model)
    with pytest.raises(ValueError, match=r"\[2\]"):
        _native.brisque_features(np.zeros(3, dtype=_native.BRISQUE_RECORD))


def _write_libsvm(model, model_path, range_path, svm_type="epsilon_svr", kernel_type="rbf", drop=None):
    with open(model_path, "w") as f:
        f.write(f"svm_type {svm_type}\nkernel_type {kernel_type}\ngamma {model['gamma']!r}\nnr_class 2\n"
                f"total_sv {model['sv'].shape[0]}\nrho {model['rho']!r}\nSV\n")
        for c, row in zip(model["sv_coef"], model["sv"]):
            f.write(repr(float(c)) + " " + " ".join(f"{k + 1}:{float(v)!r}" for k, v in enumerate(row) if v != 0.0) + " \n")
    with open(range_path, "w") as f:
        f.write(f"x\n{model['lower']!r} {model['upper']!r}\n")
        for k in range(36):
            if k != drop:
                f.write(f"{k + 1} {float(model['feature_min'][k])!r} {float(model['feature_max'][k])!r}\n")


def test_model_files(tmp_path):
    import quality_assessment_module as qam
    model = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in R.fixture_model().items()}   # the fixture stays as it is
    model["sv"][3, 7] = 0.0                                                  # a sparse row: absent means 0
    npz, txt, rng = str(tmp_path / "svr.npz"), str(tmp_path / "svr.model"), str(tmp_path / "svr.range")
    qam.save_brisque_model(npz, model)
    a = qam.load_brisque_model(npz)
    _write_libsvm(model, txt, rng)
    b = qam.brisque_model_from_libsvm(txt, rng)
    for key in ("sv", "sv_coef", "feature_min", "feature_max"):
        assert np.array_equal(a[key], model[key]) and np.array_equal(b[key], model[key]), key
    for key in ("gamma", "rho", "lower", "upper"):
        assert a[key] == b[key] == model[key], key
    with np.load(R.GOLDEN, allow_pickle=False) as z:
        f = z["probe_features"][2]
    assert _native.brisque_score(f, a) == _native.brisque_score(f, b) == _native.brisque_score(f, model)
    # lower / upper are optional in the .npz
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: model[k] for k in ("sv", "sv_coef", "gamma", "rho", "feature_min", "feature_max")})
    assert qam.load_brisque_model(bare)["lower"] == -1.0 and qam.load_brisque_model(bare)["upper"] == 1.0
    np.savez(bare, **{k: model[k] for k in ("sv", "sv_coef", "gamma", "feature_min", "feature_max")})
    with pytest.raises(ValueError, match="rho"):
        qam.load_brisque_model(bare)
    pickled = str(tmp_path / "pickled.npz")
    np.savez(pickled, **dict({k: model[k] for k in ("sv_coef", "gamma", "rho", "feature_min", "feature_max")},
                             sv=np.array([{"a": 1}], dtype=object)))
    with pytest.raises(ValueError):
        qam.load_brisque_model(pickled)                                      # allow_pickle=False
    with pytest.raises(ValueError, match=".npz"):
        qam.load_brisque_model(str(tmp_path / "svr.yaml"))
    # a feature absent from the range file was constant in training: it scales to 0
    _write_libsvm(model, txt, rng, drop=4)
    c = qam.brisque_model_from_libsvm(txt, rng)
    assert c["feature_min"][4] == c["feature_max"][4]
    # anything but an RBF epsilon-SVR is refused by name
    for kw, word in ((dict(svm_type="nu_svr"), "nu_svr"), (dict(kernel_type="linear"), "linear"), (dict(svm_type="c_svc"), "c_svc"),
                     (dict(kernel_type="polynomial"), "polynomial")):
        _write_libsvm(model, txt, rng, **kw)
        with pytest.raises(ValueError, match=word):
            qam.brisque_model_from_libsvm(txt, rng)


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    model = R.fixture_model()
    img = np.zeros((40, 48, 3), np.uint8)
    with pytest.raises(ValueError, match="needs the keys"):
        q.calculate_brisque_model(img, {"sv": model["sv"]})
    with pytest.raises(_native.SrShapeError, match="at least 16"):
        q.calculate_brisque_model(img, model, crop_border=13)
    with pytest.raises(_native.SrShapeError, match="at least 16"):
        q.brisque_features(img[:12])
    with pytest.raises(ValueError, match="crop_border"):
        q.brisque_features(img, crop_border=-1)
    with pytest.raises(ValueError, match="3 channels"):
        q.brisque_features(np.zeros((40, 48, 2), np.uint8))
    with pytest.raises(NotImplementedError, match="uint8"):
        q.brisque_features(img.astype(np.float32))                           # float inputs are out of scope
    with pytest.raises(ValueError, match="null device pointer"):
        q.calculate_brisque_model_device(0, (40, 48, 3), model)
    with pytest.raises(_native.SrShapeError, match="at least 16"):
        q.calculate_brisque_model_device(256, (40, 12), model)
    with pytest.raises(ValueError, match="needs the keys"):
        q.calculate_brisque_model_device(256, (40, 48), {})
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_brisque_model(img, model)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_brisque_model_device(256, (40, 48), model)


def test_pipeline_option_defaults_off():
    import main as sr_main
    assert sr_main.PipelineConfig().qa_brisque_model == ""
    text = open(os.path.join(ROOT, "super-resolution-system_amd", "main.py")).read()
    assert "--qa-brisque-model" in text


def test_niqe_features_keep_their_bits():
    """The Gamma-ratio table and its argmin moved from sr_niqe_host.cpp into sr_niqe.h for BRISQUE to share: sr_niqe_features on
    seeded records in _niqe_ref's layout (drawn, not summed, so that their bits do not depend on NumPy's summation order) gives
    the bits it gave before."""
    rec = _seeded_niqe_records()
    assert rec.dtype == _niqe_ref.RECORD
    feat = _native.niqe_features(rec)
    assert np.isfinite(feat).all() and np.unique(feat[:, _niqe_ref.alpha_slots()]).size > 100
    assert hashlib.sha256(feat.tobytes()).hexdigest() == NIQE_FEATURES_SHA256


def _seeded_niqe_records(nblocks: int = 64) -> np.ndarray:
    rng = np.random.default_rng(20130331)
    rec = np.zeros((2, nblocks), dtype=_native.NIQE_RECORD)
    for s in range(2):
        n = (96 >> s) ** 2
        neg = rng.integers(n // 4, 3 * n // 4, size=(nblocks, 5))
        rec[s]["x"]["n_neg"], rec[s]["x"]["n_pos"] = neg, n - neg
        ls, rs = rng.uniform(0.3, 1.2, size=(2, nblocks, 5))
        rec[s]["x"]["ssq_neg"], rec[s]["x"]["ssq_pos"] = neg * ls * ls, (n - neg) * rs * rs
        # E|X| / sqrt(E X^2) of a generalised Gaussian lies in (0.3, 0.95) over the table
        rec[s]["x"]["sabs"] = rng.uniform(0.45, 0.9, size=(nblocks, 5)) * (neg * ls + (n - neg) * rs)
        rec[s]["sum_sigma"] = rng.uniform(5.0, 20.0, size=nblocks) * n
    return rec
