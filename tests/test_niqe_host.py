"""CPU: the host side of NIQE (csrc/sr_niqe_host.cpp: sr_niqe_plan, sr_niqe_features, sr_niqe_fit, sr_niqe_score; every
refusal of sr_niqe_u8 and of the module methods before a device call; the parameter files; the pipeline option's default)
against the NumPy / SciPy restatement tests/_niqe_ref.py, and the guards of that restatement's image generator.

Bars.  Features: 1e-12 relative (two Gamma implementations, a few ulp each, through at most a square root and a product).
Fit: 1e-12 (a mean and a covariance of 90 rows).  Score: measured on the restatement, not on the code under test -- its moments
moved by a seeded relative 1e-9, the largest change of its score over the scoreable cases, times 100 (ten for the distance
between two correct eigen-solvers, ten for headroom); R.score_bar() does it and the test prints both figures."""
import ctypes as C
import os

import numpy as np
import pytest

import _native
import _niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(h, w, cb, cn) for (h, w, cb) in R.SHAPES for cn in (1, 3)]


def test_records_are_the_header_structs():
    assert C.sizeof(_native.NiqeMoments) == 40 and C.sizeof(_native.NiqeBlock) == 208
    assert _native.NIQE_RECORD.itemsize == 208 and _native.NIQE_RECORD == R.RECORD
    text = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    # the contract's words on parity stand in the header
    assert "PARITY UNPINNED with BasicSR, pyiqa and MATLAB" in text and "niqe_pris_params.npz" in text


def test_plan_against_closed_forms():
    for h, w in ((96, 96), (97, 191), (200, 301), (288, 288), (11550, 17320)):
        for cb in (0, 1, 3, 52):
            for cn in (1, 3):
                ch, cw = h - 2 * cb, w - 2 * cb
                if min(ch, cw) < 96:
                    with pytest.raises(_native.SrShapeError, match=r"at least 96\b"):
                        _native.niqe_plan(h, w, cn, cb)
                    continue
                p = _native.niqe_plan(h, w, cn, cb)
                nby, nbx = ch // 96, cw // 96
                assert p["blocks"] == (nby, nbx) and p["size"] == (96 * nby, 96 * nbx), (h, w, cb)
                need = 48 * nby * 48 * nbx * 4 + 2 * nby * nbx * 208
                assert need <= p["scratch_bytes"] <= need + 2 * 256, (h, w, cb, p)
    assert _native.load().sr_niqe_plan(96, 96, 3, 0, None, None, None, None, None) == _native.SR_OK     # outputs may be NULL


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=0), "channels"), (dict(crop_border=-1), "crop_border"),
                     (dict(h=0), "h, w"), (dict(w=-5), "h, w")):
        args = dict(h=128, w=128, cn=3, crop_border=2)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.niqe_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    for h, w, cb in ((95, 128, 0), (128, 95, 0), (103, 128, 4), (128, 103, 4), (8, 8, 4), (128, 128, 400)):
        with pytest.raises(_native.SrShapeError, match=r"at least 96\b"):
            _native.niqe_plan(h, w, 3, cb)
    with pytest.raises(ValueError):
        _native.niqe_plan(128, 128, 3, 1.5)
    _native.niqe_plan(104, 104, 3, 4)                                      # exactly 96 left


def test_entry_points_refuse_before_any_device_call():
    """With a null context every valid argument list ends in 'null or destroyed context'; every refusal below comes first."""
    lib = _native.load()
    out = (_native.NiqeBlock * 2)()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, s=384, h=100, w=128, cn=3, cb=2, o=C.cast(out, C.c_void_p)):
        rc = lib.sr_niqe_u8(None, a, s, h, w, cn, cb, o)
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
    for kw, word in ((dict(s=383), "stride"), (dict(cn=1, s=127), "stride"), (dict(h=99), "at least 96"), (dict(w=99, s=297), "at least 96"),
                     (dict(cb=3), "at least 96"), (dict(cb=1000), "at least 96")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
    assert lib.sr_niqe_half_plane(None, None) == _native.SR_ERR_INVALID_ARG and "null argument" in _native.last_error()
    assert lib.sr_niqe_half_plane(None, p) == _native.SR_ERR_INVALID_ARG and "context" in _native.last_error()
    # the host-only entry points
    feat, mu, cov = np.zeros((2, 36)), np.zeros(36), np.zeros((36, 36))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
    assert lib.sr_niqe_features(None, 1, vp(feat)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_niqe_features(C.cast(out, C.c_void_p), 1, None) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_niqe_features(C.cast(out, C.c_void_p), 0, vp(feat)) == _native.SR_ERR_INVALID_ARG
    off = np.array([0, 2], dtype=np.int64)
    sharp = np.ones(2)
    used = C.c_int64(-1)
    for args in ((None, vp(sharp), vp(off), 1, 0.75, vp(mu), vp(cov)), (vp(feat), None, vp(off), 1, 0.75, vp(mu), vp(cov)),
                 (vp(feat), vp(sharp), None, 1, 0.75, vp(mu), vp(cov)), (vp(feat), vp(sharp), vp(off), 1, 0.75, None, vp(cov)),
                 (vp(feat), vp(sharp), vp(off), 1, 0.75, vp(mu), None), (vp(feat), vp(sharp), vp(off), 0, 0.75, vp(mu), vp(cov)),
                 (vp(feat), vp(sharp), vp(off), 1, 1.0, vp(mu), vp(cov)), (vp(feat), vp(sharp), vp(off), 1, -0.1, vp(mu), vp(cov)),
                 (vp(feat), vp(sharp), vp(off), 1, float("nan"), vp(mu), vp(cov)),
                 (vp(feat), vp(sharp), vp(np.array([1, 2], dtype=np.int64)), 1, 0.75, vp(mu), vp(cov)),
                 (vp(feat), vp(sharp), vp(np.array([0, 2, 1], dtype=np.int64)), 2, 0.75, vp(mu), vp(cov))):
        assert lib.sr_niqe_fit(*args, C.byref(used)) == _native.SR_ERR_INVALID_ARG, args
    for args in ((None, 2, vp(mu), vp(cov)), (vp(feat), 2, None, vp(cov)), (vp(feat), 2, vp(mu), None)):
        v = lib.sr_niqe_score(*args)
        assert v != v and "null argument" in _native.last_error()


def test_wrong_parameter_shapes():
    import quality_assessment_module as qam
    mu, cov = np.zeros(36), np.eye(36)
    good = {"mu_pris_param": mu, "cov_pris_param": cov}
    assert qam.check_niqe_params(good)["mu_pris_param"].shape == (36,)
    assert qam.check_niqe_params({"mu_pris_param": mu.reshape(1, 36), "cov_pris_param": cov})["mu_pris_param"].shape == (36,)
    for bad in ({"mu_pris_param": np.zeros(35), "cov_pris_param": cov}, {"mu_pris_param": np.zeros((36, 1)), "cov_pris_param": cov},
                {"mu_pris_param": mu, "cov_pris_param": np.eye(35)}, {"mu_pris_param": mu, "cov_pris_param": np.zeros((36, 36, 1))},
                {"mu_pris_param": mu}, {"cov_pris_param": cov}, None, (mu, cov)):
        with pytest.raises(ValueError, match="mu_pris_param|cov_pris_param"):
            qam.check_niqe_params(bad)
    feat = np.zeros((3, 36))
    with pytest.raises(ValueError, match="mu_pris"):
        _native.niqe_score(feat, np.zeros(35), cov)
    with pytest.raises(ValueError, match="cov_pris"):
        _native.niqe_score(feat, mu, np.eye(35))
    with pytest.raises(ValueError, match="features"):
        _native.niqe_score(np.zeros((3, 35)), mu, cov)
    with pytest.raises(ValueError, match="records"):
        _native.niqe_features(np.zeros(4, dtype=_native.NIQE_RECORD))
    with pytest.raises(ValueError):
        _native.niqe_fit([np.zeros((3, 35))], [np.zeros(3)])
    with pytest.raises(ValueError):
        _native.niqe_fit([np.zeros((3, 36))], [np.zeros(2)])
    with pytest.raises(ValueError):
        _native.niqe_fit([], [])


def test_module_methods_refuse_before_any_device_call(tmp_path):
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    params = {"mu_pris_param": np.zeros(36), "cov_pris_param": np.eye(36)}
    a = np.zeros((100, 128, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        q.niqe_features(a.astype(np.float32))
    with pytest.raises(ValueError, match="3 channels"):
        q.niqe_features(np.zeros((100, 128, 4), np.uint8))
    with pytest.raises(ValueError, match="at least 96"):
        q.niqe_features(a, crop_border=3)
    with pytest.raises(ValueError, match="at least 96"):
        q.calculate_niqe_model(a[:95], params)
    with pytest.raises(ValueError, match="crop_border"):
        q.calculate_niqe_model(a, params, crop_border=-1)
    with pytest.raises(ValueError, match="cov_pris_param"):
        q.calculate_niqe_model(a, {"mu_pris_param": np.zeros(36), "cov_pris_param": np.eye(3)})
    with pytest.raises(ValueError, match="null"):
        q.calculate_niqe_model_device(0, (100, 128, 3), params)
    with pytest.raises(ValueError, match="at least 96"):
        q.calculate_niqe_model_device(256, (100, 90), params)
    # a valid call gets as far as the context, and no further
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_niqe_model(a, params, crop_border=2)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_niqe_model_device(256, (100, 128), params)
    with pytest.raises(AssertionError, match="device context"):
        qam.fit_niqe_model([a], module=q)
    # the existing stand-in is untouched and the pipeline option is off by default
    assert q._niqe_available is False
    import main as sr_main
    assert sr_main.PipelineConfig().qa_niqe_params == ""


def test_parameter_files(tmp_path):
    import quality_assessment_module as qam
    mu, cov = R.pristine()[:2]
    params = {"mu_pris_param": mu, "cov_pris_param": cov}
    for name in ("model.npz", "model.mat"):
        path = str(tmp_path / name)
        qam.save_niqe_params(path, params)
        back = qam.load_niqe_params(path)
        assert back["mu_pris_param"].shape == (36,) and back["cov_pris_param"].shape == (36, 36)
        assert np.array_equal(back["mu_pris_param"], mu) and np.array_equal(back["cov_pris_param"], cov)
    with np.load(str(tmp_path / "model.npz")) as z:                        # BasicSR's layout
        assert sorted(z.files) == ["cov_pris_param", "mu_pris_param"] and z["mu_pris_param"].shape == (1, 36)
    from scipy import io as sio
    z = sio.loadmat(str(tmp_path / "model.mat"))                           # MATLAB's layout
    assert z["mu_prisparam"].shape == (1, 36) and z["cov_prisparam"].shape == (36, 36)
    with pytest.raises(ValueError, match="npz or .mat"):
        qam.save_niqe_params(str(tmp_path / "model.json"), params)
    with pytest.raises(ValueError, match="npz or .mat"):
        qam.load_niqe_params(str(tmp_path / "model.json"))
    np.savez(str(tmp_path / "short.npz"), mu_pris_param=np.zeros((1, 35)), cov_pris_param=cov)
    with pytest.raises(ValueError, match="mu_pris_param"):
        qam.load_niqe_params(str(tmp_path / "short.npz"))
    np.savez(str(tmp_path / "other.npz"), mu=mu)
    with pytest.raises(ValueError, match="mu_pris_param"):
        qam.load_niqe_params(str(tmp_path / "other.npz"))


def test_half_taps_and_window():
    taps = R.half_taps()
    assert np.array_equal(taps * 256.0, [-3, -9, 29, 111, 111, 29, -9, -3]) and taps.sum() == 1.0
    assert np.array_equal(taps, 0.5 * R.cubic([1.75, 1.25, 0.75, 0.25, 0.25, 0.75, 1.25, 1.75]))
    k = R.window()
    assert k.shape == (7,) and abs(k.sum() - 1.0) < 1e-15 and np.array_equal(k, k[::-1]) and k[3] == k.max()
    assert k[2] / k[3] == pytest.approx(np.exp(-1.0 / (2.0 * (7.0 / 6.0) ** 2)), rel=1e-15)


def test_half_plane_is_integral():
    for h, w, cb, cn in CASES:
        img, _, half, (H, W, nby, nbx), *_ = R.case(h, w, cb, cn)
        p = R.plane(img, cb)
        assert p.shape == (H, W) == (96 * nby, 96 * nbx)
        k = R.half_plane(p) * 65536.0
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2 ** 25 and np.array_equal(k, half)
        assert half.shape == (H // 2, W // 2)
        # a constant plane stays constant (the taps sum to 1, the reflection keeps every index inside)
    assert np.array_equal(R.half_plane(np.full((96, 192), 77.0)), np.full((48, 96), 77.0))
    # the borders reflect symmetrically: output 0 reads inputs 2, 1, 0, 0, 1, 2, 3, 4
    ramp = np.tile(np.arange(96.0), (96, 1))
    want0 = (-3 * 2 - 9 * 1 + 29 * 0 + 111 * 0 + 111 * 1 + 29 * 2 - 9 * 3 - 3 * 4) / 256.0
    want_last = (-3 * 91 - 9 * 92 + 29 * 93 + 111 * 94 + 111 * 95 + 29 * 95 - 9 * 94 - 3 * 93) / 256.0
    got = R._half_axis(ramp, 1)
    assert got[0, 0] == want0 and got[0, -1] == want_last


def test_generator_guards():
    """What the device test's integer equalities rest on: no MSCN value or product within 1e-9 of 0 (so a sign can not flip at
    rounding level), no fit within 1e-9 relative of a midpoint of the Gamma-ratio table (so alpha can not)."""
    n_fits = n_near = 0
    for h, w, cb, cn in CASES:
        *_, feat, fits, least = R.case(h, w, cb, cn)
        assert least.min() > 1e-9, (h, w, cb, cn, least.min())
        assert not np.isnan(feat).any()
        d = R.midpoint_distance(fits)
        n_fits += d.size
        n_near += int((d < 1e-9).sum())
        print(f"{h}x{w} cb {cb} cn {cn}: least |X| {least.min():.3e}, nearest midpoint {d.min():.3e} (relative)")
    assert n_fits == 10 * (1 + 2 + 9 + 6) * 2                                # ten fits per block, 18 blocks, two channel counts
    assert n_near == 0 and n_near <= n_fits // 100                           # the exemption is never needed on these inputs
    assert (np.diff(R.R_GAM) / R.R_GAM[1:]).min() > 2e-6                     # the table's spacing


@pytest.mark.parametrize("h,w,cb,cn", CASES, ids=[f"{h}x{w}-cb{cb}-cn{cn}" for h, w, cb, cn in CASES])
def test_features_match_the_restatement(h, w, cb, cn):
    _, rec, _, _, want, *_ = R.case(h, w, cb, cn)
    got = _native.niqe_features(rec)
    assert got.shape == want.shape
    a = R.alpha_slots()
    assert np.array_equal(got[:, a], want[:, a])
    rel = np.abs(got - want) / np.abs(want)
    print("largest relative difference", rel.max())
    assert rel.max() < 1e-12, np.unravel_index(rel.argmax(), rel.shape)
    assert np.array_equal(_native.niqe_sharpness(rec), R.sharpness(rec))


def test_features_of_degenerate_records():
    rec = R.case(96, 192, 0, 1)[1].copy()
    rec[0, 1]["x"][2]["n_neg"] = 0                                           # scale 1, block 1, shift (1, 0): no negative sample
    rec[1, 0]["x"][0]["n_pos"] = 0                                           # scale 2, block 0, X_0: no positive sample
    got, want = _native.niqe_features(rec), R.features(rec)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[1, 6:10]).all() and np.isnan(got[0, 18:20]).all() and np.isnan(got).sum() == 6
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max() < 1e-12
    # alpha saturates at both ends of the table instead of running off it
    flat = rec.copy()
    flat[0, 0]["x"][0] = (4608, 4608, 4608.0, 4608.0, 9216.0)               # |X| = 1 everywhere: R = 1, above the table
    peaked = rec.copy()
    peaked[0, 0]["x"][0] = (4608, 4608, 4.608e9, 4.608e9, 9216.0)           # R near 0, below the table
    assert _native.niqe_features(flat)[0, 0] == R.GAM[-1] and _native.niqe_features(peaked)[0, 0] == R.GAM[0]


def test_fit_matches_numpy_and_the_threshold_rule():
    mu, cov, n, feats, sharps = R.pristine()
    g_mu, g_cov, g_n = _native.niqe_fit(feats, sharps)
    assert g_n == n >= 37
    assert np.abs(g_mu - mu).max() / np.abs(mu).max() < 1e-12 and np.abs(g_cov - cov).max() / np.abs(cov).max() < 1e-12
    assert np.array_equal(g_cov, g_cov.T)
    # the threshold is relative to each image's own sharpest block, strict, and a NaN row is dropped
    rnd = np.random.default_rng(5)
    feats2 = [rnd.standard_normal((40, 36)), rnd.standard_normal((30, 36)) + 1.0]
    sharps2 = [np.concatenate([[10.0], np.full(19, 7.5), rnd.uniform(7.6, 9.9, 20)]),       # 7.5 = 0.75 * 10 exactly: out
               np.concatenate([[2.0], rnd.uniform(1.51, 1.99, 24), rnd.uniform(0.1, 1.49, 5)])]
    feats2[0][25, 7] = np.nan
    w_mu, w_cov, w_n = R.fit(feats2, sharps2)
    g_mu, g_cov, g_n = _native.niqe_fit(feats2, sharps2)
    assert g_n == w_n == (1 + 20 - 1) + (1 + 24)
    assert np.abs(g_mu - w_mu).max() < 1e-12 and np.abs(g_cov - w_cov).max() < 1e-12
    # another threshold keeps other rows
    assert _native.niqe_fit(feats2, sharps2, 0.0)[2] == 40 - 1 + 30 and R.fit(feats2, sharps2, 0.0)[2] == 69
    assert np.abs(_native.niqe_fit(feats2, sharps2, 0.5)[0] - R.fit(feats2, sharps2, 0.5)[0]).max() < 1e-12
    # fewer than 37 rows: refused, and the message gives the count
    clean = rnd.standard_normal((37, 36))
    with pytest.raises(_native.SrShapeError, match=r"\b36 blocks"):
        _native.niqe_fit([clean[:36]], [np.ones(36)])
    assert _native.niqe_fit([clean], [np.ones(37)])[2] == 37
    with pytest.raises(_native.SrShapeError, match=r"\b20 blocks"):
        _native.niqe_fit(feats2[:1], sharps2[:1])


def test_score_matches_the_restatement_under_the_measured_bar():
    mu, cov = R.pristine()[:2]
    change, bar = R.score_bar()
    print(f"largest change of the restated score under a relative 1e-9 on its moments: {change:.3e}; bar {bar:.3e}")
    assert 0.0 < bar < 1e-2
    for h, w, cb, cn in CASES:
        feat = R.case(h, w, cb, cn)[4]
        got, want = _native.niqe_score(feat, mu, cov), R.score(feat, mu, cov)
        print(f"{h}x{w} cb {cb} cn {cn}: {got!r} ref {want!r} diff {abs(got - want):.3e}")
        if feat.shape[0] < 2:
            assert got != got and want != want and "at least 2" in _native.last_error()
            continue
        assert abs(got - want) < bar, (h, w, cb, cn)
        assert _native.niqe_score(feat, mu.reshape(1, 36), cov) == got
    # rank-deficient: feature 5 duplicated into slot 9 on both sides, so that the sum of the covariances is singular and the
    # eigenvalue cut is what keeps the score finite
    feat = R.case(288, 288, 0, 1)[4].copy()
    feats, sharps = [f.copy() for f in R.pristine()[3]], R.pristine()[4]
    feat[:, 9] = feat[:, 5]
    for f in feats:
        f[:, 9] = f[:, 5]
    mu_s, cov_s, _ = R.fit(feats, sharps)
    assert np.linalg.matrix_rank((cov_s + np.cov(feat, rowvar=False)) / 2.0) == 35
    got, want = _native.niqe_score(feat, mu_s, cov_s), R.score(feat, mu_s, cov_s)
    print(f"rank 35: {got!r} ref {want!r} diff {abs(got - want):.3e}")
    assert np.isfinite(want) and abs(got - want) < bar
    # NaN rows: left out of the covariance, their other entries still count in the mean
    feat = R.case(288, 288, 0, 3)[4].copy()
    feat[2, 4] = np.nan
    feat[7, 30:] = np.nan
    got, want = _native.niqe_score(feat, mu, cov), R.score(feat, mu, cov)
    assert abs(got - want) < bar and abs(got - R.score(np.delete(feat, (2, 7), 0), mu, cov)) > bar
    # fewer than two NaN-free blocks
    feat = R.case(96, 192, 0, 1)[4].copy()
    feat[1, 0] = np.nan
    v = _native.niqe_score(feat, mu, cov)
    assert v != v and "1 of 2 blocks" in _native.last_error() and R.score(feat, mu, cov) != R.score(feat, mu, cov)
    v = _native.niqe_score(feat[:0], mu, cov)
    assert v != v
