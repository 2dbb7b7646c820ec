"""CPU: the host side of FSIM (csrc/sr_fsim_host.cpp) against the NumPy restatement tests/_fsim_ref.py, and the restatement
against its own mutants.

* F at 383 / 384 / 639 / 640 / 895 / 896 and the pooled sizes;
* the eight filter planes, EM_n, S2 and Sij at 1e-12 on odd x odd, even x even and mixed sides -- the restatement forms S2 and
  Sij the long way, through real(ifft2(filter)), so the Parseval shortcut of the host unit is held against it;
* sr_fsim_value (ratios, NaN) and sr_fsim_chroma_weight (the negative S_i S_q branch);
* every refusal;
* mutants: each deliberate mistake moves the restatement's value by more than the GPU test's bar (1e-9 relative) on an input
  tests/test_gpu_fsim.py uses, so that bar tells the definition from its near misses."""
import math

import numpy as np
import pytest

import _fsim_ref as R
import _native

BAR = 1e-9          # tests/test_gpu_fsim.py: TOL


@pytest.mark.parametrize("side,F", [(383, 1), (384, 2), (639, 2), (640, 3), (895, 3), (896, 4), (16, 1), (127, 1), (128, 1)])
def test_f_and_the_pooled_size(side, F):
    for h, w in ((side, side + 301), (side + 77, side)):
        p = _native.fsim_plan(h, w, 3)
        assert p["F"] == F == R.auto_f(h, w)
        assert p["size"] == (-(-h // F), -(-w // F)) == R.pooled_int(np.zeros((h, w), np.uint8), F).shape[1:]
        assert p["workspace_bytes"] > 6 * 8 * p["size"][0] * p["size"][1]


def test_the_window_of_the_pooling():
    """Window i covers i F + floor(F / 2) - F + 1 .. i F + floor(F / 2), zero outside: against a direct loop."""
    rnd = np.random.default_rng(2)
    for h, w, F in ((13, 19, 3), (16, 16, 4), (17, 23, 5), (9, 11, 2), (7, 7, 8)):
        img = rnd.integers(0, 256, (h, w), dtype=np.uint8)
        got = R.pool_int(img.astype(np.int64), F)
        for i in range(got.shape[0]):
            for j in range(got.shape[1]):
                ys, xs = i * F + F // 2 - F + 1, j * F + F // 2 - F + 1
                want = sum(int(img[y, x]) for y in range(ys, ys + F) for x in range(xs, xs + F) if 0 <= y < h and 0 <= x < w)
                assert got[i, j] == want, (h, w, F, i, j)


@pytest.mark.parametrize("rows,cols", [(17, 23), (16, 16), (16, 19), (33, 32), (64, 65), (101, 50)], ids=lambda v: str(v))
def test_filters_and_noise_sums_match_the_restatement(rows, cols):
    f = _native.fsim_filters(rows, cols)
    lg, sp = R.filters(rows, cols)
    em, s2, sij = R.noise_sums(lg, sp)
    assert np.abs(f["log_gabor"] - lg).max() <= 1e-12 and np.abs(f["spread"] - sp).max() <= 1e-12
    for k, want in (("em", em), ("s2", s2), ("sij", sij)):
        rel = np.abs(f[k] / want - 1).max()
        print(rows, cols, k, rel)
        assert rel <= 1e-12, k
    assert (f["log_gabor"][:, 0, 0] == 0).all() and f["log_gabor"].max() <= 1.0 and f["spread"].min() > 0


def test_value_and_chroma_weight():
    assert _native.fsim_value({"sum_s": 3.0, "sum_sc": 2.0, "sum_pcm": 4.0}) == (0.75, 0.5)
    assert all(math.isnan(v) for v in _native.fsim_value({"sum_s": 0.0, "sum_sc": 0.0, "sum_pcm": 0.0}))
    assert all(math.isnan(v) for v in _native.fsim_value({"sum_s": float("nan"), "sum_sc": float("nan"), "sum_pcm": float("nan")}))
    for si, sq in ((1.0, 1.0), (0.3, 0.9), (-0.4, 0.7), (0.2, -0.9), (-0.5, -0.5), (0.0, 0.4)):
        want = float(np.real(complex(si * sq) ** 0.03))
        assert _native.fsim_chroma_weight(si, sq) == pytest.approx(want, rel=1e-15, abs=0), (si, sq)
    assert _native.fsim_chroma_weight(-0.4, 0.7) == pytest.approx(0.28 ** 0.03 * math.cos(0.03 * math.pi), rel=1e-15)
    assert _native.fsim_chroma_weight(-0.4, 0.7) < 0.28 ** 0.03 * 0.999


def test_refusals():
    for cn in (0, 2, 5):
        with pytest.raises(ValueError):
            _native.fsim_plan(64, 64, cn)
    with pytest.raises(ValueError):
        _native.fsim_plan(0, 64, 3)
    for h, w in ((15, 64), (64, 15)):
        with pytest.raises(_native.SrShapeError):
            _native.fsim_plan(h, w, 3)
        assert "at least 16" in _native.last_error()
    for h, w in ((100, 2049), (2049, 300), (383, 4000)):
        with pytest.raises(_native.SrNativeError):
            _native.fsim_plan(h, w, 3)
        assert "2048" in _native.last_error()
    assert _native.fsim_plan(100, 2048, 3)["size"] == (100, 2048)
    assert _native.fsim_plan(10000, 20000, 3) == {"F": 39, "size": (257, 513), "workspace_bytes": _native.fsim_plan(10000, 20000, 3)["workspace_bytes"]}
    with pytest.raises(_native.SrShapeError):
        _native.fsim_filters(15, 16)
    with pytest.raises(_native.SrNativeError):
        _native.fsim_filters(16, 2049)
    with pytest.raises(ValueError):
        _native.fsim_filters(0, 16)
    if _native.device_count() == 0:                     # without a device the compute entries fail loudly
        with pytest.raises(_native.SrNativeError):
            _native.Context(0)


def test_restatement_self_comparison_and_symmetry():
    for h, w, cn in ((16, 16, 1), (17, 23, 3), (32, 45, 3)):
        a, b = R.case(h, w, cn)
        s = R.fsim(a, a)
        assert s["fsim"] == 1.0 and s["fsimc"] == 1.0
        ab, ba = R.fsim(a, b), R.fsim(b, a)
        assert ab["fsim"] == pytest.approx(ba["fsim"], rel=1e-12) and ab["fsimc"] == pytest.approx(ba["fsimc"], rel=1e-12)
        assert ab["an_all_min"] >= 1e-3
    flat = np.full((24, 31, 3), 0, np.uint8)
    assert math.isnan(R.fsim(flat, flat)["fsim"])


# (mutant, an input of tests/test_gpu_fsim.py on which it must show): lower_median needs an even count, window_if an F of 3 or
# more (at F = 2 the window starts at i F either way), abs_pow a negative S_i S_q
MUTANTS = [("grid_swap", (17, 23, 3)), ("grid_swap", (64, 64, 1)), ("lower_median", (16, 16, 1)), ("lower_median", (64, 64, 1)),
           ("window_if", (640, 641, 1)), ("abs_pow", (383, 200, 3)), ("no_17", (17, 23, 3)), ("no_17", (32, 45, 3))]


@pytest.mark.parametrize("mut,shape", MUTANTS, ids=[f"{m}-{s[0]}x{s[1]}" for m, s in MUTANTS])
def test_mutants_move_the_value_beyond_the_bar(mut, shape):
    a, b = R.case(*shape)
    good, bad = R.fsim(a, b), R.fsim(a, b, mut=mut)
    key = "fsimc" if mut == "abs_pow" else "fsim"
    rel = abs(bad[key] / good[key] - 1)
    print(mut, shape, key, good[key], bad[key], rel)
    if mut == "abs_pow":
        assert good["min_siq"] < 0
    assert rel > 100 * BAR
