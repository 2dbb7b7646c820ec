"""Host side of the per-cell quality map (no GPU): the closed-form per-cell sample counts against brute-force counting,
every refusal of the C ABI and of the Python layers before a device is touched, the per-tile cells of the uniform tiling,
and the soundness of the restatement (tests/_qmap_ref.py) against the oracle's own SSIM means."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _native
import _qmap_ref as R
import quality_assessment_module as qam
import tiling_module as tm
from oracle import oracle_np as onp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (h, w, x_edges, y_edges): uniform, non-dividing, cells narrower than the crops (1, 2, 3 pixels at the borders), one cell,
# one-pixel cells, images smaller than a window
COUNT_CASES = [
    (97, 131, R.uniform_edges(131, 4), R.uniform_edges(97, 4)),
    (97, 131, R.uniform_edges(131, 16), R.uniform_edges(97, 16)),
    (97, 131, R.uniform_edges(131, 37), R.uniform_edges(97, 37)),
    (97, 131, [0, 131], [0, 97]),
    (97, 131, [0, 5, 6, 70, 131], [0, 1, 50, 97]),
    (23, 29, R.uniform_edges(29, 1), R.uniform_edges(23, 1)),
    (23, 29, [0, 1, 3, 4, 6, 23, 24, 26, 28, 29], [0, 2, 5, 18, 20, 22, 23]),
    (40, 40, [0, 3, 5, 35, 37, 40], [0, 3, 5, 35, 37, 40]),
    (9, 200, R.uniform_edges(200, 64), [0, 4, 9]),          # no gauss sample at all (h < 11)
    (200, 6, [0, 1, 6], R.uniform_edges(200, 50)),           # neither uniform nor gauss
    (11, 11, [0, 5, 6, 11], [0, 5, 6, 11]),                  # exactly one gauss sample, in the centre cell
    (523, 771, R.uniform_edges(771, 64), R.uniform_edges(523, 64)),
]


@pytest.mark.parametrize("h,w,xe,ye", COUNT_CASES, ids=[f"{c[0]}x{c[1]}-{len(c[3]) - 1}x{len(c[2]) - 1}" for c in COUNT_CASES])
def test_counts_equal_brute_force(h, w, xe, ye):
    for mode in ("uniform", "gauss", "simple"):
        got = _native.quality_map_counts(h, w, mode, xe, ye)
        want = R.bin_map(R.valid_mask(h, w, mode), xe, ye)
        assert got.dtype == np.uint64 and got.shape == (len(ye) - 1, len(xe) - 1)
        assert np.array_equal(got.astype(np.int64), want), mode
        assert int(got.sum()) == _native.ssim_count(h, w, mode), mode


def _call_u8(h=32, w=40, cn=3, shift=15, xe=(0, 40), ye=(0, 32), flags=_native.ASSESS_ALL, ctx=None, a=1, out=True,
             stride=None):
    """The C entry point itself with no context behind it: an argument error must be reported before the context is looked at."""
    lib = _native.load()
    xa, ya = (C.c_int * len(xe))(*xe), (C.c_int * len(ye))(*ye)
    recs = (_native.QualityCell * max((len(xe) - 1) * (len(ye) - 1), 1))()
    st = w * cn if stride is None else stride
    rc = lib.sr_quality_map_u8(ctx, C.c_void_p(a), st, C.c_void_p(1), st, h, w, cn, shift, 255.0, xa, len(xe) - 1, ya,
                               len(ye) - 1, flags, recs if out else None)
    return rc, _native.last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(xe=(0, 20, 20, 40)), "strictly increasing"),
    (dict(xe=(0, 30, 20, 40)), "strictly increasing"),
    (dict(ye=(0, 16, 8, 32)), "strictly increasing"),
    (dict(xe=(1, 40)), "from 0 to 40"),
    (dict(xe=(0, 39)), "from 0 to 40"),
    (dict(ye=(0, 33)), "from 0 to 32"),
    (dict(xe=(0,)), "at least one cell"),
    (dict(ye=(0,)), "at least one cell"),
    (dict(cn=2), "1 or 3 channels"),
    (dict(cn=4), "1 or 3 channels"),
    (dict(flags=16), "unknown flag bits"),
    (dict(flags=-1), "unknown flag bits"),
    (dict(shift=13), "gray_shift"),
    (dict(h=0, ye=(0, 0)), "h,w >= 1"),
    (dict(w=0, xe=(0, 0)), "h,w >= 1"),
    (dict(a=None), "null"),
    (dict(out=False), "null"),
])
def test_c_abi_refuses_before_the_context(kw, word):
    rc, msg = _call_u8(**kw)
    assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (rc, msg)


def test_c_abi_statuses_follow_assess():
    rc, msg = _call_u8(stride=100)                              # a stride below the row: the status sr_assess_u8 returns
    assert rc == _native.SR_ERR_SHAPE and "stride" in msg
    rc, msg = _call_u8()                                        # every argument fine: only now the context is missed
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    lib = _native.load()
    n = (C.c_uint64 * 4)()
    e = (C.c_int * 2)(0, 8)
    assert lib.sr_quality_map_counts(8, 8, 3, e, 1, e, 1, n) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_quality_map_counts(8, 8, 0, e, 1, e, 1, None) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_quality_map_counts(0, 8, 0, e, 1, e, 1, n) == _native.SR_ERR_INVALID_ARG


def test_python_binding_refuses_before_any_device_call():
    ctx_free = _native.Context.__new__(_native.Context)           # no device behind it: the checks must come first
    call = lambda **k: _native.Context.quality_map_u8(ctx_free, 0, 120, 0, 120, **{**dict(h=32, w=40, cn=3, x_edges=[0, 40],
                                                                                          y_edges=[0, 32]), **k})
    for kw in (dict(x_edges=[0, 20, 20, 40]), dict(x_edges=[0, 41]), dict(y_edges=[5, 32]), dict(x_edges=[0]), dict(y_edges=[]),
               dict(x_edges=[0.0, 40.0]), dict(x_edges=[[0, 40]]), dict(cn=2), dict(cn=4), dict(flags=32), dict(gray_shift=16),
               dict(h=0, y_edges=[0, 0]), dict(x_edges=[0, 2 ** 31])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AttributeError):                           # all arguments fine: the first use of the (absent) device
        call()
    with pytest.raises(ValueError):
        _native.quality_map_counts(32, 40, "gauss", [0, 40, 40], [0, 32])
    with pytest.raises(KeyError):
        _native.quality_map_counts(32, 40, "box", [0, 40], [0, 32])


class _NoDevice(qam.QualityAssessmentModule):
    def _ctx(self):
        raise AssertionError("a device call was made")


def test_evaluate_quality_map_argument_errors():
    q = _NoDevice()
    a = np.full((32, 40, 3), 7, np.uint8)
    g = np.full((32, 40), 7, np.uint8)
    bad = [dict(cell=0), dict(cell=-3), dict(cell=2.5), dict(cell=64, x_edges=[0, 40], y_edges=[0, 32]),
           dict(x_edges=[0, 40]), dict(y_edges=[0, 32]), dict(x_edges=[0, 39], y_edges=[0, 32]),
           dict(x_edges=[0, 20, 10, 40], y_edges=[0, 32]), dict(x_edges=[0, 20.5, 40], y_edges=[0, 32])]
    for kw in bad:
        with pytest.raises(ValueError):
            q.evaluate_quality_map(a, a, **kw)
        with pytest.raises(ValueError):
            q.evaluate_quality_map_device(256, a.shape, 512, a.shape, **kw)
    with pytest.raises(ValueError):
        q.evaluate_quality_map(a, g)                                        # channel layouts differ
    with pytest.raises(ValueError):
        q.evaluate_quality_map(np.full((8, 8, 4), 9, np.uint8), np.full((8, 8, 4), 9, np.uint8))
    with pytest.raises(ValueError):
        q.evaluate_quality_map_device(256, (8, 8, 3), 512, (8, 8))
    with pytest.raises(NotImplementedError):
        q.evaluate_quality_map(np.full((8, 8), 300, np.uint16), np.full((8, 8), 300, np.uint16))
    # the edges are taken on the common top-left rectangle: 30 x 36 here
    with pytest.raises(ValueError):
        q.evaluate_quality_map(a, a[:30, :36], x_edges=[0, 40], y_edges=[0, 32])
    with pytest.raises(AssertionError, match="device call"):                # a sound request reaches the device
        q.evaluate_quality_map(a, a[:30, :36], x_edges=[0, 36], y_edges=[0, 30])
    assert q._map_edges(100, 130, None, None, None) == ([0, 130], [0, 100])             # default cell 256
    assert q._map_edges(100, 130, 64, None, None) == ([0, 64, 128, 130], [0, 64, 100])


def test_tile_cell_edges_on_the_golden_grid():
    g = json.load(open(os.path.join(GOLD, "bookkeeping.json")))
    case = next(c for c in g["tiling"] if (c["w"], c["h"], c["block"]) == (4096, 4096, 1024))
    assert case["overlap_px"] == 204
    xe, ye = tm.tile_cell_edges(case["positions"], 204, 2, 8192, 8192)
    # tile columns start at 0, 820, 1640, 2460, 3280: the cuts are 2 * x + (2 * 204) // 2
    assert xe == ye == [0, 1844, 3484, 5124, 6764, 8192]
    xe1, _ = tm.tile_cell_edges(case["positions"], 205, 1, 4096, 4096)     # an odd overlap: floor of the half
    assert xe1 == [0, 820 + 102, 1640 + 102, 2460 + 102, 3280 + 102, 4096]
    # the cells partition the canvas, one per tile, each inside its tile
    assert int(_native.quality_map_counts(8192, 8192, "simple", xe, ye).sum()) == 8192 * 8192
    assert (len(xe) - 1) * (len(ye) - 1) == len(case["positions"])
    for (x, y, w, h) in case["positions"]:
        c, r = xe.index(0 if x == 0 else 2 * x + 204), ye.index(0 if y == 0 else 2 * y + 204)
        assert 2 * x <= xe[c] and xe[c + 1] <= 2 * (x + w) and 2 * y <= ye[r] and ye[r + 1] <= 2 * (y + h)
    for case in g["tiling"]:                                    # every golden grid gives a partition
        s = 2
        xe, ye = tm.tile_cell_edges(case["positions"], case["overlap_px"], s, s * case["w"], s * case["h"])
        assert xe[0] == ye[0] == 0 and xe[-1] == s * case["w"] and ye[-1] == s * case["h"]
        assert (len(xe) - 1) * (len(ye) - 1) == len(case["positions"])
        assert all(b > a for a, b in zip(xe, xe[1:])) and all(b > a for a, b in zip(ye, ye[1:]))


def test_tile_cell_edges_refuses_what_is_not_a_uniform_grid():
    grid = [(x, y, 100, 100) for y in (0, 80) for x in (0, 80, 160)]
    assert tm.tile_cell_edges(grid, 20, 1, 260, 180) == ([0, 90, 170, 260], [0, 90, 180])
    for bad in (grid[:-1], grid + [(40, 40, 100, 100)], [], [(10, 0, 100, 100)], grid + [grid[0]]):
        with pytest.raises(ValueError):
            tm.tile_cell_edges(bad, 20, 1, 260, 180)
    with pytest.raises(ValueError):
        tm.tile_cell_edges(grid, 20, 1, 170, 180)               # the last cut is not inside the canvas
    with pytest.raises(ValueError):
        tm.tile_cell_edges(grid, -1, 1, 260, 180)


def test_restatement_means_are_the_oracles():
    rng = np.random.default_rng(5)
    a, b = R.img_pair(rng, 41, 57)
    ref = R.Reference(a, b)
    g1, g2 = R.gray(a), R.gray(b)
    assert int(ref.sq.sum()) == int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    for mode in ("uniform", "gauss", "simple"):
        n = _native.ssim_count(41, 57, mode)
        assert ref.maps[mode].sum() / n == pytest.approx(onp.ssim(g1, g2, mode), rel=1e-13)
    cells = ref.cells(R.uniform_edges(57, 16), R.uniform_edges(41, 16))
    assert int(cells["sse"].sum()) == int(ref.sq.sum())
    assert cells["ssim_gauss"].sum() == pytest.approx(ref.maps["gauss"].sum(), rel=1e-13)


def test_pipeline_config_default_is_off():
    import main as sr_main
    assert sr_main.PipelineConfig().qa_map_cell == 0
