"""Every variant of the fused assessment march (k_assess_march, csrc/sr_assess.hip) at small shapes, against the float64
SSIM maps of tests/_qmap_ref.py: the twelve instantiations (CN x {GAUSS, UNIF} x SAMEC -- SAMEC false is what a u8 call
with data_range != 255 runs), every chunk count 2..12 (SR_ASSESS_NCH), row strips cut inside the border rows, flag
subsets, saturating inputs, frames smaller than the windows, the column edges of the 4-pixel loader, and the three
samplers in front of the march (sr_assess_resized_u8).

For a strip [r0, r1) the wanted sum of a mode is math.fsum of rows r0:r1 of the reference's masked map and the wanted SSE
the sum of rows r0:r1 of the squared-error map.  Bars: SSE exact; |got - want| <= 1e-9 * max(count, 1) for every SSIM sum
(the absolute 1e-9 on the mean of fuzz_blend.py); a field whose flag is not set, or whose window does not fit the frame,
is exactly 0.0; two identical calls return bit-identical sums (fixed-order reductions); sums that differ only in the order
of their additions (chunk counts, strips) agree to 1e-12 relative, as in test_ssim_row_ranges_add_up."""
import math

import numpy as np
import pytest

import _qmap_ref as qr
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

SSE, UNIFORM, GAUSS, SIMPLE, ALL = 1, 2, 4, 8, 15          # _native.ASSESS_*
MODES = (("uniform", UNIFORM), ("gauss", GAUSS), ("simple", SIMPLE))
RANGES = (255.0, 100.0)

_pairs, _refs = {}, {}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every test starts from the cost rule's chunk count and the default sampler; those that want another set it."""
    monkeypatch.delenv("SR_ASSESS_NCH", raising=False)
    monkeypatch.delenv("SR_RESIZE_MARCH", raising=False)


def _pair(rng, h, w, cn):
    """qr.img_pair, drawn once per shape and shared."""
    key = (h, w, cn)
    if key not in _pairs:
        _pairs[key] = tuple(np.ascontiguousarray(x) for x in qr.img_pair(rng, h, w, cn))
    return _pairs[key]


def _ref(key, a, b, data_range, shift=15):
    """qr.Reference of a pair, computed once per (key, data_range, shift) and never changed."""
    k = (key, float(data_range), shift)
    if k not in _refs:
        _refs[k] = qr.Reference(a, b, shift, float(data_range))
    return _refs[k]


class _Dev:
    """Both images of a pair in device memory for the calls of one test."""

    def __init__(self, ctx, a, b):
        self.ctx, self.h, self.w = ctx, a.shape[0], a.shape[1]
        self.cn = 3 if a.ndim == 3 else 1
        self.da, self.db = ctx.upload(a), ctx.upload(b)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.da.free()
        self.db.free()

    def assess(self, **kw):
        s = self.w * self.cn
        return self.ctx.assess_u8(self.da.ptr, s, self.db.ptr, s, self.h, self.w, self.cn, **kw)


def _want(ref, r0=0, r1=None):
    """Wanted sums and sample counts of rows [r0, r1) -> ({field: sum}, {field: count})."""
    r1 = ref.h if r1 is None else r1
    want, count = {"sse": float(int(ref.sq[r0:r1].sum()))}, {}
    for mode, _ in MODES:
        want[f"ssim_{mode}"] = math.fsum(ref.maps[mode][r0:r1].ravel().tolist())
        count[f"ssim_{mode}"] = int(qr.valid_mask(ref.h, ref.w, mode)[r0:r1].sum())
    return want, count


def _check(got, ref, flags, r0=0, r1=None, what=""):
    want, count = _want(ref, r0, r1)
    print(what, "flags", flags, "rows", r0, r1, "got", got, "want", want)
    assert got["sse"] == (want["sse"] if flags & SSE else 0.0), (what, "sse")
    for mode, bit in MODES:
        k = f"ssim_{mode}"
        if not flags & bit:
            assert got[k] == 0.0, (what, k, "flag not set")
        elif count[k] == 0:
            assert got[k] == 0.0, (what, k, "no valid sample")
        else:
            assert abs(got[k] - want[k]) <= 1e-9 * count[k], (what, k, got[k], want[k], count[k])


def _same_sums(x, y, what=""):
    """Two runs that differ only in the order of their additions."""
    assert x["sse"] == y["sse"], what
    for mode, _ in MODES:
        k = f"ssim_{mode}"
        assert x[k] == pytest.approx(y[k], rel=1e-12, abs=0.0), (what, k)


def _ref_moves_with_range(ref255, ref_other):
    """The reference's own gauss and uniform means move by more than 1e-3 with data_range (a kernel that ignored the
    argument could pass otherwise); its simple map does not depend on it."""
    w255, n = _want(ref255)
    wo, _ = _want(ref_other)
    for k in ("ssim_gauss", "ssim_uniform"):
        assert abs(w255[k] - wo[k]) / n[k] > 1e-3, k
    assert w255["ssim_simple"] == wo["ssim_simple"]


# ---- a. all twelve instantiations -------------------------------------------------------------------------------
FLAG_SETS = (SSE, GAUSS, SIMPLE, UNIFORM, GAUSS | SIMPLE, GAUSS | UNIFORM, SIMPLE | UNIFORM | SSE, ALL)


@pytest.mark.parametrize("data_range", [255.0, 100.0, 510.0])
@pytest.mark.parametrize("cn", [1, 3])
def test_instantiations(ctx, rng, cn, data_range):
    """<CN, GAUSS, UNIF, SAMEC>: SSE alone is <CN, false, false, true>, UNIFORM (+ SSE) <CN, false, true, true>, any of
    GAUSS / SIMPLE <CN, true, ., data_range == 255>.  47 x 261: two column blocks, the second 5 columns wide (narrower
    than the halo), four block rows of 12."""
    a, b = _pair(rng, 47, 261, cn)
    ref = _ref((47, 261, cn), a, b, data_range)
    with _Dev(ctx, a, b) as d:
        for flags in FLAG_SETS:
            got = d.assess(flags=flags, data_range=data_range)
            _check(got, ref, flags, what=f"cn={cn} range={data_range}")
            assert d.assess(flags=flags, data_range=data_range) == got, ("not deterministic", flags)


@pytest.mark.parametrize("data_range", RANGES)
def test_instantiations_gray_shift_14(ctx, rng, data_range):
    a, b = _pair(rng, 47, 261, 3)
    ref = _ref((47, 261, 3), a, b, data_range, shift=14)
    assert not np.array_equal(qr.gray(a, 14), qr.gray(a, 15))
    with _Dev(ctx, a, b) as d:
        _check(d.assess(flags=ALL, data_range=data_range, gray_shift=14), ref, ALL, what=f"shift 14 range={data_range}")


@pytest.mark.parametrize("cn", [1, 3])
def test_data_range_moves_gauss_and_uniform_only(ctx, rng, cn):
    a, b = _pair(rng, 47, 261, cn)
    r255 = _ref((47, 261, cn), a, b, 255.0)
    with _Dev(ctx, a, b) as d:
        g255 = d.assess(flags=ALL, data_range=255.0)
        for other in (100.0, 510.0):
            _ref_moves_with_range(r255, _ref((47, 261, cn), a, b, other))
            g = d.assess(flags=ALL, data_range=other)
            _, n = _want(r255)
            assert g["sse"] == g255["sse"]
            # the same values in the same order (SAMEC true adds them to sum_all, SAMEC false too)
            assert g["ssim_simple"] == pytest.approx(g255["ssim_simple"], rel=1e-12, abs=0.0)
            for k in ("ssim_gauss", "ssim_uniform"):
                assert abs(g[k] - g255[k]) / n[k] > 1e-3, (k, other)


# ---- b. chunk counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", range(2, 13))
def test_chunk_counts(ctx, rng, monkeypatch, nch):
    """A block marches nch chunks of 11 rows and produces ty = 11 nch - 10: one block a row short, exactly full and one
    row over, and three block rows whose last has 4 rows.  The uniform-7 ring's slot (r mod 7) meets every phase of the
    11-row chunk, and r reaches 131 at nch = 12.  Every nch must also give the sums of nch = 2."""
    ty = 11 * nch - 10
    for cn in (3, 1) if nch in (2, 7, 12) else (3,):
        for h in (ty - 1, ty, ty + 1, 2 * ty + 4):
            a, b = _pair(rng, h, 259, cn)
            with _Dev(ctx, a, b) as d:
                for data_range in RANGES:
                    ref = _ref((h, 259, cn), a, b, data_range)
                    monkeypatch.setenv("SR_ASSESS_NCH", str(nch))
                    got = d.assess(flags=ALL, data_range=data_range)
                    _check(got, ref, ALL, what=f"nch={nch} h={h} cn={cn} range={data_range}")
                    assert d.assess(flags=ALL, data_range=data_range) == got, "not deterministic"
                    monkeypatch.setenv("SR_ASSESS_NCH", "2")
                    _same_sums(got, d.assess(flags=ALL, data_range=data_range), f"nch={nch} against 2, h={h}")


def test_chunk_count_switch_ignores_other_values(ctx, rng, monkeypatch):
    """Anything but an integer in [2, 12] leaves the cost rule's choice (2 at this size): bit-identical sums."""
    a, b = _pair(rng, 47, 261, 3)
    with _Dev(ctx, a, b) as d:
        base = d.assess(flags=ALL)
        for v in ("", "1", "13", "-3", "x", "3x", "2.5"):
            monkeypatch.setenv("SR_ASSESS_NCH", v)
            assert d.assess(flags=ALL) == base, v
        monkeypatch.setenv("SR_ASSESS_NCH", "2")
        assert d.assess(flags=ALL) == base


def test_chunk_count_switch_takes_effect(ctx, monkeypatch):
    """The sums are right at any chunk count, so a switch that did nothing would pass every test above.  What the chunk
    count does change is how the rows are grouped into blocks, i.e. the order of the fp64 additions: on one fixed pair
    (its own generator: the outcome must not depend on which tests ran before) the thirty SSIM sums of nch = 3 .. 12 are
    not all bit-identical to those of nch = 2 -- the reductions are fixed-order, so this is deterministic."""
    a, b = qr.img_pair(np.random.default_rng(7), 137, 259, 3)
    with _Dev(ctx, np.ascontiguousarray(a), np.ascontiguousarray(b)) as d:
        monkeypatch.setenv("SR_ASSESS_NCH", "2")
        base = d.assess(flags=ALL)
        moved = 0
        for nch in range(3, 13):
            monkeypatch.setenv("SR_ASSESS_NCH", str(nch))
            got = d.assess(flags=ALL)
            _same_sums(got, base, f"nch={nch}")
            moved += sum(got[f"ssim_{m}"] != base[f"ssim_{m}"] for m, _ in MODES)
        print("sums that moved in their last bits:", moved, "of 30")
        assert moved > 0


# ---- c. strips against the reference ----------------------------------------------------------------------------
STRIP_H, STRIP_W = 73, 270
CUTS = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 37, STRIP_H - 6, STRIP_H - 5, STRIP_H - 4, STRIP_H - 3, STRIP_H - 1, STRIP_H)


@pytest.mark.parametrize("nch", [None, 3])
@pytest.mark.parametrize("data_range", RANGES)
@pytest.mark.parametrize("cn", [3, 1])
def test_strips_match_reference_and_add_up(ctx, rng, monkeypatch, cn, data_range, nch):
    """Strips that begin or end inside the 3 (uniform) and 5 (gauss) border rows -- at data_range 255 the cropped Gaussian
    sum of a strip is its full-frame sum minus the rows outside the crop (EDGE) -- each against the reference, and their
    total against the whole-frame call.  nch = 3 (blocks of 23 rows): strips that span several block rows."""
    if nch is not None:
        monkeypatch.setenv("SR_ASSESS_NCH", str(nch))
    a, b = _pair(rng, STRIP_H, STRIP_W, cn)
    ref = _ref((STRIP_H, STRIP_W, cn), a, b, data_range)
    _ref_moves_with_range(_ref((STRIP_H, STRIP_W, cn), a, b, 255.0), _ref((STRIP_H, STRIP_W, cn), a, b, 100.0))
    with _Dev(ctx, a, b) as d:
        whole = d.assess(flags=ALL, data_range=data_range)
        _check(whole, ref, ALL, what="whole frame")
        parts = []
        for r0, r1 in zip(CUTS[:-1], CUTS[1:]):
            got = d.assess(flags=ALL, data_range=data_range, row_begin=r0, row_end=r1)
            _check(got, ref, ALL, r0, r1, what=f"strip cn={cn} range={data_range} nch={nch}")
            parts.append(got)
        total = {k: math.fsum(p[k] for p in parts) for k in whole}
        _same_sums(total, whole, "strips against the whole frame")
        # one mode at a time takes other instantiations (no uniform ring, no SSE) with the same guards
        for flags in (UNIFORM, GAUSS, SIMPLE | SSE):
            for r0, r1 in ((2, 5), (4, 12), (37, STRIP_H - 4), (STRIP_H - 4, STRIP_H)):
                _check(d.assess(flags=flags, data_range=data_range, row_begin=r0, row_end=r1), ref, flags, r0, r1, what="subset strip")
        zeros = {k: 0.0 for k in whole}
        for r0, r1 in ((20, 20), (30, 20), (0, 0), (STRIP_H, STRIP_H), (STRIP_H, STRIP_H + 9), (-4, 0)):
            assert d.assess(flags=ALL, data_range=data_range, row_begin=r0, row_end=r1) == zeros, (r0, r1)


# ---- d. saturation ----------------------------------------------------------------------------------------------
def _saturating_pairs(h, w, cn):
    shape = (h, w, 3) if cn == 3 else (h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    board = np.ascontiguousarray(np.repeat(board[..., None], 3, axis=2)) if cn == 3 else board
    full, zero = np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)
    return {"255/255": (full, full), "255/0": (full, zero), "board/inverse": (board, 255 - board), "board/board": (board, board)}


@pytest.mark.parametrize("h,w,cn,nch", [(130, 300, 3, 12), (40, 64, 1, None)])
def test_saturation(ctx, monkeypatch, h, w, cn, nch):
    """Gray 255 everywhere (or in half the samples): the packed x | y << 14 window sums reach 12495, the 7-tap sum of x*y
    fills both parts of its split field, and at nch = 12 a thread's 32-bit SSE is at its maximum (432 differences of
    65025); 130 x 300 x 3 x 65025 is the largest SSE of the shape."""
    if nch is not None:
        monkeypatch.setenv("SR_ASSESS_NCH", str(nch))
    for name, (a, b) in _saturating_pairs(h, w, cn).items():
        assert int(qr.gray(a).max()) == 255
        with _Dev(ctx, a, b) as d:
            for data_range in RANGES:
                ref = _ref(("sat", name, h, w, cn), a, b, data_range)
                got = d.assess(flags=ALL, data_range=data_range)
                _check(got, ref, ALL, what=f"{name} {h}x{w}x{cn} range={data_range}")
                assert d.assess(flags=ALL, data_range=data_range) == got, "not deterministic"
                if name == "255/0":
                    assert got["sse"] == float(h * w * cn * 65025)
                if a is b:
                    assert got["sse"] == 0.0
                    _, count = _want(ref)
                    for k, n in count.items():
                        assert abs(got[k] - n) <= 1e-9 * n, (name, k)


# ---- e. small and thin frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (3, 4), (5, 5), (6, 6), (7, 7), (10, 10), (11, 11), (12, 300), (300, 12)])
def test_small_and_thin_frames(ctx, rng, h, w):
    """'simple' has no crop, so every size is legal and REFLECT_101 iterates below 6 rows or columns; a mode whose window
    does not fit (uniform below 7, gauss below 11) returns exactly 0.0 (_check: no valid sample)."""
    for cn in (1, 3):
        a, b = _pair(rng, h, w, cn)
        with _Dev(ctx, a, b) as d:
            for data_range in RANGES:
                ref = _ref((h, w, cn), a, b, data_range)
                _, count = _want(ref)
                assert count["ssim_simple"] == h * w
                assert (count["ssim_uniform"] == 0) == (min(h, w) < 7) and (count["ssim_gauss"] == 0) == (min(h, w) < 11)
                _check(d.assess(flags=ALL, data_range=data_range), ref, ALL, what=f"{h}x{w}x{cn} range={data_range}")
                _check(d.assess(flags=SIMPLE, data_range=data_range), ref, SIMPLE, what=f"simple alone {h}x{w}x{cn}")


# ---- f. column edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [252, 253, 255, 256, 257, 259, 261, 262, 512, 515])
def test_column_edges(ctx, rng, w):
    """The loader takes 4-pixel groups with one wide load where the group lies inside the image and reflected single pixels
    where it crosses the right edge; the last column block is 1 to 6 columns wide at 257 .. 262 and 3 at 515."""
    for cn in (3, 1):
        a, b = _pair(rng, 30, w, cn)
        with _Dev(ctx, a, b) as d:
            for data_range in RANGES:
                ref = _ref((30, w, cn), a, b, data_range)
                _check(d.assess(flags=ALL, data_range=data_range), ref, ALL, what=f"w={w} cn={cn} range={data_range}")


# ---- g. the samplers in front of the march ----------------------------------------------------------------------
def _cubic_ofs(n_src, n_dst):
    """First-tap offsets of cubic_table (csrc/sr_assess.hip): floor of the fp32 source coordinate."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    return [int(math.floor(np.float32((d + 0.5) * scale - 0.5))) for d in range(n_dst)]


def _sampler(h, w, cn, dh, dw, march_switch):
    """The host rule of sr_assess_resized_u8_async, restated: which kernel samples this shape."""
    if not (cn == 3 and dw < w and dh < h):
        return "generic"                                    # k_resize_gray_pair<CN>
    ofs = _cubic_ofs(w, dw)

    def window_pitch(cols):
        span = 0
        for x0 in range(0, dw, cols):
            lo, hi = max(ofs[x0] - 1, 0), min(ofs[min(x0 + cols - 1, dw - 1)] + 2, w - 1)
            span = max(span, (hi + 1) * 3 - ((lo * 3) & ~15))
        return (span + 15) // 16 * 16 + 16

    lp = window_pitch(64)
    march = lp <= 64 * 16 + 16 or window_pitch(32) <= 64 * 16 + 16
    if march and march_switch != "0":
        return "march"                                      # k_resize_gray_pair_march
    return "lds" if 32 * lp <= 64 * 1024 else "generic"     # k_resize_gray_pair_lds / k_resize_gray_pair<3>


# (source shape, (dst_h, dst_w), SR_RESIZE_MARCH, the sampler _sampler() derives from window_pitch)
RESIZED = [
    # the down-sampling shapes of test_assess_resized_equals_resize_then_assess through the block-staged sampler ...
    *[(s, d, "0", "lds") for s, d in [((300, 411, 3), (111, 152)), ((193, 257, 3), (19, 25)), ((64, 64, 3), (5, 6)),
                                      ((257, 300, 3), (129, 151)), ((100, 700, 3), (77, 333)), ((333, 90, 3), (100, 81)),
                                      ((70, 200, 3), (65, 66)), ((400, 330, 3), (80, 66)), ((391, 345, 3), (100, 90)),
                                      ((300, 640, 3), (61, 128)), ((600, 1000, 3), (60, 100)), ((410, 777, 3), (50, 90))]],
    # ... and two of them through the column march, which that test compares with the oracle for SSE and uniform only
    ((257, 300, 3), (129, 151), None, "march"), ((600, 1000, 3), (60, 100), None, "march"),
    # scale 0.067 on a wide source: 64 destination columns span 2880 source bytes (> 2048: no LDS window), 32 span 1440
    # (> 1040: no march), so the generic kernel down-samples it, with or without the switch
    ((200, 1500, 3), (14, 100), None, "generic"), ((200, 1500, 3), (14, 100), "0", "generic"),
    # up-sampling and mixed (one axis up, one down), and every one-channel shape: the generic kernel
    ((40, 50, 3), (97, 131), None, "generic"), ((40, 50), (97, 131), None, "generic"),
    ((120, 60, 3), (50, 140), None, "generic"), ((120, 60), (50, 140), None, "generic"),
    ((60, 140, 3), (120, 50), None, "generic"), ((60, 140), (120, 50), None, "generic"),
    ((128, 640), (51, 256), "0", "generic"),
]


@pytest.mark.parametrize("shape,dst,switch,sampler", RESIZED)
def test_resized_samplers_match_resize_then_reference(ctx, rng, monkeypatch, shape, dst, switch, sampler):
    """sr_assess_resized_u8 against the oracle's cv2.resize(INTER_CUBIC) of both images followed by the float64 maps --
    not against sr_assess_u8 of the GPU's own resize."""
    h, w = shape[:2]
    cn = 3 if len(shape) == 3 else 1
    dh, dw = dst
    assert _sampler(h, w, cn, dh, dw, switch) == sampler
    if switch is not None:
        monkeypatch.setenv("SR_RESIZE_MARCH", switch)
    a, b = _pair(rng, h, w, cn)
    key = ("resized", shape, dst)
    if key not in _pairs:
        _pairs[key] = (oc.resize_cubic_u8(a, dw, dh), oc.resize_cubic_u8(b, dw, dh))
    oa, ob = _pairs[key]
    da, db = ctx.upload(a), ctx.upload(b)
    try:
        for data_range in RANGES:
            ref = _ref(key, oa, ob, data_range)
            got = ctx.assess_resized_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, dh, dw, flags=ALL, data_range=data_range)
            _check(got, ref, ALL, what=f"{shape}->{dst} {sampler} range={data_range}")
    finally:
        da.free()
        db.free()
