"""GPU: sr_color_correct_u8 at EVERY radius 1..16 of both local filters, byte for byte against oracle_np.

include/sr_hip.h promises radius 1..16 and results that do not depend on which kernels run; the other test files compare
with the oracle at radius 8 only.  Here ctx.color_correct_u8 is called directly and

    want = clip(f(corrected, img.astype(float32), radius, eps), 0, 255).astype(uint8)
    corrected[..., c] = table[c][img[..., c]]                  (float32)
    f = oracle_np.simple_guided_filter     for local_filter 1  (r x r box, anchor r // 2, BORDER_REFLECT_101)
    f = oracle_np.guided_filter_ximgproc   for local_filter 2  ((2 r + 1)^2 box, centred, BORDER_REFLECT)

No tolerance: both sides spell out one summation order (window row left to right, row sums top to bottom, fp64), the library
is compiled with -ffp-contract=off, and every other operation is one IEEE fp32 operation on both sides.

Which kernels a parametrisation reaches (csrc/sr_adjust.hip, sr_color_correct_u8):

  local_filter 1
    radius != 8                     k_cc_coeff + k_cc_apply (dynamic LDS; radius 9 is the last launch at or under 64 KiB of
                                    LDS, radius 10 the first above it, radius 16 the largest: 83 088 bytes)
    radius 8, h < 16 or w < 16      k_cc_coeff8 + k_cc_apply8 (the unfused radius-8 kernels; also every in-place call)
    radius 8, h >= 16 and w >= 16   k_cc_fused8 / k_cc_fused8f / k_cc_coeff8 + k_cc_apply8 by the table's class
  local_filter 2
    radius != 8, cn 1               k_gf_planes, 4 x k_gf_box, k_gf_coeff, 2 x k_gf_box, k_gf_out (its cn == 1 branch)
    radius != 8, cn 3               k_gf_planes, 21 x k_gf_box, k_gf_coeff, 12 x k_gf_box (the nmab = 12 second-stage means),
                                    k_gf_out's THREE-CHANNEL branch: R = 2 r + 1 != 17, so the host's `cn == 3 && R == GB_R`
                                    test fails and neither k_gfx_coeff17 nor k_gf_box17_out can be chosen.  That is every
                                    (ximgproc, cn 3, radius != 8) id below: 15 radii at (37, 131), 6 at each other shape,
                                    the flat / noise cases and the in-place cases.
    radius 8, cn 3                  k_gfx_coeff17 (integer table, out of place) or 21 x k_gf_box17 + k_gf_coeff, then
                                    k_gf_box17_out -- never k_gf_out
    radius 8, cn 1                  k_gf_box17 for the six box means, k_gf_out's cn == 1 branch

Blocks are 64 x 16 outputs.  Shapes: (37, 131) 3 x 3 blocks, ragged right and bottom, an interior block whose halo is all
real data at small radii; (16, 64) exactly one block; (5, 7) smaller than every window from radius 4 up (reflection
iterates); (1, 40) and (40, 1) the n == 1 branch of cc_reflect101 / gf_reflect; (17, 65) one row and one column into the
second block.  Radii: all sixteen at (37, 131); elsewhere {1, 2, 7, 9, 10, 16} -- both anchor parities, the LDS threshold,
the largest -- and 8 only where h < 16 or w < 16."""
import numpy as np
import pytest

from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

BIG = (37, 131)
SMALL = [(16, 64), (5, 7), (1, 40), (40, 1), (17, 65)]
FILTERS = [(1, 1), (1, 3), (1, 4), (2, 1), (2, 3)]                 # (local_filter, cn)
FILTER_IDS = [f"{'simple' if lf == 1 else 'ximgproc'}-cn{cn}" for lf, cn in FILTERS]
EPS = (0.01, 1e-4)
FILL = 0x5B


def _small_radii(shape):
    return [1, 2, 7] + ([8] if min(shape) < 16 else []) + [9, 10, 16]


SWEEP = [(BIG, r) for r in range(1, 17)] + [(s, r) for s in SMALL for r in _small_radii(s)]


def _tables(cn):
    """identity; an integer table that is not the identity, different per channel; a float mean_std-style table with
    entries below 0 and above 255 (guide != source in the last two)."""
    v = np.arange(256, dtype=np.float64)
    ident = np.tile(np.arange(256, dtype=np.float32), (cn, 1))
    whole = np.stack([np.clip(np.rint(v * (0.9 - 0.1 * c) + 10 + 7 * c), 0, 255) for c in range(cn)]).astype(np.float32)
    base = np.arange(256, dtype=np.float32)[None, :]
    c = np.arange(cn, dtype=np.float32)[:, None]
    flt = (base - (np.float32(140.25) + np.float32(3.0) * c)) * (np.float32(2.5) - np.float32(0.25) * c) + (np.float32(100.5) + c)
    assert flt.dtype == np.float32 and flt.min() < 0 and flt.max() > 255 and not np.array_equal(whole, ident)
    return {"identity": ident, "integer": whole, "float": np.ascontiguousarray(flt)}


def _scene(rng, h, w, cn):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(xx / 19.0) + 40 * np.cos(yy / 13.0)
    img = base[..., None] + rng.integers(-25, 26, (h, w, cn)) + np.arange(cn) * 9
    return np.clip(img, 0, 255).astype(np.uint8)


_IMAGES = {}


def _image(rng, shape, cn):
    """One scene per (shape, cn), made once and shared."""
    key = (shape, cn)
    if key not in _IMAGES:
        _IMAGES[key] = _scene(rng, shape[0], shape[1], cn)
        _IMAGES[key].setflags(write=False)
    return _IMAGES[key]


def _want(img, lut, local_filter, radius, eps):
    """The reference bytes, or None where the reference leaves its domain (a NaN / inf: its cast to u8 is undefined on both
    sides); img is (h, w, cn), the oracle takes gray images as (h, w)."""
    cn = img.shape[2]
    corrected = np.stack([lut[c][img[..., c]] for c in range(cn)], axis=-1).astype(np.float32)
    src = img.astype(np.float32)
    if cn == 1:
        corrected, src = corrected[..., 0], src[..., 0]
    f = onp.simple_guided_filter if local_filter == 1 else onp.guided_filter_ximgproc
    with np.errstate(all="ignore"):
        q = f(corrected, src, radius, eps)
    if not np.all(np.isfinite(q)):
        return None
    return np.clip(q, 0, 255).astype(np.uint8).reshape(img.shape)


def _run(ctx, img, lut, local_filter, radius, eps, in_place=False):
    h, w, cn = img.shape
    d = ctx.upload(img)
    o = d if in_place else ctx.alloc(img.size)
    try:
        ctx.color_correct_u8(d.ptr, w * cn, h, w, cn, lut, local_filter, radius, eps, o.ptr, w * cn)
        return ctx.download(o.ptr, img.shape, np.uint8)
    finally:
        d.free()
        if not in_place:
            o.free()


def _compare(ctx, img, local_filter, radius, tables=None, eps_list=EPS, in_place=False, redraw=None):
    """Every table x eps of one (image, filter, radius).  The colour form of local_filter 2 inverts a 3 x 3 covariance whose
    window may hold fewer than four distinct pixels (radius 1 on a one-pixel-wide image: three): its fp32 determinant is then
    eps times a rounding residue and can come out exactly 0.  Such an image is outside the reference's domain whatever the
    kernel does, so it is drawn again (redraw; three times at the most) -- the case itself stays."""
    cn = img.shape[2]
    tables = tables or _tables(cn)
    for attempt in range(4):
        wants = {(name, eps): _want(img, lut, local_filter, radius, eps) for name, lut in tables.items() for eps in eps_list}
        if all(w is not None for w in wants.values()):
            break
        assert redraw is not None and attempt < 3, f"the reference is not finite: {[k for k, w in wants.items() if w is None]}"
        img = redraw()
    for name, lut in tables.items():
        for eps in eps_list:
            want = wants[name, eps]
            got = _run(ctx, img, lut, local_filter, radius, eps, in_place)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (f"filter {local_filter} cn {cn} shape {img.shape[:2]} radius {radius} table {name} eps {eps}"
                                   f"{' in place' if in_place else ''}: {len(bad)} bytes differ, first at {bad[0].tolist()}: "
                                   f"got {int(got[tuple(bad[0])])} want {int(want[tuple(bad[0])])}")


@pytest.mark.parametrize("local_filter,cn", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("shape,radius", SWEEP, ids=[f"{s[0]}x{s[1]}-r{r}" for s, r in SWEEP])
def test_radius_sweep(ctx, rng, shape, radius, local_filter, cn):
    """Three tables x two eps per id.  The first hardware launch of radius >= 10 with local_filter 1 (more than 64 KiB of
    dynamic LDS) is the r10 .. r16 ids of this test."""
    _compare(ctx, _image(rng, shape, cn), local_filter, radius, redraw=lambda: _scene(rng, shape[0], shape[1], cn))


@pytest.mark.parametrize("local_filter,cn", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("radius", [1, 3, 16])
def test_flat_image_is_a_fixed_point(ctx, radius, local_filter, cn):
    """Zero variance everywhere: a = 0 / eps (identity table: cov = var = 0 exactly, every mean of a constant is the
    constant), b = mean -- with the identity table the output is the image itself, with the others the oracle's bytes."""
    for shape in (BIG, (17, 65)):
        flat = np.full(shape + (cn,), 77, np.uint8)
        tabs = _tables(cn)
        _compare(ctx, flat, local_filter, radius, tabs)
        for eps in EPS:
            assert np.array_equal(_run(ctx, flat, tabs["identity"], local_filter, radius, eps), flat), (shape, radius, eps)


@pytest.mark.parametrize("local_filter,cn", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("radius", [3, 16])
def test_full_range_noise(ctx, rng, radius, local_filter, cn):
    """rng.integers(0, 256): every byte value, no spatial correlation -- large variances and covariances of either sign."""
    key = ("noise", cn)
    if key not in _IMAGES:
        _IMAGES[key] = rng.integers(0, 256, BIG + (cn,), dtype=np.uint8)
        _IMAGES[key].setflags(write=False)
    _compare(ctx, _IMAGES[key], local_filter, radius, redraw=lambda: rng.integers(0, 256, BIG + (cn,), dtype=np.uint8))


@pytest.mark.parametrize("local_filter", [1, 2], ids=["simple", "ximgproc"])
@pytest.mark.parametrize("radius", [5, 12])
def test_in_place(ctx, rng, radius, local_filter):
    """d_out == d_img at an odd radius under the LDS threshold and an even one above it: the pass-structured kernels read
    the whole image into a / b (or the float planes) before the first byte is stored."""
    for cn in (3, 1):
        tabs = _tables(cn)
        _compare(ctx, _image(rng, BIG, cn), local_filter, radius, {k: tabs[k] for k in ("integer", "float")}, in_place=True,
                 redraw=lambda: _scene(rng, BIG[0], BIG[1], cn))


def _refused(ctx, img, lut, local_filter, radius):
    """The call must raise ValueError (SR_ERR_INVALID_ARG) and leave a fill-byte output untouched."""
    h, w, cn = img.shape
    d, o = ctx.upload(img), ctx.alloc(img.size)
    try:
        ctx.memset(o.ptr, FILL, img.size)
        with pytest.raises(ValueError) as ei:
            ctx.color_correct_u8(d.ptr, w * cn, h, w, cn, lut, local_filter, radius, 0.01, o.ptr, w * cn)
        assert not isinstance(ei.value, _shape_error()), "SR_ERR_INVALID_ARG expected, not SR_ERR_SHAPE"
        assert np.all(ctx.download(o.ptr, img.shape, np.uint8) == FILL), (local_filter, radius, cn, "output was written")
    finally:
        d.free()
        o.free()


def _shape_error():
    import _native
    return _native.SrShapeError


@pytest.mark.parametrize("local_filter", [1, 2], ids=["simple", "ximgproc"])
@pytest.mark.parametrize("radius", [0, 17, -1])
def test_radius_outside_1_16_is_refused(ctx, rng, radius, local_filter):
    img = _image(rng, (17, 65), 3)
    _refused(ctx, img, _tables(3)["integer"], local_filter, radius)


@pytest.mark.parametrize("cn", [2, 4])
def test_ximgproc_refuses_two_and_four_channels(ctx, rng, cn):
    img = _scene(rng, 17, 65, cn)
    for radius in (5, 8):
        _refused(ctx, img, _tables(cn)["integer"], 2, radius)


@pytest.mark.parametrize("radius", [0, 17, -3, 8])
def test_radius_is_ignored_without_a_local_filter(ctx, rng, radius):
    """local_filter 0 is the table alone, whatever the radius says: out = u8(clip(table[c][v], 0, 255))."""
    for cn in (1, 3, 4):
        img = _image(rng, (17, 65), cn)
        for name, lut in _tables(cn).items():
            want = np.clip(np.stack([lut[c][img[..., c]] for c in range(cn)], axis=-1), 0, 255).astype(np.uint8)
            assert np.array_equal(_run(ctx, img, lut, 0, radius, 0.01), want), (cn, name, radius)
