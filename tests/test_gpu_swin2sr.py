"""GPU: the Swin2SR backend of csrc/sr_swin2sr.hip (SwinV2 cosine window attention with a continuous position bias, post-norm,
1 x 1 projections) against

* the golden fixtures tests/golden/swin2sr_*.npz: random-weight models of `transformers` 5.15.0's
  Swin2SRForImageSuperResolution run in float64 (tests/golden/make_swin2sr_golden.py) -- the package's key layout is PINNED;
* the restatement tests/_swin2sr_ref.py (which reproduces those fixtures to 1e-9, tests/test_swin2sr_host.py) on seeded
  synthetic weights, for what the package cannot give: other widths, the other upsamplers, sides that are no multiple of 8, the
  official key layout and its -100 mask.

The bar is the project's: err <= 8 e32, e32 = the float32 restatement's distance from the float64 truth on the same input.  Also:
the u8 output byte for byte away from rounding boundaries, the padding probe, the attention and the LayerNorm + skip on their own
(sr_swin2sr_attention_f32, sr_swin2sr_layernorm_add_f32) on padded, offset views in guarded parents, every tail bit-equal, a
0xFF-filled workspace, determinism, strided views, refusals, the ensemble, the network class and the pipeline with
``sr_weights``.  The largest input of the float bar is 24 x 40; the pipeline's picture is larger because it needs several blocks."""
import asyncio
import math
import os

import numpy as np
import pytest

import _ensemble_ref as E
import _swin2sr_ref as ref
import _views as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("swin2sr_direct_x2.npz", "swin2sr_shuffle_x2.npz")


@pytest.fixture(scope="module")
def nets():
    """One network per description (and mask value), made once and closed at teardown."""
    import sr_network
    cache = {}

    def get(*key, mask_value=None):
        k = key + (mask_value,)
        if k not in cache:
            cache[k] = sr_network.Swin2SRNet(ref.synthetic_state(*key), mask_value=mask_value)
        return cache[k]

    yield get
    for n in cache.values():
        n.close()


def _f32(ctx, net, img, tail=0):
    h, w = img.shape[:2]
    s = net.scale
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * s * w * s * 3 * 4)
    try:
        net.model(ctx).forward_f32(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * 3 * 4, tail)
        return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.float32)
    finally:
        d_src.free(); d_dst.free()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _round_u8(f):
    return np.rint(np.clip(f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def _ulps(a, b):
    """Distance in fp32 units in the last place (both finite)."""
    def key(x):
        i = _bits(x.astype(np.float32)).astype(np.int64)
        return np.where(i < 2 ** 31, i, 2 ** 31 - i)
    return np.abs(key(a) - key(b))


def _exempt_cap(e32):
    """The share of bytes check_u8 may exempt.  A byte is exempt where the float64 level lies within 255 * 8 * e32 of a rounding
    boundary; with fractional parts spread evenly that is 2 * 255 * 8 * e32 of the bytes (4 % at e32 = 1e-5, where the other
    families' 1 % was set for e32 near 1e-6), a quarter on top for the spread.  It depends on the reference alone, not on the
    code under test."""
    return min(1.0, 1.25 * 2 * 255 * 8 * e32)


def _bar(ctx, net, state, img, f64, e32, what):
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"swin2sr {what}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert got.shape == f64.shape and np.isfinite(got).all()
    assert 0 < e32 < 1e-3
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32, _exempt_cap(e32))
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, _round_u8(got))                     # the float form rounded


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("layout", ["package", "official"])
def test_golden_fixtures_of_the_package(ctx, name, layout):
    """The package's float64 outputs, through the package's key layout (mask -200 from the parser) and through the same state
    converted to the official layout with the mask set back to the package's -200: one kernel path, two parsers."""
    import sr_network
    state, cases = ref.load_golden(os.path.join(GOLDEN, name))
    if layout == "package":
        net = sr_network.Swin2SRNet(state)
    else:
        net = sr_network.Swin2SRNet(ref.to_official(state), mask_value=ref.MASK_PACKAGE)
    assert net.mask_value == ref.MASK_PACKAGE
    try:
        for img, f64 in cases:
            _bar(ctx, net, state, img, f64, ref.e32_of(state, img, f64), f"{name} {layout} {img.shape[0]}x{img.shape[1]}")
    finally:
        net.close()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    net = nets(*case[:7])
    state, img, f64, e32 = ref.case(*case)
    _bar(ctx, net, state, img, f64, e32, ref.case_id(case))


def test_official_layout_and_its_mask(ctx):
    """The official key layout parses to the -100 mask, and the forward follows the restatement run with -100."""
    import sr_network
    case = ref.CASES[1]
    state, img, f64, e32 = ref.case(*case, ref.MASK_OFFICIAL)
    net = sr_network.Swin2SRNet(ref.to_official(state))
    try:
        assert net.mask_value == ref.MASK_OFFICIAL
        _bar(ctx, net, state, img, f64, e32, "official layout, mask -100")
    finally:
        net.close()


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[3]], ids=ref.case_id)
def test_padding_probe(ctx, nets, case):
    """forward(img) == forward(np.pad(img, symmetric)) cropped, bit for bit: the padded picture is what the trunk sees."""
    net = nets(*case[:7])
    img = ref.case(*case)[1]
    h, w, s = img.shape[0], img.shape[1], case[5]
    padded = ref.pad_image(img)
    assert padded.shape[:2] != img.shape[:2]
    a, b = _f32(ctx, net, img), _f32(ctx, net, padded)[:h * s, :w * s]
    assert np.array_equal(_bits(a), _bits(b))


def _planar_in(ctx, x, k, fill):
    """Planes (P, h, w) fp32 one below the other inside a guarded parent -> (parent, pointer, plane stride, row stride)."""
    P, h, w = x.shape
    parent, ptr, stride = V.embed(ctx, np.ascontiguousarray(x).view(np.uint8).reshape(P * h, w * 4), *V.pick(V.LAYOUTS_F32, k), fill)
    return parent, ptr, h * stride, stride


def _attention(ctx, qkv, table, scale, mask_value, heads, shift, k, fill):
    import _native
    C3, hp, wp = qkv.shape
    C = C3 // 3
    src, d_x, ps, rs = _planar_in(ctx, qkv, k, fill)
    dst, d_out, ostride = V.out_view(ctx, C * hp, wp * 4, *V.pick(V.LAYOUTS_F32, k + 3), fill)
    try:
        _native.swin2sr_attention(ctx, d_x, ps, rs, C, heads, hp, wp, shift, table, scale, mask_value, d_out, hp * ostride, ostride)
        return V.check_guard(ctx, dst, np.float32, (C, hp, wp), what="swin2sr attention")
    finally:
        src.free(); dst.free()


@pytest.mark.parametrize("hp,wp", [(8, 8), (16, 24)])
@pytest.mark.parametrize("d", [8, 10, 30])
def test_attention_zero_probe_is_bit_exact(ctx, hp, wp, d):
    """q = k = 0 (the norm 0 is lifted to 1e-12, the unit vectors are 0 and no NaN appears), a zero bias, positive integer-valued
    v: every score is 0 (or the mask value across regions), so the output is the mean of v over the tokens of the same window and
    region -- 16, 32 or 64 of them -- exactly, in any summation order.  Zero tolerance on the roll, the partition, the mask and
    the write-back, at shift 0 and 4 and at both mask values; a scale of 100 must not matter."""
    heads = 2
    C = heads * d
    rng = np.random.default_rng(hp * 100 + wp + d)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = rng.integers(1, 1000, (C, hp, wp)).astype(np.float32)
    table = np.zeros((225, heads), np.float32)
    scale = np.array([100.0, 3.0], np.float32)
    for shift in (0, 4):
        for mv in (ref.MASK_PACKAGE, ref.MASK_OFFICIAL):
            want = ref.np_attention(qkv, table, scale, heads, shift, mv, np.float64)
            want32 = want.astype(np.float32)
            assert np.array_equal(want32.astype(np.float64) * 64, np.round(want * 64))      # multiples of 1 / 64: exact in fp32
            got = _attention(ctx, qkv, table, scale, mv, heads, shift, d + shift, V.FILLS[shift // 4])
            bad = np.argwhere(_bits(got) != _bits(want32))
            assert not len(bad), (shift, mv, len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


@pytest.mark.parametrize("hp,wp", [(8, 8), (16, 24)])
def test_attention_bias_parity_probe_is_bit_exact(ctx, hp, wp):
    """q = k = 0 and a bias table of 0 and -1000: head 0 keeps the keys whose column offset to the query is even, head 1 those
    whose row offset is even (exp(-1000) is 0 in fp32), so a query weighs half of the keys of its window and region -- 8, 16 or 32
    of them -- by exactly 1 / n and the output is their mean of integer-valued v: exact in any order, bit for bit.  A transposed
    table, a wrong relative-position index, swapped heads or offsets, the roll, the partition and the mask (both values) all show."""
    heads, d = 2, 10
    C = heads * d
    rng = np.random.default_rng(hp + wp)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = rng.integers(1, 1000, (C, hp, wp)).astype(np.float32)
    t = np.arange(225)
    dy, dx = t // 15 - 7, t % 15 - 7
    table = np.stack([np.where(dx % 2 == 0, 0.0, -1000.0), np.where(dy % 2 == 0, 0.0, -1000.0)], 1).astype(np.float32)
    scale = np.array([100.0, 3.0], np.float32)
    for shift in (0, 4):
        for mv in (ref.MASK_PACKAGE, ref.MASK_OFFICIAL):
            want = ref.np_attention(qkv, table, scale, heads, shift, mv, np.float64)
            want32 = want.astype(np.float32)
            assert np.array_equal(want32.astype(np.float64) * 32, np.round(want * 32))      # multiples of 1 / 32: exact in fp32
            assert not np.array_equal(want, ref.np_attention(qkv, table[:, ::-1], scale, heads, shift, mv, np.float64))
            got = _attention(ctx, qkv, table, scale, mv, heads, shift, 7 + shift, V.FILLS[shift // 4])
            bad = np.argwhere(_bits(got) != _bits(want32))
            assert not len(bad), (shift, mv, len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


@pytest.mark.parametrize("shift", [0, 4])
def test_attention_bias_probe_is_within_the_bar(ctx, shift):
    """q = k = 0, a random position bias in 16 sigmoid's range, one-hot v: o_i[dd] = the sum of p[i][j] over the keys j = dd mod d, so
    a transposed table, a wrong index or a swapped head axis shows."""
    heads, d, hp, wp = 3, 10, 16, 24
    C = heads * d
    rng = np.random.default_rng(31 + shift)
    table = rng.uniform(0.0, 16.0, (225, heads)).astype(np.float32)
    scale = np.array([100.0, 7.0, 30.0], np.float32)
    onehot = (np.arange(64)[None, :] % d == np.arange(d)[:, None]).astype(np.float32)             # (dd, token)
    v = ref._unwindows(np.broadcast_to(np.tile(onehot, (heads, 1))[:, None, :], (C, hp * wp // 64, 64)).copy(), hp, wp)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = np.roll(v, (shift, shift), (1, 2)) if shift else v
    _attention_bar(ctx, qkv, table, scale, ref.MASK_PACKAGE, heads, shift, 1 + shift, "bias probe")
    wrong = ref.np_attention(qkv, table[:, ::-1], scale, heads, shift, ref.MASK_PACKAGE, np.float64)
    assert np.abs(wrong - ref.np_attention(qkv, table, scale, heads, shift, ref.MASK_PACKAGE, np.float64)).max() > 1e-2


@pytest.mark.parametrize("d", [8, 10, 30])
def test_attention_one_hot_scores_are_exactly_the_scale(ctx, d):
    """One-hot q and k (one channel per head) with power-of-two magnitudes from 2^-20 to 2^20 and signs: the sums of squares, the
    roots and the divisions are exact, so every score must be EXACTLY +scale_h or -scale_h.  Every window holds 32 keys of either
    sign, and exp(-2 scale_h) is 0 in fp32, so a query weighs the 32 keys of its own sign by exactly 1 / 32 and the output is the
    mean of their small-integer v: exact in any order, compared bit for bit.  One score off by an ulp of 100 (a reciprocal in
    place of the division, the scale applied before the sum, the norm from another order) makes exp(a - max) differ from 1 and
    the bits move."""
    heads, hp, wp = 2, 16, 24
    C = heads * d
    rng = np.random.default_rng(77 + d)
    nwin = hp * wp // 64

    chans = [int(rng.integers(0, d)) for _ in range(heads)]       # the same channel for q and k of a head, else every score is 0

    def onehot(sign):                                             # sign (windows, 64) -> planes (C, hp, wp)
        out = np.zeros((C, nwin, 64), np.float32)
        for hd in range(heads):
            out[hd * d + chans[hd]] = sign * (2.0 ** rng.integers(-20, 21, (nwin, 64))).astype(np.float32)
        return ref._unwindows(out, hp, wp)

    ksign = np.stack([rng.permutation(np.repeat([-1.0, 1.0], 32)) for _ in range(nwin)]).astype(np.float32)
    qsign = rng.choice([-1.0, 1.0], (nwin, 64)).astype(np.float32)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    q, k = onehot(qsign), onehot(ksign)
    qkv[:C], qkv[C:2 * C] = q, k
    qkv[2 * C:] = rng.integers(-8, 9, (C, hp, wp)).astype(np.float32)
    table = np.zeros((225, heads), np.float32)
    scale = np.array([100.0, 64.0], np.float32)
    want = ref.np_attention(qkv, table, scale, heads, 0, ref.MASK_PACKAGE, np.float64)
    want32 = want.astype(np.float32) + np.float32(0.0)       # a mean of 0 is +0: the contract's chains start at +0, numpy's matmul may give -0
    assert np.array_equal(want32.astype(np.float64) * 32, np.round(want * 32))          # multiples of 1 / 32: exact in fp32
    assert np.abs(want).max() > 0
    got = _attention(ctx, qkv, table, scale, ref.MASK_PACKAGE, heads, 0, 5 + d, V.FILLS[0])
    bad = np.argwhere(_bits(got) != _bits(want32))
    assert not len(bad), (len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


def _attention_bar(ctx, qkv, table, scale, mv, heads, shift, k, what):
    want64 = ref.np_attention(qkv, table, scale, heads, shift, mv, np.float64)
    chain = ref.np_attention(qkv, table, scale, heads, shift, mv, np.float32, chain=True)
    e32 = float(np.max(np.abs(chain.astype(np.float64) - want64)))
    got = _attention(ctx, qkv, table, scale, mv, heads, shift, k, V.FILLS[k % 2])
    err = float(np.max(np.abs(got.astype(np.float64) - want64)))
    print(f"swin2sr attention {what} shift {shift}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert e32 > 0 and err <= 8 * e32, (err, e32)


@pytest.mark.parametrize("heads,d,hp,wp,shift,mv", [(6, 30, 16, 24, 4, -200.0), (2, 32, 8, 8, 4, -100.0), (4, 16, 24, 16, 0, -200.0),
                                                     (3, 4, 16, 8, 4, -100.0), (3, 8, 16, 16, 4, -200.0), (2, 10, 8, 16, 4, -200.0)])
def test_attention_random(ctx, heads, d, hp, wp, shift, mv):
    """Random q, k, v, bias in [0, 16] and scales on both sides of 10, within 8 e32 of float64; e32 is the documented order in
    fp32 (tests/_swin2sr_ref.np_attention, chain=True)."""
    C = heads * d
    rng = np.random.default_rng(heads * 10 + d)
    qkv = (rng.standard_normal((3 * C, hp, wp)) * 2).astype(np.float32)
    table = rng.uniform(0.0, 16.0, (225, heads)).astype(np.float32)
    scale = np.exp(rng.uniform(math.log(3.0), math.log(100.0), heads)).astype(np.float32)
    scale[0] = 100.0
    _attention_bar(ctx, qkv, table, scale, mv, heads, shift, heads + d, f"random {heads}x{d} {hp}x{wp}")


def _layernorm_add(ctx, x, gamma, beta, skip, k, fill, in_place):
    import _native
    C, h, w = x.shape
    src, d_x, ps, rs = _planar_in(ctx, x, k, fill)
    sk, d_s, sps, srs = _planar_in(ctx, skip, k + 1, fill)
    dst, d_out, ostride = V.out_view(ctx, C * h, w * 4, *V.pick(V.LAYOUTS_F32, k + 2), fill)
    try:
        if in_place:
            _native.swin2sr_layernorm_add(ctx, d_x, ps, rs, C, h, w, gamma, beta, d_s, sps, srs, d_s, sps, srs)
            return V.check_guard(ctx, sk, np.float32, (C, h, w), what="swin2sr layernorm + skip, in place")
        _native.swin2sr_layernorm_add(ctx, d_x, ps, rs, C, h, w, gamma, beta, d_s, sps, srs, d_out, h * ostride, ostride)
        return V.check_guard(ctx, dst, np.float32, (C, h, w), what="swin2sr layernorm + skip")
    finally:
        src.free(); sk.free(); dst.free()


@pytest.mark.parametrize("C,h,w,k", [(60, 5, 37, 1), (24, 16, 24, 2), (180, 3, 40, 3)])
def test_layernorm_add_alone(ctx, C, h, w, k):
    """sr_swin2sr_layernorm_add_f32 on padded, offset views, into a buffer of its own and in place over the skip: within one ulp of
    the float64 form skip + (float)LN(x) (the kernel's one fp32 add rounds it: half an ulp)."""
    rng = np.random.default_rng(300 + k)
    x = (rng.standard_normal((C, h, w)) * 3 + rng.standard_normal((1, h, w))).astype(np.float32)
    skip = (rng.standard_normal((C, h, w)) * 2).astype(np.float32)
    g, b = rng.uniform(0.8, 1.2, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)
    want = ref.np_layernorm_add(x, g, b, skip)
    for fill, in_place in zip(V.FILLS, (False, True)):
        got = _layernorm_add(ctx, x, g, b, skip, k, fill, in_place)
        u = _ulps(got, want.astype(np.float32))
        print(f"swin2sr layernorm + skip C{C} {h}x{w} in_place={in_place}: worst {int(u.max())} ulp")
        assert u.max() <= 1


def test_inspection_refusals():
    import _native
    one = np.ones(4, np.float32)
    t1, s1 = np.zeros((225, 1)), np.ones(1)
    with pytest.raises(NotImplementedError):
        _native.swin2sr_layernorm_add(None, 256, 64, 16, 300, 4, 4, np.ones(300), np.ones(300), 512, 64, 16, 1024, 64, 16)
    with pytest.raises(ValueError):
        _native.swin2sr_layernorm_add(None, 256, 64, 12, 4, 4, 4, one, one, 512, 64, 16, 1024, 64, 16)      # a row stride below a row
    with pytest.raises(ValueError):
        _native.swin2sr_layernorm_add(None, 256, 64, 16, 4, 4, 4, one, one, 512, 64, 16, 256, 64, 16)       # the output is x itself
    with pytest.raises(ValueError):
        _native.swin2sr_attention(None, 256, 4 * 64 * 8, 32, 4, 1, 8, 12, 0, t1, s1, -200.0, 256, 4 * 64 * 8, 48)   # 12 columns
    with pytest.raises(NotImplementedError):
        _native.swin2sr_attention(None, 256, 4 * 64 * 8, 32, 4, 1, 8, 8, 2, t1, s1, -200.0, 256, 4 * 64 * 8, 32)    # shift 2
    with pytest.raises(NotImplementedError):
        _native.swin2sr_attention(None, 256, 4 * 64 * 8, 32, 66, 2, 8, 8, 0, np.zeros((225, 2)), np.ones(2), -200.0, 256, 4 * 64 * 8, 32)   # d = 33
    with pytest.raises(NotImplementedError):
        _native.swin2sr_attention(None, 256, 4 * 64 * 8, 32, 4, 1, 8, 8, 0, t1, s1, float("nan"), 256, 4 * 64 * 8, 32)


TAIL_NETS = [((24, 3, 48, 1, 2, 2, "pixelshuffledirect"), 21, 37), ((24, 3, 48, 1, 1, 4, "pixelshuffle"), 13, 19),
             ((24, 3, 48, 1, 1, 3, "pixelshuffle"), 20, 11), ((24, 3, 48, 1, 2, 4, "nearest+conv"), 12, 21)]


@pytest.mark.parametrize("key,h,w", TAIL_NETS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_tail_is_bit_equal(ctx, nets, key, h, w):
    """fp32 bits and u8 bytes of every tail equal those of one tail piece; the plan is SwinIR's rule."""
    img = ref.make_image(h, w, seed=11)
    net = nets(*key)
    m = net.model(ctx)
    one_f, one_u = _f32(ctx, net, img, 64), net.upscale(img, tail=64)
    assert np.isfinite(one_f).all() and one_f.std() > 0
    assert np.array_equal(one_u, _round_u8(one_f))
    for tail in (1, 7, 64, 0):
        assert m.plan(h, w, tail) == ref.plan(key[0], key[2], key[5], key[6], h, w, tail)
        assert np.array_equal(_bits(_f32(ctx, net, img, tail)), _bits(one_f)), tail
        assert np.array_equal(net.upscale(img, tail=tail), one_u), tail


def test_deterministic_nan_workspace_and_regrowth(ctx):
    """Two runs give equal bits; the first forward after the workspace was filled with NaN bytes (0xFF) equals them; a larger
    image after a smaller one (the buffers are regrown) and the small one again; a second model of the same state agrees."""
    import sr_network
    key = (60, 6, 120, 1, 2, 2, "pixelshuffle")                   # C and hidden are not multiples of 64: padded planes exist
    st = ref.synthetic_state(*key)
    small, large = ref.make_image(13, 21), ref.make_image(24, 40)
    net, other = sr_network.Swin2SRNet(st), sr_network.Swin2SRNet(st)
    try:
        net.model(ctx).fill_workspace(13, 21, 0xFF)
        a = _f32(ctx, net, small)
        assert np.isfinite(a).all()
        b = _f32(ctx, net, small)
        assert np.array_equal(_bits(a), _bits(b))
        big = _f32(ctx, net, large)
        net.model(ctx).fill_workspace(24, 40, 0xFF)
        assert np.array_equal(_bits(_f32(ctx, net, large)), _bits(big))
        assert np.array_equal(_bits(_f32(ctx, net, small)), _bits(a))
        assert np.array_equal(_bits(_f32(ctx, other, small)), _bits(a)) and np.array_equal(_bits(_f32(ctx, other, large)), _bits(big))
        assert np.array_equal(net.upscale(small), _round_u8(a))
    finally:
        net.close(); other.close()


@pytest.mark.parametrize("case,k", [(ref.CASES[0], 1), (ref.CASES[1], 2), (ref.CASES[3], 3)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
def test_views(ctx, nets, case, k):
    """Padded, offset source view; destinations inside guarded parents; u8 (small tail) and fp32 entry points: equal bits and no
    byte written outside the view."""
    h, w, s = case[7], case[8], case[5]
    net, img = nets(*case[:7]), ref.case(*case)[1]
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 5)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="swin2sr u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="swin2sr f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_refusals(ctx, nets):
    """Bad arguments raise before any launch (the guarded output stays untouched); the cap is refused by message from a plan
    alone; a destroyed handle is refused, not dereferenced; a k bias and a non-finite logit scale are refused by the create."""
    import ctypes as C

    import _native
    net = nets(*ref.CASES[1][:7])
    img = ref.make_image(13, 21)
    h, w = 13, 21
    with pytest.raises(ValueError, match="no tile"):
        net.upscale(img, tile=16)
    with pytest.raises(ValueError):
        net.upscale(img[:, :, :1])
    m = net.model(ctx)
    with pytest.raises(ValueError, match="SR_SWIN2SR_TRUNK_CAP"):
        m.plan(6000, 6000)
    d_src = ctx.upload(img)
    dst, d_dst, dstride = V.out_view(ctx, h * 2, w * 2 * 3, 0, 0, V.FILLS[0])
    try:
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, w * 2 * 3 - 1, 0)          # destination stride shorter than a row
        with pytest.raises(ValueError):
            m.forward_f32(d_src.ptr, w * 3, h, w, d_dst, w * 2 * 3 * 4 - 4, 0)
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, 0, w, d_dst, dstride, 0)                # h = 0
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3 - 1, h, w, d_dst, dstride, 0)            # short source stride
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, -1)               # tail < 0
        with pytest.raises(TypeError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, 0, 0)             # there is no tile
        with pytest.raises(ValueError):
            m.upscale_u8(0, w * 3, h, w, d_dst, dstride, 0)
        gone = _native.Swin2srModel(ctx, net.desc, net._w, net._b)
        handle = C.c_void_p(gone.handle.value)
        gone.close()
        for fn in (ctx.lib.sr_swin2sr_u8, ctx.lib.sr_swin2sr_f32):
            assert fn(handle, C.c_void_p(d_src.ptr), w * 3, h, w, C.c_void_p(d_dst), dstride, 0) == _native.SR_ERR_INVALID_ARG
        assert "destroyed" in _native.last_error()
        assert ctx.lib.sr_swin2sr_destroy(handle) == _native.SR_OK                  # a second destroy is a no-op
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(ValueError):                                                 # a table of the wrong shape
        _native.Swin2srModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)
    with pytest.raises(ValueError):
        _native.Swin2srModel(ctx, net.desc, net._w[:-1], net._b[:-1])
    kb = [None if b is None else b.copy() for b in net._b]
    kb[3][net.n_feat + 1] = 0.5                                                     # table 3: the first layer's qkv
    with pytest.raises(NotImplementedError, match="k bias"):
        _native.Swin2srModel(ctx, net.desc, net._w, kb)
    lw = [a.copy() for a in net._w]
    lw[4][0] = np.inf                                                               # table 4: its logit_scale
    with pytest.raises(NotImplementedError, match="logit_scale"):
        _native.Swin2srModel(ctx, net.desc, lw, net._b)


def _run(ctx, net, img, ens=None, u8=False, tail=0):
    h, w = img.shape[:2]
    s = net.scale
    px = 3 if u8 else 12
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * s * w * s * px)
    try:
        m = net.model(ctx)
        if ens is None:
            (m.upscale_u8 if u8 else m.forward_f32)(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * px, tail)
        else:
            (m.ensemble_u8 if u8 else m.ensemble_f32)(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * px, tail, mask=ens)
        return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.uint8 if u8 else np.float32)
    finally:
        d_src.free(); d_dst.free()


def test_ensemble_equals_the_rule_bit_for_bit(ctx, nets):
    """Swin2SR+: members from the family's own forward_f32 on host-transformed inputs (each reflected and windowed on its own),
    summed in ascending order and divided as tests/_ensemble_ref.py states; masks 0x03 and 0xFF, fp32 bits and u8 bytes."""
    net = nets(24, 3, 48, 1, 2, 2, "pixelshuffledirect")
    img = ref.make_image(13, 21, seed=11)
    ys = [E.d4_inv(_run(ctx, net, E.d4(img, k)), k) for k in range(8)]
    assert not np.array_equal(ys[0], ys[1]) and not np.array_equal(ys[0], ys[4])     # the network is not equivariant
    for mask in (0x03, 0xFF):
        want = E.mean_f32([ys[k] for k in E.members(mask)])
        assert np.array_equal(_bits(_run(ctx, net, img, ens=mask)), _bits(want)), hex(mask)
        assert np.array_equal(_bits(_run(ctx, net, img, ens=mask, tail=5)), _bits(want)), hex(mask)
        assert np.array_equal(_run(ctx, net, img, ens=mask, u8=True), E.to_u8(want)), hex(mask)
    assert np.array_equal(net.upscale(img, ensemble=8), E.to_u8(E.mean_f32(ys)))


def test_network_class_upscale_and_upscale_device(ctx, nets):
    net = nets(*ref.CASES[1][:7])
    img = ref.make_image(19, 37)
    h, w = img.shape[:2]
    want = _round_u8(_f32(ctx, net, img))
    assert np.array_equal(net.upscale(img), want)
    src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, 4), V.FILLS[1])
    dst, d_dst, dstride = V.out_view(ctx, h * 2, w * 2 * 3, *V.pick(V.LAYOUTS_U8, 7), V.FILLS[1])
    try:
        net.upscale_device(d_src, (h, w, 3), d_dst, dstride, src_stride=sstride, ctx=ctx, tail=16)
        assert np.array_equal(V.check_guard(ctx, dst, np.uint8, (h * 2, w * 2, 3), what="upscale_device"), want)
    finally:
        src.free(); dst.free()
    import sr_network
    tmp = sr_network.Swin2SRNet(ref.synthetic_state(*ref.CASES[1][:7]))
    tmp.model(ctx)
    tmp.close()
    assert tmp._models == {}


def test_pipeline_with_sr_weights(tmp_path):
    """process() with sr_weights pointing at a saved Swin2SR (the package's layout with a ``mask_value`` entry): the family is
    picked from the file, the run stays device-resident, and tile 0 -- reflected, padded and windowed on its own, as every tile is
    -- matches the restatement."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(24, 3, 48, 1, 2, 2, "pixelshuffle")
    state["mask_value"] = np.array(-150.0, np.float32)               # a loader that drops the .npz entry must show
    wpath = str(tmp_path / "swin2sr.npz")
    np.savez(wpath, **state)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, block_size=64, sr_scale=2, num_pyramid_levels=4))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.Swin2SRNet) and pipe._builtin_backend()
    assert pipe.sr_net.desc.mask_value == np.float32(-150.0)                        # the .npz extras
    res = asyncio.run(pipe.process(src, str(tmp_path / "out.png")))
    assert res.success, res.error_message
    assert res.total_blocks == res.successful_blocks > 1 and res.failed_blocks == 0
    assert "sr_net" in pipe.stage_times and "sr_stub" not in pipe.stage_times
    assert pipe.transfers["h2d_bytes"] == img.nbytes                                # the network keeps the run device-resident
    assert np.asarray(Image.open(str(tmp_path / "out.png"))).shape == (160, 192, 3)
    tile0 = pipe.tiling_module.split_image(src)[0].data
    del state["mask_value"]
    f64 = ref.forward(state, tile0, "float64", mask_value=-150.0)
    e32 = ref.e32_of(state, tile0, f64, -150.0)
    ref.check_u8(pipe.sr_net.upscale(tile0), f64, e32, _exempt_cap(e32))
