"""GPU: the SwinIR backend of csrc/sr_swinir.hip (shifted-window attention, LayerNorm, linear layers and 3 x 3 convolutions on
fp32 MFMA) against the torch-CPU restatement of its contract (tests/_swinir_ref.py) on seeded SYNTHETIC weights.

PARITY UNPINNED: neither BasicSR, the official repository nor a checkpoint exists offline.  What is checked: the float forward
against the float64 restatement within 8 x the error torch's own float32 forward makes on the same input (tests/test_swinir_host.py
holds the documented order alone inside it and shows that no shift, a dropped mask, a transposed bias table, an unscaled q, the
sample variance, the tanh GELU and zero padding all miss it), the u8 output byte for byte away from rounding boundaries, the
LayerNorm and the window attention on their own (sr_swinir_layernorm_f32, sr_swinir_attention_f32) on padded, offset views in
guarded parents -- the attention's roll, partition, mask and write-back bit for bit through the q = k = 0 probe -- every tail
bit-equal, a NaN-filled workspace, buffer regrowth, strided views, determinism, the ensemble, the network class and the pipeline
with ``sr_weights``.

Worst figures of the float bar on one MI355X are in DESIGN.md ("SwinIR")."""
import asyncio

import numpy as np
import pytest

import _ensemble_ref as E
import _swinir_ref as ref
import _views as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets():
    """One network per description, made once and closed at teardown."""
    import sr_network
    cache = {}

    def get(*key):
        if key not in cache:
            st = ref.synthetic_state(*key)
            cache[key] = sr_network.SwinIRSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"])
        return cache[key]

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


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    net = nets(*case[:7])
    state, img, f64, e32 = ref.case(*case)
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"swinir {ref.case_id(case)}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert got.shape == f64.shape and np.isfinite(got).all()
    assert 0 < e32 < 1e-4
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, _round_u8(got))                     # the float form rounded


def _planar_in(ctx, x, k, fill):
    """Planes (P, h, w) fp32 one below the other inside a guarded parent -> (parent, pointer, plane stride, row stride)."""
    P, h, w = x.shape
    parent, ptr, stride = V.embed(ctx, np.ascontiguousarray(x).view(np.uint8).reshape(P * h, w * 4), *V.pick(V.LAYOUTS_F32, k), fill)
    return parent, ptr, h * stride, stride


def _layernorm(ctx, x, gamma, beta, k, fill):
    import _native
    C, h, w = x.shape
    src, d_x, ps, rs = _planar_in(ctx, x, k, fill)
    dst, d_out, ostride = V.out_view(ctx, C * h, w * 4, *V.pick(V.LAYOUTS_F32, k + 2), fill)
    try:
        _native.swinir_layernorm(ctx, d_x, ps, rs, C, h, w, gamma, beta, d_out, h * ostride, ostride)
        return V.check_guard(ctx, dst, np.float32, (C, h, w), what="swinir layernorm")
    finally:
        src.free(); dst.free()


@pytest.mark.parametrize("C,h,w,k", [(60, 5, 37, 1), (6, 16, 24, 2), (180, 3, 70, 3)])
def test_layernorm_alone(ctx, C, h, w, k):
    """sr_swinir_layernorm_f32 on padded, offset views.  Integer-valued inputs x = m +- a (half of the channels each) with
    gamma 1, beta 0: the mean m and the variance a^2 are exact in float64 in any order, so y = +-a / sqrt(a^2 + 1e-5) to one
    fp32 ulp -- a wrong divisor (C - 1, or the padded plane count) or a plane beyond C entering the sums misses that by
    thousands of ulps.  Then random inputs with random gamma / beta within one ulp of the float64 restatement."""
    rng = np.random.default_rng(200 + k)
    m = rng.integers(-50, 51, (h, w)).astype(np.float64)
    a = rng.integers(1, 9, (h, w)).astype(np.float64)
    sign = np.where(rng.permutation(C) % 2 == 0, 1.0, -1.0)[:, None, None]
    x = (m[None] + sign * a[None]).astype(np.float32)
    want = (sign * a[None] * (1.0 / np.sqrt(a * a + 1e-5))[None]).astype(np.float32)
    ones, zeros = np.ones(C, np.float32), np.zeros(C, np.float32)
    assert np.array_equal(want, ref.np_layernorm(x, ones, zeros))
    xr = (rng.standard_normal((C, h, w)) * 3 + rng.standard_normal((1, h, w))).astype(np.float32)
    g, b = rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)
    want_r = ref.np_layernorm(xr, g, b)
    for fill in V.FILLS:
        got = _layernorm(ctx, x, ones, zeros, k, fill)
        u = _ulps(got, want)
        print(f"swinir layernorm C{C} {h}x{w}: exact case worst {int(u.max())} ulp")
        assert u.max() <= 1
        ur = _ulps(_layernorm(ctx, xr, g, b, k + 1, fill), want_r)
        print(f"  random case worst {int(ur.max())} ulp")
        assert ur.max() <= 1


def _attention(ctx, qkv, table, heads, shift, k, fill):
    import _native
    C3, hp, wp = qkv.shape
    C = C3 // 3
    src, d_x, ps, rs = _planar_in(ctx, qkv, k, fill)
    dst, d_out, ostride = V.out_view(ctx, C * hp, wp * 4, *V.pick(V.LAYOUTS_F32, k + 3), fill)
    try:
        _native.swinir_attention(ctx, d_x, ps, rs, C, heads, hp, wp, shift, table, d_out, hp * ostride, ostride)
        return V.check_guard(ctx, dst, np.float32, (C, hp, wp), what="swinir attention")
    finally:
        src.free(); dst.free()


@pytest.mark.parametrize("hp,wp", [(8, 8), (16, 24), (24, 16)])
@pytest.mark.parametrize("d", [10, 30, 32])
def test_attention_mean_probe_is_bit_exact(ctx, hp, wp, d):
    """q = k = 0, a zero bias table, positive integer-valued v: every score is 0 (or -100 across regions), so the output is the
    mean of v over the tokens of the same window and region -- 16, 32 or 64 of them -- exactly, in any summation order (a
    masked term weighs exp(-100) / 16 and vanishes against a sum of at least 1 / 16).  Zero tolerance on the roll, the window
    partition, the mask and the write-back, at shift 0 and 4."""
    heads = 2
    C = heads * d
    rng = np.random.default_rng(hp * 100 + wp + d)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = rng.integers(1, 1000, (C, hp, wp)).astype(np.float32)
    table = np.zeros((225, heads), np.float32)
    for shift in (0, 4):
        want = ref.np_attention(qkv, table, heads, shift, np.float64)
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64) * 64, np.round(want * 64))      # multiples of 1 / 64: exact in fp32
        got = _attention(ctx, qkv, table, heads, shift, d + shift, V.FILLS[shift // 4])
        bad = np.argwhere(_bits(got) != _bits(want32))
        assert not len(bad), (shift, len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


def _attention_bar(ctx, qkv, table, heads, shift, k, what):
    want64 = ref.np_attention(qkv, table, heads, shift, np.float64)
    e32 = float(np.max(np.abs(ref.np_attention(qkv, table, heads, shift).astype(np.float64) - want64)))
    got = _attention(ctx, qkv, table, heads, shift, k, V.FILLS[k % 2])
    err = float(np.max(np.abs(got.astype(np.float64) - want64)))
    print(f"swinir attention {what} shift {shift}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert e32 > 0 and err <= 8 * e32, (err, e32)


@pytest.mark.parametrize("shift", [0, 4])
def test_attention_bias_table_probe(ctx, shift):
    """q = k = 0, a random bias table (every head its own), v one-hot over the tokens: o_i[dd] = the sum of p[i][j] over the
    keys j = dd mod d, so a transposed table, a wrong relative-position index or a swapped head axis moves the result by
    orders of magnitude more than the bar: 8 x the error of the fp32 restatement against the float64 one."""
    heads, d, hp, wp = 3, 10, 16, 24
    C = heads * d
    rng = np.random.default_rng(31 + shift)
    table = rng.standard_normal((225, heads)).astype(np.float32)
    onehot = (np.arange(64)[None, :] % d == np.arange(d)[:, None]).astype(np.float32)             # (dd, token)
    v = ref._unwindows(np.broadcast_to(np.tile(onehot, (heads, 1))[:, None, :], (C, hp * wp // 64, 64)).copy(), hp, wp)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = np.roll(v, (shift, shift), (1, 2)) if shift else v
    _attention_bar(ctx, qkv, table, heads, shift, 1 + shift, "bias probe")
    wrong = ref.np_attention(qkv, table[:, ::-1], heads, shift, np.float64)                       # the probe sees the head axis
    assert np.abs(wrong - ref.np_attention(qkv, table, heads, shift, np.float64)).max() > 1e-2


@pytest.mark.parametrize("heads,d,hp,wp,shift", [(6, 30, 16, 24, 4), (2, 32, 8, 8, 4), (4, 16, 24, 16, 0), (3, 4, 16, 8, 4)])
def test_attention_random(ctx, heads, d, hp, wp, shift):
    C = heads * d
    rng = np.random.default_rng(heads * 10 + d)
    qkv = rng.standard_normal((3 * C, hp, wp)).astype(np.float32)
    qkv[:C] *= np.float32(d ** -0.5)
    table = (rng.standard_normal((225, heads)) * 0.5).astype(np.float32)
    _attention_bar(ctx, qkv, table, heads, shift, heads + d, f"random {heads}x{d} {hp}x{wp}")


def test_inspection_refusals():
    import _native
    one = np.ones(4, np.float32)
    with pytest.raises(NotImplementedError):
        _native.swinir_layernorm(None, 256, 64, 16, 300, 4, 4, np.ones(300), np.ones(300), 256, 64, 16)
    with pytest.raises(ValueError):
        _native.swinir_layernorm(None, 256, 64, 12, 4, 4, 4, one, one, 256, 64, 16)              # a row stride below a row
    with pytest.raises(ValueError):
        _native.swinir_attention(None, 256, 4 * 64 * 8, 32, 4, 1, 8, 12, 0, np.zeros((225, 1)), 256, 4 * 64 * 8, 48)   # 12 columns
    with pytest.raises(NotImplementedError):
        _native.swinir_attention(None, 256, 4 * 64 * 8, 32, 4, 1, 8, 8, 2, np.zeros((225, 1)), 256, 4 * 64 * 8, 32)    # shift 2
    with pytest.raises(NotImplementedError):
        _native.swinir_attention(None, 256, 4 * 64 * 8, 32, 66, 2, 8, 8, 0, np.zeros((225, 2)), 256, 4 * 64 * 8, 32)   # d = 33


TAIL_NETS = [((60, 6, 120, 1, 2, 2, "pixelshuffledirect"), 21, 37), ((64, 2, 128, 1, 1, 4, "pixelshuffle"), 13, 19),
             ((64, 2, 128, 1, 1, 3, "pixelshuffle"), 20, 11), ((64, 4, 128, 1, 2, 4, "nearest+conv"), 12, 21)]


@pytest.mark.parametrize("key,h,w", TAIL_NETS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_tail_is_bit_equal(ctx, nets, key, h, w):
    """fp32 bits and u8 bytes of every tail equal those of one tail piece; the plan is the restatement's."""
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
    """Two runs give equal bits; the first forward after the workspace was filled with NaN bytes (0xFF) equals them -- no
    padded plane and nothing an earlier image left is read before it is written; a larger image after a smaller one (the
    buffers are regrown) and the small one again."""
    import sr_network
    key = (60, 6, 120, 1, 2, 2, "pixelshuffle")                   # C and hidden are not multiples of 64: padded planes exist
    st = ref.synthetic_state(*key)
    small, large = ref.make_image(13, 21), ref.make_image(45, 70)
    net = sr_network.SwinIRSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"])
    other = sr_network.SwinIRSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"])
    try:
        net.model(ctx).fill_workspace(13, 21, 0xFF)
        a = _f32(ctx, net, small)
        assert np.isfinite(a).all()
        b = _f32(ctx, net, small)
        assert np.array_equal(_bits(a), _bits(b))
        big = _f32(ctx, net, large)
        net.model(ctx).fill_workspace(45, 70, 0xFF)
        assert np.array_equal(_bits(_f32(ctx, net, large)), _bits(big))
        assert np.array_equal(_bits(_f32(ctx, net, small)), _bits(a))
        assert np.array_equal(_bits(_f32(ctx, other, small)), _bits(a)) and np.array_equal(_bits(_f32(ctx, other, large)), _bits(big))
        assert np.array_equal(net.upscale(small), _round_u8(a))
    finally:
        net.close(); other.close()


@pytest.mark.parametrize("case,k", [(ref.CASES[0], 1), (ref.CASES[1], 2), (ref.CASES[4], 3)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
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
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="swinir u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="swinir f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_refusals(ctx, nets):
    """Bad arguments raise before any launch (the guarded output stays untouched); the cap is refused by message from a plan
    alone; a destroyed handle is refused, not dereferenced."""
    import ctypes as C

    import _native
    net = nets(*ref.CASES[0][:7])
    img = ref.make_image(13, 21)
    h, w = 13, 21
    with pytest.raises(ValueError, match="no tile"):
        net.upscale(img, tile=16)
    with pytest.raises(ValueError):
        net.upscale(img[:, :, :1])
    m = net.model(ctx)
    with pytest.raises(ValueError, match="SR_SWINIR_TRUNK_CAP"):
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
        gone = _native.SwinirModel(ctx, net.desc, net._w, net._b)
        handle = C.c_void_p(gone.handle.value)
        gone.close()
        for fn in (ctx.lib.sr_swinir_u8, ctx.lib.sr_swinir_f32):
            assert fn(handle, C.c_void_p(d_src.ptr), w * 3, h, w, C.c_void_p(d_dst), dstride, 0) == _native.SR_ERR_INVALID_ARG
        assert "destroyed" in _native.last_error()
        assert ctx.lib.sr_swinir_destroy(handle) == _native.SR_OK                   # a second destroy is a no-op
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(ValueError):                                                 # a table of the wrong shape
        _native.SwinirModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)
    with pytest.raises(ValueError):
        _native.SwinirModel(ctx, net.desc, net._w[:-1], net._b[:-1])


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
    """SwinIR+: members from the family's own forward_f32 on host-transformed inputs (each reflected and windowed on its own),
    summed in ascending order and divided as tests/_ensemble_ref.py states; masks 0x03 and 0xFF, fp32 bits and u8 bytes."""
    net = nets(60, 6, 120, 1, 2, 2, "pixelshuffledirect")
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
    net = nets(*ref.CASES[0][:7])
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
    st = ref.synthetic_state(*ref.CASES[0][:7])
    tmp = sr_network.SwinIRSRNet(st)
    tmp.model(ctx)
    tmp.close()
    assert tmp._models == {}


def test_pipeline_with_sr_weights(tmp_path):
    """process() with sr_weights pointing at a saved SwinIR: the family is picked from the file, the run stays
    device-resident, and tile 0 -- reflected, padded and windowed on its own, as every tile is -- matches the restatement."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(60, 6, 120, 1, 2, 2, "pixelshuffle")
    wpath = str(tmp_path / "swinir.npz")
    np.savez(wpath, **state)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, block_size=64, sr_scale=2, num_pyramid_levels=4))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.SwinIRSRNet) and pipe._builtin_backend()
    assert pipe.sr_net.desc.range == np.float32(ref.IMG_RANGE)                      # the .npz extras
    res = asyncio.run(pipe.process(src, str(tmp_path / "out.png")))
    assert res.success, res.error_message
    assert res.total_blocks == res.successful_blocks > 1 and res.failed_blocks == 0
    assert "sr_net" in pipe.stage_times and "sr_stub" not in pipe.stage_times
    assert pipe.transfers["h2d_bytes"] == img.nbytes                                # the network keeps the run device-resident
    assert np.asarray(Image.open(str(tmp_path / "out.png"))).shape == (160, 192, 3)
    tile0 = pipe.tiling_module.split_image(src)[0].data
    f64 = ref.forward(state, tile0, "float64")
    e32 = float(np.max(np.abs(ref.forward(state, tile0, "float32").astype(np.float64) - f64)))
    ref.check_u8(pipe.sr_net.upscale(tile0), f64, e32)
