"""GPU: the HAT backend of csrc/sr_hat.hip (16 x 16 window attention, overlapping cross-attention, the channel-attention
convolution branch, on SwinIR's trunk kernels) against the torch-CPU restatement of its contract (tests/_hat_ref.py) on seeded
SYNTHETIC weights.

PARITY UNPINNED: neither the HAT package nor a checkpoint exists offline.  What is checked: the float forward against the
float64 restatement within 8 x the error torch's own float32 forward makes on the same input (tests/test_hat_host.py shows that
symmetric padding, masked OCA padding, the CAB on x, the mean over the unpadded image, conv_scale 1 and shift 4 all miss it);
the u8 output byte for byte away from rounding boundaries; the two attention kernels on their own (sr_hat_attention_f32,
sr_hat_oca_f32) on padded, offset views in guarded parents -- the roll, partition, mask, zero keys and write-back bit for bit
through the q = k = 0 probes -- every tail bit-equal, a 0xFF-filled workspace, buffer regrowth, strided views, determinism, the
ensemble, the network class and the pipeline with ``sr_weights``.

Worst figures of the float bar on one MI355X are in DESIGN.md ("HAT")."""
import asyncio

import numpy as np
import pytest

import _ensemble_ref as E
import _hat_ref as ref
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
            cache[key] = sr_network.HATSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"], conv_scale=float(st["conv_scale"]))
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


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    net = nets(*case[:8])
    state, img, f64, e32 = ref.case(*case)
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"hat {ref.case_id(case)}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
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


def _attention(ctx, qkv, table, heads, shift, k, fill, index=None, oca=False):
    import _native
    C3, hp, wp = qkv.shape
    C = C3 // 3
    src, d_x, ps, rs = _planar_in(ctx, qkv, k, fill)
    dst, d_out, ostride = V.out_view(ctx, C * hp, wp * 4, *V.pick(V.LAYOUTS_F32, k + 3), fill)
    try:
        if oca:
            _native.hat_oca(ctx, d_x, ps, rs, C, heads, hp, wp, table, index, d_out, hp * ostride, ostride)
        else:
            _native.hat_attention(ctx, d_x, ps, rs, C, heads, hp, wp, shift, table, d_out, hp * ostride, ostride)
        return V.check_guard(ctx, dst, np.float32, (C, hp, wp), what="hat oca" if oca else "hat attention")
    finally:
        src.free(); dst.free()


@pytest.mark.parametrize("hp,wp", [(16, 16), (32, 48), (48, 32)])
@pytest.mark.parametrize("d", [10, 30, 32])
def test_attention_mean_probe_is_bit_exact(ctx, hp, wp, d):
    """q = k = 0, a zero bias table, positive integer-valued v: every score is 0 (or -100 across regions), so the output is the
    mean of v over the tokens of the same window and region -- 64, 128 or 256 of them -- exactly, in any summation order (a
    masked term weighs expf(-100) / 64, which is below half the smallest fp32 subnormal).  Zero tolerance on the roll, the
    window partition, the mask and the write-back, at shift 0 and 8; 16 x 16 with shift 8 is the one window in which all nine
    regions meet."""
    heads = 2
    C = heads * d
    rng = np.random.default_rng(hp * 100 + wp + d)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = rng.integers(1, 1000, (C, hp, wp)).astype(np.float32)
    table = np.zeros((ref.REL_ROWS, heads), np.float32)
    for shift in (0, 8):
        want = ref.np_window_attention(qkv, table, heads, shift, np.float64)
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64) * 256, np.round(want * 256))    # multiples of 1 / 256: exact in fp32
        got = _attention(ctx, qkv, table, heads, shift, d + shift, V.FILLS[shift // 8])
        bad = np.argwhere(_bits(got) != _bits(want32))
        assert not len(bad), (shift, len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


def _bar(ctx, qkv, table, heads, shift, k, what, index=None, oca=False):
    if oca:
        want64 = ref.np_oca(qkv, table, index, heads, np.float64)
        e32 = float(np.max(np.abs(ref.np_oca(qkv, table, index, heads).astype(np.float64) - want64)))
    else:
        want64 = ref.np_window_attention(qkv, table, heads, shift, np.float64)
        e32 = float(np.max(np.abs(ref.np_window_attention(qkv, table, heads, shift).astype(np.float64) - want64)))
    got = _attention(ctx, qkv, table, heads, shift, k, V.FILLS[k % 2], index, oca)
    err = float(np.max(np.abs(got.astype(np.float64) - want64)))
    print(f"hat {'oca' if oca else 'attention'} {what} shift {shift}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert e32 > 0 and err <= 8 * e32, (err, e32)
    return want64


@pytest.mark.parametrize("shift", [0, 8])
def test_attention_bias_table_probe(ctx, shift):
    """q = k = 0, a random bias table (every head its own), v one-hot over the tokens: o_i[dd] = the sum of p[i][j] over the
    keys j = dd mod d, so a transposed table, a wrong relative-position index or a swapped head axis moves the result by
    orders of magnitude more than the bar: 8 x the error of the fp32 restatement against the float64 one."""
    heads, d, hp, wp = 3, 10, 16, 32
    C = heads * d
    rng = np.random.default_rng(31 + shift)
    table = rng.standard_normal((ref.REL_ROWS, heads)).astype(np.float32)
    onehot = (np.arange(ref.TOK)[None, :] % d == np.arange(d)[:, None]).astype(np.float32)          # (dd, token)
    v = ref._unwindows(np.broadcast_to(np.tile(onehot, (heads, 1))[:, None, :], (C, hp * wp // ref.TOK, ref.TOK)).copy(), hp, wp)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = np.roll(v, (shift, shift), (1, 2)) if shift else v
    want = _bar(ctx, qkv, table, heads, shift, 1 + shift, "bias probe")
    wrong = ref.np_window_attention(qkv, table[:, ::-1], heads, shift, np.float64)                   # the probe sees the head axis
    assert np.abs(wrong - want).max() > 1e-2


@pytest.mark.parametrize("hp,wp", [(16, 16), (32, 48), (48, 48)])
@pytest.mark.parametrize("d", [10, 30, 32])
def test_oca_mean_probe_is_bit_exact(ctx, hp, wp, d):
    """q = k = 0, a zero bias table, v = 576 m with integers m in 1 .. 8: every one of the 576 scores is 0 -- those of the keys
    outside the image too, which are NOT masked -- so p = fl(1 / 576) = (1 + 2^-27) / 576 for every key and every partial sum
    of the fmaf chain is an integer plus less than 2^-23 of itself: each rounds to the integer, and the output is
    (sum of the in-image v of the enlarged window) / 576 exactly.  A kernel that masks the padding, or divides by the in-image
    count, fails this: in 16 x 16 every window touches all four borders (256 of 576 keys inside), 48 x 48 has one interior
    window."""
    heads = 2
    C = heads * d
    rng = np.random.default_rng(hp * 100 + wp + d)
    m = rng.integers(1, 9, (C, hp, wp))
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = (576 * m).astype(np.float32)
    table = np.zeros((ref.OCA_ROWS, heads), np.float32)
    sums = ref._ext_windows(m).sum(-1)                                                              # (C, windows): exact integers
    want32 = ref._unwindows(np.broadcast_to(sums[:, :, None], sums.shape + (ref.TOK,)).copy(), hp, wp).astype(np.float32)
    want64 = ref.np_oca(qkv, table, None, heads, np.float64)
    assert np.abs(want64 - want32).max() < 1e-9
    masked = ref.np_oca(qkv, table, None, heads, np.float64, masked=True)                           # what the probe must tell apart
    assert np.abs(masked - want64).max() > 1.0
    got = _attention(ctx, qkv, table, heads, 0, d, V.FILLS[d % 2], None, oca=True)
    bad = np.argwhere(_bits(got) != _bits(want32))
    assert not len(bad), (len(bad), bad[:4], got[tuple(bad[0])], want32[tuple(bad[0])])


def test_oca_index_probe(ctx):
    """q = k = 0, a random bias table, a caller-supplied index with negative (wrapped) values, v one-hot over positions: the
    result follows the caller's index, not the default formula, and a negative entry reads row + 1521."""
    heads, d, hp, wp = 3, 10, 32, 32
    C = heads * d
    rng = np.random.default_rng(77)
    table = rng.standard_normal((ref.OCA_ROWS, heads)).astype(np.float32)
    index = rng.integers(-ref.OCA_ROWS, ref.OCA_ROWS, (ref.TOK, ref.KEYS))
    assert (index < 0).any() and (index >= 0).any()
    yy, xx = np.mgrid[0:hp, 0:wp]
    onehot = ((yy * 7 + xx) % d == np.arange(d)[:, None, None]).astype(np.float32)                  # (dd, hp, wp)
    qkv = np.zeros((3 * C, hp, wp), np.float32)
    qkv[2 * C:] = np.tile(onehot, (heads, 1, 1))
    want = _bar(ctx, qkv, table, heads, 0, 2, "index probe", index, oca=True)
    assert np.abs(ref.np_oca(qkv, table, None, heads, np.float64) - want).max() > 1e-2             # the default formula is far
    assert np.abs(ref.np_oca(qkv, table, np.where(index < 0, -index - 1, index), heads, np.float64) - want).max() > 1e-2   # so is a dropped sign
    _bar(ctx, qkv, table, heads, 0, 3, "default index", None, oca=True)
    _bar(ctx, qkv, table, heads, 0, 4, "raw default index", ref.oca_index_raw(), oca=True)


@pytest.mark.parametrize("heads,d,hp,wp,shift", [(6, 30, 16, 32, 8), (2, 32, 16, 16, 8), (2, 16, 48, 16, 0), (3, 4, 32, 32, 8)])
def test_attention_random(ctx, heads, d, hp, wp, shift):
    C = heads * d
    rng = np.random.default_rng(heads * 10 + d)
    qkv = rng.standard_normal((3 * C, hp, wp)).astype(np.float32)
    qkv[:C] *= np.float32(d ** -0.5)
    table = (rng.standard_normal((ref.REL_ROWS, heads)) * 0.5).astype(np.float32)
    _bar(ctx, qkv, table, heads, shift, heads + d, f"random {heads}x{d} {hp}x{wp}")


@pytest.mark.parametrize("heads,d,hp,wp", [(6, 30, 16, 32), (2, 32, 16, 16), (2, 16, 48, 48), (3, 4, 32, 16)])
def test_oca_random(ctx, heads, d, hp, wp):
    C = heads * d
    rng = np.random.default_rng(heads * 10 + d + 1)
    qkv = rng.standard_normal((3 * C, hp, wp)).astype(np.float32)
    qkv[:C] *= np.float32(d ** -0.5)
    table = (rng.standard_normal((ref.OCA_ROWS, heads)) * 0.5).astype(np.float32)
    _bar(ctx, qkv, table, heads, 0, heads + d, f"random {heads}x{d} {hp}x{wp}", None, oca=True)


def test_file_index_reaches_the_forward(ctx):
    """A state that carries relative_position_index_OCA (raw, with its negative values) gives the bits of the default formula;
    a different index in the file gives different values: the file's index is the one used."""
    import sr_network
    key = (60, 6, 120, 20, 2, 1, 1, 2)
    img = ref.make_image(19, 21, seed=3)
    outs = []
    for variant in ("none", "raw", "other"):
        st = ref.synthetic_state(*key, file_index=variant != "none")
        if variant == "other":
            st[ref.OCA_KEY] = -st[ref.OCA_KEY][::-1] - 1
        net = sr_network.HATSRNet(st, img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"], conv_scale=float(st["conv_scale"]))
        try:
            outs.append(_f32(ctx, net, img))
            if variant == "other":
                f64 = ref.forward(st, img, "float64")
                e32 = float(np.max(np.abs(ref.forward(st, img, "float32").astype(np.float64) - f64)))
                err = float(np.max(np.abs(outs[-1].astype(np.float64) - f64)))
                print(f"hat file index: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
                assert err <= 8 * e32
        finally:
            net.close()
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert not np.array_equal(outs[0], outs[2])


TAIL_NETS = [((60, 6, 120, 20, 2, 1, 2, 2), 21, 37), ((64, 2, 128, 16, 4, 1, 1, 4), 13, 19), ((64, 2, 128, 16, 4, 1, 1, 3), 20, 11)]


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
        assert m.plan(h, w, tail) == ref.plan(key[0], key[2], key[3], key[7], h, w, tail)
        assert np.array_equal(_bits(_f32(ctx, net, img, tail)), _bits(one_f)), tail
        assert np.array_equal(net.upscale(img, tail=tail), one_u), tail


def test_deterministic_ff_workspace_and_regrowth(ctx):
    """Two runs give equal bits; the first forward after the workspace was filled with 0xFF bytes (NaN) equals them -- no padded
    plane and nothing an earlier image left is read before it is written; a larger image after a smaller one (the buffers are
    regrown) and the small one again."""
    import sr_network
    key = (60, 6, 120, 20, 2, 1, 2, 2)                            # C, n_mid and hidden are not multiples of 64: padded planes exist
    st = ref.synthetic_state(*key)
    kw = dict(img_range=float(st["img_range"]), rgb_mean=st["rgb_mean"], conv_scale=float(st["conv_scale"]))
    small, large = ref.make_image(13, 21), ref.make_image(45, 70)
    net, other = sr_network.HATSRNet(st, **kw), sr_network.HATSRNet(st, **kw)
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


@pytest.mark.parametrize("case,k", [(ref.CASES[0], 1), (ref.CASES[4], 2), (ref.EDGE_CASES[0], 3)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
def test_views(ctx, nets, case, k):
    """Padded, offset source view; destinations inside guarded parents; u8 (small tail) and fp32 entry points: equal bits and no
    byte written outside the view."""
    h, w, s = case[8], case[9], case[7]
    net, img = nets(*case[:8]), ref.case(*case)[1]
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 5)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="hat u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="hat f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_refusals(ctx, nets):
    """Bad arguments raise before any launch (the guarded output stays untouched); the cap is refused by message from a plan
    alone; a destroyed handle is refused, not dereferenced."""
    import ctypes as C

    import _native
    net = nets(*ref.CASES[0][:8])
    img = ref.make_image(13, 21)
    h, w = 13, 21
    with pytest.raises(ValueError, match="no tile"):
        net.upscale(img, tile=16)
    with pytest.raises(ValueError):
        net.upscale(img[:, :, :1])
    m = net.model(ctx)
    with pytest.raises(ValueError, match="SR_HAT_TRUNK_CAP"):
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
        with pytest.raises(ValueError):
            m.ensemble_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, 0, mask=0)
        gone = _native.HatModel(ctx, net.desc, net._w, net._b)
        handle = C.c_void_p(gone.handle.value)
        gone.close()
        for fn in (ctx.lib.sr_hat_u8, ctx.lib.sr_hat_f32):
            assert fn(handle, C.c_void_p(d_src.ptr), w * 3, h, w, C.c_void_p(d_dst), dstride, 0) == _native.SR_ERR_INVALID_ARG
        assert "destroyed" in _native.last_error()
        assert ctx.lib.sr_hat_destroy(handle) == _native.SR_OK                      # a second destroy is a no-op
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(ValueError):                                                 # a table of the wrong shape
        _native.HatModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)
    with pytest.raises(ValueError):
        _native.HatModel(ctx, net.desc, net._w[:-1], net._b[:-1])
    with pytest.raises(ValueError):                                                 # an index value outside the table
        _native.HatModel(ctx, net.desc, net._w, net._b, np.full((256, 576), 1521))


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
    """HAT+: members from the family's own forward_f32 on host-transformed inputs (each reflected, windowed and pooled on its
    own), summed in ascending order and divided as tests/_ensemble_ref.py states; masks 0x03 and 0xFF, fp32 bits and u8 bytes."""
    net = nets(60, 6, 120, 20, 2, 1, 2, 2)
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
    net = nets(*ref.CASES[0][:8])
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
    st = ref.synthetic_state(*ref.CASES[0][:8])
    tmp = sr_network.HATSRNet(st)
    tmp.model(ctx)
    tmp.close()
    assert tmp._models == {}


def test_pipeline_with_sr_weights(tmp_path):
    """process() with sr_weights pointing at a saved HAT: the family is picked from the file (before SwinIR's key), the run stays
    device-resident, and tile 0 -- reflected, padded, windowed and pooled on its own, as every tile is -- matches the
    restatement."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(60, 6, 120, 20, 2, 1, 2, 2)
    wpath = str(tmp_path / "hat.npz")
    np.savez(wpath, **state)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, block_size=64, sr_scale=2, num_pyramid_levels=4))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.HATSRNet) and pipe._builtin_backend()
    assert pipe.sr_net.desc.range == np.float32(ref.IMG_RANGE) and pipe.sr_net.desc.conv_scale == np.float32(ref.CONV_SCALE)
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
