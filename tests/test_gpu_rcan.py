"""GPU: the RCAN backend of csrc/sr_rcan.hip (residual channel attention on fp32 MFMA, the attention in float64) against the
torch-CPU restatement of its contract (tests/_rcan_ref.py) on seeded SYNTHETIC weights.

PARITY UNPINNED: the BasicSR package and its checkpoints do not exist offline.  What is checked: the float forward against the
float64 restatement within 8 x the error torch's own float32 forward makes on the same input (tests/test_rcan_host.py holds
the documented order alone inside it, and shows that a mean over padded blocks, a wrong divisor, a shifted s or a dropped
res_scale misses it by three orders of magnitude), the u8 output byte for byte away from rounding boundaries, the mean and the
attention on their own (sr_rcan_attention_f32), every tail bit-equal, strided views, determinism, the ensemble, the network
class and the pipeline with ``sr_weights``.

The exact-arithmetic networks and one-hot probes of _rcan_ref -- every partial sum representable in fp32 and s = 0.5 exactly,
proved on the CPU in tests/test_rcan_host.py -- must be reproduced bit for bit whatever the summation order: the zero-tolerance
check of the buffer rotation, the in-place skips, the scale-and-skip pass, the shuffle and the padding at the true border."""
import asyncio
import ctypes as C
import math

import numpy as np
import pytest

import _ensemble_ref as E
import _rcan_ref as ref
import _views as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets():
    """One network per (F, R, G, B, s), made once and closed at teardown."""
    import sr_network
    cache = {}

    def get(F, R, G, B, s):
        key = (F, R, G, B, s)
        if key not in cache:
            st = ref.synthetic_state(F, R, G, B, s)
            cache[key] = sr_network.RCANSRNet(st, res_scale=float(st["res_scale"]))
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
    return x.view(np.uint32)


def _round_u8(f):
    return np.rint(np.clip(f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts
    ("RCAN")."""
    net = nets(*case[:5])
    state, img, f64, e32 = ref.case(*case)
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"rcan {ref.case_id(case)}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert 0 < e32 < 1e-4
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, _round_u8(got))                     # the float form rounded


@pytest.mark.parametrize("F,R,h,w,k", [(64, 4, 11, 37, 1), (64, 1, 40, 70, 2), (128, 8, 40, 70, 3), (5, 5, 33, 300, 4)])
def test_attention_alone(ctx, F, R, h, w, k):
    """sr_rcan_attention_f32 on planes of integer-valued floats inside a padded, offset parent: every partial sum is exact in
    float64, so the mean is np.float32(fsum / (h w)) bit for bit whatever the order -- unless a padded column, a guard byte or a
    wrong divisor entered it -- and s is within one fp32 ulp of the float64 restatement (the float64 exp's own error is far
    below half an fp32 ulp)."""
    import _native
    rng = np.random.default_rng(100 + k)
    x = rng.integers(-3000, 3001, (F, h, w)).astype(np.float32)
    x += (np.arange(F, dtype=np.float32) * 7 - 100)[:, None, None]            # every channel its own mean
    w1 = (rng.standard_normal((R, F)) * 0.002 / np.sqrt(F)).astype(np.float32)
    b1 = rng.uniform(0.5, 1.5, R).astype(np.float32)
    w2 = (rng.standard_normal((F, R)) * 0.25 / np.sqrt(R)).astype(np.float32)
    b2 = rng.uniform(-1.0, 1.0, F).astype(np.float32)
    want_m, want_s, _ = ref.attention(x, w1, b1, w2, b2)
    assert all(want_m[c] == np.float32(math.fsum(x[c].astype(np.float64).ravel().tolist()) / (h * w)) for c in range(F))
    base_off, pad = V.pick(V.LAYOUTS_F32, k)
    rows = x.reshape(F * h, w)                                     # planes one below the other: plane stride = h row strides
    for fill in V.FILLS:
        parent, d_x, stride = V.embed(ctx, rows.view(np.uint8).reshape(F * h, w * 4), base_off, pad, fill)
        try:
            m, s = _native.rcan_attention(ctx, d_x, h * stride, stride, F, R, h, w, w1, b1, w2, b2)
        finally:
            parent.free()
        assert np.array_equal(_bits(m), _bits(want_m)), np.argwhere(_bits(m) != _bits(want_m))[:4]
        ulps = np.abs(_bits(s).astype(np.int64) - _bits(want_s).astype(np.int64))
        print(f"rcan attention F{F} R{R} {h}x{w}: s {s.min():.3f} .. {s.max():.3f}, worst {int(ulps.max())} ulp")
        assert ulps.max() <= 1
        assert s.min() < 0.45 and s.max() > 0.55


@pytest.mark.parametrize("F,R,G,B,s,h,w", [(64, 4, 2, 2, 4, 21, 37), (64, 4, 1, 1, 3, 20, 30), (64, 4, 2, 0, 2, 5, 6), (128, 4, 1, 1, 1, 12, 35)])
def test_every_tail_is_bit_equal(ctx, nets, F, R, G, B, s, h, w):
    """fp32 bits and u8 bytes of every tail equal those of one tail piece; the piece count is the plan's."""
    img = ref.make_image(h, w, seed=11)
    net = nets(F, R, G, B, s)
    m = net.model(ctx)
    assert m.plan(h, w, 64)[:2] == (ref.plan(F, s, h, w)[0], 1)
    one_f, one_u = _f32(ctx, net, img, 64), net.upscale(img, tail=64)
    assert np.isfinite(one_f).all() and one_u.std() > 5
    assert np.array_equal(one_u, _round_u8(one_f))
    for tail in (1, 5, 16, 0):
        assert m.plan(h, w, tail) == ref.plan(F, s, h, w, tail)
        assert m.plan(h, w, tail)[1] == -(-h // (tail or 256)) * -(-w // (tail or 256))
        assert np.array_equal(_bits(_f32(ctx, net, img, tail)), _bits(one_f)), tail
        assert np.array_equal(net.upscale(img, tail=tail), one_u), tail


@pytest.mark.parametrize("case,k", [(ref.CASES[1], 1), (ref.CASES[2], 2), (ref.CASES[5], 3)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
def test_views(ctx, nets, case, k):
    """Padded, offset source view; destinations inside guarded parents; u8 (small tail) and fp32 entry points: equal bits and no
    byte written outside the view."""
    h, w, s = case[5], case[6], case[4]
    net, img = nets(*case[:5]), ref.case(*case)[1]
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 5)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="rcan u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="rcan f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_model_reuse_across_shapes(ctx, nets):
    """One model, small image, larger image (the buffers are regrown), the small image again: first and last are bit-equal and
    every result equals another model's -- nothing of an earlier image's planes or chunk sums enters a mean."""
    import sr_network
    small, large = ref.make_image(12, 20), ref.make_image(70, 45)
    other = nets(64, 4, 2, 2, 2)
    st = ref.synthetic_state(64, 4, 2, 2, 2)
    net = sr_network.RCANSRNet(st, res_scale=float(st["res_scale"]))
    try:
        a, b, c = _f32(ctx, net, small), _f32(ctx, net, large), _f32(ctx, net, small)
        assert np.array_equal(_bits(a), _bits(c))
        assert np.array_equal(_bits(a), _bits(_f32(ctx, other, small))) and np.array_equal(_bits(b), _bits(_f32(ctx, other, large)))
        assert np.array_equal(net.upscale(small), _round_u8(a))
    finally:
        net.close()


def test_deterministic_and_refusals(ctx, nets):
    """Equal inputs give equal bits over two calls; bad arguments raise before any launch (the guarded output stays untouched);
    a destroyed handle is refused, not dereferenced."""
    import _native
    net = nets(64, 4, 2, 2, 2)
    img = ref.make_image(19, 37)
    a, b = _f32(ctx, net, img), _f32(ctx, net, img)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(net.upscale(img), net.upscale(img))
    for bad in (img[:, :, 0], np.dstack([img, img[:, :, :1]]), img[:, :, :1]):
        with pytest.raises(ValueError):
            net.upscale(bad)
    with pytest.raises(ValueError):
        net.upscale(img.astype(np.float32))
    with pytest.raises(ValueError, match="no tile"):
        net.upscale(img, tile=16)
    m = net.model(ctx)
    h, w = 19, 37
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
            m.upscale_u8(d_src.ptr, w * 3, h, w, 0, dstride, 0)
        gone = _native.RcanModel(ctx, net.desc, net._w, net._b)                     # a destroyed handle: refused by the live-model set
        handle = C.c_void_p(gone.handle.value)
        gone.close()
        for fn in (ctx.lib.sr_rcan_u8, ctx.lib.sr_rcan_f32):
            assert fn(handle, C.c_void_p(d_src.ptr), w * 3, h, w, C.c_void_p(d_dst), dstride, 0) == _native.SR_ERR_INVALID_ARG
        assert "destroyed" in _native.last_error()
        assert ctx.lib.sr_rcan_destroy(handle) == _native.SR_OK                     # a second destroy is a no-op
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(ValueError):                                                 # a table of the wrong shape
        _native.RcanModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)
    with pytest.raises(ValueError):
        _native.RcanModel(ctx, net.desc, net._w[:3] + [net._w[3].T] + net._w[4:], net._b)


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
    """RCAN+: members from the family's own forward_f32 on host-transformed inputs (each pools over its own planes), summed in
    ascending order and divided as tests/_ensemble_ref.py states; masks 0x03 and 0xFF, fp32 bits and u8 bytes, any tail."""
    net = nets(64, 4, 1, 1, 2)
    img = ref.make_image(23, 37, seed=11)
    ys = [E.d4_inv(_run(ctx, net, E.d4(img, k)), k) for k in range(8)]
    assert not np.array_equal(ys[0], ys[1]) and not np.array_equal(ys[0], ys[4])     # the network is not equivariant
    for mask in (0x03, 0xFF):
        want = E.mean_f32([ys[k] for k in E.members(mask)])
        assert np.array_equal(_bits(_run(ctx, net, img, ens=mask)), _bits(want)), hex(mask)
        assert np.array_equal(_bits(_run(ctx, net, img, ens=mask, tail=5)), _bits(want)), hex(mask)
        assert np.array_equal(_run(ctx, net, img, ens=mask, u8=True), E.to_u8(want)), hex(mask)
    assert np.array_equal(_bits(_run(ctx, net, img, ens=1)), _bits(ys[0]))            # mask 1 is the plain forward
    assert np.array_equal(net.upscale(img, ensemble=8), E.to_u8(E.mean_f32(ys)))
    assert np.array_equal(net.upscale(img, ensemble=2, tail=7), E.to_u8(E.mean_f32(ys[:2])))


def test_network_class_upscale_and_upscale_device(ctx, nets):
    net = nets(64, 4, 2, 2, 2)
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


def test_pipeline_with_sr_weights(tmp_path):
    """process() with sr_weights pointing at a saved RCAN: the family is picked from the file, the run stays device-resident,
    and tile 0 -- which pools over itself, as every tile does -- matches the restatement under the u8 rule."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(64, 4, 1, 1, 2)
    wpath = str(tmp_path / "rcan.npz")
    np.savez(wpath, **state)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, block_size=64, sr_scale=2, num_pyramid_levels=4))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.RCANSRNet) and pipe._builtin_backend()
    assert pipe.sr_net.desc.res_scale == np.float32(ref.RES_SCALE)                  # the .npz extras
    res = asyncio.run(pipe.process(src, str(tmp_path / "out.png")))
    assert res.success, res.error_message
    assert res.total_blocks == res.successful_blocks > 1 and res.failed_blocks == 0
    assert "sr_net" in pipe.stage_times and "sr_stub" not in pipe.stage_times
    assert pipe.transfers["h2d_bytes"] == img.nbytes                                # the network keeps the run device-resident
    assert np.asarray(Image.open(str(tmp_path / "out.png"))).shape == (160, 192, 3)
    tile0 = pipe.tiling_module.split_image(src)[0].data                              # tile 0 through the module against the restatement
    f64 = ref.forward(state, tile0, "float64")
    e32 = float(np.max(np.abs(ref.forward(state, tile0, "float32").astype(np.float64) - f64)))
    ref.check_u8(pipe.sr_net.upscale(tile0), f64, e32)


# ---- exact networks and one-hot probes ------------------------------------------------------------------------------------
def _same_bits(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want)) if got.dtype == np.float32 else np.argwhere(got != want)
    if len(bad):
        y, x, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at (Y {y}, X {x}, channel {c}): "
                             f"got {got[y, x, c]!r}, expected {want[y, x, c]!r}; rows {sorted(set(bad[:, 0].tolist()))[:12]}, "
                             f"columns {sorted(set(bad[:, 1].tolist()))[:12]}")


def _check_exact(ctx, name, k):
    """GPU == chain_forward bit for bit (fp32) and byte for byte (u8): one tail piece, tail pieces of 3, and through a padded,
    offset source view into guarded destinations."""
    import sr_network
    state, img, chain = ref.exact_case(name)
    h, w = img.shape[:2]
    want_u8 = _round_u8(chain)
    net = sr_network.RCANSRNet(state, res_scale=float(state["res_scale"]), img_range=float(state["img_range"]), rgb_mean=state["rgb_mean"])
    s = net.scale
    try:
        m = net.model(ctx)
        for tail in (0, 3):
            _same_bits(_f32(ctx, net, img, tail), chain, f"{name}: fp32, tail {tail}")
            _same_bits(net.upscale(img, tail=tail), want_u8, f"{name}: u8, tail {tail}")
        fill = V.FILLS[k % len(V.FILLS)]
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 3)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what=f"{name} u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what=f"{name} f32")
        finally:
            src.free(); dst.free(); dstf.free()
        _same_bits(got_u, want_u8, f"{name}: u8 through views")
        _same_bits(got_f, chain, f"{name}: fp32 through views")
    finally:
        net.close()


EXACT_IDS = [n[0] for n in ref.EXACT_NETS]
PROBE_IDS = [p[0] for p in ref.PROBES]


@pytest.mark.parametrize("name", EXACT_IDS)
def test_exact_networks_bit_equal(ctx, name):
    """Networks whose every partial sum is exact in fp32 and whose s is 0.5 exactly (proved in tests/test_rcan_host.py): no
    summation order can change a bit, so any difference is an index or a buffer error."""
    _check_exact(ctx, name, EXACT_IDS.index(name) + 1)


@pytest.mark.parametrize("name", PROBE_IDS)
def test_one_hot_probes_bit_equal(ctx, name):
    """A permutation of the channels at one off-centre tap of one convolution -- each RCAB convolution of a group's first and
    second block, both group convolutions, conv_after_body, a shuffle stage, the last convolution -- between centre-tap
    identities: a failure names the layer and the tap."""
    _check_exact(ctx, name, PROBE_IDS.index(name))
