"""GPU: the RRDB backend of csrc/sr_rrdb.hip (ESRGAN / Real-ESRGAN x4 on fp32 MFMA) against the torch-CPU restatement of its
contract (tests/_rrdb_ref.py) on seeded SYNTHETIC weights.

PARITY UNPINNED: the BasicSR / Real-ESRGAN packages and their checkpoints do not exist offline.  What is checked: the float
forward against the float64 restatement within 8 x the error torch's own float32 forward makes on the same input
(tests/test_rrdb_host.py holds the documented summation order alone inside it), the u8 output byte for byte away from rounding
boundaries, every (tile, tail) of the two-phase streaming == one trunk piece + one tail piece bit for bit, strided views,
determinism, reuse across shapes, the refusals, and the pipeline with ``sr_weights``.

The exact-arithmetic networks and one-hot probes of _rrdb_ref -- every partial sum representable in fp32, proved on the CPU in
tests/test_rrdb_host.py -- must be reproduced bit for bit whatever the summation order: the zero-tolerance check of the
concatenation's plane order in the dense buffer, the register -> cout map at both cout widths, the weight-slab layout, the tap
order, the double skip in place, the 2 x 2 replicating store at both stages and the padding at the true border."""
import asyncio
import ctypes as C

import numpy as np
import pytest

import _rrdb_ref as ref
import _views as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets():
    """One network per (F, G, B, conv_last bias), made once and closed at teardown."""
    import sr_network
    cache = {}

    def get(F, G, B, last_bias=ref.LAST_BIAS):
        key = (F, G, B, tuple(last_bias))
        if key not in cache:
            cache[key] = sr_network.RRDBSRNet(ref.synthetic_state(F, G, B, last_bias=last_bias))
        return cache[key]

    yield get
    for n in cache.values():
        n.close()


def _f32(ctx, net, img, tile=0, tail=0):
    h, w = img.shape[:2]
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * 4 * w * 4 * 3 * 4)
    try:
        net.model(ctx).forward_f32(d_src.ptr, w * 3, h, w, d_dst.ptr, w * 4 * 3 * 4, tile, tail)
        return ctx.download(d_dst.ptr, (h * 4, w * 4, 3), np.float32)
    finally:
        d_src.free(); d_dst.free()


def _bits(x):
    return x.view(np.uint32)


def _round_u8(f):
    return np.rint(np.clip(f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def _check_against(ctx, nets, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    F, G, B, h, w = case
    net = nets(F, G, B, ref.last_bias_of(case))
    state, img, f64, e32 = ref.case(*case)
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"rrdb {ref.case_id(case)}: e32 {e32:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}")
    assert 0 < e32 < 1e-5
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, _round_u8(got))                     # the float form rounded


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """Prints e32, the GPU error and the ratio per case before asserting ("RRDB network")."""
    _check_against(ctx, nets, case)


@pytest.mark.parametrize("case", ref.EDGE_CASES, ids=ref.case_id)
def test_degenerate_and_block_edge_shapes(ctx, nets, case):
    """One pixel, one row, one column, and exact / one-past multiples of the convolution's 8 x 32 block."""
    _check_against(ctx, nets, case)


@pytest.mark.parametrize("F,G,B,h,w,tiles,tails", [
    (64, 32, 1, 21, 37, (8, 13, 32, 0), (0, 5, 1)),
    (64, 32, 2, 20, 30, (4,), (0,)),          # the piece is below the halo of 34: every extent is clipped
    (64, 32, 1, 5, 6, (1,), (1,)),            # one-pixel trunk pieces and tail pieces
    (64, 32, 6, 16, 40, (8,), (8,)),          # the anime depth: a halo of 94 beyond the image on all sides
    (128, 64, 1, 12, 35, (7,), (3,)),         # two cout tiles, the 64-wide dense convolutions
])
def test_streaming_is_bit_equal(ctx, nets, F, G, B, h, w, tiles, tails):
    """fp32 bits and u8 bytes of every (tile, tail) equal those of one trunk piece + one tail piece; the piece counts are the
    plan's."""
    img = ref.make_image(h, w, seed=11)
    net = nets(F, G, B)
    m = net.model(ctx)
    assert m.plan(h, w, 64, 64)[:3] == (15 * B + 4, 1, 1)
    one_f, one_u = _f32(ctx, net, img, 64, 64), net.upscale(img, tile=64, tail=64)
    assert np.isfinite(one_f).all() and one_u.std() > 5
    assert np.array_equal(one_u, _round_u8(one_f))
    for tile in tiles:
        for tail in tails:
            t = tile or 2048                                     # tile 0: one piece on an image this small
            pieces = [(lo, min(lo + t, n)) for n in (h, w) for lo in range(0, n, t)]
            ny, nx = -(-h // t), -(-w // t)
            sub = lambda a, b: -(-(b - a) // (tail or 256))
            want_tail = sum(sub(*p) for p in pieces[:ny]) * sum(sub(*p) for p in pieces[ny:])
            assert m.plan(h, w, tile, tail)[1:3] == (ny * nx, want_tail), (tile, tail)
            assert m.plan(h, w, tile, tail) == ref.plan(F, G, B, h, w, tile, tail)
            assert np.array_equal(_bits(_f32(ctx, net, img, tile, tail)), _bits(one_f)), (tile, tail)
            assert np.array_equal(net.upscale(img, tile=tile, tail=tail), one_u), (tile, tail)


@pytest.mark.parametrize("case,k", [(ref.CASES[0], 1), (ref.CASES[2], 2), (ref.CASES[3], 3)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
def test_views(ctx, nets, case, k):
    """Padded, offset source view; destinations inside guarded parents; u8 (streamed) and fp32 entry points: equal bits and no
    byte written outside the view."""
    F, G, B, h, w = case
    net, img = nets(F, G, B), ref.case(*case)[1]
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * 4, w * 4 * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * 4, w * 4 * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 16, 5)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * 4, w * 4, 3), what="rrdb u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * 4, w * 4, 3), what="rrdb f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_model_reuse_across_shapes(ctx, nets):
    """One model, small image, larger image (the buffers are regrown), a streamed call, the small image again: first and last
    are bit-equal and every result equals another model's."""
    import sr_network
    small, large = ref.make_image(12, 20), ref.make_image(30, 45)
    other = nets(64, 32, 1)
    net = sr_network.RRDBSRNet(ref.synthetic_state(64, 32, 1))
    try:
        a = _f32(ctx, net, small)
        b = _f32(ctx, net, large)
        c = _f32(ctx, net, large, tile=16, tail=7)
        d = _f32(ctx, net, small)
        assert net.model(ctx).plan(30, 45, 16, 7)[1:3] == (6, (3 + 2) * (3 + 3 + 2))
        assert np.array_equal(_bits(a), _bits(d)) and np.array_equal(_bits(c), _bits(b))
        assert np.array_equal(_bits(a), _bits(_f32(ctx, other, small))) and np.array_equal(_bits(b), _bits(_f32(ctx, other, large)))
        assert np.array_equal(net.upscale(small), _round_u8(a))
    finally:
        net.close()


def test_deterministic_and_refusals(ctx, nets):
    """Equal inputs give equal bits over two calls; bad arguments raise before any launch (the guarded output stays untouched);
    a destroyed handle is refused, not dereferenced."""
    import _native
    net = nets(64, 32, 1)
    img = ref.make_image(19, 37)
    a, b = _f32(ctx, net, img), _f32(ctx, net, img)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(net.upscale(img), net.upscale(img))
    for bad in (img[:, :, 0], np.dstack([img, img[:, :, :1]]), img[:, :, :1]):
        with pytest.raises(ValueError):
            net.upscale(bad)
    with pytest.raises(ValueError):
        net.upscale(img.astype(np.float32))
    m = net.model(ctx)
    h, w = 19, 37
    d_src = ctx.upload(img)
    dst, d_dst, dstride = V.out_view(ctx, h * 4, w * 4 * 3, 0, 0, V.FILLS[0])
    try:
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, w * 4 * 3 - 1, 0, 0)       # destination stride shorter than a row
        with pytest.raises(ValueError):
            m.forward_f32(d_src.ptr, w * 3, h, w, d_dst, w * 4 * 3 * 4 - 4, 0, 0)
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, 0, w, d_dst, dstride, 0, 0)             # h = 0
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3 - 1, h, w, d_dst, dstride, 0, 0)         # short source stride
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, -1, 0)            # tile < 0
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, 0, -1)            # tail < 0
        with pytest.raises(ValueError):
            m.upscale_u8(0, w * 3, h, w, d_dst, dstride, 0, 0)
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, 0, dstride, 0, 0)
        # a destroyed handle: refused by the live-model set
        desc, ws, bs = net.desc, net._w, net._b
        gone = _native.RrdbModel(ctx, desc, ws, bs)
        handle = C.c_void_p(gone.handle.value)
        gone.close()
        for fn in (ctx.lib.sr_rrdb_u8, ctx.lib.sr_rrdb_f32):
            assert fn(handle, C.c_void_p(d_src.ptr), w * 3, h, w, C.c_void_p(d_dst), dstride, 0, 0) == _native.SR_ERR_INVALID_ARG
        assert "destroyed" in _native.last_error()
        assert ctx.lib.sr_rrdb_destroy(handle) == _native.SR_OK                    # a second destroy is a no-op
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(NotImplementedError):
        _native.RrdbModel(ctx, _native.rrdb_desc(96, 32, 1), [], [])
    with pytest.raises(NotImplementedError):
        _native.RrdbModel(ctx, _native.rrdb_desc(64, 32, 1, scale=2), [], [])
    with pytest.raises(ValueError):                                                 # a convolution of the wrong shape
        _native.RrdbModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)


def test_pipeline_with_sr_weights(tmp_path):
    """process() with sr_weights pointing at a saved RRDB network: the run stays device-resident, the canvas is byte-equal to the
    same run with sr_backend= a host callable around RRDBSRNet.upscale, and tile 0 matches the restatement."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(64, 32, 1)
    wpath = str(tmp_path / "net.npz")
    np.savez(wpath, **state)
    kw = dict(block_size=64, sr_scale=4, num_pyramid_levels=4)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.RRDBSRNet) and pipe._builtin_backend()
    res = asyncio.run(pipe.process(src, str(tmp_path / "out_dev.png")))
    assert res.success, res.error_message
    assert res.total_blocks == res.successful_blocks > 1 and res.failed_blocks == 0
    assert "sr_net" in pipe.stage_times and "sr_stub" not in pipe.stage_times
    assert pipe.transfers["h2d_bytes"] == img.nbytes                                # the network keeps the run device-resident
    net = sr_network.load_network(wpath)
    calls = []

    def backend(pipeline, tile, prompt):
        calls.append(tile.data.shape)
        return net.upscale(np.ascontiguousarray(tile.data))

    try:
        host = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw), sr_backend=backend)
        host.tiling_module.l2_cache_dir = tmp_path
        res2 = asyncio.run(host.process(src, str(tmp_path / "out_host.png")))
        assert res2.success and len(calls) == res.total_blocks
    finally:
        net.close()
    a, b = np.asarray(Image.open(str(tmp_path / "out_dev.png"))), np.asarray(Image.open(str(tmp_path / "out_host.png")))
    assert a.shape == (320, 384, 3) and np.array_equal(a, b)
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
    """GPU == chain_forward bit for bit (fp32) and byte for byte (u8): one piece, trunk pieces of 4 with tail pieces of 3, and
    through a padded, offset source view into guarded destinations."""
    import sr_network
    state, img, slope, beta, chain = ref.exact_case(name)
    h, w = img.shape[:2]
    want_u8 = _round_u8(chain)
    net = sr_network.RRDBSRNet(state, slope=slope, res_scale=beta)
    try:
        m = net.model(ctx)
        for tile, tail in ((0, 0), (4, 3)):
            _same_bits(_f32(ctx, net, img, tile, tail), chain, f"{name}: fp32, tile {tile}, tail {tail}")
            _same_bits(net.upscale(img, tile=tile, tail=tail), want_u8, f"{name}: u8, tile {tile}, tail {tail}")
        fill = V.FILLS[k % len(V.FILLS)]
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * 4, w * 4 * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * 4, w * 4 * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 4, 3)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * 4, w * 4, 3), what=f"{name} u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * 4, w * 4, 3), what=f"{name} f32")
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
    """Networks whose every partial sum is exact in fp32 (proved in tests/test_rrdb_host.py): no summation order, and nothing the
    MFMA does inside its two-term step, can change a bit, so any difference is an index error."""
    _check_exact(ctx, name, EXACT_IDS.index(name) + 1)


@pytest.mark.parametrize("name", PROBE_IDS)
def test_one_hot_probes_bit_equal(ctx, name):
    """A single unit weight at (cout, concatenation channel, tap) of one dense convolution -- every k, first and last channel of
    every segment, the three dense blocks, the double skip behind the third -- or a permutation at an off-centre tap of
    conv_body / conv_up1 / conv_up2 across the 2 x 2 replication on an odd-sized image: a failure names the layer and the tap."""
    _check_exact(ctx, name, PROBE_IDS.index(name))
