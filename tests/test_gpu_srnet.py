"""GPU: the compact SR network of csrc/sr_srnet.hip (fp32 MFMA) against the torch-CPU restatement of its contract
(tests/_srnet_ref.py) on seeded SYNTHETIC weights.

PARITY UNPINNED: the Real-ESRGAN package and its checkpoints do not exist offline.  What is checked: the float forward
against the float64 restatement within 8 x the error torch's own float32 forward makes on the same input (the kernel sums
9 F terms in one sequential fp32 chain, the CPU library in blocks: about sqrt(8) per layer on a random-walk error model),
the u8 output byte for byte away from rounding boundaries, streamed == unstreamed bit for bit, the exact structure (pixel
shuffle order, nearest base), strided views, determinism, the refusals, and the pipeline with ``sr_weights``.

The random-walk argument does not carry the bar on its own: ref.chain_forward restates the kernel's documented summation order
in numpy fp32, and tests/test_srnet_host.py asserts that this order alone stays within 8 x e32 on every case here (worst 5.07
at F = 256).  The accuracy tests print e_chain and both ratios beside the GPU error."""
import asyncio

import numpy as np
import pytest

import _srnet_ref as ref
import _views as V

pytestmark = pytest.mark.gpu

CASES = ref.CASES


def _net(state, act="prelu"):
    import sr_network
    return sr_network.CompactSRNet(state, act=act)


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(F, D, s):
        if (F, D, s) not in cache:
            cache[(F, D, s)] = _net(ref.synthetic_state(F, D, s))
        return cache[(F, D, s)]

    yield get
    for n in cache.values():
        n.close()


def _f32(ctx, net, img, tile=0):
    h, w = img.shape[:2]
    s = net.scale
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * s * w * s * 3 * 4)
    try:
        net.model(ctx).forward_f32(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * 3 * 4, tile)
        return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.float32)
    finally:
        d_src.free(); d_dst.free()


def _check_against(ctx, net, img, f64, e32, e_chain, what):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"srnet {what}: e32 {e32:.3e}  e_chain {e_chain:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}  "
          f"e_chain / e32 {e_chain / e32:.3f}  gpu / e_chain {err / e_chain:.3f}")
    assert 0 < e32 < 1e-5
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    # the u8 form is the float form rounded: exactly
    assert np.array_equal(u8, np.rint(np.clip(got, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))


@pytest.mark.parametrize("F,D,s,h,w", CASES)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, F, D, s, h, w):
    """Checks 1 and 2.  Prints e32, e_chain (the documented summation order in numpy fp32), the GPU error and the ratios per
    case before asserting ("Local SR network")."""
    state, img, f64, e32 = ref.case(F, D, s, h, w)
    assert (f64 < 0).any() or (f64 > 1).any()              # this case clamps (both sides over the cases: the test below)
    _check_against(ctx, nets(F, D, s), img, f64, e32, ref.chain_case(F, D, s, h, w)[1], f"F={F} D={D} s={s} {h}x{w}")


def test_reference_exercises_both_clamps():
    """Check 2's condition on the inputs: every case has reference outputs above 1, and every case has some below 0 except
    exactly the two small scale-4 images, 9 x 11 and 12 x 35: they are bright everywhere (x / 7 and y / 5 stay below pi / 2
    over most of them), so they only clamp at 1.  The other scale-4 case (19 x 37) clamps on both sides."""
    lo = {c: int((ref.case(*c)[2] < 0).sum()) for c in CASES}
    hi = {c: int((ref.case(*c)[2] > 1).sum()) for c in CASES}
    assert all(v > 0 for v in hi.values()), hi
    assert {c for c, v in lo.items() if v == 0} == {(64, 0, 4, 9, 11), (256, 2, 4, 12, 35)}, lo
    assert lo[(128, 2, 4, 19, 37)] > 0 and hi[(128, 2, 4, 19, 37)] > 0        # the two-half tail clamps on both sides


@pytest.mark.parametrize("F,D,s,h,w", ref.EDGE_CASES)
def test_degenerate_and_block_edge_shapes(ctx, nets, F, D, s, h, w):
    """One pixel, one row, one column, and exact / one-past multiples of the convolution's 8 x 32 block, against the
    restatement with the bars of the test above (the images are too small to ask for clamping)."""
    state, img, f64, e32 = ref.case(F, D, s, h, w)
    _check_against(ctx, nets(F, D, s), img, f64, e32, ref.chain_case(F, D, s, h, w)[1], f"F={F} D={D} s={s} {h}x{w}")


@pytest.mark.parametrize("act,slope", [("relu", 0.0), ("leakyrelu", 0.1), ("prelu", None)])
def test_activations_other_than_per_channel_prelu(ctx, act, slope):
    """act='relu' and act='leakyrelu' on a state without slope entries, and act='prelu' with one shared slope per layer,
    against the restatement given the same slopes (F = 64, D = 2, s = 2 on 20 x 35)."""
    st = ref.synthetic_state(64, 2, 2)
    if slope is None:
        state = dict(st)
        for k, v in ((1, 0.25), (3, 0.05), (5, 0.3)):
            state[f"body.{k}.weight"] = np.array([v], np.float32)               # nn.PReLU(): one value for every channel
        slope = 0.0
    else:
        state = {k: v for k, v in st.items() if np.asarray(v).ndim != 1 or k.endswith("bias")}
        assert len(state) == len(st) - 3
    img = ref.make_image(20, 35)
    f64 = ref.forward(state, img, "float64", default_slope=slope)
    e32 = float(np.max(np.abs(ref.forward(state, img, "float32", default_slope=slope).astype(np.float64) - f64)))
    e_chain = float(np.max(np.abs(ref.chain_forward(state, img, default_slope=slope).astype(np.float64) - f64)))
    # the activation matters: the per-channel network's output is far from this one
    assert np.max(np.abs(ref.forward(st, img, "float64") - f64)) > 1e-3
    net = _net(state, act)
    try:
        _check_against(ctx, net, img, f64, e32, e_chain, f"act={act} F=64 D=2 s=2 20x35")
    finally:
        net.close()


def test_streaming_is_bit_equal(ctx, nets):
    """Check 3: every sub-tile size gives the bits of tile 160 -- u8 and fp32."""
    img = ref.make_image(150, 210, seed=11)
    net = nets(64, 16, 2)
    assert net.model(ctx).plan(150, 210, 160)[:2] == (18, 2)
    assert net.model(ctx).plan(300, 210, 160)[1] == 4
    base_f = _f32(ctx, net, img, tile=160)
    base_u = net.upscale(img, tile=160)
    assert np.isfinite(base_f).all() and base_u.std() > 10
    # 150 x 210 under tile 160 is 1 x 2 sub-tiles; tile 96 gives 2 x 3 and covers a four-neighbour corner
    for tile in (32, 64, 96, 0):
        assert np.array_equal(_f32(ctx, net, img, tile=tile).view(np.uint32), base_f.view(np.uint32)), tile
        assert np.array_equal(net.upscale(img, tile=tile), base_u), tile
    small = nets(64, 2, 2)
    one = _f32(ctx, small, img, tile=256)                                       # a single sub-tile
    assert small.model(ctx).plan(150, 210, 256)[1] == 1
    for tile in (75, 105, 0):                                                   # four sub-tiles: 2 x 2
        assert np.array_equal(_f32(ctx, small, img, tile=tile).view(np.uint32), one.view(np.uint32)), tile
    assert small.model(ctx).plan(150, 210, 105)[1] == 4
    assert np.array_equal(small.upscale(img, tile=105), small.upscale(img, tile=256))


@pytest.mark.parametrize("F,D,s,h,w,tiles", [
    (128, 3, 3, 40, 70, {16: 3 * 5, 27: 2 * 3}),           # scale 3, two cout tiles
    (64, 1, 4, 21, 37, {8: 3 * 5, 13: 2 * 3}),             # scale 4: the two-half tail's origin arithmetic
    (64, 16, 2, 20, 30, {8: 3 * 4}),                       # tile < halo (18): every extent of every sub-tile is clipped by the image
    (64, 1, 2, 5, 6, {1: 30}),                             # one-pixel sub-tiles
])
def test_streaming_other_scales_and_tiny_tiles(ctx, nets, F, D, s, h, w, tiles):
    """Check 3 where the sub-tile arithmetic depends on the scale, on the cout tile and on clipping: fp32 bits and u8 bytes of
    every sub-tile size equal those of one sub-tile."""
    img = ref.make_image(h, w, seed=11)
    net = nets(F, D, s)
    m = net.model(ctx)
    assert m.plan(h, w, 128)[:2] == (D + 2, 1)
    one_f, one_u = _f32(ctx, net, img, tile=128), net.upscale(img, tile=128)
    assert np.isfinite(one_f).all() and one_u.std() > 5
    assert np.array_equal(one_u, np.rint(np.clip(one_f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
    for tile, count in tiles.items():
        assert m.plan(h, w, tile)[1] == count, tile
        assert np.array_equal(_f32(ctx, net, img, tile=tile).view(np.uint32), one_f.view(np.uint32)), tile
        assert np.array_equal(net.upscale(img, tile=tile), one_u), tile


def test_model_reuse_regrows_buffers(ctx, nets):
    """One model, small image, larger image (the activation buffers are freed and reallocated), a streamed call, then the
    small image again: the first and last results are bit-equal and every result equals a fresh model's."""
    small, large = ref.make_image(20, 35), ref.make_image(45, 77)
    ref_net = nets(64, 2, 2)                               # other tests have used it: its buffers are at their largest
    want_small, want_large = _f32(ctx, ref_net, small), _f32(ctx, ref_net, large)
    net = _net(ref.synthetic_state(64, 2, 2))
    fresh = _net(ref.synthetic_state(64, 2, 2))
    try:
        a = _f32(ctx, net, small)
        b = _f32(ctx, net, large)                          # regrowth
        c = _f32(ctx, net, large, tile=32)                 # streamed, 2 x 3 sub-tiles of the regrown buffers
        d = _f32(ctx, net, small)
        assert net.model(ctx).plan(45, 77, 32)[1] == 6
        bits = lambda x: x.view(np.uint32)
        assert np.array_equal(bits(a), bits(d))
        assert np.array_equal(bits(b), bits(_f32(ctx, fresh, large)))      # a model whose first call is the large image
        assert np.array_equal(bits(c), bits(b))
        assert np.array_equal(bits(a), bits(want_small)) and np.array_equal(bits(b), bits(want_large))
        ua, ub, ud = net.upscale(small), net.upscale(large, tile=32), net.upscale(small)
        assert np.array_equal(ua, ud) and np.array_equal(ub, fresh.upscale(large))
        assert np.array_equal(ua, np.rint(np.clip(a, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
    finally:
        net.close(); fresh.close()


def test_exact_structure(ctx):
    """Check 4: zero weights give the nearest upsample; a tail bias of k / 255 on a black image spells out the pixel-shuffle
    order out[Y, X, c] == c s^2 + (Y % s) s + (X % s)."""
    img = ref.make_image(21, 37, seed=3)
    for s in (2, 3, 4):
        st = {k: np.zeros_like(v) for k, v in ref.synthetic_state(64, 1, s).items()}
        net = _net(st)
        try:
            assert np.array_equal(net.upscale(img), np.repeat(np.repeat(img, s, axis=0), s, axis=1))
            st["body.4.bias"] = (np.arange(3 * s * s) / 255.0).astype(np.float32)
            net2 = _net(st)
            out = net2.upscale(np.zeros((7, 9, 3), np.uint8))
            Y, X, c = np.meshgrid(np.arange(7 * s), np.arange(9 * s), np.arange(3), indexing="ij")
            assert np.array_equal(out, (c * s * s + (Y % s) * s + (X % s)).astype(np.uint8))
            net2.close()
        finally:
            net.close()


@pytest.mark.parametrize("k", [1, 4])
def test_views(ctx, nets, k):
    """Check 5: padded, offset source view; destination inside a guarded parent; u8 and fp32 entry points."""
    _check_views(ctx, nets(64, 2, 2), ref.make_image(45, 77), k)


@pytest.mark.parametrize("F,D,s,h,w,k", [(128, 2, 4, 19, 37, 2), (128, 3, 3, 33, 41, 3)])
def test_views_at_scale_3_and_4(ctx, nets, F, D, s, h, w, k):
    """Check 5 where the HWC store's row and column arithmetic differs: scale 4 (two-half tail) and scale 3."""
    _check_views(ctx, nets(F, D, s), ref.case(F, D, s, h, w)[1], k)


def _check_views(ctx, net, img, k):
    (h, w), s = img.shape[:2], net.scale
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 32)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="srnet u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="srnet f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(got_f.view(np.uint32), dense_f.view(np.uint32))


def test_deterministic_and_refusals(ctx, nets):
    """Check 6: equal inputs give equal bits over two calls; bad arguments raise before any launch (the guarded output stays
    untouched)."""
    import _native
    net = nets(64, 2, 2)
    img = ref.make_image(45, 77)
    a, b = _f32(ctx, net, img), _f32(ctx, net, img)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(net.upscale(img), net.upscale(img))
    for bad in (img[:, :, 0], np.dstack([img, img[:, :, :1]]), img[:, :, :1]):     # cn != 3 through the module
        with pytest.raises(ValueError):
            net.upscale(bad)
    with pytest.raises(ValueError):
        net.upscale(img.astype(np.float32))
    m = net.model(ctx)
    h, w = 45, 77
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
            m.upscale_u8(d_src.ptr, w * 3 - 1, h, w, d_dst, dstride, 0)
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, -1)
        with pytest.raises(ValueError):
            m.upscale_u8(0, w * 3, h, w, d_dst, dstride, 0)
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, 0, dstride, 0)
        ctx.sync()
        rect = V.check_guard(ctx, dst, np.uint8, what="refused calls")
        assert (rect == V.FILLS[0]).all()                                           # nothing was launched
    finally:
        d_src.free(); dst.free()
    with pytest.raises(NotImplementedError):
        _native.SrNetModel(ctx, 48, 1, 2, [], [], [])


def test_pipeline_with_sr_weights(rng, tmp_path):
    """Check 7: process() with a saved (64, 2, 2) network; device-resident and host-array paths agree byte for byte; tile 0's SR
    output satisfies the u8 check against the restatement."""
    import main as sr_main
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)                                            # a 96 x 80 PNG
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(64, 2, 2)
    wpath = str(tmp_path / "net.npz")
    np.savez(wpath, **state)
    kw = dict(block_size=64, sr_scale=2, num_pyramid_levels=4, sr_weights=wpath)
    outs = {}
    for resident in (True, False):
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(device_resident=resident, **kw))
        pipe.tiling_module.l2_cache_dir = tmp_path
        out = str(tmp_path / f"out{int(resident)}.png")
        res = asyncio.run(pipe.process(src, out))
        assert res.success, res.error_message
        assert res.total_blocks == res.successful_blocks > 1 and res.failed_blocks == 0
        outs[resident] = np.asarray(Image.open(out))
        if resident:
            assert "sr_net" in pipe.stage_times and "sr_stub" not in pipe.stage_times
            tr = pipe.transfers
            assert tr["h2d_bytes"] == img.nbytes                                    # the network keeps the run device-resident
    assert outs[True].shape == (160, 192, 3) and np.array_equal(outs[True], outs[False])
    # not the stub's output
    stub = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(block_size=64, sr_scale=2, num_pyramid_levels=4))
    res = asyncio.run(stub.process(src, str(tmp_path / "stub.png")))
    assert res.success and "sr_stub" in stub.stage_times
    assert not np.array_equal(np.asarray(Image.open(str(tmp_path / "stub.png"))), outs[True])
    # tile 0 through the module against the restatement
    tile0 = pipe.tiling_module.split_image(src)[0].data
    assert tile0.shape == (64, 64, 3)
    f64 = ref.forward(state, tile0, "float64")
    e32 = float(np.max(np.abs(ref.forward(state, tile0, "float32").astype(np.float64) - f64)))
    ref.check_u8(pipe.sr_net.upscale(tile0), f64, e32)
