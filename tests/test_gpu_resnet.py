"""GPU: the residual SR family of csrc/sr_resnet.hip (MSRResNet / EDSR on fp32 MFMA) against the torch-CPU restatement of its
contract (tests/_resnet_ref.py) on seeded SYNTHETIC weights.

PARITY UNPINNED: the BasicSR package and its checkpoints do not exist offline.  What is checked: the float forward against the
float64 restatement within 8 x the error torch's own float32 forward makes on the same input (the project's yardstick;
tests/test_resnet_host.py holds the documented summation order alone inside it), the u8 output byte for byte away from rounding
boundaries, streamed == unstreamed bit for bit across both resolution changes, strided views, determinism, reuse across shapes,
the refusals, and the pipeline with ``sr_weights``.

Beyond the two presets the loader produces, the C ABI's descriptor is driven directly (_native.ResNetModel): the descriptor-space
list (every flag combination, every scale, distinct non-preset slopes, res_scale, mean and range) against the same bars, and
the exact-arithmetic networks and one-hot probes of _resnet_ref -- every partial sum representable in fp32, proved on the CPU
in tests/test_resnet_host.py -- which the GPU must reproduce bit for bit whatever its summation order: the zero-tolerance
check of the register -> cout map, the weight-slab layout, the tap order, the shuffle scatter, the in-place skip and the
padding at the true border."""
import asyncio
import dataclasses

import numpy as np
import pytest

import _resnet_ref as ref
import _views as V

pytestmark = pytest.mark.gpu


def _net(preset, F, B, s, res_scale=1.0):
    import sr_network
    st = ref.synthetic_state(preset, F, B, s, res_scale=res_scale)
    return sr_network.ResidualSRNet(st, **{k: st[k] for k in ("res_scale", "img_range", "rgb_mean") if k in st})


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(preset, F, B, s, res_scale=1.0):
        key = (preset, F, B, s, res_scale)
        if key not in cache:
            cache[key] = _net(*key)
        return cache[key]

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


def _bits(x):
    return x.view(np.uint32)


def _check_against(ctx, net, case):
    """The float bar (err <= 8 e32), the u8 check and u8 == the float form rounded; prints every figure before it asserts."""
    state, img, f64, e32 = ref.case(*case)
    e_chain = ref.chain_case(*case)[1]
    got = _f32(ctx, net, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"resnet {ref.case_id(case)}: e32 {e32:.3e}  e_chain {e_chain:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}  "
          f"e_chain / e32 {e_chain / e32:.3f}  gpu / e_chain {err / e_chain:.3f}")
    assert 0 < e32 < 1e-5
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = net.upscale(img)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, np.rint(np.clip(got, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))   # the float form rounded


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_float_forward_and_u8_match_the_restatement(ctx, nets, case):
    """Prints e32, e_chain, the GPU error and the ratios per case before asserting ("Residual SR network")."""
    preset, F, B, s, h, w, rs = case
    _check_against(ctx, nets(preset, F, B, s, rs), case)


@pytest.mark.parametrize("case", ref.EDGE_CASES, ids=ref.case_id)
def test_degenerate_and_block_edge_shapes(ctx, nets, case):
    """One pixel, one row, one column, and exact / one-past multiples of the convolution's 8 x 32 block."""
    preset, F, B, s, h, w, rs = case
    _check_against(ctx, nets(preset, F, B, s, rs), case)


@pytest.mark.parametrize("preset,F,B,s,h,w,tiles", [
    ("msr", 64, 1, 4, 21, 37, {8: 3 * 5, 13: 2 * 3, 32: 1 * 2, 0: 1}),      # two shuffle stages, the HR conv and the bilinear base
    ("edsr", 64, 1, 4, 21, 37, {8: 3 * 5, 13: 2 * 3, 32: 1 * 2, 0: 1}),     # ... and the long skip, h kept across the block
    ("edsr", 128, 1, 3, 40, 70, {16: 3 * 5, 27: 2 * 3, 0: 1}),              # r = 3 (the outward division is not exact), two cout tiles
    ("msr", 64, 1, 3, 40, 70, {16: 3 * 5, 27: 2 * 3, 0: 1}),
    ("msr", 64, 2, 2, 20, 30, {4: 5 * 8}),                                  # sub-tile (4) smaller than the halo (7): every extent clipped
    ("edsr", 64, 2, 2, 5, 6, {1: 30}),                                      # one-pixel sub-tiles; in-place blocks behind a kept h
    ("msr", 64, 0, 1, 20, 35, {7: 3 * 5}),                                  # no block, no shuffle
    ("edsr", 64, 16, 2, 16, 40, {8: 2 * 5}),                                # the shipped depth: a halo of 35 beyond the image, every extent clipped on all sides
])
def test_streaming_is_bit_equal(ctx, nets, preset, F, B, s, h, w, tiles):
    """fp32 bits and u8 bytes of every sub-tile size equal those of one sub-tile."""
    img = ref.make_image(h, w, seed=11)
    net = nets(preset, F, B, s, 0.1 if preset == "edsr" else 1.0)
    m = net.model(ctx)
    assert m.plan(h, w, 128)[1] == 1
    one_f, one_u = _f32(ctx, net, img, tile=128), net.upscale(img, tile=128)
    assert np.isfinite(one_f).all() and one_u.std() > 5
    assert np.array_equal(one_u, np.rint(np.clip(one_f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
    for tile, count in tiles.items():
        assert m.plan(h, w, tile)[1] == count, tile
        assert np.array_equal(_bits(_f32(ctx, net, img, tile=tile)), _bits(one_f)), tile
        assert np.array_equal(net.upscale(img, tile=tile), one_u), tile


@pytest.mark.parametrize("case,k", [(ref.CASES[0], 1), (ref.CASES[1], 2), (ref.CASES[5], 3), (ref.CASES[4], 4)], ids=lambda v: v if isinstance(v, int) else ref.case_id(v))
def test_views(ctx, nets, case, k):
    """Padded, offset source view; destinations inside guarded parents; u8 (streamed) and fp32 entry points: equal bits and no
    byte written outside the view."""
    preset, F, B, s, h, w, rs = case
    net, img = nets(preset, F, B, s, rs), ref.case(*case)[1]
    dense_u, dense_f = net.upscale(img), _f32(ctx, net, img)
    m = net.model(ctx)
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 16)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what="resnet u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what="resnet f32")
        finally:
            src.free(); dst.free(); dstf.free()
        assert np.array_equal(got_u, dense_u)
        assert np.array_equal(_bits(got_f), _bits(dense_f))


def test_model_reuse_across_shapes(ctx, nets):
    """One model, small image, larger image (the buffers are regrown), a streamed call, the small image again: first and last
    are bit-equal and every result equals another model's."""
    small, large = ref.make_image(20, 35), ref.make_image(45, 77)
    for preset in ("msr", "edsr"):
        other = nets(preset, 64, 2, 2, 0.1 if preset == "edsr" else 1.0)
        net = _net(preset, 64, 2, 2, 0.1 if preset == "edsr" else 1.0)
        try:
            a = _f32(ctx, net, small)
            b = _f32(ctx, net, large)
            c = _f32(ctx, net, large, tile=32)
            d = _f32(ctx, net, small)
            assert net.model(ctx).plan(45, 77, 32)[1] == 6
            assert np.array_equal(_bits(a), _bits(d)) and np.array_equal(_bits(c), _bits(b))
            assert np.array_equal(_bits(a), _bits(_f32(ctx, other, small))) and np.array_equal(_bits(b), _bits(_f32(ctx, other, large)))
            assert np.array_equal(net.upscale(small), np.rint(np.clip(a, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))
        finally:
            net.close()


def test_exact_structure(ctx):
    """Zero weights: MSRResNet gives the bilinear base (the image itself at odd-scale centres and at scale 1), EDSR the mean;
    res_scale scales the residual branch only."""
    import sr_network
    img = ref.make_image(21, 37, seed=3)
    for s in (1, 2, 3, 4):
        st = {k: np.zeros_like(v) for k, v in ref.synthetic_state("msr", 64, 1, s).items()}
        net = sr_network.ResidualSRNet(st)
        try:
            out = net.upscale(img)
            assert out.shape == (21 * s, 37 * s, 3)
            want = ref.quantize(ref.chain_forward(st, img))
            assert np.abs(out.astype(int) - want.astype(int)).max() <= 1 and (out != want).mean() < 0.01
            if s % 2:
                assert np.array_equal(out[s // 2::s, s // 2::s], img)
        finally:
            net.close()
    ed = {k: np.zeros_like(v) for k, v in ref.synthetic_state("edsr", 64, 1, 2).items()}
    net = sr_network.ResidualSRNet(ed)                           # BasicSR's default mean and range
    try:
        assert np.array_equal(net.upscale(img), np.broadcast_to(ref.quantize(np.array(ref.RGB_MEAN, np.float32)), (42, 74, 3)))
    finally:
        net.close()
    st = ref.synthetic_state("edsr", 64, 1, 2)
    outs = []
    for rs in (0.0, 0.1):
        net = sr_network.ResidualSRNet(st, res_scale=rs)
        outs.append(_f32(ctx, net, img))
        net.close()
    no_block = {k: v for k, v in st.items() if not k.startswith("body.")}
    net = sr_network.ResidualSRNet(no_block)
    try:
        assert np.array_equal(_bits(outs[0]), _bits(_f32(ctx, net, img)))           # res_scale 0: the block is the identity
        assert np.max(np.abs(outs[0] - outs[1])) > 1e-3
    finally:
        net.close()


def test_deterministic_and_refusals(ctx, nets):
    """Equal inputs give equal bits over two calls; bad arguments raise before any launch (the guarded output stays untouched)."""
    import _native
    net = nets("msr", 64, 2, 2)
    img = ref.make_image(45, 77)
    for n in (net, nets("edsr", 64, 2, 2, 0.1)):
        a, b = _f32(ctx, n, img), _f32(ctx, n, img)
        assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(n.upscale(img), n.upscale(img))
    for bad in (img[:, :, 0], np.dstack([img, img[:, :, :1]]), img[:, :, :1]):
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
            m.upscale_u8(d_src.ptr, w * 3 - 1, h, w, d_dst, dstride, 0)            # short source stride
        with pytest.raises(ValueError):
            m.upscale_u8(d_src.ptr, w * 3, h, w, d_dst, dstride, -1)               # tile < 0
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
        _native.ResNetModel(ctx, _native.resnet_desc(96, 1, 2), [], [])
    with pytest.raises(ValueError):                                                 # a convolution of the wrong shape
        _native.ResNetModel(ctx, net.desc, net._w[:-1] + [net._w[-1][:2]], net._b)


@pytest.mark.parametrize("preset", ["msr", "edsr"])
def test_pipeline_with_sr_weights(tmp_path, preset):
    """process() with sr_weights pointing at a saved network of each preset: the canvas is byte-equal to the same run with
    sr_backend= a host callable around ResidualSRNet.upscale; a mismatched sr_scale raises."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(preset, 64, 1, 2, res_scale=0.1)
    wpath = str(tmp_path / "net.npz")
    np.savez(wpath, **state)
    kw = dict(block_size=64, sr_scale=2, num_pyramid_levels=4)
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, **kw))
    pipe.tiling_module.l2_cache_dir = tmp_path
    assert isinstance(pipe.sr_net, sr_network.ResidualSRNet) and pipe._builtin_backend()
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
    assert a.shape == (160, 192, 3) and np.array_equal(a, b)
    tile0 = pipe.tiling_module.split_image(src)[0].data                              # tile 0 through the module against the restatement
    f64 = ref.forward(state, tile0, "float64")
    e32 = float(np.max(np.abs(ref.forward(state, tile0, "float32").astype(np.float64) - f64)))
    ref.check_u8(pipe.sr_net.upscale(tile0), f64, e32)
    with pytest.raises(ValueError, match="sr_scale"):
        sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, block_size=64, sr_scale=4))


# ---- the descriptor itself, through _native.ResNetModel ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(ctx):
    """One model per (descriptor, weights tag), created once and closed at teardown."""
    import _native
    cache = {}

    def get(desc, tag, weights, biases):
        key = (desc, tag)
        if key not in cache:
            cache[key] = _native.ResNetModel(ctx, _native.resnet_desc(**dataclasses.asdict(desc)), weights, biases)
        return cache[key]

    yield get
    for m in cache.values():
        m.close()


def _run(ctx, m, img, tile=0, u8=False):
    h, w = img.shape[:2]
    s, esz = m.scale, 1 if u8 else 4
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * s * w * s * 3 * esz)
    try:
        (m.upscale_u8 if u8 else m.forward_f32)(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * 3 * esz, tile)
        return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.uint8 if u8 else np.float32)
    finally:
        d_src.free(); d_dst.free()


def _round_u8(f):
    return np.rint(np.clip(f, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


@pytest.mark.parametrize("case", ref.DESC_CASES, ids=ref.desc_id)
def test_descriptor_space(ctx, models, case):
    """Every flag combination, every scale and distinct non-preset slopes, res_scale, mean and range (tests/test_resnet_host.py
    shows that each field moves the result by more than 100 e32): the float bar, the u8 check, u8 == the float form rounded, and
    sub-tiles of 5 and 16 bit-equal to one sub-tile.  Prints every figure before it asserts."""
    name, desc = case
    ws, bs, img, f64, e32 = ref.desc_case(desc)
    e_chain = ref.desc_chain_case(desc)[1]
    m = models(desc, "synthetic", ws, bs)
    got = _run(ctx, m, img)
    err = float(np.max(np.abs(got.astype(np.float64) - f64)))
    print(f"resnet desc {name}: e32 {e32:.3e}  e_chain {e_chain:.3e}  gpu err {err:.3e}  gpu / e32 {err / e32:.3f}  "
          f"e_chain / e32 {e_chain / e32:.3f}  gpu / e_chain {err / e_chain:.3f}")
    assert 0 < e32 < 1e-5
    assert err <= 8 * e32, (err, e32, err / e32)
    u8 = _run(ctx, m, img, u8=True)
    share = ref.check_u8(u8, f64, e32)
    print(f"  u8: exempt share {share:.4%}, bytes != rint(f64): {int((u8 != ref.quantize(f64)).sum())}")
    assert np.array_equal(u8, _round_u8(got))
    for tile in (5, 16):
        assert m.plan(ref.DESC_H, ref.DESC_W, tile)[1] == -(-ref.DESC_H // tile) * -(-ref.DESC_W // tile)
        assert np.array_equal(_bits(_run(ctx, m, img, tile=tile)), _bits(got)), tile
        assert np.array_equal(_run(ctx, m, img, tile=tile, u8=True), u8), tile


def _same_bits(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want)) if got.dtype == np.float32 else np.argwhere(got != want)
    if len(bad):
        y, x, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at (Y {y}, X {x}, channel {c}): "
                             f"got {got[y, x, c]!r}, expected {want[y, x, c]!r}; rows {sorted(set(bad[:, 0].tolist()))[:12]}, "
                             f"columns {sorted(set(bad[:, 1].tolist()))[:12]}")


def _check_exact(ctx, models, name, k):
    """GPU == chain_forward_desc bit for bit (fp32) and byte for byte (u8): one sub-tile, sub-tiles of 4, and through a padded,
    offset source view into guarded destinations."""
    desc, ws, bs, img, chain = ref.exact_case(name)
    h, w = img.shape[:2]
    s = desc.scale
    want_u8 = _round_u8(chain)
    m = models(desc, name, ws, bs)
    for tile in (0, 4):
        assert m.plan(h, w, tile)[1] == (1 if tile == 0 else -(-h // 4) * -(-w // 4))
        _same_bits(_run(ctx, m, img, tile=tile), chain, f"{name}: fp32, tile {tile}")
        _same_bits(_run(ctx, m, img, tile=tile, u8=True), want_u8, f"{name}: u8, tile {tile}")
    for fill in V.FILLS:
        src, d_src, sstride = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
        dst, d_dst, dstride = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
        dstf, d_dstf, dstridef = V.out_view(ctx, h * s, w * s * 3 * 4, *V.pick(V.LAYOUTS_F32, k), fill)
        try:
            m.upscale_u8(d_src, sstride, h, w, d_dst, dstride, 4)
            m.forward_f32(d_src, sstride, h, w, d_dstf, dstridef, 0)
            got_u = V.check_guard(ctx, dst, np.uint8, (h * s, w * s, 3), what=f"{name} u8")
            got_f = V.check_guard(ctx, dstf, np.float32, (h * s, w * s, 3), what=f"{name} f32")
        finally:
            src.free(); dst.free(); dstf.free()
        _same_bits(got_u, want_u8, f"{name}: u8 through views, fill {fill:#x}")
        _same_bits(got_f, chain, f"{name}: fp32 through views, fill {fill:#x}")


EXACT_IDS = [n[0] for n in ref.EXACT_NETS]
PROBE_IDS = [p[0] for p in ref.PROBES]


@pytest.mark.parametrize("name", EXACT_IDS)
def test_exact_networks_bit_equal(ctx, models, name):
    """Networks whose every partial sum is exact in fp32 (proved in tests/test_resnet_host.py): no summation order, and nothing the
    MFMA does inside its two-term step, can change a bit, so any difference is an index error."""
    _check_exact(ctx, models, name, EXACT_IDS.index(name) + 1)        # k: the view layouts walked, one pair per network


@pytest.mark.parametrize("name", PROBE_IDS)
def test_one_hot_probes_bit_equal(ctx, models, name):
    """One convolution is a pure tap with permuted channels, every other one the centre-tap identity: the output is a shifted,
    permuted copy with zeros entering at the true image border only, and a failure names the layer and the tap."""
    _check_exact(ctx, models, name, PROBE_IDS.index(name))
