"""GPU: the geometric self-ensemble of csrc/sr_ensemble.hip against the NumPy restatement of include/sr_hip.h
(tests/_ensemble_ref.py).

The primitives (sr_d4_u8, sr_d4_acc_f32, sr_ens_finish_*) are byte-equal to the restatement for all eight transforms, on
shapes around the kernel's LDS tile (64 pixels for u8, 32 for fp32) and on padded, offset, guarded views.  The composition is
bit-equal, for each of the three families, to the restatement driven by the family's existing forward_f32 on host-transformed
inputs; it does not depend on tile / tail; and for the compact network the full ensemble stays within the single forward's
bar (8 x torch-float32's own error) of the mean of eight torch-float64 forwards."""
import asyncio

import numpy as np
import pytest

import _ensemble_ref as E
import _native
import _srnet_ref as ref
import _views as V

pytestmark = pytest.mark.gpu

U8_TILE, F32_TILE = 64, 32                                        # D4Tile<uint8_t>::TP, D4Tile<float>::TP of csrc/sr_ensemble.hip
SHAPES = [(1, 1), (1, 37), (37, 1), (31, 33), (64, 64), (65, 63), (130, 257),
          (32, 32), (31, 32), (33, 32), (32, 31), (32, 33), (63, 64), (65, 64), (64, 63), (64, 65)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _floats(rng, shape):
    """fp32 values with negatives, values above 1, and magnitudes far apart (so an addition in another order shows)."""
    a = rng.standard_normal(shape).astype(np.float32) * np.float32(1.5)
    a[rng.random(shape) < 0.1] *= np.float32(1e-4)
    return a


# ---- primitives ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_d4_u8_equals_the_restatement(ctx, rng, h, w):
    x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d_x = ctx.upload(x)
    d_t = ctx.alloc(h * w * 3)
    try:
        for k in range(8):
            want = E.d4(x, k)
            ctx.memset(d_t.ptr, 0xEE, h * w * 3)
            _native.d4_u8(ctx, d_x.ptr, w * 3, h, w, k, d_t.ptr, want.shape[1] * 3)
            assert np.array_equal(ctx.download(d_t.ptr, want.shape, np.uint8), want), k
    finally:
        d_x.free(); d_t.free()


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_d4_acc_first_then_add_equals_the_restatement(ctx, rng, H, W):
    """acc = T_k^-1(y1), then acc = acc + T_k^-1(y2), over two different inputs; compared as bits."""
    d_acc = ctx.alloc(H * W * 12)
    try:
        for k in range(8):
            ys = (W, H, 3) if k & 4 else (H, W, 3)
            y1, y2 = _floats(rng, ys), _floats(rng, ys)
            d1, d2 = ctx.upload(y1), ctx.upload(y2)
            ctx.memset(d_acc.ptr, 0xEE, H * W * 12)
            _native.d4_acc_f32(ctx, d1.ptr, ys[1] * 12, H, W, k, True, d_acc.ptr, W * 12)
            first = ctx.download(d_acc.ptr, (H, W, 3), np.float32)
            _native.d4_acc_f32(ctx, d2.ptr, ys[1] * 12, H, W, k, False, d_acc.ptr, W * 12)
            both = ctx.download(d_acc.ptr, (H, W, 3), np.float32)
            d1.free(); d2.free()
            assert np.array_equal(bits(first), bits(E.d4_inv(y1, k))), k
            assert np.array_equal(bits(both), bits((E.d4_inv(y1, k) + E.d4_inv(y2, k)).astype(np.float32))), k
    finally:
        d_acc.free()


def _finish_values(rng, H, W, n):
    """Accumulator values whose quotient by n covers negatives, values above 1 and exact .5 / 255 ties of the u8 rule."""
    acc = (_floats(rng, (H, W, 3)) * np.float32(n)).astype(np.float32)
    m = np.arange(0, 255, dtype=np.float32)
    o = ((m + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    s = (o * np.float32(n)).astype(np.float32)
    q = (s / np.float32(n)).astype(np.float32)
    tie = (q * np.float32(255.0)).astype(np.float32) == m + np.float32(0.5)
    ties = s[tie]
    flat = acc.reshape(-1)
    flat[:ties.size] = ties
    flat[ties.size:ties.size + 4] = [np.float32(-0.0), np.float32(0.0), np.float32(n), np.float32(3e-39)]
    return acc, int(ties.size)


@pytest.mark.parametrize("n", range(1, 9))
def test_finish_divides_and_rounds_as_defined(ctx, rng, n):
    H, W = 33, 47
    acc, n_ties = _finish_values(rng, H, W, n)
    assert n_ties >= 20                                           # the ties exist for every n
    o = (acc / np.float32(n)).astype(np.float32)
    assert (o < 0).any() and (o > 1).any()
    d_acc, d_f, d_u = ctx.upload(acc), ctx.alloc(H * W * 12), ctx.alloc(H * W * 3)
    try:
        _native.ens_finish(ctx, d_acc.ptr, W * 12, H, W, n, d_f.ptr, W * 12, False)
        _native.ens_finish(ctx, d_acc.ptr, W * 12, H, W, n, d_u.ptr, W * 3, True)
        got_f, got_u = ctx.download(d_f.ptr, (H, W, 3), np.float32), ctx.download(d_u.ptr, (H, W, 3), np.uint8)
    finally:
        d_acc.free(); d_f.free(); d_u.free()
    assert np.array_equal(bits(got_f), bits(o))
    assert np.array_equal(got_u, E.to_u8(o))


# ---- strided views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(8))
def test_primitives_on_views(ctx, rng, k):
    """Source, accumulator and destination as padded, offset views inside guarded parents: results equal the dense ones and
    not a byte outside a view is written."""
    h, w = 45, 70
    fill = V.FILLS[k % 2]
    x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = E.d4(x, k)
    th, tw = want.shape[:2]
    src, d_src, sst = V.embed(ctx, x.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, k), fill)
    dst, d_dst, dst_st = V.out_view(ctx, th, tw * 3, *V.pick(V.LAYOUTS_U8, k + 5), fill)
    try:
        _native.d4_u8(ctx, d_src, sst, h, w, k, d_dst, dst_st)
        assert np.array_equal(V.check_guard(ctx, dst, np.uint8, want.shape, what=f"sr_d4_u8 k {k}"), want)
    finally:
        src.free(); dst.free()
    y1, y2 = _floats(rng, (th, tw, 3)), _floats(rng, (th, tw, 3))
    s = (E.d4_inv(y1, k) + E.d4_inv(y2, k)).astype(np.float32)
    p1, d1, st1 = V.embed(ctx, y1.reshape(th, tw * 3), *V.pick(V.LAYOUTS_F32, k), fill)
    p2, d2, st2 = V.embed(ctx, y2.reshape(th, tw * 3), *V.pick(V.LAYOUTS_F32, k + 1), fill)
    pa, da, sta = V.out_view(ctx, h, w * 12, *V.pick(V.LAYOUTS_F32, k + 2), fill)
    pf, df, stf = V.out_view(ctx, h, w * 12, *V.pick(V.LAYOUTS_F32, k + 3), fill)
    pu, du, stu = V.out_view(ctx, h, w * 3, *V.pick(V.LAYOUTS_U8, k + 7), fill)
    try:
        _native.d4_acc_f32(ctx, d1, st1, h, w, k, True, da, sta)
        _native.d4_acc_f32(ctx, d2, st2, h, w, k, False, da, sta)
        assert np.array_equal(bits(V.check_guard(ctx, pa, np.float32, (h, w, 3), what=f"sr_d4_acc_f32 k {k}")), bits(s))
        _native.ens_finish(ctx, da, sta, h, w, 2, df, stf, False)
        _native.ens_finish(ctx, da, sta, h, w, 2, du, stu, True)
        o = (s / np.float32(2)).astype(np.float32)
        assert np.array_equal(bits(V.check_guard(ctx, pf, np.float32, (h, w, 3), what="sr_ens_finish_f32")), bits(o))
        assert np.array_equal(V.check_guard(ctx, pu, np.uint8, (h, w, 3), what="sr_ens_finish_u8"), E.to_u8(o))
        V.check_guard(ctx, pa, np.float32, (h, w, 3), what="accumulator after the finish")
    finally:
        for p in (p1, p2, pa, pf, pu):
            p.free()


def test_row_stride_beyond_32_bits(ctx, rng):
    """Two rows 2^32 + 4100 bytes apart (one 4.0 GiB allocation, set to a fill on the device): as the source of sr_d4_u8, then
    as the accumulator of sr_d4_acc_f32 and of both finishes.  A kernel that formed a row offset in 32 bits would read or
    write row 1 at byte 4100."""
    stride, lead, fill = (1 << 32) + 4100, 256, V.FILLS[0]
    w = 40
    total = lead + stride + w * 12 + V.GUARD
    assert stride > 1 << 32 and total < 8 << 30
    big = ctx.alloc(total)
    base = big.ptr + lead
    try:
        ctx.memset(big.ptr, fill, total)
        x = rng.integers(0, 256, (2, w, 3), dtype=np.uint8)
        d_x = ctx.upload(x)
        for r in range(2):
            ctx.copy_d2d(base + r * stride, d_x.ptr + r * w * 3, w * 3)
        d_t = ctx.alloc(w * 2 * 3)
        _native.d4_u8(ctx, base, stride, 2, w, 5, d_t.ptr, 6)
        assert np.array_equal(ctx.download(d_t.ptr, (w, 2, 3), np.uint8), E.d4(x, 5))
        d_x.free(); d_t.free()
        # the accumulator: 2 x 40 from a dense 40 x 2 source (k = 6), first and add
        ctx.memset(big.ptr, fill, total)
        y1, y2 = _floats(rng, (w, 2, 3)), _floats(rng, (w, 2, 3))
        d1, d2 = ctx.upload(y1), ctx.upload(y2)
        _native.d4_acc_f32(ctx, d1.ptr, 24, 2, w, 6, True, base, stride)
        _native.d4_acc_f32(ctx, d2.ptr, 24, 2, w, 6, False, base, stride)
        s = (E.d4_inv(y1, 6) + E.d4_inv(y2, 6)).astype(np.float32)
        d_f, d_u = ctx.alloc(2 * w * 12), ctx.alloc(2 * w * 3)
        _native.ens_finish(ctx, base, stride, 2, w, 2, d_f.ptr, w * 12, False)
        _native.ens_finish(ctx, base, stride, 2, w, 2, d_u.ptr, w * 3, True)
        for r in range(2):
            row = ctx.download(base + r * stride - 64, (64 + w * 12 + 64,), np.uint8)
            assert np.all(row[:64] == fill) and np.all(row[-64:] == fill), f"bytes beside accumulator row {r} were written"
            assert np.array_equal(row[64:-64].view(np.uint32), bits(s[r]).reshape(-1)), f"accumulator row {r}"
        low = ctx.download(base + 4100 - 64, (64 + w * 12 + 64,), np.uint8)        # where a 32-bit row offset would land
        assert np.all(low == fill)
        o = (s / np.float32(2)).astype(np.float32)
        assert np.array_equal(bits(ctx.download(d_f.ptr, (2, w, 3), np.float32)), bits(o))
        assert np.array_equal(ctx.download(d_u.ptr, (2, w, 3), np.uint8), E.to_u8(o))
        for d in (d1, d2, d_f, d_u):
            d.free()
    finally:
        ctx.sync()
        big.free()


# ---- composition, bit for bit ------------------------------------------------------------------------------------------------
H0, W0 = 23, 37
MASKS = [0x01] + [1 << k for k in range(1, 8)] + [0x03, 0x0F, 0xFF, 0xA5, 0x07]


def _make_net(family):
    import sr_network
    if family == "compact":
        return sr_network.CompactSRNet(ref.synthetic_state(64, 1, 2))
    if family == "msrresnet":
        import _resnet_ref
        return sr_network.ResidualSRNet(_resnet_ref.synthetic_state("msr", 64, 1, 2))
    import _rrdb_ref
    return sr_network.RRDBSRNet(_rrdb_ref.synthetic_state(64, 32, 1))


def _forward(ctx, net, img, ens=None, u8=False, **run):
    """forward_f32 / upscale_u8 (ens None) or ensemble_f32 / ensemble_u8 (ens = mask) of a host image -> host array."""
    h, w = img.shape[:2]
    s = net.scale
    px = 3 if u8 else 12
    d_src, d_dst = ctx.upload(img), ctx.alloc(h * s * w * s * px)
    try:
        m = net.model(ctx)
        if ens is None:
            (m.upscale_u8 if u8 else m.forward_f32)(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * px, **run)
        else:
            (m.ensemble_u8 if u8 else m.ensemble_f32)(d_src.ptr, w * 3, h, w, d_dst.ptr, w * s * px, mask=ens, **run)
        return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.uint8 if u8 else np.float32)
    finally:
        d_src.free(); d_dst.free()


@pytest.fixture(scope="module")
def families(ctx):
    """Per family: the network, the image, and y_k = T_k^-1(forward_f32(T_k(x))) for the eight k -- computed once, read-only."""
    cache = {}

    def get(family):
        if family not in cache:
            net = _make_net(family)
            img = ref.make_image(H0, W0, seed=11)
            ys = []
            for k in range(8):
                y = E.d4_inv(_forward(ctx, net, E.d4(img, k)), k)
                y.setflags(write=False)
                ys.append(y)
            cache[family] = (net, img, ys)
        return cache[family]

    yield get
    for net, _, _ in cache.values():
        net.close()


@pytest.mark.parametrize("family", ["compact", "msrresnet", "rrdb"])
def test_ensemble_equals_the_restatement_bit_for_bit(ctx, families, family):
    net, img, ys = families(family)
    assert not np.array_equal(ys[0], ys[1]) and not np.array_equal(ys[0], ys[4])     # the networks are not equivariant
    plain_f, plain_u = _forward(ctx, net, img), _forward(ctx, net, img, u8=True)
    for mask in MASKS:
        want = E.mean_f32([ys[k] for k in E.members(mask)])
        got_f = _forward(ctx, net, img, ens=mask)
        got_u = _forward(ctx, net, img, ens=mask, u8=True)
        assert np.array_equal(bits(got_f), bits(want)), f"{family} mask {mask:#x}"
        assert np.array_equal(got_u, E.to_u8(want)), f"{family} mask {mask:#x}"
        if mask & (mask - 1) == 0:                                # a one-bit mask gives y_k itself
            assert np.array_equal(bits(got_f), bits(ys[mask.bit_length() - 1]))
    assert np.array_equal(bits(_forward(ctx, net, img, ens=1)), bits(plain_f))       # mask 1 is the plain forward
    assert np.array_equal(_forward(ctx, net, img, ens=1, u8=True), plain_u)
    full = E.mean_f32(ys)
    assert not np.array_equal(E.to_u8(full), plain_u)


def test_ensemble_does_not_depend_on_tile_or_tail_and_is_deterministic(ctx, families):
    net, img, ys = families("rrdb")
    want = E.mean_f32(ys)
    for run in (dict(tile=64, tail=64), dict(tile=8, tail=5), dict(tile=13, tail=1), dict(tile=0, tail=0)):
        assert np.array_equal(bits(_forward(ctx, net, img, ens=0xFF, **run)), bits(want)), run
        assert np.array_equal(_forward(ctx, net, img, ens=0xFF, u8=True, **run), E.to_u8(want)), run
    a, b = _forward(ctx, net, img, ens=0xFF), _forward(ctx, net, img, ens=0xFF)
    assert np.array_equal(bits(a), bits(b))
    cnet, cimg, cys = families("compact")
    for tile in (8, 13, 0):
        assert np.array_equal(bits(_forward(ctx, cnet, cimg, ens=0xFF, tile=tile)), bits(E.mean_f32(cys))), tile


def test_model_ensemble_on_views_and_refusals(ctx, families):
    """The model entry points on padded, offset, guarded views; refused calls launch nothing."""
    net, img, ys = families("compact")
    m, (h, w), s = net.model(ctx), img.shape[:2], net.scale
    want = E.mean_f32(ys)
    fill = V.FILLS[1]
    src, d_src, sst = V.embed(ctx, img.reshape(h, w * 3), *V.pick(V.LAYOUTS_U8, 4), fill)
    pu, du, stu = V.out_view(ctx, h * s, w * s * 3, *V.pick(V.LAYOUTS_U8, 2), fill)
    pf, df, stf = V.out_view(ctx, h * s, w * s * 12, *V.pick(V.LAYOUTS_F32, 3), fill)
    try:
        for bad in (0, 256, -1):
            with pytest.raises(ValueError):
                m.ensemble_u8(d_src, sst, h, w, du, stu, mask=bad)
        with pytest.raises(ValueError):
            m.ensemble_u8(d_src, sst, h, w, du, w * s * 3 - 1, mask=0xFF)
        with pytest.raises(_native.SrShapeError):
            m.ensemble_f32(d_src, sst, h, w, df, stf + 2, mask=0xFF)
        with pytest.raises(ValueError):
            m.ensemble_u8(d_src, sst, h, w, du, stu, -1, mask=0xFF)
        with pytest.raises(ValueError):
            m.ensemble_u8(0, sst, h, w, du, stu, mask=0xFF)
        with pytest.raises(ValueError):
            m.ensemble_u8(d_src, sst, 0, w, du, stu, mask=0xFF)
        with pytest.raises(TypeError):
            m.ensemble_u8(d_src, sst, h, w, du, stu, 0, 0xFF)                     # the mask is given by name
        ctx.sync()
        assert (V.check_guard(ctx, pu, np.uint8, what="refused calls") == fill).all()
        m.ensemble_u8(d_src, sst, h, w, du, stu, 13, mask=0xFF)
        m.ensemble_f32(d_src, sst, h, w, df, stf, mask=0xFF)
        assert np.array_equal(V.check_guard(ctx, pu, np.uint8, (h * s, w * s, 3), what="ensemble u8"), E.to_u8(want))
        assert np.array_equal(bits(V.check_guard(ctx, pf, np.float32, (h * s, w * s, 3), what="ensemble f32")), bits(want))
        V.check_guard(ctx, src, np.uint8, what="the source")
    finally:
        src.free(); pu.free(); pf.free()


def test_compact_ensemble_against_eight_float64_forwards(ctx):
    """The full ensemble of the compact network against the mean of eight torch-float64 forwards of tests/_srnet_ref.py, within
    the bar tests/test_gpu_srnet.py holds a single forward to: 8 x torch-float32's own error against float64.  Averaging eight
    values that each lie within a bar of their truths stays within it, and the seven fp32 additions and the division add at
    most 8 roundings of 2^-24 relative to values of order 1 (5e-7), far below 8 e32's slack over the forwards' measured error."""
    import sr_network
    F, D, s, h, w = 64, 2, 2, 45, 77
    state, img, f64, e32 = ref.case(F, D, s, h, w)
    truth = np.mean([E.d4_inv(ref.forward(state, E.d4(img, k), "float64"), k) for k in range(8)], axis=0)
    net = sr_network.CompactSRNet(state)
    try:
        got = _forward(ctx, net, np.asarray(img), ens=0xFF)
        one = _forward(ctx, net, np.asarray(img))
    finally:
        net.close()
    err = float(np.max(np.abs(got.astype(np.float64) - truth)))
    err_one = float(np.max(np.abs(one.astype(np.float64) - f64)))
    print(f"ensemble 0xFF F={F} D={D} s={s} {h}x{w}: e32 {e32:.3e}  single forward err {err_one:.3e}  ensemble err {err:.3e}  "
          f"ensemble / e32 {err / e32:.3f}")
    assert 0 < e32 < 1e-5
    assert err <= 8 * e32, (err, e32, err / e32)
    assert np.max(np.abs(truth - f64)) > 1e-3                     # the ensemble is not the single forward


# ---- layers ------------------------------------------------------------------------------------------------------------------
def test_network_upscale_with_ensemble_equals_the_device_form(ctx, families):
    for family in ("compact", "rrdb"):
        net, img, ys = families(family)
        want = E.to_u8(E.mean_f32(ys))
        assert np.array_equal(net.upscale(img, ensemble=8), want), family
        assert np.array_equal(net.upscale(img, ensemble=8), _forward(ctx, net, img, ens=0xFF, u8=True)), family
        assert np.array_equal(net.upscale(img, ensemble=2), E.to_u8(E.mean_f32(ys[:2]))), family
        assert np.array_equal(net.upscale(img, ensemble=4, tile=8), E.to_u8(E.mean_f32(ys[:4]))), family
        assert np.array_equal(net.upscale(img, ensemble=1), net.upscale(img)), family


def test_pipeline_with_sr_ensemble(tmp_path):
    """process() with sr_weights + sr_ensemble=4: a canvas unlike sr_ensemble=1's, equal to the one blended from tiles upscaled
    with ensemble=4 by hand; sr_ensemble=1 gives the bytes of a run without the field."""
    import main as sr_main
    import sr_network
    from PIL import Image
    img = ref.make_image(80, 96, seed=5)
    src = str(tmp_path / "in.png")
    Image.fromarray(img).save(src)
    state = ref.synthetic_state(64, 1, 2)
    wpath = str(tmp_path / "net.npz")
    np.savez(wpath, **state)
    kw = dict(block_size=64, sr_scale=2, num_pyramid_levels=4)

    def run(name, backend=None, **cfg):
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(**kw, **cfg), sr_backend=backend)
        pipe.tiling_module.l2_cache_dir = tmp_path
        out = str(tmp_path / f"{name}.png")
        res = asyncio.run(pipe.process(src, out))
        assert res.success, res.error_message
        assert res.total_blocks == res.successful_blocks > 1
        return np.asarray(Image.open(out)), pipe

    unset, _ = run("unset", sr_weights=wpath)
    one, _ = run("one", sr_weights=wpath, sr_ensemble=1)
    four, pipe4 = run("four", sr_weights=wpath, sr_ensemble=4)
    assert "sr_net" in pipe4.stage_times and "sr_stub" not in pipe4.stage_times
    four_host, _ = run("four_host", sr_weights=wpath, sr_ensemble=4, device_resident=False)
    net = sr_network.CompactSRNet(state)
    try:
        by_hand, _ = run("by_hand", backend=lambda pipeline, tile, prompt: net.upscale(np.ascontiguousarray(tile.data), ensemble=4))
    finally:
        net.close()
    assert np.array_equal(one, unset)
    assert not np.array_equal(four, one)
    assert np.array_equal(four, by_hand) and np.array_equal(four, four_host)
