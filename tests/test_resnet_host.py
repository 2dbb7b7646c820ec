"""CPU: the host side of the residual SR backend (MSRResNet / EDSR) -- sr_resnet_plan (no context, no GPU) against a Python
restatement of the backward extent rule, the BasicSR state-dict parser, load_network's dispatch, the ABI's refusals, and the
accuracy condition of tests/test_gpu_resnet.py held against the documented summation order.  The descriptor-driven reference
(_resnet_ref.forward_desc / chain_forward_desc) is held to the two preset forwards bit for bit, the descriptor-space list to the
same bars plus a sensitivity check (every live field moves the result by more than 100 e32), and the exact-arithmetic networks
to their proof of exactness and their coverage.  No device call is made here."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _native
import _resnet_ref as ref
import _srnet_ref as sref
import main as sr_main
import sr_network


def _desc(preset, F, B, s, res_scale=1.0):
    if preset == "edsr":
        return _native.resnet_desc(F, B, s, long_skip=True, res_scale=res_scale, mean=ref.RGB_MEAN, range=255.0)
    return _native.resnet_desc(F, B, s, conv_hr=True, bilinear_base=True, a_head=0.1, a_up=0.1, a_hr=0.1)


def _ops(preset, B, s):
    """(shuffle factor, resolution multiplier of the convolution) in forward order."""
    ops = [(1, 1)] * (1 + 2 * B + (1 if preset == "edsr" else 0))
    m = 1
    for r in ref.STAGES[s]:
        ops.append((r, m))
        m *= r
    return ops + [(1, s)] * (2 if preset == "msr" else 1)


def _extents(ops, s, lo, hi, n):
    """The issue's rule on one axis: backwards from the sub-tile's output range, grown by one per convolution, divided by r
    (outward) across a shuffle, clipped to the layer's image -> the length r (b - a) each layer stores."""
    a, b, out = lo * s, hi * s, []
    for r, mult in reversed(ops):
        a, b = a // r, -(-b // r)
        out.append((b - a) * r)
        a, b = max(a - 1, 0), min(b + 1, n * mult)
    return out[::-1]


def _plan(preset, F, B, s, h, w, tile):
    ops = _ops(preset, B, s)
    halo = 0
    for r, _ in reversed(ops):
        halo = -(-halo // r) + 1
    if tile == 0:
        fits = [t for t in range(32, 2049, 32) if 3 * F * (s * (t + 2 * halo)) ** 2 * 4 <= 1 << 30]
        tile = max(fits) if fits else 32
    ty, tx = -(-h // tile), -(-w // tile)
    rows = np.max([_extents(ops, s, i * tile, min(i * tile + tile, h), h) for i in range(ty)], axis=0)
    cols = np.max([_extents(ops, s, i * tile, min(i * tile + tile, w), w) for i in range(tx)], axis=0)
    plane = int(np.max(rows[:-1] * ((cols[:-1] + 3) // 4 * 4)))
    return halo, ty * tx, 3 * F * plane * 4


def test_plan_matches_the_backward_extent_rule():
    # halo: one per convolution, halved (outward) across a shuffle
    assert _native.resnet_plan(_desc("msr", 64, 1, 4), 19, 37, 8)[0] == 5          # last 1, hr 2, up 2, up 2, conv2 3, conv1 4, head 5
    assert _native.resnet_plan(_desc("msr", 64, 16, 2), 100, 100, 32)[0] == 2 + 32 + 1
    assert _native.resnet_plan(_desc("edsr", 64, 2, 3), 100, 100, 32)[0] == 1 + 1 + 1 + 4 + 1
    assert _native.resnet_plan(_desc("edsr", 64, 0, 1), 10, 10, 0)[0] == 3
    for preset, F, B, s, h, w, tile in (("msr", 64, 2, 2, 45, 77, 0), ("msr", 64, 2, 2, 45, 77, 16), ("msr", 64, 1, 4, 19, 37, 8),
                                        ("msr", 64, 1, 4, 19, 37, 13), ("msr", 64, 1, 3, 40, 70, 27), ("msr", 64, 0, 1, 20, 35, 7),
                                        ("edsr", 128, 1, 3, 17, 40, 16), ("edsr", 256, 1, 4, 12, 35, 1), ("edsr", 64, 2, 2, 5, 6, 1),
                                        ("edsr", 64, 32, 2, 3000, 2000, 0), ("msr", 256, 16, 4, 4096, 4096, 0),
                                        ("msr", 64, 16, 4, 300, 5000, 0)):
        assert _native.resnet_plan(_desc(preset, F, B, s), h, w, tile) == _plan(preset, F, B, s, h, w, tile), (preset, F, B, s, h, w, tile)
    # tile 0 comes from the 1 GiB workspace cap, not from a fixed 2048: F = 64 at scale 4 streams a 4096 x 4096 input
    halo, n, ws = _native.resnet_plan(_desc("msr", 64, 16, 4), 4096, 4096, 0)
    assert n > 1 and ws <= 1 << 30
    assert _native.resnet_plan(_desc("edsr", 64, 16, 1), 2048, 2048, 0)[1] > 1      # 3 x 64 x 2048^2 floats is 3 GiB
    assert _native.resnet_plan(_desc("edsr", 64, 16, 1), 1000, 1000, 0)[1] == 1
    # one sub-tile: the workspace is three F-channel buffers of the whole HR image
    assert _native.resnet_plan(_desc("msr", 64, 1, 2), 20, 30, 64) == (5, 1, 3 * 64 * 40 * 60 * 4)


def test_plan_and_create_refusals():
    for F, B, s in ((96, 1, 2), (48, 1, 2), (64, 65, 2), (64, 1, 5), (64, -1, 2), (64, 1, 0), (320, 1, 2)):
        with pytest.raises(NotImplementedError):
            _native.resnet_plan(_desc("msr", F, B, s), 100, 100, 0)
    for field, value in (("long_skip", 2), ("range", 0.0), ("range", float("nan")), ("res_scale", float("inf"))):
        d = _desc("edsr", 64, 1, 2)
        setattr(d, field, value)
        with pytest.raises(NotImplementedError):
            _native.resnet_plan(d, 100, 100, 0)
    d = _desc("msr", 64, 1, 2)
    with pytest.raises(ValueError):
        _native.resnet_plan(d, 100, 100, -1)                     # tile < 0
    with pytest.raises(ValueError):
        _native.resnet_plan(d, 0, 100, 0)                        # h < 1
    with pytest.raises(ValueError):
        _native.resnet_plan(d, 100, 0, 0)
    with pytest.raises(ValueError):                              # (h s) x (w s x 3) must fit int
        _native.resnet_plan(_desc("msr", 64, 1, 4), 100, 200_000_000, 64)
    with pytest.raises(ValueError):                              # a sub-tile beyond the kernels' 32-bit offsets
        _native.resnet_plan(d, 30000, 30000, 30000)
    lib = _native.load()
    assert lib.sr_resnet_plan(None, 10, 10, 0, None, None, None) == _native.SR_ERR_INVALID_ARG       # null description
    assert lib.sr_resnet_plan(C.byref(d), 10, 10, 0, None, None, None) == _native.SR_OK              # outputs may be NULL
    out = C.c_void_p()
    assert lib.sr_resnet_create(None, None, None, None, 0, C.byref(out)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_resnet_create(None, C.byref(d), None, None, 0, None) == _native.SR_ERR_INVALID_ARG  # null out
    assert lib.sr_resnet_create(None, C.byref(d), None, None, 6, C.byref(out)) == _native.SR_ERR_INVALID_ARG   # null tables
    assert lib.sr_resnet_create(None, C.byref(_desc("msr", 96, 1, 2)), None, None, 6, C.byref(out)) == _native.SR_ERR_UNSUPPORTED
    for fn in (lib.sr_resnet_u8, lib.sr_resnet_f32):             # null model
        assert fn(None, None, 0, 1, 1, None, 0, 0) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_resnet_destroy(None) == _native.SR_OK
    with pytest.raises(NotImplementedError):
        _native.ResNetModel(None, _desc("msr", 96, 1, 2), [], [])                  # refused before the context is looked at
    with pytest.raises(ValueError):
        _native.ResNetModel(None, d, [], [])                                        # wrong number of arrays, before the context


@pytest.mark.parametrize("preset,F,B,s", [("msr", 64, 2, 2), ("msr", 64, 1, 4), ("msr", 128, 0, 1), ("edsr", 64, 2, 2), ("edsr", 128, 1, 3),
                                          ("edsr", 64, 1, 4)])
def test_parse_both_presets(preset, F, B, s):
    st = ref.synthetic_state(preset, F, B, s, res_scale=0.1)
    kw = {k: st[k] for k in ("res_scale", "img_range", "rgb_mean") if k in st}
    desc, w, b = sr_network.parse_residual_state(st, **kw)
    assert (desc.n_feat, desc.n_blocks, desc.scale) == (F, B, s)
    shapes = _native.resnet_conv_shapes(desc)
    assert [x.shape for x in w] == [(co, ci, 3, 3) for co, ci in shapes] and [x.shape for x in b] == [(co,) for co, _ in shapes]
    assert all(x.dtype == np.float32 and x.flags.c_contiguous for x in w + b)
    n_up = len(ref.STAGES[s])
    if preset == "msr":
        assert (desc.long_skip, desc.conv_hr, desc.bilinear_base) == (0, 1, 1)
        assert (desc.a_head, desc.a_up, desc.a_hr, desc.res_scale, desc.range) == (np.float32(0.1),) * 3 + (1.0, 1.0) and list(desc.mean) == [0, 0, 0]
        names = ["conv_first"] + [f"body.{i}.conv{j}" for i in range(B) for j in (1, 2)] + [f"upconv{k + 1}" for k in range(n_up)] + ["conv_hr", "conv_last"]
    else:
        assert (desc.long_skip, desc.conv_hr, desc.bilinear_base) == (1, 0, 0)
        assert (desc.a_head, desc.a_up, desc.res_scale, desc.range) == (1.0, 1.0, np.float32(0.1), 255.0)
        assert list(desc.mean) == [float(np.float32(v)) for v in ref.RGB_MEAN]
        names = (["conv_first"] + [f"body.{i}.conv{j}" for i in range(B) for j in (1, 2)] + ["conv_after_body"]
                 + [f"upsample.{2 * k}" for k in range(n_up)] + ["conv_last"])
    assert len(names) == len(w)
    for name, wk, bk in zip(names, w, b):
        assert np.array_equal(wk, st[f"{name}.weight"]) and np.array_equal(bk, st[f"{name}.bias"])
    net = sr_network.ResidualSRNet({"params_ema": st}, **kw)
    assert (net.n_feat, net.n_blocks, net.scale, net.preset) == (F, B, s, "edsr" if preset == "edsr" else "msrresnet")
    # EDSR defaults when nothing is said: BasicSR's
    if preset == "edsr":
        d2 = sr_network.parse_residual_state({k: v for k, v in st.items() if k not in kw})[0]
        assert (d2.res_scale, d2.range) == (1.0, 255.0) and list(d2.mean) == [float(np.float32(v)) for v in ref.RGB_MEAN]


def test_parse_refusals_name_the_key():
    msr, edsr = ref.synthetic_state("msr", 64, 2, 2), ref.synthetic_state("edsr", 64, 1, 3)

    def bad(state, key, value, match):
        st = dict(state)
        if value is None:
            del st[key]
        else:
            st[key] = value
        with pytest.raises(ValueError, match=match):
            sr_network.parse_residual_state(st)

    z = lambda *shape: np.zeros(shape, np.float32)
    bad(msr, "body.1.conv1.weight", z(64, 32, 3, 3), r"body\.1\.conv1\.weight takes 32 channels")       # wrong cin
    bad(msr, "conv_first.weight", z(64, 4, 3, 3), r"conv_first\.weight takes 4 channels")
    bad(msr, "body.0.conv2.bias", None, r"body\.0\.conv2\.bias")                                          # missing bias
    bad(edsr, "conv_after_body.bias", None, r"conv_after_body\.bias")
    bad(msr, "conv_hr.weight", z(64, 64, 5, 5), r"conv_hr\.weight: only 3x3")                             # non-3x3
    bad(edsr, "body.0.conv1.weight", z(64, 64, 1, 1), r"body\.0\.conv1\.weight: only 3x3")
    bad(msr, "upconv1.weight", z(128, 64, 3, 3), r"upconv1\.weight gives 128 channels")                   # couts != F r^2
    bad(edsr, "upsample.0.weight", z(64 * 5, 64, 3, 3), r"upsample\.0\.weight gives 320 channels")
    bad(msr, "conv_last.weight", z(12, 64, 3, 3), r"conv_last\.weight gives 12 channels")
    bad(msr, "conv_hr.weight", None, r"conv_hr\.weight")
    bad(msr, "body.1.conv2.weight", z(32, 64, 3, 3), r"body\.1\.conv2\.weight gives 32 channels")
    bad(msr, "conv_last.bias", z(4), r"conv_last\.bias")
    x4 = ref.synthetic_state("msr", 64, 1, 4)
    bad(x4, "upconv2.weight", z(64 * 9, 64, 3, 3), r"upconv2\.weight gives 576 channels")                 # two stages are 2 x 2
    gap = {k.replace("body.1.", "body.2."): v for k, v in msr.items()}
    with pytest.raises(ValueError, match="body"):
        sr_network.parse_residual_state(gap)
    with pytest.raises(ValueError, match="conv_first"):
        sr_network.parse_residual_state(sref.synthetic_state(64, 1, 2))
    with pytest.raises(NotImplementedError):                     # F = 96 chains but is outside the kernels' range
        sr_network.parse_residual_state(ref.synthetic_state("msr", 96, 1, 2))
    with pytest.raises(NotImplementedError):
        sr_network.ResidualSRNet(ref.synthetic_state("edsr", 96, 1, 2))
    with pytest.raises(ValueError, match="rgb_mean"):
        sr_network._residual_extras({"rgb_mean": np.zeros(2)})


def test_load_network_dispatch(tmp_path):
    compact = tmp_path / "compact.npz"
    np.savez(compact, **sref.synthetic_state(64, 2, 2))
    net = sr_network.load_network(str(compact))
    assert type(net) is sr_network.CompactSRNet and (net.n_feat, net.n_body, net.scale) == (64, 2, 2)
    plain = {k: v for k, v in sref.synthetic_state(64, 1, 3).items() if np.asarray(v).ndim != 1 or k.endswith("bias")}
    np.savez(tmp_path / "plain.npz", **plain)
    net = sr_network.load_network(str(tmp_path / "plain.npz"), act="leakyrelu")
    assert type(net) is sr_network.CompactSRNet and all(np.all(s == np.float32(0.1)) for s in net._s)
    st = ref.synthetic_state("edsr", 64, 1, 2, res_scale=0.1)
    st["img_range"], st["rgb_mean"] = np.array(1.0, np.float32), np.array([0.5, 0.25, 0.125], np.float32)
    np.savez(tmp_path / "edsr.npz", **st)
    net = sr_network.load_network(str(tmp_path / "edsr.npz"), act="relu")          # act is ignored for this family
    assert type(net) is sr_network.ResidualSRNet and net.preset == "edsr" and net.scale == 2
    assert (net.desc.res_scale, net.desc.range, list(net.desc.mean)) == (np.float32(0.1), 1.0, [0.5, 0.25, 0.125])
    again = sr_network.ResidualSRNet.from_file(str(tmp_path / "edsr.npz"), res_scale=0.5)
    assert (again.desc.res_scale, again.desc.range) == (0.5, 1.0)
    np.savez(tmp_path / "bare.npz", **{k: v for k, v in st.items() if k not in ("res_scale", "img_range", "rgb_mean")})
    bare = sr_network.load_network(str(tmp_path / "bare.npz"))
    assert (bare.desc.res_scale, bare.desc.range) == (1.0, 255.0)
    np.savez(tmp_path / "msr.npz", **ref.synthetic_state("msr", 64, 1, 4))
    net = sr_network.load_network(str(tmp_path / "msr.npz"))
    assert type(net) is sr_network.ResidualSRNet and net.preset == "msrresnet" and net.scale == 4


def test_pth_loader_unwraps_params(tmp_path):
    torch = pytest.importorskip("torch")
    st = ref.synthetic_state("msr", 64, 1, 3)
    torch.save({"params": {k: torch.from_numpy(v) for k, v in st.items()}}, str(tmp_path / "net.pth"))
    net = sr_network.load_network(str(tmp_path / "net.pth"))
    assert type(net) is sr_network.ResidualSRNet and net.scale == 3 and np.array_equal(net._w[1], st["body.0.conv1.weight"])


def test_pipeline_config_and_scale_mismatch(tmp_path):
    for preset in ("msr", "edsr"):
        path = tmp_path / f"{preset}.npz"
        np.savez(path, **ref.synthetic_state(preset, 64, 1, 4))
        with pytest.raises(ValueError, match="sr_scale"):        # no device is touched: this passes without a GPU
            sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=2))
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=4, block_size=64))
        assert isinstance(pipe.sr_net, sr_network.ResidualSRNet) and pipe.sr_net.scale == 4 and pipe._builtin_backend()


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_documented_summation_order_stays_inside_the_gpu_bar(case):
    """The accuracy bar of tests/test_gpu_resnet.py, err <= 8 e32, held against the kernels' documented summation order
    restated in numpy fp32 (ref.chain_forward): the order alone must fit the bar, or the bar says nothing about the kernels.
    Measured e_chain / e32 on the first seven CASES: 5.85, 5.32, 3.63, 3.08, 2.32, 2.58, 3.08; on the B = 16 and F = 192 cases
    4.59, 1.70, 4.75, 4.08; on the edge shapes 1.0 ... 4.4.  The exempt share of the u8 check stays below 0.25 % against its
    1 % cap."""
    preset, F, B, s, h, w, _ = case
    state, img, f64, e32 = ref.case(*case)
    chain, e_chain = ref.chain_case(*case)
    assert chain.dtype == np.float32 and chain.shape == f64.shape == (h * s, w * s, 3)
    f32 = ref.forward(state, img, "float32")
    d = float(np.max(np.abs(chain.astype(np.float64) - f32.astype(np.float64))))
    print(f"resnet chain {ref.case_id(case)}: e32 {e32:.3e}  e_chain {e_chain:.3e}  ratio {e_chain / e32:.3f}  |chain - f32| / e32 {d / e32:.3f}")
    assert e32 > 0
    assert e_chain <= 8 * e32, (e_chain, e32, e_chain / e32)     # the documented order alone is inside the GPU bar
    share = ref.check_u8(ref.quantize(chain), f64, e32)          # ... and inside the u8 check with its 1 % exempt cap
    print(f"  u8 of the chain: exempt share {share:.4%}")


def test_chain_forward_spells_out_the_structure():
    """chain_forward on hand-made states: zero weights give the bilinear base (MSRResNet; at scale 1 the image itself) or the
    mean (EDSR); a one-hot upconv bias lands where PixelShuffle puts it."""
    img = sref.make_image(5, 7, seed=3)
    x = img.astype(np.float32) / np.float32(255.0)
    for s in (1, 2, 3, 4):
        st = {k: np.zeros_like(v) for k, v in ref.synthetic_state("msr", 64, 1, s).items()}
        out = ref.chain_forward(st, img)
        assert out.shape == (5 * s, 7 * s, 3)
        if s == 1:
            assert np.array_equal(out, x)
        else:
            assert np.array_equal(out[s // 2::s, s // 2::s] if s % 2 else out[:1, :1], x if s % 2 else x[:1, :1])
            assert out.min() >= x.min() and out.max() <= x.max() + 1e-6
        ed = {k: np.zeros_like(v) for k, v in ref.synthetic_state("edsr", 64, 1, s).items()}
        ed["img_range"], ed["rgb_mean"] = np.array(255.0, np.float32), np.array(ref.RGB_MEAN, np.float32)
        assert np.array_equal(ref.chain_forward(ed, img), np.broadcast_to(np.array(ref.RGB_MEAN, np.float32), (5 * s, 7 * s, 3)))
    v = np.arange(2 * 9 * 2 * 3, dtype=np.float32).reshape(18, 2, 3)
    u = ref._shuffle(v, 3)
    assert u.shape == (2, 6, 9) and u[1, 4, 5] == v[9 + 1 * 3 + 2, 1, 1] and u[0, 0, 2] == v[2, 0, 0]


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_descriptor_reference_reproduces_the_preset_forwards(case):
    """forward_desc (float32 and float64) and chain_forward_desc on a preset's descriptor give the bits of forward and
    chain_forward: the generalisation itself is held to the two forwards it came from.  conv_roles restates the product's
    convolution list."""
    state, img, f64, _ = ref.case(*case)
    desc, ws, bs = ref.desc_of_state(state)
    assert [(co, ci) for _, co, ci in ref.conv_roles(desc)] == _native.resnet_conv_shapes(_native.resnet_desc(**dataclasses.asdict(desc)))
    assert np.array_equal(_bits(ref.forward_desc(desc, ws, bs, img, "float64")), _bits(f64))
    assert np.array_equal(_bits(ref.forward_desc(desc, ws, bs, img, "float32")), _bits(ref.forward(state, img, "float32")))
    assert np.array_equal(_bits(ref.chain_forward_desc(desc, ws, bs, img)), _bits(ref.chain_case(*case)[0]))


def _drop(desc, ws, bs, role):
    k = [r for r, _, _ in ref.conv_roles(desc)].index(role)
    return ws[:k] + ws[k + 1:], bs[:k] + bs[k + 1:]


def _perturbations(desc, ws, bs):
    """(what, perturbed descriptor, weights, biases, live): one field changed; live: whether the header's arithmetic reads it."""
    rep = dataclasses.replace
    ups = desc.scale > 1
    yield "a_head <-> a_up", rep(desc, a_head=desc.a_up, a_up=desc.a_head), ws, bs, desc.a_head != desc.a_up
    yield "a_up <-> a_hr", rep(desc, a_up=desc.a_hr, a_hr=desc.a_up), ws, bs, desc.a_up != desc.a_hr and (ups or desc.conv_hr)
    yield "res_scale -> 1", rep(desc, res_scale=1.0), ws, bs, desc.n_blocks > 0 and desc.res_scale != 1.0
    yield "mean rotated", rep(desc, mean=desc.mean[1:] + desc.mean[:1]), ws, bs, len(set(desc.mean)) > 1
    yield "range -> 1", rep(desc, range=1.0), ws, bs, desc.range != 1.0
    yield "bilinear_base flipped", rep(desc, bilinear_base=not desc.bilinear_base), ws, bs, True
    if desc.long_skip:                                           # a flag is switched off by dropping its convolution
        yield ("long_skip off", rep(desc, long_skip=False)) + _drop(desc, ws, bs, "after_body") + (True,)
    if desc.conv_hr:
        yield ("conv_hr off", rep(desc, conv_hr=False)) + _drop(desc, ws, bs, "hr") + (True,)


@pytest.mark.parametrize("case", ref.DESC_CASES, ids=ref.desc_id)
def test_descriptor_space_reference_bars_and_sensitivity(case):
    """For every descriptor of the GPU test's list: the documented order alone is inside 8 e32 and inside the u8 check's cap, and
    every field the descriptor reads moves the float64 forward by more than 100 e32 when perturbed (a field that is not read
    moves nothing) -- a case that did not would not be testing that field."""
    name, desc = case
    ws, bs, img, f64, e32 = ref.desc_case(desc)
    chain, e_chain = ref.desc_chain_case(desc)
    assert f64.shape == chain.shape == (ref.DESC_H * desc.scale, ref.DESC_W * desc.scale, 3)
    print(f"resnet desc {name}: e32 {e32:.3e}  e_chain {e_chain:.3e}  ratio {e_chain / e32:.3f}")
    assert 0 < e32 < 1e-5
    assert e_chain <= 8 * e32, (e_chain, e32, e_chain / e32)
    share = ref.check_u8(ref.quantize(chain), f64, e32)
    print(f"  u8 of the chain: exempt share {share:.4%}")
    for what, d2, w2, b2, live in _perturbations(desc, list(ws), list(bs)):
        moved = float(np.max(np.abs(ref.forward_desc(d2, w2, b2, img, "float64") - f64)))
        print(f"  {what}: moved {moved:.3e} = {moved / e32:.0f} e32 ({'live' if live else 'not read'})")
        if live:
            assert moved > 100 * e32, (name, what, moved, e32)
        else:
            assert moved == 0.0, (name, what, moved)


def test_descriptor_list_holds_what_it_promises():
    """All eight flag combinations at s = 2, every scale under (1, 1, 1), the long skip with no block, three blocks behind a kept
    h, and the slope / res_scale / range variants; every field is a non-preset value."""
    descs = dict(ref.DESC_CASES)
    assert len(descs) == len(ref.DESC_CASES) == 19
    assert {(d.long_skip, d.conv_hr, d.bilinear_base) for d in descs.values() if d.scale == 2 and d.n_blocks == 1} == {
        (a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    assert {d.scale for d in descs.values() if (d.long_skip, d.conv_hr, d.bilinear_base) == (True, True, True)} == {1, 2, 3, 4}
    assert {(d.scale, d.n_blocks) for d in descs.values() if (d.long_skip, d.conv_hr, d.bilinear_base) == (True, False, False)} >= {(1, 0), (2, 0)}
    assert descs["flags110-B3-x2"].n_blocks == 3 and descs["a_up-zero"].a_up == 0 and descs["a_hr-negative"].a_hr == -0.5
    assert descs["a_head-above-1"].a_head == 1.5 and descs["res_scale-negative"].res_scale == -0.5
    assert descs["range-255-base"].range == 255.0 and descs["range-255-base"].bilinear_base
    d = descs["flags111-B1-x2"]
    assert (d.n_feat, d.a_head, d.a_up, d.a_hr, d.res_scale, d.mean, d.range) == (64, 0.25, 0.05, 0.5, 0.5, (0.45, 0.30, 0.60), 2.0)


EXACT_IDS = [n[0] for n in ref.EXACT_NETS]
PROBE_IDS = [p[0] for p in ref.PROBES]


@pytest.mark.parametrize("name", EXACT_IDS + PROBE_IDS)
def test_exact_networks_are_exact(name):
    """The proof behind the zero-tolerance GPU tests: per convolution, every value is a whole multiple of the layer's unit and
    the absolute-value forward sum|w| |x| + |b| (a bound on every partial sum in any order), the skip add and the stored result
    stay below 2^24 units, so fp32 holds every intermediate exactly.  Then the float64 and float32 torch forwards and the
    numpy chain must agree to the bit -- three summation orders, one result."""
    desc, ws, bs, img, chain = ref.exact_case(name)
    assert set(np.unique(img)) == {0, 255}
    for w, b in zip(ws, bs):
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and np.array_equal(b, np.round(b)) and np.abs(b).max() <= 3
    rows = ref.exact_proof(desc, ws, bs, img)
    assert [r[0] for r in rows] == [r for r, _, _ in ref.conv_roles(desc)]
    for role, k, bound, whole, _, _ in rows:
        print(f"exact {name} {role}: unit 2^-{k}, largest partial sum <= 2^{np.log2(max(bound, 1)):.1f} units")
        assert whole, (name, role)
        assert bound < 2 ** 24, (name, role, bound)
    f64 = ref.forward_desc(desc, ws, bs, img, "float64")
    assert np.array_equal(chain.astype(np.float64), f64)
    assert np.array_equal(ref.forward_desc(desc, ws, bs, img, "float32"), chain)
    if desc.bilinear_base:
        assert desc.scale in (1, 2, 4)


@pytest.mark.parametrize("name", EXACT_IDS)
def test_exact_networks_cover_the_index_maps(name):
    """A zero-tolerance check sees an index only if something non-zero depends on it: every (cin mod 8, tap) pair and every cin
    chunk of every MFMA convolution (every (cin, tap) of the head) carries a weight, every cout has one, both signs reach every
    activation, at least a quarter of every layer's stored values is non-zero, and the output clamps on both sides in u8 and is
    not constant."""
    desc, ws, bs, img, chain = ref.exact_case(name)
    rows = ref.exact_proof(desc, ws, bs, img)
    for (role, cout, cin), w, (_, _, _, _, pre, st) in zip(ref.conv_roles(desc), ws, rows):
        nz = np.asarray(w).reshape(cout, cin, 9) != 0
        assert nz.any(axis=(1, 2)).all(), (name, role, "a cout without a weight")
        if cin == 3:
            assert nz.any(axis=0).all(), (name, role)
        else:
            assert nz.reshape(cout, cin // 8, 8, 9).any(axis=(0, 1)).all(), (name, role, "(cin mod 8, tap)")
            assert nz.reshape(cout, cin // 8, 72).any(axis=(0, 2)).all(), (name, role, "cin chunk")
        per = nz.sum(axis=(1, 2))
        assert per.max() <= (ref.LAST_NNZ if role == "last" else 4) and per.min() >= 1
        assert (pre < 0).any() and (pre > 0).any(), (name, role)
        assert np.mean(st != 0) >= 0.25, (name, role, float(np.mean(st != 0)))
    u8 = np.rint(np.clip(chain, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    assert chain.std() > 0 and (chain < 0).any() and (chain > 1).any() and ((chain > 0) & (chain < 1)).any()
    assert (u8 == 0).any() and (u8 == 255).any()


def test_probes_move_and_permute():
    """Every tap of a probed body convolution gives a different output, and a probe's output is the centre-tap probe's output
    shifted by the tap, with the zero padding entering at the true border only (spelled out on the last convolution)."""
    outs = {}
    for name, desc, role, tap in ref.PROBES:
        chain = ref.exact_case(name)[4]
        assert chain.std() > 0
        outs[name] = chain
    for role in ("conv1.0", "conv2.0"):                          # nine taps, nine different outputs
        body = [n for n in outs if n.startswith(role)]
        assert len(body) == 9
        for i, a in enumerate(body):
            for b in body[i + 1:]:
                assert not np.array_equal(outs[a], outs[b]), (a, b)
    # the last convolution at tap 7 (dy 2, dx 1) against the same probe at the centre: row Y of one is row Y + 1 of the other,
    # and the last row reads the zero padding below the image
    name, desc, role, tap = ref.PROBES[-1]
    assert (role, tap) == ("last", 7)
    _, ws, bs, img, chain = ref.exact_case(name)
    wc, _ = ref.probe_weights(desc, role, 4)
    centre = ref.chain_forward_desc(desc, wc, bs, img)
    base = ref.chain_forward_desc(desc, [np.zeros_like(w) for w in ws], bs, img)     # mean + bilinear base alone
    assert np.array_equal(chain[:-1] - base[:-1], centre[1:] - base[1:])
    assert np.array_equal(chain[-1], base[-1]) and not np.array_equal(centre[-1], base[-1])
