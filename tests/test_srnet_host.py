"""CPU: the host side of the local SR backend -- sr_srnet_plan (no context, no GPU), the state-dict parser of
sr_network.CompactSRNet, the .npz loader and the pipeline's configuration rules.  No device call is made here."""
import numpy as np
import pytest

import _native
import _srnet_ref as ref
import main as sr_main
import sr_network


def _ws(F, D, rows, cols, halo):
    r, c = rows, (cols + 3) // 4 * 4
    return 2 * F * r * c * 4


def test_plan_halo_tiles_workspace():
    # one sub-tile: the padded sub-tile is the whole image
    assert _native.srnet_plan(150, 210, 64, 16, 2, 256) == (18, 1, _ws(64, 16, 150, 210, 18))
    # four sub-tiles of 160: min(tile, side) + 2 halo, clipped to the image
    halo, n, ws = _native.srnet_plan(150, 210, 64, 16, 2, 160)
    assert (halo, n) == (18, 1 * 2) and ws == _ws(64, 16, 150, min(160 + 36, 210), 18)
    halo, n, ws = _native.srnet_plan(300, 210, 64, 16, 2, 160)
    assert (halo, n) == (18, 2 * 2)
    halo, n, ws = _native.srnet_plan(150, 210, 128, 3, 3, 32)
    assert (halo, n) == (5, 5 * 7) and ws == _ws(128, 3, 42, 42, 5)
    # tile 0: the library's choice (2048) -- one sub-tile for a pipeline tile of 2048
    halo, n, ws = _native.srnet_plan(2048, 2048, 64, 32, 4, 0)
    assert (halo, n) == (34, 1) and ws == 2 * 64 * 2048 * 2048 * 4
    assert _native.srnet_plan(4096, 2049, 64, 0, 1, 0)[:2] == (2, 2 * 2)
    assert _native.srnet_plan(1, 1, 256, 64, 4, 1) == (66, 1, 2 * 256 * 1 * 4 * 4)


def test_plan_refusals():
    for F, D, s in ((48, 16, 2), (64, 65, 2), (64, 16, 5), (64, -1, 2), (64, 16, 0), (320, 1, 2)):
        with pytest.raises(NotImplementedError):
            _native.srnet_plan(100, 100, F, D, s, 0)
    with pytest.raises(ValueError):
        _native.srnet_plan(100, 100, 64, 16, 2, -1)
    with pytest.raises(ValueError):
        _native.srnet_plan(0, 100, 64, 16, 2, 0)
    with pytest.raises(ValueError):
        _native.srnet_plan(100, 0, 64, 16, 2, 0)
    with pytest.raises(ValueError):                              # (h s) x (w s x 3) must fit int
        _native.srnet_plan(100, 200_000_000, 64, 16, 4, 64)
    with pytest.raises(ValueError):                              # a sub-tile beyond the kernels' 32-bit offsets
        _native.srnet_plan(30000, 30000, 64, 2, 2, 30000)


def test_parse_prelu_state():
    st = ref.synthetic_state(64, 3, 2)
    net = sr_network.CompactSRNet(st)
    assert (net.n_feat, net.n_body, net.scale) == (64, 3, 2)
    F, D, s, w, b, sl = sr_network.parse_state(st)
    assert len(w) == len(b) == 5 and len(sl) == 4
    assert w[0].shape == (64, 3, 3, 3) and w[-1].shape == (12, 64, 3, 3) and all(x.dtype == np.float32 for x in w + b + sl)
    for k in range(4):
        assert np.array_equal(sl[k], st[f"body.{2 * k + 1}.weight"]) and np.array_equal(w[k], st[f"body.{2 * k}.weight"])
    assert (sr_network.CompactSRNet(ref.synthetic_state(128, 0, 3)).scale, sr_network.CompactSRNet(ref.synthetic_state(64, 1, 4)).scale) == (3, 4)
    assert sr_network.CompactSRNet(ref.synthetic_state(64, 1, 1)).scale == 1


def test_parse_relu_leaky_and_broadcast():
    st = ref.synthetic_state(64, 2, 2)
    plain = {k: v for k, v in st.items() if np.asarray(v).ndim != 1 or k.endswith("bias")}       # no PReLU entries
    assert len(plain) == len(st) - 3
    for act, slope in (("relu", 0.0), ("leakyrelu", 0.1)):
        sl = sr_network.parse_state(plain, act)[5]
        assert len(sl) == 3 and all(np.array_equal(x, np.full(64, slope, np.float32)) for x in sl)
    with pytest.raises(ValueError):
        sr_network.parse_state(plain, "prelu")                   # nothing to take the slopes from
    with pytest.raises(ValueError):
        sr_network.parse_state(plain, "gelu")
    one = dict(st)
    one["body.1.weight"] = np.array([0.25], np.float32)          # nn.PReLU() with one shared slope
    sl = sr_network.parse_state(one, "relu")[5]
    assert np.array_equal(sl[0], np.full(64, 0.25, np.float32)) and np.array_equal(sl[1], st["body.3.weight"])
    # consecutive convolutions without activation modules between them (indices 0, 1, 2, 3)
    dense = {}
    for k in range(4):
        dense[f"body.{k}.weight"], dense[f"body.{k}.bias"] = st[f"body.{2 * k}.weight"], st[f"body.{2 * k}.bias"]
    F, D, s, w, b, sl = sr_network.parse_state(dense, "leakyrelu")
    assert (F, D, s) == (64, 2, 2) and all(np.all(x == np.float32(0.1)) for x in sl)


def test_parse_wrappers_and_errors():
    st = ref.synthetic_state(64, 1, 2)
    for key in ("params_ema", "params"):
        assert sr_network.CompactSRNet({key: st}).n_body == 1
    bad = dict(st)
    bad["body.4.weight"] = np.zeros((10, 64, 3, 3), np.float32)  # 10 is not 3 s^2
    bad["body.4.bias"] = np.zeros(10, np.float32)
    with pytest.raises(ValueError, match="3 s\\^2"):
        sr_network.CompactSRNet(bad)
    chain = dict(st)
    chain["body.2.weight"] = np.zeros((64, 32, 3, 3), np.float32)
    with pytest.raises(ValueError, match="channels"):
        sr_network.CompactSRNet(chain)
    with pytest.raises(ValueError):
        sr_network.CompactSRNet({"body.0.weight": st["body.0.weight"], "body.0.bias": st["body.0.bias"]})
    with pytest.raises(NotImplementedError):                     # F = 48 chains but is outside the kernels' range
        s48 = ref.synthetic_state(48, 1, 2)
        sr_network.CompactSRNet(s48)
    with pytest.raises(NotImplementedError):
        sr_network.CompactSRNet(ref.synthetic_state(64, 1, 5))
    with pytest.raises(NotImplementedError):
        _native.SrNetModel(None, 64, 65, 2, [], [], [])          # refused before the context is looked at


def test_npz_round_trip(tmp_path):
    st = ref.synthetic_state(64, 2, 2)
    path = tmp_path / "net.npz"
    np.savez(path, **st)
    net = sr_network.CompactSRNet.from_file(str(path))
    a, b = sr_network.parse_state(st), (net.n_feat, net.n_body, net.scale, net._w, net._b, net._s)
    assert a[:3] == b[:3]
    for x, y in zip(a[3] + a[4] + a[5], b[3] + b[4] + b[5]):
        assert np.array_equal(x, y)


def test_pth_loader_unwraps_params_ema(tmp_path):
    torch = pytest.importorskip("torch")
    st = ref.synthetic_state(64, 1, 3)
    path = tmp_path / "net.pth"
    torch.save({"params_ema": {k: torch.from_numpy(v) for k, v in st.items()}}, str(path))
    net = sr_network.CompactSRNet.from_file(str(path))
    assert (net.n_feat, net.n_body, net.scale) == (64, 1, 3) and np.array_equal(net._w[1], st["body.2.weight"])


@pytest.mark.parametrize("F,D,s,h,w", ref.CASES + ref.EDGE_CASES)
def test_documented_summation_order_stays_inside_the_gpu_bar(F, D, s, h, w):
    """The accuracy bar of tests/test_gpu_srnet.py, err <= 8 e32, held against the kernel's documented summation order
    restated in numpy fp32 (ref.chain_forward): the order alone must fit the bar, or the bar says nothing about the kernel.
    Measured e_chain / e32 on the eight CASES: 1.46, 2.17, 2.76, 1.30, 1.72, 4.41 (F = 192), 5.07 (F = 256), 2.63; the ratio
    grows with F.  The exempt share of the u8 check stays 0.05 % ... 0.15 % against its 1 % cap."""
    state, img, f64, e32 = ref.case(F, D, s, h, w)
    chain, e_chain = ref.chain_case(F, D, s, h, w)
    assert chain.dtype == np.float32 and chain.shape == f64.shape == (h * s, w * s, 3)
    f32 = ref.forward(state, img, "float32")
    d = float(np.max(np.abs(chain.astype(np.float64) - f32.astype(np.float64))))
    print(f"srnet chain F={F} D={D} s={s} {h}x{w}: e32 {e32:.3e}  e_chain {e_chain:.3e}  ratio {e_chain / e32:.3f}  |chain - f32| / e32 {d / e32:.3f}")
    assert e32 > 0
    assert d <= 8 * e32, (d, e32)                                # 1: the two float32 statements agree
    assert e_chain <= 8 * e32, (e_chain, e32, e_chain / e32)     # 2: the documented order alone is inside the GPU bar
    share = ref.check_u8(ref.quantize(chain), f64, e32)          # 3: ... and inside the u8 check with its 1 % exempt cap
    print(f"  u8 of the chain: exempt share {share:.4%}")


def test_chain_forward_spells_out_shuffle_and_slopes():
    """chain_forward on hand-made states: zero weights give the nearest upsample exactly; a tail bias k / 256 on a black image
    gives out[Y, X, c] = (c s^2 + (Y % s) s + (X % s)) / 256; default_slope reaches layers without slope entries."""
    img = ref.make_image(5, 7, seed=3)
    for s in (1, 2, 3, 4):
        st = {k: np.zeros_like(v) for k, v in ref.synthetic_state(64, 1, s).items()}
        x = img.astype(np.float32) / np.float32(255.0)
        assert np.array_equal(ref.chain_forward(st, img), np.repeat(np.repeat(x, s, axis=0), s, axis=1))
        st["body.4.bias"] = (np.arange(3 * s * s) / 256.0).astype(np.float32)
        out = ref.chain_forward(st, np.zeros((3, 4, 3), np.uint8))
        Y, X, c = np.meshgrid(np.arange(3 * s), np.arange(4 * s), np.arange(3), indexing="ij")
        assert np.array_equal(out, ((c * s * s + (Y % s) * s + (X % s)) / 256.0).astype(np.float32))
    st = ref.synthetic_state(64, 1, 2)
    plain = {k: v for k, v in st.items() if np.asarray(v).ndim != 1 or k.endswith("bias")}
    for slope in (0.0, 0.1):
        f64 = ref.forward(plain, img, "float64", default_slope=slope)
        assert np.max(np.abs(ref.chain_forward(plain, img, default_slope=slope) - f64)) < 1e-5
    assert np.max(np.abs(ref.forward(plain, img, "float64", 0.0) - ref.forward(plain, img, "float64", 0.1))) > 1e-3


def test_pipeline_config_and_scale_mismatch(tmp_path):
    c = sr_main.PipelineConfig()
    assert c.sr_weights == "" and c.sr_act == "prelu" and c.sr_scale == 2 and c.device_resident is True
    plain = sr_main.SuperResolutionPipeline(c)
    assert plain.sr_backend is sr_main.bicubic_stub_backend and plain.sr_net is None
    path = tmp_path / "x4.npz"
    np.savez(path, **ref.synthetic_state(64, 1, 4))
    with pytest.raises(ValueError, match="sr_scale"):            # no device is touched: this passes without a GPU
        sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=2))
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=4, block_size=64))
    assert pipe.sr_backend is sr_main.compact_net_backend and pipe.sr_net.scale == 4 and pipe._builtin_backend()
    # an explicit backend wins over sr_weights
    custom = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path)), sr_backend=lambda p, t, s: None)
    assert custom.sr_net is None and not custom._builtin_backend()
