"""Host side of the SwinIR backend (no GPU): the state-dict parser on every variant and every refusal by key, the plan against
its restatement, load_network's dispatch, the relative-position index of the C side, and the restatement itself -- the
documented-order numpy forward lies inside the float bar (8 x the error of torch's own float32 forward against float64), and
the mutants a wrong kernel would compute miss it, so the GPU cases can see them.

PARITY UNPINNED: neither BasicSR nor the official SwinIR repository nor a checkpoint exists offline (tests/_swinir_ref.py)."""
import numpy as np
import pytest

import _swinir_ref as ref

SMALL = (60, 6, 120, 1, 2, 2, "pixelshuffledirect")
VARIANTS = [(60, 6, 120, 2, 2, 2, "pixelshuffledirect"), (64, 2, 128, 1, 2, 4, "pixelshuffle"), (180, 6, 360, 1, 2, 3, "pixelshuffle"),
            (64, 4, 256, 2, 3, 4, "nearest+conv"), (60, 6, 120, 1, 2, 1, "pixelshuffledirect"), (96, 6, 192, 1, 1, 2, "pixelshuffle"),
            (60, 6, 120, 1, 2, 3, "pixelshuffledirect"), (60, 6, 120, 1, 2, 4, "pixelshuffledirect")]


@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: "-".join(map(str, v)))
def test_parser_reads_the_description_off_the_shapes(v):
    import _native
    import sr_network
    C, heads, hidden, L, D, s, up = v
    state = ref.synthetic_state(*v)
    desc, ws, bs = sr_network.parse_swinir_state(state, img_range=3.0, rgb_mean=(0.1, 0.2, 0.3))
    assert (desc.n_feat, desc.n_heads, desc.n_hidden, desc.n_groups, desc.depth, desc.scale) == (C, heads, hidden, L, D, s)
    assert desc.upsampler == _native.SWINIR_UPSAMPLERS[up] and desc.range == 3.0 and list(desc.mean) == [np.float32(x) for x in (0.1, 0.2, 0.3)]
    assert _native.swinir_table_names(desc) == ref.table_names(L, D, s, up)
    assert _native.swinir_table_shapes(desc) == ref.table_shapes(C, heads, hidden, L, D, s, up)
    want_w, want_b = ref.arrays(state)
    assert len(ws) == len(want_w) == len(bs)
    for k, (w, b, ww, wb) in enumerate(zip(ws, bs, want_w, want_b)):
        assert w.dtype == np.float32 and w.flags.c_contiguous and np.array_equal(w, ww), k
        assert (b is None and wb is None) or np.array_equal(b, wb), k
    assert sum(b is None for b in bs) == L * D                    # the bias tables; the two ignored buffers are not tables


def _refused(state, key_part, exc=ValueError):
    import sr_network
    with pytest.raises(exc) as e:
        sr_network.parse_swinir_state(state)
    assert key_part in str(e.value), str(e.value)


def test_parser_refuses_by_key():
    b0 = "layers.0.residual_group.blocks.0"
    base = ref.synthetic_state(60, 6, 120, 2, 2, 2, "pixelshuffle")

    def variant(**changes):
        st = dict(base)
        for k, v in changes.items():
            if v is None:
                st.pop(k)
            else:
                st[k] = v
        return st

    z = np.zeros
    _refused(variant(**{"layers.0.conv.0.weight": z((15, 60, 3, 3), np.float32)}), "layers.0.conv.0.weight")          # 3conv
    _refused(variant(absolute_pos_embed=z((1, 64, 60), np.float32)), "absolute_pos_embed")
    st = {k: (z((169, 6), np.float32) if k.endswith("bias_table") else v) for k, v in base.items()}                   # window 7
    _refused(st, f"{b0}.attn.relative_position_bias_table")
    _refused(variant(**{"layers.1.residual_group.blocks.1.attn.relative_position_bias_table": z((169, 6), np.float32)}),
             "layers.1.residual_group.blocks.1.attn.relative_position_bias_table")
    st = {k: v for k, v in base.items() if not k.startswith(("conv_before_upsample", "upsample"))}                   # denoising / JPEG
    _refused(st, "conv_last.weight")
    _refused(variant(**{f"{b0}.attn.logit_scale": z((6, 1, 1), np.float32)}), f"{b0}.attn.logit_scale")                 # Swin2SR
    _refused(variant(**{f"{b0}.attn.qkv.weight": base[f"{b0}.attn.qkv.weight"].astype(np.float16)}), f"{b0}.attn.qkv.weight")
    st = {k: v for k, v in base.items() if not k.startswith("layers.1.residual_group.blocks.1.")}                     # unequal depths
    _refused(st, "layers.1.residual_group.blocks.1.attn.qkv.weight")
    _refused(variant(**{"layers.1.residual_group.blocks.0.attn.relative_position_bias_table": z((225, 3), np.float32)}),  # unequal heads
             "layers.1.residual_group.blocks.0.attn.relative_position_bias_table")
    st = {k: v for k, v in base.items() if not k.startswith("layers.0.")}                                             # RSTBs 1 .. only
    _refused(st, "layers.0.residual_group.blocks.0.attn.qkv.weight")
    _refused(variant(**{f"{b0}.norm2.bias": None}), f"{b0}.norm2.bias")
    _refused(variant(**{f"{b0}.mlp.fc2.weight": z((60, 121), np.float32)}), f"{b0}.mlp.fc2.weight")
    _refused(variant(**{"layers.1.conv.weight": z((60, 60, 1, 1), np.float32)}), "layers.1.conv.weight")
    _refused(variant(**{"upsample.0.weight": z((128, 64, 3, 3), np.float32)}), "upsample.0.weight")
    _refused({k: v for k, v in base.items() if k != "upsample.0.weight" and k != "upsample.0.bias"}, "upsample.0.weight")
    _refused({"conv_first.weight": base["conv_first.weight"]}, "layers.0.residual_group.blocks.0.attn.qkv.weight")


def test_ranges_are_refused_by_name():
    """What only the kernels' ranges exclude is SR_ERR_UNSUPPORTED from the host-only plan call."""
    import _native
    for args, word in [((260, 10, 520, 1, 2, 2), "embed_dim"), ((62, 2, 124, 1, 2, 2), "embed_dim"), ((132, 4, 264, 1, 2, 2), "num_heads"),
                       ((60, 7, 120, 1, 2, 2), "num_heads"), ((60, 6, 241, 1, 2, 2), "hidden"), ((60, 6, 120, 13, 2, 2), "RSTBs"),
                       ((60, 6, 120, 1, 13, 2), "RSTBs"), ((60, 6, 120, 1, 2, 5), "scale")]:
        with pytest.raises(NotImplementedError, match=word):
            _native.swinir_plan(_native.swinir_desc(*args), 8, 8)
    for up, s in [("pixelshuffle", 1), ("nearest+conv", 2), ("pixelshuffledirect", 0), (3, 2)]:
        with pytest.raises(NotImplementedError, match="upsampler"):
            _native.swinir_plan(_native.swinir_desc(60, 6, 120, 1, 2, s, up), 8, 8)
    with pytest.raises(NotImplementedError, match="range"):
        _native.swinir_plan(_native.swinir_desc(60, 6, 120, 1, 2, 2, range=0.0), 8, 8)
    with pytest.raises(NotImplementedError, match="finite"):
        _native.swinir_plan(_native.swinir_desc(60, 6, 120, 1, 2, 2, mean=(0.0, float("nan"), 0.0)), 8, 8)


@pytest.mark.parametrize("v", VARIANTS[:5], ids=lambda v: "-".join(map(str, v)))
def test_plan_matches_the_restatement(v):
    import _native
    C, heads, hidden, L, D, s, up = v
    desc = _native.swinir_desc(*v)
    for h, w in [(1, 1), (8, 8), (13, 21), (40, 70), (257, 300), (512, 512)]:
        for tail in (0, 1, 7, 64, 300):
            if tail == 1 and h * w > 3000:
                continue
            assert _native.swinir_plan(desc, h, w, tail) == ref.plan(C, hidden, s, up, h, w, tail), (h, w, tail)
    assert _native.swinir_plan(desc, 13, 21)[:2] == (16, 24)


def test_plan_refusals_and_the_trunk_cap():
    """A plan only: nothing is allocated.  The cap is a policy constant and the message names it."""
    import _native
    desc = _native.swinir_desc(180, 6, 360, 6, 6, 4)
    assert _native.swinir_plan(desc, 2048, 2048)[4] > 0           # one pipeline block fits
    assert 5376 * 2048 * 2048 <= ref.TRUNK_CAP
    with pytest.raises(ValueError, match="SR_SWINIR_TRUNK_CAP = 32 GiB.*6391320 pixels"):
        _native.swinir_plan(desc, 2600, 2600)
    for h, w, tail in [(0, 5, 0), (5, 0, 0), (5, 5, -1)]:
        with pytest.raises(ValueError):
            _native.swinir_plan(desc, h, w, tail)


def test_relative_position_index_of_the_c_side():
    import _native
    got = _native.swinir_rel_index()
    assert got.shape == (64, 64) and np.array_equal(got, ref.rel_index())
    assert got.min() == 0 and got.max() == 224 and (np.diag(got) == 112).all()


def test_load_network_dispatch(tmp_path):
    """A SwinIR state reaches SwinIRSRNet (it used to be handed to ResidualSRNet because of its conv_first.weight), with the
    .npz constants; the residual parser refuses it by name; the other families dispatch as before."""
    import _rcan_ref
    import _resnet_ref
    import sr_network
    state = ref.synthetic_state(*SMALL)
    path = str(tmp_path / "swinir.npz")
    np.savez(path, **state)
    net = sr_network.load_network(path)
    assert type(net) is sr_network.SwinIRSRNet
    assert (net.n_feat, net.n_heads, net.n_hidden, net.n_groups, net.depth, net.scale) == SMALL[:6]
    assert net.desc.range == np.float32(ref.IMG_RANGE) and list(net.desc.mean) == [np.float32(v) for v in ref.RGB_MEAN]
    plain = {k: v for k, v in state.items() if k not in ("img_range", "rgb_mean")}
    assert sr_network.SwinIRSRNet(plain).desc.range == 1.0       # SwinIR's default
    with pytest.raises(ValueError, match="SwinIR state"):
        sr_network.ResidualSRNet(state)
    with pytest.raises(ValueError, match="no tile"):
        net.upscale_device(0, (8, 8, 3), 0, 48, tile=16)
    rc = str(tmp_path / "rcan.npz")
    np.savez(rc, **_rcan_ref.synthetic_state(64, 4, 1, 1, 2))
    assert type(sr_network.load_network(rc)) is sr_network.RCANSRNet
    rn = str(tmp_path / "resnet.npz")
    np.savez(rn, **_resnet_ref.synthetic_state("edsr", 64, 1, 2))
    assert type(sr_network.load_network(rn)) is sr_network.ResidualSRNet


def test_region_counts_of_the_shifted_image():
    """The tokens of one window that share a region number 16, 32 or 64 at shift 4 (what the GPU's q = k = 0 probe averages
    over)."""
    for hp, wp in [(8, 8), (16, 24), (24, 16)]:
        m = ref.attn_mask(hp, wp)
        counts = (m == 0).sum(-1)
        assert set(np.unique(counts).tolist()) <= {16, 32, 64}
        assert (counts[-1] == 16).all()                          # the corner window: four regions of 16
        if hp > 8 and wp > 8:
            assert (counts[0] == 64).all()


@pytest.fixture(scope="module")
def small_case():
    return ref.case(*SMALL, 13, 21)


def test_documented_order_lies_inside_the_float_bar(small_case):
    state, img, f64, e32 = small_case
    chain = ref.chain_forward(state, img)
    err = float(np.max(np.abs(chain.astype(np.float64) - f64)))
    print(f"swinir chain forward: e32 {e32:.3e}  chain err {err:.3e}  ratio {err / e32:.3f}")
    assert chain.shape == (26, 42, 3) and e32 > 0
    assert err <= 8 * e32


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_mutants_miss_the_bar(small_case, mutant):
    """What a wrong kernel would compute misses 8 x e32 by a wide margin, so the bar sees it."""
    state, img, f64, e32 = small_case
    err = float(np.max(np.abs(ref.forward(state, img, "float64", mutant) - f64)))
    print(f"swinir mutant {mutant}: {err / e32:.1f} x e32")
    assert err > (20 if mutant == "tanh-gelu" else 1000) * e32


def test_numpy_pieces_match_torch():
    """np_layernorm and np_attention (float64 form) against torch's layer_norm and a softmax attention written with torch."""
    import torch
    import torch.nn.functional as Fn
    rng = np.random.default_rng(3)
    x = rng.standard_normal((20, 5, 7)).astype(np.float32) * 3 + 1
    g, b = rng.uniform(0.5, 1.5, 20).astype(np.float32), rng.standard_normal(20).astype(np.float32)
    want = Fn.layer_norm(torch.from_numpy(x).double().permute(1, 2, 0), (20,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-5)
    assert np.abs(ref.np_layernorm(x, g, b).astype(np.float64) - want.permute(2, 0, 1).numpy()).max() < 1e-6
    assert np.abs(ref.np_layernorm(x, g, b, -1) - ref.np_layernorm(x, g, b)).max() > 1e-3
    C, heads = 12, 2
    qkv = rng.standard_normal((3 * C, 16, 24)).astype(np.float32)
    table = rng.standard_normal((225, heads)).astype(np.float32)
    for shift in (0, 4):
        o64 = ref.np_attention(qkv, table, heads, shift, np.float64)
        o32 = ref.np_attention(qkv, table, heads, shift)
        assert o32.dtype == np.float32 and np.abs(o32 - o64).max() < 1e-5
        y = torch.from_numpy(qkv).double()
        if shift:
            y = torch.roll(y, (-shift, -shift), (1, 2))
        win = y.view(3, heads, C // heads, 2, 8, 3, 8).permute(0, 3, 5, 1, 4, 6, 2).reshape(3, 6, heads, 64, C // heads)
        a = win[0] @ win[1].transpose(-2, -1) + torch.from_numpy(table).double()[torch.from_numpy(ref.rel_index().reshape(-1))].view(64, 64, heads).permute(2, 0, 1)
        if shift:
            a = a + torch.from_numpy(ref.attn_mask(16, 24))[:, None]
        o = (Fn.softmax(a, -1) @ win[2]).view(2, 3, heads, 8, 8, C // heads).permute(2, 5, 0, 3, 1, 4).reshape(C, 16, 24)
        if shift:
            o = torch.roll(o, (shift, shift), (1, 2))
        assert np.abs(o.numpy() - o64).max() < 1e-12
