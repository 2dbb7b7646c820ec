"""Host side of the HAT backend (no GPU): the description read off a state dict's shapes for the HAT, HAT-S and HAT-L layouts,
every refusal by key name, both relative-position indices against the restatement (tests/_hat_ref.py), a file index with
negative values and a wrong relative_position_index_SA under the bare top-level keys HAT registers them with (and nested), the
mutants of the restatement that the GPU cases must see, the plan, and load_network's dispatch -- a HAT state carries SwinIR's key
too and must reach HATSRNet, a SwinIR state still SwinIRSRNet."""
import numpy as np
import pytest

import _hat_ref as ref
import _swinir_ref as swref


def _layout_state(C, heads, hidden, mid, sq, L, D, scale):
    """Zero arrays of the right shapes under HAT's key names: enough for the parser, cheap at HAT's real sizes."""
    st = {}
    for name, (ws, bs) in zip(ref.table_names(L, D, scale), ref.table_shapes(C, heads, hidden, mid, sq, L, D, scale)):
        if bs is None:
            st[name] = np.zeros(ws, np.float32)
        else:
            st[f"{name}.weight"] = np.zeros(ws, np.float32)
            st[f"{name}.bias"] = np.zeros(bs, np.float32)
    return st


@pytest.mark.parametrize("dims", [(180, 6, 360, 60, 6, 6, 6, 4), (144, 6, 288, 6, 6, 6, 6, 2), (180, 6, 360, 60, 6, 12, 6, 3)],
                         ids=["HAT", "HAT-S", "HAT-L"])
def test_description_is_read_off_the_shapes(dims):
    import _native
    import sr_network
    desc, ws, bs, rpi = sr_network.parse_hat_state(_layout_state(*dims))
    got = (desc.n_feat, desc.n_heads, desc.n_hidden, desc.n_mid, desc.n_squeeze, desc.n_groups, desc.depth, desc.scale)
    assert got == dims
    assert desc.conv_scale == np.float32(0.01) and desc.range == 1.0 and tuple(desc.mean) == tuple(np.float32(sr_network.HAT_RGB_MEAN))
    assert rpi is None
    names, shapes = _native.hat_table_names(desc), _native.hat_table_shapes(desc)
    L, D = dims[5], dims[6]
    assert len(ws) == len(bs) == len(names) == len(shapes) == 2 + L * (11 * D + 8) + 2 + (4 if dims[7] == 4 else 3)
    assert names == ref.table_names(L, D, dims[7])
    for w, b, (sw, sb) in zip(ws, bs, shapes):
        assert w.shape == sw and w.dtype == np.float32 and w.flags.c_contiguous
        assert (b is None) == (sb is None) and (b is None or b.shape == sb)


def test_synthetic_state_and_extras():
    import sr_network
    st = ref.synthetic_state(60, 6, 120, 20, 2, 2, 2, 3)
    desc, ws, bs, rpi = sr_network.parse_hat_state(st, **sr_network._hat_extras(st))
    assert desc.range == np.float32(ref.IMG_RANGE) and desc.conv_scale == np.float32(ref.CONV_SCALE) and desc.scale == 3
    assert rpi is None
    names = ref.table_names(2, 2, 3)
    for n, w, b in zip(names, ws, bs):
        key = n if n.endswith("bias_table") else f"{n}.weight"
        assert np.array_equal(w.reshape(np.shape(st[key])), st[key]), n
        assert b is None or np.array_equal(b, st[f"{n}.bias"]), n


def _refused(st, match, exc=ValueError):
    import sr_network
    with pytest.raises(exc, match=match):
        sr_network.parse_hat_state(st)


def test_every_refusal_names_its_key():
    base = ref.synthetic_state(60, 6, 120, 20, 2, 1, 2, 2)
    b0, oc = "layers.0.residual_group.blocks.0", "layers.0.residual_group.overlap_attn"

    def without(*keys):
        return {k: v for k, v in base.items() if k not in keys}

    def with_(**kv):
        return {**base, **kv}

    _refused(without(f"{oc}.qkv.weight"), "not a HAT")
    _refused(with_(absolute_pos_embed=np.zeros((1, 4, 60), np.float32)), "absolute_pos_embed")
    _refused(without("layers.0.conv.weight"), r"layers\.0\.conv\.weight.*identity")
    _refused(with_(**{"layers.0.conv.0.weight": np.zeros((15, 60, 3, 3), np.float32)}), r"layers\.0\.conv\.0\.weight")
    _refused(with_(**{f"{b0}.attn.relative_position_bias_table": np.zeros((225, 6), np.float32)}), r"attn\.relative_position_bias_table.*window_size 16")
    _refused(with_(**{f"{oc}.relative_position_bias_table": np.zeros((37 * 37, 6), np.float32)}), r"overlap_attn\.relative_position_bias_table.*overlap")
    _refused(with_(**{f"layers.0.residual_group.blocks.1.attn.relative_position_bias_table": np.zeros((961, 3), np.float32)}), r"blocks\.1\.attn.*heads")
    _refused(with_(**{f"{b0}.attn.qkv.weight": np.zeros((180, 61), np.float32)}), r"blocks\.0\.attn\.qkv\.weight")
    _refused(with_(**{f"{b0}.conv_block.cab.2.weight": np.zeros((60, 21, 3, 3), np.float32)}), r"conv_block\.cab\.2\.weight")
    _refused(with_(**{f"{b0}.conv_block.cab.3.attention.3.weight": np.zeros((60, 3, 1, 1), np.float32)}), r"cab\.3\.attention\.3\.weight")
    _refused(without(f"{b0}.conv_block.cab.3.attention.1.bias"), r"cab\.3\.attention\.1\.bias")
    _refused(without(f"{oc}.mlp.fc2.bias"), r"overlap_attn\.mlp\.fc2\.bias")
    _refused(with_(**{f"{b0}.norm1.weight": np.zeros(60, np.float16)}), r"norm1\.weight.*float16")
    _refused(with_(**{"conv_up1.weight": np.zeros((64, 64, 3, 3), np.float32)}), "conv_up1")
    _refused(without("conv_before_upsample.0.weight", "conv_before_upsample.0.bias"), r"conv_before_upsample\.0\.weight")
    _refused(without("upsample.0.weight", "upsample.0.bias"), r"upsample\.0\.weight")
    x8 = with_(**{f"upsample.{k}.weight": base["upsample.0.weight"] for k in (2, 4)}, **{f"upsample.{k}.bias": base["upsample.0.bias"] for k in (2, 4)})
    _refused(x8, r"upsample\.0\.weight.*3 stage")
    two = ref.synthetic_state(60, 6, 120, 20, 2, 2, 2, 2)
    _refused({k: v for k, v in two.items() if not k.startswith("layers.1.residual_group.blocks.1.")}, "same depth")
    _refused({k.replace("layers.1.", "layers.2."): v for k, v in two.items()}, r"layers\.1\.conv\.weight")
    # what only the kernels' ranges exclude: C 264 (heads of 33 channels)
    _refused(_layout_state(264, 8, 528, 20, 2, 1, 1, 2), "embed_dim", NotImplementedError)
    _refused(_layout_state(132, 4, 264, 20, 2, 1, 1, 2), "num_heads", NotImplementedError)


def test_window_index_and_a_wrong_index_sa():
    import _native
    import sr_network
    rel = _native.hat_rel_index()
    assert rel.shape == (256, 256) and np.array_equal(rel, ref.rel_index())
    i, j = 3 * 16 + 5, 14 * 16 + 9
    assert rel[i, j] == (3 - 14 + 15) * 31 + (5 - 9 + 15)
    st = ref.synthetic_state(60, 6, 120, 20, 2, 1, 2, 2)
    nested = "layers.0.residual_group.blocks.1.attn.relative_position_index_SA"
    assert ref.SA_KEY in st                                                  # the bare top-level key, as HAT registers it
    sr_network.parse_hat_state(st)                                          # the correct buffer passes
    sr_network.parse_hat_state({**st, nested: st[ref.SA_KEY]})              # and so does a nested copy
    for key in (ref.SA_KEY, nested, "some.other.place.relative_position_index_SA"):
        for wrong in (st[ref.SA_KEY].T.copy(), np.zeros((64, 64), np.int64)):
            with pytest.raises(ValueError, match=key.replace(".", r"\.") + ": differs"):
                sr_network.parse_hat_state({**st, key: wrong})              # never ignored, wherever it sits


def test_oca_index_default_and_from_the_file():
    import _native
    import sr_network
    idx = _native.hat_oca_index()
    raw = ref.oca_index_raw()
    assert idx.shape == (256, 576) and np.array_equal(idx, ref.oca_index())
    assert raw.min() == -22 * 39 - 22 and raw.max() == 16 * 39 + 16 and (raw < 0).any()
    assert idx.min() >= 0 and idx.max() < 1521
    table = np.arange(1521)
    assert np.array_equal(table[raw], idx)                                   # numpy wraps a negative index as torch does
    q, k = 2 * 16 + 3, 20 * 24 + 11
    assert raw[q, k] == (20 - 2 - 7) * 39 + (11 - 3 - 7)
    # a file's top-level buffer with negative values is accepted, handed on as it is (the library wraps) and used instead of
    # the formula
    st = ref.synthetic_state(60, 6, 120, 20, 2, 2, 1, 2, file_index=True)
    assert ref.OCA_KEY in st and (st[ref.OCA_KEY] < 0).any()
    rpi = sr_network.parse_hat_state(st)[3]
    assert rpi.dtype == np.int32 and np.array_equal(rpi, raw) and (rpi < 0).any()
    other = (raw[::-1] % 1521).copy()
    assert np.array_equal(sr_network.parse_hat_state({**st, ref.OCA_KEY: other})[3], other)
    # the nested form is read the same way, alone or beside the top-level one
    n0, n1 = (f"layers.{g}.residual_group.overlap_attn.relative_position_index_OCA" for g in (0, 1))
    bare = {k: v for k, v in st.items() if k != ref.OCA_KEY}
    assert sr_network.parse_hat_state(bare)[3] is None
    assert np.array_equal(sr_network.parse_hat_state({**bare, n0: other, n1: other})[3], other)
    assert np.array_equal(sr_network.parse_hat_state({**st, n1: raw})[3], raw)
    for key in (ref.OCA_KEY, n1):
        for wrong, match in ((np.full((256, 576), 1521), r"relative_position_index_OCA.*\[-1521, 1520\]"),
                             (np.full((256, 576), -1522), "relative_position_index_OCA"), (np.zeros((576, 256), np.int64), r"\(256, 576\)"),
                             (np.zeros((256, 576), np.float32), "integer")):
            with pytest.raises(ValueError, match=match):
                sr_network.parse_hat_state({**bare, key: wrong})
    with pytest.raises(ValueError, match=r"relative_position_index_OCA: differs from layers\.1\."):
        sr_network.parse_hat_state({**st, n1: other})                        # two copies disagree (sorted: the nested one first)
    with pytest.raises(ValueError, match=r"layers\.1\..*relative_position_index_OCA: differs"):
        sr_network.parse_hat_state({**bare, n0: raw, n1: other})
    with pytest.raises(ValueError):
        _native.hat_oca(None, 256, 64, 16, 4, 1, 16, 16, np.zeros((1521, 1)), np.full((256, 576), 1521), 256, 64, 16)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_exceeds_the_bar(mutant):
    """What the GPU cases can see: each wrong forward misses the float64 restatement by more than the bar of
    tests/test_gpu_hat.py, 8 e32, on at least one of its cases."""
    worst = 0.0
    for case in (ref.CASES[0], ref.CASES[4]):
        state, img, f64, e32 = ref.case(*case)
        diff = float(np.max(np.abs(ref.forward(state, img, "float64", mutant) - f64)))
        print(f"hat mutant {mutant} on {ref.case_id(case)}: diff {diff:.3e}  diff / (8 e32) {diff / (8 * e32):.1f}")
        worst = max(worst, diff / (8 * e32))
        if worst > 1:
            break
    assert worst > 1, (mutant, worst)


def test_reflection_without_the_edge_pixel():
    for n, total in ((19, 32), (37, 48), (9, 16), (2, 16)):
        want = np.pad(np.arange(n), (0, total - n), mode="reflect")
        assert np.array_equal(ref.reflect_index(n, total), want), (n, total)
    assert np.array_equal(ref.reflect_index(1, 16), np.zeros(16))
    assert not np.array_equal(ref.reflect_index(19, 32), ref.reflect_index(19, 32, symmetric=True))


@pytest.mark.parametrize("dims,h,w", [((60, 6, 120, 20, 2, 2, 2, 2), 19, 37), ((180, 6, 360, 60, 6, 6, 6, 4), 512, 512),
                                      ((144, 6, 288, 6, 6, 1, 2, 3), 16, 16), ((60, 6, 120, 20, 2, 1, 2, 2), 1, 21)])
def test_plan(dims, h, w):
    import _native
    desc = _native.hat_desc(*dims)
    for tail in (0, 1, 7, 64) if h * w < 4000 else (0, 64, 300):
        assert _native.hat_plan(desc, h, w, tail) == ref.plan(dims[0], dims[2], dims[3], dims[7], h, w, tail), tail


def test_plan_refusals():
    import _native
    assert ref.bytes_per_pixel(180, 360, 60) == 6400                         # the figure the header states
    desc = _native.hat_desc(180, 6, 360, 60, 6, 6, 6, 4)
    fit = ref.TRUNK_CAP // 6400
    assert _native.hat_plan(desc, 2048, 2048)[:2] == (2048, 2048)
    with pytest.raises(ValueError, match=rf"SR_HAT_TRUNK_CAP = 32 GiB.*{fit} pixels"):
        _native.hat_plan(desc, 2400, 2400)
    with pytest.raises(ValueError):
        _native.hat_plan(desc, 0, 5)
    with pytest.raises(ValueError):
        _native.hat_plan(desc, 5, 5, -1)
    for bad in ((180, 6, 360, 0, 6, 6, 6, 4), (180, 6, 360, 181, 6, 6, 6, 4), (180, 6, 360, 60, 0, 6, 6, 4), (180, 6, 360, 60, 6, 13, 6, 4),
                (180, 6, 360, 60, 6, 6, 13, 4), (180, 6, 360, 60, 6, 6, 6, 1), (180, 6, 360, 60, 6, 6, 6, 8), (180, 5, 360, 60, 6, 6, 6, 4),
                (182, 7, 360, 60, 6, 6, 6, 4), (180, 6, 721, 60, 6, 6, 6, 4)):
        with pytest.raises(NotImplementedError):
            _native.hat_plan(_native.hat_desc(*bad), 16, 16)
    with pytest.raises(NotImplementedError):
        _native.hat_plan(_native.hat_desc(180, 6, 360, 60, 6, 6, 6, 4, conv_scale=float("nan")), 16, 16)
    with pytest.raises(NotImplementedError):
        _native.hat_attention(None, 256, 4 * 256 * 16, 64, 4, 1, 16, 16, 4, np.zeros((961, 1)), 256, 4 * 256 * 16, 64)      # shift 4
    with pytest.raises(ValueError):
        _native.hat_attention(None, 256, 4 * 256 * 16, 64, 4, 1, 16, 24, 0, np.zeros((961, 1)), 256, 4 * 256 * 16, 96)      # 24 columns
    with pytest.raises(ValueError):
        _native.hat_oca(None, 256, 4 * 256 * 16, 64, 4, 1, 16, 16, np.zeros((961, 1)), None, 256, 4 * 256 * 16, 64)         # the wrong table


def test_load_network_dispatches_a_hat_state_to_hat(tmp_path):
    """A HAT state holds ``layers.0.residual_group.blocks.0.attn.qkv.weight`` too: it must not reach the SwinIR parser."""
    import sr_network
    st = ref.synthetic_state(60, 6, 120, 20, 2, 1, 2, 2)
    assert sr_network.SWINIR_KEY in st and sr_network.HAT_KEY in st
    path = str(tmp_path / "hat.npz")
    np.savez(path, **st)
    net = sr_network.load_network(path)
    assert isinstance(net, sr_network.HATSRNet) and net.scale == 2
    assert net.desc.range == np.float32(ref.IMG_RANGE) and net.desc.conv_scale == np.float32(ref.CONV_SCALE)
    assert (net.n_feat, net.n_heads, net.n_hidden, net.n_groups, net.depth) == (60, 6, 120, 1, 2)
    with pytest.raises(ValueError, match="no tile"):
        net.upscale_device(0, (4, 4, 3), 0, 24, tile=8)


def test_load_network_still_dispatches_swinir(tmp_path):
    import sr_network
    st = swref.synthetic_state(60, 6, 120, 1, 2, 2, "pixelshuffle")
    assert sr_network.HAT_KEY not in st
    path = str(tmp_path / "swinir.npz")
    np.savez(path, **st)
    net = sr_network.load_network(path)
    assert type(net) is sr_network.SwinIRSRNet and net.scale == 2
