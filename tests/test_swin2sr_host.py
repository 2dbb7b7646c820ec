"""CPU: the host side of the Swin2SR backend -- the restatement against the package's stored outputs, the parser on both key
layouts, the plan, the continuous position bias and the logit scale of csrc/sr_swin2sr_host.cpp, every refusal before a device
call, the order in which load_network tells the families apart."""
import math
import os

import numpy as np
import pytest

import _swin2sr_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"swin2sr_direct_x2.npz": ("pixelshuffledirect", [(8, 8), (16, 24)]), "swin2sr_shuffle_x2.npz": ("pixelshuffle", [(16, 24)])}


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def fixture(request):
    return (request.param,) + ref.load_golden(os.path.join(GOLDEN, request.param))


def test_restatement_equals_the_package_at_1e_9(fixture):
    """The float64 restatement on the stored fp32 weights and u8 inputs against the float64 `reconstruction` the package gave:
    1e-9 is six orders below e32 and three above float64 rounding through about 30 layers."""
    name, state, cases = fixture
    up, sizes = FIXTURES[name]
    assert ref.dims(state) == (24, 2, 48, 2, 2, 2, up) and [c[0].shape[:2] for c in cases] == sizes
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= os.path.getsize(os.path.join(GOLDEN, "metrics_skimage.npz"))
    for k, a in state.items():
        assert a.dtype == np.float32, k
        if k.endswith("logit_scale"):                              # heads on both sides of the clamp
            assert (a > math.log(100.0)).any() and (a < math.log(100.0)).any()
    for img, want in cases:
        assert img.dtype == np.uint8 and want.dtype == np.float64 and want.shape == (img.shape[0] * 2, img.shape[1] * 2, 3)
        got = ref.forward(state, img, "float64")
        err = float(np.max(np.abs(got - want)))
        e32 = ref.e32_of(state, img, want)
        print(f"{name} {img.shape[0]}x{img.shape[1]}: restatement - package {err:.2e}, e32 {e32:.2e}, range [{want.min():.2f}, {want.max():.2f}]")
        assert err <= 1e-9
        assert 1e-6 < e32 < 1e-4


@pytest.mark.parametrize("mutant", [m for m in ref.MUTANTS if m != "mask-100"])
def test_mutants_miss_the_stored_output(fixture, mutant):
    """What a wrong reading of the model computes lands outside 8 e32 of every stored output (the -100 mask: below)."""
    name, state, cases = fixture
    for img, want in cases:
        e32 = ref.e32_of(state, img, want)
        err = float(np.max(np.abs(ref.forward(state, img, "float64", mutant=mutant) - want)))
        assert err > 8 * e32, (name, mutant, err, e32)


def test_the_package_masks_twice(fixture):
    """The package adds the shifted-window mask twice: -100 in place of -200 lands outside 8 e32 of the 16 x 24 output of either
    fixture.  (In the single wrapped window of the 8 x 8 input the two do not differ measurably: for -100 to show, a masked key's
    score must lie some 90 above every unmasked one's.)"""
    name, state, cases = fixture
    img, want = cases[-1]
    assert img.shape[:2] == (16, 24)
    err = float(np.max(np.abs(ref.forward(state, img, "float64", mutant="mask-100") - want)))
    assert err > 8 * ref.e32_of(state, img, want)


def test_both_layouts_parse_to_equal_tables(fixture):
    """The package's layout and the same state converted to the official one: bit-equal tables in create order, mask -200 and
    -100; the description read off the shapes; the buffers (filled with poison by the conversion) are never read."""
    import _native
    import sr_network
    name, state, _ = fixture
    d, w, b = sr_network.parse_swin2sr_state(state)
    o, wo, bo = sr_network.parse_swin2sr_state(ref.to_official(state))
    up = FIXTURES[name][0]
    assert (d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale, d.upsampler) == (24, 2, 48, 2, 2, 2, _native.SWINIR_UPSAMPLERS[up])
    assert (o.n_feat, o.n_heads, o.n_hidden, o.n_groups, o.depth, o.scale, o.upsampler) == (24, 2, 48, 2, 2, 2, _native.SWINIR_UPSAMPLERS[up])
    assert d.mask_value == -200.0 and o.mask_value == -100.0 and d.range == 1.0
    assert np.allclose(list(d.mean), ref.RGB_MEAN)
    shapes = _native.swin2sr_table_shapes(d)
    assert len(w) == len(wo) == len(shapes) == len(_native.swin2sr_table_names(d)) == 3 + 2 * (9 * 2 + 2) + 2 + (1 if up == "pixelshuffledirect" else 3)
    for k, (x, y, (sw, sb)) in enumerate(zip(w, wo, shapes)):
        assert x.dtype == np.float32 and x.flags.c_contiguous and x.reshape(sw).shape == sw, k
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    for k, (x, y, (sw, sb)) in enumerate(zip(b, bo, shapes)):
        assert (x is None) == (y is None) == (sb is None), k
        if x is not None:
            assert x.shape == sb and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    # the stacked qkv: query, key, value rows; the k bias zero
    a = f"{ref.layer_prefix(0, 0)}.attention.self"
    assert np.array_equal(w[3], np.concatenate([state[f"{a}.{n}.weight"] for n in ("query", "key", "value")]))
    assert np.array_equal(b[3], np.concatenate([state[f"{a}.query.bias"], np.zeros(24, np.float32), state[f"{a}.value.bias"]]))
    assert sr_network.parse_swin2sr_state(state, mask_value=-150.0)[0].mask_value == -150.0
    with pytest.raises(ValueError, match="Swin2SR state"):              # SwinIR's parser keeps refusing such a state as before
        sr_network.parse_swinir_state(ref.to_official(state))
    with pytest.raises(ValueError, match="not a SwinIR"):
        sr_network.parse_swinir_state(state)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_parser_on_every_synthetic_description(case):
    import _native
    import sr_network
    st = ref.synthetic_state(*case[:7])
    for state, mv in ((st, -200.0), (ref.to_official(st), -100.0)):
        d, w, b = sr_network.parse_swin2sr_state(state)
        assert (d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale) == case[:6]
        assert d.upsampler == _native.SWINIR_UPSAMPLERS[case[6]] and d.mask_value == mv
        for x, (sw, _) in zip(w, _native.swin2sr_table_shapes(d)):
            assert x.shape == sw
    assert _native.swin2sr_plan(d, case[7], case[8]) == ref.plan(case[0], case[2], case[5], case[6], case[7], case[8])


def test_plan_is_swinirs_and_names_its_cap():
    import _native
    d = _native.swin2sr_desc(180, 6, 360, 6, 6, 4, "pixelshuffle")
    s = _native.swinir_desc(180, 6, 360, 6, 6, 4, "pixelshuffle")
    for h, w, tail in [(1, 1, 0), (13, 21, 0), (512, 512, 0), (100, 37, 7), (2048, 2048, 0)]:
        assert _native.swin2sr_plan(d, h, w, tail) == _native.swinir_plan(s, h, w, tail)
    with pytest.raises(ValueError, match="SR_SWIN2SR_TRUNK_CAP"):
        _native.swin2sr_plan(d, 6000, 6000)
    with pytest.raises(ValueError):
        _native.swin2sr_plan(d, 0, 8)
    with pytest.raises(ValueError):
        _native.swin2sr_plan(d, 8, 8, -1)


def test_ranges_are_refused_by_name():
    import _native
    ok = dict(n_feat=60, n_heads=6, n_hidden=120, n_groups=1, depth=2, scale=2, upsampler="pixelshuffle")
    _native.swin2sr_plan(_native.swin2sr_desc(**ok), 8, 8)
    for bad, word in [(dict(n_feat=260, n_heads=10), "embed_dim"), (dict(n_feat=62), "embed_dim"), (dict(n_heads=1), "num_heads"),
                      (dict(n_hidden=241), "hidden"), (dict(n_groups=13), "RSTB"), (dict(depth=13), "RSTB"), (dict(scale=5), "scale"),
                      (dict(upsampler="nearest+conv", scale=2), "nearest"), (dict(upsampler=3), "upsampler"), (dict(range=0.0), "range"),
                      (dict(mean=(0.0, float("nan"), 0.0)), "finite"), (dict(mask_value=float("-inf")), "mask_value")]:
        with pytest.raises(NotImplementedError, match=word):
            _native.swin2sr_plan(_native.swin2sr_desc(**{**ok, **bad}), 8, 8)


def test_cpb_bias_and_logit_scale_of_the_c_side():
    """sr_swin2sr_cpb_bias against numpy in float64 from float64 coordinates: both round a float64 value whose two evaluations
    differ by float64 rounding in a 512-term sum, so the fp32 results agree except where that value lies within ~1e-13 of a
    rounding boundary: at most one ulp, on at most a few entries.  Against the package's form (fp32 coordinates) the distance is
    the rounding-level one the header speaks of.  scale_h: exp of the clamped logit, exactly 100.0f at and above the clamp."""
    import _native
    rng = np.random.default_rng(5)
    heads = 6
    w1 = (rng.standard_normal((512, 2)) * 1.5 / math.sqrt(2)).astype(np.float32)
    b1 = (rng.standard_normal(512) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((heads, 512)) * 1.5 / math.sqrt(512)).astype(np.float32)
    ls = np.array([math.log(200.0), math.log(100.0), math.log(5.0), math.log(99.0), 10.0, -3.0], np.float32)
    table, scale = _native.swin2sr_cpb_bias(w1, b1, w2, ls)
    assert table.shape == (225, heads) and table.dtype == np.float32 and np.array_equal(table, _native.swin2sr_cpb_bias(w1, b1, w2))
    want = ref.cpb_table(w1, b1, w2, np.float64, coords=ref.coords_table64())
    assert 0 < want.min() and want.max() < 16 and want.std() > 1
    ulp = np.abs(table.view(np.int32).astype(np.int64) - want.astype(np.float32).view(np.int32))
    print(f"cpb table: {int((ulp > 0).sum())} of {ulp.size} entries differ, worst {int(ulp.max())} ulp")
    assert ulp.max() <= 1 and (ulp > 0).sum() <= 4
    pack = ref.cpb_table(w1, b1, w2, np.float32)                        # what the package computes, in fp32
    assert np.abs(table.astype(np.float64) - pack).max() < 2e-5
    assert scale.dtype == np.float32 and scale[0] == np.float32(100.0) and scale[1] == np.float32(100.0) and scale[4] == np.float32(100.0)
    want_s = np.exp(np.minimum(ls.astype(np.float64), math.log(100.0))).astype(np.float32)
    assert np.array_equal(scale, want_s) and scale[2] == np.float32(np.exp(np.float64(ls[2]))) and scale[3] < 100.0
    with pytest.raises(ValueError):
        _native.swin2sr_cpb_bias(w1[:100], b1, w2)
    with pytest.raises(ValueError):
        _native.swin2sr_cpb_bias(w1, b1, w2, ls[:3])


def _official(case=ref.CASES[1]):
    return ref.to_official(ref.synthetic_state(*case[:7]))


def test_parser_refuses_by_key():
    """Everything out of scope is a ValueError that names the key, in both layouts, before any device call."""
    import sr_network
    parse = sr_network.parse_swin2sr_state
    pk = ref.synthetic_state(*ref.CASES[1][:7])                         # pixelshuffle x2, C 60, 6 heads, L 1, D 2
    of = ref.to_official(pk)
    a_pk, a_of = f"{ref.layer_prefix(0, 1)}.attention.self", "layers.0.residual_group.blocks.1.attn"

    def refused(state, match, **change):
        st = {k: v for k, v in state.items() if k not in change.get("drop", ())}
        st.update(change.get("add", {}))
        with pytest.raises(ValueError, match=match):
            parse(st)

    with pytest.raises(ValueError, match="not a Swin2SR"):
        parse({"conv_first.weight": np.zeros((4, 3, 3, 3), np.float32)})
    z = np.zeros((64, 3, 3, 3), np.float32)
    refused(pk, "upsample.conv_bicubic.weight", add={"upsample.conv_bicubic.weight": z})            # pixelshuffle_aux
    refused(of, "conv_bicubic.weight", add={"conv_bicubic.weight": z})
    tail_pk = [k for k in pk if k.startswith("upsample.")]
    tail_of = [k for k in of if k.startswith(("conv_before_upsample", "upsample.", "conv_last"))]
    refused(pk, "JPEG / denoising", drop=tail_pk, add={"final_convolution.weight": z})              # no upsampler
    refused(of, "JPEG / denoising", drop=tail_of, add={"conv_last.weight": z})
    refused(pk, "3conv", add={"swin2sr.encoder.stages.0.conv.0.weight": z})
    refused(of, "3conv", add={"layers.0.conv.0.weight": z})
    refused(pk, "absolute position", add={"swin2sr.embeddings.position_embeddings": np.zeros((1, 65, 60), np.float32)})
    refused(of, "absolute position", add={"absolute_pos_embed": np.zeros((1, 64, 60), np.float32)})
    refused(of, "window_size 8", add={f"{a_of}.relative_position_index": np.zeros((256, 256), np.int64)})    # window 16
    refused(of, "window_size 8", add={f"{a_of}.relative_coords_table": np.zeros((1, 31, 31, 2), np.float32)})
    refused(pk, f"{a_pk}.key.bias", add={f"{a_pk}.key.bias": np.full(60, 0.1, np.float32)})         # a k bias that is not zero
    qkv_bias = np.concatenate([of[f"{a_of}.q_bias"], np.full(60, 0.1, np.float32), of[f"{a_of}.v_bias"]])
    refused(of, f"{a_of}.qkv.bias", drop=[f"{a_of}.q_bias", f"{a_of}.v_bias"], add={f"{a_of}.qkv.bias": qkv_bias})
    parse({**pk, f"{a_pk}.key.bias": np.zeros(60, np.float32)})                                     # a zero one is fine
    refused(pk, "same number of heads", add={f"{a_pk}.logit_scale": np.zeros((3, 1, 1), np.float32)})
    refused(of, "same number of heads", add={f"{a_of}.cpb_mlp.2.weight": np.zeros((3, 512), np.float32)})
    two = ref.synthetic_state(24, 3, 48, 2, 2, 2, "pixelshuffledirect")
    deep = {k: v for k, v in two.items() if ".stages.1.layers.1." not in k}                          # stage 1 one layer short
    with pytest.raises(ValueError, match="same depth"):
        parse(deep)
    with pytest.raises(ValueError, match="same depth"):
        parse({k: v for k, v in ref.to_official(two).items() if "layers.1.residual_group.blocks.1." not in k})
    with pytest.raises(ValueError, match="numbered"):
        parse({k: v for k, v in two.items() if ".stages.1.layers.0." not in k})
    refused(pk, "float16", add={f"{a_pk}.query.weight": pk[f"{a_pk}.query.weight"].astype(np.float16)})
    refused(of, "float16", add={"conv_first.weight": of["conv_first.weight"].astype(np.float16)})
    refused(pk, "expected shape", add={f"{a_pk}.continuous_position_bias_mlp.0.weight": np.zeros((256, 2), np.float32)})
    refused(pk, "patch_size 1", add={"swin2sr.embeddings.patch_embeddings.projection.weight": np.zeros((60, 60, 2, 2), np.float32)})
    refused(pk, "not in the state", drop=[f"{a_pk}.value.bias"])
    with pytest.raises(NotImplementedError):                                                        # only the kernels' range: d = 60
        parse(ref.synthetic_state(60, 1, 120, 1, 1, 2, "pixelshuffledirect"))


def test_model_tables_are_checked_before_any_device_call():
    """_native.Swin2srModel checks counts and shapes on the host; ctx is never touched (None)."""
    import _native
    import sr_network
    d, w, b = sr_network.parse_swin2sr_state(ref.synthetic_state(*ref.CASES[0][:7]))
    with pytest.raises(ValueError, match="tables"):
        _native.Swin2srModel(None, d, w[:-1], b[:-1])
    with pytest.raises(ValueError, match="table 4"):
        _native.Swin2srModel(None, d, w[:4] + [w[4][:2]] + w[5:], b)
    bad = _native.swin2sr_desc(60, 7, 120, 1, 1, 2)
    with pytest.raises(NotImplementedError):
        _native.Swin2srModel(None, bad, w, b)


def test_create_refuses_a_k_bias_and_a_bad_logit_scale_without_a_context():
    """sr_swin2sr_create decides on the host: with a null context a k bias that is not zero and a non-finite logit_scale come back
    as SR_ERR_UNSUPPORTED by name, a good set of tables gets as far as the context (SR_ERR_INVALID_ARG)."""
    import ctypes as C

    import _native
    import sr_network
    d, w, b = sr_network.parse_swin2sr_state(ref.synthetic_state(*ref.CASES[0][:7]))
    lib = _native.load()

    def create(ws, bs):
        bs = [np.zeros(1, np.float32) if x is None else x for x in bs]
        pw, pb = ((C.c_void_p * len(t))(*[a.ctypes.data for a in t]) for t in (ws, bs))
        h = C.c_void_p()
        return lib.sr_swin2sr_create(None, C.byref(d), pw, pb, len(ws), C.byref(h)), h.value

    kb = [None if x is None else x.copy() for x in b]
    kb[3][d.n_feat] = 1e-3                                                                          # table 3: the first qkv
    assert create(w, kb) == (_native.SR_ERR_UNSUPPORTED, None) and "k bias" in _native.last_error()
    lw = [x.copy() for x in w]
    lw[4][1] = np.nan                                                                               # table 4: its logit_scale
    assert create(lw, b) == (_native.SR_ERR_UNSUPPORTED, None) and "logit_scale" in _native.last_error()
    rc, h = create(w, b)
    assert rc == _native.SR_ERR_INVALID_ARG and h is None
    assert create(w[:-1], b[:-1])[0] == _native.SR_ERR_INVALID_ARG and "tables" in _native.last_error()


def test_load_network_order(tmp_path):
    """Swin2SR's keys are tested before SwinIR's (an official-layout state carries SwinIR's key too); a .npz entry ``mask_value``
    overrides the layout's."""
    import sr_network
    import _swinir_ref
    pk = ref.synthetic_state(*ref.CASES[0][:7])
    of = ref.to_official(pk)
    assert sr_network.SWINIR_KEY in of and sr_network.swin2sr_layout(of) == "official" and sr_network.swin2sr_layout(pk) == "package"
    for name, state, mv in (("pk.npz", pk, -200.0), ("of.npz", of, -100.0), ("mv.npz", {**of, "mask_value": np.array(-150.0, np.float32)}, -150.0)):
        path = str(tmp_path / name)
        np.savez(path, **state)
        net = sr_network.load_network(path)
        assert isinstance(net, sr_network.Swin2SRNet) and net.mask_value == mv and net.scale == 2 and net.n_heads == 3
    sw = _swinir_ref.synthetic_state(60, 6, 120, 1, 2, 2, "pixelshuffledirect")
    path = str(tmp_path / "swinir.npz")
    np.savez(path, **sw)
    assert isinstance(sr_network.load_network(path), sr_network.SwinIRSRNet)                        # SwinIR still goes to SwinIR


def test_safetensors_file_is_read_where_the_package_imports(tmp_path):
    """``model.safetensors`` is what the published Swin2SR checkpoints ship as; without the package load_state raises by name."""
    import sr_network
    pk = ref.synthetic_state(*ref.CASES[0][:7])
    try:
        import safetensors.numpy as st
    except ImportError:
        with pytest.raises(RuntimeError, match="safetensors"):
            sr_network.load_state(str(tmp_path / "model.safetensors"))
        return
    path = str(tmp_path / "model.safetensors")
    st.save_file({k: np.ascontiguousarray(v) for k, v in pk.items()}, path)
    net = sr_network.load_network(path)
    assert isinstance(net, sr_network.Swin2SRNet) and net.mask_value == -200.0
    d0 = sr_network.parse_swin2sr_state(pk)
    assert all(np.array_equal(x, y) for x, y in zip(net._w, d0[1]))
    with pytest.raises(ValueError, match="no tile"):
        net.upscale_device(0, (8, 8, 3), 0, 48, tile=16)


@pytest.mark.parametrize("scale,up", [(2, "pixelshuffle"), (3, "pixelshuffle"), (4, "pixelshuffle"), (1, "pixelshuffledirect"), (4, "nearest+conv")])
def test_table_names_are_the_packages_keys(scale, up):
    """_native.swin2sr_table_names in create order: every name but the stacked qkv and logit_scale is a '<name>.weight' key of the
    package's state dict, and the reconstruction's names are the package's."""
    import _native
    names = _native.swin2sr_table_names(_native.swin2sr_desc(24, 3, 48, 2, 2, scale, up))
    keys = ref.state_shapes(24, 3, 48, 2, 2, scale, up)
    assert names[-len(ref.tail_names(scale, up)):] == ref.tail_names(scale, up)
    for n in names:
        if n.endswith(".qkv"):
            assert all(f"{n[:-4]}.{part}.weight" in keys for part in ("query", "key", "value"))
        elif n.endswith("logit_scale"):
            assert n in keys
        else:
            assert f"{n}.weight" in keys, n
