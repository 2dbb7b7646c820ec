"""CPU: the host side of the RRDB backend (ESRGAN / Real-ESRGAN x4) -- the BasicSR state-dict parser and its refusals,
load_network's dispatch, sr_rrdb_plan (no context, no GPU) against the Python restatement of the two-phase plan rule, the ABI's
refusals that need no device, and the numerical bars of tests/test_gpu_rrdb.py held on the CPU first: the documented summation
order alone inside err <= 8 e32 and inside the u8 check, and the exact-arithmetic networks and probes proved exact (float64 ==
float32 == the documented order, bit for bit).  No device call is made here."""
import ctypes as C

import numpy as np
import pytest

import _native
import _resnet_ref as resref
import _rrdb_ref as ref
import _srnet_ref as sref
import main as sr_main
import sr_network


def _desc(F, G, B, scale=4, slope=0.2, res_scale=0.2):
    return _native.rrdb_desc(F, G, B, scale, slope, res_scale)


@pytest.mark.parametrize("F,G,B", [(64, 32, 1), (64, 32, 2), (128, 64, 1), (64, 64, 1), (256, 32, 0)])
def test_parser_round_trip(F, G, B):
    st = ref.synthetic_state(F, G, B)
    desc, w, b = sr_network.parse_rrdb_state(st)
    assert (desc.n_feat, desc.n_grow, desc.n_blocks, desc.scale) == (F, G if B else 32, B, 4)
    assert (desc.slope, desc.res_scale) == (np.float32(0.2), np.float32(0.2))
    shapes = _native.rrdb_conv_shapes(desc)
    assert shapes == ref.conv_shapes(F, desc.n_grow, B) and len(shapes) == 1 + 15 * B + 5
    assert [x.shape for x in w] == [(co, ci, 3, 3) for co, ci in shapes] and [x.shape for x in b] == [(co,) for co, _ in shapes]
    assert all(x.dtype == np.float32 and x.flags.c_contiguous for x in w + b)
    for name, wk, bk in zip(ref.conv_names(B), w, b):
        assert np.array_equal(wk, st[f"{name}.weight"]) and np.array_equal(bk, st[f"{name}.bias"])
    for wrap in ("params_ema", "params"):
        net = sr_network.RRDBSRNet({wrap: st}, slope=0.1, res_scale=0.3)
        assert (net.n_feat, net.n_grow, net.n_blocks, net.scale) == (F, desc.n_grow, B, 4)
        assert (net.desc.slope, net.desc.res_scale) == (np.float32(0.1), np.float32(0.3))
    assert issubclass(sr_network.RRDBSRNet, sr_network.CompactSRNet)


def test_parse_refusals_name_the_key():
    good = ref.synthetic_state(64, 32, 2)

    def bad(key, value, match, exc=ValueError):
        st = dict(good)
        if value is None:
            del st[key]
        else:
            st[key] = value
        with pytest.raises(exc, match=match):
            sr_network.parse_rrdb_state(st)

    z = lambda *shape: np.zeros(shape, np.float32)
    bad("body.1.rdb2.conv3.weight", z(32, 96, 3, 3), r"body\.1\.rdb2\.conv3\.weight takes 96 channels")       # wrong cin
    bad("conv_first.weight", z(64, 4, 3, 3), r"conv_first\.weight takes 4 channels")
    bad("body.0.rdb1.conv5.weight", z(32, 192, 3, 3), r"body\.0\.rdb1\.conv5\.weight gives 32 channels")      # wrong cout
    bad("conv_last.weight", z(12, 64, 3, 3), r"conv_last\.weight gives 12 channels")
    bad("conv_up2.weight", z(256, 64, 3, 3), r"conv_up2\.weight gives 256 channels")
    bad("body.0.rdb3.conv2.bias", None, r"body\.0\.rdb3\.conv2\.bias")                                         # missing bias
    bad("conv_body.bias", None, r"conv_body\.bias")
    bad("conv_hr.weight", None, r"conv_hr\.weight")
    bad("conv_last.bias", z(4), r"conv_last\.bias")
    bad("conv_hr.weight", z(64, 64, 5, 5), r"conv_hr\.weight: only 3x3")                                       # non-3x3
    bad("body.1.rdb1.conv1.weight", z(32, 64, 1, 1), r"body\.1\.rdb1\.conv1\.weight: only 3x3")
    bad("body.0.rdb2.conv2.weight", z(64, 96, 3, 3), r"body\.0\.rdb2\.conv2\.weight gives 64 channels")        # unequal G
    bad("body.1.rdb3.conv4.weight", z(16, 160, 3, 3), r"body\.1\.rdb3\.conv4\.weight gives 16 channels")
    bad("body.0.rdb1.conv1.weight", None, r"body\.0\.rdb1\.conv1\.weight")
    gap = {k.replace("body.1.", "body.2."): v for k, v in good.items()}
    with pytest.raises(ValueError, match=r"body\.1\.rdb1\.conv1\.weight"):                                      # a gap in body.{i}
        sr_network.parse_rrdb_state(gap)
    with pytest.raises(ValueError, match="conv_first"):
        sr_network.parse_rrdb_state(sref.synthetic_state(64, 1, 2))
    for cin in (12, 48):                                         # the x2 / x1 variants: a pixel-unshuffle in front of conv_first
        bad("conv_first.weight", z(64, cin, 3, 3), "pixel-unshuffle", NotImplementedError)
    with pytest.raises(NotImplementedError):                     # chains, but outside the kernels' range
        sr_network.parse_rrdb_state(ref.synthetic_state(96, 32, 1))
    with pytest.raises(NotImplementedError):
        sr_network.parse_rrdb_state(ref.synthetic_state(64, 16, 1))
    with pytest.raises(NotImplementedError):
        sr_network.RRDBSRNet(good, slope=float("nan"))
    with pytest.raises(ValueError, match="res_scale"):
        sr_network._rrdb_extras({"res_scale": np.zeros(2)})


def test_load_network_dispatch(tmp_path):
    st = ref.synthetic_state(64, 32, 1)
    np.savez(tmp_path / "rrdb.npz", **st)
    net = sr_network.load_network(str(tmp_path / "rrdb.npz"), act="relu")          # act is ignored for this family
    assert type(net) is sr_network.RRDBSRNet and (net.n_feat, net.n_grow, net.n_blocks, net.scale) == (64, 32, 1, 4)
    assert (net.desc.slope, net.desc.res_scale) == (np.float32(0.2), np.float32(0.2))
    np.savez(tmp_path / "extras.npz", slope=np.array(0.1, np.float32), res_scale=np.array(0.5, np.float32), **st)
    net = sr_network.load_network(str(tmp_path / "extras.npz"))
    assert type(net) is sr_network.RRDBSRNet and (net.desc.slope, net.desc.res_scale) == (np.float32(0.1), 0.5)
    again = sr_network.RRDBSRNet.from_file(str(tmp_path / "extras.npz"), res_scale=0.25)
    assert (again.desc.slope, again.desc.res_scale) == (np.float32(0.1), 0.25)
    # every other file dispatches as before
    np.savez(tmp_path / "compact.npz", **sref.synthetic_state(64, 2, 2))
    assert type(sr_network.load_network(str(tmp_path / "compact.npz"))) is sr_network.CompactSRNet
    for preset in ("msr", "edsr"):
        np.savez(tmp_path / f"{preset}.npz", **resref.synthetic_state(preset, 64, 1, 2))
        assert type(sr_network.load_network(str(tmp_path / f"{preset}.npz"))) is sr_network.ResidualSRNet


def test_pth_loader_unwraps_params(tmp_path):
    torch = pytest.importorskip("torch")
    st = ref.synthetic_state(64, 32, 1)
    torch.save({"params_ema": {k: torch.from_numpy(v) for k, v in st.items()}}, str(tmp_path / "net.pth"))
    net = sr_network.load_network(str(tmp_path / "net.pth"))
    assert type(net) is sr_network.RRDBSRNet and net.scale == 4 and np.array_equal(net._w[1], st["body.0.rdb1.conv1.weight"])


def test_pipeline_config_and_scale_mismatch(tmp_path):
    path = tmp_path / "rrdb.npz"
    np.savez(path, **ref.synthetic_state(64, 32, 1))
    with pytest.raises(ValueError, match="sr_scale"):            # no device is touched: this passes without a GPU
        sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=2))
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=4, block_size=64))
    assert isinstance(pipe.sr_net, sr_network.RRDBSRNet) and pipe.sr_net.scale == 4 and pipe._builtin_backend()


def test_plan_matches_the_restated_rule():
    for B, want in ((0, 4), (1, 19), (2, 34), (6, 94), (23, 349), (32, 15 * 32 + 4)):       # last 1, hr 2, up2 3, up1 3, body 3, then 15 B + 1
        assert ref.halo(B) == want and _native.rrdb_plan(_desc(64, 32, B), 10, 10)[0] == want
    grid = [(F, G, B, h, w, tile, tail)
            for F, G, B in ((64, 32, 1), (64, 32, 2), (128, 64, 1), (64, 64, 6), (256, 32, 0))
            for h, w in ((21, 37), (5, 6), (1, 1), (1, 40), (64, 33))
            for tile, tail in ((0, 0), (8, 0), (8, 5), (13, 1), (1, 1), (4, 3), (32, 7), (7, 64))]
    grid += [(64, 32, 23, 2048, 2048, 0, 0), (64, 32, 23, 2048, 2048, 512, 128), (64, 32, 6, 3000, 2000, 0, 0), (256, 64, 23, 4000, 3000, 0, 0),
             (128, 64, 2, 300, 5000, 0, 100), (64, 32, 1, 4096, 4096, 0, 0)]
    for F, G, B, h, w, tile, tail in grid:
        assert _native.rrdb_plan(_desc(F, G, B), h, w, tile, tail) == ref.plan(F, G, B, h, w, tile, tail), (F, G, B, h, w, tile, tail)
    # the default block of the pipeline, 2048 x 2048 at F 64 G 32, runs the trunk in one piece under the 16 GiB cap; the tail
    # phase walks it in 8 x 8 sub-pieces of 256
    halo, n, nt, ws = _native.rrdb_plan(_desc(64, 32, 23), 2048, 2048)
    assert (halo, n, nt) == (349, 1, 64) and ws <= ref.TRUNK_CAP
    assert ws == 4 * ((3 * 192 + 64) * 2048 * 2048 + 64 * 4096 * 4096 + 2 * 64 * (4 * 256 + 8) ** 2)       # an interior sub-piece: 3 each side at 4 x, rounded outwards to 2 x
    # ... and F 256 does not: tile 0 comes from the cap
    halo, n, nt, ws = _native.rrdb_plan(_desc(256, 64, 23), 4000, 3000)
    assert n > 1
    # one piece of each: the counts and the formula by hand (trunk planes 21 x 40, f at 2 x 42 x 76, tail 84 x 148)
    assert _native.rrdb_plan(_desc(64, 32, 1), 21, 37, 64, 64) == (19, 1, 1, 4 * ((3 * 192 + 64) * 21 * 40 + 64 * 42 * 76 + 2 * 64 * 84 * 148))
    # pieces smaller than the halo and one-pixel pieces count as the grid says
    assert _native.rrdb_plan(_desc(64, 32, 2), 20, 30, 4)[1:3] == (5 * 8, 5 * 8)
    assert _native.rrdb_plan(_desc(64, 32, 1), 5, 6, 1, 1)[1:3] == (30, 30)
    assert _native.rrdb_plan(_desc(64, 32, 1), 21, 37, 8, 5)[1:3] == (3 * 5, (2 + 2 + 1) * (2 * 4 + 1))


def test_plan_and_create_refusals():
    for F, G, B, s in ((96, 32, 1, 4), (48, 32, 1, 4), (64, 16, 1, 4), (64, 48, 1, 4), (64, 32, 33, 4), (64, 32, -1, 4), (320, 32, 1, 4),
                       (64, 32, 1, 2), (64, 32, 1, 1), (64, 32, 1, 3), (64, 32, 1, 8)):
        with pytest.raises(NotImplementedError):
            _native.rrdb_plan(_desc(F, G, B, s), 100, 100)
    for field in ("slope", "res_scale"):
        for value in (float("nan"), float("inf")):
            with pytest.raises(NotImplementedError):
                _native.rrdb_plan(_desc(64, 32, 1, **{field: value}), 100, 100)
    d = _desc(64, 32, 1)
    for args in ((100, 100, -1, 0), (100, 100, 0, -1), (0, 100, 0, 0), (100, 0, 0, 0)):                # tile / tail < 0, h / w < 1
        with pytest.raises(ValueError):
            _native.rrdb_plan(d, *args)
    with pytest.raises(ValueError):                              # (4 h) x (4 w x 3) must fit int
        _native.rrdb_plan(d, 100, 200_000_000, 64)
    with pytest.raises(ValueError):                              # a piece beyond the kernels' 32-bit offsets
        _native.rrdb_plan(d, 30000, 30000, 30000)
    lib = _native.load()
    assert lib.sr_rrdb_plan(None, 10, 10, 0, 0, None, None, None, None) == _native.SR_ERR_INVALID_ARG  # null description
    assert lib.sr_rrdb_plan(C.byref(d), 10, 10, 0, 0, None, None, None, None) == _native.SR_OK         # outputs may be NULL
    out = C.c_void_p()
    assert lib.sr_rrdb_create(None, None, None, None, 0, C.byref(out)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_rrdb_create(None, C.byref(d), None, None, 21, None) == _native.SR_ERR_INVALID_ARG     # null out
    assert lib.sr_rrdb_create(None, C.byref(d), None, None, 21, C.byref(out)) == _native.SR_ERR_INVALID_ARG   # null tables
    tab = (C.c_void_p * 21)()
    assert lib.sr_rrdb_create(None, C.byref(d), tab, tab, 20, C.byref(out)) == _native.SR_ERR_INVALID_ARG     # a wrong n_conv
    assert "21 convolutions" in _native.last_error()
    assert lib.sr_rrdb_create(None, C.byref(d), tab, tab, 21, C.byref(out)) == _native.SR_ERR_INVALID_ARG     # null arrays
    assert lib.sr_rrdb_create(None, C.byref(_desc(96, 32, 1)), None, None, 21, C.byref(out)) == _native.SR_ERR_UNSUPPORTED
    assert lib.sr_rrdb_create(None, C.byref(_desc(64, 32, 1, 2)), None, None, 21, C.byref(out)) == _native.SR_ERR_UNSUPPORTED
    for fn in (lib.sr_rrdb_u8, lib.sr_rrdb_f32):                 # null model
        assert fn(None, None, 0, 1, 1, None, 0, 0, 0) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_rrdb_destroy(None) == _native.SR_OK
    with pytest.raises(NotImplementedError):
        _native.RrdbModel(None, _desc(96, 32, 1), [], [])                           # refused before the context is looked at
    with pytest.raises(ValueError):
        _native.RrdbModel(None, d, [], [])                                          # wrong number of arrays, before the context


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_documented_summation_order_stays_inside_the_gpu_bar(case):
    """The accuracy bar of tests/test_gpu_rrdb.py, err <= 8 e32, held against the kernels' documented summation order restated
    in numpy fp32 (ref.chain_forward): the order alone must fit the bar, or the bar says nothing about the kernels.  The u8
    rule's exempt share stays under its 1 % cap, and CASES[0] clamps a visible share at both ends."""
    F, G, B, h, w = case
    state, img, f64, e32 = ref.case(*case)
    chain, e_chain = ref.chain_case(*case)
    assert chain.dtype == np.float32 and chain.shape == f64.shape == (h * 4, w * 4, 3)
    lo, hi = float((f64 <= 0).mean()), float((f64 >= 1).mean())
    print(f"rrdb chain {ref.case_id(case)}: e32 {e32:.3e}  e_chain {e_chain:.3e}  ratio {e_chain / e32:.3f}  clamps at 0 {lo:.2%}  at 1 {hi:.2%}")
    assert 0 < e32 < 1e-5
    assert e_chain <= 8 * e32, (e_chain, e32, e_chain / e32)     # the documented order alone is inside the GPU bar
    share = ref.check_u8(ref.quantize(chain), f64, e32)          # ... and inside the u8 check with its 1 % exempt cap
    print(f"  u8 of the chain: exempt share {share:.4%}")
    if case == ref.CASES[0]:
        assert lo > 0.01 and hi > 0.01


@pytest.mark.parametrize("name", [n[0] for n in ref.EXACT_NETS] + [p[0] for p in ref.PROBES])
def test_exact_networks_and_probes_are_exact(name):
    """float64 == float32 == the documented order, bit for bit, and the reason: every value is a multiple of 2^-bits and the
    absolute-value forward (which bounds every partial sum in any order) stays below 2^24 of those units."""
    state, img, slope, beta, chain = ref.exact_case(name)
    bits, bound, o64 = ref.exact_proof(state, img, slope, beta)
    print(f"rrdb exact {name}: unit 2^-{bits}, bound {bound:.1f} = 2^{np.log2(bound) + bits:.2f} units")
    assert bound * 2.0 ** bits < 2 ** 24
    f64, f32 = ref.forward(state, img, "float64", slope, beta), ref.forward(state, img, "float32", slope, beta)
    assert np.array_equal(f64, o64)
    assert np.array_equal(f32.astype(np.float64), f64) and np.array_equal(chain.astype(np.float64), f64)
    assert np.array_equal(f32.view(np.uint32), chain.view(np.uint32))
    assert len(np.unique(chain)) > 4 and (chain < 0).any() and (chain > 1).any()     # not degenerate; the u8 form clamps both ways


def test_probes_show_a_shifted_copy_of_the_probed_plane():
    """What a probe is: against the same network with the probed weight at the centre tap, the output moves; against the network
    without the probed weight, it differs in the one output channel the probed block's conv5 feeds (a dense probe)."""
    seen = set()
    for name, spec in ref.PROBES:
        if spec[0] != "dense":
            continue
        d, k, co, j, t = spec[1:]
        seen.add((k, j))
        state, img, slope, beta, chain = ref.exact_case(name)
        key = f"body.0.rdb{d}.conv{k}.weight"
        assert state[key].sum() == 1.0 and state[key][co, j, t // 3, t % 3] == 1.0
        off = {kk: np.array(v) for kk, v in state.items()}
        off[key][...] = 0.0
        base = ref.chain_forward(off, img, slope, beta)
        diff = np.argwhere(base != chain)
        assert len(diff) > 0, name
        feat = co % 64 if k < 5 else co
        assert set(diff[:, 2].tolist()) == {feat % 3}, (name, set(diff[:, 2].tolist()))
    # every dense convolution k, first and last channel of each concatenated segment
    assert seen == {(k, j) for k in range(1, 6) for j in ref._segment_ends(k)}
    assert {spec[1] for _, spec in ref.PROBES if spec[0] == "dense"} == {1, 2, 3}
    assert {spec[1] for _, spec in ref.PROBES if spec[0] == "perm"} >= {"conv_body", "conv_up1", "conv_up2"}
    assert ref.PROBE_H % 2 == 1 and ref.PROBE_W % 2 == 1
