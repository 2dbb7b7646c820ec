"""CPU: the host side of the RCAN backend -- the BasicSR state-dict parser and its refusals, load_network's dispatch (an RCAN
state no longer comes back as an EDSR of zero blocks), sr_rcan_plan (no context, no GPU) against the Python restatement, the ABI's
refusals that need no device, the cap's message, and the numerical bars of tests/test_gpu_rcan.py held on the CPU first: the
documented order alone inside err <= 8 e32 and inside the u8 check, the mutants that the cases must be able to see, and the
exact-arithmetic networks and probes proved exact.  No device call is made here."""
import ctypes as C

import numpy as np
import pytest

import _native
import _rcan_ref as ref
import _resnet_ref as resref
import _rrdb_ref as rrdbref
import _srnet_ref as sref
import main as sr_main
import sr_network


def _desc(F=64, R=4, G=1, B=1, s=2, **kw):
    return _native.rcan_desc(F, R, G, B, s, **kw)


@pytest.mark.parametrize("F,R,G,B,s", [(64, 4, 2, 2, 2), (64, 1, 1, 1, 4), (128, 8, 1, 2, 3), (64, 64, 3, 1, 1), (256, 16, 1, 0, 2)])
def test_parser_round_trip(F, R, G, B, s):
    st = ref.synthetic_state(F, R, G, B, s)
    desc, w, b = sr_network.parse_rcan_state(st, res_scale=0.25, img_range=2.0, rgb_mean=(0.1, 0.2, 0.3))
    assert (desc.n_feat, desc.n_squeeze, desc.n_groups, desc.n_blocks, desc.scale) == (F, R if B else max(1, F // 16), G, B, s)
    assert (desc.res_scale, desc.range, tuple(desc.mean)) == (0.25, 2.0, tuple(np.float32((0.1, 0.2, 0.3))))
    shapes = _native.rcan_conv_shapes(desc)
    assert shapes == ref.table_shapes(F, desc.n_squeeze, G, B, s) and len(shapes) == 1 + G * (4 * B + 1) + 1 + len(ref.STAGES[s]) + 1
    assert [x.shape for x in w] == [(co, ci, 3, 3) if k == 3 else (co, ci) for co, ci, k in shapes]
    assert [x.shape for x in b] == [(co,) for co, _, _ in shapes]
    assert all(x.dtype == np.float32 and x.flags.c_contiguous for x in w + b)
    rw, rb = ref.arrays(st)
    assert all(np.array_equal(x, y) for x, y in zip(w + b, rw + rb))
    for wrap in ("params_ema", "params"):
        net = sr_network.RCANSRNet({wrap: st})
        assert (net.n_feat, net.n_squeeze, net.n_groups, net.n_blocks, net.scale) == (F, desc.n_squeeze, G, B, s)
        assert (net.desc.res_scale, net.desc.range) == (1.0, 255.0)                  # BasicSR's defaults
        assert tuple(net.desc.mean) == tuple(np.float32(sr_network.EDSR_RGB_MEAN))
    assert issubclass(sr_network.RCANSRNet, sr_network.CompactSRNet)


def test_parse_refusals_name_the_key():
    good = ref.synthetic_state(64, 4, 2, 2, 2)

    def bad(key, value, match, exc=ValueError):
        st = dict(good)
        if value is None:
            del st[key]
        else:
            st[key] = value
        with pytest.raises(exc, match=match):
            sr_network.parse_rcan_state(st)

    z = lambda *shape: np.zeros(shape, np.float32)
    r = "body.1.residual_group.1.rcab"
    bad(f"{r}.2.bias", None, r"body\.1\.residual_group\.1\.rcab\.2\.bias")                            # a missing key
    bad(f"{r}.3.attention.3.weight", None, r"rcab\.3\.attention\.3\.weight")
    bad("body.0.conv.weight", None, r"body\.0\.conv\.weight")
    bad("conv_after_body.bias", None, r"conv_after_body\.bias")
    bad("conv_last.weight", None, r"conv_last\.weight")
    bad(f"{r}.3.attention.1.weight", z(8, 64, 1, 1), r"body\.1\.residual_group\.1\.rcab\.3\.attention\.1\.weight: expected the 1x1")   # a wrong 1 x 1 shape
    bad(f"{r}.3.attention.3.weight", z(64, 4, 3, 3), r"attention\.3\.weight: expected the 1x1")
    bad(f"{r}.3.attention.3.weight", z(64, 4), r"attention\.3\.weight: expected the 1x1")
    bad(f"{r}.3.attention.1.bias", z(5), r"attention\.1\.bias: expected 4 values")
    bad(f"{r}.0.weight", z(64, 32, 3, 3), r"rcab\.0\.weight takes 32 channels")
    bad(f"{r}.2.weight", z(64, 64, 1, 1), r"rcab\.2\.weight: only 3x3")
    bad("body.1.conv.weight", z(32, 64, 3, 3), r"body\.1\.conv\.weight gives 32 channels")
    bad("upsample.0.weight", z(128, 64, 3, 3), r"upsample\.0\.weight gives 128 channels")
    bad("conv_last.weight", z(4, 64, 3, 3), r"conv_last\.weight gives 4 channels")
    gap = {k.replace("body.1.", "body.2."): v for k, v in good.items()}                                # a gap in the groups
    with pytest.raises(ValueError, match=r"body\.1\.conv\.weight"):
        sr_network.parse_rcan_state(gap)
    gap = {k.replace("body.0.residual_group.1.", "body.0.residual_group.2."): v for k, v in good.items()}   # ... in a group's blocks
    with pytest.raises(ValueError, match=r"body\.0\.residual_group\.1\.rcab\.0\.weight"):
        sr_network.parse_rcan_state(gap)
    unequal = {k: v for k, v in good.items() if not k.startswith("body.1.residual_group.1.")}          # unequal groups
    with pytest.raises(ValueError, match=r"body\.1\.residual_group\.1\.rcab\.0\.weight: every group must have the same number"):
        sr_network.parse_rcan_state(unequal)
    with pytest.raises(ValueError, match="conv_first"):
        sr_network.parse_rcan_state(sref.synthetic_state(64, 1, 2))
    with pytest.raises(NotImplementedError, match="96 features"):                                      # chains, but outside the kernels' range
        sr_network.parse_rcan_state(ref.synthetic_state(96, 4, 1, 1, 2))
    with pytest.raises(NotImplementedError, match="17 groups"):
        sr_network.parse_rcan_state(ref.synthetic_state(64, 4, 17, 0, 2))
    x8 = dict(ref.synthetic_state(64, 4, 1, 1, 4))
    x8["upsample.4.weight"], x8["upsample.4.bias"] = z(256, 64, 3, 3), z(256)                          # three shuffle stages
    with pytest.raises(NotImplementedError, match="scale 8"):
        sr_network.parse_rcan_state(x8)
    with pytest.raises(NotImplementedError):
        sr_network.RCANSRNet(good, res_scale=float("nan"))
    with pytest.raises(NotImplementedError):
        sr_network.RCANSRNet(good, img_range=0.0)


def test_an_rcan_state_is_no_longer_an_edsr_of_zero_blocks(tmp_path):
    """The regression: load_network used to hand an RCAN file to the residual parser, which found no body.{i}.conv1 and returned
    an EDSR with n_blocks == 0 without a word."""
    st = ref.synthetic_state(64, 4, 2, 2, 2)
    np.savez(tmp_path / "rcan.npz", **st)
    net = sr_network.load_network(str(tmp_path / "rcan.npz"))
    assert type(net) is sr_network.RCANSRNet and not isinstance(net, sr_network.ResidualSRNet)
    assert (net.n_groups, net.n_blocks) == (2, 2)
    with pytest.raises(ValueError, match="RCAN"):                # ... and the residual parser itself says so when asked directly
        sr_network.parse_residual_state(st)


def test_load_network_dispatch(tmp_path):
    st = ref.synthetic_state(64, 4, 1, 1, 2)
    np.savez(tmp_path / "rcan.npz", **st)
    net = sr_network.load_network(str(tmp_path / "rcan.npz"), act="relu")          # act is ignored for this family
    assert type(net) is sr_network.RCANSRNet and (net.n_feat, net.n_squeeze, net.n_groups, net.n_blocks, net.scale) == (64, 4, 1, 1, 2)
    assert (net.desc.res_scale, net.desc.range) == (np.float32(ref.RES_SCALE), 255.0)     # the .npz extras
    plain = {k: v for k, v in st.items() if "." in k}
    np.savez(tmp_path / "plain.npz", **plain)
    net = sr_network.load_network(str(tmp_path / "plain.npz"))
    assert (net.desc.res_scale, net.desc.range, tuple(net.desc.mean)) == (1.0, 255.0, tuple(np.float32(sr_network.EDSR_RGB_MEAN)))
    again = sr_network.RCANSRNet.from_file(str(tmp_path / "rcan.npz"), res_scale=0.25)
    assert (again.desc.res_scale, again.desc.range) == (0.25, 255.0)
    # all four families, the other three exactly as before
    np.savez(tmp_path / "compact.npz", **sref.synthetic_state(64, 2, 2))
    assert type(sr_network.load_network(str(tmp_path / "compact.npz"))) is sr_network.CompactSRNet
    for preset in ("msr", "edsr"):
        np.savez(tmp_path / f"{preset}.npz", **resref.synthetic_state(preset, 64, 1, 2))
        got = sr_network.load_network(str(tmp_path / f"{preset}.npz"))
        assert type(got) is sr_network.ResidualSRNet and got.n_blocks == 1
    np.savez(tmp_path / "rrdb.npz", **rrdbref.synthetic_state(64, 32, 1))
    assert type(sr_network.load_network(str(tmp_path / "rrdb.npz"))) is sr_network.RRDBSRNet


def test_pipeline_config_and_tile_refusal(tmp_path):
    path = tmp_path / "rcan.npz"
    np.savez(path, **ref.synthetic_state(64, 4, 1, 1, 2))
    with pytest.raises(ValueError, match="sr_scale"):            # no device is touched: this passes without a GPU
        sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=4))
    pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=str(path), sr_scale=2, block_size=64, sr_ensemble=8))
    assert isinstance(pipe.sr_net, sr_network.RCANSRNet) and pipe.sr_net.scale == 2 and pipe._builtin_backend()
    with pytest.raises(ValueError, match="no tile"):             # before the model is made
        pipe.sr_net.upscale_device(0, (8, 8, 3), 0, 48, tile=16)


def test_plan_matches_the_restated_rule():
    for s, want in ((1, 1), (2, 2), (3, 2), (4, 2)):
        assert _native.rcan_plan(_desc(s=s), 10, 10)[0] == ref.plan(64, s, 10, 10)[0] == want
    grid = [(F, s, h, w, tail) for F in (64, 128, 256) for s in (1, 2, 3, 4)
            for h, w in ((11, 37), (5, 6), (1, 1), (1, 50), (50, 1), (40, 70), (64, 33)) for tail in (0, 1, 5, 16, 64)]
    grid += [(64, 4, 2048, 2048, 0), (64, 2, 3000, 4000, 100), (256, 3, 1000, 1500, 0), (64, 1, 3600, 3600, 0)]
    for F, s, h, w, tail in grid:
        assert _native.rcan_plan(_desc(F, 4, 2, 2, s), h, w, tail) == ref.plan(F, s, h, w, tail), (F, s, h, w, tail)
    # by hand: one sub-piece, 11 x 37 at x4 (planes 11 x 40; the first stage's output 22 x 74 -> 76, the second's 44 x 148)
    assert _native.rcan_plan(_desc(s=4), 11, 37) == (2, 1, 4 * (5 * 64 * 11 * 40 + 2 * 64 * 44 * 148) + 8 * 64 + 4 * 64)
    assert _native.rcan_plan(_desc(s=2), 40, 70, 16)[1] == 3 * 5
    # an interior sub-piece of 256 at x4: one output pixel each side at 4 x, rounded outwards to 2 x
    assert _native.rcan_plan(_desc(s=4), 2048, 2048)[1:] == (64, 4 * (5 * 64 * 2048 * 2048 + 2 * 64 * (4 * 256 + 4) ** 2) + 8 * 64 * 64 + 4 * 64)
    # the plan does not depend on the depth or on the squeeze width
    assert _native.rcan_plan(_desc(64, 1, 16, 32, 2), 40, 70) == _native.rcan_plan(_desc(64, 64, 1, 0, 2), 40, 70)


def test_plan_and_create_refusals():
    for F, R, G, B, s in ((96, 4, 1, 1, 2), (48, 4, 1, 1, 2), (320, 4, 1, 1, 2), (64, 0, 1, 1, 2), (64, 65, 1, 1, 2), (64, 4, 0, 1, 2),
                          (64, 4, 17, 1, 2), (64, 4, 1, -1, 2), (64, 4, 1, 33, 2), (64, 4, 1, 1, 0), (64, 4, 1, 1, 5), (64, 4, 1, 1, 8)):
        with pytest.raises(NotImplementedError, match="is outside"):
            _native.rcan_plan(_desc(F, R, G, B, s), 100, 100)
    for kw in (dict(res_scale=float("nan")), dict(res_scale=float("inf")), dict(range=float("nan")), dict(mean=(0.0, float("inf"), 0.0)),
               dict(range=0.0)):
        with pytest.raises(NotImplementedError):
            _native.rcan_plan(_desc(**{"range": 1.0, **kw}), 100, 100)
    d = _desc(range=255.0)
    for args in ((100, 100, -1), (0, 100, 0), (100, 0, 0)):      # tail < 0, h / w < 1
        with pytest.raises(ValueError):
            _native.rcan_plan(d, *args)
    with pytest.raises(ValueError):                              # (2 h) x (2 w x 3) must fit int
        _native.rcan_plan(d, 3, 400_000_000)
    with pytest.raises(_native.SrShapeError, match="too large"):  # a plane beyond the kernels' 32-bit offsets
        _native.rcan_plan(d, 16400, 16400)
    with pytest.raises(_native.SrShapeError, match="rows"):       # more rows than one launch covers
        _native.rcan_plan(d, 300_000, 8)
    lib = _native.load()
    assert lib.sr_rcan_plan(None, 10, 10, 0, None, None, None) == _native.SR_ERR_INVALID_ARG            # null description
    assert lib.sr_rcan_plan(C.byref(d), 10, 10, 0, None, None, None) == _native.SR_OK                   # outputs may be NULL
    n = len(_native.rcan_conv_shapes(d))
    assert n == 9
    out = C.c_void_p()
    assert lib.sr_rcan_create(None, None, None, None, 0, C.byref(out)) == _native.SR_ERR_INVALID_ARG
    assert lib.sr_rcan_create(None, C.byref(d), None, None, n, None) == _native.SR_ERR_INVALID_ARG      # null out
    assert lib.sr_rcan_create(None, C.byref(d), None, None, n, C.byref(out)) == _native.SR_ERR_INVALID_ARG    # null tables
    tab = (C.c_void_p * n)()
    assert lib.sr_rcan_create(None, C.byref(d), tab, tab, n - 1, C.byref(out)) == _native.SR_ERR_INVALID_ARG  # a wrong n_tables
    assert f"{n} convolutions" in _native.last_error()
    assert lib.sr_rcan_create(None, C.byref(d), tab, tab, n, C.byref(out)) == _native.SR_ERR_INVALID_ARG      # null arrays
    assert lib.sr_rcan_create(None, C.byref(_desc(96)), None, None, n, C.byref(out)) == _native.SR_ERR_UNSUPPORTED
    assert lib.sr_rcan_create(None, C.byref(_desc(s=8)), None, None, n, C.byref(out)) == _native.SR_ERR_UNSUPPORTED
    for fn in (lib.sr_rcan_u8, lib.sr_rcan_f32):                 # null model
        assert fn(None, None, 0, 1, 1, None, 0, 0) == _native.SR_ERR_INVALID_ARG
    for fn in (lib.sr_rcan_ens_u8, lib.sr_rcan_ens_f32):
        assert fn(None, None, 0, 1, 1, None, 0, 0, 0) == _native.SR_ERR_INVALID_ARG                      # mask 0
        assert fn(None, None, 0, 1, 1, None, 0, -1, 1) == _native.SR_ERR_INVALID_ARG                     # tail < 0
        assert fn(None, None, 0, 1, 1, None, 0, 0, 1) == _native.SR_ERR_INVALID_ARG                      # null model
    assert lib.sr_rcan_destroy(None) == _native.SR_OK
    with pytest.raises(NotImplementedError):
        _native.RcanModel(None, _desc(96), [], [])                                  # refused before the context is looked at
    with pytest.raises(ValueError):
        _native.RcanModel(None, d, [], [])                                          # wrong number of arrays, before the context
    # sr_rcan_attention_f32: every argument is refused before the context is looked at
    w1, b1, w2, b2 = np.zeros((4, 64), np.float32), np.zeros(4, np.float32), np.zeros((64, 4), np.float32), np.zeros(64, np.float32)
    ok = dict(plane_stride=11 * 40 * 4, row_stride=40 * 4, n_feat=64, n_squeeze=4, h=11, w=37)
    for kw, exc in ((dict(n_feat=0), NotImplementedError), (dict(n_feat=257), NotImplementedError), (dict(n_squeeze=0), NotImplementedError),
                    (dict(n_squeeze=65), NotImplementedError), (dict(h=0), ValueError), (dict(w=0), ValueError), (dict(row_stride=36 * 4), ValueError),
                    (dict(plane_stride=10 * 40 * 4), ValueError), (dict(row_stride=40 * 4 + 2, plane_stride=11 * 40 * 4 + 24), ValueError)):
        a = {**ok, **kw}
        with pytest.raises(exc):
            _native.rcan_attention(None, 4096, a["plane_stride"], a["row_stride"], a["n_feat"], a["n_squeeze"], a["h"], a["w"], w1, b1, w2, b2)
    with pytest.raises(ValueError):
        _native.rcan_attention(None, 0, 11 * 40 * 4, 40 * 4, 64, 4, 11, 37, w1, b1, w2, b2)           # null tensor
    with pytest.raises(ValueError):
        _native.rcan_attention(None, 4098, 11 * 40 * 4, 40 * 4, 64, 4, 11, 37, w1, b1, w2, b2)        # misaligned tensor
    with pytest.raises(ValueError, match="w1"):
        _native.rcan_attention(None, 4096, 11 * 40 * 4, 40 * 4, 64, 4, 11, 37, w1[:3], b1, w2, b2)


def test_trunk_cap_message_names_the_largest_input():
    """The trunk is one piece of five F-plane buffers: 1280 bytes per pixel at F = 64, 16 GiB / 1280 = 13 421 772 pixels."""
    assert _native.rcan_plan(_desc(), 3600, 3600)[2] <= ref.TRUNK_CAP                   # 12.96 MP fits
    with pytest.raises(_native.SrShapeError) as e:
        _native.rcan_plan(_desc(), 4000, 4000)
    msg = str(e.value)
    assert "16 GiB" in msg and "F = 64" in msg and str((16 << 30) // 1280) in msg and "13.4 MP" in msg and "4000x4000" in msg
    with pytest.raises(_native.SrShapeError) as e:
        _native.rcan_plan(_desc(256, 16), 2048, 2048)
    assert str((16 << 30) // 5120) in str(e.value) and "F = 256" in str(e.value)
    assert _native.rcan_plan(_desc(256, 16), 1800, 1800)[2] <= ref.TRUNK_CAP + 2 * 256 * 4 * (2 * 258) ** 2 + (1 << 20)


@pytest.mark.parametrize("case", ref.CASES + ref.EDGE_CASES, ids=ref.case_id)
def test_documented_order_stays_inside_the_gpu_bar(case):
    """The accuracy bar of tests/test_gpu_rcan.py, err <= 8 e32, held against the documented order restated in numpy
    (ref.chain_forward): the order alone must fit the bar, or the bar says nothing about the kernels.  The u8 rule's exempt share
    stays under its 1 % cap, and the attention spreads."""
    F, R, G, B, s, h, w = case
    state, img, f64, e32 = ref.case(*case)
    chain, e_chain, rec = ref.chain_case(*case)
    assert chain.dtype == np.float32 and chain.shape == f64.shape == (h * s, w * s, 3)
    print(f"rcan chain {ref.case_id(case)}: e32 {e32:.3e}  e_chain {e_chain:.3e}  ratio {e_chain / e32:.3f}")
    assert 0 < e32 < 1e-4
    assert e_chain <= 8 * e32, (e_chain, e32, e_chain / e32)     # the documented order alone is inside the GPU bar
    share = ref.check_u8(ref.quantize(chain), f64, e32)          # ... and inside the u8 check with its 1 % exempt cap
    print(f"  u8 of the chain: exempt share {share:.4%}")
    assert len(rec) == G * B
    for sv in rec:                                               # s spreads over roughly 0.2 .. 0.8
        assert sv.shape == (F,) and 0.08 < sv.min() < 0.4 and 0.6 < sv.max() < 0.92, (float(sv.min()), float(sv.max()))


@pytest.mark.parametrize("mutant", ["padded-mean", "divisor", "shift-s", "no-res-scale"])
def test_the_cases_see_a_wrong_mean_a_wrong_s_and_a_dropped_res_scale(mutant):
    """A kernel that pools over the padded 8 x 32 blocks, divides by their pixel count, scales channel c by s[c - 1] or forgets
    res_scale must fail every case with more than one block: its float64 forward already misses the bar."""
    assert len(ref.MULTI_BLOCK_CASES) >= 5 and {(c[5], c[6]) for c in ref.MULTI_BLOCK_CASES} >= {(9, 33), (11, 37), (40, 70)}
    for case in ref.MULTI_BLOCK_CASES:
        state, img, f64, e32 = ref.case(*case)
        err = float(np.max(np.abs(ref.forward(state, img, "float64", mutant) - f64)))
        print(f"rcan mutant {mutant} {ref.case_id(case)}: err / e32 {err / e32:.1f}")
        assert err > 100 * 8 * e32, (mutant, case, err / e32)


@pytest.mark.parametrize("name", [n[0] for n in ref.EXACT_NETS] + [p[0] for p in ref.PROBES])
def test_exact_networks_and_probes_are_exact(name):
    """float64 == float32 == the documented order, bit for bit, and the reason: every value is a multiple of 2^-bits and the
    absolute-value forward (which bounds every partial sum in any order) stays below 2^24 of those units; s is 0.5 exactly."""
    state, img, chain = ref.exact_case(name)
    bits, bound, o64 = ref.exact_proof(state, img)
    print(f"rcan exact {name}: unit 2^-{bits}, bound {bound:.1f} = 2^{np.log2(bound) + bits:.2f} units")
    assert bound * 2.0 ** bits < 2 ** 24
    f64, f32 = ref.forward(state, img, "float64"), ref.forward(state, img, "float32")
    assert np.array_equal(f64, o64)
    assert np.array_equal(f32.astype(np.float64), f64) and np.array_equal(chain.astype(np.float64), f64)
    assert np.array_equal(f32.view(np.uint32), chain.view(np.uint32))
    assert len(np.unique(chain)) > 4 and (chain < 0).any() and (chain > 1).any()     # not degenerate; the u8 form clamps both ways


def test_probes_move_the_output():
    """What a probe is: against the same network with the probed permutation at the centre tap, the output differs."""
    for name, table, tap in ref.PROBES:
        state, img, chain = ref.exact_case(name)
        w = np.array(state[f"{table}.weight"])
        assert tap != 4 and w[:, :, tap // 3, tap % 3].sum() == w.sum() == w.shape[0]
        moved = {k: np.array(v) for k, v in state.items()}
        moved[f"{table}.weight"] = np.zeros_like(w)
        moved[f"{table}.weight"][:, :, 1, 1] = w[:, :, tap // 3, tap % 3]
        assert not np.array_equal(ref.chain_forward(moved, img), chain), name
    tables = {t for _, t, _ in ref.PROBES}
    assert {"body.0.residual_group.0.rcab.0", "body.0.residual_group.0.rcab.2", "body.0.conv", "body.1.conv", "upsample.0"} <= tables
