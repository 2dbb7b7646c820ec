"""CPU: the host side of the geometric self-ensemble (include/sr_hip.h, csrc/sr_ensemble.hip) -- the NumPy restatement of the
eight transforms, sr_ens_plan, every refusal of the new entry points (they are decided before the context is looked at, so a
null context reaches them on a machine without a GPU), the ``ensemble`` -> mask mapping and the pipeline's configuration
rules.  No device call is made here."""
import ctypes as C

import numpy as np
import pytest

import _ensemble_ref as E
import _native
import _srnet_ref as ref
import main as sr_main
import sr_network

INVALID, SHAPE = _native.SR_ERR_INVALID_ARG, _native.SR_ERR_SHAPE


def _image(h=5, w=7, c=3):
    return np.arange(h * w * c, dtype=np.int32).reshape(h, w, c)


def test_inverse_undoes_every_transform_on_a_non_square_image():
    x = _image()
    for k in range(8):
        t = E.d4(x, k)
        assert t.shape == ((7, 5, 3) if k & 4 else (5, 7, 3)), k
        assert np.array_equal(E.d4_inv(t, k), x), k
        assert np.array_equal(E.d4(E.d4_inv(t, k), k), t), k


def test_the_eight_transforms_are_distinct_and_t0_is_the_identity():
    x = _image(6, 6)                                              # square: every T_k(x) has one shape and can be compared
    ts = [E.d4(x, k) for k in range(8)]
    assert np.array_equal(ts[0], x)
    for a in range(8):
        for b in range(a + 1, 8):
            assert not np.array_equal(ts[a], ts[b]), (a, b)
    # the steps in the order of the definition: horizontal flip, vertical flip, transpose
    assert np.array_equal(ts[1], x[:, ::-1]) and np.array_equal(ts[2], x[::-1]) and np.array_equal(ts[4], x.transpose(1, 0, 2))
    assert np.array_equal(ts[5], x[:, ::-1].transpose(1, 0, 2)) and np.array_equal(ts[7], x[::-1, ::-1].transpose(1, 0, 2))
    # a group: the inverse of each member is a member (5 and 6 are each other's, the rest their own)
    inv = {k: next(j for j in range(8) if np.array_equal(E.d4(ts[k], j), x)) for k in range(8)}
    assert inv == {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}


def test_ensemble_restatement_order_and_division():
    x = ref.make_image(4, 6)
    fwd = lambda im: np.repeat(np.repeat(im.astype(np.float32) / np.float32(255.0), 2, 0), 2, 1) * np.float32(1.7) - np.float32(0.3)
    assert np.array_equal(E.ensemble(fwd, x, 1), fwd(x))
    for k in range(8):                                            # this forward commutes with the transforms
        assert np.array_equal(E.ensemble(fwd, x, 1 << k), fwd(x)), k
    o = E.ensemble(fwd, x, 0x07)
    assert o.dtype == np.float32 and np.array_equal(o, ((fwd(x) + fwd(x) + fwd(x)).astype(np.float32) / np.float32(3)))
    assert np.array_equal(E.to_u8(np.array([-1.0, 0.2 / 255, 1.6 / 255, 0.999, 7.0], np.float32)), [0, 0, 2, 255, 255])


@pytest.mark.parametrize("h,w,scale,mask,n", [
    (23, 37, 2, 0x01, 1), (23, 37, 2, 0x03, 2), (23, 37, 4, 0x0F, 4), (23, 37, 2, 0xFF, 8), (23, 37, 4, 0xA5, 4), (23, 37, 3, 0x07, 3),
    (37, 23, 2, 0x10, 1), (1, 1, 1, 0x80, 1), (2048, 2048, 4, 0xFF, 8), (100, 300, 1, 0x30, 2), (300, 100, 2, 0x02, 1),
])
def test_plan_members_and_workspace(h, w, scale, mask, n):
    assert _native.ens_plan(h, w, scale, mask) == (n, E.workspace_bytes(h, w, scale, mask))


def test_plan_workspace_spelled_out():
    # 23 x 37 at x2, all of D4: 46 x 74 accumulator rows of 888 -> 896 bytes; the forward output also 74 x 46 (552 -> 560);
    # the u8 input 23 rows of 111 -> 112 and 37 rows of 69 -> 80; every section rounded up to 256
    r256 = lambda v: (v + 255) // 256 * 256
    want = r256(46 * 896) + max(r256(46 * 896), r256(74 * 560)) + max(r256(23 * 112), r256(37 * 80))
    assert _native.ens_plan(23, 37, 2, 0xFF) == (8, want)
    # mask 1 transforms nothing: no u8 section
    assert _native.ens_plan(23, 37, 2, 0x01) == (1, 2 * r256(46 * 896))
    lib = _native.load()
    assert lib.sr_ens_plan(23, 37, 2, 0xFF, None, None) == _native.SR_OK          # outputs may be NULL


def test_plan_refusals():
    for mask in (0, 256, -1, 1 << 20):
        with pytest.raises(ValueError) as e:
            _native.ens_plan(10, 10, 2, mask)
        assert not isinstance(e.value, _native.SrShapeError)
    with pytest.raises(ValueError):
        _native.ens_plan(10, 10, 0, 1)
    for h, w in ((0, 10), (10, 0), (-3, 10)):
        with pytest.raises(_native.SrShapeError):
            _native.ens_plan(h, w, 2, 1)
    with pytest.raises(_native.SrShapeError):                     # (w s x 3) beyond int
        _native.ens_plan(100, 200_000_000, 4, 1)
    assert _native.ens_plan(200_000_000, 3, 4, 0x0F)[0] == 4      # 800 M rows of 12 pixels fit ...
    with pytest.raises(_native.SrShapeError):                     # ... but not transposed: 12 rows of 800 M pixels x 3
        _native.ens_plan(200_000_000, 3, 4, 0x10)
    with pytest.raises(ValueError):
        _native.ens_plan(10.5, 10, 2, 1)


A, B = 0x10000, 0x900000                                          # two made-up device addresses, far apart, never dereferenced


def _rc(name, *args):
    return getattr(_native.load(), name)(None, *args)             # null context: only reached when nothing is refused


def test_d4_u8_refusals_through_the_c_abi():
    ok = (C.c_void_p(A), 21, 5, 7, 3, C.c_void_p(B), 21)
    assert _rc("sr_d4_u8", *ok) == INVALID and "context" in _native.last_error()      # every argument passes; no context
    assert _rc("sr_d4_u8", None, 21, 5, 7, 3, C.c_void_p(B), 21) == INVALID and "null" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 3, None, 21) == INVALID
    for k in (-1, 8):
        assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, k, C.c_void_p(B), 21) == INVALID and "k" in _native.last_error()
    for h, w in ((0, 7), (5, 0), (-1, 7)):
        assert _rc("sr_d4_u8", C.c_void_p(A), 21, h, w, 3, C.c_void_p(B), 21) == SHAPE
    assert _rc("sr_d4_u8", C.c_void_p(A), 20, 5, 7, 3, C.c_void_p(B), 21) == SHAPE             # source stride < 7 x 3
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 3, C.c_void_p(B), 20) == SHAPE
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 4, C.c_void_p(B), 15) == INVALID           # transposed: rows of 5 x 3 are enough
    assert "context" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 4, C.c_void_p(B), 14) == SHAPE
    assert _rc("sr_d4_u8", C.c_void_p(A), -21, 5, 7, 0, C.c_void_p(B), 21) == SHAPE
    # overlap: the same buffer, the last byte of the source, the byte after it
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 1, C.c_void_p(A), 21) == INVALID and "overlap" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 1, C.c_void_p(A + 5 * 21 - 1), 21) == INVALID and "overlap" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A), 21, 5, 7, 1, C.c_void_p(A + 5 * 21), 21) == INVALID and "context" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A + 7 * 15), 21, 5, 7, 4, C.c_void_p(A), 15) == INVALID and "context" in _native.last_error()
    assert _rc("sr_d4_u8", C.c_void_p(A + 7 * 15 - 1), 21, 5, 7, 4, C.c_void_p(A), 15) == INVALID and "overlap" in _native.last_error()


def test_d4_acc_f32_refusals_through_the_c_abi():
    H, W = 5, 7
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, 3, 1, C.c_void_p(B), W * 12) == INVALID and "context" in _native.last_error()
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), H * 12, H, W, 5, 0, C.c_void_p(B), W * 12) == INVALID and "context" in _native.last_error()
    assert _rc("sr_d4_acc_f32", None, W * 12, H, W, 3, 1, C.c_void_p(B), W * 12) == INVALID and "null" in _native.last_error()
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, 3, 1, None, W * 12) == INVALID
    for k in (-1, 8):
        assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, k, 1, C.c_void_p(B), W * 12) == INVALID
    for h, w in ((0, W), (H, 0)):
        assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, h, w, 3, 1, C.c_void_p(B), W * 12) == SHAPE
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12 - 4, H, W, 3, 1, C.c_void_p(B), W * 12) == SHAPE
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, 3, 1, C.c_void_p(B), W * 12 - 4) == SHAPE
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), H * 12, H, W, 3, 1, C.c_void_p(B), W * 12) == SHAPE      # d_y is H x W for k = 3 ...
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12 - 4, H, W, 6, 1, C.c_void_p(B), W * 12) == INVALID  # ... W x H for k = 6
    assert "context" in _native.last_error()
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12 + 2, H, W, 3, 1, C.c_void_p(B), W * 12) == SHAPE  # fp32 stride not a multiple of 4
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, 3, 1, C.c_void_p(B), W * 12 + 3) == SHAPE
    assert _rc("sr_d4_acc_f32", C.c_void_p(A), W * 12, H, W, 3, 1, C.c_void_p(A + 4), W * 12) == INVALID and "overlap" in _native.last_error()


@pytest.mark.parametrize("name,px", [("sr_ens_finish_f32", 12), ("sr_ens_finish_u8", 3)])
def test_finish_refusals_through_the_c_abi(name, px):
    H, W = 5, 7
    assert _rc(name, C.c_void_p(A), W * 12, H, W, 3, C.c_void_p(B), W * px) == INVALID and "context" in _native.last_error()
    assert _rc(name, None, W * 12, H, W, 3, C.c_void_p(B), W * px) == INVALID and "null" in _native.last_error()
    assert _rc(name, C.c_void_p(A), W * 12, H, W, 3, None, W * px) == INVALID
    for n in (0, 9, -1):
        assert _rc(name, C.c_void_p(A), W * 12, H, W, n, C.c_void_p(B), W * px) == INVALID and "n " in _native.last_error()
    for h, w in ((0, W), (H, 0)):
        assert _rc(name, C.c_void_p(A), W * 12, h, w, 3, C.c_void_p(B), W * px) == SHAPE
    assert _rc(name, C.c_void_p(A), W * 12 - 4, H, W, 3, C.c_void_p(B), W * px) == SHAPE
    assert _rc(name, C.c_void_p(A), W * 12, H, W, 3, C.c_void_p(B), W * px - 1) == SHAPE
    assert _rc(name, C.c_void_p(A), W * 12 + 1, H, W, 3, C.c_void_p(B), W * px) == SHAPE
    if px == 12:
        assert _rc(name, C.c_void_p(A), W * 12, H, W, 3, C.c_void_p(B), W * px + 2) == SHAPE
    else:
        assert _rc(name, C.c_void_p(A), W * 12, H, W, 3, C.c_void_p(B), W * px + 2) == INVALID and "context" in _native.last_error()


@pytest.mark.parametrize("kind,extra", [("srnet", (0,)), ("resnet", (0,)), ("rrdb", (0, 0))])
def test_model_entry_points_refuse_the_mask_and_a_null_model(kind, extra):
    lib = _native.load()
    for form, px in (("u8", 3), ("f32", 12)):
        fn = getattr(lib, f"sr_{kind}_ens_{form}")
        for mask in (0, 256, -7):
            assert fn(None, C.c_void_p(A), 21, 5, 7, C.c_void_p(B), 7 * 4 * px, *extra, mask) == INVALID and "mask" in _native.last_error()
        assert fn(None, C.c_void_p(A), 21, 5, 7, C.c_void_p(B), 7 * 4 * px, *extra, 0xFF) == INVALID and "model" in _native.last_error()
        neg = tuple(-1 for _ in extra)
        assert fn(None, C.c_void_p(A), 21, 5, 7, C.c_void_p(B), 7 * 4 * px, *neg, 0xFF) == INVALID and "tile" in _native.last_error()


def test_refusals_through_the_python_wrappers():
    with pytest.raises(ValueError, match="k "):
        _native.d4_u8(None, A, 21, 5, 7, 8, B, 21)
    with pytest.raises(_native.SrShapeError):
        _native.d4_u8(None, A, 20, 5, 7, 1, B, 21)
    with pytest.raises(ValueError, match="overlap"):
        _native.d4_u8(None, A, 21, 5, 7, 1, A + 3, 21)
    with pytest.raises(ValueError, match="null"):
        _native.d4_u8(None, 0, 21, 5, 7, 1, B, 21)
    with pytest.raises(ValueError, match="context"):              # nothing to refuse: the null context is what is left
        _native.d4_u8(None, A, 21, 5, 7, 1, B, 21)
    with pytest.raises(ValueError):
        _native.d4_u8(None, A, 21, 5, 7, 1.5, B, 21)
    with pytest.raises(ValueError, match="k "):
        _native.d4_acc_f32(None, A, 84, 5, 7, -1, True, B, 84)
    with pytest.raises(_native.SrShapeError):
        _native.d4_acc_f32(None, A, 84, 5, 7, 2, True, B, 86)
    with pytest.raises(_native.SrShapeError):
        _native.d4_acc_f32(None, A, 84, 0, 7, 2, False, B, 84)
    for u8 in (False, True):
        with pytest.raises(ValueError, match="n "):
            _native.ens_finish(None, A, 84, 5, 7, 9, B, 84, u8)
        with pytest.raises(_native.SrShapeError):
            _native.ens_finish(None, A, 80, 5, 7, 2, B, 84, u8)
        with pytest.raises(ValueError, match="null"):
            _native.ens_finish(None, A, 84, 5, 7, 2, 0, 84, u8)


def test_ensemble_to_mask_mapping():
    assert sr_network.ENSEMBLE_MASKS == {1: 0x01, 2: 0x03, 4: 0x0F, 8: 0xFF}
    assert [sr_network.ensemble_mask(e) for e in (1, 2, 4, 8)] == [1, 3, 15, 255]
    assert sr_network.ensemble_mask(np.int64(4)) == 15
    for e in (1, 2, 4, 8):
        assert _native.ens_plan(8, 8, 2, sr_network.ensemble_mask(e))[0] == e
    for bad in (0, 3, 5, 6, 7, 16, -1, 255, True, 2.0, "8", None):
        with pytest.raises(ValueError):
            sr_network.ensemble_mask(bad)


def test_network_refuses_a_bad_ensemble_before_any_device_call(monkeypatch):
    """upscale / upscale_device raise on the value alone: the model (a device object) is never asked for."""
    nets = [sr_network.CompactSRNet(ref.synthetic_state(64, 1, 2))]
    import _resnet_ref
    import _rrdb_ref
    nets.append(sr_network.ResidualSRNet(_resnet_ref.synthetic_state("msr", 64, 1, 2)))
    nets.append(sr_network.RRDBSRNet(_rrdb_ref.synthetic_state(64, 32, 1)))
    img = ref.make_image(8, 9)
    for net in nets:
        def no_model(ctx=None):
            raise AssertionError("a device object was asked for")
        monkeypatch.setattr(net, "model", no_model)
        monkeypatch.setattr(_native, "default_context", no_model)
        for bad in (0, 3, 16, True, "2"):
            with pytest.raises(ValueError, match="ensemble"):
                net.upscale(img, ensemble=bad)
            with pytest.raises(ValueError, match="ensemble"):
                net.upscale_device(A, (8, 9, 3), B, 54, ensemble=bad)


def test_pipeline_config_rules(tmp_path):
    assert sr_main.PipelineConfig().sr_ensemble == 1
    wpath = str(tmp_path / "net.npz")
    np.savez(wpath, **ref.synthetic_state(64, 1, 2))
    for e in (1, 2, 4, 8):
        pipe = sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, sr_scale=2, sr_ensemble=e))
        assert pipe.sr_net is not None and pipe.config.sr_ensemble == e and pipe._builtin_backend()
    for e in (2, 4, 8):
        with pytest.raises(ValueError, match="sr_weights"):      # the bicubic stub has nothing to ensemble
            sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_ensemble=e))
    for bad in (0, 3, 16, -2):
        with pytest.raises(ValueError, match="ensemble"):
            sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_weights=wpath, sr_scale=2, sr_ensemble=bad))
        with pytest.raises(ValueError):
            sr_main.SuperResolutionPipeline(sr_main.PipelineConfig(sr_ensemble=bad))
    sr_main.SuperResolutionPipeline(sr_main.PipelineConfig())    # the default needs no weights
