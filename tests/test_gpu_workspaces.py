"""GPU: the grow-only device buffers (DevBuf) and the per-call temporaries (DevTemp) of csrc/sr_ctx.h.

Every case makes its own context: the session fixture's buffers have been grown by other tests.  A case runs small, large,
small on ONE context (first allocation, regrow, reuse of the larger buffer) and compares each result, bit for bit, with the
same call on a fresh context that has seen only that shape.  What a regrow could break: a result read from the freed buffer,
a cached table whose host shadow survives its device buffer, planes kept for a later call that the regrow threw away."""
import numpy as np
import pytest

import _qmap_ref as R
from oracle import lpips_oracle as lo

pytestmark = pytest.mark.gpu


def _img(h, w, cn=3, salt=0):
    return np.random.default_rng(20261019 + 7919 * h + 31 * w + cn + 101 * salt).integers(0, 256, (h, w, cn) if cn > 1 else (h, w),
                                                                                         dtype=np.uint8)


def _same(got, want, what):
    if isinstance(got, dict):
        assert got.keys() == want.keys(), what
        for k in got:
            _same(got[k], want[k], f"{what}[{k!r}]")
    elif isinstance(got, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{what}[{i}]")
    elif isinstance(got, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        if got.dtype.names:                                  # records: every byte
            assert got.tobytes() == want.tobytes(), what
        else:
            assert np.array_equal(got, want), what
    else:
        assert got == want, (what, got, want)


def _sequence(steps, setup=None):
    """steps: [(call, shape)], call(ctx, state, shape) -> result; state = setup(ctx) (closed at the end when it can be)."""
    import _native

    def fresh():
        c = _native.Context(0)
        return c, (setup(c) if setup else None)

    def close(c, state):
        if state is not None:
            state.close()
        c.close()

    ctx, state = fresh()
    try:
        for i, (call, shape) in enumerate(steps):
            got = call(ctx, state, shape)
            c2, s2 = fresh()
            try:
                want = call(c2, s2, shape)
            finally:
                close(c2, s2)
            _same(got, want, f"step {i} {call.__name__}{shape}")
    finally:
        close(ctx, state)


def _pair_call(fn):
    """call(ctx, state, (h, w, cn)) that uploads a seeded pair and returns fn(ctx, state, da, db, h, w, cn)."""
    def call(ctx, state, shape):
        h, w, cn = shape
        da, db = ctx.upload(_img(h, w, cn)), ctx.upload(_img(h, w, cn, salt=1))
        try:
            return fn(ctx, state, da, db, h, w, cn)
        finally:
            da.free(); db.free()
    call.__name__ = fn.__name__
    return call


def _small_large_small(call, small, large, setup=None):
    _sequence([(call, small), (call, large), (call, small)], setup)


# ---- the context's buffers -----------------------------------------------------------------------------------------------

def test_scratch_floor_then_regrow():
    """histogram_u8 takes the 1 MiB floor, the assessment's 8 MiB request regrows it, histogram_u8 then runs in the larger one."""
    @_pair_call
    def histogram(ctx, _, da, db, h, w, cn):
        return ctx.histogram_u8(da.ptr, w * cn, h, w, cn)

    @_pair_call
    def assess(ctx, _, da, db, h, w, cn):
        return ctx.assess_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn)

    _sequence([(histogram, (24, 32, 3)), (assess, (24, 32, 3)), (histogram, (24, 32, 3))])


def test_gray_planes():
    @_pair_call
    def assess_resized(ctx, _, da, db, h, w, cn):
        import _native
        return ctx.assess_resized_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, h // 2, w // 2, flags=_native.ASSESS_ALL)

    _small_large_small(assess_resized, (24, 32, 3), (96, 128, 3))


def test_commercial_workspace():
    @_pair_call
    def commercial(ctx, _, da, db, h, w, cn):
        return ctx.commercial_u8(da.ptr, w * cn, h, w, cn, 4095)

    _small_large_small(commercial, (32, 32, 3), (96, 96, 3))


def test_msssim_workspace_and_kept_planes():
    import _native
    side = next(s for s in range(1, 1024) if _plan_ok(_native.ms_ssim_plan, s, s, 5))
    assert not _plan_ok(_native.ms_ssim_plan, side - 1, side, 5) and not _plan_ok(_native.ms_ssim_plan, side, side - 1, 5)

    @_pair_call
    def ms_ssim(ctx, _, da, db, h, w, cn):
        levels = ctx.ms_ssim_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, levels=5)
        return levels, ctx.ms_ssim_planes(1, _native.ms_ssim_plan(h, w, 5)["sizes"][1])

    _small_large_small(ms_ssim, (side, side, 3), (2 * side, 2 * side, 3))


def _plan_ok(plan, *args):
    try:
        plan(*args)
        return True
    except ValueError:
        return False


def test_srbench_workspace():
    @_pair_call
    def bench(ctx, _, da, db, h, w, cn):
        import _native
        return ctx.bench_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, mode=_native.BENCH_Y)

    _small_large_small(bench, (24, 32, 3), (96, 128, 3))


def test_niqe_workspace_and_kept_half_plane():
    import _native
    side = next(s for s in range(1, 1024) if _plan_ok(_native.niqe_plan, s, s, 3))
    assert not _plan_ok(_native.niqe_plan, side - 1, side, 3) and not _plan_ok(_native.niqe_plan, side, side - 1, 3)

    @_pair_call
    def niqe(ctx, _, da, db, h, w, cn):
        rec = ctx.niqe_u8(da.ptr, w * cn, h, w, cn)
        H, W = _native.niqe_plan(h, w, cn)["size"]
        return rec, ctx.niqe_half_plane((H // 2, W // 2))

    _small_large_small(niqe, (side, side, 3), (2 * side, 2 * side, 3))


def test_cached_table_shadow_after_regrow():
    """resize_cubic_u8's tables live in a CachedTable: the larger table regrows it, and the small table, identical to the
    shadow of before the regrow, must be uploaded again."""
    @_pair_call
    def resize(ctx, _, da, db, h, w, cn):
        out = ctx.alloc((h // 2) * (w // 2) * cn)
        try:
            ctx.resize_cubic_u8(da.ptr, w * cn, h, w, cn, out.ptr, (w // 2) * cn, h // 2, w // 2)
            return ctx.download(out.ptr, (h // 2, w // 2, cn), np.uint8)
        finally:
            out.free()

    _small_large_small(resize, (16, 16, 3), (64, 64, 3))


# ---- the models' buffers -------------------------------------------------------------------------------------------------

_LPIPS_WEIGHTS = {}


@pytest.mark.parametrize("tile", [0, 64], ids=["untiled", "tile64"])
@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_lpips_buffers(net, tile):
    import _native
    if net not in _LPIPS_WEIGHTS:
        _LPIPS_WEIGHTS[net] = lo.synthetic_weights(net)

    @_pair_call
    def layer_sums(ctx, model, da, db, h, w, cn):
        return model.layer_sums(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, tile=tile)

    _small_large_small(layer_sums, (33, 47, 3), (96, 160, 3), setup=lambda c: _native.LpipsModel(c, net, _LPIPS_WEIGHTS[net]))


@pytest.mark.parametrize("tile", [0, 64], ids=["untiled", "tile64"])
def test_dists_buffers(tile):
    import _native
    if "dists" not in _LPIPS_WEIGHTS:
        _LPIPS_WEIGHTS["dists"] = _native.dists_synthetic_weights()

    @_pair_call
    def sums(ctx, model, da, db, h, w, cn):
        return model.sums(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, tile)

    _small_large_small(sums, (33, 47, 3), (96, 160, 3), setup=lambda c: _native.DistsModel(c, _LPIPS_WEIGHTS["dists"]))


# ---- per-call temporaries ------------------------------------------------------------------------------------------------

def test_per_call_temporaries():
    """Every entry point that allocates for one call, twice with two shapes on one context: the second call's temporary
    must not depend on what the first one left behind (freed after the stream has drained, on every return path)."""
    import _native
    base = np.arange(256, dtype=np.float32)
    int_table = np.repeat(np.clip(np.rint(base * 0.9 + 10.0), 0, 255)[None, :], 3, 0)
    float_table = np.repeat(((base - np.float32(140.25)) * np.float32(2.5) + np.float32(100.5))[None, :], 3, 0)
    assert _native.color_table_class(int_table) == 1 and _native.color_table_class(float_table) == 2

    def color_correct(table, local_filter, radius):
        @_pair_call
        def run(ctx, _, da, db, h, w, cn):
            out = ctx.alloc(h * w * cn)
            try:
                ctx.color_correct_u8(da.ptr, w * cn, h, w, cn, table, local_filter, radius, 0.01, out.ptr, w * cn)
                return ctx.download(out.ptr, (h, w, cn), np.uint8)
            finally:
                out.free()
        run.__name__ = f"color_correct(filter {local_filter}, radius {radius})"
        return run

    def ssim_float(ctx, _, shape):
        h, w = shape
        a = _img(h, w, 1).astype(np.float32) * np.float32(0.9) + np.float32(3.3)
        b = _img(h, w, 1, salt=1).astype(np.float32) * np.float32(1.02)
        da, db = ctx.upload(a), ctx.upload(b)
        try:
            return ctx.ssim_float(da.ptr, w * 4, db.ptr, w * 4, h, w, 1, _native.SR_F32, "gauss")
        finally:
            da.free(); db.free()

    def quality_map(ctx, _, shape):
        h, w, cn, cell = shape
        da, db = ctx.upload(_img(h, w, cn)), ctx.upload(_img(h, w, cn, salt=1))
        try:
            return ctx.quality_map_u8(da.ptr, w * cn, db.ptr, w * cn, h, w, cn, R.uniform_edges(w, cell), R.uniform_edges(h, cell))
        finally:
            da.free(); db.free()

    def fusion(ctx, _, shape):
        th, tw, rows, cols, ov, levels, wt = shape
        tiles = [_img(th, tw, 3, salt=i) for i in range(rows * cols)]
        pos = [((i // cols) * (th - ov), (i % cols) * (tw - ov)) for i in range(rows * cols)]
        canvas = (rows * th - (rows - 1) * ov, cols * tw - (cols - 1) * ov)
        return ctx.fusion_np(tiles, pos, canvas, levels, wt, laplacian=True, return_float=True)

    small = [(16, 16, 3), (17, 64, 3)]
    steps = []
    for call in (color_correct(int_table, 2, 8), color_correct(float_table, 2, 8), color_correct(int_table, 1, 5)):
        steps += [(call, s) for s in small]
    steps += [(ssim_float, (90, 120)), (ssim_float, (97, 131))]
    steps += [(quality_map, (23, 29, 3, 4)), (quality_map, (97, 131, 3, 16))]
    steps += [(fusion, (64, 64, 1, 3, 16, 6, "linear")), (fusion, (40, 200, 2, 1, 8, 1, "cosine"))]
    _sequence(steps)
