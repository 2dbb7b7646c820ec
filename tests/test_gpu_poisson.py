"""GPU: the Poisson solver and the seam-repair helpers of csrc/sr_poisson.hip against the NumPy / SciPy restatement
(tests/_poisson_ref.py), and BlendingModule.poisson_fusion / repair_seams end to end.

Solver bounds: every byte within 1 level of the float64 restatement (a condition); the number of bytes that differ at all is
held to 8x the number the same restatement shows when evaluated in float32 on the same input, with a floor of 16 -- the rule
and margin tests/test_gpu_content.py uses for the same FFT engine (the device FFT mixes radices and Bluestein with fp32
twiddles where pocketfft is one fp32 algorithm).  The blur, the resize and the fallback are integer / NumPy arithmetic on both
sides: byte-equal.  Region SSIM: exact integer moments, so 1e-12 against the float64 formula."""
import numpy as np
import pytest

import _native
import _poisson_ref as R
import blending_module as bm
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

MODES = [R.NORMAL, R.MIXED, R.MONOCHROME]


def _clone(ctx, dest, patch, mask, mode):
    h, w = mask.shape
    bufs = [ctx.upload(dest), ctx.upload(patch), ctx.upload(mask), ctx.alloc(h * w * 3)]
    try:
        ctx.poisson_clone_u8(bufs[0].ptr, w * 3, bufs[1].ptr, w * 3, bufs[2].ptr, w, h, w, mode, bufs[3].ptr, w * 3)
        return ctx.download(bufs[3].ptr, (h, w, 3), np.uint8)
    finally:
        ctx.sync()
        for b in bufs:
            b.free()


def _within_one(got, want, what):
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: max |diff| {int(diff.max())}, differing {int(np.count_nonzero(diff))} of {diff.size}")
    assert int(diff.max()) <= 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", R.SOLVER_CASES)
def test_solver_matches_restatement(ctx, h, w, mode):
    dest, patch, mask = R.solver_inputs(h, w)
    want = R.clone(dest, patch, mask, mode, np.float64)
    f32 = R.clone(dest, patch, mask, mode, np.float32)
    got = _clone(ctx, dest, patch, mask, mode)
    assert float(np.mean(want != dest)) > 0.2                        # the clone does something
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    n_diff, n_f32 = int(np.count_nonzero(diff)), int(np.count_nonzero(f32 != want))
    allowed = max(8.0 * n_f32, 16.0)
    print(f"poisson {h}x{w} mode {mode}: max |diff| {int(diff.max())}, differing {n_diff} bytes (share {n_diff / diff.size:.3g}), "
          f"float32 restatement {n_f32} bytes (share {n_f32 / diff.size:.3g}), allowed {allowed:.0f}")
    assert int(diff.max()) <= 1
    assert n_diff <= allowed
    assert np.array_equal(got[0], dest[0]) and np.array_equal(got[-1], dest[-1])        # the frame is the destination's
    assert np.array_equal(got[:, 0], dest[:, 0]) and np.array_equal(got[:, -1], dest[:, -1])
    assert np.array_equal(_clone(ctx, dest, patch, mask, mode), got)                     # two calls, identical bytes


@pytest.mark.parametrize("h,w", R.SOLVER_CASES + [(4124, 2970)])
def test_cloning_the_destination_onto_itself_changes_nothing(ctx, h, w):
    dest, _, mask = R.solver_inputs(h, w)
    for mode in (R.NORMAL, R.MIXED):
        assert np.array_equal(_clone(ctx, dest, dest, mask, mode), dest)
    gray = np.repeat(R.rgb2gray(dest)[..., None], 3, axis=2)
    assert np.array_equal(_clone(ctx, gray, gray, mask, R.MONOCHROME), gray)


def test_zero_mask_and_degenerate_sizes_return_the_destination(ctx):
    dest, patch, mask = R.solver_inputs(120, 90)
    for mode in MODES:
        assert np.array_equal(_clone(ctx, dest, patch, np.zeros_like(mask), mode), dest)
    for h, w in ((1, 1), (2, 40), (40, 2), (3, 3)):
        d, p, m = R.solver_inputs(h, w)
        m[:] = 255
        assert np.array_equal(_clone(ctx, d, p, m, R.NORMAL), R.clone(d, p, m, R.NORMAL))
    with pytest.raises(ValueError):
        _clone(ctx, dest, patch, mask, 4)


def test_poisson_fusion_end_to_end(ctx):
    b = bm.BlendingModule()
    dst = R.synth(200, 260, 1)
    src = np.clip(R.synth(90, 120, 2).astype(int) + 25, 0, 255).astype(np.uint8)
    # default mask and centre
    _within_one(b.poisson_fusion(src, dst), R.poisson_fusion(src, dst), "default mask and centre")
    # an off-centre blob, every mode
    yy, xx = np.mgrid[0:90, 0:120]
    blob = (((xx - 80) / 30.0) ** 2 + ((yy - 30) / 22.0) ** 2 <= 1).astype(np.uint8) * 255
    for mode in bm.PoissonMode:
        got = b.poisson_fusion(src, dst, blob, (70, 150), mode)
        _within_one(got, R.poisson_fusion(src, dst, blob, (70, 150), mode.value), f"blob, {mode.name}")
        assert not np.array_equal(got, dst)
    # float inputs and a float mask
    fs, fd = src.astype(np.float32) * 1.2 - 10.5, dst.astype(np.float64) + 0.4
    _within_one(b.poisson_fusion(fs, fd, blob.astype(np.float32) / 255), R.poisson_fusion(fs, fd, blob.astype(np.float32) / 255),
                "float inputs")
    # roi_d outside the destination: the host blend on both sides
    assert np.array_equal(b.poisson_fusion(src, dst, blob, (5, 5)), R.poisson_fusion(src, dst, blob, (5, 5)))


@pytest.mark.parametrize("h,w,cn", [(97, 130, 3), (64, 64, 1), (40, 51, 4), (9, 80, 3), (30, 5, 1), (1, 1, 3), (14, 14, 4)])
def test_blur_is_byte_equal(ctx, h, w, cn):
    img = np.random.default_rng(h * w).integers(0, 256, (h, w, cn), dtype=np.uint8)
    img = img[..., 0] if cn == 1 else img
    d_in, d_out = ctx.upload(img), ctx.alloc(img.size)
    try:
        ctx.gaussian_blur15_u8(d_in.ptr, w * cn, h, w, cn, d_out.ptr, w * cn)
        assert np.array_equal(ctx.download(d_out.ptr, img.shape, np.uint8), R.gaussian_blur15(img))
        ctx.gaussian_blur15_u8(d_in.ptr, w * cn, h, w, cn, d_in.ptr, w * cn)             # in place
        assert np.array_equal(ctx.download(d_in.ptr, img.shape, np.uint8), R.gaussian_blur15(img))
    finally:
        ctx.sync()
        d_in.free()
        d_out.free()


def test_region_ssim_and_linear_resize(ctx):
    rng = np.random.default_rng(8)
    for (h, w, cn), (dh, dw) in [((120, 170, 3), (77, 201)), ((50, 40, 1), (50, 40)), ((33, 90, 3), (131, 17)), ((256, 256, 4), (100, 300))]:
        img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
        img = img[..., 0] if cn == 1 else img
        d_in, d_out = ctx.upload(img), ctx.alloc(dh * dw * cn)
        try:
            ctx.resize_linear_u8(d_in.ptr, w * cn, h, w, cn, d_out.ptr, dw * cn, dh, dw)
            got = ctx.download(d_out.ptr, (dh, dw) if cn == 1 else (dh, dw, cn), np.uint8)
            want = onp.resize_linear_u8(img, dw, dh)
            assert np.array_equal(got, want)
            if cn != 4:
                other = np.clip(want.astype(int) + rng.integers(-30, 31, want.shape), 0, 255).astype(np.uint8)
                d_o = ctx.upload(other)
                try:
                    s = ctx.region_ssim_u8(d_out.ptr, dw * cn, d_o.ptr, dw * cn, dh, dw, cn)
                finally:
                    d_o.free()
                assert abs(s - R.region_ssim(want, other)) <= 1e-12
        finally:
            ctx.sync()
            d_in.free()
            d_out.free()


def _fused_canvas():
    """A 1230 x 820 canvas fused from a 2 x 2 grid with one tile brightened."""
    H, W, th, tw = 820, 1230, 450, 680
    base = R.synth(H, W, 7)
    pos = [(0, 0), (W - tw, 0), (0, H - th), (W - tw, H - th)]
    tiles = [np.ascontiguousarray(base[y:y + th, x:x + tw]) for (x, y) in pos]
    tiles[3] = np.clip(tiles[3].astype(int) * 1.25 + 30, 0, 255).astype(np.uint8)
    b = bm.BlendingModule(ssim_threshold=0.95)
    infos = [bm.TileInfo(t, x, y, i // 2, i % 2) for i, (t, (x, y)) in enumerate(zip(tiles, pos))]
    canvas = b.laplacian_fusion(infos, output_shape=(H, W))
    return b, canvas, infos, tiles


def _disjoint(seams, shape, limit, max_side=96):
    """Seams whose padded boxes do not overlap (greedy, list order), at most `limit` per method.  Seams longer than
    max_side are left out: the saturated canvas perimeter merges into seams whose padded box is the whole canvas."""
    taken, out, count = [], [], {}
    for s in seams:
        if s.suggested_fix == "none" or count.get(s.suggested_fix, 0) >= limit or max(s.width, s.height) > max_side:
            continue
        xa, ya, xb, yb = R.padded_box(s, shape)
        if any(xa < X2 and X1 < xb and ya < Y2 and Y1 < yb for (X1, Y1, X2, Y2) in taken):
            continue
        taken.append((xa, ya, xb, yb))
        out.append(s)
        count[s.suggested_fix] = count.get(s.suggested_fix, 0) + 1
    return out, taken


def test_repair_seams_on_a_fused_canvas(ctx):
    b, canvas, infos, tiles = _fused_canvas()
    found = b.detect_seams(canvas, infos)
    sev = {s.severity for s in found}
    assert "high" in sev and "medium" in sev, sev
    seams, boxes = _disjoint(found, canvas.shape, 6)
    assert {s.suggested_fix for s in seams} == {"poisson_refinement", "increase_blend_width"}
    got = b.repair_seams(canvas, seams, tiles)
    want = R.repair_seams(canvas, seams, tiles)
    outside = np.ones(canvas.shape[:2], bool)
    for s, (xa, ya, xb, yb) in zip(seams, boxes):
        outside[ya:yb, xa:xb] = False
        if s.suggested_fix == "increase_blend_width":
            assert np.array_equal(got[ya:yb, xa:xb], want[ya:yb, xa:xb])
        else:
            _within_one(got[ya:yb, xa:xb], want[ya:yb, xa:xb], f"poisson box {xb - xa}x{yb - ya}")
        assert not np.array_equal(got[ya:yb, xa:xb], canvas[ya:yb, xa:xb])
    assert np.array_equal(got[outside], canvas[outside])
    # the whole list, overlapping boxes included: no more high-severity seams than before
    repaired = b.repair_seams(canvas, found, tiles)
    before = sum(s.severity == "high" for s in found)
    after = sum(s.severity == "high" for s in b.detect_seams(repaired, infos))
    print(f"high-severity seams: {before} before, {after} after repair")
    assert after <= before


def test_repair_seams_overlapping_blurs_are_ordered(ctx):
    b = bm.BlendingModule()
    img = R.synth(300, 420, 9)
    seams = [bm.Seam(100, 90, 32, 16, 0.9), bm.Seam(140, 100, 16, 48, 0.88), bm.Seam(0, 280, 64, 16, 0.9),
             bm.Seam(150, 120, 16, 16, 0.99), bm.Seam(400, 0, 16, 16, 0.86)]
    got = b.repair_seams(img, seams, [img])
    assert np.array_equal(got, R.repair_seams(img, seams, [img]))
    assert not np.array_equal(got, R.repair_seams(img, seams[::-1], [img]))
    assert np.array_equal(b.repair_seams(img, seams, [img], "increase_blend_width"),
                          R.repair_seams(img, seams, [img], "increase_blend_width"))
