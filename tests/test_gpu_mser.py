"""GPU: MSER text regions (csrc/sr_mser.hip) against the Python restatement (tests/_mser_ref.py) and, at the size Python is
too slow for, against the host restatement sr_mser_host_u8.  Records and node tables are compared for EQUALITY: every field
is an integer and the tree is a property of the image.  The unions are not tiled (one launch per level over the level's pixel
list), so there are no tile seams to walk; the shapes are the smallest at which each mechanism can fail: single pixels and
lines, one level / one root (the contention case), N / 2 singletons merging in one level, a chain of 256 nested nodes, the
longest find path, late joins, noise, and the two text fixtures of the definition."""
import functools

import numpy as np
import pytest

import _content_ref as CR
import _mser_ref as R
import _native
import _views as V
import tiling_module as tm

pytestmark = pytest.mark.gpu

CASES = R.gpu_cases()


def as_rows(recs):
    """A structured array of the C ABI as an int64 matrix."""
    return np.stack([recs[f].astype(np.int64) for f in recs.dtype.names], axis=1) if len(recs) else np.zeros((0, 9), np.int64)


def want_regions(g, mask=3, **params):
    r = R.regions(g, polarity_mask=mask, **params)
    return np.array(r, dtype=np.int64).reshape(-1, 9)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    g, params = CASES[name]
    return want_regions(g, **params), [R.node_table(R.tree(g)), R.node_table(R.tree(255 - g))]


def gpu_regions(ctx, img, mask=3, **params):
    img = np.ascontiguousarray(img)
    cn = img.shape[2] if img.ndim == 3 else 1
    d = ctx.upload(img)
    try:
        return as_rows(ctx.mser(d.ptr, img.shape[1] * cn, img.shape[0], img.shape[1], cn, _native.mser_params(**params), mask))
    finally:
        d.free()


def gpu_tree(ctx, img, polarity):
    img = np.ascontiguousarray(img)
    cn = img.shape[2] if img.ndim == 3 else 1
    d = ctx.upload(img)
    try:
        return as_rows(ctx.mser_tree(d.ptr, img.shape[1] * cn, img.shape[0], img.shape[1], cn, polarity))
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_regions_and_tree_equal_restatement(ctx, name):
    g, params = CASES[name]
    want, trees = case_reference(name)
    got = gpu_regions(ctx, g, **params)
    print(f"{name}: {g.shape}, {len(trees[0])} dark / {len(trees[1])} bright nodes, {len(want)} regions")
    assert np.array_equal(got, want)
    for pol in (0, 1):
        assert np.array_equal(gpu_tree(ctx, g, pol), trees[pol])


def test_flat_image_is_one_region_and_no_text_box(ctx):
    got = gpu_regions(ctx, CASES["flat64"][0])
    assert got.tolist() == [[0, 128, 4096, 0, 0, 63, 63, 0, 4096], [1, 127, 4096, 0, 0, 63, 63, 0, 4096]]
    assert tm.MserTextDetector()(CASES["flat64"][0]) == []


def test_text_fixture(ctx):
    g = CASES["text"][0]
    want, trees = case_reference("text")
    assert len(trees[0]) == 4721 and len(want) == 10 and set(want[:, 0]) == {0}      # what the restatement gives
    det = tm.MserTextDetector()
    regs = det.regions(g)
    assert regs.dtype == _native.MSER_REGION_DTYPE and np.array_equal(as_rows(regs), want)
    boxes = det(g)
    assert boxes == R.text_boxes([tuple(r) for r in want.tolist()], g.shape[1])
    sizes = sorted((w, h) for _, _, w, h in boxes)
    assert sizes == [(22, 12)] * 5 + [(30, 20)] * 5
    for bx, by, bw, bh in R.TEXT_BARS:                                                 # every bar lies inside a returned box
        assert any(x <= bx and y <= by and x + w >= bx + bw and y + h >= by + bh for x, y, w, h in boxes)


def test_nested_flat_keeps_glyphs_panel_and_page(ctx):
    got = gpu_regions(ctx, CASES["nested"][0], mask=1)
    assert got[:, 2].tolist() == [384, 384, 384, 384, 8400, 12800]                     # the tie rule: nobody is knocked out
    assert np.array_equal(got, want_regions(CASES["nested"][0], mask=1))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_channel_counts(ctx, rng, cn):
    img = rng.integers(0, 256, size=(37, 53, cn)).astype(np.uint8)
    img[8:30, 10:40] //= 8                                                             # a dark patch on noise
    got = gpu_regions(ctx, img if cn > 1 else img[..., 0], min_area=1)
    assert np.array_equal(got, want_regions(R.gray_swapped(img), min_area=1))
    if cn == 4:
        other = img.copy()
        other[..., 3] ^= 0xFF
        assert np.array_equal(gpu_regions(ctx, other, min_area=1), got)                # alpha is ignored


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_polarity_masks(ctx, mask):
    g = CASES["noise"][0]
    got = gpu_regions(ctx, g, mask=mask, min_area=4)
    assert np.array_equal(got, want_regions(g, mask=mask, min_area=4))
    assert set(got[:, 0]) <= {p for p in (0, 1) if mask >> p & 1}


@pytest.mark.parametrize("params", [dict(delta=1), dict(delta=40), dict(min_diversity=0.0), dict(min_diversity=0.9),
                                    dict(max_variation=0.0), dict(delta=255, min_area=1, max_area=10 ** 6, max_variation=1e9)],
                         ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_non_default_parameters(ctx, params):
    for name in ("text", "noise"):
        g = CASES[name][0]
        assert np.array_equal(gpu_regions(ctx, g, **params), want_regions(g, **params)), name


@functools.lru_cache(maxsize=None)
def baseline():
    img = R.baseline_source()
    return img, as_rows(_native.mser_host(img)), [as_rows(_native.mser_tree_host(img, pol)) for pol in (0, 1)]


def test_baseline_source_equals_host_restatement(ctx):
    img, want, trees = baseline()
    got = gpu_regions(ctx, img)
    print(f"720 x 1080: {len(trees[0])} dark / {len(trees[1])} bright nodes, {len(want)} regions")
    assert np.array_equal(got, want)
    for pol in (0, 1):
        assert np.array_equal(gpu_tree(ctx, img, pol), trees[pol])


def test_a_short_first_buffer_does_not_run_the_detection_again(ctx, monkeypatch):
    """1025 regions through a first buffer of 4: the rest comes from the copy the context keeps (sr_mser_last_regions); the
    profile counts the level launches of ONE run, four per non-empty level and polarity."""
    g, params = CASES["checkerboard"]
    want = case_reference("checkerboard")[0]
    assert len(want) == 1025
    monkeypatch.setattr(_native, "MSER_FIRST_CAP", 4)
    d = ctx.upload(g)
    ctx.prof_select(None)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        got = as_rows(ctx.mser(d.ptr, g.shape[1], g.shape[0], g.shape[1], 1, _native.mser_params(**params)))
        ctx.sync()
        launches = sum(n for k, (_, n) in ctx.prof_get().items() if k in ("ms_note", "ms_union", "ms_create", "ms_accum"))
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        d.free()
    assert np.array_equal(got, want)
    assert launches == 2 * 4 * len(np.unique(g))
    import ctypes as C
    n = C.c_int64(0)
    one = np.zeros(1, _native.MSER_REGION_DTYPE)
    _native.check(ctx.lib.sr_mser_last_regions(ctx.handle, C.c_void_p(one.ctypes.data), 1, C.byref(n)))
    assert n.value == 1025 and as_rows(one)[0].tolist() == want[0].tolist()


def test_equal_inputs_give_equal_bytes(ctx):
    g = CASES["noise3"][0]
    d = ctx.upload(g)
    try:
        a, b = (ctx.mser(d.ptr, g.shape[1], g.shape[0], g.shape[1], 1) for _ in range(2))
        ta, tb = (ctx.mser_tree(d.ptr, g.shape[1], g.shape[0], g.shape[1], 1, 0) for _ in range(2))
    finally:
        d.free()
    assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes()


def test_large_small_large_on_a_poisoned_workspace(ctx):
    img, want, _ = baseline()
    small, small_params = CASES["spirals"]
    for g, w in ((img, want), (small, case_reference("spirals")[0]), (img, want)):
        ptr, nbytes = ctx.mser_workspace()
        if nbytes:
            ctx.memset(ptr, 0xFF, nbytes)                                              # a call never reads what was there
        assert np.array_equal(gpu_regions(ctx, g, **(small_params if g is small else {})), w)
    assert ctx.mser_workspace()[1] >= _native.mser_plan(720, 1080)["workspace_bytes"]  # grow-only


def test_guarded_strided_views(ctx):
    g = CASES["text"][0]
    rgb = np.stack([g, g // 2, 255 - g], axis=2)
    for k, fill in enumerate(V.FILLS):
        for img in (g, rgb):
            cn = img.shape[2] if img.ndim == 3 else 1
            lay = V.pick(V.LAYOUTS_U8, 3 * k + cn)
            parent, ptr, stride = V.embed(ctx, img, lay[0], lay[1], fill)
            try:
                got = as_rows(ctx.mser(ptr, stride, img.shape[0], img.shape[1], cn))
                V.check_guard(ctx, parent, what="input")                               # not a byte written outside the outputs
            finally:
                parent.free()
            assert np.array_equal(got, want_regions(R.gray_swapped(img)))


def test_row_stride_beyond_32_bits(ctx):
    g = np.ascontiguousarray(CASES["nested"][0][:3])                                   # 3 rows: offsets 0, 2^32 + 7, 2^33 + 14
    stride = (1 << 32) + 7
    buf = ctx.alloc(2 * stride + g.shape[1])
    dense = ctx.upload(g)
    try:
        for r in range(3):
            ctx.copy_d2d(buf.ptr + r * stride, dense.ptr + r * g.shape[1], g.shape[1])
        ctx.sync()
        got = as_rows(ctx.mser(buf.ptr, stride, 3, g.shape[1], 1, _native.mser_params(min_area=1)))
    finally:
        dense.free()
        buf.free()
    assert np.array_equal(got, want_regions(g, min_area=1))


def test_forbidden_zone_map_with_the_detector(ctx):
    g = CASES["text"][0]
    img = np.stack([g, g, g], axis=2)
    gray = R.gray_swapped(img)
    boxes = R.text_boxes(R.regions(gray), img.shape[1])
    assert len(boxes) == 10
    ca = tm.ContentAnalyzer(text_detector='mser')
    for salient in (False, True):
        # the saliency plane has its own test and bound (tests/test_gpu_content.py): here the map is held to the reference
        # fed the restatement's boxes and the plane the GPU made
        sal = ca.compute_saliency_map(img) if salient else None
        want = CR.forbidden_map(img, texts=boxes, protect_salient=salient, saliency_map=sal).astype(np.uint8)
        got = ca.create_forbidden_zone_map(img, protect_faces=False, protect_salient=salient)
        d_img = ctx.upload(img)
        try:
            fmap = ca.create_forbidden_zone_map_device(d_img.ptr, img.shape, protect_faces=False, protect_salient=salient)
            try:
                dev = fmap.download()
            finally:
                fmap.free()
        finally:
            d_img.free()
        assert np.array_equal(got, want) and want.sum() >= sum(w * h for _, _, w, h in boxes[5:])
        assert np.array_equal(dev, want)                                               # the device form needs no host_image


def test_split_array_roi_flags_from_the_detector(ctx):
    g = CASES["text"][0]
    img = np.stack([g, g, g], axis=2)
    boxes = R.text_boxes(R.regions(R.gray_swapped(img)), img.shape[1])
    fmap = np.zeros(img.shape[:2], np.uint8)
    for x, y, w, h in boxes:
        fmap[y:y + h, x:x + w] = 1
    tiler = tm.TilingModule(block_size=64, overlap_ratio=0.25, content_analyzer=tm.ContentAnalyzer(text_detector='mser'),
                            forbidden_zone_args=dict(protect_faces=False, protect_salient=False))
    try:
        tiles = tiler.split_array(img, device_resident=True)
        assert len(tiles) > 1
        want = CR.tile_flags(fmap.astype(bool), [(t.metadata.global_x, t.metadata.global_y, t.metadata.input_w, t.metadata.input_h)
                                                 for t in tiles])
        assert [t.metadata.roi_flags for t in tiles] == want and any(f['has_forbidden_zone'] for f in want)
    finally:
        tiler.release_device_tiles()
