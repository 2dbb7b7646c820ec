"""GPU: cascade detection (csrc/sr_cascade.hip) against the NumPy restatement (tests/_cascade_ref.py) and the host twin
(sr_cascade_host_u8).  Candidates, grouped boxes, stage maps and every scaled plane are compared for EQUALITY: all of them
are integers.  The shapes are the smallest at which each mechanism can fail: the window itself, the step-2 edges, one below /
at / above the constants of the kernels (256 threads per block: plane samples, table columns, window positions; 64 samples
per scan step; 4 table rows per block), both steps, every position a detection, none, a checkerboard half, the recorded
scikit-image planes, and the 720 x 1080 source at the size Python is too slow for (held to the host twin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cascade_ref as R
import _content_ref as CR
import _native
import _views as V
import tiling_module as tm

pytestmark = pytest.mark.gpu


def rows(c):
    return np.array(c, dtype=np.int64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def tables(name):
    if name == "real":
        return tm.load_cascade(R.LBP_XML)
    return {"accept": R.accept_all, "reject": R.reject_all, "checker": R.checker, "lbp": R.random_lbp,
            "lbp3": lambda: R.random_lbp(window=(3, 3), seed=11, stages=(2, 3))}[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    return _native.CascadeModel(tables(name))


@functools.lru_cache(maxsize=None)
def fixture():
    return R.skimage_fixture()


def on_gpu(ctx, img, fn):
    img = np.ascontiguousarray(img)
    cn = img.shape[2] if img.ndim == 3 else 1
    d = ctx.upload(img)
    try:
        return fn(d.ptr, img.shape[1] * cn, img.shape[0], img.shape[1], cn)
    finally:
        d.free()


def gpu_candidates(ctx, m, img, **kw):
    return rows(on_gpu(ctx, img, lambda p, s, h, w, cn: ctx.cascade(m, p, s, h, w, cn, _native.cascade_params(**kw))))


def check_everything(ctx, t, m, img, python=True, **kw):
    """Candidates, every scaled plane and both stage maps of one gray image: GPU == host twin (== restatement)."""
    params = _native.cascade_params(**kw)
    want = rows(m.host(img, params))
    if python:
        assert np.array_equal(want, rows(R.candidates(img, t, **kw)))
    got = gpu_candidates(ctx, m, img, **kw)
    assert np.array_equal(got, want)
    assert np.array_equal(rows(_native.cascade_group(got, 2)), rows(R.group(want.tolist(), 2)))
    scales = m.plan(img.shape[0], img.shape[1], params)["scales"]
    ref_planes = R.planes(img, t, **kw) if python else [m.plane_host(img, k, params) for k in range(len(scales))]
    assert len(ref_planes) == len(scales)
    for k, p in enumerate(ref_planes):
        assert np.array_equal(on_gpu(ctx, img, lambda a, s, h, w, cn: ctx.cascade_plane(m, a, s, h, w, cn, k, params)), p), k
    for step in (1, 2):
        smap = on_gpu(ctx, img, lambda a, s, h, w, cn: ctx.cascade_stage_map(m, a, s, h, w, cn, step))
        assert np.array_equal(smap, m.stage_map_host(img, step))
        if python and smap.size <= 4000:
            assert np.array_equal(smap, R.stage_map(t, img, step))
    return got


def test_image_smaller_than_the_window_launches_nothing(ctx):
    ctx.prof_select(None)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for shape in ((23, 40), (40, 23), (1, 1)):
            assert len(gpu_candidates(ctx, model("accept"), R.noise_image(*shape))) == 0
            assert on_gpu(ctx, R.noise_image(*shape), lambda a, s, h, w, cn: ctx.cascade_stage_map(model("accept"), a, s, h, w, cn, 1)).shape == (0, 0)
        ctx.sync()
        assert not [k for k in ctx.prof_get() if k.startswith("cc_")]
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert tm.CascadeFaceDetector(tables("accept"))(R.noise_image(10, 10)) == []


@pytest.mark.parametrize("shape,count", [((24, 24), 1), ((24, 25), 1), ((26, 24), 2), ((26, 26), 5)], ids=str)
def test_the_window_itself_and_the_step_two_edges(ctx, shape, count):
    """24 x 24: one window; a 25th column adds no step-2 position; 26 rows add one; 26 x 26 holds 2 x 2 and one more at
    f = 1.1, where 26 / 1.1 rounds to the window's 24."""
    img = R.noise_image(*shape)
    for name in ("accept", "lbp"):
        got = check_everything(ctx, tables(name), model(name), img)
        assert name != "accept" or len(got) == count


EDGES = [(24, 63), (25, 64), (26, 65), (27, 127), (24, 128), (28, 129), (24, 255), (25, 256), (24, 257), (27, 278), (26, 279), (25, 281),
         (63, 24), (64, 25), (65, 26), (255, 24), (256, 25), (257, 24), (24, 534), (25, 535), (26, 536)]


@pytest.mark.parametrize("shape", EDGES, ids=str)
def test_sides_around_the_kernels_constants(ctx, shape):
    """Widths and heights one below, at and above 64 (a scan step), 128, 256 (a block of samples, of columns: sw + 1, of
    positions: 278 / 279 / 281 columns give 128 and 129 positions per row; 534 .. 536 give 256 and 257)."""
    check_everything(ctx, tables("lbp"), model("lbp"), R.noise_image(*shape, seed=shape[1]))


def test_both_steps_on_56_x_64(ctx):
    img = R.noise_image(56, 64)
    steps = [s["step"] for s in model("lbp").plan(56, 64)["scales"]]
    assert set(steps) == {1, 2}
    got = check_everything(ctx, tables("lbp"), model("lbp"), img)
    assert len(got) > 0
    check_everything(ctx, tables("checker"), model("checker"), R.checker_image(56, 64))


def test_accept_everything_and_a_short_first_buffer(ctx, monkeypatch):
    """Every position of every scale is a candidate: the counts, the atomic append and the canonical sort; then the same
    call through a first buffer of 7, the rest fetched from the copy the context keeps, with ONE run of the kernels."""
    img = R.noise_image(80, 96)
    m, t = model("accept"), tables("accept")
    plan = m.plan(80, 96)
    want = rows(R.candidates(img, t))
    assert len(want) == plan["positions"] == sum(s["nx"] * s["ny"] for s in plan["scales"]) and len(plan["scales"]) > 8
    got = check_everything(ctx, t, m, img)
    assert np.array_equal(got, want)
    monkeypatch.setattr(_native, "CASCADE_FIRST_CAP", 7)
    ctx.prof_select(None)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        short = gpu_candidates(ctx, m, img)
        ctx.sync()
        prof = {k: n for k, (_, n) in ctx.prof_get().items() if k.startswith("cc_")}
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert np.array_equal(short, want)
    # one scope per launch: five launches, the model ends inside the dense stages
    assert prof == {"cc_gray": 1, "cc_planes": 1, "cc_rows": 1, "cc_cols": 1, "cc_dense": 1}
    n = C.c_int64(0)
    two = np.zeros((2, 4), np.int32)
    _native.check(ctx.lib.sr_cascade_last_candidates(ctx.handle, C.c_void_p(two.ctypes.data), 2, C.byref(n)))
    assert n.value == len(want) and two.tolist() == want[:2].tolist()


def test_reject_everything(ctx):
    assert len(check_everything(ctx, tables("reject"), model("reject"), R.noise_image(80, 96))) == 0


def test_checkerboard_half_survives_stage_zero(ctx):
    """Stage 0 passes a checkerboard half of the scale-0 positions and stage 1 is longer than the dense stages hold: the
    compaction sees every wave half full, in a pattern."""
    img = R.checker_image(80, 96)
    m, t = model("checker"), tables("checker")
    assert m.info()["n_stages"] == 2 and 1 == len([1 for c in t["stage_counts"] if c <= 64])
    smap = on_gpu(ctx, img, lambda a, s, h, w, cn: ctx.cascade_stage_map(m, a, s, h, w, cn, 2))
    yy, xx = np.mgrid[0:smap.shape[0], 0:smap.shape[1]]
    assert np.array_equal(smap >= 1, (xx + yy) % 2 == 0) and smap.shape == (29, 37)
    got = check_everything(ctx, t, m, img)
    ctx.prof_select(None)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        gpu_candidates(ctx, m, img)
        ctx.sync()
        prof = {k: n for k, (_, n) in ctx.prof_get().items() if k.startswith("cc_")}
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert prof == {"cc_gray": 1, "cc_planes": 1, "cc_rows": 1, "cc_cols": 1, "cc_dense": 1, "cc_tail": 1}     # six launches
    print(f"checker: {len(got)} candidates")


def test_tail_takes_more_than_one_pass_over_the_survivors(ctx):
    """k_cc_tail walks the survivor list with a grid-stride loop of at most 8 blocks per compute unit (256 units: 524 288
    survivors a pass).  A stage 0 that passes everything followed by a stage longer than the dense stages hold, on a
    600 x 800 image: every one of its positions survives the dense stages, so the loop takes a second pass, a partial one."""
    img = np.ascontiguousarray(R.gray_swapped(R.baseline_source())[60:660, 140:940])
    t = R.permissive_then_tail()
    m = _native.CascadeModel(t)
    positions = m.plan(600, 800)["positions"]
    assert positions > 256 * 8 * 256 and positions % (256 * 8 * 256) % 256 != 0 and list(t["stage_counts"]) == [0, 65]
    want = rows(m.host(img))
    got = gpu_candidates(ctx, m, img)
    print(f"600 x 800: {positions} survivors of the dense stage, {len(want)} candidates")
    assert np.array_equal(got, want) and 0 < len(want) < positions


@pytest.mark.parametrize("side", [72, 80, 88])
def test_scikit_image_planes(ctx, side):
    """PINNED PARITY on the GPU: the scale-1 windows that pass all 20 stages equal skimage.feature.Cascade's."""
    f = fixture()
    plane, want = f[f"plane{side}"], f[f"windows{side}"]
    smap = on_gpu(ctx, plane, lambda a, s, h, w, cn: ctx.cascade_stage_map(model("real"), a, s, h, w, cn, 1))
    assert np.argwhere(smap == 20).tolist() == want.tolist()
    check_everything(ctx, tables("real"), model("real"), plane, python=side == 72)


@functools.lru_cache(maxsize=None)
def crop_reference():
    cands = R.candidates(fixture()["crop"], tables("real"))
    return cands, R.group(cands, 4)


def test_crop_with_the_defaults(ctx):
    f = fixture()
    cands, boxes = crop_reference()
    det = tm.CascadeFaceDetector(R.LBP_XML)
    assert np.array_equal(rows(det.candidates(f["crop"])), rows(cands))
    got = det(f["crop"])
    assert got == boxes and len(boxes) >= 1
    r, c, w, h = (int(v) for v in f["multiscale_box"])
    assert any(b[0] <= c + w / 2 <= b[0] + b[2] and b[1] <= r + h / 2 <= b[1] + b[3] and c <= b[0] + b[2] / 2 <= c + w
               and r <= b[1] + b[3] / 2 <= r + h for b in got), (got, (c, r, w, h))
    for k, p in enumerate(R.planes(f["crop"], tables("real"))):
        assert np.array_equal(on_gpu(ctx, f["crop"], lambda a, s, hh, ww, cn: ctx.cascade_plane(model("real"), a, s, hh, ww, cn, k)), p)


@functools.lru_cache(maxsize=None)
def baseline():
    img = R.baseline_source()
    return img, rows(model("real").host(img))


def test_baseline_source_equals_host_twin(ctx):
    img, want = baseline()
    m = model("real")
    got = gpu_candidates(ctx, m, img)
    plan = m.plan(img.shape[0], img.shape[1])
    print(f"720 x 1080: {len(plan['scales'])} scales, {plan['positions']} positions, {len(want)} candidates")
    assert img.shape[:2] == (720, 1080) and len(plan["scales"]) >= 30 and np.array_equal(got, want)
    for k in (0, 1, 7, len(plan["scales"]) - 1):
        assert np.array_equal(on_gpu(ctx, img, lambda a, s, h, w, cn: ctx.cascade_plane(m, a, s, h, w, cn, k)), m.plane_host(img, k))
    smap = on_gpu(ctx, img, lambda a, s, h, w, cn: ctx.cascade_stage_map(m, a, s, h, w, cn, 2))
    assert np.array_equal(smap, m.stage_map_host(img, 2))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_channel_counts(ctx, rng, cn):
    img = rng.integers(0, 256, size=(41, 58, cn)).astype(np.uint8)
    gray = R.gray_swapped(img)
    want = rows(R.candidates(gray, tables("lbp")))
    got = gpu_candidates(ctx, model("lbp"), img if cn > 1 else img[..., 0])
    assert np.array_equal(got, want) and np.array_equal(rows(model("lbp").host(img)), want)
    assert np.array_equal(on_gpu(ctx, img, lambda a, s, h, w, c: ctx.cascade_plane(model("lbp"), a, s, h, w, c, 0)), gray)
    if cn == 4:
        other = img.copy()
        other[..., 3] ^= 0xFF
        assert np.array_equal(gpu_candidates(ctx, model("lbp"), other), got)             # alpha is ignored


@pytest.mark.parametrize("name", sorted(R.HAAR_INPUTS))
def test_constructed_haar_cascades(ctx, name):
    """HAAR is tested on constructed cascades only.  The restatement keeps every stump away from its threshold
    (tests/test_cascade_host.py asserts the margin on these same inputs), so equality does not rest on a square root's
    last bit."""
    t, img, kw = R.HAAR_INPUTS[name]()
    margins = R.Margins()
    want = R.candidates(img, t, margins=margins, **kw)
    assert margins.worst > 1e-9
    got = check_everything(ctx, t, _native.CascadeModel(t), img, **kw)
    assert np.array_equal(got, rows(want))


@pytest.mark.parametrize("kw", [dict(min_size=(30, 30)), dict(max_size=(40, 40)), dict(min_size=(29, 29), max_size=(29, 29)),
                                dict(min_size=(200, 200)), dict(scale_factor=1.05), dict(scale_factor=2.0), dict(scale_factor=7.5),
                                dict(scale_factor=1.3, min_size=(25, 0), max_size=(64, 50))], ids=str)
def test_size_and_factor_edges(ctx, kw):
    img = R.noise_image(64, 90, seed=9)
    for name in ("accept", "lbp"):
        t, m = tables(name), model(name)
        want = rows(R.candidates(img, t, **kw))
        assert np.array_equal(gpu_candidates(ctx, m, img, **kw), want)
        if name == "accept" and "min_size" in kw and len(want):
            assert want[:, 2].min() >= kw["min_size"][0]
    det = tm.CascadeFaceDetector(tables("lbp"), min_neighbors=1, **kw)
    assert det(img) == R.group(R.candidates(img, tables("lbp"), **kw), 1)


def test_equal_inputs_give_equal_bytes(ctx):
    img = R.noise_image(120, 150, seed=3)
    m = model("lbp")
    a, b = (on_gpu(ctx, img, lambda p, s, h, w, cn: ctx.cascade(m, p, s, h, w, cn)) for _ in range(2))
    sa, sb = (on_gpu(ctx, img, lambda p, s, h, w, cn: ctx.cascade_stage_map(m, p, s, h, w, cn, 1)) for _ in range(2))
    assert len(a) > 0 and a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()


def test_large_small_large_on_a_poisoned_workspace(ctx):
    img, want = baseline()
    small = R.noise_image(56, 64)
    small_want = rows(model("lbp").host(small))
    hm, himg, kw = R.HAAR_INPUTS["flat"]()
    haar = _native.CascadeModel(hm)
    for m, g, w in ((model("real"), img, want), (model("lbp"), small, small_want), (haar, himg, rows(haar.host(himg))),
                    (model("real"), img, want)):
        ptr, nbytes = ctx.cascade_workspace()
        if nbytes:
            ctx.memset(ptr, 0xFF, nbytes)                                                  # a call never reads what was there
        assert np.array_equal(gpu_candidates(ctx, m, g), w)
    assert ctx.cascade_workspace()[1] >= model("real").plan(720, 1080)["workspace_bytes"]  # grow-only


def test_guarded_strided_views(ctx):
    g = R.noise_image(45, 70, seed=5)
    rgb = np.stack([g, g // 2, 255 - g], axis=2)
    m = model("lbp")
    for k, fill in enumerate(V.FILLS):
        for img in (g, rgb):
            cn = img.shape[2] if img.ndim == 3 else 1
            lay = V.pick(V.LAYOUTS_U8, 3 * k + cn)
            parent, ptr, stride = V.embed(ctx, img, lay[0], lay[1], fill)
            try:
                got = rows(ctx.cascade(m, ptr, stride, img.shape[0], img.shape[1], cn))
                smap = ctx.cascade_stage_map(m, ptr, stride, img.shape[0], img.shape[1], cn, 2)
                V.check_guard(ctx, parent, what="input")                                   # not a byte written outside the outputs
            finally:
                parent.free()
            assert np.array_equal(got, rows(m.host(img))) and np.array_equal(smap, m.stage_map_host(img, 2))
            assert np.array_equal(got, rows(R.candidates(R.gray_swapped(img), tables("lbp"))))


def test_row_stride_beyond_32_bits(ctx):
    g = R.noise_image(3, 40, seed=7)                                                       # 3 rows: offsets 0, 2^32 + 7, 2^33 + 14
    m, t = model("lbp3"), tables("lbp3")
    stride = (1 << 32) + 7
    buf = ctx.alloc(2 * stride + g.shape[1])
    dense = ctx.upload(g)
    try:
        for r in range(3):
            ctx.copy_d2d(buf.ptr + r * stride, dense.ptr + r * g.shape[1], g.shape[1])
        ctx.sync()
        got = rows(ctx.cascade(m, buf.ptr, stride, 3, g.shape[1], 1))
        plane = ctx.cascade_plane(m, buf.ptr, stride, 3, g.shape[1], 1, 0)
    finally:
        dense.free()
        buf.free()
    assert np.array_equal(plane, g) and np.array_equal(got, rows(R.candidates(g, t))) and len(m.plan(3, 40)["scales"]) == 2 and len(got) == 11


# ---- through ContentAnalyzer ---------------------------------------------------------------------------------------------------
def crop_rgb():
    g = fixture()["crop"]
    return np.stack([g, g, g], axis=2)                                                    # gray of equal channels is the value itself


def test_forbidden_zone_map_with_the_margin_rule(ctx):
    img = crop_rgb()
    assert np.array_equal(R.gray_swapped(img), fixture()["crop"])
    _, boxes = crop_reference()
    ca = tm.ContentAnalyzer(face_cascade=R.LBP_XML)
    assert ca.detect_faces(img) == boxes
    want = np.zeros(img.shape[:2], np.uint8)
    for x, y, w, h in boxes:
        margin = int(max(w, h) * 0.2)
        want[max(0, y - margin):y + h + margin, max(0, x - margin):x + w + margin] = 1
    assert np.array_equal(want, CR.forbidden_map(img, faces=boxes, texts=None, protect_salient=False).astype(np.uint8)) and want.any()
    got = ca.create_forbidden_zone_map(img, protect_text=False, protect_salient=False)
    assert np.array_equal(got, want)
    d_img = ctx.upload(img)
    try:
        fmap = ca.create_forbidden_zone_map_device(d_img.ptr, img.shape, protect_text=False, protect_salient=False)
        try:
            dev = fmap.download()
            flags = ca.tile_flags(fmap, [(0, 0, 128, 128), (128, 128, 128, 128), (0, 0, 256, 256)])
        finally:
            fmap.free()
    finally:
        d_img.free()
    assert np.array_equal(dev, want)                                                       # the device form needs no host_image
    assert flags == CR.tile_flags(want.astype(bool), [(0, 0, 128, 128), (128, 128, 128, 128), (0, 0, 256, 256)])
    assert flags[2]["has_forbidden_zone"]


def test_split_array_roi_flags_from_the_detector(ctx):
    img = crop_rgb()
    _, boxes = crop_reference()
    fmap = CR.forbidden_map(img, faces=boxes, texts=None, protect_salient=False)
    tiler = tm.TilingModule(block_size=128, overlap_ratio=0.25, content_analyzer=tm.ContentAnalyzer(face_cascade=R.LBP_XML),
                            forbidden_zone_args=dict(protect_text=False, protect_salient=False))
    try:
        tiles = tiler.split_array(img, device_resident=True)
        assert len(tiles) > 1
        want = CR.tile_flags(fmap.astype(bool), [(t.metadata.global_x, t.metadata.global_y, t.metadata.input_w, t.metadata.input_h)
                                                 for t in tiles])
        assert [t.metadata.roi_flags for t in tiles] == want and any(f['has_forbidden_zone'] for f in want)
    finally:
        tiler.release_device_tiles()


def test_default_analyzer_still_returns_no_faces(ctx):
    ca = tm.ContentAnalyzer()
    assert ca.detect_faces(crop_rgb()) == [] and ca.face_cascade is None
    got = ca.create_forbidden_zone_map(crop_rgb(), protect_text=False, protect_salient=False)
    assert not got.any()
