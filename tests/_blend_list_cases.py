"""Fixtures for the stand-alone blend-path kernels (csrc/sr_gradient.hip, the feather merge and the seam scan of
csrc/sr_tiles.hip), built deterministically from seeds, and the pure-NumPy restatements of the kernels' launch geometry that
tests/test_blend_list_cases_host.py uses to show that every fixture reaches the branch it is meant for:

  * the ballot-compacted tile lists (64 table entries per ballot round, at most 64 listed tiles, above that the walk of the
    whole table): tables that need several rounds, windows / blocks with exactly 64 and with 65 hits;
  * one cosine LUT per distinct feather width (tiles of several sizes, two sizes sharing a width);
  * the chunk edges of the row pass (256 row elements, 16 rows) and of the column pass (64 row elements, 64 rows);
  * the copy fast path of the feather merge on the edges of its ramps;
  * seam-scan tile lists that hold tiles without a window, and a scan with more hits than the first record buffer.

Everything here is NumPy; the GPU tests import the fixtures, the host test their preconditions."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import oracle_np as onp

# launch geometry of the kernels (csrc/sr_gradient.hip, csrc/sr_tiles.hip)
GR_ROWS, GR_CHUNK, GC_COLS, GC_ROWS, MAXLIST = 16, 256, 64, 64, 64
FM_BW, FM_BH = 256, 4

# ---- gradient-domain fusion ---------------------------------------------------------------------------------------------
GradCase = namedtuple("GradCase", "name rects cn shape seed")      # rects: (y, x, h, w) in list order; shape: (H, W)


def grad_positions(case):
    return [(y, x) for (y, x, _, _) in case.rects]


def grad_tiles(case, f32: bool = False):
    """A smooth ramp common to all tiles (20 + a x + b y in canvas coordinates), a per-tile offset of a few levels and
    noise of +-2: the integrated canvas (about 4 (a x + b y): a Sobel is 8 times the slope, the two sums are halved) stays
    between 0 and 255 almost everywhere, so its bytes carry information.  f32: non-integer data (* 0.731 + 0.3)."""
    H, W = case.shape
    rng = np.random.default_rng(case.seed)
    a, b = rng.uniform(0.1, 0.5, 2)
    s = min(1.0, 230.0 / (4.0 * (a * W + b * H)))
    a, b = max(0.1, a * s), max(0.1, b * s)
    out = []
    for (y, x, h, w) in case.rects:
        yy, xx = np.mgrid[y:y + h, x:x + w]
        base = 20.0 + a * xx + b * yy + float(rng.integers(-3, 4))
        img = np.rint(base)[..., None] + rng.integers(-2, 3, (h, w, case.cn))
        img = np.clip(img, 0, 255).astype(np.uint8)
        if case.cn == 1:
            img = img[..., 0]
        out.append(img.astype(np.float32) * np.float32(0.731) + np.float32(0.3) if f32 else img)
    return out


def _hits(rects, y0, y1, x0, x1):
    r = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    y, x, h, w = r.T
    return int(np.count_nonzero((x < x1) & (x + w > x0) & (y < y1) & (y + h > y0)))


def grad_row_hits(case):
    """Tiles met by each window of k_grad_row (16 canvas rows x one chunk of 256 row elements) -> list of counts."""
    H, W = case.shape
    wc, cn, out = W * case.cn, case.cn, []
    for y0 in range(0, H, GR_ROWS):
        for e0 in range(0, wc, GR_CHUNK):
            ne = min(GR_CHUNK, wc - e0)
            out.append(_hits(case.rects, y0, min(y0 + GR_ROWS, H), e0 // cn, (e0 + ne - 1) // cn + 1))
    return out


def grad_col_hits(case):
    """The same for k_grad_col (64 row elements x one chunk of 64 canvas rows)."""
    H, W = case.shape
    wc, cn, out = W * case.cn, case.cn, []
    for e0 in range(0, wc, GC_COLS):
        ne = min(GC_COLS, wc - e0)
        for y0 in range(0, H, GC_ROWS):
            out.append(_hits(case.rects, y0, min(y0 + GC_ROWS, H), e0 // cn, (e0 + ne - 1) // cn + 1))
    return out


def ballot_rounds_with_hits(case):
    """Over the windows of k_grad_row: the largest number of 64-entry ballot rounds that each contribute a listed tile."""
    H, W = case.shape
    wc, cn, best = W * case.cn, case.cn, 0
    for y0 in range(0, H, GR_ROWS):
        for e0 in range(0, wc, GR_CHUNK):
            ne = min(GR_CHUNK, wc - e0)
            best = max(best, sum(1 for b in range(0, len(case.rects), 64)
                                 if _hits(case.rects[b:b + 64], y0, min(y0 + GR_ROWS, H), e0 // cn, (e0 + ne - 1) // cn + 1)))
    return best


def grid130(cn: int) -> GradCase:
    """130 tiles of 32 x 40 on a 10 x 13 grid with 8 px of overlap, the list permuted: a 248 x 424 canvas, a table of three
    ballot rounds, no window above 64 tiles."""
    th, tw, ov = 32, 40, 8
    rects = [(r * (th - ov), c * (tw - ov), th, tw) for r in range(10) for c in range(13)]
    order = np.random.default_rng(1300 + cn).permutation(len(rects))
    return GradCase(f"grid130-cn{cn}", [rects[i] for i in order], cn, (10 * th - 9 * ov, 13 * tw - 12 * ov), 130 + cn)


def pile(n: int, cn: int = 3) -> GradCase:
    """n tiles of 32 x 40 at (y, x) = (i % 7, 5 i % 61) on a 40 x 100 canvas: every tile meets the first 16-row window."""
    return GradCase(f"pile{n}", [(i % 7, (5 * i) % 61, 32, 40) for i in range(n)], cn, (40, 100), 9000 + n)


def mixed_sizes(cn: int = 3) -> GradCase:
    """Feather widths min(h, w) // 8 = 5, 1, 4, 2, 4, 5, 3 in list order: not sorted, 34 x 70 and 44 x 36 share width 4,
    40 x 52 and 47 x 41 share width 5."""
    rects = [(0, 0, 40, 52), (30, 20, 12, 60), (10, 40, 34, 70), (25, 0, 20, 30), (36, 70, 44, 36), (33, 10, 47, 41),
             (0, 95, 30, 24)]
    return GradCase(f"mixed-cn{cn}", rects, cn, (80, 112), 77 + cn)


# (H, W * cn, cn): every H once, every row length once per channel count
# (a one-row canvas is all zeros, see the host test; 258 elements of cn 3 is the one shape here whose second chunk starts off
# a pixel boundary -- the chain phase -- so it goes with a tall canvas)
CHUNK_EDGE_SHAPES = [(1, 255, 1), (15, 256, 1), (16, 257, 1), (17, 513, 1), (63, 256, 2), (64, 258, 2), (16, 255, 3),
                     (65, 258, 3), (1, 256, 4), (64, 260, 4)]


def chunk_edge(H: int, wc: int, cn: int) -> GradCase:
    """Three overlapping tiles (smaller side >= 32) over an H x (wc / cn) canvas: two side by side, the right one reaching
    past the right edge, and one across their seam in the lower half; all reach past the bottom of a low canvas."""
    assert wc % cn == 0
    W = wc // cn
    th, half = max(H, 32), W // 2
    rects = [(0, 0, th + 3, half + 10), (0, half - 10, th, W - (half - 10) + 5),
             (H // 2, W // 3, max(32, H - H // 2 + 4), max(32, W // 3))]
    return GradCase(f"edge-{H}x{wc}-cn{cn}", rects, cn, (H, W), 5000 + 7 * H + wc + cn)


# ---- feather merge ------------------------------------------------------------------------------------------------------
MergeCase = namedtuple("MergeCase", "name tiles metas descs W H")


def _merge_entry(x, y, ow, oh, ov, sw=None, sh=None):
    sw, sh = sw or ow, sh or oh
    meta = dict(global_x=x, global_y=y, output_w=ow, output_h=oh, overlap_top=ov[0], overlap_bottom=ov[1],
                overlap_left=ov[2], overlap_right=ov[3])
    desc = dict(x=x, y=y, src_w=sw, src_h=sh, out_w=ow, out_h=oh, ov_t=ov[0], ov_b=ov[1], ov_l=ov[2], ov_r=ov[3])
    return meta, desc


def _merge_data(rng, h, w, f32):
    d = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    return d.astype(np.float32) * np.float32(0.731) + np.float32(0.3) if f32 else d


def merge_block_hits(case):
    """Tiles met by each 256 x 4 block of k_feather_merge -> list of counts."""
    r = [(d["y"], d["x"], d["out_h"], d["out_w"]) for d in case.descs]
    return [_hits(r, by, by + FM_BH, bx, bx + FM_BW) for by in range(0, case.H, FM_BH) for bx in range(0, case.W, FM_BW)]


def merge_pile(n: int, f32: bool = False) -> MergeCase:
    """n tiles of 12 x 20 (h x w) at x = 3 i, y = i % 3, ramps (3, 4, 5, 6), on a canvas 256 wide and 20 high: every tile
    meets block (0, 0)."""
    rng = np.random.default_rng(640 + n + (1000 if f32 else 0))
    tiles, metas, descs = [], [], []
    for i in range(n):
        m, d = _merge_entry(3 * i, i % 3, 20, 12, (3, 4, 5, 6))
        tiles.append(_merge_data(rng, 12, 20, f32))
        metas.append(m)
        descs.append(d)
    return MergeCase(f"pile{n}-{'f32' if f32 else 'u8'}", tiles, metas, descs, 256, 20)


def merge_spread150() -> MergeCase:
    """150 tiles of 33 x 44 on a 10 x 15 grid (steps 30 / 40) over a 300 x 600 canvas, the list permuted, every fourth tile
    resized from about half its size: three ballot rounds, a block meets at most 16 tiles."""
    rng = np.random.default_rng(150)
    entries = []
    for i in range(150):
        r, c = divmod(i, 15)
        sw, sh = (25, 18) if i % 4 == 1 else (44, 33)
        m, d = _merge_entry(40 * c, 30 * r, 44, 33, (3, 3, 4, 4), sw, sh)
        entries.append((_merge_data(rng, sh, sw, False), m, d))
    order = rng.permutation(150)
    tiles, metas, descs = zip(*[entries[i] for i in order])
    return MergeCase("spread150", list(tiles), list(metas), list(descs), 600, 300)


def copy_edge(ov_l: int, ov_r: int, ov_t: int, ov_b: int, cw: int, second: bool) -> MergeCase:
    """One unresized u8 tile 600 wide and 40 high at the origin.  Blocks of 256 x 4: with ov_l = 256 block column 1 begins
    on the first pixel past the left ramp, with 257 one pixel inside it; with ov_r = 88 the right ramp begins at column 512,
    where block column 2 does, with 120 inside block column 1; ov_t / ov_b = 4 or 5 put block rows 1 and 8 on or one row
    inside the ramps.  cw 598: a 2-pixel tail; cw 500: the canvas ends inside block column 1.  second: another tile over
    columns 0..99 only."""
    rng = np.random.default_rng(600)
    m, d = _merge_entry(0, 0, 600, 40, (ov_t, ov_b, ov_l, ov_r))
    tiles, metas, descs = [_merge_data(rng, 40, 600, False)], [m], [d]
    if second:
        m2, d2 = _merge_entry(0, 0, 100, 40, (3, 3, 10, 10))
        tiles.append(_merge_data(rng, 40, 100, False))
        metas.append(m2)
        descs.append(d2)
    return MergeCase(f"copy-l{ov_l}-r{ov_r}-t{ov_t}-b{ov_b}-w{cw}-{'two' if second else 'one'}", tiles, metas, descs, cw, 40)


def copy_edge_cases(cw: int, second: bool):
    """The product of ov_l {256, 257} x ov_r {88, 120} x ov_t {4, 5} x ov_b {4, 5}, and one side at a time further in.
    A linspace ramp includes its end point, so the ramp pixel next to the tile's interior has weight exactly 1 and is still
    the tile's own byte (ov_l 257, ov_r 89, ov_t / ov_b 5: a copy would be right there; the kernel does not take it).
    Further in trunc(fp32(p w) / w) differs from p for some byte values only; ov_l 259 (column 257: w = 257 / 258),
    ov_r 90 (column 511: w = 88 / 89) and ov_t / ov_b 7 (rows 5 / 34: w = 5 / 6) are the shortest ramps for which the
    first block column / row past the ramp's nominal end holds such values (asserted by the host test)."""
    out = [copy_edge(l, r, t, b, cw, second) for l in (256, 257) for r in (88, 120) for t in (4, 5) for b in (4, 5)]
    out += [copy_edge(259, 88, 4, 4, cw, second), copy_edge(256, 89, 4, 4, cw, second), copy_edge(256, 90, 4, 4, cw, second),
            copy_edge(256, 88, 7, 4, cw, second), copy_edge(256, 88, 4, 7, cw, second)]
    if cw < 512:        # the canvas ends inside block column 1: its last column takes the part of the block's right end
        out += [copy_edge(256, 600 - cw + k, 4, 4, cw, second) for k in (0, 1, 2)]
    return out


def ramp_length_cases():
    """Ramps of one pixel on each side in turn (np.linspace(0, 1, 1) is [0]: the weight is 0, and where no other tile covers
    the pixel the 1e-6 floor divides), and ramps as long as the tile.  A second tile covers the right half."""
    out = []
    full = [(24, 0, 36, 0), (0, 24, 0, 36), (24, 24, 36, 36)]
    for k, ov in enumerate([(1, 3, 3, 3), (3, 1, 3, 3), (3, 3, 1, 3), (3, 3, 3, 1), (1, 1, 1, 1)] + full):
        rng = np.random.default_rng(70 + k)
        m, d = _merge_entry(2, 1, 36, 24, ov)
        m2, d2 = _merge_entry(20, 0, 30, 26, (2, 2, 6, 6))
        out.append(MergeCase("ramp-" + "-".join(map(str, ov)), [_merge_data(rng, 24, 36, False), _merge_data(rng, 26, 30, False)],
                             [m, m2], [d, d2], 52, 27))
    return out


# ---- seam scan ----------------------------------------------------------------------------------------------------------
SeamCase = namedtuple("SeamCase", "name canvas tiles rects cn")     # rects: (x, y, w, h)


def seam_hits(canvas, tiles, rects, threshold, window, stride):
    """The window loop of oracle_np.detect_seams with the tile index kept and without the merge of adjacent windows:
    [(tile, x, y, score)] in (tile, y, x) order.  test_blend_list_cases_host.py ties it to detect_seams."""
    out = []
    H, W = canvas.shape[:2]
    for t, (img, (tx, ty, _, _)) in enumerate(zip(tiles, rects)):
        th, tw = img.shape[:2]
        rw, rh = min(tx + tw, W) - tx, min(ty + th, H) - ty
        if rw <= 0 or rh <= 0:
            continue
        for y in range(0, rh - window + 1, stride):
            for x in range(0, rw - window + 1, stride):
                sc = onp.window_ssim(img[y:y + window, x:x + window], canvas[ty + y:ty + y + window, tx + x:tx + x + window])
                if sc < threshold:
                    out.append((t, tx + x, ty + y, sc))
    return out


def _seam_scene(rng, h, w, cn):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(xx / 9.0) + 40 * np.cos(yy / 7.0)
    img = np.clip(base[..., None] + rng.integers(-20, 21, (h, w, cn)), 0, 255).astype(np.uint8)
    return img if cn == 3 else img[..., 0]


def _disturb(rng, img, amp):
    return np.clip(img.astype(np.int16) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def seam_two_tiles(cn: int) -> SeamCase:
    """Two 48 x 40 tiles side by side (8 px apart in x) under a 48 x 72 canvas that is the tiles' content, disturbed."""
    rng = np.random.default_rng(480 + cn)
    scene = _seam_scene(rng, 48, 72, cn)
    tiles = [np.ascontiguousarray(scene[:, 0:40]), np.ascontiguousarray(scene[:, 32:72])]
    return SeamCase(f"two-cn{cn}", _disturb(rng, scene, 25), tiles, [(0, 0, 40, 48), (32, 0, 40, 48)], cn)


def seam_zero_window_tiles(cn: int) -> SeamCase:
    """Seven tiles on a 64 x 150 canvas; for windows of 16 and of 12 pixels the first (10 wide), the fourth and the fifth
    (9 high; clipped by the right canvas edge to 8 columns) and the last (clipped by the bottom edge to 5 rows) hold no
    window; the sixth is clipped by the bottom edge to 34 rows and keeps its windows."""
    rng = np.random.default_rng(700 + cn)
    H, W = 64, 150
    scene = _seam_scene(rng, H + 40, W + 40, cn)
    rects = [(0, 0, 10, 40), (5, 3, 40, 40), (30, 10, 50, 36), (60, 0, 40, 9), (W - 8, 12, 40, 40), (90, 30, 40, 40),
             (100, H - 5, 40, 40)]
    tiles = [np.ascontiguousarray(scene[y:y + h, x:x + w]) for (x, y, w, h) in rects]
    return SeamCase(f"zero-cn{cn}", _disturb(rng, np.ascontiguousarray(scene[:H, :W]), 25), tiles, rects, cn)


def seam_split_threshold(case, window, stride):
    """A threshold half way between the two middle scores of the case's windows: half of them are hits, and none is so
    close to the threshold that the last bits of a score decide."""
    s = sorted(h[3] for h in seam_hits(case.canvas, case.tiles, case.rects, 2.0, window, stride))
    k = len(s) // 2
    assert s[k] - s[k - 1] > 1e-6
    return 0.5 * (s[k - 1] + s[k])


def seam_window_counts(case, window, stride):
    H, W = case.canvas.shape[:2]
    out = []
    for (x, y, w, h) in case.rects:
        rw, rh = min(x + w, W) - x, min(y + h, H) - y
        nx = (rw - window) // stride + 1 if rw >= window else 0
        ny = (rh - window) // stride + 1 if rh >= window else 0
        out.append(nx * ny)
    return out


def seam_gray540() -> SeamCase:
    """One gray 540 x 540 tile at the origin: with window 8, stride 1 and a threshold no score reaches, 533^2 = 284 089
    records, more than the 2^18 the first pass of Context.seam_scan has room for."""
    rng = np.random.default_rng(540)
    tile = _seam_scene(rng, 540, 540, 1)
    return SeamCase("gray540", _disturb(rng, tile, 30), [tile], [(0, 0, 540, 540)], 1)


def window_ssim_all(tile_gray, canvas_gray, window):
    """window_ssim of every window position (stride 1) of two equal-sized gray u8 images at once: the five window sums from
    integral images (exact integers), then the float64 expression of _compute_ssim on them -> (ny, nx) float64."""
    a, b = tile_gray.astype(np.int64), canvas_gray.astype(np.int64)

    def box(v):
        s = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
        s[1:, 1:] = v.cumsum(0).cumsum(1)
        return s[window:, window:] - s[:-window, window:] - s[window:, :-window] + s[:-window, :-window]

    n = float(window * window)
    sx, sy, sxx, syy, sxy = box(a), box(b), box(a * a), box(b * b), box(a * b)
    mu1, mu2 = sx / n, sy / n
    s1, s2, s12 = sxx / n - mu1 * mu1, syy / n - mu2 * mu2, sxy / n - mu1 * mu2
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
