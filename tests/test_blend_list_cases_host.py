"""CPU: the fixtures of tests/_blend_list_cases.py reach the branches they are built for.

The GPU tests (test_gpu_gradient_lists.py, test_gpu_feather_merge_lists.py, test_gpu_seam_scan_edges.py) compare the kernels
with the oracle on these fixtures; here each fixture's precondition is asserted on the oracle and on the restated launch
geometry alone, so that a case cannot quietly stop reaching its branch:
  * tile lists: the largest number of tiles any window (k_grad_row: 16 rows x 256 row elements, k_grad_col: 64 x 64) or
    block (k_feather_merge: 256 x 4 pixels) meets -- at most 64 with a table of three ballot rounds, exactly 64, 65, more;
  * the tiles past the 64th matter to the oracle's canvas, and the list order to the fp32 row prefix sums;
  * the gradient canvases are not saturated;
  * the copy-path cases differ from a plain copy exactly where the ramps are;
  * the seam-scan restatements are the oracle's."""
import numpy as np
import pytest

import _blend_list_cases as L
import _gradient_ref as gref
from oracle import oracle_np as onp

GRAD_CASES = ([L.grid130(3), L.grid130(2)] + [L.pile(n) for n in (64, 65, 150)] + [L.mixed_sizes(3)]
              + [L.chunk_edge(*s) for s in L.CHUNK_EDGE_SHAPES])


def _canvas(case, f32=False):
    return gref.gradient_domain_fusion(L.grad_tiles(case, f32), L.grad_positions(case), case.shape)


def _merge(case, blending=True, keep=None):
    n = len(case.tiles) if keep is None else keep
    return onp.merge_tiles(case.tiles[:n], case.metas[:n], case.W, case.H, 1.0, blending)


def test_row_prefix_plane_is_the_loop_form():
    """row_prefix_plane against the running sums of the scalar-loop form, bit for bit, on one tiny grid: the loops' canvas is
    pinned to the vectorised one, and the plane is the first half of the same sequence."""
    case = L.GradCase("tiny", [(0, 0, 12, 16), (0, 10, 12, 16), (6, 4, 12, 18)], 3, (18, 26), 3)
    tiles, pos = L.grad_tiles(case), L.grad_positions(case)
    want = gref.gradient_domain_fusion_loops(tiles, pos, case.shape)
    assert np.array_equal(gref.gradient_domain_fusion(tiles, pos, case.shape), want)
    plane = gref.row_prefix_plane(tiles, pos, case.shape)
    assert plane.dtype == np.float32 and plane.shape == (18, 26, 3)
    # the plane plus the column sums of the same fields, halved and clipped, is the canvas
    _, gy = gref._normalised_gradients(tiles, pos, case.shape)
    r = (plane + np.cumsum(gy, axis=0)) / 2
    assert np.array_equal(np.clip(r, 0, 255).astype(np.uint8), want)
    # a sequential fp32 chain per row and channel, as the loops run it
    gx, _ = gref._normalised_gradients(tiles, pos, case.shape)
    run = np.zeros((18, 3), np.float32)
    for j in range(26):
        run = (run + gx[:, j, :]).astype(np.float32)
        assert np.array_equal(run.view(np.uint32), plane[:, j, :].view(np.uint32))


def test_gradient_list_sizes():
    for cn in (3, 2):
        g = L.grid130(cn)
        assert len(g.rects) == 130 and g.shape == (248, 424)
        assert max(L.grad_row_hits(g)) <= 64 and max(L.grad_col_hits(g)) <= 64
        assert L.ballot_rounds_with_hits(g) == 3                 # a window's list is filled from all three ballot rounds
        assert sorted(g.rects) != g.rects                        # the list order is not the grid's
    assert -(-248 // L.GC_ROWS) == 4 and -(-424 * 3 // L.GR_CHUNK) == 5
    assert max(L.grad_row_hits(L.pile(64))) == 64
    assert max(L.grad_row_hits(L.pile(65))) == 65
    assert max(L.grad_row_hits(L.pile(150))) == 150
    assert max(L.grad_col_hits(L.pile(64))) <= 64                # the column pass lists the pile of 64, too
    assert max(L.grad_col_hits(L.pile(150))) > 64                # and walks the table for the pile of 150
    for n in (64, 65, 150):
        assert all(min(h, w) >= 32 for (_, _, h, w) in L.pile(n).rects)


def test_mixed_sizes_feather_widths():
    for cn in (3, 1):
        fw = [min(h, w) // 8 for (_, _, h, w) in L.mixed_sizes(cn).rects]
        assert len(fw) >= 6 and {1, 2, 4, 5} <= set(fw)
        assert fw != sorted(fw) and fw != sorted(fw, reverse=True) and fw[0] != min(fw)
        sizes = {}
        for (_, _, h, w), f in zip(L.mixed_sizes(cn).rects, fw):
            sizes.setdefault(f, set()).add((h, w))
        assert any(len(s) >= 2 for s in sizes.values())          # two sizes share one table
        rects = L.mixed_sizes(cn).rects
        assert any(a != b and a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]
                   for a in rects for b in rects)


def test_chunk_edge_shapes():
    hs = [s[0] for s in L.CHUNK_EDGE_SHAPES]
    assert set(hs) == {1, 15, 16, 17, 63, 64, 65}
    per_cn = {cn: sorted(s[1] for s in L.CHUNK_EDGE_SHAPES if s[2] == cn) for cn in (1, 2, 3, 4)}
    assert per_cn == {1: [255, 256, 257, 513], 2: [256, 258], 3: [255, 258], 4: [256, 260]}
    assert len(L.CHUNK_EDGE_SHAPES) == 10                        # every row length once, no full product
    for s in L.CHUNK_EDGE_SHAPES:
        case = L.chunk_edge(*s)
        H, W = case.shape
        assert 2 <= len(case.rects) <= 3 and all(min(h, w) >= 32 for (_, _, h, w) in case.rects)
        assert all(0 <= y < H and 0 <= x < W for (y, x, _, _) in case.rects)
        cover = np.zeros((H, W), bool)
        for (y, x, h, w) in case.rects:
            cover[y:y + h, x:x + w] = True
        assert cover.all()
        assert any(x + w > W for (_, x, _, w) in case.rects) and any(y + h > H for (y, _, h, _) in case.rects)
    # the chain phase j0 differs from the channel index only where a chunk starts off a pixel boundary
    # (256 % cn is 0 for cn 1, 2, 4), and a one-row canvas is all zeros: the cn 3 row of 258 elements needs more rows
    assert any(cn == 3 and wc > L.GR_CHUNK and h > 1 for (h, wc, cn) in L.CHUNK_EDGE_SHAPES)


@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: c.name)
def test_gradient_canvases_are_not_saturated(case):
    c = _canvas(case)
    if case.shape[0] == 1:
        # A tile's position is inside the canvas, so the only row of a one-row canvas is row 0 of every tile that meets it:
        # distance 0 from the tile's edge, cosine weight 0, and 0 / max(0, 1e-6) = 0.  Such a canvas is all zeros whatever
        # the tiles hold; the case is there for the row arithmetic of H = 1 (rows = 1, one chain per channel), not for its bytes.
        assert not c.any() and not gref.row_prefix_plane(L.grad_tiles(case), L.grad_positions(case), case.shape).any()
        return
    frac = float(np.mean((c > 0) & (c < 255)))
    assert frac >= 0.5, (case.name, frac)


def test_list_order_and_late_tiles_are_observable():
    p150 = L.pile(150)
    tiles, pos = L.grad_tiles(p150), L.grad_positions(p150)
    a = gref.row_prefix_plane(tiles, pos, p150.shape)
    b = gref.row_prefix_plane(tiles[::-1], pos[::-1], p150.shape)
    assert np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)) > 0
    for n in (65, 150):                                          # a walk that stopped at the 64th tile shows in the canvas
        case = L.pile(n)
        tiles, pos = L.grad_tiles(case), L.grad_positions(case)
        full = gref.gradient_domain_fusion(tiles, pos, case.shape)
        cut = gref.gradient_domain_fusion(tiles[:64], pos[:64], case.shape)
        assert np.count_nonzero(full != cut) > 0, n
    for f32 in (False, True):
        for n in (65, 70):
            case = L.merge_pile(n, f32)
            assert np.count_nonzero(_merge(case) != _merge(case, keep=64)) > 0, (n, f32)


def test_merge_list_sizes():
    assert [max(L.merge_block_hits(L.merge_pile(n))) for n in (64, 65, 70)] == [64, 65, 70]
    s = L.merge_spread150()
    assert len(s.tiles) == 150 and (s.H, s.W) == (300, 600)
    assert max(L.merge_block_hits(s)) <= 64
    assert any(d["src_w"] != d["out_w"] for d in s.descs) and any(d["src_w"] == d["out_w"] for d in s.descs)
    grid_order = sorted(range(150), key=lambda i: (s.descs[i]["y"], s.descs[i]["x"]))
    assert grid_order != list(range(150))
    # a block's list takes tiles from all three ballot rounds
    r = [(d["y"], d["x"], d["out_h"], d["out_w"]) for d in s.descs]
    assert any(all(L._hits(r[b:b + 64], by, by + 4, bx, bx + 256) for b in (0, 64, 128))
               for by in range(0, 300, 4) for bx in range(0, 600, 256))


def test_copy_path_cases_sit_on_the_ramp_edges():
    for ov_r, differs in ((120, True), (88, False)):
        case = L.copy_edge(256, ov_r, 4, 4, 600, False)
        out = _merge(case)
        band = (slice(4, 36), slice(480, 512))                    # beyond the row ramps
        assert bool(np.any(out[band] != case.tiles[0][band])) == differs, ov_r
    # A ramp includes its end point: the ramp pixel next to the interior has weight exactly 1 and keeps the tile's byte
    # (column 256 with ov_l 257, column 511 with ov_r 89, rows 4 / 35 with ov_t / ov_b 5); pixels further in do not.
    inner, rows = slice(260, 510), slice(8, 32)

    def same(case, idx):
        return np.array_equal(_merge(case)[idx], case.tiles[0][idx])
    assert same(L.copy_edge(257, 88, 4, 4, 600, False), (rows, 256)) and not same(L.copy_edge(259, 88, 4, 4, 600, False), (rows, 257))
    assert same(L.copy_edge(256, 89, 4, 4, 600, False), (rows, 511)) and not same(L.copy_edge(256, 90, 4, 4, 600, False), (rows, 511))
    assert same(L.copy_edge(256, 88, 5, 4, 600, False), (4, inner)) and not same(L.copy_edge(256, 88, 7, 4, 600, False), (5, inner))
    assert same(L.copy_edge(256, 88, 4, 5, 600, False), (35, inner)) and not same(L.copy_edge(256, 88, 4, 7, 600, False), (34, inner))
    assert same(L.copy_edge(256, 101, 4, 4, 500, False), (rows, 499)) and not same(L.copy_edge(256, 102, 4, 4, 500, False), (rows, 499))
    a = L.copy_edge(256, 88, 5, 5, 600, False)
    # without blending every covered pixel is the tile's
    assert np.array_equal(_merge(a, blending=False), a.tiles[0])
    two = L.copy_edge(256, 88, 4, 4, 598, True)
    assert two.descs[1]["x"] + two.descs[1]["out_w"] == 100 and len(L.copy_edge_cases(500, True)) == 24


def test_ramp_length_cases():
    cases = L.ramp_length_cases()
    ovs = [tuple(c.descs[0][k] for k in ("ov_t", "ov_b", "ov_l", "ov_r")) for c in cases]
    for side in range(4):
        assert any(o[side] == 1 for o in ovs)
    assert any(o[2] == cases[0].descs[0]["out_w"] for o in ovs) and any(o[0] == cases[0].descs[0]["out_h"] for o in ovs)
    assert np.linspace(0, 1, 1).tolist() == [0.0]
    # a one-pixel ramp zeroes the only weight of the pixels it covers alone: the oracle's floor gives 0 there
    c = cases[2]                                                 # ov_l = 1: column 2 of rows the second tile does not cover
    assert np.all(_merge(c)[4:20, 2] == 0)


@pytest.mark.parametrize("cn", [1, 3])
def test_seam_hits_is_detect_seams(cn):
    for case, fixed in ((L.seam_two_tiles(cn), None), (L.seam_zero_window_tiles(cn), 2.0)):
        for (win, st) in ((16, 8), (12, 6)):
            thr = fixed or L.seam_split_threshold(case, win, st)
            hits = L.seam_hits(case.canvas, case.tiles, case.rects, thr, win, st)
            want = onp.detect_seams(case.canvas, case.tiles, [(x, y) for (x, y, _, _) in case.rects], thr, win, st)
            assert onp.merge_adjacent_seams([(x, y, win, win, s) for (_, x, y, s) in hits], win) == want
            counts = L.seam_window_counts(case, win, st)
            if thr > 1.0:                                        # every window is a hit: the hits per tile are the windows
                assert [sum(1 for h in hits if h[0] == t) for t in range(len(case.rects))] == counts
            else:
                assert 7 < len(hits) < sum(counts), (cn, win, st, len(hits), sum(counts))


def test_zero_window_tiles_are_where_they_should_be():
    for cn in (1, 3):
        case = L.seam_zero_window_tiles(cn)
        for (win, st) in ((16, 8), (12, 6)):
            c = L.seam_window_counts(case, win, st)
            assert len(c) == 7 and [n == 0 for n in c] == [True, False, False, True, True, False, True], (win, c)
        (x, y, w, h) = case.rects[5]
        assert y + h > case.canvas.shape[0]                      # a clipped tile that keeps its windows
        assert case.rects[0][2] < 12 and case.rects[3][3] < 12 and case.rects[4][0] + 12 > case.canvas.shape[1]


def test_window_ssim_all_is_window_ssim():
    case = L.seam_gray540()
    tile, canvas = case.tiles[0], case.canvas
    assert tile.shape == canvas.shape == (540, 540) and tile.dtype == np.uint8
    scores = L.window_ssim_all(tile, canvas, 8)
    assert scores.shape == (533, 533) and scores.size == 284089 > 1 << 18
    assert float(scores.max()) < 2.0
    pick = np.random.default_rng(8).integers(0, 533, (200, 2)).tolist() + [[0, 0], [532, 532], [0, 532], [532, 0]]
    for (y, x) in pick:
        want = onp.window_ssim(tile[y:y + 8, x:x + 8], canvas[y:y + 8, x:x + 8])
        assert scores[y, x] == pytest.approx(want, rel=1e-9, abs=1e-12)
