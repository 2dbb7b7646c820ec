"""GPU: the tile list, the copy fast path and the ramp lengths of k_feather_merge (csrc/sr_tiles.hip) through
Context.feather_merge_np, byte-equal to oracle_np.merge_tiles, on the fixtures of tests/_blend_list_cases.py (their
preconditions: tests/test_blend_list_cases_host.py).

  pile64/65/70   block (0, 0) meets exactly 64 tiles (the full list), 65 and 70 (the walk of the whole table); u8 and float32,
                 blending on and off
  spread150      a table of three ballot rounds in permuted order, every block's list at most 16 tiles long and filled from all
                 rounds (base += 64, the cnt + popc carry), every fourth tile resized
  copy path      one unresized u8 tile of 600 x 40 whose ramps end on, one pixel inside and further inside the 256 x 4 blocks
                 next to them; canvases of 600, 598 (a 2-pixel tail: the nx < 4 copy) and 500 pixels (min(bx0 + 256, cw));
                 blending off (no ramps: every inner block copies); a second tile over columns 0..99 (ncand == 2 in block
                 column 0 only)
  ramp lengths   ramps of one pixel (weight 0: the 1e-6 floor where nothing else covers the pixel) and as long as the tile"""
import numpy as np
import pytest

import _blend_list_cases as L
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu


def _check(ctx, case, blending):
    want = onp.merge_tiles(case.tiles, case.metas, case.W, case.H, 1.0, blending)
    got = ctx.feather_merge_np(case.tiles, case.descs, case.W, case.H, blending)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), (f"{case.name} blending {blending}: {len(bad)} of {case.W * case.H} pixels differ, first at (y, x) = "
                          f"{tuple(int(v) for v in bad[0])}: {got[tuple(bad[0])].tolist()} for {want[tuple(bad[0])].tolist()}")


@pytest.mark.parametrize("blending", [True, False], ids=["blend", "plain"])
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [64, 65, 70])
def test_pile_full_list_and_table_walk(ctx, n, f32, blending):
    _check(ctx, L.merge_pile(n, f32), blending)


@pytest.mark.parametrize("blending", [True, False], ids=["blend", "plain"])
def test_spread150_three_ballot_rounds(ctx, blending):
    _check(ctx, L.merge_spread150(), blending)


@pytest.mark.parametrize("second", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("cw", [600, 598, 500])
def test_copy_path_on_the_ramp_edges(ctx, cw, second):
    for case in L.copy_edge_cases(cw, second):
        for blending in (True, False):
            _check(ctx, case, blending)


def test_one_pixel_and_full_length_ramps(ctx):
    for case in L.ramp_length_cases():
        _check(ctx, case, True)
