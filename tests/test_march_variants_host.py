"""CPU: the geometry list of tests/_march_geoms.py reaches every specialised loop of the marched canvas gather.

The marched kernels (csrc/sr_march.inc) are compiled as a fan of straight-line loops and an item picks one at run time:
    k_final_march1     (1, 'unit1', FL, e0)  x 16      (1, 'general', e0)  x 2
    k_final_marchn<NT> (NT, FL, e0)          x 16      for NT = 2, 3, 4
with FL = MT_XO | MT_YO | MT_P1 and e0 the parity of the first level-1 row: 66 loops.  This is a coverage proof on the
restatement alone (tests/_march_ref.py); tests/test_gpu_march_variants.py shows on the device that the planner's items are the
restatement's, so that the keys promised here are the loops that ran.  The 66 / 66 coverage, the 16 geometries and the 1 MP per
canvas are conditions: a change of the planner that loses a loop has to be answered with another geometry, not a smaller set."""
import numpy as np
import pytest

import _march_geoms as G
import _march_ref as R
import _native

NUM_CU = 256                                         # an MI355X; the small canvases here give the same lists for any count


def _keys(geom, **kw):
    return G.expected_keys(geom, _native.weight_lut, NUM_CU, **kw)


def test_list_is_small():
    assert len(G.GEOMETRIES) <= 16
    assert len({g.name for g in G.GEOMETRIES}) == len(G.GEOMETRIES)
    for g in G.GEOMETRIES:
        assert g.H * g.W <= 1_000_000, g.name
        for (x, y, w, h) in g.rects:
            assert x >= 0 and y >= 0 and x + w <= g.W and y + h <= g.H, g.name
    assert set(G.STORAGE_SUBSET) <= set(G.BY_NAME) and set(G.GUARDED) <= set(G.BY_NAME)
    assert any(n.startswith("grid-") for n in G.GUARDED) and any(n.startswith("tj-") for n in G.GUARDED)


def test_every_loop_is_reached():
    want = R.all_variant_keys()
    got = set()
    for g in G.GEOMETRIES:
        got |= _keys(g)
    assert got <= want
    assert not (want - got), f"loops no geometry reaches: {sorted(want - got, key=str)}"
    # the cosine geometries alone reach them, too: the linear and the sigmoid grid are there for their weight tables
    cos = set()
    for g in G.GEOMETRIES:
        if g.weight == "cosine":
            cos |= _keys(g)
    assert cos == want


def test_three_tile_zones_come_from_the_junctions():
    for g in G.GEOMETRIES:
        items = G.expected_items(g, NUM_CU)
        if g.name.startswith("tj-"):
            assert items[3] and items[2] and items[1] and not items[4], g.name
        else:
            assert items[4] and items[2] and items[1] and not items[3], g.name


def test_storage_subset_holds_every_x_phase():
    """fp32 level-1 planes and gray tiles run on STORAGE_SUBSET only: every tile x mod 4 (the alignment of the lane's level-1
    pair and of its pixel bytes) with either parity of the first level-1 row, in the one-tile and the two-tile kernel."""
    want = {(p, e0) for p in range(4) for e0 in (False, True)}
    for nt in (1, 2):
        got = set()
        for name in G.STORAGE_SUBSET:
            g = G.BY_NAME[name]
            got |= G.phase_pairs(G.expected_items(g, NUM_CU), g.rects, nt)
        assert got == want, (nt, sorted(want - got))


def test_marched_cells_are_covered_once():
    for g in G.GEOMETRIES:
        for long_items in (False, True):
            cnt = R.marched_cell_counts(G.expected_items(g, NUM_CU, long_items), g.H, g.W)
            assert cnt.max() == 1 and 0 < cnt.sum() < cnt.size, g.name


@pytest.mark.parametrize("name", G.GRIDS)
def test_long_items_of_the_grids(name):
    """One round per list (SR_MARCH_ROUNDS a small fraction) with the taper on: the one- and two-tile lists hold items of
    MARCH_SEG steps, the taper cuts the end of each list into more items than uniform segments give, and -- except under
    sigmoid weights -- an item of 64 steps takes a unit-weight loop (`unit1` depends on the item's length)."""
    g = G.BY_NAME[name]
    luts = G.luts(g, _native.weight_lut)
    for cu in (64, NUM_CU, 304):
        tapered = G.expected_items(g, cu, long_items=True)
        uniform = G.expected_items(g, cu, long_items=True, taper=False)
        for nt in (1, 2):
            assert max(it.nstep for it in tapered[nt]) == R.MAX_STEPS, (nt, cu)
            assert len(tapered[nt]) > len(uniform[nt]), (nt, cu)
        assert tapered == G.expected_items(g, NUM_CU, long_items=True), "the lists do not depend on the device's size here"
    long_unit = [it for it in tapered[1] if it.nstep == R.MAX_STEPS and R.variant_keys(it, g.rects, luts)[0][1] == "unit1"]
    assert bool(long_unit) == (g.weight != "sigmoid")


def test_default_items_are_eight_steps():
    for g in G.GEOMETRIES:
        for cu in (64, NUM_CU, 304):
            items = G.expected_items(g, cu)
            assert all(it.nstep <= R.MIN_STEPS and it.nstep % 2 == 0 for lst in items.values() for it in lst)
            assert items == G.expected_items(g, NUM_CU)


def test_weight_tables_decide_unit1():
    """`unit1` needs lut[fw] == 1: exact for the cosine and the linear ramp, not for the sigmoid (1 / (1 + e^-5))."""
    for g in G.GEOMETRIES:
        tops = {float(l[-1]) for l in G.luts(g, _native.weight_lut)}
        unit = {k for k in _keys(g) if k[0] == 1 and k[1] == "unit1"}
        if g.weight == "sigmoid":
            assert all(t != 1.0 for t in tops) and not unit
        else:
            assert tops == {1.0}
            if g.name.startswith("grid-"):
                assert unit, g.name
    assert {k[1] for k in _keys(G.BY_NAME["grid-sigmoid"]) if k[0] == 1} == {"general"}


def test_phase_rule():
    """The rule DESIGN.md states: -x mod 4 of the tile gives (XO, P1), (y0 - y) mod 4 gives (YO, e0)."""
    for dx in range(8):
        for dy in range(8):
            it = R.Item(16, 24, 3, 8, (0,))
            fl, e0 = R.phase_flags(it, (dx, dy, 100, 100))
            px, py = (16 - dx) % 4, (24 - dy) % 4
            assert (bool(fl & R.MT_XO), bool(fl & R.MT_P1)) == {0: (False, False), 1: (True, True), 2: (False, True), 3: (True, False)}[px]
            assert (bool(fl & R.MT_YO), e0) == {0: (False, False), 1: (True, True), 2: (False, True), 3: (True, False)}[py]
