"""The tile arrangements of the march-variant tests, in one place: tests/test_march_variants_host.py proves on the restatement
(tests/_march_ref.py) that they reach every specialised loop of the marched gather, tests/test_gpu_march_variants.py runs them.

Two families, both as small as the rules allow:
  * 2 x 2 grids of 424 x 400 tiles with 96 px of overlap (canvas about 707 x 755): 1-, 2- and 4-tile zones.  424 px of width
    make the single-coverage run longer than one strip of 62 cells, so that one of its two strips lies wholly more than
    fw + 6 = 56 px inside the tile -- the condition of the unit-weight loops; 400 px of height leave bands of about 150 steps,
    enough for items of 64 steps.
  * T-junctions: two 160 x 136 tiles above one wide tile, 48 px of overlap (canvas about 227 x 275): 3-tile zones, which a
    regular grid never has.
The whole arrangement is shifted by (dx, dy) and its second column / row by a further (ex, ey), all in 0 .. 3: a tile's
x mod 4 and its distance to an item's first row mod 4 select the loop.  A shifted arrangement leaves up to 3 empty pixels at
the top and left (weight sum 0), which the oracle and the kernels both define."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import _march_ref as R

LEVELS = 6
Geometry = namedtuple("Geometry", "name rects H W weight")


def _grid(name, dx, dy, ex, ey, weight="cosine", tw=424, th=400, ov=96):
    sx, sy = tw - ov + ex, th - ov + ey
    rects = [(dx, dy, tw, th), (dx + sx, dy, tw, th), (dx, dy + sy, tw, th), (dx + sx, dy + sy, tw, th)]
    return Geometry(name, rects, dy + sy + th, dx + sx + tw, weight)


def _tjunction(name, dx, dy, ex, ey, weight="cosine", tw=160, th=136, ov=48):
    sx, sy = tw - ov + ex, th - ov + ey
    rects = [(dx, dy, tw, th), (dx + sx, dy, tw, th), (dx, dy + sy, sx + tw, th)]
    return Geometry(name, rects, dy + sy + th, dx + sx + tw, weight)


GEOMETRIES = [
    _grid("grid-0013", 0, 0, 1, 3),
    _grid("grid-2013", 2, 0, 1, 3),
    _grid("grid-0111", 0, 1, 1, 1),
    _grid("grid-2111", 2, 1, 1, 1),
    _grid("grid-0012", 0, 0, 1, 2),
    _grid("grid-2012", 2, 0, 1, 2),
    _tjunction("tj-0011", 0, 0, 1, 1),
    _tjunction("tj-1013", 1, 0, 1, 3),
    _tjunction("tj-2011", 2, 0, 1, 1),
    _tjunction("tj-3013", 3, 0, 1, 3),
    _tjunction("tj-0111", 0, 1, 1, 1),
    _tjunction("tj-2111", 2, 1, 1, 1),
    _grid("grid-linear", 1, 2, 2, 0, weight="linear"),
    _grid("grid-sigmoid", 3, 3, 0, 1, weight="sigmoid"),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
GRIDS = [g.name for g in GEOMETRIES if g.name.startswith("grid-")]
# the geometries that also run with fp32 level-1 planes (SR_G1_U16=0) and as gray tiles (CN = 1): together they hold every
# x phase (tile x mod 4) with either parity of the first level-1 row, in the one-tile and in the two-tile kernel (the two
# grids alone do; the T-junction adds the three-tile kernel)
STORAGE_SUBSET = ["grid-0013", "grid-2012", "tj-1013"]
# one grid and one T-junction also blend into a guarded, prefilled canvas view
GUARDED = ["grid-0111", "tj-1013"]
# the long-item form: one round, so that items are as long as the band allows (MARCH_SEG = 64 steps), tapered at the list's end
LONG_ROUNDS = "0.0001"


def luts(geom, weight_lut):
    """Per tile the weight table: weight_lut(fw, weight type) -> fw + 1 floats (sr_weight_lut)."""
    return [np.asarray(weight_lut(R.feather_width(w, h), geom.weight), np.float32) for (_, _, w, h) in geom.rects]


def expected_items(geom, num_cu, long_items=False, taper=True):
    return R.plan_items(geom.rects, geom.H, geom.W, LEVELS, num_cu, LONG_ROUNDS if long_items else None, taper)


def expected_keys(geom, weight_lut, num_cu=256, long_items=False):
    return R.keys_of(expected_items(geom, num_cu, long_items), geom.rects, luts(geom, weight_lut))


def phase_pairs(items, rects, nt):
    """{(tile x mod 4, e0)} over the waves of the nt-tile list."""
    out = set()
    for it in items[nt]:
        for t in it.tiles:
            out.add((rects[t][0] % 4, R.phase_flags(it, rects[t])[1]))
    return out


def make_tiles(geom, cn=3, seed=7):
    """Tiles that disagree where they overlap: a smooth pattern with a per-tile offset and phase plus seeded noise; the top
    half of tile 1 saturated, the lower left of tile 0 zero (the 16-bit row and column sums at their extremes)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (_, _, w, h) in enumerate(geom.rects):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 64 * np.sin(xx / 37.0 + i) + 48 * np.cos(yy / 23.0 + 0.5 * i)
        img = np.clip(base[..., None] + rng.integers(-12, 13, (h, w, cn)) + 7 * i, 0, 255).astype(np.uint8)
        out.append(img)
    out[1][: geom.rects[1][3] // 2] = 255
    out[0][geom.rects[0][3] // 2:, : geom.rects[0][2] // 3] = 0
    return [np.ascontiguousarray(t if cn > 1 else t[..., 0]) for t in out]
