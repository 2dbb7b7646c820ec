"""A NumPy / pure-Python restatement of the marched gather's planner and of the loop variant a work item takes.

Written from the rules the sources state in prose (csrc/sr_engine.hip: "Work lists of the marched gather"; csrc/sr_march.inc:
the header, MarchItem, march_tile_uv, k_final_march1 / k_final_marchn), cell by cell on the whole canvas instead of interval by
interval, so that a slip in either form shows up as a difference (tests/test_gpu_march_variants.py compares the two item for
item through sr_blend_plan_march_items).  No GPU and no native library is needed: weight tables come in as arguments.

Geometry.  The canvas is cut into cells of 4 x 2 pixels; only whole cells can be marched.  For one tile a cell column (row) is
    outside   no pixel of the cell lies in the tile,
    marchable every level-1 / level-2 tap of the cell is a plain interior tap (rule below),
    border    anything else.
A cell is marched when every tile that touches it is marchable there in both directions, and there are 1 .. 4 such tiles.
Rows fall into bands between two consecutive class changes of any tile; a band keeps an even number of cell rows.  Inside a
band, maximal runs of cells with the same tile list give up one cell per side to the halo lanes and are cut into strips of at
most 62 cells; strips are cut into items of `seg` steps (one step = one cell row).

Variant.  A wave handles one (item, tile) pair.  With lx0 = item.x0 - tile.x and ly0 = item.y0 - tile.y (tile-local position
of lane 0's cell):
    XO = lx0 odd,  P1 = the first own level-1 column ((lx0 - 1) >> 1) + 1 is odd,  YO = ly0 odd,
    FL = XO | YO << 1 | P1 << 2,   e0 = the first tap row (ly0 - 1) >> 1 of level 1 is even.
Only -tile.x mod 4 and ly0 mod 4 matter: they give the four (XO, P1) and the four (YO, e0) pairs.  The one-tile kernel has, on
top, the `unit1` loops: every column weight of the useful lanes, every row weight and the level-1 weight W_1 are exactly 1.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

CELL_W, CELL_H = 4, 2
MAX_TILES = 4                    # most tiles of a marched zone
STRIP_CELLS = 62                 # 64 lanes less two halo lanes
MAX_STEPS = 64                   # MARCH_SEG
MIN_STEPS = 8
ROUNDS = {1: 4.0, 2: 3.0, 3: 2.0, 4: 2.0}
W1_MARGIN = 6                    # MARCH_W1_MARGIN
MT_XO, MT_YO, MT_P1 = 1, 2, 4

Item = namedtuple("Item", "x0 y0 ncell nstep tiles")

OUTSIDE, MARCHABLE, BORDER = 0, 1, 2


def level_sizes(h, w, levels, max_levels=6):
    """[(H_i, W_i)] of the tile's pyramid: halving (rounding up) while both sides are at least 2."""
    out = [(h, w)]
    while len(out) < min(levels, max_levels) and out[-1][0] >= 2 and out[-1][1] >= 2:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def feather_width(w, h):
    return max(min(w, h) // 8, 1)


def _axis_class(first, extent, cell, size1, size2, deep, low_tap):
    """Class of the cell that starts at tile-local `first` and is `cell` pixels long, along one axis of a tile of `extent`
    pixels whose levels 1 / 2 have size1 / size2 samples there.  deep: the tile has a level 2 at all.
    The pixels first .. first + cell - 1 are pyrUp outputs of level-1 samples t .. t + cell/2 + 1 with t = (first - 1) >> 1;
    along x those samples (t .. t + 3) are formed from level-2 samples (t >> 1) .. (t >> 1) + 2; along y the march keeps a ring
    of level-1 rows, the first of which (row t) is formed from level-2 rows starting at (t - 1) >> 1, and the last one (t + 2)
    reads level-2 rows up to ((t + 1) >> 1) + 2.  Marchable: all of them exist (no reflected or clamped tap)."""
    if first + cell <= 0 or first >= extent:
        return OUTSIDE
    if not deep or first < 0 or first + cell > extent:
        return BORDER
    t = (first - 1) >> 1
    if cell == CELL_W:
        ok = t >= low_tap and t + 3 <= size1 - 1 and (t >> 1) + 2 <= size2 - 1
    else:
        ok = t >= low_tap and t + 2 <= size1 - 1 and ((t + 1) >> 1) + 2 <= size2 - 1
    return MARCHABLE if ok else BORDER


def cell_classes(rects, canvas_h, canvas_w, levels):
    """-> (xc, yc): classes [tile][cell column], [tile][cell row] over the whole cells of the canvas."""
    ncx, ncy = canvas_w // CELL_W, canvas_h // CELL_H
    xc = np.zeros((len(rects), ncx), np.uint8)
    yc = np.zeros((len(rects), ncy), np.uint8)
    for t, (x, y, w, h) in enumerate(rects):
        sz = level_sizes(h, w, levels)
        deep = len(sz) >= 3
        h1, w1 = sz[1] if len(sz) > 1 else (0, 0)
        h2, w2 = sz[2] if deep else (0, 0)
        for c in range(ncx):
            xc[t, c] = _axis_class(CELL_W * c - x, w, CELL_W, w1, w2, deep, 0)
        for r in range(ncy):
            yc[t, r] = _axis_class(CELL_H * r - y, h, CELL_H, h1, h2, deep, 1)
    return xc, yc


def _runs(keys):
    """Maximal runs [a, b) of equal consecutive keys."""
    out, a = [], 0
    for i in range(1, len(keys) + 1):
        if i == len(keys) or keys[i] != keys[a]:
            out.append((a, i))
            a = i
    return out


def strips(rects, canvas_h, canvas_w, levels):
    """-> list of (first cell column, end, first cell row, end, tile list), in the planner's order: bands top to bottom, runs
    left to right, strips left to right."""
    xc, yc = cell_classes(rects, canvas_h, canvas_w, levels)
    ncx, ncy = xc.shape[1], yc.shape[1]
    if ncx < 3 or ncy < 2 or len(rects) > 128:
        return []
    # a column boundary is where any tile's class changes; runs never cross the canvas' whole-cell range.  Cells of one run
    # share their tile list, and two neighbouring column intervals with the same list are one run, so the runs are simply the
    # maximal stretches of cells with the same (valid) list.
    out = []
    for ra, rb in _runs([tuple(yc[:, r]) for r in range(ncy)]):
        re_ = ra + (rb - ra) // 2 * 2
        if re_ - ra < 2:
            continue
        row_cls = yc[:, ra]
        lists = []
        for c in range(ncx):
            touching = [t for t in range(len(rects)) if xc[t, c] != OUTSIDE and row_cls[t] != OUTSIDE]
            ok = touching and len(touching) <= MAX_TILES and all(xc[t, c] == MARCHABLE and row_cls[t] == MARCHABLE for t in touching)
            lists.append(tuple(touching) if ok else None)
        # an invalid cell separates runs even from another invalid cell: give each its own key
        keys = [l if l is not None else ("bad", c) for c, l in enumerate(lists)]
        for ca, cb in _runs(keys):
            if lists[ca] is None:
                continue
            ua, ub = ca + 1, cb - 1                                  # the halo lanes' cells
            nu = ub - ua
            if nu < 1:
                continue
            ns = -(-nu // STRIP_CELLS)
            for s in range(ns):
                out.append((ua + nu * s // ns, ua + nu * (s + 1) // ns, ra, re_, lists[ca]))
    return out


def segment_rule(nt, total_steps, num_cu, rounds_env=None, taper=True):
    """-> (seg, tail): steps of a full item of the `nt`-tile list and the number of trailing strip-steps that get shorter
    items.  rounds_env: the SR_MARCH_ROUNDS string or None."""
    rounds = ROUNDS[nt]
    if rounds_env:
        vals = []
        for part in rounds_env.split(",")[:3]:
            try:
                vals.append(float(part))
            except ValueError:
                break
        if vals:
            v = vals[min({1: 0, 2: 1}.get(nt, 2), len(vals) - 1)]
            if v > 0:
                rounds = v
    slots = num_cu * 8 // nt
    want = max(int(slots * rounds), 1)
    seg = min(MAX_STEPS, max(MIN_STEPS, total_steps // want)) // 2 * 2
    tail = min(max(slots, 1) * seg, total_steps // 3) if taper and seg > MIN_STEPS else 0
    return seg, tail


def plan_items(rects, canvas_h, canvas_w, levels, num_cu, rounds_env=None, taper=True):
    """-> {nt: [Item]} for nt = 1 .. 4, launch order."""
    st = strips(rects, canvas_h, canvas_w, levels)
    items = {nt: [] for nt in range(1, MAX_TILES + 1)}
    for nt in items:
        mine = [s for s in st if len(s[4]) == nt]
        total = sum(s[3] - s[2] for s in mine)
        if not total:
            continue
        seg, tail = segment_rule(nt, total, num_cu, rounds_env, taper)
        done = 0
        for ca, cb, ra, rb, tl in mine:
            r = ra
            while r < rb:
                left = total - done
                if left <= tail // 4:
                    n = MIN_STEPS
                elif left <= tail:
                    n = max(MIN_STEPS, seg // 4 * 2)
                else:
                    n = seg
                n = min(n, rb - r)
                items[nt].append(Item(CELL_W * (ca - 1), CELL_H * r, cb - ca, n, tl))
                r += n
                done += n
    return items


def marched_cell_counts(items, canvas_h, canvas_w, rect_items=()):
    """How often each cell of ceil(W / 4) x ceil(H / 2) is covered by the items' useful lanes (lanes 1 .. ncell, 2 nstep rows)
    and by the rectangles (x, y in pixels, w, h in cells)."""
    cnt = np.zeros((-(-canvas_h // CELL_H), -(-canvas_w // CELL_W)), np.int32)
    for lst in items.values():
        for it in lst:
            assert it.x0 % CELL_W == 0 and it.y0 % CELL_H == 0
            cx, cy = it.x0 // CELL_W + 1, it.y0 // CELL_H
            assert cx >= 1 and cy >= 0 and cx + it.ncell <= cnt.shape[1] and cy + it.nstep <= cnt.shape[0], it
            cnt[cy:cy + it.nstep, cx:cx + it.ncell] += 1
    for (x, y, w, h) in rect_items:
        assert x % CELL_W == 0 and y % CELL_H == 0 and x >= 0 and y >= 0
        cx, cy = x // CELL_W, y // CELL_H
        assert cx + w <= cnt.shape[1] and cy + h <= cnt.shape[0], (x, y, w, h)
        cnt[cy:cy + h, cx:cx + w] += 1
    return cnt


# ---- which loop a wave takes ---------------------------------------------------------------------------------------------
def phase_flags(item, rect):
    """-> (FL, e0) of the wave that handles `rect` in `item`."""
    lx0, ly0 = item.x0 - rect[0], item.y0 - rect[1]
    own = ((lx0 - 1) >> 1) + 1
    fl = (MT_XO if lx0 & 1 else 0) | (MT_YO if ly0 & 1 else 0) | (MT_P1 if own & 1 else 0)
    return fl, (((ly0 - 1) >> 1) & 1) == 0


def is_unit1(item, rect, lut):
    """The one-tile kernel's test for its unit-weight loops.  lut: the tile's weight table, fw + 1 entries."""
    x, y, w, h = rect
    fw = feather_width(w, h)
    assert len(lut) == fw + 1
    if lut[fw] != 1.0:
        return False
    ly0 = item.y0 - y
    if min(ly0, h - 2 * item.nstep - ly0) < fw + W1_MARGIN:          # (implies the row weights' bound, fw)
        return False
    # column weights of the useful lanes' four pixels
    for lane in range(1, item.ncell + 1):
        lx = item.x0 + CELL_W * lane - x
        for k in range(CELL_W):
            if lut[min(lx + k, w - 1 - lx - k, fw)] != 1.0:
                return False
    # W_1: all 64 lanes, the ones beyond the right halo lane repeat it
    for lane in range(64):
        lx = item.x0 + CELL_W * min(lane, item.ncell + 1) - x
        if min(lx, w - CELL_W - lx) < fw + W1_MARGIN:
            return False
    return True


def variant_keys(item, rects, luts):
    """Keys of the loops the item's waves take: (1, 'unit1', FL, e0) / (1, 'general', e0) / (nt, FL, e0)."""
    nt = len(item.tiles)
    out = []
    for t in item.tiles:
        fl, e0 = phase_flags(item, rects[t])
        if nt == 1:
            out.append((1, "unit1", fl, e0) if is_unit1(item, rects[t], luts[t]) else (1, "general", e0))
        else:
            out.append((nt, fl, e0))
    return out


def all_variant_keys():
    keys = {(1, "unit1", fl, e0) for fl in range(8) for e0 in (False, True)}
    keys |= {(1, "general", e0) for e0 in (False, True)}
    keys |= {(nt, fl, e0) for nt in (2, 3, 4) for fl in range(8) for e0 in (False, True)}
    assert len(keys) == 66
    return keys


def keys_of(items, rects, luts):
    out = set()
    for lst in items.values():
        for it in lst:
            out.update(variant_keys(it, rects, luts))
    return out


def items_from_flat(flat, nt):
    """The accessor's 8 ints per item -> [Item]."""
    a = np.asarray(flat, np.int64).reshape(-1, 8)
    return [Item(int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(v) for v in r[4:4 + nt])) for r in a]
