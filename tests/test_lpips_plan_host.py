"""CPU: the per-tile plan of the LPIPS and DISTS forwards (csrc/sr_vgg_ranges.h: lp_geometry, lp_ranges, lp_plan) against a brute force.

Whether a tiled LPIPS equals the untiled one rests on that range algebra alone: what a tile owns of every tap must partition the
tap, and what it computes of every activation must cover what its owned outputs depend on.  sr_lpips_tile_plan returns, without
a GPU, what sr_lpips_u8 itself calls per tile, sr_dists_tile_plan the same for sr_dists_u8.  The restatement here uses no interval arithmetic: it walks the layers backwards
one axis at a time with SETS of indices (an output index o of a k / s / p layer depends on the inputs o s - p .. o s - p + k - 1
that exist), and the owned cells come from tests/_lpips_ref.owned, written from the rule's statement.  Both axes are independent
in the plan (a tile that owns rows but no columns of a tap still plans the rows), and so they are here."""
import functools

import pytest

import _lpips_ref as R
import _native
from oracle import lpips_oracle as lo

SIDES = (16, 17, 31, 33, 35, 47, 53, 64, 67, 99, 131, 300)
TILES = (0, 16, 32, 48, 64, 128)


def _layers(net):
    """[(kind, k, s, p, cout or None)] in forward order; a tap's k is its index."""
    out = []
    if net == "dists":                     # the image as stage 0, VGG16's convolutions, a padded 3 / 2 / 1 pooling for every max pooling
        out.append(("tap", 0, 1, 0, None))
        for layer in lo.ARCH["vgg"]:
            if layer[0] == "conv":
                out.append(("conv", layer[3], layer[4], layer[5], layer[1]))
            elif layer[0] == "pool":
                out.append(("pool", 3, 2, 1, None))
            else:
                out.append(("tap", layer[1] + 1, 1, 0, None))
        return out
    for layer in lo.ARCH[net]:
        if layer[0] == "conv":
            out.append(("conv", layer[3], layer[4], layer[5], layer[1]))
        elif layer[0] == "pool":
            out.append(("pool", layer[1], layer[2], 0, None))
        else:
            out.append(("tap", layer[1], 1, 0, None))
    return out


def _tap_strides(net):
    s, out = 1, []
    for kind, _, st, _, _ in _layers(net):
        if kind == "tap":
            out.append(s)
        else:
            s *= st
    return out


@functools.lru_cache(maxsize=None)
def _extents(net, n):
    """Extent of every activation along one axis of n input pixels, or None where the net refuses it."""
    ext = [n]
    for kind, k, s, p, _ in _layers(net):
        if kind == "tap":
            continue
        if ext[-1] + 2 * p < k:
            return None
        ext.append((ext[-1] + 2 * p - k) // s + 1)
    return tuple(ext)


def _channels(net):
    c = [3]
    for kind, _, _, _, cout in _layers(net):
        if kind != "tap":
            c.append(cout if kind == "conv" else c[-1])
    return c


@functools.lru_cache(maxsize=None)
def _brute_axis(net, n, tile, t, ntiles):
    """Per activation the exact set of indices tile t needs along an axis of n pixels, and per tapped activation the owned
    [a, b)."""
    ext = _extents(net, n)
    strides = _tap_strides(net)
    need = [set() for _ in ext]
    own = {}
    # the activation every layer reads
    act, j = [], 0
    for kind, *_ in _layers(net):
        act.append(j)
        j += kind != "tap"
    for (kind, k, s, p, _), ai in reversed(list(zip(_layers(net), act))):
        if kind == "tap":
            a, b = R.owned(ext[ai], strides[k], tile, t, ntiles)
            own[ai] = (a, b)
            need[ai] |= set(range(a, b))
            continue
        for o in need[ai + 1]:
            need[ai] |= {i for i in range(o * s - p, o * s - p + k) if 0 <= i < ext[ai]}
    return need, own


def _check_axis(net, n, tile, t, ntiles, acts, need_key, own_key, ext_key):
    ext = _extents(net, n)
    need, own = _brute_axis(net, n, tile, t, ntiles)
    assert [a[ext_key] for a in acts] == list(ext)
    for j, a in enumerate(acts):
        lo_, hi_ = a[need_key]
        if not need[j]:
            assert hi_ <= lo_, (net, n, tile, t, j, a[need_key])              # empty exactly where nothing is needed
        else:
            assert (lo_, hi_) == (min(need[j]), max(need[j]) + 1), (net, n, tile, t, j, a[need_key])
        if j in own:
            oa, ob = a[own_key]
            assert (oa, max(oa, ob)) == own[j], (net, n, tile, t, j, a[own_key])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("net", ["alex", "vgg", "dists"])
def test_plan_matches_brute_force(net, tile):
    lib = _native.load()
    chans = _channels(net)
    tapped = [j for j, _ in sorted(_brute_axis(net, 300, 0, 0, 1)[1].items())]
    assert len(tapped) == (6 if net == "dists" else 5)
    assert _tap_strides(net) == ([1, 1, 2, 4, 8, 16] if net == "dists" else R.tap_strides(net))
    count = lib.sr_dists_tile_count if net == "dists" else lib.sr_lpips_tile_count
    seen = 0
    for h in SIDES:
        for w in SIDES:
            n = _native.C.c_int(0)
            if _extents(net, h) is None or _extents(net, w) is None:
                with pytest.raises(_native.SrShapeError):
                    _native.lpips_tile_plan(net, h, w, tile, 0)
                continue
            seen += 1
            _native.check(count(h, w, tile, _native.C.byref(n)))
            tiles_y, tiles_x = R.tile_grid(h, w, tile)
            assert n.value == tiles_y * tiles_x
            with pytest.raises(ValueError):
                _native.lpips_tile_plan(net, h, w, tile, n.value)               # one past the last plan
            sizes = [(_extents(net, h)[j], _extents(net, w)[j]) for j in tapped]
            if net != "dists":
                assert sizes == lo.layer_sizes(net, h, w)
            cover = [[[0] * sw for _ in range(sh)] for sh, sw in sizes]
            for t in range(n.value):
                plan = _native.lpips_tile_plan(net, h, w, tile, t)
                acts = plan["acts"]
                assert [a["C"] for a in acts] == chans
                _check_axis(net, h, tile, t // tiles_x, tiles_y, acts, "need_y", "own_y", "H")
                _check_axis(net, w, tile, t % tiles_x, tiles_x, acts, "need_x", "own_x", "W")
                for j, a in enumerate(acts[1:], 1):
                    rows, cols = max(a["need_y"][1] - a["need_y"][0], 0), max(a["need_x"][1] - a["need_x"][0], 0)
                    assert a["pitch"] >= cols and a["pitch"] % 4 == 0
                    assert plan["buffer_floats"] >= a["C"] * rows * a["pitch"]
                for k, j in enumerate(tapped):
                    (ya, yb), (xa, xb) = acts[j]["own_y"], acts[j]["own_x"]
                    for y in range(ya, yb):
                        row = cover[k][y]
                        for x in range(xa, xb):
                            row[x] += 1
            for k in range(len(tapped)):                                        # the owned cells partition every tap
                assert all(v == 1 for row in cover[k] for v in row), (net, h, w, tile, k)
    assert seen >= 100


def test_plan_empty_cells_exist_at_small_tiles():
    """The geometries test_gpu_lpips_small.py relies on for the forward's empty-range branches: tiles of 16 on VGG 35 x 53
    own nothing of taps 2 / 3 / 4 in 4 / 6 / 6 of 12 tiles, 9 of 24 tiles of AlexNet 63 x 95 own nothing of some tap, and a
    tile whose deeper activations are not needed plans them empty."""
    z = (R.cell_sizes("vgg", 35, 53, 16) == 0).sum(axis=0)
    assert z.tolist() == [0, 0, 4, 6, 6]
    assert int((R.cell_sizes("alex", 63, 95, 16) == 0).any(axis=1).sum()) == 9
    assert (R.cell_sizes("alex", 79, 131, 32) == 0).sum(axis=0).tolist()[:2] == [3, 3]
    plan = _native.lpips_tile_plan("vgg", 35, 53, 16, 11)                       # the last tile: rows 32 .. 34, columns 48 .. 52
    last = plan["acts"][-1]
    assert last["need_y"][1] <= last["need_y"][0] or last["need_x"][1] <= last["need_x"][0]


def test_plan_refusals():
    with pytest.raises(ValueError):
        _native.lpips_tile_plan("vgg", 64, 64, 24, 0)                           # not a multiple of 16
    with pytest.raises(ValueError):
        _native.lpips_tile_plan("vgg", 64, 64, 16, -1)
    with pytest.raises(_native.SrShapeError):
        _native.lpips_tile_plan("alex", 30, 64, 0, 0)
    with pytest.raises(ValueError):
        _native.lpips_tile_plan("dists", 64, 64, 24, 0)
    assert len(_native.lpips_tile_plan("dists", 1, 1, 0, 0)["acts"]) == 18      # DISTS refuses no size
