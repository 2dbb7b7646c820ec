"""Host-only checks of tests/_views.py: the layout arithmetic behind the GPU view tests and its guard detector."""
import numpy as np
import pytest

import _views as V


@pytest.mark.parametrize("lay", V.LAYOUTS_U8 + V.LAYOUTS_F32, ids=V.layout_id)
@pytest.mark.parametrize("fill", V.FILLS)
def test_embed_extract_round_trip(lay, fill):
    rng = np.random.default_rng(7)
    for arr in (rng.integers(0, 256, (9, 13, 3), dtype=np.uint8), rng.integers(0, 256, (5, 1), dtype=np.uint8),
                rng.standard_normal((6, 7, 3)).astype(np.float32)):
        h, rowbytes = arr.shape[0], arr.nbytes // arr.shape[0]
        parent, first, stride = V.embed_host(arr, lay[0], lay[1], fill)
        nbytes, first2, stride2 = V.layout(h, rowbytes, *lay)
        assert (parent.nbytes, first, stride) == (nbytes, first2, stride2) and stride == rowbytes + lay[1]
        # the lead is a multiple of 256: the view's residue is the base offset's
        assert (first - lay[0]) % 256 == 0 and first - lay[0] >= V.GUARD + stride
        assert nbytes - (first + (h - 1) * stride + rowbytes) >= V.GUARD + stride
        back = V.extract_host(parent, h, rowbytes, first, stride)
        assert np.array_equal(back.view(arr.dtype).reshape(arr.shape), arr)
        assert V.guard_violations(parent, h, rowbytes, first, stride, fill) == []
        # everything outside the rectangle is fill: the parent holds exactly h * rowbytes other bytes at most
        assert int((parent != fill).sum()) <= h * rowbytes


def test_layout_lists_cover_the_residues():
    assert {b % 4 for b, _ in V.LAYOUTS_U8} == {0, 1, 2, 3} and {p % 4 for _, p in V.LAYOUTS_U8} == {0, 1, 2, 3}
    assert {b for b, _ in V.LAYOUTS_U8} >= {0, 1, 2, 3, 7, 12} and {p for _, p in V.LAYOUTS_U8} >= {0, 1, 2, 3, 13, 64}
    assert (4, 0) in V.LAYOUTS_U8                                   # dense, base misaligned by 4 bytes
    assert all(b % 4 == 0 and p % 4 == 0 for b, p in V.LAYOUTS_F32)
    assert any(b % 16 for b, _ in V.LAYOUTS_F32) and any(p % 16 for _, p in V.LAYOUTS_F32)
    assert V.FILLS[0] != V.FILLS[1] and not {0, 255} & set(V.FILLS)


@pytest.mark.parametrize("lay", [(0, 0), (3, 2), (12, 64)], ids=V.layout_id)
def test_guard_detector_fires_on_one_flipped_byte(lay):
    fill = V.FILLS[0]
    arr = np.full((6, 10), fill, dtype=np.uint8)                    # content equal to the fill: only the position can tell
    h, rowbytes = arr.shape
    parent, first, stride = V.embed_host(arr, lay[0], lay[1], fill)
    last = first + (h - 1) * stride + rowbytes
    spots = {"before": [0, first - 1], "after": [last, parent.size - 1]}
    if lay[1]:
        spots["gap row 2"] = [first + 2 * stride + rowbytes, first + 3 * stride - 1]
    for where, offs in spots.items():
        for off in offs:
            p = parent.copy()
            p[off] ^= 0x01
            bad = V.guard_violations(p, h, rowbytes, first, stride, fill)
            assert bad == [(where, off, fill ^ 0x01)], (where, off, bad)
    # a flipped byte inside the rectangle is not the guard's business ...
    p = parent.copy()
    p[first + 3 * stride] ^= 0x01
    assert V.guard_violations(p, h, rowbytes, first, stride, fill) == []
    # ... unless its row lies outside the row window
    assert V.guard_violations(p, h, rowbytes, first, stride, fill, rows=(0, 3)) == \
        [("row 3 outside the window", first + 3 * stride, fill ^ 0x01)]
    assert V.guard_violations(p, h, rowbytes, first, stride, fill, rows=(3, 6)) == []
