"""Padded, offset, guarded views for the tests of the strided C ABI (include/sr_hip.h takes (pointer, stride) pairs).

A view is an h x rowbytes rectangle inside a larger parent allocation:

    parent:  [ lead: >= GUARD bytes and one spare row | base_off | row 0 | pad | row 1 | pad | ... | row h-1 | tail ]

Every byte of the parent outside the rectangle holds `fill`.  The lead is a multiple of 256 bytes (device allocations are
256-byte aligned), so the residue of the view's first byte modulo 4 / 16 is exactly `base_off`; the tail holds the last
row's pad, one spare row and GUARD bytes.  An over-read or over-write of one vector therefore stays inside the allocation
and shows up as a changed result or as a failed check_guard, never as a fault.

The layout arithmetic is NumPy only (layout / embed_host / extract_host / guard_violations; tests/test_views_host.py);
embed / out_view / check_guard add the device copies."""
from __future__ import annotations

import numpy as np

GUARD = 256                      # least number of bytes before and after a view (beside the spare rows)

# (base_off, pad) in bytes for u8 buffers: every base residue mod 4 with every stride residue mod 4, a base that is a multiple
# of 4 but not of 16 (12), one that is not a multiple of 4 beyond the first dword (7), a large gap (64) and the dense aligned
# layout.  One shared list: tests walk it, they do not take its cross product with their shapes.
LAYOUTS_U8 = [(0, 0), (1, 3), (2, 1), (3, 2), (7, 13), (12, 64), (0, 1), (4, 0), (12, 3), (1, 0), (3, 64), (2, 13)]
# fp32 buffers: offsets and pads are multiples of 4 bytes, some of them not multiples of 16
LAYOUTS_F32 = [(0, 0), (4, 4), (8, 12), (12, 64), (16, 20), (4, 0)]
# two fills, both unlike a border value (0, 255, a replicated edge pixel): a kernel that reads outside its rectangle gives
# different results under the two
FILLS = (0x5B, 0xA6)


def layout_id(lay) -> str:
    return f"off{lay[0]}-pad{lay[1]}"


def pick(layouts, k: int):
    """k-th layout of a list, cyclic: independent input / output layouts from one list without a cross product."""
    return layouts[k % len(layouts)]


def layout(h: int, rowbytes: int, base_off: int, pad: int):
    """-> (parent bytes, offset of the view's first byte, row stride)."""
    assert h >= 0 and rowbytes >= 0 and base_off >= 0 and pad >= 0
    stride = rowbytes + pad
    lead = GUARD + -(-max(stride, 1) // 256) * 256               # GUARD + one spare row, rounded up to 256
    first = lead + base_off
    nbytes = first + h * stride + stride + GUARD
    return nbytes, first, stride


def _rows(parent: np.ndarray, h: int, rowbytes: int, first: int, stride: int) -> np.ndarray:
    """The rectangle as a strided (h, rowbytes) window of the parent's bytes (no copy)."""
    return np.lib.stride_tricks.as_strided(parent[first:], shape=(h, rowbytes), strides=(stride, 1), writeable=parent.flags.writeable)


def embed_host(array: np.ndarray, base_off: int, pad: int, fill: int):
    """-> (parent uint8 array, first, stride): `array` (rows = its first axis) laid into a parent full of `fill`."""
    a = np.ascontiguousarray(array)
    h = a.shape[0] if a.ndim else 1
    rowbytes = a.nbytes // max(h, 1)
    nbytes, first, stride = layout(h, rowbytes, base_off, pad)
    parent = np.full(nbytes, fill, dtype=np.uint8)
    if h and rowbytes:
        _rows(parent, h, rowbytes, first, stride)[:] = a.view(np.uint8).reshape(h, rowbytes)
    return parent, first, stride


def extract_host(parent: np.ndarray, h: int, rowbytes: int, first: int, stride: int) -> np.ndarray:
    """The rectangle's bytes as a dense (h, rowbytes) uint8 array."""
    return np.ascontiguousarray(_rows(parent, h, rowbytes, first, stride))


def guard_violations(parent: np.ndarray, h: int, rowbytes: int, first: int, stride: int, fill: int, rows=None):
    """Bytes outside the rectangle that differ from `fill` -> list of (where, byte offset in the parent, value), where in
    'before' / 'gap row r' / 'after' / 'row r outside the window'.  rows = (a, b): rows outside [a, b) count as guard too."""
    mask = np.ones(parent.shape, dtype=bool)
    a, b = (0, h) if rows is None else rows
    if rowbytes:
        _rows(mask, h, rowbytes, first, stride)[a:b] = False
    bad = np.flatnonzero(mask & (parent != fill))
    out = []
    for off in bad[:8].tolist():
        if off < first:
            where = "before"
        elif off >= first + (h - 1) * stride + rowbytes if h else True:
            where = "after"
        else:
            r, c = divmod(off - first, stride)
            where = f"gap row {r}" if c >= rowbytes else f"row {r} outside the window"
        out.append((where, off, int(parent[off])))
    return out


class Parent:
    """One guarded device allocation holding one view."""

    def __init__(self, buf, nbytes, first, stride, h, rowbytes, fill, lay):
        self.buf, self.nbytes, self.first, self.stride = buf, nbytes, first, stride
        self.h, self.rowbytes, self.fill, self.lay = h, rowbytes, fill, lay

    @property
    def ptr(self) -> int:
        return self.buf.ptr + self.first

    def free(self):
        self.buf.free()


def embed(ctx, array: np.ndarray, base_off: int, pad: int, fill: int):
    """Uploads a parent full of `fill` that holds `array` as a view -> (parent, device pointer of the view, stride)."""
    host, first, stride = embed_host(array, base_off, pad, fill)
    a = np.ascontiguousarray(array)
    h = a.shape[0]
    p = Parent(ctx.upload(host), host.nbytes, first, stride, h, a.nbytes // max(h, 1), fill, (base_off, pad))
    assert p.buf.ptr % 256 == 0, "device allocations are expected to be 256-byte aligned"
    return p, p.ptr, stride


def out_view(ctx, h: int, rowbytes: int, base_off: int, pad: int, fill: int):
    """A parent full of `fill` with an h x rowbytes output view that is not yet written -> (parent, pointer, stride)."""
    nbytes, first, stride = layout(h, rowbytes, base_off, pad)
    buf = ctx.alloc(nbytes)
    ctx.memset(buf.ptr, fill, nbytes)
    p = Parent(buf, nbytes, first, stride, h, rowbytes, fill, (base_off, pad))
    assert buf.ptr % 256 == 0, "device allocations are expected to be 256-byte aligned"
    return p, p.ptr, stride


def check_guard(ctx, parent: Parent, dtype=np.uint8, shape=None, rows=None, what: str = ""):
    """Downloads the parent, asserts that every byte outside the view (and, with rows = (a, b), every row of the view outside
    [a, b)) still equals the fill, and returns the rectangle as `dtype` (reshaped to `shape` when given)."""
    host = ctx.download(parent.buf.ptr, (parent.nbytes,), np.uint8)
    bad = guard_violations(host, parent.h, parent.rowbytes, parent.first, parent.stride, parent.fill, rows)
    assert not bad, (f"{what or 'output'} view {layout_id(parent.lay)} ({parent.h} x {parent.rowbytes} bytes, fill "
                     f"{parent.fill:#x}): bytes outside the view were written: {bad}")
    rect = extract_host(host, parent.h, parent.rowbytes, parent.first, parent.stride).view(dtype)
    return rect.reshape(shape) if shape is not None else rect
