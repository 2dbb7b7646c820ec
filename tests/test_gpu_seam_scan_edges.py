"""GPU: the record cap, the repeat-with-room loop and tile lists with window-less tiles of sr_seam_scan (csrc/sr_tiles.hip:
k_seam_scan for any geometry, k_seam_scan_cells for windows of 16 every 8), on the fixtures of tests/_blend_list_cases.py.

  cap          the C ABI with room for 0 (and no buffer at all), 1 and 7 records under a scan with more hits: the count is the
               number of hits, the records are that many distinct hits with the full scan's scores (k < cap, count > cap)
  repeat       Context.seam_scan on 533^2 = 284 089 hits, more than its first buffer of 2^18: the scan is repeated with room
               and every window comes back at its position
  zero-window  seven tiles of which the first, two in the middle and the last hold no window (narrower or shorter than it, or
               clipped by the canvas to below it): their `first` / `bfirst` repeat, and the walk
               `while (tiles[t + 1].first <= gid) ++t` of both kernels has to step over them; every window is a hit, so a
               window given to the wrong tile shows as a wrong record"""
import ctypes as C

import numpy as np
import pytest

import _blend_list_cases as L
import _native

pytestmark = pytest.mark.gpu

GEOMETRIES = [(16, 8), (12, 6)]                                  # the cell kernel, the one-thread-per-window kernel


class _Scene:
    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.H, self.W = case.canvas.shape[:2]
        self.dc = ctx.upload(case.canvas)
        self.dts = [ctx.upload(t) for t in case.tiles]
        self.strides = [t.shape[1] * case.cn for t in case.tiles]

    def scan(self, win, st, thr):
        return self.ctx.seam_scan(self.dc.ptr, self.W * self.case.cn, self.H, self.W, self.case.cn, self.case.rects,
                                  [d.ptr for d in self.dts], self.strides, win, st, thr)

    def scan_capped(self, win, st, thr, cap):
        """sr_seam_scan itself with room for cap records (none at all for cap 0) -> (count, records)."""
        n = len(self.case.rects)
        rects = (_native.TileRect * n)(*[_native.TileRect(*r) for r in self.case.rects])
        ptrs = (C.c_void_p * n)(*[C.c_void_p(d.ptr) for d in self.dts])
        strides = (C.c_int64 * n)(*self.strides)
        recs = (_native.SeamRecord * cap)() if cap else None
        cnt = C.c_int(-1)
        _native.check(self.ctx.lib.sr_seam_scan(self.ctx.handle, C.c_void_p(self.dc.ptr), self.W * self.case.cn, self.H, self.W,
                                                self.case.cn, rects, ptrs, strides, n, win, st, 15, thr, recs, cap, C.byref(cnt)))
        return cnt.value, [(recs[i].tile, recs[i].x, recs[i].y, recs[i].score) for i in range(min(cap, max(cnt.value, 0)))]

    def free(self):
        for d in [self.dc] + self.dts:
            d.free()


def _same(got, want):
    assert [g[:3] for g in got] == [w[:3] for w in want]
    assert all(g[3] == pytest.approx(w[3], rel=1e-9, abs=1e-12) for g, w in zip(got, want))


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["cells", "windows"])
@pytest.mark.parametrize("cn", [3, 1])
def test_record_cap(ctx, cn, geom):
    win, st = geom
    case = L.seam_two_tiles(cn)
    thr = L.seam_split_threshold(case, win, st)
    want = L.seam_hits(case.canvas, case.tiles, case.rects, thr, win, st)
    K = len(want)
    assert K > 7
    s = _Scene(ctx, case)
    try:
        full = s.scan(win, st, thr)
        _same(full, want)
        scores = {f[:3]: f[3] for f in full}
        for cap in (0, 1, 7):
            count, recs = s.scan_capped(win, st, thr, cap)
            assert count == K, (cap, count, K)
            assert len(recs) == cap and len({r[:3] for r in recs}) == cap
            for r in recs:
                assert r[:3] in scores and r[3] == scores[r[:3]], (cap, r)
    finally:
        s.free()


def test_repeat_with_room(ctx):
    case = L.seam_gray540()
    want = L.window_ssim_all(case.tiles[0], case.canvas, 8)      # tied to oracle_np.window_ssim by the host test
    assert want.size == 284089 > 1 << 18
    s = _Scene(ctx, case)
    try:
        got = s.scan(8, 1, 2.0)
    finally:
        s.free()
    assert len(got) == want.size
    g = np.array(got, dtype=np.float64)                          # sorted by (tile, y, x)
    ys, xs = np.divmod(np.arange(want.size), 533)
    assert not g[:, 0].any() and np.array_equal(g[:, 1], xs) and np.array_equal(g[:, 2], ys)
    w = want.ravel()
    assert np.all(np.abs(g[:, 3] - w) <= np.maximum(1e-9 * np.abs(w), 1e-12))      # pytest.approx(rel=1e-9, abs=1e-12)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["cells", "windows"])
@pytest.mark.parametrize("cn", [3, 1])
def test_tiles_without_windows_in_the_list(ctx, cn, geom):
    win, st = geom
    case = L.seam_zero_window_tiles(cn)
    counts = L.seam_window_counts(case, win, st)
    assert [c == 0 for c in counts] == [True, False, False, True, True, False, True]
    s = _Scene(ctx, case)
    try:
        for thr in (2.0, L.seam_split_threshold(case, win, st)):  # every window, and the half below the median score
            want = L.seam_hits(case.canvas, case.tiles, case.rects, thr, win, st)
            got = s.scan(win, st, thr)
            _same(got, want)
            if thr == 2.0:
                assert [sum(1 for g in got if g[0] == t) for t in range(7)] == counts
    finally:
        s.free()
