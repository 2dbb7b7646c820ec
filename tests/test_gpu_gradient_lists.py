"""GPU: the tile lists, cosine tables and chunk edges of sr_gradient_fusion (csrc/sr_gradient.hip: list_tiles, k_grad_row,
k_grad_col) on the fixtures of tests/_blend_list_cases.py, whose preconditions tests/test_blend_list_cases_host.py asserts.

Every case is called through Context.gradient_fusion so that the workspace can be downloaded, and checked twice:
  * the u8 canvas is byte-equal to _gradient_ref.gradient_domain_fusion;
  * the workspace, which holds the row prefix sums on return, is bit-equal (uint32 view) to _gradient_ref.row_prefix_plane.
    The canvas hides most fp32 differences (a reversed list of 150 tiles moves one byte, and a third of the plane).

  grid130         a table of three ballot rounds, lists of at most 64 filled from all rounds (base += 64, the cnt + popc carry),
                  five row chunks and four column chunks; cn 3 (chain phase j0 != channel in every other chunk) and cn 2
  pile64/65/150   exactly 64 listed tiles (the full list), 65 and 150 (the walk of the whole table), u8 and float32
  mixed sizes     one cosine table per feather width, G.lut != 0, two sizes sharing a table, u8 and float32, cn 3 and 1
  chunk edges     rows of 255, 256, 257, 513 (cn 1), 256, 258 (cn 2), 255, 258 (cn 3), 256, 260 (cn 4) elements on canvases
                  of 1, 15, 16, 17, 63, 64 and 65 rows: the last-chunk sizes of both passes, the chain phase, one-row canvases"""
import functools

import numpy as np
import pytest

import _blend_list_cases as L
import _gradient_ref as gref
import _native
import blending_module as bm

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(tiles, positions, canvas, plane) of a case, computed once; key = (constructor name, args, f32)."""
    make, args, f32 = key
    case = getattr(L, make)(*args)
    tiles, pos = L.grad_tiles(case, f32), L.grad_positions(case)
    want = gref.gradient_domain_fusion(tiles, pos, case.shape)
    plane = gref.row_prefix_plane(tiles, pos, case.shape)
    for a in tiles + [want, plane]:
        a.setflags(write=False)
    return case, tiles, pos, want, plane


def _gpu(ctx, case, tiles, f32):
    H, W = case.shape
    cn, es = case.cn, 4 if f32 else 1
    shape = (H, W) if tiles[0].ndim == 2 else (H, W, cn)
    bufs = [ctx.upload(t) for t in tiles]
    canvas, work = ctx.alloc(H * W * cn), ctx.alloc(H * W * cn * 4)
    try:
        ctx.memset(canvas.ptr, 0xA5, H * W * cn)                     # neither plane may keep what was there
        ctx.memset(work.ptr, 0xFF, H * W * cn * 4)
        ctx.gradient_fusion(_native.SR_F32 if f32 else _native.SR_U8, [b.ptr for b in bufs], [t.shape[1] * cn * es for t in tiles],
                            [(x, y, w, h) for (y, x, h, w) in case.rects], cn, H, W, canvas.ptr, W * cn, work.ptr)
        return ctx.download(canvas.ptr, shape, np.uint8), ctx.download(work.ptr, shape, np.float32)
    finally:
        ctx.sync()
        for b in bufs + [canvas, work]:
            b.free()


def _check(ctx, make, args, f32=False):
    case, tiles, pos, want, plane = _reference((make, tuple(args), f32))
    got, work = _gpu(ctx, case, tiles, f32)
    bad = work.view(np.uint32) != plane.view(np.uint32)
    assert not bad.any(), (f"{case.name}: {int(bad.sum())} of {bad.size} row prefix sums differ, first at "
                           f"{tuple(int(v) for v in np.argwhere(bad)[0])}")
    assert np.array_equal(got, want), f"{case.name}: {int((got != want).sum())} of {got.size} canvas bytes differ"
    return case, tiles, pos, want


@pytest.mark.parametrize("cn", [3, 2])
def test_grid130_three_ballot_rounds(ctx, cn):
    _check(ctx, "grid130", (cn,))


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [64, 65, 150])
def test_pile_full_list_and_table_walk(ctx, n, f32):
    _check(ctx, "pile", (n,), f32)


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("cn", [3, 1])
def test_mixed_sizes_one_table_per_feather_width(ctx, cn, f32):
    _check(ctx, "mixed_sizes", (cn,), f32)


def test_mixed_sizes_through_the_module(ctx):
    case, tiles, pos, want, _ = _reference(("mixed_sizes", (3,), False))
    got = bm.BlendingModule().gradient_domain_fusion(list(tiles), pos, case.shape)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("shape", L.CHUNK_EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-cn{s[2]}")
def test_chunk_edges(ctx, shape):
    case, tiles, pos, want = _check(ctx, "chunk_edge", shape)
    # the two smallest against the scalar-loop form, too -- both are one-row canvases, which are all zeros (see the host test),
    # so the smallest canvas with more than one row joins them
    if shape in sorted(L.CHUNK_EDGE_SHAPES, key=lambda s: s[0] * s[1])[:3]:
        assert np.array_equal(gref.gradient_domain_fusion_loops(tiles, pos, case.shape), want)
