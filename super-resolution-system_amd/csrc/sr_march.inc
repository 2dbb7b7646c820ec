// sr_march.inc -- the column-marching form of the final gather (part of sr_engine.hip: it uses that file's FinalDesc,
// vector typedefs and load helpers).  Reference: blending_module.py:340-363 (collapse of level 1) and :474-506 (acc += R_0,
// wacc += W_0, normalise, clip, truncate) -- the same arithmetic as k_final_fused, expression for expression.
//
// Where the canvas is covered by a FIXED list of tiles and every 4 x 2 cell is an interior visit of each of them (no
// border rule anywhere in the level-2 -> level-1 -> level-0 chain), nothing has to be recomputed or staged through LDS:
// a wave owns a strip of up to 62 cells (248 pixels) and walks down it two canvas rows per step.  Per tile and plane a
// lane keeps
//   * the horizontal pyrUp sums of the last two level-2 rows at its two own level-1 columns ((G_2, R_2) pairs),
//   * the horizontal pyrUp sums of the last two level-1 rows at its four pixel columns (G_1 and R_1, pixel columns
//     paired by phase: (0, 2) and (1, 3)),
// so a step produces ONE new level-1 row of R_1 = up(R_2) + (G_1 - up(G_2)) * W_1 at the lane's two columns, fetches the two
// neighbouring columns from the adjacent lanes (lanes 0 and ncell + 1 are halo lanes: they only produce), runs ONE
// horizontal pass and the vertical pass of the step's two pixel rows, all in packed fp32.  k_final_fused recomputes a
// 12 x 72 window of R_1 per 8 x 64 used and the three horizontal passes of every cell; here every value of every level is
// formed exactly once per strip.  Results are bit-identical (same operands, same order, -ffp-contract=off).
//
// Memory goes through buffer instructions: one resource per array, a per-lane 32-bit offset that never changes, and the
// row in a scalar offset register that the scalar unit advances -- no vector instruction is spent on an address.
// (MARCH_NT, MARCH_SEG, MARCH_CELLS, the rounds per list and MarchItem: sr_blend_tables.h -- the planner cuts the lists by them)
#ifndef MARCH1_WAVES
#define MARCH1_WAVES 2                /* waves per SIMD the one-tile kernel is held to (256 registers) */
#endif
#ifndef MARCHN_WAVES
#define MARCHN_WAVES 2                /* the same for the several-tile kernel */
#endif
#ifndef MARCH_PLANE_FENCE
#define MARCH_PLANE_FENCE __builtin_amdgcn_sched_barrier(0)
#endif
typedef __amdgpu_buffer_rsrc_t march_rsrc;

__device__ __forceinline__ march_rsrc march_make_rsrc(const void *base, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f2_t march_ld2(march_rsrc r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(f2_t, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ u3_t march_ld3(march_rsrc r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(u3_t, __builtin_amdgcn_raw_buffer_load_b96(r, voff, soff, 0));
}
// G_1 at a lane's two own columns as it is stored (G1<>, sr_engine.hip): 8 bytes of fp32, or 4 bytes of 16-bit integers (at
// an odd column a request that is only 2-byte aligned, like the pixel rows' 12-byte ones)
template <int G1F>
__device__ __forceinline__ typename G1<G1F>::pair_t march_ldg1(march_rsrc r, unsigned voff, unsigned soff)
{
    if constexpr (G1F == G1_U16) return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
    else return march_ld2(r, voff, soff);
}

// the value `v` of the lane to the left / right: a whole-wave shift by one lane (DPP wave_shr:1 / wave_shl:1 -- probed on
// gfx950, tools/ubench_cvt.hip: lane i takes lane i - 1 / i + 1 across all 64 lanes; the end lane keeps `v`).  One VALU move
// with a few cycles of latency; the same fetch through the LDS crossbar (ds_bpermute_b32) costs no VALU slot but parks the
// wave for a full LDS round trip four times per plane and step -- 58 % of the waves' time in the first version.
__device__ __forceinline__ float lane_left(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_right(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

enum { MT_XO = 1, MT_YO = 2, MT_P1 = 4, MT_FXUNIT = 8, MT_W1UNIT = 16 };
#define MARCH_W1_MARGIN 6            /* pixels beyond the feather width from which the level-1 weight is exactly 1, too */

// per tile: wave-uniform part
struct MarchU {
    march_rsrc px;                   // the tile's pixels (row 0 may be virtual: only rows in use are touched)
    unsigned g1, w1;                 // arena byte offset of the level-1 row the next request takes (plane 0 / weight level)
    unsigned g2, r2;                 // arena byte offset of the level-2 row the next even level-1 row takes (plane 0)
    unsigned pxe, pxo;               // byte offset of the next step's pixel row of even / odd pyrUp phase
    unsigned p1b, p2b, px2;          // row pitches of levels 1 (W_1) and 2, two pixel rows, in bytes
    unsigned p1g;                    // row pitch of G_1 in bytes (p1b, or half of it where G_1 is stored in 16 bits)
    unsigned plane1b, plane2b;       // plane sizes of G_1 and of level 2 in bytes
    int r0;                          // level-1 row of the first step's first tap row (its parity picks the loop variant)
    int lye, lyo;                    // tile-local row of the next step's even- / odd-phase pixel row
    int h1, fw;                      // tile height - 1, feather width
    const float *lut;
    unsigned flags;                  // MT_XO: first pixel column odd; MT_YO: first pixel row odd; MT_P1: own column a odd;
                                     // MT_FXUNIT: every column weight of the wave's useful cells is exactly 1
                                     // MT_W1UNIT: every lane's columns (halo lanes included) lie MARCH_W1_MARGIN pixels deeper
};
// per tile: per-lane part that does not depend on the plane
struct MarchV {
    unsigned v1, v2, vpx;            // byte offsets: own column a of level 1 (W_1), column n0 of level 2, the cell's first pixel
    unsigned v1g;                    // own column a of G_1
    f2_t fx02, fx13;                 // column weights
};
// per tile and plane
struct MarchP {
    f2_t H2[2][2];                   // [row m, m + 1][column a, a + 1] horizontal sums of (G_2, R_2)
    f2_t HG[2][2], HR[2][2];         // [ring slot][pixel columns (0, 2) / (1, 3)] horizontal sums of G_1 / R_1
};

// horizontal pyrUp sums of one level-2 row at the own level-1 columns (up_block_interior_pk's expressions per column)
__device__ __forceinline__ void march_l2_hpass(bool p1, u3_t g, u3_t r, f2_t &na, f2_t &nb)
{
    f2_t v0, v1, v2;
    v0.x = __uint_as_float(g.x); v0.y = __uint_as_float(r.x);
    v1.x = __uint_as_float(g.y); v1.y = __uint_as_float(r.y);
    v2.x = __uint_as_float(g.z); v2.y = __uint_as_float(r.z);
    if (!p1) {                                                      // column a even: taps n0 .. n0 + 2; a + 1 odd: n0 + 1, n0 + 2
        na = (v0 + v1 * 6.0f) + v2;
        nb = v1 + v2;
    } else {                                                        // a odd: n0, n0 + 1; a + 1 even: n0 .. n0 + 2
        asm volatile("" ::: "memory");                              // keep the two forms as branches (no operand selects)
        na = v0 + v1;
        nb = (v0 + v1 * 6.0f) + v2;
    }
}

// One new level-1 row of one plane: R_1 at the own columns from the level-2 ring, the neighbours' columns, the horizontal
// pyrUp sums of the four pixel columns (up_pairs' expressions, pixel columns paired by phase): hg / hr = {(h0, h2), (h1, h3)}
// of G_1 / R_1.  g = G_1 at the own columns (a, a + 1), w = W_1 there, l2g / l2r = the new level-2 row (EVEN rows only).
template <bool EVEN, bool W1U = false>
__device__ __forceinline__ void march_l1_row(unsigned flags, MarchP &S, f2_t g, f2_t w, u3_t l2g, u3_t l2r,
                                             f2_t (&hg)[2], f2_t (&hr)[2])
{
    const bool p1 = (flags & MT_P1) != 0;
    f2_t ua, ub;
    // pyrUp scales: 1/64 where both phases are even, 1/16 where one is odd, 1/4 where both are (selected on the scalar unit)
    if (EVEN) {                                                     // even row 2m: rows m - 1, m are held, m + 1 arrives
        f2_t na, nb;
        march_l2_hpass(p1, l2g, l2r, na, nb);
        ua = ((S.H2[0][0] + S.H2[1][0] * 6.0f) + na) * (p1 ? (1.0f / 16.0f) : (1.0f / 64.0f));
        ub = ((S.H2[0][1] + S.H2[1][1] * 6.0f) + nb) * (p1 ? (1.0f / 64.0f) : (1.0f / 16.0f));
        S.H2[0][0] = S.H2[1][0];
        S.H2[0][1] = S.H2[1][1];
        S.H2[1][0] = na;
        S.H2[1][1] = nb;
    } else {                                                        // odd row 2m + 1: rows m, m + 1
        ua = (S.H2[0][0] + S.H2[1][0]) * (p1 ? (1.0f / 4.0f) : (1.0f / 16.0f));
        ub = (S.H2[0][1] + S.H2[1][1]) * (p1 ? (1.0f / 16.0f) : (1.0f / 4.0f));
    }
    // W1U: W_1 is exactly 1 at these columns and rows (x * 1 == x): neither loaded nor multiplied
    const float ra = W1U ? ua.y + (g.x - ua.x) : ua.y + (g.x - ua.x) * w.x;
    const float rb = W1U ? ub.y + (g.y - ub.x) : ub.y + (g.y - ub.x) * w.y;
    // taps 0 .. 3 of the cell: the left lane's column a + 1, the own columns, the right lane's column a
    f2_t g01, g23, r01, r12, r23;
    g01.x = lane_left(g.y); g01.y = g.x;
    g23.x = g.y; g23.y = lane_right(g.x);
    r01.x = lane_left(rb); r01.y = ra;
    r12.x = ra; r12.y = rb;
    r23.x = rb; r23.y = lane_right(ra);
    if (!(flags & MT_XO)) {
        hg[0] = (g01 + g * 6.0f) + g23;
        hg[1] = g + g23;
        hr[0] = (r01 + r12 * 6.0f) + r23;
        hr[1] = r12 + r23;
    } else {
        asm volatile("" ::: "memory");
        hg[0] = g01 + g;
        hg[1] = (g01 + g * 6.0f) + g23;
        hr[0] = r01 + r12;
        hr[1] = (r01 + r12 * 6.0f) + r23;
    }
}

// vertical pyrUp of one plane by phase: u?[0] = the pixel row of even phase (three taps), u?[1] = of odd phase (two taps; the
// odd-phase row follows the even one unless the tile-local first row is odd).  PH: the ring slot that holds the older of the
// two level-1 rows: the new row's sums replace it (the ring turns by renaming, the step loop is unrolled by two).
template <int PH>
__device__ __forceinline__ void march_vpass(unsigned flags, MarchP &S, const f2_t (&hg)[2], const f2_t (&hr)[2], f2_t (&ug)[2][2],
                                            f2_t (&ur)[2][2])
{
    f2_t (&og)[2] = S.HG[PH], (&mg)[2] = S.HG[1 - PH], (&orr)[2] = S.HR[PH], (&mr)[2] = S.HR[1 - PH];
    const bool xo = (flags & MT_XO) != 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        // pixel columns p, p + 2 are an odd pyrUp phase when (lx0 + p) is odd
        const bool podd = (p != 0) != xo;
        const float ce = podd ? (1.0f / 16.0f) : (1.0f / 64.0f);
        ug[0][p] = ((og[p] + mg[p] * 6.0f) + hg[p]) * ce;
        ur[0][p] = ((orr[p] + mr[p] * 6.0f) + hr[p]) * ce;
    }
    if (!(flags & MT_YO)) {                                         // taps r0 + 1, r0 + 2
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float co = ((p != 0) != xo) ? (1.0f / 4.0f) : (1.0f / 16.0f);
            ug[1][p] = (mg[p] + hg[p]) * co;
            ur[1][p] = (mr[p] + hr[p]) * co;
        }
    } else {                                                        // taps r0, r0 + 1
        asm volatile("" ::: "memory");
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float co = ((p != 0) != xo) ? (1.0f / 4.0f) : (1.0f / 16.0f);
            ug[1][p] = (og[p] + mg[p]) * co;
            ur[1][p] = (orr[p] + mr[p]) * co;
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        og[p] = hg[p];
        orr[p] = hr[p];
    }
}

// wave-uniform integer minimum on the scalar unit (left to itself the compiler forms the row-weight index with vector
// instructions and reads it back through v_readfirstlane)
__device__ __forceinline__ int march_smin(int a, int b)
{
    int r;
    asm("s_min_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b));
    return r;
}

// the uniform and per-lane parts of one tile for the item at (x of the lane's cell, first canvas row y0)
template <int G1F>
__device__ __forceinline__ void march_tile_uv(MarchU &U, MarchV &V, const FinalDesc &D, const float *__restrict__ luts, int x_lane,
                                              int x_px, int y0, bool useful, int pxsize)
{
    const int lx0 = x_lane - D.x, ly0 = y0 - D.y;
    const int c0 = (lx0 - 1) >> 1, r0 = (ly0 - 1) >> 1;
    const int a = c0 + 1, n0 = c0 >> 1, m0 = (r0 - 1) >> 1;
    const int yo = ly0 & 1;
    U.flags = ((__builtin_amdgcn_readfirstlane(lx0) & 1) ? MT_XO : 0) | (yo ? MT_YO : 0) |
              ((__builtin_amdgcn_readfirstlane(a) & 1) ? MT_P1 : 0);
    U.p1b = (unsigned)D.P1 * 4u;
    U.p2b = (unsigned)D.P2 * 4u;
    U.px2 = (unsigned)(2 * D.stride);
    U.p1g = (unsigned)D.P1 * G1<G1F>::ES;
    U.plane1b = (unsigned)D.H1 * U.p1g;
    U.plane2b = (unsigned)D.H2 * U.p2b;
    U.h1 = D.h - 1;
    U.fw = D.fw;
    U.lut = luts + D.lut_off;
    U.g1 = (unsigned)(D.g1 * 4) + (unsigned)r0 * U.p1g;
    U.w1 = (unsigned)(D.w1 * 4) + (unsigned)r0 * U.p1b;
    U.g2 = (unsigned)(D.g2 * 4) + (unsigned)m0 * U.p2b;
    U.r2 = (unsigned)(D.r2 * 4) + (unsigned)m0 * U.p2b;
    // the pixel row of even pyrUp phase is the first of the step's two unless the tile-local row is odd
    U.lye = ly0 + yo;
    U.lyo = ly0 + 1 - yo;
    U.px = march_make_rsrc(D.src, 0xFFFFFFFFu);
    U.pxe = (unsigned)U.lye * (unsigned)D.stride;
    U.pxo = (unsigned)U.lyo * (unsigned)D.stride;
    U.r0 = r0;
    V.v1 = (unsigned)a * 4u;
    V.v1g = (unsigned)a * G1<G1F>::ES;
    V.v2 = (unsigned)n0 * 4u;
    V.vpx = (unsigned)(x_px - D.x) * (unsigned)pxsize;
    float fx[4];
    bool one = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        fx[k] = U.lut[min(min(lx0 + k, D.w - 1 - lx0 - k), D.fw)];
        one = one && fx[k] == 1.0f;
    }
    // level 1: W_1 = pyrDown(W_0) is exactly 1 where its 5 x 5 taps of W_0 are; the columns a - 1 .. a + 2 a lane (halo lanes
    // included) forms R_1 at reach 4 pixels beyond its cell
    if (__all(min(lx0, D.w - 4 - lx0) >= D.fw + MARCH_W1_MARGIN) != 0) U.flags |= MT_W1UNIT;
    V.fx02.x = fx[0]; V.fx02.y = fx[2];
    V.fx13.x = fx[1]; V.fx13.y = fx[3];
    if (__all(one || !useful) != 0) U.flags |= MT_FXUNIT;
}

// warm-up of one plane: the level-2 ring (rows m0, m0 + 1), then level-1 rows r0 and r0 + 1 into ring slots 0 and 1.
// g1 / w1 / g2 / r2: this plane's arena offsets of rows r0 / m0 (not advanced here: the caller advances the tile's rows
// once for all planes).  Loads are waited for on the spot: once per work item.
template <int G1F>
__device__ __forceinline__ void march_plane_warmup(const MarchU &U, const MarchV &V, MarchP &S, march_rsrc arena, unsigned g1,
                                                   unsigned w1, unsigned g2, unsigned r2)
{
    const bool p1 = (U.flags & MT_P1) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
        march_l2_hpass(p1, march_ld3(arena, V.v2, g2 + i * U.p2b), march_ld3(arena, V.v2, r2 + i * U.p2b), S.H2[i][0], S.H2[i][1]);
    // r0 odd: row r0 takes no new level-2 row, row r0 + 1 does (row m0 + 2); r0 even: the other way round
    const u3_t n2g = march_ld3(arena, V.v2, g2 + 2 * U.p2b), n2r = march_ld3(arena, V.v2, r2 + 2 * U.p2b);
    const f2_t ga = G1<G1F>::pair(march_ldg1<G1F>(arena, V.v1g, g1)), gb = G1<G1F>::pair(march_ldg1<G1F>(arena, V.v1g, g1 + U.p1g));
    const f2_t wa = march_ld2(arena, V.v1, w1), wb = march_ld2(arena, V.v1, w1 + U.p1b);
    if (U.r0 & 1) {
        march_l1_row<false>(U.flags, S, ga, wa, n2g, n2r, S.HG[0], S.HR[0]);
        march_l1_row<true>(U.flags, S, gb, wb, n2g, n2r, S.HG[1], S.HR[1]);
    } else {
        march_l1_row<true>(U.flags, S, ga, wa, n2g, n2r, S.HG[0], S.HR[0]);
        march_l1_row<false>(U.flags, S, gb, wb, n2g, n2r, S.HG[1], S.HR[1]);
    }
}

// the tile's row offsets after the warm-up: level-1 rows r0, r0 + 1 and level-2 rows m0 .. m0 + 2 are consumed
__device__ __forceinline__ void march_after_warmup(MarchU &U)
{
    U.g1 += 2 * U.p1g;
    U.w1 += 2 * U.p1b;
    U.g2 += 3 * U.p2b;
    U.r2 += 3 * U.p2b;
}

// ---------------------------------------------------------------------------------------------
// One tile, all planes in one wave (u8 tiles): the pixels of a row are one 12-byte load and one 12-byte store per lane.
// ---------------------------------------------------------------------------------------------
// What a step needs from memory, requested TWO steps ahead (a step of a wave is ~1 us of issue time with two waves on a
// SIMD; a load under this traffic takes about twice that): two sets of request registers, one per step parity (the loop is
// unrolled by two), each refilled for the step after next the moment its values are consumed -- the per-plane arrays right
// after the plane's level-1 row, what all planes share (W_1, the pixel bytes) at the end of the step.  Only the set of the
// even level-1 rows carries level-2 rows, so the second set costs six registers.
template <int CN, int G1F>
struct MarchPlaneLoad {
    typename G1<G1F>::pair_t g[CN];                                 // as stored: converted where the row is formed
    u3_t l2g[CN], l2r[CN];
};
template <int CN>
struct MarchSharedLoad {
    f2_t w;
    unsigned pxw[2][CN == 3 ? 3 : 1];                               // the cell's pixel bytes, [even / odd phase row][dword]
};

template <int CN>
__device__ __forceinline__ void march_ldpx(march_rsrc px, unsigned voff, unsigned soff, unsigned (&wd)[CN == 3 ? 3 : 1])
{
    if constexpr (CN == 3) {
        const u3_t q = march_ld3(px, voff, soff);
        wd[0] = q.x; wd[1] = q.y; wd[2] = q.z;
    } else {
        wd[0] = __builtin_amdgcn_raw_buffer_load_b32(px, voff, soff, 0);
    }
}

// the shared part of the step that follows the one whose rows U points at (its rows are then U's current ones)
template <int CN, bool W1U = false>
__device__ __forceinline__ void march_request_shared(MarchU &U, const MarchV &V, march_rsrc arena, MarchSharedLoad<CN> &H)
{
    if (!W1U) H.w = march_ld2(arena, V.v1, U.w1);
    march_ldpx<CN>(U.px, V.vpx, U.pxe, H.pxw[0]);
    march_ldpx<CN>(U.px, V.vpx, U.pxo, H.pxw[1]);
    if (!W1U) U.w1 += U.p1b;
    U.pxe += U.px2;
    U.pxo += U.px2;
}

// the per-plane part of the first step
template <int CN, bool EVEN, int G1F>
__device__ __forceinline__ void march_request_planes(MarchU &U, const MarchV &V, march_rsrc arena, MarchPlaneLoad<CN, G1F> &L)
{
#pragma unroll
    for (int c = 0; c < CN; ++c) L.g[c] = march_ldg1<G1F>(arena, V.v1g, U.g1 + c * U.plane1b);
    if (EVEN) {
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            L.l2g[c] = march_ld3(arena, V.v2, U.g2 + c * U.plane2b);
            L.l2r[c] = march_ld3(arena, V.v2, U.r2 + c * U.plane2b);
        }
        U.g2 += U.p2b;
        U.r2 += U.p2b;
    }
    U.g1 += U.p1g;
}

// one byte of an output row into its dword: clip, then truncate (blending_module.py:501-506).  v_cvt_pk_u8_f32 saturates to
// [0, 255] and rounds to nearest even (probed: tools/ubench_cvt.hip), so on floor(v) it is exactly clip-then-truncate.
__device__ __forceinline__ unsigned march_put_u8(float v, int byte, unsigned word)
{
    return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(v), byte, word);
}

// the weights of a step, [phase][pair], and whether any weight sum of the wave's useful cells differs from 1
__device__ __forceinline__ void march_weights(MarchU &U, const MarchV &V, f2_t (&w0)[2][2])
{
    float fy[2];
    fy[0] = U.lut[march_smin(march_smin(U.lye, U.h1 - U.lye), U.fw)];          // wave-uniform
    fy[1] = U.lut[march_smin(march_smin(U.lyo, U.h1 - U.lyo), U.fw)];
    U.lye += 2;
    U.lyo += 2;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        w0[q][0].x = __builtin_fminf(fy[q], V.fx02.x); w0[q][0].y = __builtin_fminf(fy[q], V.fx02.y);
        w0[q][1].x = __builtin_fminf(fy[q], V.fx13.x); w0[q][1].y = __builtin_fminf(fy[q], V.fx13.y);
    }
}

// 1 / max(w, 1e-6) for div_shared's IEEE-correct fma chain, two pixels per packed instruction
__device__ __forceinline__ f2_t march_recip(f2_t wsum, f2_t &wc)
{
    asm volatile("" ::: "memory");
    f2_t r, one2;
    wc.x = __builtin_fmaxf(wsum.x, 1e-6f); wc.y = __builtin_fmaxf(wsum.y, 1e-6f);
    r.x = __builtin_amdgcn_rcpf(wc.x); r.y = __builtin_amdgcn_rcpf(wc.y);
    one2.x = one2.y = 1.0f;
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-wc, r, one2), r, r);
}
__device__ __forceinline__ f2_t march_div(f2_t a, f2_t wc, f2_t rr)
{
    asm volatile("" ::: "memory");                                  // stays behind its (wave-uniform) branch: never speculated into selects
    f2_t t = a * rr;
    t = __builtin_elementwise_fma(__builtin_elementwise_fma(-wc, t, a), rr, t);
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-wc, t, a), rr, t);
}

// the pixels of columns p and p + 2 of plane c in a row's dwords
template <int CN>
__device__ __forceinline__ f2_t march_px_pair(const unsigned (&wd)[CN == 3 ? 3 : 1], int p, int c)
{
    const int b0 = CN * p + c, b1 = CN * (p + 2) + c;
    f2_t px;
    px.x = (float)((wd[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu);
    px.y = (float)((wd[b1 >> 2] >> (8 * (b1 & 3))) & 0xFFu);
    return px;
}

// ---------------------------------------------------------------------------------------------
// One tile, all planes in one wave (u8 tiles): the pixels of a row are one 12-byte load and one 12-byte store per lane.
// ---------------------------------------------------------------------------------------------
// One step.  o_e / o_o: canvas byte offsets of the even- / odd-phase row.
// UNIT: every weight the item touches is exactly 1 (beyond the feather width of a linear / cosine ramp), so lap * w == lap
// and the weight sum is 1: multiplies, weights and the division are left out (bit-identical: x * 1 == x, x / 1 == x).
// L / H hold this step's data on entry and, when `more`, the data of the step after next (same parity) on return.
template <int CN, int PH, bool EVEN, bool UNIT, int FL, bool W1U, int G1F>
__device__ __forceinline__ void march1_step(MarchU &U, const MarchV &V, MarchP (&S)[CN], MarchPlaneLoad<CN, G1F> &L,
                                            MarchSharedLoad<CN> &H, march_rsrc arena, bool more, bool useful, march_rsrc out,
                                            unsigned vout, unsigned o_e, unsigned o_o, march_rsrc outf, bool with_f, unsigned f_e,
                                            unsigned f_o)
{
    const unsigned flags = FL >= 0 ? (unsigned)FL : U.flags;          // the phases as constants where the caller knows them
    f2_t zero;
    zero.x = zero.y = 0.f;
    f2_t w0[2][2], wc[2][2], rr[2][2];                              // [phase][pair]: weights, clamped sums, their reciprocals
    bool dodiv = false;
    if (!UNIT) {
        march_weights(U, V, w0);
        bool ones = true;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int p = 0; p < 2; ++p) ones = ones && w0[q][p].x == 1.0f && w0[q][p].y == 1.0f;
        dodiv = __all(ones || !useful) == 0;                        // x / 1 == x: skipped where every weight sum of the wave is 1
        if (dodiv) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int p = 0; p < 2; ++p) rr[q][p] = march_recip(zero + w0[q][p], wc[q][p]);        // wacc = 0; wacc += W_0
        }
    }
    unsigned wd[2][CN == 3 ? 3 : 1];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < (CN == 3 ? 3 : 1); ++i) wd[q][i] = 0u;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        f2_t hg[2], hr[2], ug[2][2], ur[2][2];
        march_l1_row<EVEN, W1U>(flags, S[c], G1<G1F>::pair(L.g[c]), H.w, L.l2g[c], L.l2r[c], hg, hr);
        if (more) {                                                 // this plane's rows of the step after next
            L.g[c] = march_ldg1<G1F>(arena, V.v1g, U.g1 + c * U.plane1b);
            if (EVEN) {
                L.l2g[c] = march_ld3(arena, V.v2, U.g2 + c * U.plane2b);
                L.l2r[c] = march_ld3(arena, V.v2, U.r2 + c * U.plane2b);
            }
        }
        march_vpass<PH>(flags, S[c], hg, hr, ug, ur);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const f2_t lap = march_px_pair<CN>(H.pxw[q], p, c) - ug[q][p];
                f2_t a;
                if (UNIT) a = zero + (ur[q][p] + lap);                      // acc = 0; acc += R_0
                else a = zero + (ur[q][p] + lap * w0[q][p]);
                if (!UNIT && dodiv) a = march_div(a, wc[q][p], rr[q][p]);
                const int b0 = CN * p + c, b1 = CN * (p + 2) + c;
                if (with_f && useful) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a.x), outf, vout * 4u + b0 * 4, q ? f_o : f_e, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a.y), outf, vout * 4u + b1 * 4, q ? f_o : f_e, 0);
                }
                wd[q][b0 >> 2] = march_put_u8(a.x, b0 & 3, wd[q][b0 >> 2]);
                wd[q][b1 >> 2] = march_put_u8(a.y, b1 & 3, wd[q][b1 >> 2]);
            }
        MARCH_PLANE_FENCE;                                          // plane by plane: the next plane's work is not pulled up
    }
    if (more) {
        U.g1 += U.p1g;
        if (EVEN) {
            U.g2 += U.p2b;
            U.r2 += U.p2b;
        }
        march_request_shared<CN, W1U>(U, V, arena, H);
    }
    if (useful) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if constexpr (CN == 3) {
                u3_t o;
                o.x = wd[q][0]; o.y = wd[q][1]; o.z = wd[q][2];
                __builtin_amdgcn_raw_buffer_store_b96(o, out, vout, q ? o_o : o_e, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(wd[q][0], out, vout, q ? o_o : o_e, 0);
            }
        }
    }
}

// The step loop of one work item, two steps per iteration: ring slots, the two shared request sets and row parities are
// static.  E0: the FIRST step's new level-1 row is even (the second step's is then odd, and so on).  FL >= 0: the tile's
// phase flags (MT_XO | MT_YO | MT_P1) as a constant -- the unit-weight loop, which runs over two thirds of a grid's canvas,
// exists once per phase combination: straight-line code, no scalar tests and branches (at two waves per SIMD a wave's own
// instruction stream, scalar instructions included, is what bounds a step).
template <int CN, bool E0, bool UNIT, int FL, bool W1U, int G1F>
__device__ __forceinline__ void march1_loop(MarchU &U, const MarchV &V, MarchP (&S)[CN], march_rsrc arena, int nstep,
                                            bool useful, march_rsrc out, unsigned vout, unsigned cstride, march_rsrc outf,
                                            bool with_f, unsigned fstride)
{
    MarchPlaneLoad<CN, G1F> LA, LB;
    MarchSharedLoad<CN> HA, HB;
    const bool yo = (U.flags & MT_YO) != 0;
    unsigned o_e = yo ? cstride : 0u, o_o = yo ? 0u : cstride, f_e = yo ? fstride : 0u, f_o = yo ? 0u : fstride;
    march_request_planes<CN, E0, G1F>(U, V, arena, LA);
    march_request_shared<CN, W1U>(U, V, arena, HA);
    march_request_planes<CN, !E0, G1F>(U, V, arena, LB);
    march_request_shared<CN, W1U>(U, V, arena, HB);
#pragma unroll 1
    for (int s = 0; s < nstep; s += 2) {
        const bool more = s + 2 < nstep;
        march1_step<CN, 0, E0, UNIT, FL, W1U, G1F>(U, V, S, LA, HA, arena, more, useful, out, vout, o_e, o_o, outf, with_f, f_e, f_o);
        o_e += 2 * cstride; o_o += 2 * cstride; f_e += 2 * fstride; f_o += 2 * fstride;
        march1_step<CN, 1, !E0, UNIT, FL, W1U, G1F>(U, V, S, LB, HB, arena, more, useful, out, vout, o_e, o_o, outf, with_f, f_e, f_o);
        o_e += 2 * cstride; o_o += 2 * cstride; f_e += 2 * fstride; f_o += 2 * fstride;
    }
}

// The work item's common start: lanes, the tile's uniform and per-lane parts, the warm-up of every plane.
struct MarchLanes {
    int x_lane, x_px;
    bool useful;
};
__device__ __forceinline__ MarchLanes march_lanes(const MarchItem &it, int lane)
{
    MarchLanes m;
    const int ncell = it.ncell;
    // lanes beyond the right halo lane repeat it, pixel addresses of the halo lanes repeat their useful neighbour's
    const int lane_c = min(lane, ncell + 1), lane_p = min(max(lane, 1), ncell);
    m.useful = lane >= 1 && lane <= ncell;
    m.x_lane = it.x0 + 4 * lane_c;
    m.x_px = it.x0 + 4 * lane_p;
    return m;
}

// arena_bytes < 4 GB and the rows of one item < 4 GB of canvas: checked on the host when the plan is made
template <int CN, int G1F>
__global__ __launch_bounds__(64, MARCH1_WAVES) void k_final_march1(const MarchItem *__restrict__ items, const FinalDesc *__restrict__ descs,
                                                      const float *__restrict__ arena_p, unsigned arena_bytes,
                                                      const float *__restrict__ luts, unsigned char *__restrict__ canvas,
                                                      long long cstride, float *__restrict__ canvas_f32, int cw)
{
    const MarchItem &it = items[blockIdx.x];
    const int nstep = it.nstep;
    const MarchLanes M = march_lanes(it, (int)threadIdx.x);
    const FinalDesc &D = descs[it.tile[0]];
    const march_rsrc arena = march_make_rsrc(arena_p, arena_bytes);
    MarchU U;
    MarchV V;
    MarchP S[CN];
    march_tile_uv<G1F>(U, V, D, luts, M.x_lane, M.x_px, it.y0, M.useful, CN);
#pragma unroll
    for (int c = 0; c < CN; ++c)
        march_plane_warmup<G1F>(U, V, S[c], arena, U.g1 + c * U.plane1b, U.w1, U.g2 + c * U.plane2b, U.r2 + c * U.plane2b);
    march_after_warmup(U);
    // every row weight of the item is lut[fw] == 1 (the column weights: MT_FXUNIT)
    const int ly0 = it.y0 - D.y;
    const bool unit = (U.flags & MT_FXUNIT) && min(ly0, D.h - 2 * nstep - ly0) >= D.fw && U.lut[D.fw] == 1.0f;
    const march_rsrc out = march_make_rsrc(canvas + (long long)it.y0 * cstride, 0xFFFFFFFFu);
    const bool with_f = canvas_f32 != nullptr;
    const unsigned fstride = (unsigned)cw * CN * 4u;
    const march_rsrc outf = march_make_rsrc(with_f ? (const void *)((const char *)canvas_f32 + (long long)it.y0 * fstride) : (const void *)canvas,
                                            with_f ? 0xFFFFFFFFu : 0u);
    const unsigned vout = (unsigned)M.x_px * CN;
    const bool e0 = !(U.r0 & 1);                                    // the first step produces level-1 row r0 + 2
#define MARCH_GO(EV, UV, FLV, WV) march1_loop<CN, EV, UV, FLV, WV, G1F>(U, V, S, arena, nstep, M.useful, out, vout, (unsigned)cstride, outf, with_f, fstride)
#define MARCH_GO_FL(FLV) do { if (e0) MARCH_GO(true, true, FLV, true); else MARCH_GO(false, true, FLV, true); } while (0)
    // ... and W_1 is 1 as well MARCH_W1_MARGIN pixels further in (all of a grid's single coverage but the strips that touch the
    // feather ramps): the phase-specialised loops leave W_1 out; unit items closer to the ramps take the general loop
    const bool unit1 = unit && (U.flags & MT_W1UNIT) && min(ly0, D.h - 2 * nstep - ly0) >= D.fw + MARCH_W1_MARGIN;
    if (unit1) {
        switch (U.flags & (MT_XO | MT_YO | MT_P1)) {
        case 0: MARCH_GO_FL(0); break;
        case 1: MARCH_GO_FL(1); break;
        case 2: MARCH_GO_FL(2); break;
        case 3: MARCH_GO_FL(3); break;
        case 4: MARCH_GO_FL(4); break;
        case 5: MARCH_GO_FL(5); break;
        case 6: MARCH_GO_FL(6); break;
        default: MARCH_GO_FL(7); break;
        }
    } else {                                                        // (unit items closer to the ramps: weights of 1 multiply exactly)
        if (e0) MARCH_GO(true, false, -1, false); else MARCH_GO(false, false, -1, false);
    }
#undef MARCH_GO_FL
#undef MARCH_GO
}

// ---------------------------------------------------------------------------------------------
// Several tiles (the overlap zones): a workgroup of NT waves per strip, wave t = tile t with all planes.  Every wave
// forms its tile's contribution to both canvas rows of a step and leaves it in LDS, [tile][canvas row]; after one
// barrier wave 0 finishes canvas row 0 and wave 1 canvas row 1, each summing the tiles in list order -- acc = 0;
// acc += tile 0's; acc += tile 1's; ... exactly as the reference accumulates -- then normalising, clipping, storing.
// Which of a tile's two rows (even / odd pyrUp phase) is which canvas row only changes the LDS ADDRESS a vector is written
// to, so no variant of the code depends on it.  The exchange slots alternate: a wave may write step s + 1 while the
// finishers still read step s; one barrier per step.
// ---------------------------------------------------------------------------------------------
template <int CN, int NT>
struct MarchX {
    static constexpr int VEC = CN + 1;                              // vectors of 4 floats a lane leaves per canvas row: planes + weights
    static constexpr int ROW = VEC * 256;                           // floats of one (tile, canvas row): [vector][pair][lane][2]
    static constexpr int SLOT = NT * 2 * ROW;                       // floats of one exchange slot: [tile][canvas row]
};

// one step of one wave: xw = this tile's [canvas row 0] vector 0 of the step's slot for this lane, xr = tile 0's [this
// wave's canvas row] (finishers only)
template <int CN, int NT, int PH, bool EVEN, int FL, int G1F>
__device__ __forceinline__ void marchn_step(MarchU &U, const MarchV &V, MarchP (&S)[CN], MarchPlaneLoad<CN, G1F> &L,
                                            MarchSharedLoad<CN> &H, march_rsrc arena, bool more, bool useful, bool finisher,
                                            float *xw, const float *xr,
                                            march_rsrc out, unsigned vout, unsigned o_fin, march_rsrc outf, bool with_f,
                                            unsigned f_fin)
{
    typedef MarchX<CN, NT> X;
    const unsigned flags = (unsigned)FL;                            // the tile's phases as constants: one loop per combination
    f2_t w0[2][2];
    march_weights(U, V, w0);
    // the tile row of even phase is canvas row 0 unless the tile-local first row is odd
    const int row_e = (flags & MT_YO) ? X::ROW : 0, row_o = X::ROW - row_e;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        f2_t hg[2], hr[2], ug[2][2], ur[2][2];
        march_l1_row<EVEN>(flags, S[c], G1<G1F>::pair(L.g[c]), H.w, L.l2g[c], L.l2r[c], hg, hr);
        if (more) {                                                 // this plane's rows of the step after next
            L.g[c] = march_ldg1<G1F>(arena, V.v1g, U.g1 + c * U.plane1b);
            if (EVEN) {
                L.l2g[c] = march_ld3(arena, V.v2, U.g2 + c * U.plane2b);
                L.l2r[c] = march_ld3(arena, V.v2, U.r2 + c * U.plane2b);
            }
        }
        march_vpass<PH>(flags, S[c], hg, hr, ug, ur);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const f2_t a = ur[q][p] + (march_px_pair<CN>(H.pxw[q], p, c) - ug[q][p]) * w0[q][p];
                // [vector][pair][lane][2]: the register pair as it stands (8-byte store), lanes contiguous
                *(f2_t *)(xw + (q ? row_o : row_e) + c * 256 + p * 128) = a;
            }
        }
        MARCH_PLANE_FENCE;                                          // plane by plane: the next plane's work is not pulled up
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int p = 0; p < 2; ++p) *(f2_t *)(xw + (q ? row_o : row_e) + CN * 256 + p * 128) = w0[q][p];
    if (more) {
        U.g1 += U.p1g;
        if (EVEN) {
            U.g2 += U.p2b;
            U.r2 += U.p2b;
        }
        march_request_shared<CN>(U, V, arena, H);
    }
    // the exchange slot is written: LDS only (the step's requests stay in flight across the barrier)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (!finisher) return;
    f2_t zero;
    zero.x = zero.y = 0.f;
    f2_t wsum[2];
    wsum[0] = wsum[1] = zero;
#pragma unroll
    for (int t = 0; t < NT; ++t) {                                  // wacc = 0; wacc += W_0 of every tile, list order
        wsum[0] += *(const f2_t *)(xr + t * 2 * X::ROW + CN * 256);
        wsum[1] += *(const f2_t *)(xr + t * 2 * X::ROW + CN * 256 + 128);
    }
    const bool ones = wsum[0].x == 1.0f && wsum[0].y == 1.0f && wsum[1].x == 1.0f && wsum[1].y == 1.0f;
    const bool dodiv = __all(ones || !useful) == 0;
    f2_t wc[2], rr[2];
    if (dodiv) {
#pragma unroll
        for (int p = 0; p < 2; ++p) rr[p] = march_recip(wsum[p], wc[p]);
    }
    unsigned wd[CN == 3 ? 3 : 1];
#pragma unroll
    for (int i = 0; i < (CN == 3 ? 3 : 1); ++i) wd[i] = 0u;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        f2_t a[2];
        a[0] = a[1] = zero;
#pragma unroll
        for (int t = 0; t < NT; ++t) {                              // acc = 0; acc += R_0 of every tile, list order
            a[0] += *(const f2_t *)(xr + t * 2 * X::ROW + c * 256);
            a[1] += *(const f2_t *)(xr + t * 2 * X::ROW + c * 256 + 128);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (dodiv) a[p] = march_div(a[p], wc[p], rr[p]);
            const int b0 = CN * p + c, b1 = CN * (p + 2) + c;
            if (with_f && useful) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a[p].x), outf, vout * 4u + b0 * 4, f_fin, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a[p].y), outf, vout * 4u + b1 * 4, f_fin, 0);
            }
            wd[b0 >> 2] = march_put_u8(a[p].x, b0 & 3, wd[b0 >> 2]);
            wd[b1 >> 2] = march_put_u8(a[p].y, b1 & 3, wd[b1 >> 2]);
        }
    }
    if (useful) {
        if constexpr (CN == 3) {
            u3_t o;
            o.x = wd[0]; o.y = wd[1]; o.z = wd[2];
            __builtin_amdgcn_raw_buffer_store_b96(o, out, vout, o_fin, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(wd[0], out, vout, o_fin, 0);
        }
    }
}

template <int CN, int NT, bool E0, int FL, int G1F>
__device__ __forceinline__ void marchn_loop(MarchU &U, const MarchV &V, MarchP (&S)[CN], march_rsrc arena, int nstep,
                                            bool useful, bool finisher, float *xw, const float *xr, march_rsrc out, unsigned vout,
                                            unsigned o_fin, unsigned cstride, march_rsrc outf, bool with_f,
                                            unsigned f_fin, unsigned fstride)
{
    typedef MarchX<CN, NT> X;
    MarchPlaneLoad<CN, G1F> LA, LB;
    MarchSharedLoad<CN> HA, HB;
    march_request_planes<CN, E0, G1F>(U, V, arena, LA);
    march_request_shared<CN>(U, V, arena, HA);
    march_request_planes<CN, !E0, G1F>(U, V, arena, LB);
    march_request_shared<CN>(U, V, arena, HB);
#pragma unroll 1
    for (int s = 0; s < nstep; s += 2) {
        const bool more = s + 2 < nstep;
        marchn_step<CN, NT, 0, E0, FL, G1F>(U, V, S, LA, HA, arena, more, useful, finisher, xw, xr, out, vout, o_fin, outf, with_f, f_fin);
        o_fin += 2 * cstride; f_fin += 2 * fstride;
        marchn_step<CN, NT, 1, !E0, FL, G1F>(U, V, S, LB, HB, arena, more, useful, finisher, xw + X::SLOT, xr + X::SLOT, out, vout, o_fin, outf, with_f, f_fin);
        o_fin += 2 * cstride; f_fin += 2 * fstride;
    }
}

template <int CN, int NT, int G1F>
__global__ __launch_bounds__(64 * NT, MARCHN_WAVES) void k_final_marchn(const MarchItem *__restrict__ items, const FinalDesc *__restrict__ descs,
                                                       const float *__restrict__ arena_p, unsigned arena_bytes,
                                                       const float *__restrict__ luts, unsigned char *__restrict__ canvas,
                                                       long long cstride, float *__restrict__ canvas_f32, int cw)
{
    typedef MarchX<CN, NT> X;
    __shared__ __attribute__((aligned(16))) float xch[2 * X::SLOT];
    const MarchItem &it = items[blockIdx.x];
    const int nstep = it.nstep;
    const int lane = (int)threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const MarchLanes M = march_lanes(it, lane);
    const FinalDesc &D = descs[it.tile[wv]];
    const march_rsrc arena = march_make_rsrc(arena_p, arena_bytes);
    MarchU U;
    MarchV V;
    MarchP S[CN];
    march_tile_uv<G1F>(U, V, D, luts, M.x_lane, M.x_px, it.y0, M.useful, CN);
#pragma unroll
    for (int c = 0; c < CN; ++c)
        march_plane_warmup<G1F>(U, V, S[c], arena, U.g1 + c * U.plane1b, U.w1, U.g2 + c * U.plane2b, U.r2 + c * U.plane2b);
    march_after_warmup(U);
    const unsigned fstride = (unsigned)cw * CN * 4u;
    const bool with_f = canvas_f32 != nullptr;
    const march_rsrc out = march_make_rsrc(canvas + (long long)it.y0 * cstride, 0xFFFFFFFFu);
    const march_rsrc outf = march_make_rsrc(with_f ? (const void *)((const char *)canvas_f32 + (long long)it.y0 * fstride) : (const void *)canvas,
                                            with_f ? 0xFFFFFFFFu : 0u);
    const unsigned vout = (unsigned)M.x_px * CN;
    const bool finisher = wv < 2;                                   // wave 0: canvas row 0, wave 1: canvas row 1
    float *xw = &xch[wv * 2 * X::ROW + lane * 2];
    const float *xr = &xch[(wv & 1) * X::ROW + lane * 2];
    const unsigned o_fin = (wv & 1) ? (unsigned)cstride : 0u, f_fin = (wv & 1) ? fstride : 0u;
    const bool e0 = !(U.r0 & 1);
#define MARCHN_GO(EV, FLV) marchn_loop<CN, NT, EV, FLV, G1F>(U, V, S, arena, nstep, M.useful, finisher, xw, xr, out, vout, o_fin, (unsigned)cstride, outf, with_f, f_fin, fstride)
#define MARCHN_GO_FL(FLV) do { if (e0) MARCHN_GO(true, FLV); else MARCHN_GO(false, FLV); } while (0)
    switch (U.flags & (MT_XO | MT_YO | MT_P1)) {                    // straight-line loops: one per phase combination of this wave's tile
    case 0: MARCHN_GO_FL(0); break;
    case 1: MARCHN_GO_FL(1); break;
    case 2: MARCHN_GO_FL(2); break;
    case 3: MARCHN_GO_FL(3); break;
    case 4: MARCHN_GO_FL(4); break;
    case 5: MARCHN_GO_FL(5); break;
    case 6: MARCHN_GO_FL(6); break;
    default: MARCHN_GO_FL(7); break;
    }
#undef MARCHN_GO_FL
#undef MARCHN_GO
}
