// sr_down2.inc -- levels 0 -> 1 -> 2 of the Gaussian pyramid of u8 RGB tiles in ONE column march (included by
// sr_engine.hip after sr_march.inc, whose buffer-resource and lane-shift helpers it uses).
// Reference: blending_module.py:217-262 (build_gaussian_pyramid: cv2.pyrDown twice), restated in oracle/sr_oracle.c.
//
// Why one kernel: G_2 was made by a second launch that read all of G_1 back (0.92 GB of the 200 MP workload, 0.27 ms).
// Here the wave that forms a row of G_1 keeps what G_2 needs of it in registers.
//
// Exactness.  Level-0 samples are integers 0..255, pyrDown's taps are 1 4 6 4 1 and its scale is 1/256, so
//   256 G_1  is an integer below 2^16   (row sums <= 16 * 255, column sums of those <= 16 * 4080 = 65280), and
//   65536 G_2 is an integer below 2^24.
// Every intermediate value is exactly representable where it is held (u16 lanes for level 1, fp32 for level 2), so the
// order of the additions is free: the results are the bits of the reference's fp32 evaluation (-> the full-size and fuzz
// comparisons with the oracle).  That is what allows the level-1 arithmetic in PACKED 16-bit integers: two samples per
// v_pk_add_u16 / v_pk_mad_u16, bytes brought into 16-bit lanes by v_perm_b32 -- 4.7 instructions per value and row
// instead of the 7.5 of the fp32 form (byte -> float conversions, unpacked adds).
//
// Layout of the work.  A lane owns column group g: level-1 columns 4 g .. 4 g + 3 (level-0 columns 8 g - 2 .. 8 g + 8)
// and level-2 columns 2 g, 2 g + 1.  Lane i of a wave is group D2_OUT s + i - 1 of strip s: lanes 1 .. D2_OUT store (their first
// group is a multiple of 8, so a wave's row of G_1 and of G_2 is made of whole 128-byte lines: the pitches are multiples of 32
// floats), lane 0 and lane D2_OUT + 1 only lend their level-1 values to their neighbours' level-2 sums, lane D2_OUT + 2 only
// its bytes; the lanes beyond idle (measured: 48 stored groups of 64 lanes 0.50 ms, 56: 0.54, 61 unaligned: 0.55).  A lane
// loads its own 24 bytes of a level-0 row (two dword-aligned 12-byte loads) and takes the 9 more its window needs from the
// lane to its right (three DPP moves), so a row costs 24 bytes per lane instead of the 36 of k_down_march.
// The march walks level-1 rows r = rs .. re of a segment of `seg2` level-2 rows; per row two level-0 rows arrive (requested
// D2_AHEAD row pairs ahead into further register sets), the five horizontal sums a level-1 row needs turn through a register ring.
// Level 2: horizontal sums h(r) of the level-1 row just formed (neighbours by DPP), then per column three accumulators:
//   even r = 2Y:  A += h -> G_2[Y - 1] done;  B += 6 h;  C = h        odd r = 2Y + 1:  B += 4 h;  C += 4 h;  A = B; B = C
// REFLECT_101 at the top (rows -1, -2 are rows 1, 2: their weights double) and at the bottom (formulas below) keeps the
// whole tile in the march.  A strip's cut tile marches the rows of its windows (TileDev g0 / g1 of levels 0, 1, 2: the
// planner's level-1 window covers what the level-2 window reads); gray and float tiles and tiles of fewer than three
// levels keep the two-launch form (down2_takes).
//
// G1F = G1_U16 (sr_engine.hip: the plan and the call decide): level 1 is stored as the 16-bit integers 256 G_1 the march holds
// anyway -- half the bytes of its largest store and of the gather's largest read; G_2 is formed from the fp32 values as before.
//
// Left to the per-pixel border rule: level-1 columns outside groups 1 .. ncg (trailing blocks of this launch, as in
// k_down_march) and level-2 columns outside 4 .. 2 ncg - 1 (k_down2_cols, a second small launch: it reads G_1).

typedef unsigned short d2_us2 __attribute__((ext_vector_type(2)));

#ifndef D2_AHEAD
#define D2_AHEAD 1                   /* level-1 row PAIRS a row's level-0 bytes are requested ahead */
#endif
#ifndef D2_ST_AUX
#define D2_ST_AUX 0                  /* cache-policy bits of the level-1 / level-2 stores */
#endif
#ifndef D2_WAVES
#define D2_WAVES 4                   /* waves per SIMD the march is compiled for */
#endif

// (D2_OUT and the rules the host evaluates, too -- down2_takes, down2_stride_fits, down2_nstrip, down2_cols_count: sr_blend_tables.h)

// the value of the lane to the right / left (DPP wave_shl:1 / wave_shr:1 as in sr_march.inc, but with bound_ctrl: the end
// lane reads 0 and no copy of the old value is needed -- the end lanes' results are never used here)
__device__ __forceinline__ unsigned d2_from_right(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ float d2_right(float v) { return __uint_as_float(d2_from_right(__float_as_uint(v))); }
__device__ __forceinline__ float d2_left(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
// 4 and 6 in both 16-bit lanes, opaque to the compiler: `x * 4 + y` stays one v_pk_mad_u16 (a visible 4 becomes shift + add)
__device__ __forceinline__ d2_us2 d2_k(unsigned v)
{
    unsigned k;
    asm("s_mov_b32 %0, %1" : "=s"(k) : "n"(v));
    return __builtin_bit_cast(d2_us2, k);
}

// what one level-0 row leaves: horizontal sums of the lane's four level-1 columns, (R, G) of column k in rg[k], B of
// columns (0, 1) and (2, 3) in b[0], b[1] -- all 16-bit lanes
struct D2Row {
    d2_us2 rg[4], b[2];
};

// the lane's own six dwords of a row (aligned: they start m bytes before the window) and that m (wave-uniform)
struct D2Raw {
    u3_t lo, hi;
    unsigned m;
};

// the level-0 row a level-1 row's tap falls on: REFLECT_101 at the tile's ends, then kept inside the rows the tile holds
// (z0 .. z1 - 1: a strip's cut tile is a window of rows with a virtual row 0; only a row of the march that is neither
// stored nor summed into a stored level-2 value can fall outside, by one level-1 row)
__device__ __forceinline__ int d2_row(int p, int hs, int z0, int z1) { return min(max(reflect101_once(p, hs), z0), z1 - 1); }

__device__ __forceinline__ void d2_request(march_rsrc px, unsigned plo, unsigned stride, int row, unsigned voff_lo, unsigned voff_hi,
                                           D2Raw &R)
{
    // window of group g: bytes [p, p + 33), p = base + row * stride + 24 g - 6; every lane of the wave has p & 3 in common
    const unsigned off = (unsigned)row * stride;
    R.m = (plo + off - 6u) & 3u;
    const unsigned soff = off + 6u - R.m;                           // the resource's base is the tile's first byte - 12
    R.lo = march_ld3(px, voff_lo, soff);
    R.hi = march_ld3(px, voff_hi, soff);
}

__device__ __forceinline__ void d2_hpass(const D2Raw &R, D2Row &H)
{
    unsigned d[10], w[9];
    d[0] = R.lo.x; d[1] = R.lo.y; d[2] = R.lo.z; d[3] = R.hi.x; d[4] = R.hi.y; d[5] = R.hi.z;
    d[6] = d2_from_right(R.lo.x); d[7] = d2_from_right(R.lo.y); d[8] = d2_from_right(R.lo.z);
    d[9] = 0u;
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], R.m);
    // pixel i (0 .. 10) of the window, channel c, is byte 3 i + c
    d2_us2 a[11], c[9];
#pragma unroll
    for (int i = 0; i < 11; ++i) {                                  // (R, G) of pixel i
        const int j = (3 * i) >> 2, o = (3 * i) & 3;
        const unsigned sel = 0x0c000c00u | ((unsigned)(o + 1) << 16) | (unsigned)o;
        a[i] = __builtin_bit_cast(d2_us2, __builtin_amdgcn_perm(w[j + 1 < 9 ? j + 1 : 8], w[j], sel));
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {                                   // B of pixels t and t + 2
        const int b0 = 3 * t + 2, b1 = 3 * t + 8;
        const int j0 = b0 >> 2, o0 = b0 & 3, j1 = b1 >> 2, o1 = b1 & 3;
        const unsigned sel = 0x0c000c00u | ((unsigned)(4 + o1) << 16) | (unsigned)o0;
        c[t] = __builtin_bit_cast(d2_us2, __builtin_amdgcn_perm(w[j1], w[j0], sel));
    }
    const d2_us2 k4 = d2_k(0x00040004u), k6 = d2_k(0x00060006u);
#pragma unroll
    for (int k = 0; k < 4; ++k) H.rg[k] = a[2 * k + 2] * k6 + ((a[2 * k + 1] + a[2 * k + 3]) * k4 + (a[2 * k] + a[2 * k + 4]));
#pragma unroll
    for (int n = 0; n < 2; ++n) H.b[n] = c[4 * n + 2] * k6 + ((c[4 * n + 1] + c[4 * n + 3]) * k4 + (c[4 * n] + c[4 * n + 4]));
}

// 256 G_1 of one row from the five row sums around it, as fp32 G_1 per plane: f[plane][0] = columns (0, 1), [1] = (2, 3), and
// the integers themselves per plane as they are stored under G1_U16: q[plane][0] = columns (0, 1) in one dword, [1] = (2, 3)
__device__ __forceinline__ void d2_vpass(const D2Row &e0, const D2Row &o0, const D2Row &e1, const D2Row &o1, const D2Row &e2,
                                         f2_t (&f)[3][2], unsigned (&q)[3][2])
{
    const d2_us2 k4 = d2_k(0x00040004u), k6 = d2_k(0x00060006u);
    f2_t sc;
    sc.x = sc.y = 1.0f / 256.0f;
    float t[3][4];
    unsigned rg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const d2_us2 v = e1.rg[k] * k6 + ((o0.rg[k] + o1.rg[k]) * k4 + (e0.rg[k] + e2.rg[k]));
        t[0][k] = (float)v.x;
        t[1][k] = (float)v.y;
        rg[k] = __builtin_bit_cast(unsigned, v);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {                                   // (R, G) per column -> two columns per plane
        q[0][n] = __builtin_amdgcn_perm(rg[2 * n + 1], rg[2 * n], 0x05040100u);
        q[1][n] = __builtin_amdgcn_perm(rg[2 * n + 1], rg[2 * n], 0x07060302u);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const d2_us2 v = e1.b[n] * k6 + ((o0.b[n] + o1.b[n]) * k4 + (e0.b[n] + e2.b[n]));
        t[2][2 * n] = (float)v.x;
        t[2][2 * n + 1] = (float)v.y;
        q[2][n] = __builtin_bit_cast(unsigned, v);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            f2_t v;
            v.x = t[c][2 * n]; v.y = t[c][2 * n + 1];
            f[c][n] = v * sc;                                       // one v_pk_mul_f32 per two values
        }
}

// horizontal level-2 sums of a level-1 row at the lane's two level-2 columns
__device__ __forceinline__ void d2_h2(const f2_t (&f)[3][2], f2_t (&h)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f0 = f[c][0].x, f1 = f[c][0].y, f2 = f[c][1].x, f3 = f[c][1].y;
        const float l2 = d2_left(f2), l3 = d2_left(f3), r0 = d2_right(f0);
        h[c].x = fmaf(f0, 6.0f, fmaf(l3 + f1, 4.0f, l2 + f2));      // columns 4g-2 .. 4g+2
        h[c].y = fmaf(f2, 6.0f, fmaf(f1 + f3, 4.0f, f0 + r0));      // columns 4g .. 4g+4
    }
}

struct D2Acc {
    f2_t a[3], b[3], c[3];           // per plane, the lane's two level-2 columns
};

struct D2Out {
    march_rsrc arena;
    unsigned v1, v2;                 // per-lane byte offsets of the group's level-1 / level-2 columns
    unsigned g1, g2;                 // byte offsets of plane 0, row 0 of G_1 / G_2
    unsigned p1b, p2b, plane1b, plane2b;        // (level 1: in the elements G_1 is stored in)
    bool st1, st2;                   // the lane stores level 1 / level 2
};

__device__ __forceinline__ f2_t d2_pair(float v)
{
    f2_t r;
    r.x = r.y = v;
    return r;
}

__device__ __forceinline__ void d2_store2(const D2Out &O, int Y, const f2_t (&v)[3])
{
    if (!O.st2) return;
    const f2_t sc = d2_pair(1.0f / 256.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f2_t o = v[c] * sc;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2_t, o), O.arena, O.v2, O.g2 + c * O.plane2b + (unsigned)Y * O.p2b, D2_ST_AUX);
    }
}

// One level-1 row r of the march.  EVEN: r is even.  `cur` holds level-0 rows 2r + 1 and 2r + 2 on entry and is re-requested
// for row r + 2 (rows 2r + 5, 2r + 6) as soon as its bytes are consumed.  Ring: e0 o0 e1 = rows 2r - 2, 2r - 1, 2r; the row
// leaves o1 e2 = rows 2r + 1, 2r + 2 in `n1`, `n2`.
template <bool EVEN, int G1F>
__device__ __forceinline__ void d2_step(int r, int rn, const D2Row &e0, const D2Row &o0, const D2Row &e1, D2Row &n1, D2Row &n2,
                                        D2Raw (&cur)[2], march_rsrc px, unsigned plo, unsigned stride, int hs, int z0, int z1,
                                        unsigned voff_lo, unsigned voff_hi, D2Acc &G, const D2Out &O, int own_lo, int own_hi, int Y0, int Y1, int h1,
                                        int h2)
{
    d2_hpass(cur[0], n1);
    d2_hpass(cur[1], n2);
    // this set's next rows: those of level-1 row rn (never past the segment's last row: the request then repeats that row's
    // and is not used)
    d2_request(px, plo, stride, d2_row(2 * rn + 1, hs, z0, z1), voff_lo, voff_hi, cur[0]);
    d2_request(px, plo, stride, d2_row(2 * rn + 2, hs, z0, z1), voff_lo, voff_hi, cur[1]);
    f2_t f[3][2];
    unsigned q[3][2];
    d2_vpass(e0, o0, e1, n1, n2, f, q);
    if (O.st1 && r >= own_lo && r < own_hi) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (G1F == G1_U16) {                          // the integers as they stand: 8 bytes per lane and plane
                u2_t o;
                o.x = q[c][0]; o.y = q[c][1];
                __builtin_amdgcn_raw_buffer_store_b64(o, O.arena, O.v1, O.g1 + c * O.plane1b + (unsigned)r * O.p1b, D2_ST_AUX);
                continue;
            }
            u4_t o;
            o.x = __float_as_uint(f[c][0].x); o.y = __float_as_uint(f[c][0].y); o.z = __float_as_uint(f[c][1].x); o.w = __float_as_uint(f[c][1].y);
            __builtin_amdgcn_raw_buffer_store_b128(o, O.arena, O.v1, O.g1 + c * O.plane1b + (unsigned)r * O.p1b, D2_ST_AUX);
        }
    }
    f2_t h[3];
    d2_h2(f, h);
    const int Y = r >> 1;
    if (EVEN) {
        // A + h (twice h where row 2 closes G_2[0]: rows -2, 2 are the same row) finishes G_2[Y - 1]
        const f2_t ka = d2_pair(Y == 1 ? 2.0f : 1.0f);
        f2_t v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __builtin_elementwise_fma(h[c], ka, G.a[c]);
        if (Y - 1 >= Y0 && Y - 1 < Y1) d2_store2(O, Y - 1, v);
        if (r == h1 - 1 && Y < Y1) {
            // h1 odd: the last level-1 row is even, rows 2Y + 1, 2Y + 2 reflect to 2Y - 1, 2Y - 2:
            // G_2[Y] = 2 (h[2Y-2] + 4 h[2Y-1]) + 6 h[2Y]
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = __builtin_elementwise_fma(G.b[c], d2_pair(2.0f), h[c] * d2_pair(6.0f));
            d2_store2(O, Y, v);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G.b[c] = __builtin_elementwise_fma(h[c], d2_pair(6.0f), G.b[c]);
            G.c[c] = h[c];
        }
    } else {
        if (r == h1 - 1 && Y < Y1 && Y >= Y0) {
            // h1 even: the last level-1 row is odd, row 2Y + 2 reflects to 2Y:  G_2[Y] = B + 4 h[2Y+1] + h[2Y], h[2Y] = C
            f2_t v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = __builtin_elementwise_fma(h[c], d2_pair(4.0f), G.b[c]) + G.c[c];
            d2_store2(O, Y, v);
        }
        // rows -1 and 1 are the same row: its weight in G_2[0] doubles
        const f2_t kb = d2_pair(Y == 0 ? 8.0f : 4.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G.a[c] = __builtin_elementwise_fma(h[c], kb, G.b[c]);
            G.b[c] = __builtin_elementwise_fma(h[c], d2_pair(4.0f), G.c[c]);
        }
    }
    (void)h2;
}

template <int CN, int G1F>
__global__ __launch_bounds__(64, D2_WAVES) void k_down2_march(const TileDev *__restrict__ tiles, const TileSrc *__restrict__ srcs, int seg2,
                                                    int march_items, const float *__restrict__ arena_p, unsigned arena_bytes,
                                                    float *__restrict__ arena_w, const float *__restrict__ luts)
{
    static_assert(CN == 3, "the fused level 0 -> 2 march is written for interleaved RGB");
    const TileDev &T = tiles[blockIdx.z];
    if (!down2_takes(T)) return;
    const int ws = T.W[0], hs = T.H[0], w1 = T.W[1], h1 = T.H[1], h2 = T.H[2];
    const int z0 = T.g0[0], z1 = T.g1[0], a1 = T.g0[1], b1 = T.g1[1], a2 = T.g0[2], b2 = T.g1[2];     // rows in use per level
    const int ncg = down_ncg(ws, w1);
    if ((int)blockIdx.x >= march_items) {
        // level-1 border columns: outputs 0 .. 3 and 4 (ncg + 1) .. w1 - 1, per pixel with the full border rule; a block
        // is 16 columns x 4 rows
        const int tid = threadIdx.x, e = tid & 15;
        const int x = e < 4 ? e : 4 * (ncg + 1) + (e - 4);
        const int y = a1 + ((int)blockIdx.x - march_items) * 4 + (tid >> 4);
        if (x >= w1 || y >= b1) return;
        down_pixel<SRC_U8, G1F>(T, srcs[blockIdx.z], 0, CN, x, y, arena_w, luts);
        return;
    }
    const int nstrip = down2_nstrip(ncg), nseg = (b2 - a2 + seg2 - 1) / seg2;
    const int item = blockIdx.x;
    if (item >= nstrip * nseg) return;
    const int seg = item / nstrip, strip = item - seg * nstrip;
    const int lane = threadIdx.x;
    const int g = D2_OUT * strip + lane - 1;                        // lane 1 of a strip: a multiple of 8 groups = a line start of G_1
    const TileSrc S = srcs[blockIdx.z];
    const unsigned stride = (unsigned)S.stride;
    const unsigned plo = (unsigned)(size_t)S.p;
    const march_rsrc px = march_make_rsrc((const char *)S.p - 12, 0xFFFFFFFFu);
    // lanes past the row's groups repeat the last loads that stay inside the row (their values are never used)
    const unsigned voff_lo = 24u * (unsigned)min(max(g, 1), ncg + 1), voff_hi = 24u * (unsigned)min(max(g, 1), ncg) + 12u;
    D2Out O;
    O.arena = march_make_rsrc(arena_p, arena_bytes);
    O.v1 = 4u * G1<G1F>::ES * (unsigned)g;
    O.v2 = 8u * (unsigned)g;
    O.g1 = (unsigned)T.g_off[1] * 4u;
    O.g2 = (unsigned)T.g_off[2] * 4u;
    O.p1b = (unsigned)T.P[1] * G1<G1F>::ES;
    O.p2b = (unsigned)T.P[2] * 4u;
    O.plane1b = (unsigned)h1 * O.p1b;
    O.plane2b = (unsigned)h2 * O.p2b;
    O.st1 = lane >= 1 && lane <= D2_OUT && g >= 1 && g <= ncg;
    O.st2 = lane >= 1 && lane <= D2_OUT && g >= 2 && g <= ncg - 1;
    // The segment's level-2 rows Y0 .. Y1 - 1; the level-1 rows it stores: those between its level-2 rows' centres, the first
    // and the last segment also what the window holds beyond them (rows only the gather reads); the rows it marches: from two
    // before the first centre (even) to the one that closes G_2[Y1 - 1].
    const int Y0 = a2 + seg * seg2, Y1 = min(Y0 + seg2, b2);
    const int own_lo = seg == 0 ? min(a1, 2 * Y0) : 2 * Y0, own_hi = seg == nseg - 1 ? max(b1, min(2 * Y1, h1)) : min(2 * Y1, h1);
    const int st_lo = max(own_lo, a1), st_hi = min(own_hi, b1);
    const int rs = min(own_lo, max(2 * Y0 - 2, 0)) & ~1, re = max(own_hi - 1, min(2 * Y1, h1 - 1));
    D2Raw rq[2 * D2_AHEAD][2], t3[3];
    D2Row A0, A1, A2, B0, B1, B2, B3;
    // rows 2 rs - 2, 2 rs - 1, 2 rs (reflected above the tile), then the two rows of each of the first 2 D2_AHEAD steps
    d2_request(px, plo, stride, d2_row(2 * rs - 2, hs, z0, z1), voff_lo, voff_hi, t3[0]);
    d2_request(px, plo, stride, d2_row(2 * rs - 1, hs, z0, z1), voff_lo, voff_hi, t3[1]);
    d2_request(px, plo, stride, d2_row(2 * rs, hs, z0, z1), voff_lo, voff_hi, t3[2]);
#pragma unroll
    for (int i = 0; i < 2 * D2_AHEAD; ++i) {
        const int rn = min(rs + i, re);
        d2_request(px, plo, stride, d2_row(2 * rn + 1, hs, z0, z1), voff_lo, voff_hi, rq[i][0]);
        d2_request(px, plo, stride, d2_row(2 * rn + 2, hs, z0, z1), voff_lo, voff_hi, rq[i][1]);
    }
    d2_hpass(t3[0], A0);
    d2_hpass(t3[1], A1);
    d2_hpass(t3[2], A2);
    D2Acc G;
#pragma unroll
    for (int c = 0; c < 3; ++c) G.a[c] = G.b[c] = G.c[c] = d2_pair(0.f);
    // Two level-1 rows per round.  Ring on entry: (A0 A1 A2) = rows 2r - 2, 2r - 1, 2r.  Row r leaves rows 2r + 1, 2r + 2 in
    // (B0 B1); row r + 1 then has (A2 B0 B1) and leaves rows 2r + 3, 2r + 4 in (B2 B3); the ring of the next round is
    // (B1 B2 B3): three moves of six registers per two rows.  A row's level-0 rows were requested 2 D2_AHEAD rows earlier, into
    // request set (row - rs) mod 2 D2_AHEAD (static: the loop body is D2_AHEAD rounds).
#define D2_ROUND(R, S0, S1)                                                                                                        \
    do {                                                                                                                           \
        if ((R) <= re) {                                                                                                           \
            d2_step<true, G1F>((R), min((R) + 2 * D2_AHEAD, re), A0, A1, A2, B0, B1, rq[S0], px, plo, stride, hs, z0, z1, voff_lo, voff_hi, G, O, \
                          st_lo, st_hi, Y0, Y1, h1, h2);                                                                                 \
            if ((R) + 1 <= re)                                                                                                     \
                d2_step<false, G1F>((R) + 1, min((R) + 1 + 2 * D2_AHEAD, re), A2, B0, B1, B2, B3, rq[S1], px, plo, stride, hs, z0, z1, voff_lo, voff_hi, \
                               G, O, st_lo, st_hi, Y0, Y1, h1, h2);                                                                 \
            A0 = B1; A1 = B2; A2 = B3;                                                                                             \
        }                                                                                                                          \
    } while (0)
#pragma unroll 1
    for (int r = rs; r <= re; r += 2 * D2_AHEAD) {
        D2_ROUND(r, 0, 1);
#if D2_AHEAD >= 2
        D2_ROUND(r + 2, 2, 3);
#endif
#if D2_AHEAD >= 3
        D2_ROUND(r + 4, 4, 5);
#endif
    }
#undef D2_ROUND
}

// level-2 columns the march leaves out -- 0 .. 3 and 2 ncg .. w2 - 1 (every column from 4 on when the tile has fewer than three
// groups) -- of the tiles down2_takes: per pixel from G_1 in memory.  This launch stands between the march and level 3 in the
// chain, and beside the previous image's assessment (whose three blocks per CU leave 110 registers per SIMD) it gets one
// block per CU and pays a loaded-memory round trip (~18 us) per block generation: the first version (16 x 16 slots of which
// 7-11 columns were in use, the planes one after the other: three round trips) took 0.26-0.30 ms in the image stream for
// 0.03 ms of work.  Here every lane has a pixel, and its 75 loads (three planes) are issued before the first use.
template <int G1F>
__global__ __launch_bounds__(256, 4) void k_down2_cols(const TileDev *__restrict__ tiles, float *__restrict__ arena)
{
    const TileDev &T = tiles[blockIdx.z];
    if (!down2_takes(T)) return;
    const int ncg = down_ncg(T.W[0], T.W[1]), w2 = T.W[2], h2 = T.H[2], h1 = T.H[1], w1 = T.W[1], p1 = T.P[1], p2 = T.P[2];
    const int c_right = ncg >= 3 ? 2 * ncg : 4;
    const int nleft = w2 < 4 ? w2 : 4, ncols = down2_cols_count(T);
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int yr = t / ncols, ci = t - yr * ncols;
    const int y = T.g0[2] + yr;                                     // rows of the level-2 window
    if (y >= T.g1[2]) return;
    const int x = ci < nleft ? ci : c_right + (ci - nleft);
    int xi[5], yi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        xi[k] = reflect101(2 * x + k - 2, w1);
        yi[k] = reflect101(2 * y + k - 2, h1);
    }
    const float *src = arena + T.g_off[1];
    const size_t splane = (size_t)h1 * p1, dplane = (size_t)h2 * p2;
    float s[3][5][5];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int j = 0; j < 5; ++j) s[c][k][j] = G1<G1F>::at(src, c * splane + (size_t)yi[k] * p1 + xi[j]);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float rowv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) rowv[k] = ((s[c][k][2] * 6.0f + (s[c][k][1] + s[c][k][3]) * 4.0f) + s[c][k][0]) + s[c][k][4];
        v[c] = (((rowv[2] * 6.0f + (rowv[1] + rowv[3]) * 4.0f) + rowv[0]) + rowv[4]) * (1.0f / 256.0f);
    }
    float *dst = arena + T.g_off[2] + (size_t)y * p2 + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * dplane] = v[c];
}
