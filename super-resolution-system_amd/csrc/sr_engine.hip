// sr_engine.hip -- the blend engine on gfx950 (CDNA4): the blend plan (its tables come from sr_blend_plan.cpp), its pyramids and
// gathers (with sr_march.inc and sr_down2.inc), the custom-weight blend, and their part of the C ABI in include/sr_hip.h.  (Context, device memory and
// profiling are sr_runtime.hip; tile extract, the dense pyramid primitives, seam scan and feather merge are sr_tiles.hip;
// the quality-assessment stage is sr_assess.hip.)
//
// Numerics contract: every fp32 expression is evaluated in the order written in
// oracle/sr_oracle.c (build with -ffp-contract=off), so the blend agrees with the CPU
// restatement bit for bit.
//
// Data layout in HBM
//   * external images / tiles / canvas: row-major HWC, u8 (or fp32 tiles), byte strides --
//     exactly the reference's ndarrays.
//   * internal pyramid levels i >= 1 of every tile live in one arena: planar fp32, plane
//     c of level i at  off[i] + c * H_i * P_i,  row pitch P_i = round_up(W_i, 32) floats (whole 128-byte lines; level 1: 64, see G1<>).
//     G_i = Gaussian level, R_i = collapsed weighted-Laplacian level, W_i = weight level
//     (one per distinct tile shape).
//   * the fp32 canvas accumulators of the reference are never materialised: the final kernel
//     is canvas-centric (gather) and sums the covering tiles in list order in registers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <type_traits>
#include <vector>

#include "sr_blend_tables.h"
#include "sr_ctx.h"
#include "sr_device.h"

// ---------------------------------------------------------------------------------------------
// live blend plans (the registry of live contexts, and what the registries are for: sr_runtime.hip)
// ---------------------------------------------------------------------------------------------
static std::mutex g_reg_mu;
static std::set<const void *> g_live_plan;
static bool plan_is_live(const sr_blend_plan *p)
{
    std::lock_guard<std::mutex> lk(g_reg_mu);
    return p && g_live_plan.count(p) != 0;
}

// ---------------------------------------------------------------------------------------------
// device helpers (border rules, vector loads / stores, TileSrc and the SRC_* tags, div_shared: sr_device.h)
// ---------------------------------------------------------------------------------------------
// One axis of cv2.pyrUp, unnormalised (x8): value of destination column x from source row `row`.
__device__ __forceinline__ float up_h(const float *__restrict__ row, int ws, int x)
{
    const int sx = x >> 1;
    if (ws == 1) return (x & 1) ? row[0] * 8.0f : row[0] * 6.0f + row[0] * 2.0f;
    if (!(x & 1)) {
        if (sx == 0) return row[0] * 6.0f + row[1] * 2.0f;
        if (sx == ws - 1) return row[sx - 1] + row[sx] * 7.0f;
        return (row[sx - 1] + row[sx] * 6.0f) + row[sx + 1];
    }
    if (sx == ws - 1) return row[sx] * 8.0f;
    return (row[sx] + row[sx + 1]) * 4.0f;
}

// cv2.pyrUp sample at destination (y, x) from one planar fp32 source plane (hs x ws, pitch).
__device__ __forceinline__ float up_sample(const float *__restrict__ src, int hs, int ws, int pitch, int y,
                                           int x)
{
    const int sy = y >> 1;
    const int yp = min(sy + 1, hs - 1);
    const float r1 = up_h(src + (size_t)sy * pitch, ws, x);
    const float r2 = up_h(src + (size_t)yp * pitch, ws, x);
    if (!(y & 1)) {
        const int ym = (sy - 1 < 0) ? (hs > 1 ? 1 : 0) : sy - 1;
        const float r0 = up_h(src + (size_t)ym * pitch, ws, x);
        return ((r0 + r1 * 6.0f) + r2) * (1.0f / 64.0f);
    }
    return ((r1 + r2) * 4.0f) * (1.0f / 64.0f);
}

// (the blend plan tables TileDev, FinalDesc, EdgeBlock, MarchItem and RectItem: sr_blend_tables.h)

// How the level-1 Gaussian planes G_1 lie in the arena.  G1_F32: fp32.  G1_U16: the integer 256 G_1 in 16 bits -- for u8
// tiles it is exact and below 2^16 (sr_down2.inc), and k_down2_march holds it in that form anyway.  A 16-bit plane starts where
// the fp32 plane it replaces would (same offsets, same pitch and plane size IN ELEMENTS: every index below is shared), so
// its rows are half as long in bytes.  Which format a call uses: g1_format() on the host, the same in sr_blend_pyramids and
// sr_blend_gather.  Every reader of G_1 goes through G1<>: (float)n * (1 / 256) is exact, the bits of the fp32 value.
enum { G1_F32 = 0, G1_U16 = 1 };
template <int G1F>
struct G1 {
    static constexpr unsigned ES = G1F == G1_U16 ? 2u : 4u;         // bytes per element
    typedef typename std::conditional<G1F == G1_U16, unsigned, f2_t>::type pair_t;      // two neighbouring elements as loaded
    static __device__ __forceinline__ float value(unsigned n) { return (float)n * (1.0f / 256.0f); }
    // element i of the planes that start at `planes` (the arena + g_off[1] / FinalDesc::g1)
    static __device__ __forceinline__ float at(const float *planes, size_t i)
    {
        if constexpr (G1F == G1_U16) return value(((const unsigned short *)planes)[i]);
        else return planes[i];
    }
    // elements i .. i + 3 (i a multiple of 4)
    static __device__ __forceinline__ f4_t quad(const float *planes, size_t i)
    {
        if constexpr (G1F == G1_U16) {
            const u2_t q = *(const u2_t *)((const unsigned short *)planes + i);
            f4_t v;
            v.x = value(q.x & 0xFFFFu); v.y = value(q.x >> 16); v.z = value(q.y & 0xFFFFu); v.w = value(q.y >> 16);
            return v;
        } else {
            return ld_f4(planes + i);
        }
    }
    static __device__ __forceinline__ f2_t pair(pair_t q)
    {
        if constexpr (G1F == G1_U16) {
            f2_t v;
            v.x = value(q & 0xFFFFu); v.y = value(q >> 16);
            return v;
        } else {
            return q;
        }
    }
};

// Source accessors for the pyrDown kernel -----------------------------------------------------
// One output pixel (all planes) of level lvl+1 from level lvl -- the generic form with every border rule.
// G1F = G1_U16 (level 0 -> 1 of u8 tiles only): the sum itself is stored, in 16 bits.
template <int SRC, int G1F = G1_F32>
__device__ __forceinline__ void down_pixel(const TileDev &T, const TileSrc S, int lvl, int cn, int x, int y,
                                           float *__restrict__ arena, const float *__restrict__ luts, int c_only = -1)
{
    const int hs = T.H[lvl], ws = T.W[lvl];
    int xi[5], yi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        xi[k] = reflect101(2 * x + k - 2, ws);
        yi[k] = reflect101(2 * y + k - 2, hs);
    }
    const int po = T.P[lvl + 1];
    float *dst = arena + T.g_off[lvl + 1] + (size_t)y * po + x;
    const size_t dplane = (size_t)T.H[lvl + 1] * po;
    // c_only >= 0: that plane alone (a thread per plane: its 25 loads are one round trip, no store of another plane between them)
    for (int c = c_only >= 0 ? c_only : 0; c < (c_only >= 0 ? c_only + 1 : cn); ++c) {
        float rowv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float s[5];
            if (SRC == SRC_U8) {
                const unsigned char *r = (const unsigned char *)S.p + (size_t)yi[k] * S.stride;
#pragma unroll
                for (int j = 0; j < 5; ++j) s[j] = (float)r[xi[j] * cn + c];
            } else if (SRC == SRC_F32) {
                const float *r = (const float *)((const char *)S.p + (size_t)yi[k] * S.stride);
#pragma unroll
                for (int j = 0; j < 5; ++j) s[j] = r[xi[j] * cn + c];
            } else if (SRC == SRC_PLANAR) {
                const float *r = arena + T.g_off[lvl] + (size_t)c * hs * T.P[lvl] + (size_t)yi[k] * T.P[lvl];
#pragma unroll
                for (int j = 0; j < 5; ++j) s[j] = r[xi[j]];
            } else {  // SRC_LUT: analytic weight map, level 0 of a weight class
                const int ry = yi[k];
                const int dy = min(ry, hs - 1 - ry);
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int dx = min(xi[j], ws - 1 - xi[j]);
                    s[j] = luts[T.lut_off + min(min(dy, dx), T.fw)];
                }
            }
            rowv[k] = ((s[2] * 6.0f + (s[1] + s[3]) * 4.0f) + s[0]) + s[4];
        }
        const float v = ((rowv[2] * 6.0f + (rowv[1] + rowv[3]) * 4.0f) + rowv[0]) + rowv[4];
        if constexpr (G1F == G1_U16) {
            static_assert(SRC == SRC_U8, "256 G_1 is a 16-bit integer for u8 tiles only");
            ((unsigned short *)(arena + T.g_off[lvl + 1]))[c * dplane + (size_t)y * po + x] = (unsigned short)v;
            continue;
        }
        dst[c * dplane] = v * (1.0f / 256.0f);
    }
}

// level i -> i+1 of every tile (or weight class) in one launch.  One thread = one output pixel,
// all planes.  Rows limited to the G window of the destination level.  (Generic kernel: weight classes,
// fp32 HWC tiles, channel counts other than 1 / 3.)
template <int SRC>
__global__ __launch_bounds__(256) void k_down(const TileDev *__restrict__ tiles, const TileSrc *__restrict__ srcs,
                                              int lvl, int cn, float *__restrict__ arena,
                                              const float *__restrict__ luts)
{
    const TileDev &T = tiles[blockIdx.z];
    if (lvl + 1 >= T.nl) return;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = T.g0[lvl + 1] + blockIdx.y * 4 + threadIdx.y;
    if (x >= T.W[lvl + 1] || y >= T.g1[lvl + 1]) return;
    TileSrc S;
    S.p = nullptr;
    S.stride = 0;
    if (SRC == SRC_U8 || SRC == SRC_F32) S = srcs[blockIdx.z];
    down_pixel<SRC>(T, S, lvl, cn, x, y, arena, luts);
}

// ---------------------------------------------------------------------------------------------
// Column-marching pyrDown.  One thread owns 4 output columns (a "column group": output x0 = 4 * cg, input columns
// 2 x0 - 2 .. 2 x0 + 8) and walks down seg_rows output rows: every input row is loaded once and its horizontal pass
// evaluated once; the five row-pass results an output row needs (rows 2y-2 .. 2y+2) live in registers.  Row indices
// go through REFLECT_101, so the top / bottom tile borders need no separate path.  Only "interior" column groups
// (whole window inside the row: cg = 1 .. ncg) take the march; the few border columns of a level are done by the
// trailing blocks of the same launch.
// Lanes are laid over (segment, column group) cells flattened per tile, so waves are full except the last one.
// seg_rows (output rows per segment, chosen per launch): longer segments amortise the 3-row prologue, shorter ones
// keep enough cells in flight on the small levels.
// ---------------------------------------------------------------------------------------------

// REFLECT_101 of a row index that leaves [0, n) by at most n - 1 (one bounce, no loop) -- the march's rows do by <= 2
__device__ __forceinline__ int reflect101_once(int p, int n)
{
    if (n == 1) return 0;
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - 2 - p : p;
}

// horizontal pass of one u8 row for the thread's 4 outputs x CN channels.  All values are integers below 2^24, so
// fp32 evaluates them exactly in any order: bit-identical to ((s2*6 + (s1+s3)*4) + s0) + s4 with two fmas.
template <int CN>
__device__ __forceinline__ void down_row_u8(const unsigned (&wds)[(CN == 3) ? 9 : 3], float (&h)[4 * CN])
{
    float s[11][CN];
#pragma unroll
    for (int b = 0; b < 11 * CN; ++b) s[b / CN][b % CN] = (float)((wds[b >> 2] >> (8 * (b & 3))) & 0xFFu);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < CN; ++c)
            h[k * CN + c] = fmaf(s[2 * k + 2][c], 6.0f, fmaf(s[2 * k + 1][c] + s[2 * k + 3][c], 4.0f, s[2 * k][c] + s[2 * k + 4][c]));
}

template <int CN>
__device__ __forceinline__ void down_load_u8(const unsigned char *__restrict__ base, long long stride, int row, int xb,
                                             unsigned (&wds)[(CN == 3) ? 9 : 3])
{
    // the tile pointer comes out of a table in memory: tell the compiler it is global memory (global_load, not flat_load)
    const unsigned char *p = base + (size_t)row * stride + (size_t)xb * CN;
    if (CN == 3) {
        // Dword-aligned loads + one funnel shift per dword instead of three byte-aligned 12-byte loads (the memory
        // pipeline was the limiter of this kernel: MemUnitStalled 70 %; -6 % run time).  m = byte offset of the window
        // inside its first dword (per lane: lanes of one wave can sit in different row segments); the 33 bytes needed lie
        // inside the nine aligned dwords [p - m, p - m + 36): no byte beyond what the unaligned loads touched is read.
        typedef u3_t u3_a4_t __attribute__((aligned(4)));
        const unsigned m = (unsigned)((size_t)p & 3u);
        const unsigned char *q = p - m;
        const u3_t q0 = *(const __attribute__((address_space(1))) u3_a4_t *)q, q1 = *(const __attribute__((address_space(1))) u3_a4_t *)(q + 12),
                   q2 = *(const __attribute__((address_space(1))) u3_a4_t *)(q + 24);
        const unsigned d[10] = {q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z, 0u};
#pragma unroll
        for (int i = 0; i < 9; ++i) wds[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], m);
    } else {
        const u3_t q0 = ld_u3_a1_g(p);
        wds[0] = q0.x; wds[1] = q0.y; wds[2] = q0.z;
    }
}

__device__ __forceinline__ void down_load_f32(const float *__restrict__ plane, int ps, int row, int xb, float (&s)[11])
{
    const float *p = plane + (size_t)row * ps + xb;          // xb = 8 cg - 2: 8-byte aligned, xb + 2 16-byte aligned
    const f2_t a = *(const f2_a8_t *)p;
    const f4_t b = ld_f4(p + 2), d = ld_f4(p + 6);
    s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y; s[4] = b.z; s[5] = b.w; s[6] = d.x; s[7] = d.y; s[8] = d.z; s[9] = d.w;
    s[10] = p[10];
}

__device__ __forceinline__ void down_row_f32(const float (&s)[11], float (&h)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = ((s[2 * k + 2] * 6.0f + (s[2 * k + 1] + s[2 * k + 3]) * 4.0f) + s[2 * k]) + s[2 * k + 4];
}

template <int SRC, int CN>
__global__ __launch_bounds__(256) void k_down_march(const TileDev *__restrict__ tiles, const TileSrc *__restrict__ srcs,
                                                    int lvl, int seg_rows, int march_blocks, float *__restrict__ arena,
                                                    const float *__restrict__ luts, int skip_down2)
{
    const TileDev &T = tiles[blockIdx.z];
    if (lvl + 1 >= T.nl) return;
    if (skip_down2 && down2_takes(T)) return;                       // levels 1 and 2 of this tile come from k_down2_march
    const int ws = T.W[lvl], hs = T.H[lvl], wo = T.W[lvl + 1];
    const int ya = T.g0[lvl + 1], yb = T.g1[lvl + 1];
    const int ncg = down_ncg(ws, wo);
    if ((int)blockIdx.x >= march_blocks) {
        // The border columns the march leaves out: outputs 0 .. 3 and 4 (ncg + 1) .. wo - 1 (at most 12 columns;
        // every column when the level has no interior column group), one pixel per thread with the full border
        // rule -- the trailing blocks of the same launch, 16 columns x 16 rows each.
        const int tid = threadIdx.y * 64 + threadIdx.x;
        const int e = tid & 15;
        const int x = (ncg <= 0 || e < 4) ? e : 4 * (ncg + 1) + (e - 4);
        const int y = ya + ((int)blockIdx.x - march_blocks) * 16 + (tid >> 4);
        if (x >= wo || y >= yb) return;
        TileSrc S;
        S.p = nullptr;
        S.stride = 0;
        if (SRC == SRC_U8) S = srcs[blockIdx.z];
        down_pixel<SRC>(T, S, lvl, CN, x, y, arena, luts);
        return;
    }
    if (ncg <= 0 || yb <= ya) return;
    const int nseg = (yb - ya + seg_rows - 1) / seg_rows;
    const int cell = blockIdx.x * 256 + threadIdx.y * 64 + threadIdx.x;
    if (cell >= ncg * nseg) return;
    const int seg = cell / ncg, x0 = (1 + cell - seg * ncg) * 4;
    const int y_begin = ya + seg * seg_rows, y_end = min(y_begin + seg_rows, yb);
    const int po = T.P[lvl + 1];
    const size_t dplane = (size_t)T.H[lvl + 1] * po;
    float *dst = arena + T.g_off[lvl + 1] + x0;
    const int xb = 2 * x0 - 2;
    if (SRC == SRC_U8) {
        constexpr int NW = (CN == 3) ? 9 : 3, NV = 4 * CN;
        const TileSrc S = srcs[blockIdx.z];
        const unsigned char *base = (const unsigned char *)S.p;
        unsigned w0[NW], w1[NW], n0[NW], n1[NW];
        float e0[NV], o0[NV], e1[NV], o1[NV], e2[NV];
        down_load_u8<CN>(base, S.stride, reflect101_once(2 * y_begin - 2, hs), xb, w0);
        down_load_u8<CN>(base, S.stride, reflect101_once(2 * y_begin - 1, hs), xb, w1);
        down_load_u8<CN>(base, S.stride, 2 * y_begin, xb, n0);
        down_row_u8<CN>(w0, e0);
        down_row_u8<CN>(w1, o0);
        down_row_u8<CN>(n0, e1);
        down_load_u8<CN>(base, S.stride, reflect101_once(2 * y_begin + 1, hs), xb, w0);
        down_load_u8<CN>(base, S.stride, reflect101_once(2 * y_begin + 2, hs), xb, w1);
        for (int y = y_begin; y < y_end; ++y) {
            // the two rows of the NEXT output row are requested first and land in their own registers: a whole
            // iteration of arithmetic (row passes of the current rows, column pass, stores) covers their latency
            // (unconditional -- the last iteration re-reads its own rows -- so the compiler can keep exactly these
            // loads outstanding with a counted s_waitcnt instead of draining at a control-flow join)
            const int yn = min(y + 1, y_end - 1);
            down_load_u8<CN>(base, S.stride, reflect101_once(2 * yn + 1, hs), xb, n0);
            down_load_u8<CN>(base, S.stride, reflect101_once(2 * yn + 2, hs), xb, n1);
            down_row_u8<CN>(w0, o1);
            down_row_u8<CN>(w1, e2);
#pragma unroll
            for (int i = 0; i < NW; ++i) { w0[i] = n0[i]; w1[i] = n1[i]; }
#pragma unroll
            for (int c = 0; c < CN; ++c) {
                f4_t ov;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = k * CN + c;    // integers below 2^24 again: exact in any order
                    o[k] = fmaf(e1[i], 6.0f, fmaf(o0[i] + o1[i], 4.0f, e0[i] + e2[i])) * (1.0f / 256.0f);
                }
                ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
                st_f4(dst + c * dplane + (size_t)y * po, ov);
            }
#pragma unroll
            for (int i = 0; i < NV; ++i) { e0[i] = e1[i]; o0[i] = o1[i]; e1[i] = e2[i]; }
        }
    } else {  // SRC_PLANAR: fp32 rounds, the reference's evaluation order is kept
        const int ps = T.P[lvl];
        const size_t splane = (size_t)hs * ps;
#pragma unroll 1
        for (int c = 0; c < CN; ++c) {
            const float *plane = arena + T.g_off[lvl] + c * splane;
            float s0[11], s1[11], t0[11], t1[11];
            float e0[4], o0[4], e1[4], o1[4], e2[4];
            down_load_f32(plane, ps, reflect101_once(2 * y_begin - 2, hs), xb, s0);
            down_load_f32(plane, ps, reflect101_once(2 * y_begin - 1, hs), xb, s1);
            down_load_f32(plane, ps, 2 * y_begin, xb, t0);
            down_row_f32(s0, e0);
            down_row_f32(s1, o0);
            down_row_f32(t0, e1);
            down_load_f32(plane, ps, reflect101_once(2 * y_begin + 1, hs), xb, s0);
            down_load_f32(plane, ps, reflect101_once(2 * y_begin + 2, hs), xb, s1);
            for (int y = y_begin; y < y_end; ++y) {
                const int yn = min(y + 1, y_end - 1);   // next output row's rows first, into their own registers
                down_load_f32(plane, ps, reflect101_once(2 * yn + 1, hs), xb, t0);
                down_load_f32(plane, ps, reflect101_once(2 * yn + 2, hs), xb, t1);
                down_row_f32(s0, o1);
                down_row_f32(s1, e2);
#pragma unroll
                for (int i = 0; i < 11; ++i) { s0[i] = t0[i]; s1[i] = t1[i]; }
                f4_t ov;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = ((((e1[k] * 6.0f + (o0[k] + o1[k]) * 4.0f) + e0[k]) + e2[k])) * (1.0f / 256.0f);
                ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
                st_f4(dst + c * dplane + (size_t)y * po, ov);
#pragma unroll
                for (int k = 0; k < 4; ++k) { e0[k] = e1[k]; o0[k] = o1[k]; e1[k] = e2[k]; }
            }
        }
    }
}

// R_i for one level of every tile:  top level: G*W;  else up(R_{i+1}) + (G_i - up(G_{i+1})) * W_i
__global__ __launch_bounds__(256) void k_up_level(const TileDev *__restrict__ tiles, int lvl, int cn,
                                                  float *__restrict__ arena)
{
    const TileDev &T = tiles[blockIdx.z];
    if (lvl >= T.nl) return;
    const int w = T.W[lvl], h = T.H[lvl], p = T.P[lvl];
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = T.r0[lvl] + blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= T.r1[lvl]) return;
    const float wv = arena[T.w_off[lvl] + (size_t)y * p + x];
    const size_t plane = (size_t)h * p;
    const float *g = arena + T.g_off[lvl] + (size_t)y * p + x;
    float *r = arena + T.r_off[lvl] + (size_t)y * p + x;
    if (lvl == T.nl - 1) {
        for (int c = 0; c < cn; ++c) r[c * plane] = g[c * plane] * wv;
        return;
    }
    const int hs = T.H[lvl + 1], ws = T.W[lvl + 1], ps = T.P[lvl + 1];
    const size_t splane = (size_t)hs * ps;
    const float *gs = arena + T.g_off[lvl + 1];
    const float *rs = arena + T.r_off[lvl + 1];
    for (int c = 0; c < cn; ++c) {
        const float ug = up_sample(gs + c * splane, hs, ws, ps, y, x);
        const float ur = up_sample(rs + c * splane, hs, ws, ps, y, x);
        const float lap = g[c * plane] - ug;
        const float wl = lap * wv;
        r[c * plane] = ur + wl;
    }
}

// Final level, canvas-centric: for each canvas pixel sum the covering tiles in list order
// (acc += R_0, wacc += W_0), normalise, clip, truncate.  LAP == false: weighted_average_fusion.
template <int DT, bool LAP>
__global__ __launch_bounds__(256) void k_final(const TileDev *__restrict__ tiles, const TileSrc *__restrict__ srcs,
                                               int n, int cn, const float *__restrict__ arena,
                                               const float *__restrict__ luts, unsigned char *__restrict__ canvas,
                                               long long cstride, float *__restrict__ canvas_f32, int cw,
                                               int row_begin, int row_end)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = row_begin + blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= row_end) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float wacc = 0.f;
    for (int t = 0; t < n; ++t) {
        const TileDev &T = tiles[t];
        const int lx = x - T.x, ly = y - T.y;
        if (lx < 0 || ly < 0 || lx >= T.w || ly >= T.h) continue;
        const int d = min(min(ly, T.h - 1 - ly), min(lx, T.w - 1 - lx));
        const float w0 = luts[T.lut_off + min(d, T.fw)];
        const char *srow = (const char *)srcs[t].p + (size_t)ly * srcs[t].stride;
        for (int c = 0; c < cn; ++c) {
            float g0;
            if (DT == SRC_U8) g0 = (float)((const unsigned char *)srow)[lx * cn + c];
            else g0 = ((const float *)srow)[lx * cn + c];
            float r;
            if (LAP && T.nl > 1) {
                const int hs = T.H[1], ws = T.W[1], ps = T.P[1];
                const size_t splane = (size_t)hs * ps;
                const float ug = up_sample(arena + T.g_off[1] + c * splane, hs, ws, ps, ly, lx);
                const float ur = up_sample(arena + T.r_off[1] + c * splane, hs, ws, ps, ly, lx);
                const float lap = g0 - ug;
                const float wl = lap * w0;
                r = ur + wl;
            } else {
                r = g0 * w0;
            }
            acc[c] += r;
        }
        wacc += w0;
    }
    const float wv = wacc > 1e-6f ? wacc : 1e-6f;
    unsigned char *o = canvas + (size_t)y * cstride + (size_t)x * cn;
    for (int c = 0; c < cn; ++c) {
        const float v = acc[c] / wv;
        if (canvas_f32) canvas_f32[((size_t)y * cw + x) * cn + c] = v;
        const float cl = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        o[c] = (unsigned char)cl;
    }
}

// ---------------------------------------------------------------------------------------------
// pyrUp of a thread's 4 x 2 pixels from ONE 3-row x 4-column neighbourhood of a level (the same per-pixel expressions as
// up_sample, 12 loads per 8 pixels instead of 6-9 per pixel).  x0 is a multiple of 4 and y0 - row_begin a multiple of 2,
// so the parity of the tile-local origin -- which selects the even/odd pyrUp phase of every pixel in the thread -- is
// uniform per tile across a launch (template XO / YO).
// ---------------------------------------------------------------------------------------------
template <int POS, bool ODD>
__device__ __forceinline__ float up_h_reg(const float (&v)[4], int ws, int sx)
{
    if (ws == 1) return ODD ? v[POS] * 8.0f : v[POS] * 6.0f + v[POS] * 2.0f;
    if (!ODD) {
        constexpr int PM = POS > 0 ? POS - 1 : 0;
        if (sx == 0) return v[POS] * 6.0f + v[POS + 1] * 2.0f;
        if (sx == ws - 1) return v[PM] + v[POS] * 7.0f;
        return (v[PM] + v[POS] * 6.0f) + v[POS + 1];
    }
    constexpr int PP = POS < 3 ? POS + 1 : 3;
    if (sx == ws - 1) return v[POS] * 8.0f;
    return (v[POS] + v[PP]) * 4.0f;
}

// h[r][k]: unnormalised horizontal pyrUp of loaded row r at thread pixel k
template <bool XO>
__device__ __forceinline__ void up_rows4(const float (&v)[3][4], int ws, int c0, float (&h)[3][4])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (!XO) {
            h[r][0] = up_h_reg<1, false>(v[r], ws, c0 + 1);
            h[r][1] = up_h_reg<1, true>(v[r], ws, c0 + 1);
            h[r][2] = up_h_reg<2, false>(v[r], ws, c0 + 2);
            h[r][3] = up_h_reg<2, true>(v[r], ws, c0 + 2);
        } else {
            h[r][0] = up_h_reg<0, true>(v[r], ws, c0);
            h[r][1] = up_h_reg<1, false>(v[r], ws, c0 + 1);
            h[r][2] = up_h_reg<1, true>(v[r], ws, c0 + 1);
            h[r][3] = up_h_reg<2, false>(v[r], ws, c0 + 2);
        }
    }
}

// vertical combination for the thread's two rows (j = 0, 1) at pixel column k
template <bool YO>
__device__ __forceinline__ void up_cols2(const float (&h)[3][4], int r0, float (&u)[2][4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!YO) {
            // j = 0: even row, sy = r0 + 1;  j = 1: odd row, sy = r0 + 1
            const float top = (r0 + 1 == 0) ? h[2][k] : h[0][k];
            u[0][k] = ((top + h[1][k] * 6.0f) + h[2][k]) * (1.0f / 64.0f);
            u[1][k] = ((h[1][k] + h[2][k]) * 4.0f) * (1.0f / 64.0f);
        } else {
            // j = 0: odd row, sy = r0;  j = 1: even row, sy = r0 + 1
            const float top = (r0 + 1 == 0) ? h[2][k] : h[0][k];
            u[0][k] = ((h[0][k] + h[1][k]) * 4.0f) * (1.0f / 64.0f);
            u[1][k] = ((top + h[1][k] * 6.0f) + h[2][k]) * (1.0f / 64.0f);
        }
    }
}

template <bool XO, bool YO>
__device__ __forceinline__ void up_block(const float *__restrict__ plane, int hs, int ws, int ps, int r0, int c0,
                                         float (&u)[2][4])
{
    float v[3][4], h[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float *row = plane + (size_t)min(max(r0 + r, 0), hs - 1) * ps;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = row[min(max(c0 + c, 0), ws - 1)];
    }
    up_rows4<XO>(v, ws, c0, h);
    up_cols2<YO>(h, r0, u);
}


// interior form of up_block: every pixel of the thread is away from the level-1 borders, so the
// border selects of up_h / the row clamps vanish; same expressions as the generic path otherwise
template <bool XO, bool YO>
__device__ __forceinline__ void up_block_interior(const float *__restrict__ plane, int ps, int r0, int c0,
                                                  float (&u)[2][4])
{
    float h[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const f4_t q = ld_f4_a4(plane + (size_t)(r0 + r) * ps + c0);
        // power-of-two factors of the odd phases are folded into the final constants (exact; see up_pairs)
        if (!XO) {
            h[r][0] = (q.x + q.y * 6.0f) + q.z;
            h[r][1] = q.y + q.z;
            h[r][2] = (q.y + q.z * 6.0f) + q.w;
            h[r][3] = q.z + q.w;
        } else {
            h[r][0] = q.x + q.y;
            h[r][1] = (q.x + q.y * 6.0f) + q.z;
            h[r][2] = q.y + q.z;
            h[r][3] = (q.y + q.z * 6.0f) + q.w;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool kodd = XO ? ((k & 1) == 0) : ((k & 1) == 1);
        const float ce = kodd ? (1.0f / 16.0f) : (1.0f / 64.0f);
        const float co = kodd ? (1.0f / 4.0f) : (1.0f / 16.0f);
        const float ev = ((h[0][k] + h[1][k] * 6.0f) + h[2][k]) * ce;
        if (!YO) {
            u[0][k] = ev;
            u[1][k] = (h[1][k] + h[2][k]) * co;
        } else {
            u[0][k] = (h[0][k] + h[1][k]) * co;
            u[1][k] = ev;
        }
    }
}

// Is the thread's 4 x 2 rectangle (tile-local origin lx0, ly0; nx x ny of it on the canvas strip) an
// "interior" visit of tile D: all eight pixels inside the tile and every level-1 tap away from the borders?
// Interior visits run in the regular blocks of k_final_fast, everything else in its edge blocks; both evaluate this same test.
template <bool LAP>
__device__ __forceinline__ bool visit_is_interior(const FinalDesc &D, int lx0, int ly0, int nx, int ny)
{
    if (nx != 4 || ny != 2 || lx0 < 0 || ly0 < 0 || lx0 + 3 >= D.w || ly0 + 1 >= D.h) return false;
    if (LAP && D.nl > 1) {
        const int r0 = (ly0 - 1) >> 1, c0 = (lx0 - 1) >> 1;
        return c0 >= 0 && c0 + 3 <= D.W1 - 1 && r0 >= 0 && r0 + 2 <= D.H1 - 1;
    }
    return true;
}

__device__ __forceinline__ void tile_weights(const FinalDesc &D, const float *__restrict__ luts, int lx0, int ly0,
                                             float (&w0)[2][4])
{
    // edge distance of the whole 4 x 2 rectangle: beyond the feather width every weight is lut[fw]
    const int dmin = min(min(ly0, D.h - 2 - ly0), min(lx0, D.w - 4 - lx0));
    if (dmin >= D.fw) {
        const float wf = luts[D.lut_off + D.fw];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) w0[j][k] = wf;
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lx = lx0 + k, ly = ly0 + j;
            const int d = min(min(ly, D.h - 1 - ly), min(lx, D.w - 1 - lx));
            w0[j][k] = luts[D.lut_off + min(max(d, 0), D.fw)];
        }
}

// weights of an interior visit (all eight pixels inside the tile).  The LUT is monotone in the edge distance, so
// lut[min(dy, dx)] == min(lut[dy], lut[dx]) exactly: 2 + 4 LUT reads and 8 v_min_f32 instead of 8 reads behind
// 8 three-way integer minima.
__device__ __forceinline__ void tile_weights_interior(const FinalDesc &D, const float *__restrict__ luts, int lx0, int ly0,
                                                      float (&w0)[2][4])
{
    const int dmin = min(min(ly0, D.h - 2 - ly0), min(lx0, D.w - 4 - lx0));
    const float *lut = luts + D.lut_off;
    if (dmin >= D.fw) {
        const float wf = lut[D.fw];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) w0[j][k] = wf;
        return;
    }
    float fy[2], fx[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) fy[j] = lut[min(min(ly0 + j, D.h - 1 - ly0 - j), D.fw)];
#pragma unroll
    for (int k = 0; k < 4; ++k) fx[k] = lut[min(min(lx0 + k, D.w - 1 - lx0 - k), D.fw)];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) w0[j][k] = __builtin_fminf(fy[j], fx[k]);
}

// interior visit of the weighted average: every global load of the visit is issued before the first use, then
// straight-line arithmetic
template <int DT, int CN>
__device__ __forceinline__ void gather_tile_fast(const FinalDesc &D, const float *__restrict__ luts, int lx0, int ly0,
                                                 float (&acc)[2][4][CN], float (&wacc)[2][4])
{
    // ---- loads of the level-0 pixels and the weights ------------------------------------------------------
    float g0[2][4][CN];
    u3_t qs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const char *srow = (const char *)D.src + (size_t)(ly0 + j) * D.stride;
        if (DT == SRC_U8 && CN == 3) {
            qs[j] = ld_u3_a1_g(srow + (size_t)lx0 * 3);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    if (DT == SRC_U8) g0[j][k][c] = (float)((const unsigned char *)srow)[(lx0 + k) * CN + c];
                    else g0[j][k][c] = ((const float *)srow)[(lx0 + k) * CN + c];
                }
        }
    }
    float w0[2][4];
    tile_weights_interior(D, luts, lx0, ly0, w0);
    // u8 RGB: the pixels stay packed (6 dwords) and each plane's eight values are pulled out when that plane is
    // processed (v_cvt_f32_ubyteN, one instruction per value either way): 18 fewer live registers than unpacking up front
    constexpr bool LAZY = (DT == SRC_U8 && CN == 3);
    auto px = [&](int j, int k, int c) -> float {
        if (LAZY) {
            const int b = 3 * k + c;
            unsigned wd = (b >> 2) == 0 ? qs[j].x : ((b >> 2) == 1 ? qs[j].y : qs[j].z);
            asm volatile("" : "+v"(wd));      // keeps the conversion at its use
            return (float)((wd >> (8 * (b & 3))) & 0xFFu);
        }
        return g0[j][k][c];
    };
#pragma unroll
    for (int c = 0; c < CN; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k][c] += px(j, k, c) * w0[j][k];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) wacc[j][k] += w0[j][k];
}

// any visit of the weighted average: per-pixel validity (tile borders, ragged canvas edges)
template <int DT, int CN>
__device__ __forceinline__ void gather_tile_generic(const FinalDesc &D, const float *__restrict__ luts, int lx0, int ly0,
                                                    unsigned valid, float (&acc)[2][4][CN], float (&wacc)[2][4])
{
    float w0[2][4];
    tile_weights(D, luts, lx0, ly0, w0);
#pragma unroll
    for (int c = 0; c < CN; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(valid & (1u << (j * 4 + k)))) continue;
                const char *srow = (const char *)D.src + (size_t)(ly0 + j) * D.stride;
                float g0;
                if (DT == SRC_U8) g0 = (float)((const unsigned char *)srow)[(lx0 + k) * CN + c];
                else g0 = ((const float *)srow)[(lx0 + k) * CN + c];
                acc[j][k][c] += g0 * w0[j][k];
            }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (valid & (1u << (j * 4 + k))) wacc[j][k] += w0[j][k];
}

// up_block_interior<false, YO> in packed fp32: the thread's 4 x 2 patch from rows r0 .. r0 + 2,
// columns c0 .. c0 + 3 of a planar level.  Pairs run over the columns of equal phase, (k0, k2) and (k1, k3): with
// A = the four taps and B = the two taps one column to the right (c0 is odd, so B is an aligned 8-byte load and A's halves
// are aligned register pairs) the horizontal pass is  (h0, h2) = (A01 + B01 * 6) + A23,  (h1, h3) = B01 + A23  -- the
// same operands in the same order as the scalar form, two results per instruction.  24 packed instead of 48 scalar.
template <bool YO>
__device__ __forceinline__ void up_block_interior_pk(const float *__restrict__ plane, int ps, int r0, int c0, float (&u)[2][4])
{
    f2_t h02[3], h13[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float *row = plane + (size_t)(r0 + r) * ps + c0;
        const f4_t a = ld_f4_a4(row);
        const f2_t b01 = *(const f2_a8_t *)(row + 1);
        f2_t a01, a23;
        a01.x = a.x; a01.y = a.y; a23.x = a.z; a23.y = a.w;
        h02[r] = (a01 + b01 * 6.0f) + a23;
        h13[r] = b01 + a23;
    }
    // columns k0, k2 are the even pyrUp phase (1/64 even rows, 1/16 odd rows), k1, k3 the odd one (1/16, 1/4)
    // (YO: the patch starts on an odd row, whose two taps are rows 0 and 1; the even row follows)
    const f2_t ev02 = ((h02[0] + h02[1] * 6.0f) + h02[2]) * (1.0f / 64.0f);
    const f2_t ev13 = ((h13[0] + h13[1] * 6.0f) + h13[2]) * (1.0f / 16.0f);
    const f2_t od02 = (YO ? (h02[0] + h02[1]) : (h02[1] + h02[2])) * (1.0f / 16.0f);
    const f2_t od13 = (YO ? (h13[0] + h13[1]) : (h13[1] + h13[2])) * (1.0f / 4.0f);
    constexpr int E = YO ? 1 : 0, O = YO ? 0 : 1;
    u[E][0] = ev02.x; u[E][2] = ev02.y; u[E][1] = ev13.x; u[E][3] = ev13.y;
    u[O][0] = od02.x; u[O][2] = od02.y; u[O][1] = od13.x; u[O][3] = od13.y;
}

// R_i for one level of every tile, register-blocked: one thread = 4 x 2 pixels of level i, all planes.
// Tile-local x0 is a multiple of 4 (so the pyrUp column phase is fixed: XO = false); the row phase follows
// the parity of the row-window start and is uniform per tile.  Same expressions as k_up_level.
template <int CN, bool YO>
__device__ __forceinline__ void up_level_thread(const TileDev &T, int lvl, float *__restrict__ arena, int x0, int y0,
                                                int ny)
{
    const int h = T.H[lvl], p = T.P[lvl];
    const size_t plane = (size_t)h * p;
    const int hs = T.H[lvl + 1], ws = T.W[lvl + 1], ps = T.P[lvl + 1];
    const size_t splane = (size_t)hs * ps;
    const int r0 = (y0 - 1) >> 1, c0 = (x0 - 1) >> 1;
    const bool interior = c0 >= 0 && c0 + 3 <= ws - 1 && r0 >= 0 && r0 + 2 <= hs - 1;
    const bool two = ny > 1;
    const float *wrow = arena + T.w_off[lvl] + (size_t)y0 * p + x0;
    const f4_t w0v = ld_f4(wrow);
    const f4_t w1v = two ? ld_f4(wrow + p) : w0v;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const float *g = arena + T.g_off[lvl] + c * plane + (size_t)y0 * p + x0;
        float *r = arena + T.r_off[lvl] + c * plane + (size_t)y0 * p + x0;
        const f4_t g0v = ld_f4(g);
        const f4_t g1v = two ? ld_f4(g + p) : g0v;
        float ug[2][4], ur[2][4];
        const float *gs = arena + T.g_off[lvl + 1] + c * splane;
        const float *rs = arena + T.r_off[lvl + 1] + c * splane;
        if (interior) {
            up_block_interior_pk<YO>(gs, ps, r0, c0, ug);
            up_block_interior_pk<YO>(rs, ps, r0, c0, ur);
        } else {
            up_block<false, YO>(gs, hs, ws, ps, r0, c0, ug);
            up_block<false, YO>(rs, hs, ws, ps, r0, c0, ur);
        }
        f4_t o0, o1;
        o0.x = ur[0][0] + (g0v.x - ug[0][0]) * w0v.x;
        o0.y = ur[0][1] + (g0v.y - ug[0][1]) * w0v.y;
        o0.z = ur[0][2] + (g0v.z - ug[0][2]) * w0v.z;
        o0.w = ur[0][3] + (g0v.w - ug[0][3]) * w0v.w;
        o1.x = ur[1][0] + (g1v.x - ug[1][0]) * w1v.x;
        o1.y = ur[1][1] + (g1v.y - ug[1][1]) * w1v.y;
        o1.z = ur[1][2] + (g1v.z - ug[1][2]) * w1v.z;
        o1.w = ur[1][3] + (g1v.w - ug[1][3]) * w1v.w;
        st_f4(r, o0);                  // columns >= w land in the row padding (pitch is a multiple of 16)
        if (two) st_f4(r + p, o1);
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_up_level_blk(const TileDev *__restrict__ tiles, int lvl, float *__restrict__ arena)
{
    const TileDev &T = tiles[blockIdx.z];
    if (lvl >= T.nl) return;
    const int w = T.W[lvl], h = T.H[lvl], p = T.P[lvl];
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y0 = T.r0[lvl] + (blockIdx.y * 4 + threadIdx.y) * 2;
    if (x0 >= w || y0 >= T.r1[lvl]) return;
    const int ny = min(2, T.r1[lvl] - y0);
    if (lvl == T.nl - 1) {
        const size_t plane = (size_t)h * p;
        for (int j = 0; j < ny; ++j) {
            const f4_t wv = ld_f4(arena + T.w_off[lvl] + (size_t)(y0 + j) * p + x0);
#pragma unroll
            for (int c = 0; c < CN; ++c) {
                const f4_t gv = ld_f4(arena + T.g_off[lvl] + c * plane + (size_t)(y0 + j) * p + x0);
                st_f4(arena + T.r_off[lvl] + c * plane + (size_t)(y0 + j) * p + x0, gv * wv);
            }
        }
        return;
    }
    if (y0 & 1) up_level_thread<CN, true>(T, lvl, arena, x0, y0, ny);
    else up_level_thread<CN, false>(T, lvl, arena, x0, y0, ny);
}

// normalise, clip, truncate and store the thread's pixels
template <int CN, int NR = 2>
__device__ __forceinline__ void store_pixels(float (&acc)[NR][4][CN], const float (&wacc)[NR][4],
                                             unsigned char *__restrict__ canvas, long long cstride,
                                             float *__restrict__ canvas_f32, int cw, int x0, int y0, int nx, int ny)
{
    const bool vec_ok = (CN == 3) && nx == 4 && ((cstride & 3) == 0) && ((((size_t)canvas) & 3) == 0);
    // x / 1.0f == x: where every pixel of the wave has sum-of-weights exactly 1 (single coverage beyond the
    // feather zone, about half of a grid canvas) the divisions are skipped -- wave-uniform branch
    bool ones = true;
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) ones = ones && (wacc[j][k] == 1.0f);
    if (__all(ones) == 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) div_shared<CN>(acc[j][k], __builtin_fmaxf(wacc[j][k], 1e-6f), acc[j][k]);
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j >= ny) continue;
        unsigned ob[4 * CN];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < CN; ++c) {
                const float v = acc[j][k][c];
                if (canvas_f32 && k < nx) canvas_f32[((size_t)(y0 + j) * cw + x0 + k) * CN + c] = v;
                ob[k * CN + c] = (unsigned)__builtin_amdgcn_fmed3f(v, 0.0f, 255.0f);     // clip, then truncate
            }
        }
        unsigned char *o = canvas + (size_t)(y0 + j) * cstride + (size_t)x0 * CN;
        if (vec_ok) {
            unsigned int *o32 = (unsigned int *)o;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                o32[q] = ob[4 * q] | (ob[4 * q + 1] << 8) | (ob[4 * q + 2] << 16) | (ob[4 * q + 3] << 24);
        } else {
            for (int k = 0; k < nx; ++k)
#pragma unroll
                for (int c = 0; c < CN; ++c) o[k * CN + c] = (unsigned char)ob[k * CN + c];
        }
    }
}

// Candidate tiles of a 256 x 8 pixel block come from a table built on the host when the plan is made (the tile
// arrangement is fixed per plan): cand_off[blk] .. cand_off[blk + 1] index cand_idx, tiles in list order.  Block
// id, list entries and the 80-byte descriptors are wave-uniform, so they travel through the scalar cache into
// SGPRs: no LDS staging and no barrier before the first vector load.

// Weighted average, border part: the cells the interior part leaves out (a border visit).  Runs over the blocks of the
// edge work list built on the host when the plan is made: 256 x 8 pixel blocks along horizontal tile edges (shape 0),
// 16 x 128 pixel blocks along vertical ones (shape 1).  These are the leading blocks of k_final_fast's launch (the
// slow, divergent ones are scheduled first, the kernel's tail is made of regular blocks).
template <int DT, int CN>
__device__ __forceinline__ void final_edge_block(const FinalDesc *__restrict__ descs, const int4 *__restrict__ edge_blocks,
                                                 int ebi, const int *__restrict__ cand_idx, const float *__restrict__ luts,
                                                 unsigned char *__restrict__ canvas, long long cstride,
                                                 float *__restrict__ canvas_f32, int cw, int row_end)
{
    const int4 eb = edge_blocks[ebi];
    const int c_begin = eb.w, c_end = edge_blocks[ebi + 1].w;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int x0 = eb.x + (eb.z ? (tid & 3) : (tid & 63)) * 4;
    const int y0 = eb.y + (eb.z ? (tid >> 2) : (tid >> 6)) * 2;
    if (x0 >= cw || y0 >= row_end) return;
    const int nx = min(4, cw - x0), ny = min(2, row_end - y0);
    bool edge = false;
    for (int i = c_begin; i < c_end; ++i) {
        const FinalDesc &D = descs[cand_idx[i]];
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        if (lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h) continue;
        if (!visit_is_interior<false>(D, lx0, ly0, nx, ny)) edge = true;
    }
    if (!edge) return;
    float acc[2][4][CN], wacc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wacc[j][k] = 0.f;
#pragma unroll
            for (int c = 0; c < CN; ++c) acc[j][k][c] = 0.f;
        }
    for (int i = c_begin; i < c_end; ++i) {
        const FinalDesc &D = descs[cand_idx[i]];
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        if (lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h) continue;
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j < ny && k < nx && lx0 + k >= 0 && lx0 + k < D.w && ly0 + j >= 0 && ly0 + j < D.h)
                    valid |= 1u << (j * 4 + k);
        gather_tile_generic<DT, CN>(D, luts, lx0, ly0, valid, acc, wacc);
    }
    store_pixels<CN>(acc, wacc, canvas, cstride, canvas_f32, cw, x0, y0, nx, ny);
}

// Weighted average (weighted_average_fusion; the Laplacian blend of 1- and 3-channel tiles is the fused gather below).
// The first n_edge blocks of the (one-dimensional) grid work through the edge list (above); the others are the regular
// FIN_BW x FIN_BH pixel blocks: threads all of whose tile visits are interior compute here, threads with any border
// visit leave their pixels to the edge blocks.
#ifndef SR_FINAL_WAVES
#define SR_FINAL_WAVES 3
#endif
// (the regular block FIN_BW x FIN_BH of FIN_TX x FIN_TY threads: sr_blend_tables.h)
template <int DT, int CN>
__global__ __launch_bounds__(256, SR_FINAL_WAVES) void k_final_fast(const FinalDesc *__restrict__ descs,
                                                       const int *__restrict__ cand_off, const int *__restrict__ cand_idx,
                                                       const int4 *__restrict__ edge_blocks, const int *__restrict__ edge_cand,
                                                       int n_edge, int nbx_r, const float *__restrict__ luts,
                                                       unsigned char *__restrict__ canvas, long long cstride,
                                                       float *__restrict__ canvas_f32, int cw, int row_begin, int row_end)
{
    if ((int)blockIdx.x < n_edge) {
        final_edge_block<DT, CN>(descs, edge_blocks, (int)blockIdx.x, edge_cand, luts, canvas, cstride, canvas_f32, cw, row_end);
        return;
    }
    // regular blocks: FIN_BW x FIN_BH canvas pixels, FIN_TX x FIN_TY threads of 4 x 2 pixels (a wave covers
    // 64 / FIN_TX thread rows)
    const int blk = (int)blockIdx.x - n_edge;
    const int by = blk / nbx_r, bx = blk - by * nbx_r;
    const int c_begin = cand_off[blk], c_end = cand_off[blk + 1];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int x0 = (bx * FIN_TX + (tid % FIN_TX)) * 4;
    const int y0 = row_begin + (by * FIN_TY + tid / FIN_TX) * 2;
    if (x0 >= cw || y0 >= row_end) return;
    const int nx = min(4, cw - x0), ny = min(2, row_end - y0);
    float acc[2][4][CN], wacc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wacc[j][k] = 0.f;
#pragma unroll
            for (int c = 0; c < CN; ++c) acc[j][k][c] = 0.f;
        }
    for (int i = c_begin; i < c_end; ++i) {
        const FinalDesc &D = descs[cand_idx[i]];
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        if (lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h) continue;
        // one border visit sends the whole thread to the edge pass (which recomputes every visit)
        if (!visit_is_interior<false>(D, lx0, ly0, nx, ny)) return;
        gather_tile_fast<DT, CN>(D, luts, lx0, ly0, acc, wacc);
    }
    store_pixels<CN>(acc, wacc, canvas, cstride, canvas_f32, cw, x0, y0, nx, ny);
}

// ---------------------------------------------------------------------------------------------
// Fused final gather: levels 1 -> 0 -> canvas in ONE kernel.  R_1 (the collapsed level 1, reference
// blending_module.py:340-363) is never written to memory: for every (block, covering tile) the block first builds the
// window of R_1 it is about to sample -- each thread one 4 x 2 patch of one plane, exactly the expressions of
// k_up_level_blk, from G_1 / W_1 / G_2 / R_2 -- into LDS together with the G_1 values it was made from, then every
// thread gathers its 4 x 4 canvas pixels from those two LDS windows (blending_module.py:474-506: acc += R_0, wacc += W_0,
// normalise, clip, truncate).  Against k_up_level_blk(level 1) + k_final_fast this drops the R_1 round trip
// (12 B written + 12-18 B re-read per level-1 pixel), one launch, and the 3 x re-read of level-1 rows (a thread's 4 x 4
// pixels share 4 level-1 rows; a block's window is fetched once, coalesced).  Same fp32 expression order everywhere:
// bit-identical to the unfused path.
//   regular block: 128 x 32 canvas pixels, 512 threads of 4 x 2 pixels; level-1 window <= 20 rows x 72 columns per plane
//   edge blocks (cells with a border visit): 256 x 16 or 32 x 128 pixels, generic per-pixel border rules, same windows
// The kernels of this path issue at one VALU instruction per 4 cycles and wave whatever the type, so the lever is the
// instruction count: the two LDS windows are interleaved per pixel and every pyrUp step runs on (g, r) pairs in v_pk_*.
// ---------------------------------------------------------------------------------------------
// (FU_THREADS, the block shapes FU_* and the LDS plane FU_PLANE: sr_blend_tables.h -- the planner cuts its work lists by them)
#ifndef FU_WAVES
#define FU_WAVES 4           /* waves per SIMD the register allocation is held to */
#endif

// The level-1 window (tile coordinates) a block of bw x bh canvas pixels at tile-local (lxa, lya) samples: rows R0 ..,
// columns C0 .. in patches of 2 rows x 4 columns (R0 even, C0 a multiple of 4: the alignment k_up_level_blk's threads have).
__device__ __forceinline__ bool fused_window(const FinalDesc &D, int lxa, int lya, int bw, int bh, int &R0, int &C0, int &npr, int &npc)
{
    const int c_lo = max((lxa - 1) >> 1, 0), r_lo = max((lya - 1) >> 1, 0);
    const int c_hi = min(((lxa + bw - 5) >> 1) + 3, D.W1 - 1), r_hi = min(((lya + bh - 3) >> 1) + 2, D.H1 - 1);
    C0 = c_lo & ~3;
    R0 = r_lo & ~1;
    if (c_hi < C0 || r_hi < R0) return false;
    npc = (c_hi - C0) / 4 + 1;
    npr = (r_hi - R0) / 2 + 1;
    return true;
}

// Stage 1: R_1 and G_1 of the window into LDS, interleaved per pixel as (g, r) pairs: lds[plane][row][col][2] -- stage 2
// then reads a pixel's two values as one aligned 8-byte pair and runs the pyrUp of both arrays in packed fp32 (v_pk_*,
// IEEE per element: same roundings as the scalar form).  One item = one 4 x 2 patch of one plane = up_level_thread's work.
template <int CN, int G1F>
__device__ __forceinline__ void fused_stage1(const FinalDesc &D, const float *__restrict__ arena, float *lds, int R0, int C0,
                                             int npr, int npc, int LP, int tid)
{
    const int per_plane = npr * npc, n_items = per_plane * CN;
    const size_t plane1 = (size_t)D.H1 * D.P1, plane2 = (size_t)D.H2 * D.P2;
    // item -> (plane, patch row, patch column) with multiply-shift divisions (x < 1024, divisor d <= 256, m = ceil(2^20 / d):
    // exact because x * (m * d - 2^20) < 1024 * 256 < 2^20)
    const unsigned m_pp = ((1u << 20) + per_plane - 1) / per_plane, m_pc = ((1u << 20) + npc - 1) / npc;
    for (int item = tid; item < n_items; item += FU_THREADS) {
        const int c = (int)(((unsigned)item * m_pp) >> 20), rem = item - c * per_plane;
        const int pr = (int)(((unsigned)rem * m_pc) >> 20), pc = rem - pr * npc;
        const int px = C0 + 4 * pc, py = R0 + 2 * pr;
        if (px >= D.W1 || py >= D.H1) continue;
        // every load of the item is issued before the first use (no branch between them: a conditional second row would
        // put a full memory round trip between the two halves); a patch on the last odd row re-reads its own row
        const int row1 = (py + 1 < D.H1) ? D.P1 : 0;
        const size_t gi = c * plane1 + (size_t)py * D.P1 + px;
        const float *wr = arena + D.w1 + (size_t)py * D.P1 + px;
        const f4_t g0v = G1<G1F>::quad(arena + D.g1, gi), g1v = G1<G1F>::quad(arena + D.g1, gi + row1);
        const f4_t w0v = ld_f4(wr), w1v = ld_f4(wr + row1);
        f4_t o0, o1;
        if (D.nl == 2) {                         // level 1 is the top of this tile's pyramid: R = G * W
            o0 = g0v * w0v;
            o1 = g1v * w1v;
        } else {
            const int r0 = (py - 1) >> 1, c0 = (px - 1) >> 1;
            const bool interior = c0 >= 0 && c0 + 3 <= D.W2 - 1 && r0 >= 0 && r0 + 2 <= D.H2 - 1;
            const float *gs = arena + D.g2 + c * plane2, *rs = arena + D.r2 + c * plane2;
            float ug[2][4], ur[2][4];
            if (interior) {
                up_block_interior_pk<false>(gs, D.P2, r0, c0, ug);
                up_block_interior_pk<false>(rs, D.P2, r0, c0, ur);
            } else {
                up_block<false, false>(gs, D.H2, D.W2, D.P2, r0, c0, ug);
                up_block<false, false>(rs, D.H2, D.W2, D.P2, r0, c0, ur);
            }
            o0.x = ur[0][0] + (g0v.x - ug[0][0]) * w0v.x;
            o0.y = ur[0][1] + (g0v.y - ug[0][1]) * w0v.y;
            o0.z = ur[0][2] + (g0v.z - ug[0][2]) * w0v.z;
            o0.w = ur[0][3] + (g0v.w - ug[0][3]) * w0v.w;
            o1.x = ur[1][0] + (g1v.x - ug[1][0]) * w1v.x;
            o1.y = ur[1][1] + (g1v.y - ug[1][1]) * w1v.y;
            o1.z = ur[1][2] + (g1v.z - ug[1][2]) * w1v.z;
            o1.w = ur[1][3] + (g1v.w - ug[1][3]) * w1v.w;
        }
        // (g, r) pairs, 32 contiguous bytes per patch row: 16-byte stores (dword stores at a 32-byte lane stride would hit
        // every LDS bank eight times)
        float *d0 = lds + c * (2 * FU_PLANE) + ((pr * 2) * LP + pc * 4) * 2;
        float *d1 = d0 + 2 * LP;
        f4_t s0, s1, s2, s3;
        s0.x = g0v.x; s0.y = o0.x; s0.z = g0v.y; s0.w = o0.y; s1.x = g0v.z; s1.y = o0.z; s1.z = g0v.w; s1.w = o0.w;
        s2.x = g1v.x; s2.y = o1.x; s2.z = g1v.y; s2.w = o1.y; s3.x = g1v.z; s3.y = o1.z; s3.z = g1v.w; s3.w = o1.w;
        st_f4(d0, s0);
        st_f4(d0 + 4, s1);
        st_f4(d1, s2);
        st_f4(d1 + 4, s3);
    }
}

// pyrUp of a 3-row x 4-column neighbourhood of (g, r) PAIRS -> the thread's 4 x 2 pixels, both arrays at once in packed
// fp32 (interior form).  q[r][i] is the pair at row r0 + r, column c0 + i.  Scaling by a power of two commutes with fp32
// rounding, so the x4 of the odd phases ((a + b) * 4) is not applied where the reference applies it but folded into the
// final constant: 1/64 (even,even), 1/16 (one odd phase), 1/4 (odd,odd).  Bit-identical to the reference order.
template <bool XO, bool YO>
__device__ __forceinline__ void up_pairs(const f2_t (&q)[3][4], f2_t (&u)[2][4])
{
    f2_t h[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (!XO) {
            h[r][0] = (q[r][0] + q[r][1] * 6.0f) + q[r][2];
            h[r][1] = q[r][1] + q[r][2];
            h[r][2] = (q[r][1] + q[r][2] * 6.0f) + q[r][3];
            h[r][3] = q[r][2] + q[r][3];
        } else {
            h[r][0] = q[r][0] + q[r][1];
            h[r][1] = (q[r][0] + q[r][1] * 6.0f) + q[r][2];
            h[r][2] = q[r][1] + q[r][2];
            h[r][3] = (q[r][1] + q[r][2] * 6.0f) + q[r][3];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool kodd = XO ? ((k & 1) == 0) : ((k & 1) == 1);
        const float ce = kodd ? (1.0f / 16.0f) : (1.0f / 64.0f);
        const float co = kodd ? (1.0f / 4.0f) : (1.0f / 16.0f);
        const f2_t ev = ((h[0][k] + h[1][k] * 6.0f) + h[2][k]) * ce;
        if (!YO) {
            u[0][k] = ev;
            u[1][k] = (h[1][k] + h[2][k]) * co;
        } else {
            u[0][k] = (h[0][k] + h[1][k]) * co;
            u[1][k] = ev;
        }
    }
}

// Stage 2, interior visit of a regular block: the thread's 4 x 2 pixels from the LDS window (pitch FU_LP pairs).  CODD: the
// first tap column is odd -- its 32 bytes per row are then 8-byte aligned only and read as 8 + 16 + 8.
// the level-0 pixels of an interior 4 x 2 visit: requested BEFORE the block's stage 1 so they arrive under it
template <int DT, int CN>
struct CellPixels {
    float g0[(DT == SRC_U8 && CN == 3) ? 1 : 2][(DT == SRC_U8 && CN == 3) ? 1 : 4][CN];
    u3_t qs[2];
};

template <int DT, int CN>
__device__ __forceinline__ void fused_load_pixels(const FinalDesc &D, int lx0, int ly0, CellPixels<DT, CN> &px)
{
    constexpr bool LAZY = (DT == SRC_U8 && CN == 3);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const char *srow = (const char *)D.src + (size_t)(ly0 + j) * D.stride;
        if (LAZY) {
            px.qs[j] = ld_u3_a1_g(srow + (size_t)lx0 * 3);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    if (DT == SRC_U8) px.g0[j][k][c] = (float)((const unsigned char *)srow)[(lx0 + k) * CN + c];
                    else px.g0[j][k][c] = ((const float *)srow)[(lx0 + k) * CN + c];
                }
        }
    }
}

template <int DT, int CN, bool XO, bool YO, bool CODD>
__device__ __forceinline__ void fused_gather_fast(const FinalDesc &D, const float *__restrict__ luts, const float *lds, int LP, int R0,
                                                  int C0, int lx0, int ly0, const CellPixels<DT, CN> &cp, float (&acc)[2][4][CN],
                                                  float (&wacc)[2][4])
{
    const bool pyr = D.nl > 1;
    constexpr bool LAZY = (DT == SRC_U8 && CN == 3);
    float w0[2][4];
    tile_weights_interior(D, luts, lx0, ly0, w0);
    auto px = [&](int j, int k, int c) -> float {
        if (LAZY) {
            const int b = 3 * k + c;
            unsigned wd = (b >> 2) == 0 ? cp.qs[j].x : ((b >> 2) == 1 ? cp.qs[j].y : cp.qs[j].z);
            asm volatile("" : "+v"(wd));      // keeps the conversion at its use (see gather_tile_fast)
            return (float)((wd >> (8 * (b & 3))) & 0xFFu);
        }
        return cp.g0[LAZY ? 0 : j][LAZY ? 0 : k][c];
    };
    // beyond the feather width every weight of the cell is lut[fw]; where that is exactly 1 (linear and cosine ramps)
    // for the whole wave, lap * w == lap and the multiplies are skipped -- wave-uniform branch, bit-identical
    const bool flat = min(min(ly0, D.h - 2 - ly0), min(lx0, D.w - 4 - lx0)) >= D.fw && luts[D.lut_off + D.fw] == 1.0f;
    const bool unit_w = __all(flat) != 0;
    if (pyr) {
        const int r0 = (ly0 - 1) >> 1, c0 = (lx0 - 1) >> 1;
        // (g, r) pairs of rows r0 .. r0 + 2, columns c0 .. c0 + 3: 32 contiguous bytes per row
        const float *base = lds + ((r0 - R0) * LP + (c0 - C0)) * 2;
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            const float *p = base + c * (2 * FU_PLANE);
            f2_t q[3][4], u[2][4];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float *pr = p + r * (2 * LP);
                if (!CODD) {
                    const f4_t a = *(const f4_t *)pr, b = *(const f4_t *)(pr + 4);
                    q[r][0].x = a.x; q[r][0].y = a.y; q[r][1].x = a.z; q[r][1].y = a.w;
                    q[r][2].x = b.x; q[r][2].y = b.y; q[r][3].x = b.z; q[r][3].y = b.w;
                } else {
                    const f2_t a = *(const f2_t *)pr, d = *(const f2_t *)(pr + 6);
                    const f4_t b = *(const f4_t *)(pr + 2);
                    q[r][0] = a; q[r][1].x = b.x; q[r][1].y = b.y; q[r][2].x = b.z; q[r][2].y = b.w; q[r][3] = d;
                }
            }
            up_pairs<XO, YO>(q, u);
            if (unit_w) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float lap = px(j, k, c) - u[j][k].x;
                        acc[j][k][c] += u[j][k].y + lap;
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float lap = px(j, k, c) - u[j][k].x;
                        const float wl = lap * w0[j][k];
                        acc[j][k][c] += u[j][k].y + wl;
                    }
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < CN; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][k][c] += px(j, k, c) * w0[j][k];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) wacc[j][k] += w0[j][k];
}

// up_block over an LDS window: same clamps and border rules, the window's origin subtracted from the clamped indices
template <bool XO, bool YO>
__device__ __forceinline__ void up_block_win(const float *win, int hs, int ws, int LP, int R0, int C0, int r0, int c0, float (&u)[2][4])
{
    float v[3][4], h[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ro = (min(max(r0 + r, 0), hs - 1) - R0) * LP - C0;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = win[(ro + min(max(c0 + c, 0), ws - 1)) * 2];      // (g, r) pairs: stride 2
    }
    up_rows4<XO>(v, ws, c0, h);
    up_cols2<YO>(h, r0, u);
}

// any 4 x 2 visit from the LDS windows (gather_tile_generic with G_1 / R_1 in LDS)
template <int DT, int CN, bool XO, bool YO>
__device__ __forceinline__ void fused_gather_generic(const FinalDesc &D, const float *__restrict__ luts, const float *lds, int LP,
                                                     int R0, int C0, int lx0, int ly0, unsigned valid, float (&acc)[2][4][CN],
                                                     float (&wacc)[2][4])
{
    float w0[2][4];
    tile_weights(D, luts, lx0, ly0, w0);
    const int r0 = (ly0 - 1) >> 1, c0 = (lx0 - 1) >> 1;
    const bool pyr = D.nl > 1;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        float ug[2][4], ur[2][4];
        if (pyr) {
            up_block_win<XO, YO>(lds + c * (2 * FU_PLANE), D.H1, D.W1, LP, R0, C0, r0, c0, ug);
            up_block_win<XO, YO>(lds + c * (2 * FU_PLANE) + 1, D.H1, D.W1, LP, R0, C0, r0, c0, ur);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(valid & (1u << (j * 4 + k)))) continue;
                const char *srow = (const char *)D.src + (size_t)(ly0 + j) * D.stride;
                float g0;
                if (DT == SRC_U8) g0 = (float)((const unsigned char *)srow)[(lx0 + k) * CN + c];
                else g0 = ((const float *)srow)[(lx0 + k) * CN + c];
                float r;
                if (pyr) {
                    const float lap = g0 - ug[j][k];
                    const float wl = lap * w0[j][k];
                    r = ur[j][k] + wl;
                } else {
                    r = g0 * w0[j][k];
                }
                acc[j][k][c] += r;
            }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (valid & (1u << (j * 4 + k))) wacc[j][k] += w0[j][k];
}

// Edge blocks of the fused gather: the 4 x 2 cells with a border visit, generic per-pixel rules from the LDS window.
template <int DT, int CN, int G1F>
__device__ __forceinline__ void fused_edge_block(const FinalDesc *__restrict__ descs, const int4 *__restrict__ edge_blocks, int ebi,
                                                 const int *__restrict__ cand_idx, const float *__restrict__ arena,
                                                 const float *__restrict__ luts, float *lds, unsigned char *__restrict__ canvas,
                                                 long long cstride, float *__restrict__ canvas_f32, int cw, int row_begin, int row_end)
{
    const int4 eb = edge_blocks[ebi];
    const int c_begin = eb.w, c_end = edge_blocks[ebi + 1].w;
    const int tid = threadIdx.x;
    const int shape = eb.z;                                   // 0: 256 x FU_E0H px (64 cells across), 1: FU_E1W x FU_E1H px (4 across)
    const int bw = shape ? FU_E1W : 256, bh = shape ? FU_E1H : FU_E0H, LP = shape ? FU_E1LP : 136;
    const int x0 = eb.x + (shape ? (tid & 3) : (tid & 63)) * 4;
    const int y0 = eb.y + (shape ? (tid >> 2) : (tid >> 6)) * 2;
    const bool inside = x0 < cw && y0 < row_end;
    const int nx = min(4, cw - x0), ny = min(2, row_end - y0);
    bool edge = false;
    if (inside)
        for (int i = c_begin; i < c_end; ++i) {
            const FinalDesc &D = descs[cand_idx[i]];
            const int lx0 = x0 - D.x, ly0 = y0 - D.y;
            if (lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h) continue;
            if (!visit_is_interior<true>(D, lx0, ly0, nx, ny)) edge = true;
        }
    float acc[2][4][CN], wacc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wacc[j][k] = 0.f;
#pragma unroll
            for (int c = 0; c < CN; ++c) acc[j][k][c] = 0.f;
        }
    for (int i = c_begin; i < c_end; ++i) {
        const FinalDesc &D = descs[cand_idx[i]];
        int R0 = 0, C0 = 0, npr = 0, npc = 0;
        const bool win = D.nl > 1 && fused_window(D, eb.x - D.x, eb.y - D.y, bw, bh, R0, C0, npr, npc);
        if (win) fused_stage1<CN, G1F>(D, arena, lds, R0, C0, npr, npc, LP, tid);
        __syncthreads();
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        const bool touches = edge && !(lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h);
        // An edge cell has a border visit of SOME tile; its visits of the other tiles are mostly interior ones (the cell
        // lies on tile A's edge and well inside tile B): those take the regular blocks' packed path (same arithmetic, same
        // results), only the border visits pay for the per-pixel border rules.  Along a tile edge the split is uniform per
        // tile, so a wave rarely runs both.
        const bool inner = DT == SRC_U8 && touches && visit_is_interior<true>(D, lx0, ly0, nx, ny);    // (float tiles: generic path only)
        if constexpr (DT == SRC_U8) if (inner) {
            CellPixels<DT, CN> cp;
            fused_load_pixels<DT, CN>(D, lx0, ly0, cp);
            const bool xo = (D.x & 1) != 0;
            const bool yo = ((row_begin - D.y) & 1) != 0;
            const bool codd = D.nl > 1 && (((((eb.x - D.x) - 1) >> 1) - C0) & 1) != 0;
#define FE_CALL(XOV, YOV, CV) fused_gather_fast<DT, CN, XOV, YOV, CV>(D, luts, lds, LP, R0, C0, lx0, ly0, cp, acc, wacc)
            if (!codd) {
                if (!xo && !yo) FE_CALL(false, false, false);
                else if (xo && !yo) FE_CALL(true, false, false);
                else if (!xo && yo) FE_CALL(false, true, false);
                else FE_CALL(true, true, false);
            } else {
                if (!xo && !yo) FE_CALL(false, false, true);
                else if (xo && !yo) FE_CALL(true, false, true);
                else if (!xo && yo) FE_CALL(false, true, true);
                else FE_CALL(true, true, true);
            }
#undef FE_CALL
        }
        if (touches && !inner) {
            unsigned valid = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j < ny && k < nx && lx0 + k >= 0 && lx0 + k < D.w && ly0 + j >= 0 && ly0 + j < D.h)
                        valid |= 1u << (j * 4 + k);
            const bool xo = (D.x & 1) != 0;
            const bool yo = ((row_begin - D.y) & 1) != 0;
            if (!xo && !yo) fused_gather_generic<DT, CN, false, false>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else if (xo && !yo) fused_gather_generic<DT, CN, true, false>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else if (!xo && yo) fused_gather_generic<DT, CN, false, true>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else fused_gather_generic<DT, CN, true, true>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
        }
        __syncthreads();                                   // the next tile's stage 1 overwrites the window
    }
    if (edge) store_pixels<CN>(acc, wacc, canvas, cstride, canvas_f32, cw, x0, y0, nx, ny);
}

template <int DT, int CN, int G1F>
__global__ __launch_bounds__(FU_THREADS, FU_WAVES) void k_final_fused(const FinalDesc *__restrict__ descs, const int *__restrict__ cand_off,
                                                        const int *__restrict__ cand_idx, const int4 *__restrict__ edge_blocks,
                                                        const int *__restrict__ edge_cand, int n_edge, int nbx_r,
                                                        const float *__restrict__ arena, const float *__restrict__ luts,
                                                        unsigned char *__restrict__ canvas, long long cstride,
                                                        float *__restrict__ canvas_f32, int cw, int row_begin, int row_end)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * CN * FU_PLANE];
    if ((int)blockIdx.x < n_edge) {
        fused_edge_block<DT, CN, G1F>(descs, edge_blocks, (int)blockIdx.x, edge_cand, arena, luts, lds, canvas, cstride, canvas_f32, cw,
                                 row_begin, row_end);
        return;
    }
    // (Measured and rejected: a workgroup marching down several blocks of a column -- one dispatch, halo rows still in
    // the CU's caches -- is slower, 1.37 -> 1.52 ms at 16 blocks: the blocks of a march run strictly one after the other
    // and each is a chain of dependent memory round trips; independent blocks overlap them.)
    const int blk = (int)blockIdx.x - n_edge;
    const int by = blk / nbx_r, bx = blk - by * nbx_r;
    const int c_begin = cand_off[blk], c_end = cand_off[blk + 1];
    const int tid = threadIdx.x;
    // (the block origin through readfirstlane: without it the float RGB instance spills a VGPR)
    const int sbx = __builtin_amdgcn_readfirstlane(bx * FU_BW), sby = __builtin_amdgcn_readfirstlane(row_begin + by * FU_BH);
    // the block's cells stop at the canvas width and at row_end: the level-1 window is built for the cells in use only,
    // and the threads are dealt over them (the cells of a ragged block fill the first waves) -- block-uniform
    const int scw = min(FU_BW / 4, (cw - sbx + 3) >> 2), sch = min(FU_BH / 2, (row_end - sby + 1) >> 1);
    const int sbw = 4 * scw, sbh = 2 * sch;
    const int scy = tid / scw, scx = tid - scy * scw;
    const int x0 = sbx + scx * 4, y0 = sby + scy * 2;
    const int nx = min(4, cw - x0), ny = min(2, row_end - y0);
    // a cell with any border visit belongs to the edge blocks (which recompute every visit of it): it stops
    // accumulating at its first border visit and stores nothing
    bool alive = scy < sch;
    float acc[2][4][CN], wacc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wacc[j][k] = 0.f;
#pragma unroll
            for (int c = 0; c < CN; ++c) acc[j][k][c] = 0.f;
        }
    for (int i = c_begin; i < c_end; ++i) {
        const FinalDesc &D = descs[cand_idx[i]];
        const int lxa = sbx - D.x, lya = sby - D.y;
        int R0 = 0, C0 = 0, npr = 0, npc = 0;
        const bool win = D.nl > 1 && fused_window(D, lxa, lya, sbw, sbh, R0, C0, npr, npc);        // block-uniform
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        bool visit = alive && !(lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h);
        if (visit && !visit_is_interior<true>(D, lx0, ly0, nx, ny)) visit = alive = false;
        CellPixels<DT, CN> cp;
        if (visit) fused_load_pixels<DT, CN>(D, lx0, ly0, cp);                                     // in flight during stage 1
        if (win) fused_stage1<CN, G1F>(D, arena, lds, R0, C0, npr, npc, FU_LP, tid);
        __syncthreads();
        if (visit) {
            const bool xo = (D.x & 1) != 0;                      // x0 is a multiple of 4
            const bool yo = ((row_begin - D.y) & 1) != 0;        // y0 - row_begin is a multiple of 2
            const bool codd = D.nl > 1 && ((((lxa - 1) >> 1) - C0) & 1) != 0;   // parity of every cell's first tap column (block-uniform)
#define FU_CALL(XOV, YOV, CV) fused_gather_fast<DT, CN, XOV, YOV, CV>(D, luts, lds, FU_LP, R0, C0, lx0, ly0, cp, acc, wacc)
            if (!codd) {
                if (!xo && !yo) FU_CALL(false, false, false);
                else if (xo && !yo) FU_CALL(true, false, false);
                else if (!xo && yo) FU_CALL(false, true, false);
                else FU_CALL(true, true, false);
            } else {
                if (!xo && !yo) FU_CALL(false, false, true);
                else if (xo && !yo) FU_CALL(true, false, true);
                else if (!xo && yo) FU_CALL(false, true, true);
                else FU_CALL(true, true, true);
            }
#undef FU_CALL
        }
        __syncthreads();                                       // the next tile's stage 1 overwrites the window
    }
    if (alive) store_pixels<CN>(acc, wacc, canvas, cstride, canvas_f32, cw, x0, y0, nx, ny);   // ragged cells without a visit: zeros
}

// ---------------------------------------------------------------------------------------------
// Round 4: what the marched zones leave -- thin bands along the tiles' edges, 1.8 % of the cells of the 200 MP grid -- as
// RECTANGLES of cells (k_final_rect).  The 128 x 16 blocks above cut a vertical band 3-5 cells wide into 722 blocks per band
// with 30-40 of their 256 cells in use, and the cells with a border visit were visited a second time by the edge blocks
// (window built twice): 9 192 + 2 700 blocks, 12 rounds of dependent round trips, 0.21 ms for 3.5 MP.  A rectangle item is
// w x h cells with w * h <= 256 and a level-1 window that fits the LDS planes (a band 5 cells wide: 5 x 51 cells, a band 6
// rows high: 32 x 6); every cell of it is finished here, whatever its visits are -- interior visits through the packed
// path, border visits through the per-pixel rules (fused_edge_block's two paths; the same expressions, bit-identical) -- so
// the edge blocks are not launched at all beside a march.  Threads are dealt column-major over tall rectangles: along a
// vertical tile edge the kind of visit is then uniform per wave.
// ---------------------------------------------------------------------------------------------
#ifndef FR_WAVES
#define FR_WAVES FU_WAVES     /* waves per SIMD the register allocation of k_final_rect is held to */
#endif
template <int CN, int G1F>
__global__ __launch_bounds__(FU_THREADS, FR_WAVES) void k_final_rect(const FinalDesc *__restrict__ descs, const RectItem *__restrict__ rects,
                                                        const int *__restrict__ rect_cand, const float *__restrict__ arena,
                                                        const float *__restrict__ luts, unsigned char *__restrict__ canvas,
                                                        long long cstride, float *__restrict__ canvas_f32, int cw, int row_begin,
                                                        int row_end)
{
    constexpr int DT = SRC_U8;
    __shared__ __attribute__((aligned(16))) float lds[2 * CN * FU_PLANE];
    const RectItem it = rects[blockIdx.x];
    const int tid = threadIdx.x;
    int scx, scy;
    if (it.colmajor) {
        scx = tid / it.h;
        scy = tid - scx * it.h;
    } else {
        scy = tid / it.w;
        scx = tid - scy * it.w;
    }
    const int x0 = it.x + 4 * scx, y0 = it.y + 2 * scy;
    const bool inside = scx < it.w && scy < it.h && x0 < cw && y0 < row_end;
    const int nx = min(4, cw - x0), ny = min(2, row_end - y0);
    const int LP = it.lp;
    float acc[2][4][CN], wacc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wacc[j][k] = 0.f;
#pragma unroll
            for (int c = 0; c < CN; ++c) acc[j][k][c] = 0.f;
        }
    for (int i = it.cand; i < it.cand + it.ncand; ++i) {
        const FinalDesc &D = descs[rect_cand[i]];
        const int lxa = it.x - D.x, lya = it.y - D.y;
        int R0 = 0, C0 = 0, npr = 0, npc = 0;
        const bool win = D.nl > 1 && fused_window(D, lxa, lya, 4 * it.w, 2 * it.h, R0, C0, npr, npc);     // block-uniform
        const int lx0 = x0 - D.x, ly0 = y0 - D.y;
        const bool touches = inside && !(lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= D.w || ly0 >= D.h);
        const bool inner = touches && visit_is_interior<true>(D, lx0, ly0, nx, ny);
        CellPixels<DT, CN> cp;
        if (inner) fused_load_pixels<DT, CN>(D, lx0, ly0, cp);                                        // in flight during stage 1
        if (win) fused_stage1<CN, G1F>(D, arena, lds, R0, C0, npr, npc, LP, tid);
        __syncthreads();
        const bool xo = (D.x & 1) != 0;                      // x0 is a multiple of 4
        const bool yo = ((row_begin - D.y) & 1) != 0;        // y0 - row_begin is a multiple of 2
        if (inner) {
            const bool codd = D.nl > 1 && ((((lxa - 1) >> 1) - C0) & 1) != 0;   // parity of every cell's first tap column (block-uniform)
#define FR_CALL(XOV, YOV, CV) fused_gather_fast<DT, CN, XOV, YOV, CV>(D, luts, lds, LP, R0, C0, lx0, ly0, cp, acc, wacc)
            if (!codd) {
                if (!xo && !yo) FR_CALL(false, false, false);
                else if (xo && !yo) FR_CALL(true, false, false);
                else if (!xo && yo) FR_CALL(false, true, false);
                else FR_CALL(true, true, false);
            } else {
                if (!xo && !yo) FR_CALL(false, false, true);
                else if (xo && !yo) FR_CALL(true, false, true);
                else if (!xo && yo) FR_CALL(false, true, true);
                else FR_CALL(true, true, true);
            }
#undef FR_CALL
        }
        if (touches && !inner) {
            unsigned valid = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j < ny && k < nx && lx0 + k >= 0 && lx0 + k < D.w && ly0 + j >= 0 && ly0 + j < D.h)
                        valid |= 1u << (j * 4 + k);
            if (!xo && !yo) fused_gather_generic<DT, CN, false, false>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else if (xo && !yo) fused_gather_generic<DT, CN, true, false>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else if (!xo && yo) fused_gather_generic<DT, CN, false, true>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
            else fused_gather_generic<DT, CN, true, true>(D, luts, lds, LP, R0, C0, lx0, ly0, valid, acc, wacc);
        }
        __syncthreads();                                       // the next tile's stage 1 overwrites the window
    }
    if (inside) store_pixels<CN>(acc, wacc, canvas, cstride, canvas_f32, cw, x0, y0, nx, ny);   // cells without a visit: zeros
}

#include "sr_march.inc"
#include "sr_down2.inc"

// weighted_average_fusion with caller-supplied weight maps (blending_module.py:729-751): thread per canvas pixel
struct CustomW {
    const float *w;      // h x w fp32 weight map of the tile, row stride in bytes
    long long stride;
};
template <int DT>
__global__ __launch_bounds__(256) void k_weighted_custom(const TileDev *__restrict__ tiles, const TileSrc *__restrict__ srcs,
                                                         const CustomW *__restrict__ wts, int n, int cn,
                                                         unsigned char *__restrict__ canvas, long long cstride,
                                                         float *__restrict__ canvas_f32, int cw, int row_begin, int row_end)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = row_begin + blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= row_end) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float wacc = 0.f;
    for (int t = 0; t < n; ++t) {
        const TileDev &T = tiles[t];
        const int lx = x - T.x, ly = y - T.y;
        if (lx < 0 || ly < 0 || lx >= T.w || ly >= T.h) continue;
        const float w0 = ((const float *)((const char *)wts[t].w + (size_t)ly * wts[t].stride))[lx];
        const char *srow = (const char *)srcs[t].p + (size_t)ly * srcs[t].stride;
        for (int c = 0; c < cn; ++c) {
            const float g0 = DT == SRC_U8 ? (float)((const unsigned char *)srow)[lx * cn + c] : ((const float *)srow)[lx * cn + c];
            acc[c] += g0 * w0;
        }
        wacc += w0;
    }
    const float wv = wacc > 1e-6f ? wacc : 1e-6f;
    unsigned char *o = canvas + (size_t)y * cstride + (size_t)x * cn;
    for (int c = 0; c < cn; ++c) {
        const float v = acc[c] / wv;
        if (canvas_f32) canvas_f32[((size_t)y * cw + x) * cn + c] = v;
        const float cl = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        o[c] = (unsigned char)cl;
    }
}

// ---------------------------------------------------------------------------------------------
// blend plan (host object)
// ---------------------------------------------------------------------------------------------
// The planner's tables (sr_blend_tables.h, built by sr_blend_plan.cpp) and where they are on the device: one allocation per
// table -- the gathers read several of them through the scalar cache.
struct sr_blend_plan : BlendTables {
    sr_ctx *ctx = nullptr;
    std::vector<void *> owned;                          // every device allocation below
    float *d_arena = nullptr, *d_luts = nullptr;
    TileDev *d_tiles = nullptr, *d_classes = nullptr;
    TileSrc *d_srcs = nullptr;                          // d_srcs, d_fdesc: written per call
    FinalDesc *d_fdesc = nullptr;
    int4 *d_edge_blocks = nullptr, *d_fedge_blocks = nullptr;       // EdgeBlock lists as the kernels read them
    int *d_edge_cand = nullptr, *d_cand_off = nullptr, *d_cand_idx = nullptr, *d_fedge_cand = nullptr, *d_fcand_off = nullptr, *d_fcand_idx = nullptr, *d_rect_cand = nullptr;
    MarchItem *d_march_items[MARCH_NT + 1] = {nullptr};
    RectItem *d_rects = nullptr;
    bool weights_ready = false;                         // weight pyramids of the classes are in the arena
    std::vector<char> sh_srcs, sh_fdesc;                // host shadows of d_srcs / d_fdesc (upload_if_changed)
    CachedTable subset_tabs[4];                         // compacted {TileDev, TileSrc} tables of recent tile subsets
    int subset_next = 0;
    ~sr_blend_plan()                                    // under the context's Guard
    {
        for (void *p : owned) (void)hipFree(p);
        for (auto &t : subset_tabs) t.buf.release();
    }
};
static_assert(sizeof(int4) == sizeof(EdgeBlock), "the kernels read an EdgeBlock as one int4");

bool plan_describe(const sr_blend_plan *p, sr_ctx **ctx, int *n, int *cn)
{
    if (!plan_is_live(p)) return false;
    if (ctx) *ctx = p->ctx;
    if (n) *n = p->n;
    if (cn) *cn = p->cn;
    return true;
}

// The environment switches of a plan: read per plan (the tests flip them between plans), and nowhere else.
static BlendSwitches switches_from_env()
{
    auto is = [](const char *name, char c) { const char *e = std::getenv(name); return e && e[0] == c; };
    BlendSwitches sw;
    sw.march = !is("SR_MARCH", '0');                  // SR_MARCH=0: every zone through k_final_fused (A/B runs)
    sw.march_force = is("SR_MARCH", '2');             // SR_MARCH=2: marches whatever the size
    sw.down2 = !is("SR_DOWN2", '0');                  // SR_DOWN2=0: levels 1 and 2 in two launches
    sw.g1_u16 = !is("SR_G1_U16", '0');                // SR_G1_U16=0: G_1 in fp32
    const char *e_tail = std::getenv("SR_MARCH_TAIL"), *e_rounds = std::getenv("SR_MARCH_ROUNDS"), *e_cells = std::getenv("SR_RECT_CELLS");
    sw.march_taper = !(e_tail && atoi(e_tail) == 0);  // SR_MARCH_TAIL=0: uniform segments (A/B runs)
    sw.stats = std::getenv("SR_MARCH_STATS") != nullptr;
    if (e_rounds) {                                   // SR_MARCH_ROUNDS="r1,r2,r4": the last value given holds for the lists after it
        double r[3] = {0, 0, 0};
        const int got = sscanf(e_rounds, "%lf,%lf,%lf", &r[0], &r[1], &r[2]);
        for (int k = 0; k < 3 && got >= 1; ++k) sw.march_rounds[k] = std::max(r[std::min(k, got - 1)], 0.0);
    }
    if (e_cells && atoi(e_cells) >= 32) sw.rect_cells = std::min(atoi(e_cells), 256);      // A/B runs: most cells per rectangle
    return sw;
}

extern "C" {

// ---- blend plan ------------------------------------------------------------------------------------
static std::vector<sr_blend_plan *> plans_of(sr_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_reg_mu);
    std::vector<sr_blend_plan *> out;
    for (const void *p : g_live_plan)
        if (((const sr_blend_plan *)p)->ctx == ctx) out.push_back((sr_blend_plan *)p);
    return out;
}

int sr_blend_plan_destroy(sr_blend_plan *plan)
{
    if (!plan) return SR_OK;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        if (!g_live_plan.erase(plan)) return SR_OK;          // already destroyed (with its context)
    }
    Guard g(plan->ctx);
    (void)hipStreamSynchronize(plan->ctx->stream);
    delete plan;
    return SR_OK;
}

int sr_blend_plan_create(sr_ctx *ctx, const sr_tile_rect *h_tiles, int n, int cn, int canvas_h, int canvas_w,
                         int levels, int weight_type, int row_begin, int row_end, sr_blend_plan **out)
{
    CTX_ENTER(ctx);
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: null out");
    *out = nullptr;
    row_begin = std::max(row_begin, 0);
    row_end = std::min(row_end, canvas_h);
    if (row_begin > row_end) row_begin = row_end;
    std::unique_ptr<sr_blend_plan> P(new sr_blend_plan());      // an early return frees what it owns
    P->ctx = ctx;
    const int rc = sr_build_blend_tables(h_tiles, n, cn, canvas_h, canvas_w, levels, weight_type, row_begin, row_end, ctx->num_cu,
                                         switches_from_env(), P.get());
    if (rc) return rc;
    // One table onto the device: an allocation of its own of max(count, 1) elements, owned by the plan, `count` elements copied
    // into it (src == nullptr: none -- the table is written per call).  The first failure sticks: the calls after it do nothing.
    int up_rc = SR_OK;
    auto up = [&](auto *&d, const void *src, size_t count, const char *name) {
        if (up_rc != SR_OK) return;
        const size_t es = sizeof(*d);
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, es * std::max<size_t>(count, 1));
        if (e != hipSuccess) {
            up_rc = dev_alloc_error("sr_blend_plan_create", name, es * std::max<size_t>(count, 1), e);
            return;
        }
        P->owned.push_back(p);
        d = static_cast<std::remove_reference_t<decltype(d)>>(p);
        if (src && count && (e = hipMemcpy(p, src, es * count, hipMemcpyHostToDevice)) != hipSuccess)
            up_rc = sr_set_error(SR_ERR_HIP, "sr_blend_plan_create: upload: %s", hipGetErrorString(e));
    };
    up(P->d_arena, nullptr, std::max<size_t>(P->arena_floats, 4), "arena");
    up(P->d_tiles, P->tiles.data(), P->tiles.size(), "tile table");
    up(P->d_classes, P->classes.data(), P->classes.size(), "class table");
    up(P->d_srcs, nullptr, n, "src table");
    up(P->d_fdesc, nullptr, n, "final table");
    up(P->d_luts, P->luts.data(), P->luts.size(), "luts");
    if (P->n_edge_blocks > 0) {
        up(P->d_edge_blocks, P->edge_blocks.data(), P->edge_blocks.size(), "edge blocks");
        up(P->d_edge_cand, P->edge_cand.data(), P->edge_cand.size(), "edge candidates");
    }
    up(P->d_cand_off, P->cand_off.data(), P->cand_off.size(), "candidate table");
    up(P->d_cand_idx, P->cand_idx.data(), P->cand_idx.size(), "candidate table");
    if (P->fused) {
        up(P->d_fedge_blocks, P->fedge_blocks.data(), P->fedge_blocks.size(), "fused edge blocks");
        up(P->d_fedge_cand, P->fedge_cand.data(), P->fedge_cand.size(), "fused edge candidates");
        up(P->d_fcand_off, P->fcand_off.data(), P->fcand_off.size(), "fused candidate table");
        up(P->d_fcand_idx, P->fcand_idx.data(), P->fcand_idx.size(), "fused candidate table");
        if (P->n_march_total > 0) {
            up(P->d_rects, P->rects.data(), P->rects.size(), "rectangle items");
            up(P->d_rect_cand, P->rect_cand.data(), P->rect_cand.size(), "rectangle candidates");
        }
        for (int k = 1; k <= MARCH_NT; ++k)
            if (P->n_march_items[k] > 0) up(P->d_march_items[k], P->march_items[k].data(), P->march_items[k].size(), "march items");
    }
    if (up_rc) return up_rc;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_live_plan.insert(P.get());
    }
    *out = P.release();
    return SR_OK;
}

int sr_blend_plan_tile_rows(const sr_blend_plan *plan, int t, int *r0, int *r1)
{
    if (!plan_is_live(plan) || t < 0 || t >= plan->n || !r0 || !r1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_tile_rows: bad args");
    *r0 = plan->tile_rows[t].a;
    *r1 = plan->tile_rows[t].b;
    return SR_OK;
}

int sr_blend_plan_workspace_bytes(const sr_blend_plan *plan, size_t *bytes)
{
    if (!plan_is_live(plan) || !bytes) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_workspace_bytes: bad args");
    *bytes = plan->arena_floats * sizeof(float);
    return SR_OK;
}

static int blend_check_tiles(sr_blend_plan *P, int dtype, void *const *h_d_tiles, const int64_t *h_strides)
{
    if (!h_d_tiles || !h_strides) return sr_set_error(SR_ERR_INVALID_ARG, "blend: null argument");
    if (dtype != SR_U8 && dtype != SR_F32) return sr_set_error(SR_ERR_INVALID_ARG, "blend: dtype must be SR_U8 or SR_F32");
    const int es = dtype == SR_U8 ? 1 : 4;
    for (int t = 0; t < P->n; ++t) {
        if (!h_d_tiles[t] && !P->tile_rows[t].empty()) return sr_set_error(SR_ERR_INVALID_ARG, "blend: tile %d pointer is null", t);
        if (h_strides[t] < (int64_t)P->tiles[t].w * P->cn * es) return sr_set_error(SR_ERR_SHAPE, "blend: tile %d stride too small", t);
    }
    return SR_OK;
}

// The format of G_1 for one call (G1<>): the plan's part, u8 tiles, and tile strides k_down2_march's 32-bit row offsets hold
// for -- every tile's, so that a subset's pyramids and the gather over all tiles decide alike.  h_strides == nullptr: strides
// that fit (the query).
static int g1_format(const sr_blend_plan *P, int dtype, const int64_t *h_strides)
{
    if (!P->g1_u16 || dtype != SR_U8) return G1_F32;
    for (int t = 0; t < P->n && h_strides; ++t)
        if (!down2_stride_fits(h_strides[t], P->tiles[t].H[0])) return G1_F32;
    return G1_U16;
}

int sr_blend_plan_g1_format(const sr_blend_plan *plan, int dtype, int *fmt)
{
    if (!plan_is_live(plan) || !fmt || (dtype != SR_U8 && dtype != SR_F32)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_g1_format: bad args");
    *fmt = g1_format(plan, dtype, nullptr);
    return SR_OK;
}

int sr_blend_plan_march_items(const sr_blend_plan *plan, int nt, int32_t *out, int64_t cap, int64_t *count)
{
    if (!plan_is_live(plan) || nt < 0 || nt > MARCH_NT || !count || (out && cap < 0))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_march_items: bad args");
    if (nt == 0) {
        const std::vector<RectItem> &r = plan->rects;
        *count = (int64_t)r.size();
        for (int64_t i = 0; out && i < std::min<int64_t>(cap, *count); ++i) {
            const int v[4] = {r[i].x, r[i].y, r[i].w, r[i].h};
            memcpy(out + 4 * i, v, sizeof(v));
        }
        return SR_OK;
    }
    static_assert(sizeof(MarchItem) == 8 * sizeof(int32_t), "eight ints per item");
    const std::vector<MarchItem> &m = plan->march_items[nt];
    *count = (int64_t)m.size();
    if (out && !m.empty()) memcpy(out, m.data(), sizeof(MarchItem) * (size_t)std::min<int64_t>(cap, *count));
    return SR_OK;
}

// Stage A of the Laplacian blend: weight pyramids (when `first`) and the down / up chains of the listed tiles.
// The listed tiles' descriptors are compacted into a scratch table, so kernels are launched over exactly them.
static int blend_pyramids(sr_blend_plan *P, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                          const int *idx, int n_idx, bool first)
{
    sr_ctx *ctx = P->ctx;
    const int rows = P->row_end - P->row_begin;
    if (rows <= 0 || P->max_nl <= 1) return SR_OK;
    dim3 block(64, 4);
    if (first && !P->weights_ready) {
        // weight pyramids: level 0 analytic (LUT) -> 1, then planar chain.  They depend only on the tile shapes and
        // the row windows, both fixed per plan: built by the first blend, kept in the arena for every later one.
        P->weights_ready = true;
        for (int i = 0; i + 1 < P->max_nl; ++i) {
            if (P->cmax_rows[i + 1] <= 0) continue;
            ProfScope ps(ctx, "weight_down");
            dim3 grid((P->cmax_w[i + 1] + 63) / 64, (P->cmax_rows[i + 1] + 3) / 4, (unsigned)P->classes.size());
            if (i == 0) hipLaunchKernelGGL(k_down<SRC_LUT>, grid, block, 0, ctx->stream, P->d_classes, (const TileSrc *)nullptr, i, 1, P->d_arena, P->d_luts);
            else hipLaunchKernelGGL(k_down<SRC_PLANAR>, grid, block, 0, ctx->stream, P->d_classes, (const TileSrc *)nullptr, i, 1, P->d_arena, P->d_luts);
        }
    }
    if (n_idx <= 0) return check_launch("weight chain");
    // compacted tables for this subset (the full tables when the subset is everything, in order)
    const TileDev *d_tiles = P->d_tiles;
    const TileSrc *d_srcs = P->d_srcs;
    std::vector<TileDev> sub_t;
    std::vector<TileSrc> sub_s(n_idx);
    bool all = (n_idx == P->n);
    for (int k = 0; k < n_idx && all; ++k) all = idx[k] == k;
    for (int k = 0; k < n_idx; ++k) {
        const int t = idx[k];
        if (t < 0 || t >= P->n) return sr_set_error(SR_ERR_INVALID_ARG, "blend: tile index %d out of range", t);
        sub_s[k].p = h_d_tiles[t];
        sub_s[k].stride = h_strides[t];
    }
    int max_w[SR_MAX_LEVELS] = {0}, max_g[SR_MAX_LEVELS] = {0}, max_r[SR_MAX_LEVELS] = {0}, max_nl = 1;
    for (int k = 0; k < n_idx; ++k) {
        const TileDev &T = P->tiles[idx[k]];
        max_nl = std::max(max_nl, T.nl);
        for (int i = 0; i < T.nl; ++i) {
            max_w[i] = std::max(max_w[i], T.W[i]);
            max_g[i] = std::max(max_g[i], T.g1[i] - T.g0[i]);
            max_r[i] = std::max(max_r[i], T.r1[i] - T.r0[i]);
        }
    }
    if (all) {
        HIPCHK(upload_if_changed(ctx, P->d_srcs, sub_s.data(), sizeof(TileSrc) * n_idx, P->sh_srcs));
    } else {
        sub_t.resize(n_idx);
        for (int k = 0; k < n_idx; ++k) sub_t[k] = P->tiles[idx[k]];
        const size_t o_src = up256(sizeof(TileDev) * n_idx), total = o_src + up256(sizeof(TileSrc) * n_idx);
        std::vector<char> packed(total, 0);
        memcpy(packed.data(), sub_t.data(), sizeof(TileDev) * n_idx);
        memcpy(packed.data() + o_src, sub_s.data(), sizeof(TileSrc) * n_idx);
        // a subset seen recently (the held / arriving halves of a staged blend alternate) keeps its device table
        CachedTable *slot = nullptr;
        for (auto &t : P->subset_tabs)
            if (t.shadow.size() == total && memcmp(t.shadow.data(), packed.data(), total) == 0) slot = &t;
        if (!slot) {
            slot = &P->subset_tabs[P->subset_next];
            P->subset_next = (P->subset_next + 1) % 4;
        }
        SRCHK(upload_cached(ctx, *slot, packed.data(), total));
        d_tiles = slot->buf.as<const TileDev>();
        d_srcs = slot->buf.as<const TileSrc>(o_src);
    }
    // tiles whose levels 1 and 2 come out of one march (u8 RGB, 32-bit offsets inside a tile and the arena; a strip's row
    // windows included)
    const int g1f = g1_format(P, dtype, h_strides);                 // G1_U16: every listed tile with level-1 rows in use is taken below
    int n_take = 0, max_take_h1 = 0, max_take_cols = 0;
    if (P->down2 && P->cn == 3 && dtype == SR_U8 && P->arena_floats * sizeof(float) < 0xFFFF0000ull) {
        bool ok = true;
        for (int k = 0; k < n_idx && ok; ++k) ok = down2_stride_fits(sub_s[k].stride, P->tiles[idx[k]].H[0]);
        for (int k = 0; k < n_idx && ok; ++k) {
            const TileDev &T = P->tiles[idx[k]];
            if (!down2_takes(T)) continue;
            ++n_take;
            max_take_h1 = std::max(max_take_h1, T.g1[1] - T.g0[1]);
            max_take_cols = std::max(max_take_cols, (T.g1[2] - T.g0[2]) * down2_cols_count(T));
        }
    }
    // Gaussian chain
    for (int i = 0; i + 1 < max_nl; ++i) {
        if (max_g[i + 1] <= 0) continue;
        ProfScope ps(ctx, i == 0 ? "down_l0" : "down_l1p");
        const bool blk = (P->cn == 3 || P->cn == 1) && !(i == 0 && dtype != SR_U8);
        int skip2 = 0;
        if (blk && i <= 1 && n_take > 0) {
            // levels 1 and 2 of the tiles with full row windows in one march (sr_down2.inc); the others keep the two launches
            if (i == 0) {
                // Segment length (level-2 rows per work item).  Every item pays three extra level-1 rows, yet short segments win:
                // measured at 200 MP (a sweep on one box) 6 .. 12 rows 0.51-0.54 ms, 16: 0.58, 32: 0.61, 64: 0.68 -- the
                // kernel is bound by its stores' way through the memory system, which many short items keep busier.  The longest
                // length up to 12 that still gives every wave slot four items, never below 6.
                int items = 0, seg2 = 12;
                {
                    const long long slots = (long long)ctx->num_cu * 16;    // four waves per SIMD
                    for (int cand = 12; cand >= 6; --cand) {
                        long long total = 0;
                        items = 0;
                        seg2 = cand;
                        for (int k = 0; k < n_idx; ++k) {
                            const TileDev &T = P->tiles[idx[k]];
                            if (!down2_takes(T)) continue;
                            const int it = down2_nstrip(down_ncg(T.W[0], T.W[1])) * ((T.g1[2] - T.g0[2] + cand - 1) / cand);
                            items = std::max(items, it);
                            total += it;
                        }
                        if (total >= 4 * slots) break;
                    }
                }
                dim3 grid2(items + (max_take_h1 + 3) / 4, 1, n_idx);
                if (g1f == G1_U16)
                    hipLaunchKernelGGL((k_down2_march<3, G1_U16>), grid2, dim3(64), 0, ctx->stream, d_tiles, d_srcs, seg2, items, P->d_arena,
                                       (unsigned)(P->arena_floats * sizeof(float)), P->d_arena, P->d_luts);
                else
                    hipLaunchKernelGGL((k_down2_march<3, G1_F32>), grid2, dim3(64), 0, ctx->stream, d_tiles, d_srcs, seg2, items, P->d_arena,
                                       (unsigned)(P->arena_floats * sizeof(float)), P->d_arena, P->d_luts);
            } else {
                dim3 grid2((max_take_cols + 255) / 256, 1, n_idx);
                if (g1f == G1_U16) hipLaunchKernelGGL(k_down2_cols<G1_U16>, grid2, dim3(256), 0, ctx->stream, d_tiles, P->d_arena);
                else hipLaunchKernelGGL(k_down2_cols<G1_F32>, grid2, dim3(256), 0, ctx->stream, d_tiles, P->d_arena);
            }
            if (n_take == n_idx) continue;
            skip2 = 1;
        }
        if (blk) {
            int max_cells = 0, seg_rows = 2;
            for (int cand = 32; cand >= 2; cand /= 2) {       // longest segments that still give ~8 blocks per CU;
                                                              // small levels end at 2 rows: short dependent chains
                long long total = 0;
                max_cells = 0;
                seg_rows = cand;
                for (int k = 0; k < n_idx; ++k) {
                    const TileDev &T = P->tiles[idx[k]];
                    if (i + 1 >= T.nl || T.g1[i + 1] <= T.g0[i + 1]) continue;
                    const int nseg = (T.g1[i + 1] - T.g0[i + 1] + cand - 1) / cand;
                    const int cells = down_ncg(T.W[i], T.W[i + 1]) * nseg;
                    max_cells = std::max(max_cells, cells);
                    total += cells;
                }
                if (total >= 512 * 1024) break;
            }
            {
                const int march_blocks = (max_cells + 255) / 256, cols_blocks = (max_g[i + 1] + 15) / 16;
                dim3 grid(march_blocks + cols_blocks, 1, n_idx);
                if (i == 0) {
                    if (P->cn == 3) hipLaunchKernelGGL((k_down_march<SRC_U8, 3>), grid, block, 0, ctx->stream, d_tiles, d_srcs, i, seg_rows, march_blocks, P->d_arena, P->d_luts, skip2);
                    else hipLaunchKernelGGL((k_down_march<SRC_U8, 1>), grid, block, 0, ctx->stream, d_tiles, d_srcs, i, seg_rows, march_blocks, P->d_arena, P->d_luts, skip2);
                } else {
                    if (P->cn == 3) hipLaunchKernelGGL((k_down_march<SRC_PLANAR, 3>), grid, block, 0, ctx->stream, d_tiles, d_srcs, i, seg_rows, march_blocks, P->d_arena, P->d_luts, skip2);
                    else hipLaunchKernelGGL((k_down_march<SRC_PLANAR, 1>), grid, block, 0, ctx->stream, d_tiles, d_srcs, i, seg_rows, march_blocks, P->d_arena, P->d_luts, skip2);
                }
            }
            continue;
        }
        dim3 grid((max_w[i + 1] + 63) / 64, (max_g[i + 1] + 3) / 4, n_idx);
        if (i == 0) {
            if (dtype == SR_U8) hipLaunchKernelGGL(k_down<SRC_U8>, grid, block, 0, ctx->stream, d_tiles, d_srcs, i, P->cn, P->d_arena, P->d_luts);
            else hipLaunchKernelGGL(k_down<SRC_F32>, grid, block, 0, ctx->stream, d_tiles, d_srcs, i, P->cn, P->d_arena, P->d_luts);
        } else {
            hipLaunchKernelGGL(k_down<SRC_PLANAR>, grid, block, 0, ctx->stream, d_tiles, d_srcs, i, P->cn, P->d_arena, P->d_luts);
        }
    }
    int rc = check_launch("down chain");
    if (rc) return rc;
    // collapse chain: levels max_nl-1 .. 1 (.. 2 when the gather is fused: it builds R_1 itself, in LDS)
    for (int i = max_nl - 1; i >= (P->fused ? 2 : 1); --i) {
        if (max_r[i] <= 0) continue;
        ProfScope ps(ctx, "up_level");
        if (P->cn == 3 || P->cn == 1) {
            dim3 grid((max_w[i] + 255) / 256, (max_r[i] + 7) / 8, n_idx);
            if (P->cn == 3) hipLaunchKernelGGL(k_up_level_blk<3>, grid, block, 0, ctx->stream, d_tiles, i, P->d_arena);
            else hipLaunchKernelGGL(k_up_level_blk<1>, grid, block, 0, ctx->stream, d_tiles, i, P->d_arena);
        } else {
            dim3 grid((max_w[i] + 63) / 64, (max_r[i] + 3) / 4, n_idx);
            hipLaunchKernelGGL(k_up_level, grid, block, 0, ctx->stream, d_tiles, i, P->cn, P->d_arena);
        }
    }
    return check_launch("up chain");
}

// Stage B: the canvas gather over all tiles (LAP: from G_1 / R_1 of stage A; else plain weighted average).
static int blend_gather(sr_blend_plan *P, bool lap, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                        uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32)
{
    sr_ctx *ctx = P->ctx;
    if (!d_canvas) return sr_set_error(SR_ERR_INVALID_ARG, "blend: null canvas");
    if (canvas_stride < (int64_t)P->canvas_w * P->cn) return sr_set_error(SR_ERR_SHAPE, "blend: canvas stride too small");
    const int rows = P->row_end - P->row_begin;
    if (rows <= 0) return SR_OK;
    std::vector<TileSrc> srcs(P->n);
    for (int t = 0; t < P->n; ++t) {
        srcs[t].p = h_d_tiles[t];
        srcs[t].stride = h_strides[t];
        P->fdesc[t].src = h_d_tiles[t];
        P->fdesc[t].stride = h_strides[t];
    }
    HIPCHK(upload_if_changed(ctx, P->d_srcs, srcs.data(), sizeof(TileSrc) * P->n, P->sh_srcs));
    HIPCHK(upload_if_changed(ctx, P->d_fdesc, P->fdesc.data(), sizeof(FinalDesc) * P->n, P->sh_fdesc));
    dim3 block(64, 4);
    {
        ProfScope ps(ctx, lap ? "final_gather" : "weighted_gather");
        if (lap && P->fused) {
            const int nbx_r = std::max((P->canvas_w + FU_BW - 1) / FU_BW, 1), nby_r = std::max((rows + FU_BH - 1) / FU_BH, 1);
            const int n_edge = P->n_fedge_blocks;
            // the marched zones first (long work items), then what is left; float tiles take the block kernel everywhere
            // The marched kernels form 32-bit byte offsets from the strides, which are known only here: a tile row as
            // (unsigned)ly * (unsigned)stride (ly < h), a canvas row as (unsigned)cstride advanced by 2 * cstride per step of an
            // item of at most MARCH_SEG steps.  A stride that does not fit (or is not positive) takes k_final_fused, whose row
            // addresses are 64-bit products, for the whole canvas: the same values from the same expressions.  (The bounds
            // leave room for the column offset the buffer instruction adds to the row's: one more canvas row, 64 KiB of a tile.)
            bool marched = dtype == SR_U8 && P->n_march_total > 0 &&
                           (unsigned long long)canvas_stride * MARCH_SPAN_ROWS < MARCH_OFF_LIMIT;
            for (int t = 0; t < P->n && marched; ++t)
                marched = h_strides[t] > 0 && (unsigned long long)h_strides[t] * (unsigned long long)P->tiles[t].h < MARCH_OFF_LIMIT;
            const unsigned arena_bytes = (unsigned)std::min<size_t>(P->arena_floats * sizeof(float), 0xFFFFFFFFu);
            const bool u16 = g1_format(P, dtype, h_strides) == G1_U16;      // (three planes, u8 tiles: the plan's and the call's part)
            if (marched && P->n_march_items[1] > 0) {
                ProfScope ps2(ctx, "gather_march1");
#define LAUNCH_MARCH1(CNV, G1V)                                                                                          \
    hipLaunchKernelGGL((k_final_march1<CNV, G1V>), dim3((unsigned)P->n_march_items[1]), dim3(64), 0, ctx->stream, P->d_march_items[1], \
                       P->d_fdesc, P->d_arena, arena_bytes, P->d_luts, d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w)
                if (u16) LAUNCH_MARCH1(3, G1_U16);
                else if (P->cn == 3) LAUNCH_MARCH1(3, G1_F32);
                else LAUNCH_MARCH1(1, G1_F32);
#undef LAUNCH_MARCH1
            }
#define LAUNCH_MARCHN(CNV, NTV, G1V)                                                                                     \
    hipLaunchKernelGGL((k_final_marchn<CNV, NTV, G1V>), dim3((unsigned)P->n_march_items[NTV]), dim3(64 * NTV), 0, ctx->stream,       \
                       P->d_march_items[NTV], P->d_fdesc, P->d_arena, arena_bytes, P->d_luts, d_canvas,                      \
                       (long long)canvas_stride, d_canvas_f32, P->canvas_w)
            static_assert(MARCH_NT == 4, "the tile counts launched here");
            for (int nt = 2; nt <= MARCH_NT && marched; ++nt) {
                if (P->n_march_items[nt] <= 0) continue;
                ProfScope ps2(ctx, nt == 2 ? "gather_march2" : (nt == 3 ? "gather_march3" : "gather_march4"));
                if (u16)             { if (nt == 2) LAUNCH_MARCHN(3, 2, G1_U16); else if (nt == 3) LAUNCH_MARCHN(3, 3, G1_U16); else LAUNCH_MARCHN(3, 4, G1_U16); }
                else if (P->cn == 3) { if (nt == 2) LAUNCH_MARCHN(3, 2, G1_F32); else if (nt == 3) LAUNCH_MARCHN(3, 3, G1_F32); else LAUNCH_MARCHN(3, 4, G1_F32); }
                else                 { if (nt == 2) LAUNCH_MARCHN(1, 2, G1_F32); else if (nt == 3) LAUNCH_MARCHN(1, 3, G1_F32); else LAUNCH_MARCHN(1, 4, G1_F32); }
            }
#undef LAUNCH_MARCHN
            ProfScope ps3(ctx, "gather_rest");
            // beside a march the remainder runs as rectangles of cells (k_final_rect: every cell finished in one visit, no edge
            // blocks); without one, the edge blocks and every regular block of k_final_fused
            if (marched) {
                if (P->n_rects > 0) {
#define LAUNCH_RECT(CNV, G1V)                                                                                            \
    hipLaunchKernelGGL((k_final_rect<CNV, G1V>), dim3((unsigned)P->n_rects), dim3(FU_THREADS), 0, ctx->stream, P->d_fdesc, P->d_rects, \
                       P->d_rect_cand, P->d_arena, P->d_luts, d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w,  \
                       P->row_begin, P->row_end)
                    if (u16) LAUNCH_RECT(3, G1_U16);
                    else if (P->cn == 3) LAUNCH_RECT(3, G1_F32);
                    else LAUNCH_RECT(1, G1_F32);
#undef LAUNCH_RECT
                }
            } else {
                dim3 grid((unsigned)(n_edge + (long long)nbx_r * nby_r)), blk1(FU_THREADS);
#define LAUNCH_FUSED(DT, CNV, G1V)                                                                                     \
    hipLaunchKernelGGL((k_final_fused<DT, CNV, G1V>), grid, blk1, 0, ctx->stream, P->d_fdesc, P->d_fcand_off, P->d_fcand_idx,  \
                       P->d_fedge_blocks, P->d_fedge_cand, n_edge, nbx_r, P->d_arena, P->d_luts, d_canvas,             \
                       (long long)canvas_stride, d_canvas_f32, P->canvas_w, P->row_begin, P->row_end)
                if (u16)             LAUNCH_FUSED(SRC_U8, 3, G1_U16);
                else if (P->cn == 3) { if (dtype == SR_U8) LAUNCH_FUSED(SRC_U8, 3, G1_F32); else LAUNCH_FUSED(SRC_F32, 3, G1_F32); }
                else                 { if (dtype == SR_U8) LAUNCH_FUSED(SRC_U8, 1, G1_F32); else LAUNCH_FUSED(SRC_F32, 1, G1_F32); }
#undef LAUNCH_FUSED
            }
        } else if (P->cn == 3 || P->cn == 1) {                  // weighted average (their Laplacian blend is fused, above)
            const int nbx_r = std::max((P->canvas_w + FIN_BW - 1) / FIN_BW, 1), nby_r = std::max((rows + FIN_BH - 1) / FIN_BH, 1);
            dim3 grid((unsigned)(P->n_edge_blocks + (long long)nbx_r * nby_r));     // edge blocks first, then the regular ones
#define LAUNCH_BLK(DT, CNV)                                                                                     \
    hipLaunchKernelGGL((k_final_fast<DT, CNV>), grid, block, 0, ctx->stream, P->d_fdesc, P->d_cand_off,           \
                       P->d_cand_idx, P->d_edge_blocks, P->d_edge_cand, P->n_edge_blocks, nbx_r, P->d_luts,  \
                       d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w, P->row_begin, P->row_end)
            if (P->cn == 3) { if (dtype == SR_U8) LAUNCH_BLK(SRC_U8, 3); else LAUNCH_BLK(SRC_F32, 3); }
            else            { if (dtype == SR_U8) LAUNCH_BLK(SRC_U8, 1); else LAUNCH_BLK(SRC_F32, 1); }
#undef LAUNCH_BLK
        } else {
            dim3 grid((P->canvas_w + 63) / 64, (rows + 3) / 4);
#define LAUNCH_FINAL(DT, LAPV)                                                                                  \
    hipLaunchKernelGGL((k_final<DT, LAPV>), grid, block, 0, ctx->stream, P->d_tiles, P->d_srcs, P->n, P->cn,     \
                       P->d_arena, P->d_luts, d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w,     \
                       P->row_begin, P->row_end)
            if (lap) {
                if (dtype == SR_U8) LAUNCH_FINAL(SRC_U8, true);
                else LAUNCH_FINAL(SRC_F32, true);
            } else {
                if (dtype == SR_U8) LAUNCH_FINAL(SRC_U8, false);
                else LAUNCH_FINAL(SRC_F32, false);
            }
#undef LAUNCH_FINAL
        }
    }
    return check_launch("final gather");
}

static int blend_impl(sr_blend_plan *P, bool lap, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                      uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32)
{
    int rc = blend_check_tiles(P, dtype, h_d_tiles, h_strides);
    if (rc) return rc;
    if (lap) {
        std::vector<int> idx(P->n);
        for (int t = 0; t < P->n; ++t) idx[t] = t;
        rc = blend_pyramids(P, dtype, h_d_tiles, h_strides, idx.data(), P->n, true);
        if (rc) return rc;
    }
    return blend_gather(P, lap, dtype, h_d_tiles, h_strides, d_canvas, canvas_stride, d_canvas_f32);
}

int sr_blend_pyramids(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                      const int *h_tile_idx, int n_idx, int first)
{
    if (!plan_is_live(plan)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_pyramids: null or destroyed plan");
    CTX_ENTER(plan->ctx);
    if (n_idx < 0 || (n_idx > 0 && !h_tile_idx)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_pyramids: bad tile list");
    int rc = blend_check_tiles(plan, dtype, h_d_tiles, h_strides);
    if (rc) return rc;
    return blend_pyramids(plan, dtype, h_d_tiles, h_strides, h_tile_idx, n_idx, first != 0);
}

int sr_blend_gather(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                    uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32)
{
    if (!plan_is_live(plan)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_gather: null or destroyed plan");
    CTX_ENTER(plan->ctx);
    int rc = blend_check_tiles(plan, dtype, h_d_tiles, h_strides);
    if (rc) return rc;
    return blend_gather(plan, true, dtype, h_d_tiles, h_strides, d_canvas, canvas_stride, d_canvas_f32);
}

int sr_laplacian_blend(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                       uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32)
{
    if (!plan_is_live(plan)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_laplacian_blend: null or destroyed plan");
    CTX_ENTER(plan->ctx);
    return blend_impl(plan, true, dtype, h_d_tiles, h_strides, d_canvas, canvas_stride, d_canvas_f32);
}

int sr_weighted_blend(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                      uint8_t *d_canvas, int64_t canvas_stride, float *d_canvas_f32)
{
    if (!plan_is_live(plan)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_weighted_blend: null or destroyed plan");
    CTX_ENTER(plan->ctx);
    return blend_impl(plan, false, dtype, h_d_tiles, h_strides, d_canvas, canvas_stride, d_canvas_f32);
}

static int fusion_host_impl(sr_ctx *ctx, bool lap, int dtype, const void *const *h_tiles, const sr_tile_rect *h_rects,
                            int n, int cn, int canvas_h, int canvas_w, int levels, int weight_type, uint8_t *h_canvas,
                            float *h_canvas_f32)
{
    if (!h_tiles || !h_rects || !h_canvas || n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "fusion_host: bad arguments");
    if (dtype != SR_U8 && dtype != SR_F32) return sr_set_error(SR_ERR_INVALID_ARG, "fusion_host: bad dtype");
    sr_blend_plan *plan = nullptr;
    int rc = sr_blend_plan_create(ctx, h_rects, n, cn, canvas_h, canvas_w, levels, weight_type, 0, canvas_h, &plan);
    if (rc) return rc;
    std::unique_ptr<sr_blend_plan, int (*)(sr_blend_plan *)> plan_owner(plan, sr_blend_plan_destroy);
    const int es = dtype == SR_U8 ? 1 : 4;
    std::vector<DevTemp> tiles;
    tiles.reserve(n);
    std::vector<void *> d_tiles(n, nullptr);
    std::vector<int64_t> strides(n);
    for (int t = 0; t < n; ++t) {
        const size_t bytes = (size_t)h_rects[t].h * h_rects[t].w * cn * es;
        strides[t] = (int64_t)h_rects[t].w * cn * es;
        tiles.emplace_back(ctx);
        SRCHK(tiles[t].alloc("fusion_host", bytes));
        d_tiles[t] = tiles[t].d;
        HIPCHK(hipMemcpyAsync(d_tiles[t], h_tiles[t], bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const size_t cbytes = (size_t)canvas_h * canvas_w * cn;
    DevTemp canvas(ctx), canvas_f32(ctx);
    SRCHK(canvas.alloc("fusion_host", cbytes));
    if (h_canvas_f32) SRCHK(canvas_f32.alloc("fusion_host", cbytes * sizeof(float)));
    SRCHK(blend_impl(plan, lap, dtype, d_tiles.data(), strides.data(), canvas.as<uint8_t>(), (int64_t)canvas_w * cn, canvas_f32.as<float>()));
    HIPCHK(hipMemcpyAsync(h_canvas, canvas.d, cbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_canvas_f32) HIPCHK(hipMemcpyAsync(h_canvas_f32, canvas_f32.d, cbytes * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_laplacian_fusion_host(sr_ctx *ctx, int dtype, const void *const *h_tiles, const sr_tile_rect *h_rects, int n,
                             int cn, int canvas_h, int canvas_w, int levels, int weight_type, uint8_t *h_canvas,
                             float *h_canvas_f32)
{
    CTX_ENTER(ctx);
    return fusion_host_impl(ctx, true, dtype, h_tiles, h_rects, n, cn, canvas_h, canvas_w, levels, weight_type, h_canvas,
                            h_canvas_f32);
}

int sr_weighted_fusion_host(sr_ctx *ctx, int dtype, const void *const *h_tiles, const sr_tile_rect *h_rects, int n,
                            int cn, int canvas_h, int canvas_w, int weight_type, uint8_t *h_canvas, float *h_canvas_f32)
{
    CTX_ENTER(ctx);
    return fusion_host_impl(ctx, false, dtype, h_tiles, h_rects, n, cn, canvas_h, canvas_w, 1, weight_type, h_canvas,
                            h_canvas_f32);
}

// ---- custom weights ----------------------------------------------------------------------------------
int sr_weighted_blend_custom(sr_blend_plan *plan, int dtype, void *const *h_d_tiles, const int64_t *h_strides,
                             const float *const *h_d_weights, const int64_t *h_weight_strides, uint8_t *d_canvas,
                             int64_t canvas_stride, float *d_canvas_f32)
{
    if (!plan_is_live(plan)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_weighted_blend_custom: null or destroyed plan");
    CTX_ENTER(plan->ctx);
    sr_blend_plan *P = plan;
    sr_ctx *c = P->ctx;
    int rc = blend_check_tiles(P, dtype, h_d_tiles, h_strides);
    if (rc) return rc;
    if (!h_d_weights || !h_weight_strides || !d_canvas) return sr_set_error(SR_ERR_INVALID_ARG, "sr_weighted_blend_custom: null argument");
    if (canvas_stride < (int64_t)P->canvas_w * P->cn) return sr_set_error(SR_ERR_SHAPE, "sr_weighted_blend_custom: canvas stride too small");
    std::vector<TileSrc> srcs(P->n);
    std::vector<CustomW> wts(P->n);
    for (int t = 0; t < P->n; ++t) {
        // like the tile itself (blend_check_tiles): a tile none of whose rows the plan reads needs no map
        if (!h_d_weights[t] && !P->tile_rows[t].empty()) return sr_set_error(SR_ERR_INVALID_ARG, "sr_weighted_blend_custom: weight map %d is null", t);
        if (h_weight_strides[t] < (int64_t)P->tiles[t].w * 4) return sr_set_error(SR_ERR_SHAPE, "sr_weighted_blend_custom: weight map %d stride too small", t);
        srcs[t].p = h_d_tiles[t];
        srcs[t].stride = h_strides[t];
        wts[t].w = h_d_weights[t];
        wts[t].stride = h_weight_strides[t];
    }
    const int rows = P->row_end - P->row_begin;
    if (rows <= 0) return SR_OK;
    void *scr = nullptr;
    rc = ctx_scratch(c, sizeof(CustomW) * P->n + 256, &scr);
    if (rc) return rc;
    HIPCHK(upload_if_changed(c, P->d_srcs, srcs.data(), sizeof(TileSrc) * P->n, P->sh_srcs));
    HIPCHK(upload_small(c, scr, wts.data(), sizeof(CustomW) * P->n));
    {
        ProfScope ps(c, "weighted_custom");
        dim3 grid((P->canvas_w + 63) / 64, (rows + 3) / 4), block(64, 4);
        if (dtype == SR_U8) hipLaunchKernelGGL(k_weighted_custom<SRC_U8>, grid, block, 0, c->stream, P->d_tiles, P->d_srcs, (const CustomW *)scr, P->n, P->cn, d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w, P->row_begin, P->row_end);
        else hipLaunchKernelGGL(k_weighted_custom<SRC_F32>, grid, block, 0, c->stream, P->d_tiles, P->d_srcs, (const CustomW *)scr, P->n, P->cn, d_canvas, (long long)canvas_stride, d_canvas_f32, P->canvas_w, P->row_begin, P->row_end);
    }
    return check_launch("weighted_custom");
}

}  // extern "C"

// sr_ctx_destroy (sr_runtime.hip) destroys a context's plans through this before the context leaves its registry.
void destroy_plans_of(sr_ctx *ctx)
{
    for (sr_blend_plan *p : plans_of(ctx)) sr_blend_plan_destroy(p);
}
