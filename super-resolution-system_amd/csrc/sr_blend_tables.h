// sr_blend_tables.h -- what the blend planner (sr_blend_plan.cpp, host only) and the blend kernels (sr_engine.hip with
// sr_march.inc and sr_down2.inc) have to agree on, once each: the table records, the block geometry, and the small rules both
// sides evaluate.  Plain C++: no HIP header is needed to read it.  Internal: nothing here is part of the C ABI.
#pragma once
#include <vector>

#include "sr_internal.h"

// HIP mode (hipcc compiles the .cpp units in it, too, without the runtime header: __forceinline__ is spelled out)
#if defined(__HIP__)
#define SR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SR_HD static inline
#endif

// ---- table records ----
struct TileDev {
    int h, w, x, y;
    int nl, fw, lut_off, cls;
    int H[SR_MAX_LEVELS], W[SR_MAX_LEVELS], P[SR_MAX_LEVELS];
    long long g_off[SR_MAX_LEVELS], r_off[SR_MAX_LEVELS], w_off[SR_MAX_LEVELS];
    int g0[SR_MAX_LEVELS], g1[SR_MAX_LEVELS];  // G row windows
    int r0[SR_MAX_LEVELS], r1[SR_MAX_LEVELS];  // R row windows
};
static_assert(sizeof(TileDev) % 16 == 0, "k_final_blk reads the leading {h,w,x,y} as one int4");

// What the final gather needs of one tile, 128 bytes (wave-uniform: read through the scalar cache).
struct FinalDesc {
    int x, y, w, h;
    int fw, lut_off, nl, pad0;
    int H1, W1, P1, pad1;
    long long g1, r1;      // float offsets of plane 0 of G_1 / R_1 in the arena (r1: read by no kernel since the unfused gather went)
    const void *src;       // level-0 tile data (row 0, possibly virtual) and its row stride in bytes
    long long stride;
    int H2, W2, P2, pad2;  // level 2 (the fused gather builds R_1 from it on the fly)
    long long g2, r2;      // float offsets of plane 0 of G_2 / R_2
    long long w1;          // float offset of the weight level 1 of the tile's class
    long long pad3;
};
static_assert(sizeof(FinalDesc) == 128, "FinalDesc layout");

// One block of an edge pass; the kernels read the list as int4 {x, y, z, w}.  A list ends with a sentinel whose `first` is
// the end of the last block's candidates.
struct EdgeBlock {
    int x, y;                        // canvas pixel of the block's corner (y includes row_begin)
    int shape;                       // 0: a wide block along horizontal tile edges, 1: a tall one along vertical edges
    int first;                       // its candidate tiles: cand[first .. next block's first), list order
};
static_assert(sizeof(EdgeBlock) == 16, "EdgeBlock layout");

struct MarchItem {                   // 32 bytes, wave-uniform (read through the scalar cache)
    int x0;                          // canvas x of lane 0's cell (the left halo cell); a multiple of 4
    int y0;                          // first canvas row
    int ncell;                       // useful cells: lanes 1 .. ncell store
    int nstep;                       // steps of two canvas rows (even)
    int tile[4];                     // the tiles of the zone, list order (their number: one item list per count)
};
static_assert(sizeof(MarchItem) == 32, "MarchItem layout");

struct RectItem {                    // 32 bytes, block-uniform
    int x, y;                        // canvas pixel of the first cell (y includes row_begin)
    int w, h;                        // cells across / down
    int cand, ncand;                 // candidate tiles: rect_cand[cand .. cand + ncand), list order
    int lp;                          // LDS pitch of the level-1 window (floats pairs per row)
    int colmajor;                    // 1: thread -> (column, row) with rows fastest
};
static_assert(sizeof(RectItem) == 32, "RectItem layout");

// ---- block geometry (the #ifndef'd values are what tools/build_variants.sh varies) ----
// k_final_fast
#ifndef FIN_TX
#define FIN_TX 64                 /* threads across a regular block */
#endif
#define FIN_TY (256 / FIN_TX)
#define FIN_BW (4 * FIN_TX)       /* canvas pixels per regular block */
#define FIN_BH (2 * FIN_TY)

// k_final_fused / k_final_rect
#ifndef FU_THREADS
#define FU_THREADS 256        /* threads (= 4 x 2 cells) per block */
#endif
#define FU_BW 128
#define FU_BH (FU_THREADS / 16)             /* 32 cells across, FU_THREADS / 32 cell rows of 2 pixels */
#define FU_E0H (FU_THREADS / 32)            /* edge shape 0: 256 x FU_E0H pixels (64 cells across) */
#define FU_E1W 16                           /* edge shape 1: FU_E1W x FU_E1H pixels (4 cells across: a vertical tile edge
                                               makes 1 - 3 of them border cells) */
#define FU_E1H (FU_THREADS / 2)
#define FU_LP 72              /* LDS pitch (floats) of a regular block's window: 18 patches of 4 columns */
/* pixels per plane window (two floats each): rows = block rows / 2 + 3, rounded up to even; 72 (regular), 136 (shape 0) or
   24 (shape 1) columns */
#define FU_ROWS_EVEN(bh) ((((bh) / 2 + 3) + 1) / 2 * 2)
#define FU_MAX3(a, b, c) ((a) > (b) ? ((a) > (c) ? (a) : (c)) : ((b) > (c) ? (b) : (c)))
#define FU_E1LP (((FU_E1W / 2 + 2 + 3) + 3) / 4 * 4)      /* window columns of shape 1, whole patches */
#define FU_PLANE FU_MAX3(FU_ROWS_EVEN(FU_BH) * 72, FU_ROWS_EVEN(FU_E0H) * 136, FU_ROWS_EVEN(FU_E1H) * FU_E1LP)

// window columns / rows fused_window can ask for, for a rectangle of w x h cells
static inline int rect_lp(int w) { return 4 * ((2 * w + 4) / 4) + 4; }
static inline int rect_rows(int h) { return 2 * ((h + 2) / 2) + 2; }

// k_final_march (sr_march.inc)
#ifndef MARCH_NT
#define MARCH_NT 4                   /* most tiles a marched zone may have */
#endif
#ifndef MARCH_SEG
#define MARCH_SEG 64                 /* most steps (of two canvas rows) per work item: a multiple of 2 */
#endif
#ifndef MARCH_ROUNDS
#define MARCH_ROUNDS 4.0             /* rounds of work items the 1-tile list is cut into (at two waves per SIMD) */
#define MARCH_ROUNDS_2 3.0           /* the 2-tile list */
#define MARCH_ROUNDS_N 2.0           /* the 3- and 4-tile lists */
#endif
#define MARCH_CELLS 62               /* useful cells per strip: 64 lanes less the two halo lanes */
// The marched kernels' byte offsets are 32-bit (buffer instructions): one item of at most MARCH_SEG steps spans
// 2 MARCH_SEG + 2 canvas rows, and the column offset the instruction adds stays below one more row; offsets stay below
// MARCH_OFF_LIMIT.  plan_march applies the bound to what it knows (arena, dense fp32 canvas), blend_gather to the strides.
static constexpr unsigned long long MARCH_SPAN_ROWS = 2ull * MARCH_SEG + 3ull, MARCH_OFF_LIMIT = 0xFFFF0000ull;

// k_down2_march (sr_down2.inc)
#ifndef D2_OUT
#define D2_OUT 48                    /* groups a wave stores (lanes 1 .. D2_OUT): 48 = whole 128-byte lines of G_1 (6) and G_2 (3) */
#endif

// ---- rules of the column-marching pyrDown kernels that the host evaluates, too ----
// number of interior column groups of a level: cg = 1 .. ncg
SR_HD int down_ncg(int ws, int wo)
{
    const int a = ws >= 10 ? (ws - 10) / 8 : 0;     // 2 x0 + 9 <= ws - 1
    const int b = wo >= 4 ? (wo - 4) / 4 : 0;       // x0 + 3 <= wo - 1
    return a < b ? a : b;
}
// the tiles k_down2_march takes: at least three levels, rows of levels 1 and 2 in use (a strip's row windows, or the whole tile), the
// level-1 window covering what the level-2 window reads (the planner's hull does: sr_plan_windows), sizes the march's shortcuts hold for
SR_HD bool down2_takes(const TileDev &T)
{
    if (T.nl < 3) return false;
    if (T.g0[1] >= T.g1[1] || T.g0[2] >= T.g1[2] || T.g0[0] >= T.g1[0]) return false;
    if (T.H[1] < 4 || T.H[0] < 8) return false;
    if (T.g0[1] > (2 * T.g0[2] - 2 > 0 ? 2 * T.g0[2] - 2 : 0)) return false;
    if (T.g1[1] < (2 * T.g1[2] + 1 < T.H[1] ? 2 * T.g1[2] + 1 : T.H[1])) return false;
    return down_ncg(T.W[0], T.W[1]) >= 1;
}
// the tile row strides the march's 32-bit row offsets hold for (h0: rows of level 0)
static inline bool down2_stride_fits(long long stride, int h0) { return stride > 0 && (unsigned long long)stride * (unsigned long long)(h0 + 2) < 0x7FFF0000ull; }
// strips of a row of groups 0 .. ncg (group 0 is a border group: its lane stores nothing)
SR_HD int down2_nstrip(int ncg) { return (ncg + D2_OUT) / D2_OUT; }
// level-2 columns the march leaves to k_down2_cols: 0 .. 3 and 2 ncg .. w2 - 1 (every column from 4 on below three groups)
SR_HD int down2_cols_count(const TileDev &T)
{
    const int ncg = down_ncg(T.W[0], T.W[1]), w2 = T.W[2];
    const int c_right = ncg >= 3 ? 2 * ncg : 4;
    return (w2 < 4 ? w2 : 4) + (w2 > c_right ? w2 - c_right : 0);
}

// ---- the planner (sr_blend_plan.cpp) ----
// The environment switches of a plan, read by the caller (sr_engine.hip: switches_from_env).
struct BlendSwitches {
    bool march = true;               // SR_MARCH != 0: marched zones where they pay
    bool march_force = false;        // SR_MARCH = 2: march whatever the size of the canvas
    bool down2 = true;               // SR_DOWN2 != 0: levels 1 and 2 of full-window u8 RGB tiles in one march (sr_down2.inc)
    bool g1_u16 = true;              // SR_G1_U16 != 0: G_1 of u8 tiles as 16-bit integers where every tile allows it
    bool march_taper = true;         // SR_MARCH_TAIL != 0: a march list ends with short items
    bool stats = false;              // SR_MARCH_STATS: the planner reports its lists on stderr
    double march_rounds[3] = {0, 0, 0};     // SR_MARCH_ROUNDS="r1,r2,r4": rounds of the 1- / 2- / 3- and 4-tile lists (0: the default)
    int rect_cells = 256;            // SR_RECT_CELLS: most cells per rectangle (32 .. 256)
};

// Everything a blend plan knows before it touches the device.  Tiles keep their list order inside every list (the reference's).
struct BlendTables {
    int n = 0, cn = 3, canvas_h = 0, canvas_w = 0, levels = 6, wtype = 1, row_begin = 0, row_end = 0, max_nl = 1;
    std::vector<TileDev> tiles;      // per tile
    std::vector<TileDev> classes;    // per weight class (pseudo tiles, cn = 1, g_off = weight levels)
    std::vector<SrWin> tile_rows;    // rows of the input tiles that are read
    std::vector<float> luts;
    size_t arena_floats = 0;
    std::vector<FinalDesc> fdesc;    // src / stride: filled per call
    bool fused = false;              // 1 or 3 channels: the Laplacian gather is k_final_fused / the marches, R_1 lives in LDS only
    bool march = false, down2 = true;
    bool g1_u16 = false;             // G_1 of u8 tiles as 16-bit integers (G1_U16): every tile whose level 1 is in use takes k_down2_march
    // launch extents per level
    int max_w[SR_MAX_LEVELS] = {0}, max_grows[SR_MAX_LEVELS] = {0}, max_rrows[SR_MAX_LEVELS] = {0};
    int cmax_w[SR_MAX_LEVELS] = {0}, cmax_rows[SR_MAX_LEVELS] = {0};
    // k_final_fast: edge pass work list, and candidate tiles per FIN_BW x FIN_BH block (CSR)
    std::vector<EdgeBlock> edge_blocks;
    std::vector<int> edge_cand, cand_off, cand_idx;
    int n_edge_blocks = 0;
    // k_final_fused: its own block tables -- regular blocks of FU_BW x FU_BH, edge blocks holding every cell with a border visit
    std::vector<EdgeBlock> fedge_blocks;
    std::vector<int> fedge_cand, fcand_off, fcand_idx;
    int n_fedge_blocks = 0;
    // marched zones (k_final_march): work items per tile count, and what they leave as rectangles of cells (k_final_rect)
    std::vector<MarchItem> march_items[MARCH_NT + 1];
    std::vector<RectItem> rects;
    std::vector<int> rect_cand;
    int n_march_items[MARCH_NT + 1] = {0};
    long long n_march_total = 0, n_rects = 0;
};

// Checks the arguments (SR_ERR_* with the message set) and fills *out.  Rows: 0 <= row_begin <= row_end <= canvas_h.
int sr_build_blend_tables(const sr_tile_rect *tiles, int n, int cn, int canvas_h, int canvas_w, int levels, int weight_type,
                          int row_begin, int row_end, int num_cu, const BlendSwitches &sw, BlendTables *out);
