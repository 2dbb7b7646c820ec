// sr_swinir.h -- what sr_swinir_host.cpp (host only: the description checks, the table lists, the relative-position index, the
// plan -- SwinIR's, and the part of them that sr_hat_host.cpp shares) hands to sr_swinir.hip, sr_hat.hip and sr_swin_common.h
// (the kernels and the forward).  Internal: nothing here is part of the C ABI.  It includes no HIP header, so that the host
// units compile with a plain C++ compiler (tools/sanitize/swinir_driver.cpp, hat_driver.cpp).
#pragma once
#include <cstddef>
#include <vector>

#include "sr_hip.h"
#include "sr_internal.h"

constexpr int SW_WIN = 8, SW_TOK = SW_WIN * SW_WIN, SW_SHIFT = SW_WIN / 2;      // window side, tokens of a window, the shift
constexpr int SW_REL = (2 * SW_WIN - 1) * (2 * SW_WIN - 1);                     // rows of a relative-position bias table
constexpr int SW_MID = 64;                                                      // num_feat of the reconstruction
constexpr int SW_LIN_CC = 32;                                                   // cin chunk of the linear layers' mainloop
constexpr int SW_DEFAULT_TAIL = 256;

inline int sw_pad64(int v) { return (v + 63) / 64 * 64; }

// The tables of sr_swinir_create in forward order.
enum {
    SW_T_HEAD = 0,     // conv_first, 3 x 3, 3 -> C
    SW_T_LN,           // a LayerNorm: weight = gamma[C], bias = beta[C]
    SW_T_QKV,          // attn.qkv, [3 C][C]
    SW_T_RPB,          // attn.relative_position_bias_table, [225][heads]; its bias entry is ignored
    SW_T_PROJ,         // attn.proj, [C][C]
    SW_T_FC1,          // mlp.fc1, [hidden][C]
    SW_T_FC2,          // mlp.fc2, [C][hidden]
    SW_T_CONV,         // 3 x 3, C -> C (an RSTB's convolution, conv_after_body)
    SW_T_CBU,          // conv_before_upsample, 3 x 3, C -> 64
    SW_T_UP,           // 3 x 3, 64 -> 64 r^2 (+ PixelShuffle(r))
    SW_T_UPD,          // pixelshuffledirect's upsample.0, 3 x 3, C -> 3 s^2
    SW_T_C64,          // 3 x 3, 64 -> 64 (conv_up1, conv_up2, conv_hr)
    SW_T_LAST          // conv_last, 3 x 3, 64 -> 3
};

struct SwTable {
    int kind, r;                   // r: the shuffle factor of SW_T_UP / SW_T_UPD, else 1
    int cout, cin, ks;             // the caller's array is [cout][cin][ks][ks] (a LayerNorm: cout = C, cin = ks = 0; the bias
                                   // table: cout = 225, cin = heads, ks = 0); the bias holds cout values (the bias table: none)
};

// One convolution of the tail phase as the extent rule sees it (sr_net_common.h's ExtStep, restated so that this header needs
// no HIP): the replication / shuffle factor behind it and the resolution multiplier of its own output.
struct SwStep {
    int r, mult;
};

struct SwGeom {
    int hp = 0, wp = 0;                                 // the padded image
    int trunk_bufs = 0;                                 // trunk buffers of cp planes (SwinIR: 4, HAT: 5)
    int cp = 0, qp = 0, tp = 0;                         // planes of a C buffer, of the qkv / hidden buffer, of HAT's CAB middle (SwinIR: 0)
    int tail = 0, halo = 0, chunks = 0;                 // chunks: row chunks of HAT's channel mean (SwinIR: 0)
    long long tail_tiles = 0;
    long long plane0 = 0, plane_t = 0;                  // a trunk plane, the largest plane of a tail buffer
    size_t red_bytes = 0;                               // HAT's chunk sums and channel scales (SwinIR: 0)
    size_t trunk_bytes = 0, workspace_bytes = 0;
};

// What tells one window-attention family's plan from another's (sw_plan_geometry).
struct SwFamily {
    int win;                       // window side: the image is padded to multiples of it
    int trunk_bufs;                // buffers of cp planes in the trunk
    int tp;                        // planes of one further trunk buffer (HAT's CAB middle tensor), or 0
    int chunk_rows;                // rows of a chunk of the channel mean (red_bytes = C chunks doubles + C floats), or 0: none
    size_t cap;                    // the trunk's largest size in bytes
    const char *cap_name;          // ... and its name in the refusal
    bool padded_rows;              // the row limit is tested on the padded rows (HAT) or on h (SwinIR): two distinct refusals
};

// The front of a description check, in the order every family tests: the widths, then (after the family's own widths) the
// depths, then the affine (what: the names in the message; extra: one more value that must be finite).
int sw_check_widths(const char *who, int C, int heads, int hidden);
int sw_check_depths(const char *who, int n_groups, int depth, const char *group_name);
int sw_check_affine(const char *who, const char *what, const float *mean, float range, float extra = 0.0f);
// The tables of an attention block (LN, QKV, the bias table of kind rpb_kind with rpb_rows rows, PROJ), of an MLP (LN, FC1,
// FC2) and of the pixelshuffle reconstruction (CBU, UP ..., LAST), appended to t.
void sw_emit_attention(std::vector<SwTable> &t, int C, int heads, int rpb_kind, int rpb_rows);
void sw_emit_mlp(std::vector<SwTable> &t, int C, int hidden);
void sw_emit_shuffle_tail(std::vector<SwTable> &t, int C, int s);
// The tables of any of the three reconstructions (SR_SWINIR_PIXELSHUFFLE / _PIXELSHUFFLEDIRECT / _NEAREST_CONV), appended to t.
void sw_emit_tail(std::vector<SwTable> &t, int C, int s, int upsampler);
std::vector<SwStep> sw_shuffle_steps(int s);
int sw_check_desc(const char *who, const sr_swinir_desc *d);
std::vector<SwTable> sw_tables(const sr_swinir_desc &d);
std::vector<SwStep> sw_tail_steps(const sr_swinir_desc &d);
// rel[i * win^2 + j]: the row of the bias table that query token i and key token j of a win x win window share.
void sw_rel_index(int win, int *rel);
// One axis of the backward extent rule (as backward_extents of sr_net_common.h).
void sw_backward_extents(const SwStep *steps, int n, int out_mult, int lo, int hi, int len, std::vector<int> &a, std::vector<int> &b);
// The plan of either family: padded size, buffer geometry, the tail's sub-piece grid, every refusal by size.
int sw_plan_geometry(const char *who, const SwFamily &f, int C, int hidden, int scale, const std::vector<SwStep> &steps, int h, int w, int tail,
                     SwGeom &g);
int sw_geometry(const char *who, const sr_swinir_desc &d, int h, int w, int tail, SwGeom &g);
// The out-parameters of sr_*_plan (each may be null).
void sw_write_plan(const SwGeom &g, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes);
