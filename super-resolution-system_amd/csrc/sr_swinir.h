// sr_swinir.h -- what sr_swinir_host.cpp (host only: the description checks, the table list, the relative-position index, the
// plan) hands to sr_swinir.hip (the kernels and the forward).  Internal: nothing here is part of the C ABI.  It includes no
// HIP header, so that the host unit compiles with a plain C++ compiler (tools/sanitize/swinir_driver.cpp).
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
    int cp = 0, qp = 0;                                 // planes of a C buffer, of the qkv / hidden buffer
    int tail = 0, halo = 0;
    long long tail_tiles = 0;
    long long plane0 = 0, plane_t = 0;                  // a trunk plane, the largest plane of a tail buffer
    size_t trunk_bytes = 0, workspace_bytes = 0;
};

int sw_check_desc(const char *who, const sr_swinir_desc *d);
std::vector<SwTable> sw_tables(const sr_swinir_desc &d);
std::vector<SwStep> sw_tail_steps(const sr_swinir_desc &d);
// rel[i * 64 + j]: the row of the bias table that query token i and key token j of a window share.
void sw_rel_index(int *rel);
// One axis of the backward extent rule (as backward_extents of sr_net_common.h).
void sw_backward_extents(const SwStep *steps, int n, int out_mult, int lo, int hi, int len, std::vector<int> &a, std::vector<int> &b);
int sw_geometry(const char *who, const sr_swinir_desc &d, int h, int w, int tail, SwGeom &g);
