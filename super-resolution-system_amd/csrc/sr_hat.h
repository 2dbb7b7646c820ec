// sr_hat.h -- what sr_hat_host.cpp (host only: the description checks, the table list, the overlapping attention's index, the
// plan) hands to sr_hat.hip (the kernels and the forward).  Internal: nothing here is part of the C ABI.  It includes no HIP
// header, so that the host unit compiles with a plain C++ compiler (tools/sanitize/hat_driver.cpp).  The geometry (SwGeom), the
// window's relative-position index (sw_rel_index at HT_WIN), the step list of the pixelshuffle tail and the extent rule are
// sr_swinir.h's.
#pragma once
#include <cstddef>
#include <vector>

#include "sr_hip.h"
#include "sr_internal.h"
#include "sr_swinir.h"

constexpr int HT_WIN = 16, HT_TOK = HT_WIN * HT_WIN, HT_SHIFT = HT_WIN / 2;     // window side, queries of a window, the shift
constexpr int HT_REL = (2 * HT_WIN - 1) * (2 * HT_WIN - 1);                     // 961 rows of a window attention's bias table
constexpr int HT_EXT = 24, HT_KEYS = HT_EXT * HT_EXT, HT_OFF = (HT_EXT - HT_WIN) / 2;   // the enlarged window: side, keys, margin
constexpr int HT_REL_OCA = (HT_WIN + HT_EXT - 1) * (HT_WIN + HT_EXT - 1);       // 1521 rows of an OCAB's bias table

// The tables of sr_hat_create in forward order.  The kinds SwinIR has keep its numbers (sr_swinir.h).
enum {
    HT_T_RPB_OCA = 32, // overlap_attn.relative_position_bias_table, [1521][heads]; its bias entry is ignored
    HT_T_CAB0,         // conv_block.cab.0, 3 x 3, C -> n_mid
    HT_T_CAB2,         // conv_block.cab.2, 3 x 3, n_mid -> C
    HT_T_ATT1,         // conv_block.cab.3.attention.1, [n_squeeze][C]
    HT_T_ATT3          // conv_block.cab.3.attention.3, [C][n_squeeze]
};

int ht_check_desc(const char *who, const sr_hat_desc *d);
std::vector<SwTable> ht_tables(const sr_hat_desc &d);
std::vector<SwStep> ht_tail_steps(const sr_hat_desc &d);
// idx[i * 576 + j]: the row of an OCAB's bias table that query i and key j of the enlarged window share (the default formula,
// negative values wrapped).
void ht_oca_index(int *idx);
// A caller's index [256][576]: every value in [-1521, 1520], negatives wrapped once into out.
int ht_wrap_oca_index(const char *who, const int *in, int *out);
// sw_plan_geometry with HAT's SwFamily: g.tp, g.chunks and g.red_bytes are set.
int ht_geometry(const char *who, const sr_hat_desc &d, int h, int w, int tail, SwGeom &g);
