// sr_swin2sr.h -- what sr_swin2sr_host.cpp (host only: the description check, the table list, the plan, the continuous position
// bias and the logit scale) hands to sr_swin2sr.hip (the kernels and the forward).  Internal: nothing here is part of the C ABI.
// It includes no HIP header, so that the host unit compiles with a plain C++ compiler (tools/sanitize/swin2sr_driver.cpp).  The
// window, the geometry (SwGeom), the relative-position index, the reconstruction's tables and steps and the extent rule are
// sr_swinir.h's.
#pragma once
#include <cstddef>
#include <vector>

#include "sr_hip.h"
#include "sr_internal.h"
#include "sr_swinir.h"

constexpr int S2_CPB_HIDDEN = 512;                     // width of the continuous position bias MLP
constexpr int S2_LAYER_TABLES = 9;                     // tables of one layer

// The tables of sr_swin2sr_create in forward order.  The kinds SwinIR has keep its numbers (sr_swinir.h): the two kinds of 1 x 1
// projection (P_0, P_i) are SW_T_PROJ.
enum {
    S2_T_LOGIT = 48,   // attention.self.logit_scale, [heads]; its bias entry is ignored
    S2_T_CPB1,         // continuous_position_bias_mlp.0, [512][2], [512]
    S2_T_CPB2          // continuous_position_bias_mlp.2, [heads][512]; its bias entry is ignored
};

// The SwinIR description with the same fields (the reconstruction, the plan and the ranges are SwinIR's).
sr_swinir_desc s2_as_swinir(const sr_swin2sr_desc &d);
int s2_check_desc(const char *who, const sr_swin2sr_desc *d);
std::vector<SwTable> s2_tables(const sr_swin2sr_desc &d);
std::vector<SwStep> s2_tail_steps(const sr_swin2sr_desc &d);
int s2_geometry(const char *who, const sr_swin2sr_desc &d, int h, int w, int tail, SwGeom &g);
// What a create refuses of the caller's arrays before any device call: a k bias that is not zero, a non-finite logit scale.
int s2_check_tables(const char *who, const sr_swin2sr_desc &d, const std::vector<SwTable> &tables, const float *const *h_w,
                    const float *const *h_b);
// table[t * heads + head] = 16 sigmoid(cpb_mlp(coords(t))) for the 225 relative offsets of a window, float64 rounded once.
void s2_cpb_table(const float *w1, const float *b1, const float *w2, int heads, float *table);
// scale[head] = (float)exp(min((double)logit[head], ln 100)).
void s2_logit_scale(const float *logit, int heads, float *scale);
