// sr_niqe.h -- what the NIQE kernels (sr_niqe.hip) take from the host unit (sr_niqe_host.cpp): the plan and the MSCN window.
// Internal: nothing here is part of the C ABI.
#pragma once
#include <cstddef>

#include "sr_internal.h"

constexpr int NQ_BLOCK = 96;        // block side at scale 1 (48 at scale 2)
constexpr int NQ_R = 3;             // MSCN window radius: 7 taps
constexpr int NQ_FEAT = 36;

struct NqPlan {
    int H, W;                       // the kept plane: multiples of 96
    int nby, nbx;
    size_t off_half, off_rec;       // context scratch: the int32 half plane, then 2 nby nbx records
    size_t total;
};

// Every shape refusal of sr_niqe_plan; scope names the caller in the message.
int nq_plan(const char *scope, int h, int w, int cn, int crop_border, NqPlan *p);
// k_i = g_i / sum g, g_i = exp(-i^2 / (2 s^2)), s = 7 / 6, i = -3 .. 3.
void nq_window(double k[2 * NQ_R + 1]);
