// sr_fft.h -- the fp32 FFT line engine of sr_commercial.hip (mixed-radix Stockham passes, Bluestein for a length with a
// prime factor above 1024) as internal functions, so that sr_content.hip transforms with the same kernels.  Internal:
// nothing here is part of the C ABI.
#pragma once
#include "sr_ctx.h"

// Table space sr_fft_lines needs for length n (float2 elements).
size_t sr_fft_tab_elems(int n);
// Line length of the work buffers for length n (n, or the Bluestein convolution length).
size_t sr_fft_work_len(int n);
// Forward DFT (sign -1, unscaled) of `lines` lines of length n held in X; P, Q are work buffers of
// lines * sr_fft_work_len(n) elements (X needs lines * n), tab holds sr_fft_tab_elems(n).  Returns the buffer with the
// result (X or P); every other buffer is free afterwards.  An inverse transform is the conjugate of the forward
// transform of the conjugate.  comp: direct-DFT passes of a radix above 32 add their terms with a Kahan compensation
// term (false: the plain sums of sr_fft_c2c and the high-frequency ratio).  Enqueues on ctx->stream, no sync.
float2 *sr_fft_lines(sr_ctx *ctx, float2 *X, float2 *P, float2 *Q, float2 *tab, long long lines, int n, bool comp);
// The workspace the commercial metrics and the content analysis share (grown on demand, freed with the context).
int sr_fft_workspace(sr_ctx *ctx, size_t bytes, char **out);
