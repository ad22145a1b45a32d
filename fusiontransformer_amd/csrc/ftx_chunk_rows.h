// The second pass of the two-pass column sums (ftx_colsum.hip: bias gradients; ftx_layernorm.hip: d gamma, d beta and the bias gradient of
// the LayerNorm backward): one kernel text for both, so the order of the sum, and with it the bits, cannot drift apart.  A `static`
// __global__: every translation unit that includes this header gets its own copy, so only the files that launch it include it.
#pragma once
#include "ftx_common.h"

namespace ftx {

// out[c] = sum over the chunk rows of part[k][c] (float64 partial rows of a first pass), rounded to float32 once.  Block = 16 columns x
// 16 chunk lanes; a lane sums every 16th partial row (independent loads), the 16 lanes are combined in lane order.
// Grid: ceil_div(cols, 16) blocks of 256 threads.
static __global__ __launch_bounds__(256) void chunk_rows_sum_kernel(const double *__restrict__ part, int chunks, int cols, float *__restrict__ out) {
  __shared__ double sh[16][16];
  const int cw = threadIdx.x & 15, cl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cw;
  double s = 0;
  if (c < cols) {
#pragma unroll 4
    for (int k = cl; k < chunks; k += 16) s += part[(int64_t)k * cols + c];
  }
  sh[cl][cw] = s;
  __syncthreads();
  if (cl == 0 && c < cols) {
    double t = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += sh[q][cw];
    out[c] = (float)t;
  }
}

}  // namespace ftx
