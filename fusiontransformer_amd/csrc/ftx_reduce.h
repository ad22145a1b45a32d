// Small ordered sums that several kernel families share.  Each text fixes a summation order, and with it the bits of every result
// that goes through it; a family with another order (sd_column_totals, lb_column_sums, loss_finalize_kernel, wgrad_reduce_kernel, the
// __shfl_xor trees whose lanes all need the sum) keeps its own.  block_sum_u64 of ftx_image.hip also stays where it is: it places its
// barriers differently and knows its wave count at compile time, and jitter_pass_kernel grew by 96 instructions on the shared form.
#pragma once
#include "ftx_common.h"

namespace ftx {

// Sum over the 64 lanes of a wave by the __shfl_down tree (32, 16, ..., 1); valid on lane 0.
template <class T>
__device__ inline T wave_sum_down(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sum over a block of whole waves: the wave tree, lane 0 of each wave to sh[wave], thread 0 adds the waves in ascending order.
// sh holds blockDim.x / 64 values and may be reused at once by the next call.  Valid on thread 0.
template <class T>
__device__ inline T block_sum(T v, T *sh) {
  v = wave_sum_down(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  T r = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sh[w];
  return r;
}

}  // namespace ftx
