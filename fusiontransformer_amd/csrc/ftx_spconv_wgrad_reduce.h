// Ordered second pass of the sparse-conv weight gradient, shared by the fp32 (ftx_spconv.hip) and bf16 (ftx_spconv_bf16.hip) kernels:
// both leave one (ca x cg) partial per tile of `tile_len` pairs in `part`, tiles numbered in offset order.
#pragma once
#include "ftx_common.h"

// dW[k] = sum of the partial tiles of offset k (tiles are numbered in offset order); an offset with ONE tile was written by the
// main kernel itself.  Block = (256/TL) float4 columns x TL tile lanes; lane l sums tiles l, l+TL, ... and the TL lane sums are
// added in lane order through LDS: a fixed summation tree, bit-reproducible.
template <int TL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, const int32_t *__restrict__ koff, int kvol,
                                                           int tile_len, int n_dense, int64_t mat, float *__restrict__ dW) {
  constexpr int COLS = 256 / TL;
  __shared__ float4 sh[TL][COLS];
  const int k = blockIdx.y;
  int first = 0, cnt = 0;
  for (int q = 0; q <= k; ++q) {
    int c = koff ? koff[q + 1] - koff[q] : n_dense;
    int nt = (c + tile_len - 1) / tile_len;
    if (q < k) first += nt; else cnt = nt;
  }
  if (cnt == 1) return;   // written directly by pairs_wgrad_kernel (block-uniform exit)
  const int col = threadIdx.x % COLS, tl = threadIdx.x / COLS;
  const int64_t chunks = ftx::ceil_div(mat / 4, COLS);
  // a block walks several column chunks: thousands of 4-KB blocks are bound by workgroup dispatch, not by bytes
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t e = (chunk * COLS + col) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < mat) {
      const float *src = part + (int64_t)first * mat + e;
      int t = tl;
      for (; t + 3 * TL < cnt; t += 4 * TL) {   // four independent loads in flight, added in tile order
        float4 v0 = *(const float4 *)&src[(int64_t)t * mat], v1 = *(const float4 *)&src[(int64_t)(t + TL) * mat];
        float4 v2 = *(const float4 *)&src[(int64_t)(t + 2 * TL) * mat], v3 = *(const float4 *)&src[(int64_t)(t + 3 * TL) * mat];
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
        s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
        s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
        s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
      }
      for (; t < cnt; t += TL) {
        float4 v = *(const float4 *)&src[(int64_t)t * mat];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
    }
    if (TL > 1) {
      sh[tl][col] = s;
      __syncthreads();
      if (tl == 0) {
#pragma unroll
        for (int l = 1; l < TL; ++l) {
          float4 v = sh[l][col];
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
      }
      __syncthreads();
    }
    if (tl == 0 && e < mat) *(float4 *)&dW[(int64_t)k * mat + e] = s;
  }
}

// Launches wgrad_reduce_kernel over the `tiles` partials (upper bound of the tile count) of a kvol-offset weight gradient.
static inline void launch_wgrad_reduce(const float *part, const int32_t *koff, int kvol, int tile_len, int n_dense, int64_t mat, int64_t tiles, float *dW,
                                       hipStream_t st) {
  // the centre offset of a submanifold map holds ~6x the average pair count: size the tile lanes for it, not for the average
  const int64_t big_tiles = kvol > 1 ? 6 * tiles / kvol : tiles;
  const int64_t want_blocks = ftx::ceil_div(1024, kvol);   // ~4 blocks per CU over all offsets
  auto rgrid = [&](int cols) { int64_t c = ftx::ceil_div(mat / 4, cols); return dim3((unsigned)(c < want_blocks ? c : want_blocks), (unsigned)kvol); };
  if (big_tiles <= 4)
    wgrad_reduce_kernel<1><<<rgrid(256), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
  else if (big_tiles <= 32)
    wgrad_reduce_kernel<4><<<rgrid(64), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
  else
    wgrad_reduce_kernel<16><<<rgrid(16), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
}
