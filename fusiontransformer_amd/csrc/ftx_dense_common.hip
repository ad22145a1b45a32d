// The one definition of what ftx_dense_common.h declares for both dense GEMM families (ftx_dense_bf16.hip, ftx_dense_split.hip): the
// ordered reduce of a split weight gradient, the token rows in front of a frame's patches, the tile and split rules and the plain entries.
#include "ftx_dense_common.h"

using namespace ftx;

// dW = part[0] + part[1] + ... + part[S-1], added in split order: a fixed summation order, bit-reproducible.
__global__ __launch_bounds__(256) void dense_wgrad_reduce_kernel(const float *__restrict__ part, int splits, int64_t n4, float *__restrict__ dW) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    float4 s = ((const float4 *)part)[e];
    for (int t = 1; t < splits; ++t) {
      const float4 v = ((const float4 *)part)[t * n4 + e];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    ((float4 *)dW)[e] = s;
  }
}

// the T0 rows in front of a frame's patches: cls + pos[0] and, with T0 = 2, dist + pos[1]; one float4 per thread
__global__ __launch_bounds__(256) void dense_tokens_head_kernel(const float *__restrict__ cls, const float *__restrict__ dist, const float *__restrict__ pos,
                                                                int b, int t0, int g, int dim, float *__restrict__ tokens) {
  const int d4 = dim >> 2;
  const int64_t total = (int64_t)b * t0 * d4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % d4) * 4, t = (int)((e / d4) % t0);
    const int64_t f = e / ((int64_t)d4 * t0);
    const float4 x = *(const float4 *)&(t == 0 ? cls : dist)[j];
    const float4 p = *(const float4 *)&pos[(int64_t)t * dim + j];
    *(float4 *)&tokens[(f * (t0 + g) + t) * dim + j] = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
  }
}

namespace ftx {

void dense_tokens_head(const float *cls, const float *dist, const float *pos, int b, int t0, int g, int dim, float *tokens, hipStream_t st) {
  dense_tokens_head_kernel<<<grid_for((int64_t)b * t0 * (dim / 4), 256), 256, 0, st>>>(cls, dist, pos, b, t0, g, dim, tokens);
}

void dense_gemm_tile(int64_t M, int N, int *mi, int *ni) {
  static const int cand[3][2] = {{2, 2}, {1, 2}, {1, 1}};
  for (const auto &c : cand) {
    if (ceil_div(M, 64 * c[0]) * ceil_div(N, 64 * c[1]) >= kDenseCUs) {
      *mi = c[0];
      *ni = c[1];
      return;
    }
  }
  *mi = 1;
  *ni = 1;
}

int64_t dense_wgrad_split_len(int64_t M, int N, int K, int *splits) {
  const int64_t tiles = ceil_div(N, kDenseDwTile) * ceil_div(K, kDenseDwTile);
  int64_t s = ceil_div(kDenseCUs, tiles);
  int64_t cap = M / 256;
  if (cap > 8) cap = 8;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  int64_t len = ceil_div(ceil_div(M, s), kDenseGranule) * kDenseGranule;
  if (len < kDenseGranule) len = kDenseGranule;
  *splits = (int)ceil_div(M, len);
  if (*splits < 1) *splits = 1;
  return len;
}

void dense_wgrad_reduce(const float *part, int splits, int64_t n4, float *dW, hipStream_t st) {
  dense_wgrad_reduce_kernel<<<grid_for(n4, 256), 256, 0, st>>>(part, splits, n4, dW);
}

size_t dense_wgrad_workspace_bytes(int64_t m, int32_t n, int32_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return 256;
  int splits;
  dense_wgrad_split_len(m, n, k, &splits);
  const size_t need = dense_wgrad_partial_bytes(splits, n, k);
  return need > 256 ? need : 256;
}

int dense_tile_entry(const char *me, int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  FTX_REQUIRE(tile_m_host && tile_n_host && split_host, "%s: null pointer", me);
  FTX_REQUIRE(m >= 1 && n >= 4 && k >= 4, "%s: bad size (m=%lld n=%d k=%d)", me, (long long)m, n, k);
  if (form == 0) {
    int mi, ni;
    dense_gemm_tile(m, n, &mi, &ni);
    *tile_m_host = 64 * mi;
    *tile_n_host = 64 * ni;
    *split_host = 1;
    return FTX_OK;
  }
  FTX_REQUIRE(form == 1, "%s: form must be 0 (GEMM) or 1 (weight gradient)", me);
  int splits;
  dense_wgrad_split_len(m, n, k, &splits);
  *tile_m_host = kDenseDwTile;
  *tile_n_host = kDenseDwTile;
  *split_host = splits;
  return FTX_OK;
}

}  // namespace ftx
