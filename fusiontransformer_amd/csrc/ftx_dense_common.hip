// The one definition of what ftx_dense_common.h declares for both dense GEMM families (ftx_dense_bf16.hip, ftx_dense_split.hip): the
// ordered reduce of a split weight gradient, the token rows in front of a frame's patches, the tile and split rules and the plain entries;
// for the training forms of the patch embedding and the tap stems the ordered sum over the frames, the materialised ReLU mask, the strip
// store and the workspace sizes.
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

// dpos[t] = dtokens[0][t] + dtokens[1][t] + ... over the frames, ascending (fp32): the gradient of pos, whose rows 0 and 1 are also the
// gradients of cls and dist; one float4 per thread
__global__ __launch_bounds__(256) void dense_frames_sum_kernel(const float *__restrict__ dtokens, int b, int t0, int g, int dim, float *__restrict__ dpos,
                                                               float *__restrict__ dcls, float *__restrict__ ddist) {
  const int d4 = dim >> 2;
  const int64_t frame4 = (int64_t)(t0 + g) * d4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < frame4; e += (int64_t)gridDim.x * 256) {
    float4 s = ((const float4 *)dtokens)[e];
    for (int f = 1; f < b; ++f) {
      const float4 v = ((const float4 *)dtokens)[f * frame4 + e];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    ((float4 *)dpos)[e] = s;
    if (e < d4) ((float4 *)dcls)[e] = s;
    else if (e < 2 * d4 && t0 == 2) ((float4 *)ddist)[e - d4] = s;
  }
}

// gm = g where y > 0, else 0 (dense_relu_mask4: the select of DenseReluMaskedRows); one float4 per thread
__global__ __launch_bounds__(256) void dense_relu_mask_kernel(const float *__restrict__ g, const float *__restrict__ y, int64_t n4, float *__restrict__ gm) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256)
    ((float4 *)gm)[e] = dense_relu_mask4(((const float4 *)g)[e], ((const float4 *)y)[e]);
}

// dtokens[f][t] = t < t0 ? 0 : src[f g + t - t0]; one float4 per thread
__global__ __launch_bounds__(256) void dense_strip_store_kernel(const float *__restrict__ src, int b, int t0, int g, int dim, float *__restrict__ dtokens) {
  const int d4 = dim >> 2;
  const int64_t total = (int64_t)b * (t0 + g) * d4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / d4;
    const int j = (int)(e - row * d4);
    const int64_t f = row / (t0 + g);
    const int t = (int)(row - f * (t0 + g));
    ((float4 *)dtokens)[e] = t < t0 ? make_float4(0.f, 0.f, 0.f, 0.f) : ((const float4 *)src)[(f * g + (t - t0)) * d4 + j];
  }
}

namespace ftx {

void dense_frames_sum(const float *dtokens, int b, int t0, int g, int dim, float *dpos, float *dcls, float *ddist, hipStream_t st) {
  dense_frames_sum_kernel<<<grid_for((int64_t)(t0 + g) * (dim / 4), 256), 256, 0, st>>>(dtokens, b, t0, g, dim, dpos, dcls, ddist);
}

void dense_relu_mask(const float *g, const float *y, int64_t elems, float *gm, hipStream_t st) {
  dense_relu_mask_kernel<<<grid_for(elems / 4, 256), 256, 0, st>>>(g, y, elems / 4, gm);
}

void dense_strip_store(const float *src, int b, int t0, int g, int dim, float *dtokens, hipStream_t st) {
  dense_strip_store_kernel<<<grid_for((int64_t)b * (t0 + g) * (dim / 4), 256), 256, 0, st>>>(src, b, t0, g, dim, dtokens);
}

// Host-only sizes: the arguments the entries refuse give the floor of 256 bytes.
size_t dense_patch_bwd_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t p, int32_t dim) {
  if (b < 1 || c < 1 || h < 1 || w < 1 || p < 1 || dim < 4 || h % p || w % p) return 256;
  const int64_t k = (int64_t)c * p * p, g = (int64_t)(h / p) * (w / p);
  if (k * dim > 0x7fffffff / 8 || b * g > 0x7fffffff / 2) return 256;
  return (size_t)dense_patch_bwd_workspace(b, g, dim, (int)k).end;
}

size_t dense_tap_bwd_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co) {
  if (b < 1 || g < 1 || dim < 4 || co < 4 || (int64_t)co * dim > 0x7fffffff / 8 || (int64_t)b * g > 0x7fffffff / 2) return 256;
  return (size_t)dense_tap_bwd_workspace(b, g, dim, co).end;
}

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
