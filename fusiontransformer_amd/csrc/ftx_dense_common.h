// What the dense MFMA GEMM families of the ViT trunk's Linears share (ftx_dense_bf16.hip, ftx_dense_split.hip): the fp32 epilogue of the
// GEMM kernels, the tile and split rules, and the host layer behind the extern "C" entries.  A family brings its kernels and a small
// description (DenseBf16, DenseSplit): the entry names that front its messages, and two launch hooks.  The pieces that need a single
// definition (the rules, dense_wgrad_reduce_kernel, the plain entries) are defined in ftx_dense_bf16.hip.
#pragma once
#include "ftx_common.h"
#include "ftx_mfma.h"

namespace ftx {

// ---------------------------------------------------------------------------------------
// device: the epilogue of a GEMM kernel
// ---------------------------------------------------------------------------------------
// nn.GELU() (approximate="none") and its derivative, in fp32
__device__ inline float gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ inline float dgelu(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * (0.39894228040143268f * expf(-0.5f * x * x));
}

// v: the finished fp32 sums of out[o .. o+3], o = m * N + n.  Bias, then the pre-activation is kept and the GELU applied, or the sum is
// multiplied by the GELU's derivative at the kept pre-activation; one float4 store per output.
template <int EPI>
__device__ inline void dense_epilogue(float4 v, int64_t o, int n, const float *__restrict__ bias, const float *__restrict__ pre_in,
                                      float *__restrict__ out, float *__restrict__ pre_out) {
  if (EPI == FTX_EPI_BIAS || EPI == FTX_EPI_BIAS_GELU) {
    const float4 b = *(const float4 *)&bias[n];
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  }
  if (EPI == FTX_EPI_BIAS_GELU) {
    *(float4 *)&pre_out[o] = v;
    v = make_float4(gelu(v.x), gelu(v.y), gelu(v.z), gelu(v.w));
  }
  if (EPI == FTX_EPI_DGELU) {
    const float4 p = *(const float4 *)&pre_in[o];
    v = make_float4(v.x * dgelu(p.x), v.y * dgelu(p.y), v.z * dgelu(p.z), v.w * dgelu(p.w));
  }
  *(float4 *)&out[o] = v;
}

// ---------------------------------------------------------------------------------------
// host: the rules, functions of the shape alone (ftx_dense_*_tile reports them)
// ---------------------------------------------------------------------------------------
constexpr int kDenseCUs = 256;      // MI355X; a constant of the tiling, not a device query
constexpr int kDenseGranule = 64;   // the GEMM's reduction is a multiple of this, and so is the length of a weight-gradient split
constexpr int kDenseDwTile = 128;   // dW tile side

// GEMM tile (64 mi) x (64 ni): the largest of 128 x 128, 64 x 128, 64 x 64 that still gives one block per CU (256 tiles); else 64 x 64.
void dense_gemm_tile(int64_t M, int N, int *mi, int *ni);
// Splits of the weight gradient's rows: enough (N/128 x K/128 x S) blocks for one per CU, at least 256 rows per split, at most 8
// splits.  Returns the split length.
int64_t dense_wgrad_split_len(int64_t M, int N, int K, int *splits);
inline size_t dense_wgrad_partial_bytes(int splits, int n, int k) { return splits > 1 ? sizeof(float) * (size_t)splits * n * k : 0; }
// dW = part[0] + part[1] + ... + part[splits-1] (dense_wgrad_reduce_kernel)
void dense_wgrad_reduce(const float *part, int splits, int64_t n4, float *dW, hipStream_t st);

size_t dense_wgrad_workspace_bytes(int64_t m, int32_t n, int32_t k);
int dense_tile_entry(const char *me, int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host);

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------
// host: the entries, generic over a family F:
//   F::gemm_name, F::wgrad_name                       the entries' names, as they front every message
//   F::gemm<MI, NI, EPI, WKN>(grid, st, args)         launches the GEMM kernel of that instantiation
//   F::wgrad(grid, st, G, X, M, N, K, len, part, dW)  launches the weight-gradient kernel
// ---------------------------------------------------------------------------------------
struct DenseGemmArgs {
  const float *A, *W, *bias, *pre_in;
  int64_t M;
  int N, K;
  float *out, *pre_out;
};

template <class F, int MI, int NI, bool WKN>
void dense_launch_epi(int epi, dim3 grid, hipStream_t st, const DenseGemmArgs &a) {
  switch (epi) {
    case FTX_EPI_NONE: F::template gemm<MI, NI, FTX_EPI_NONE, WKN>(grid, st, a); break;
    case FTX_EPI_BIAS: F::template gemm<MI, NI, FTX_EPI_BIAS, WKN>(grid, st, a); break;
    case FTX_EPI_BIAS_GELU: F::template gemm<MI, NI, FTX_EPI_BIAS_GELU, WKN>(grid, st, a); break;
    default: F::template gemm<MI, NI, FTX_EPI_DGELU, WKN>(grid, st, a); break;
  }
}

template <class F, int MI, int NI>
void dense_launch_gemm(int w_kn, int epi, dim3 grid, hipStream_t st, const DenseGemmArgs &a) {
  if (w_kn) dense_launch_epi<F, MI, NI, true>(epi, grid, st, a);
  else dense_launch_epi<F, MI, NI, false>(epi, grid, st, a);
}

template <class F>
int dense_gemm_entry(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n, int32_t k,
                     int32_t epilogue, float *out, float *pre_out, void *stream) {
  const char *me = F::gemm_name;
  FTX_REQUIRE(m >= 0 && n >= 4 && k >= kDenseGranule, "%s: bad size (m=%lld n=%d k=%d)", me, (long long)m, n, k);
  FTX_REQUIRE(k % kDenseGranule == 0, "%s: k must be a multiple of %d (k=%d)", me, kDenseGranule, k);
  FTX_REQUIRE(n % 4 == 0, "%s: n must be a multiple of 4 (n=%d)", me, n);
  FTX_REQUIRE(w_kn == 0 || w_kn == 1, "%s: w_kn must be 0 or 1", me);
  FTX_REQUIRE(epilogue >= FTX_EPI_NONE && epilogue <= FTX_EPI_DGELU, "%s: unknown epilogue %d", me, epilogue);
  FTX_REQUIRE(m <= 0x7fffffff / 2 && (int64_t)n * k <= 0x7fffffff, "%s: too large", me);
  if (m == 0) return FTX_OK;
  FTX_REQUIRE(A && W && out, "%s: null pointer", me);
  FTX_REQUIRE(epilogue == FTX_EPI_NONE || epilogue == FTX_EPI_DGELU || bias, "%s: null pointer (bias)", me);
  FTX_REQUIRE(epilogue != FTX_EPI_BIAS_GELU || pre_out, "%s: null pointer (pre_out)", me);
  FTX_REQUIRE(epilogue != FTX_EPI_DGELU || pre_in, "%s: null pointer (pre_in)", me);
  FTX_REQUIRE(aligned16(A) && aligned16(W) && aligned16(out) && aligned16(bias) && aligned16(pre_in) && aligned16(pre_out),
              "%s: pointers must be 16-byte aligned", me);
  int mi, ni;
  dense_gemm_tile(m, n, &mi, &ni);
  const dim3 grid((unsigned)ceil_div(n, 64 * ni), (unsigned)ceil_div(m, 64 * mi));
  const hipStream_t st = (hipStream_t)stream;
  const DenseGemmArgs a = {A, W, bias, pre_in, m, n, k, out, pre_out};
  if (mi == 2) dense_launch_gemm<F, 2, 2>(w_kn, epilogue, grid, st, a);
  else if (ni == 2) dense_launch_gemm<F, 1, 2>(w_kn, epilogue, grid, st, a);
  else dense_launch_gemm<F, 1, 1>(w_kn, epilogue, grid, st, a);
  return check_launch(me);
}

// A split count of 1 writes dW directly; otherwise each split writes its own (N x K) partial into the workspace and they are added in
// split order.
template <class F>
int dense_wgrad_entry(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                      void *stream) {
  const char *me = F::wgrad_name;
  FTX_REQUIRE(m >= 0 && n >= 4 && k >= 4, "%s: bad size (m=%lld n=%d k=%d)", me, (long long)m, n, k);
  FTX_REQUIRE(n % 4 == 0 && k % 4 == 0, "%s: n and k must be multiples of 4 (n=%d k=%d)", me, n, k);
  FTX_REQUIRE((int64_t)n * k <= 0x7fffffff / 8 && m <= 0x7fffffff / 2, "%s: too large", me);
  FTX_REQUIRE(dW, "%s: null pointer (dW)", me);
  FTX_REQUIRE(aligned16(dW) && aligned16(G) && aligned16(X) && aligned16(workspace), "%s: pointers must be 16-byte aligned", me);
  const hipStream_t st = (hipStream_t)stream;
  if (m == 0) {
    if (hipMemsetAsync(dW, 0, sizeof(float) * (size_t)n * k, st) != hipSuccess) {
      char what[64];
      snprintf(what, sizeof(what), "%s memset", me);
      return check_launch(what);
    }
    return FTX_OK;
  }
  FTX_REQUIRE(G && X, "%s: null pointer", me);
  int splits;
  const int64_t len = dense_wgrad_split_len(m, n, k, &splits);
  const size_t need = dense_wgrad_partial_bytes(splits, n, k);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace %zu < required %zu", me, workspace_bytes, need);
    return FTX_EWORKSPACE;
  }
  float *part = (float *)workspace;
  const dim3 grid((unsigned)ceil_div(k, kDenseDwTile), (unsigned)ceil_div(n, kDenseDwTile), (unsigned)splits);
  F::wgrad(grid, st, G, X, m, n, k, len, part, dW);
  if (splits > 1) dense_wgrad_reduce(part, splits, (int64_t)n * k / 4, dW, st);
  return check_launch(me);
}

}  // namespace ftx
