// What the dense MFMA GEMM families of the ViT trunk's Linears share (ftx_dense_bf16.hip, ftx_dense_split.hip): the fp32 epilogue of the
// GEMM kernels, the tile and split rules, and the host layer behind the extern "C" entries.  A family brings its kernels and a small
// description (DenseBf16, DenseSplit): the entry names that front its messages, and two launch hooks.  The pieces that need a single
// definition (the rules, dense_wgrad_reduce_kernel, the plain entries) are defined in ftx_dense_bf16.hip.
//
// Where the rows of A live and what happens to a finished sum is a policy of the GEMM kernels (DenseRows, DensePatches, DenseTapRows
// below): the tile rule, the staging, the MFMA order and the reduction order do not depend on it, so a form returns the bits of the
// plain entry run on a materialised copy of its A.
#pragma once
#include "ftx_bn_eval_op.h"
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
// device: the A-addressing forms of a GEMM kernel.  A form answers three questions:
//   row(r)    where row r of A starts (r < M, already clamped)
//   koff(k)   the offset of reduction index k from that start; k is a multiple of 4 and the four floats at it are contiguous
//   store     what the epilogue does with the finished sums of out[m][n .. n+3]
// ---------------------------------------------------------------------------------------
// A (M, K) row-major; the epilogue is the template's EPI (dense_epilogue): the plain entries
struct DenseRows {
  const float *A;
  int K;
  __device__ const float *row(int64_t r) const { return A + r * K; }
  __device__ int64_t koff(int k) const { return k; }
  template <int EPI>
  __device__ void store(float4 v, int64_t m, int n, int N, const float *__restrict__ bias, const float *__restrict__ pre_in, float *__restrict__ out,
                        float *__restrict__ pre_out) const {
    dense_epilogue<EPI>(v, m * N + n, n, bias, pre_in, out, pre_out);
  }
};

// The patch embedding: A is the unfold of img (b, C, H, W) that is never written.  Row r = (frame, gy, gx), k = (c, py, px) reads
// img[frame][c][gy P + py][gx P + px]; P % 4 == 0 keeps the four floats of a load inside one px run, 16-byte aligned.
// Epilogue: (sum + bias) + pos[T0 + patch], to row T0 + patch of the frame's (T0 + G) token rows.
struct DensePatches {
  const float *img, *pos;
  int C, H, W, P, gw, G, T0;
  __device__ const float *row(int64_t r) const {
    const int64_t f = r / G;
    const int g = (int)(r - f * G), gy = g / gw, gx = g - gy * gw;
    return img + (f * C * H + (int64_t)gy * P) * W + gx * P;
  }
  __device__ int64_t koff(int k) const {
    const int c = k / (P * P), rem = k - c * P * P, py = rem / P, px = rem - py * P;
    return ((int64_t)c * H + py) * W + px;
  }
  template <int EPI>
  __device__ void store(float4 v, int64_t m, int n, int N, const float *__restrict__ bias, const float *__restrict__, float *__restrict__ out,
                        float *__restrict__) const {
    const int64_t f = m / G;
    const int t = T0 + (int)(m - f * G);
    const float4 b = *(const float4 *)&bias[n];
    const float4 p = *(const float4 *)&pos[(int64_t)t * N + n];
    v = make_float4((v.x + b.x) + p.x, (v.y + b.y) + p.y, (v.z + b.z) + p.z, (v.w + b.w) + p.w);
    *(float4 *)&out[(f * (T0 + G) + t) * N + n] = v;
  }
};

// The tap stem: A is the token buffer (b, T0 + G, K) with the T0 leading rows of every frame skipped.  Epilogue: bias, ReLU, then the
// eval-mode BatchNorm of ftx_bn_eval_op.h (Conv1x1 -> ReLU -> BatchNorm), to out (b G, N): channels-last (b, gh, gw, N).
struct DenseTapRows {
  const float *tokens, *gamma, *beta, *mean, *var;
  float eps;
  int K, G, T0;
  __device__ const float *row(int64_t r) const {
    const int64_t f = r / G;
    return tokens + (f * (T0 + G) + T0 + (r - f * G)) * K;
  }
  __device__ int64_t koff(int k) const { return k; }
  template <int EPI>
  __device__ void store(float4 v, int64_t m, int n, int N, const float *__restrict__ bias, const float *__restrict__, float *__restrict__ out,
                        float *__restrict__) const {
    const float4 b = *(const float4 *)&bias[n];
    float o[4] = {v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = o[e] < 0.f ? 0.f : o[e];   // nn.ReLU: NaN stays NaN
      o[e] = bn_eval_elem(x, mean[n + e], var[n + e], eps, gamma[n + e], beta[n + e], 0.f, 0);
    }
    *(float4 *)&out[m * N + n] = make_float4(o[0], o[1], o[2], o[3]);
  }
};

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
//   F::gemm_name, F::wgrad_name, F::patch_name, F::tap_name   the entries' names, as they front every message
//   F::gemm<MI, NI, EPI, WKN>(grid, st, form, args)   launches the GEMM kernel of that instantiation on an A-addressing form
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
  const DenseRows rows = {a.A, a.K};
  switch (epi) {
    case FTX_EPI_NONE: F::template gemm<MI, NI, FTX_EPI_NONE, WKN>(grid, st, rows, a); break;
    case FTX_EPI_BIAS: F::template gemm<MI, NI, FTX_EPI_BIAS, WKN>(grid, st, rows, a); break;
    case FTX_EPI_BIAS_GELU: F::template gemm<MI, NI, FTX_EPI_BIAS_GELU, WKN>(grid, st, rows, a); break;
    default: F::template gemm<MI, NI, FTX_EPI_DGELU, WKN>(grid, st, rows, a); break;
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

// A GEMM on a form other than DenseRows: W (n, k) as nn.Linear stores it, the form's own epilogue, the tile of dense_gemm_tile(m, n).
template <class F, class Form>
void dense_launch_form(const Form &form, const DenseGemmArgs &a, hipStream_t st) {
  int mi, ni;
  dense_gemm_tile(a.M, a.N, &mi, &ni);
  const dim3 grid((unsigned)ceil_div(a.N, 64 * ni), (unsigned)ceil_div(a.M, 64 * mi));
  if (mi == 2) F::template gemm<2, 2, FTX_EPI_BIAS, false>(grid, st, form, a);
  else if (ni == 2) F::template gemm<1, 2, FTX_EPI_BIAS, false>(grid, st, form, a);
  else F::template gemm<1, 1, FTX_EPI_BIAS, false>(grid, st, form, a);
}

// tokens[f][0] = cls + pos[0], tokens[f][1] = dist + pos[1] (T0 = 2): the rows in front of the patches (dense_tokens_head_kernel)
void dense_tokens_head(const float *cls, const float *dist, const float *pos, int b, int t0, int g, int dim, float *tokens, hipStream_t st);

// ftx_vit_patch_embed_<family>: tokens (b, t0 + gh gw, dim) from img (b, c, h, w) without the unfold
template <class F>
int dense_patch_embed_entry(const float *img, const float *W, const float *bias, const float *cls, const float *dist, const float *pos, int32_t b,
                            int32_t c, int32_t h, int32_t w, int32_t p, int32_t dim, int32_t t0, float *tokens, void *stream) {
  const char *me = F::patch_name;
  FTX_REQUIRE(b >= 0 && c >= 1 && h >= 1 && w >= 1 && p >= 1 && dim >= 4, "%s: bad size (b=%d c=%d h=%d w=%d patch=%d dim=%d)", me, b, c, h, w, p, dim);
  FTX_REQUIRE(t0 == 1 || t0 == 2, "%s: t0 must be 1 or 2 (t0=%d)", me, t0);
  FTX_REQUIRE(p % 4 == 0, "%s: patch must be a multiple of 4 (patch=%d)", me, p);
  FTX_REQUIRE(h % p == 0 && w % p == 0, "%s: the image must be whole patches (h=%d w=%d patch=%d)", me, h, w, p);
  FTX_REQUIRE(dim % 4 == 0, "%s: dim must be a multiple of 4 (dim=%d)", me, dim);
  const int64_t k = (int64_t)c * p * p, g = (int64_t)(h / p) * (w / p);
  FTX_REQUIRE(k % kDenseGranule == 0, "%s: c * patch * patch must be a multiple of %d (%lld)", me, kDenseGranule, (long long)k);
  FTX_REQUIRE((int64_t)b * g <= 0x7fffffff / 2 && k * dim <= 0x7fffffff && (int64_t)b * c * h * w <= 0x7fffffff && (g + t0) * dim <= 0x7fffffff,
              "%s: too large", me);
  if (b == 0) return FTX_OK;
  FTX_REQUIRE(img && W && bias && cls && pos && tokens, "%s: null pointer", me);
  FTX_REQUIRE(dist || t0 == 1, "%s: null pointer (dist with t0 = 2)", me);
  FTX_REQUIRE(aligned16(img) && aligned16(W) && aligned16(bias) && aligned16(cls) && aligned16(dist) && aligned16(pos) && aligned16(tokens),
              "%s: pointers must be 16-byte aligned", me);
  const hipStream_t st = (hipStream_t)stream;
  const DensePatches form = {img, pos, c, h, w, p, w / p, (int)g, t0};
  const DenseGemmArgs a = {nullptr, W, bias, nullptr, (int64_t)b * g, dim, (int)k, tokens, nullptr};
  dense_launch_form<F>(form, a, st);
  dense_tokens_head(cls, dist, pos, b, t0, (int)g, dim, tokens, st);
  return check_launch(me);
}

// ftx_vit_tap_stem_<family>: out (b, g, co) = BatchNorm(ReLU(tokens[:, t0:] W^T + bias)) in eval mode
template <class F>
int dense_tap_stem_entry(const float *tokens, const float *W, const float *bias, const float *gamma, const float *beta, const float *mean,
                         const float *var, float eps, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *out, void *stream) {
  const char *me = F::tap_name;
  FTX_REQUIRE(b >= 0 && g >= 1 && dim >= kDenseGranule && co >= 4, "%s: bad size (b=%d g=%d dim=%d co=%d)", me, b, g, dim, co);
  FTX_REQUIRE(t0 >= 0 && t0 <= 2, "%s: t0 must be 0, 1 or 2 (t0=%d)", me, t0);
  FTX_REQUIRE(dim % kDenseGranule == 0, "%s: dim must be a multiple of %d (dim=%d)", me, kDenseGranule, dim);
  FTX_REQUIRE(co % 4 == 0, "%s: co must be a multiple of 4 (co=%d)", me, co);
  FTX_REQUIRE((int64_t)b * (g + t0) <= 0x7fffffff / 2 && (int64_t)co * dim <= 0x7fffffff, "%s: too large", me);
  if (b == 0) return FTX_OK;
  FTX_REQUIRE(tokens && W && bias && gamma && beta && mean && var && out, "%s: null pointer", me);
  FTX_REQUIRE(aligned16(tokens) && aligned16(W) && aligned16(bias) && aligned16(out), "%s: pointers must be 16-byte aligned", me);
  const DenseTapRows form = {tokens, gamma, beta, mean, var, eps, dim, g, t0};
  const DenseGemmArgs a = {nullptr, W, bias, nullptr, (int64_t)b * g, co, dim, out, nullptr};
  dense_launch_form<F>(form, a, (hipStream_t)stream);
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
