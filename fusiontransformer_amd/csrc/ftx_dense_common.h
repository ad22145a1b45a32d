// What the dense MFMA GEMM families of the ViT trunk's Linears share (ftx_dense_bf16.hip, ftx_dense_split.hip): everything but the way an
// fp32 operand becomes bf16 pieces and what is done with the pieces.  Here are the fp32 epilogue, the A-addressing forms, the tile and
// split rules, the one GEMM kernel and the one weight-gradient kernel (dense_gemm_kernel, dense_wgrad_kernel) and the host layer behind
// the extern "C" entries.  A family brings its entries and a description P (DenseBf16, DenseSplit), which says, and alone says:
//   P::NP, P::BK, P::STRIDE   bf16 images per operand, reduction elements staged per step, bf16 per LDS row, each with its reason
//   P::MIN_BLOCKS             the blocks per CU the kernels' registers are held to
//   P::pieces(float4)         the one place an operand is rounded or split: NP bf16x4
//   P::PROD, P::sum           the piece products of a 16-wide k-step, in order, each with its accumulator; the accumulators' one fp32 sum
//   P::gemm_name, ...         the entries' names, as they front every message
// The kernels do not ask which family they serve.  What needs a single definition (the rules, dense_wgrad_reduce_kernel,
// dense_tokens_head_kernel, the plain entries) is defined in ftx_dense_common.hip.
//
// Where the rows of A live and what happens to a finished sum is a policy of the GEMM kernel (DenseRows, DensePatches, DenseTapRows,
// DenseTapReluRows, DenseStripFold below): the tile rule, the staging, the MFMA order and the reduction order do not depend on it, so a
// form returns the bits of the plain entry run on a materialised copy of its A.  The weight-gradient kernel takes the same kind of
// policy for each of its two operands (the same forms, and DenseReluMaskedRows); the training forms of the patch embedding and the tap
// stems are built from them.
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

// The tap stem in training: DenseTapRows' rows, and the epilogue stops behind the ReLU: rows (b G, N) = ReLU(sum + bias).  The batch
// statistics of the BatchNorm behind it need every row, so it stays a pass of its own (ftx_bn_train_fwd on `rows`).
struct DenseTapReluRows {
  const float *tokens;
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
    for (int e = 0; e < 4; ++e) o[e] = o[e] < 0.f ? 0.f : o[e];   // nn.ReLU: NaN stays NaN
    *(float4 *)&out[m * N + n] = make_float4(o[0], o[1], o[2], o[3]);
  }
};

// The patch embedding's image gradient: A is the gradient of the tokens (b, T0 + G, K) behind its T0 leading rows (the strip), the sum
// is row (frame, gy, gx), column n = (c, py, px) of the unfold's gradient.  The patches do not overlap, so the fold is a permuted
// store: out = dimg (b, C, H, W), every pixel written exactly once, P % 4 == 0 keeps a float4 inside one px run.
struct DenseStripFold {
  const float *dtokens;
  int K, C, H, W, P, gw, G, T0;
  __device__ const float *row(int64_t r) const {
    const int64_t f = r / G;
    return dtokens + (f * (T0 + G) + T0 + (r - f * G)) * K;
  }
  __device__ int64_t koff(int k) const { return k; }
  template <int EPI>
  __device__ void store(float4 v, int64_t m, int n, int, const float *__restrict__, const float *__restrict__, float *__restrict__ out,
                        float *__restrict__) const {
    const int64_t f = m / G;
    const int g = (int)(m - f * G), gy = g / gw, gx = g - gy * gw;
    const int c = n / (P * P), rem = n - c * P * P, py = rem / P, px = rem - py * P;
    *(float4 *)&out[((f * C + c) * H + (int64_t)gy * P + py) * W + gx * P + px] = v;
  }
};

// ---------------------------------------------------------------------------------------
// device: the operand forms of the weight-gradient kernel.  Both operands are read along their channels, row r of the reduction at a
// time; a form answers row(r) (r < M, already clamped) and koff(c), the offset of channel c (a multiple of 4, four contiguous floats)
// from that start.  The A-forms above serve: DenseRows is the plain (M, channels) matrix, DensePatches the unfold of an image (X of
// the patch embedding), DenseTapRows the rows of a (b, T0 + G, channels) buffer behind the T0 leading rows of every frame (X of the
// tap stem, G of the patch embedding).  dense_load4 is the one read; a form may give it an overload.
// ---------------------------------------------------------------------------------------
template <class Form>
__device__ inline float4 dense_load4(const Form &f, int64_t r, int c) {
  return *(const float4 *)(f.row(r) + f.koff(c));
}

// G of the tap stem: the gradient of the BatchNorm's input, (M, N) plain rows, times the ReLU's mask taken from the saved output Y
// (M, N).  A select, not a product: g where y > 0, else 0 (also where y is NaN), so the sums are those of the plain entry run on the
// materialised masked gradient (dense_relu_mask_kernel writes that one for the bias gradient and the data gradient).
struct DenseReluMaskedRows {
  const float *G, *Y;
  int N;
  __device__ const float *row(int64_t r) const { return G + r * N; }
  __device__ int64_t koff(int c) const { return c; }
};
__device__ inline float4 dense_relu_mask4(float4 g, float4 y) {
  return make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f, y.w > 0.f ? g.w : 0.f);
}
__device__ inline float4 dense_load4(const DenseReluMaskedRows &f, int64_t r, int c) {
  return dense_relu_mask4(*(const float4 *)&f.G[r * f.N + c], *(const float4 *)&f.Y[r * f.N + c]);
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
// device: the two kernels, generic over a description P (the header comment lists its members), on v_mfma_f32_32x32x16_bf16.
//
// Operand maps (ftx_spconv_bf16.hip, cdna_hip_programming.md section 3): lane (r = lane & 31, h = lane >> 5) holds row r, k = 8h + j of
// both fragments of a 16-wide k-step, read with one ds_read_b128 from a bf16 LDS image whose rows are k-contiguous.  mfma(F1, F2)
// leaves C[row of F1][row of F2] with F2's row on the lane and four consecutive F1 rows in accumulator registers 4q..4q+3
// ((g&3) + 8(g>>2) + 4h), so every store below is a float4 along the output row.
// ---------------------------------------------------------------------------------------
// The staging geometry of a description: the block's 256 threads move one float4 each per pass.
template <class P>
struct DenseStage {
  static_assert(kDenseGranule % P::BK == 0, "the entry admits every multiple of kDenseGranule as the reduction");
  static constexpr int F4 = P::BK / 4;      // float4 per staged row
  static constexpr int ROWS = 256 / F4;     // rows per pass: thread -> (row tid / F4, float4 tid % F4)
  static constexpr int passes(int rows) { return rows / ROWS; }   // float4 per thread and step of an operand of that many rows
  // a [reduction][channel] operand stored transposed: item = (reduction pair, channel float4), two float4 per item
  static constexpr int pair_items(int channels) { return (P::BK / 2) * (channels / 4) / 256; }   // channels * BK / 2048
};

// One float4 of a staged row to offset o of every image: the pieces of four consecutive reduction elements.
template <class P>
__device__ inline void dense_store_row(__bf16 *img, int img_len, int o, float4 v) {
  const typename P::Pieces4 s = P::pieces(v);
#pragma unroll
  for (int c = 0; c < P::NP; ++c) *(bf16x4 *)&img[c * img_len + o] = s.p[c];
}

// Two float4 of reduction rows 2kp, 2kp+1 at channels ch .. ch+3, stored TRANSPOSED into image rows ch .. ch+3 as packed pairs.
template <class P>
__device__ inline void dense_store_pairs(__bf16 *img, int img_len, int ch, int kp, float4 v0, float4 v1) {
  const typename P::Pieces4 x0 = P::pieces(v0), x1 = P::pieces(v1);
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < P::NP; ++c) *(bf16x2 *)&img[c * img_len + (ch + e) * P::STRIDE + 2 * kp] = (bf16x2){x0.p[c][e], x1.p[c][e]};
}

// Registers 4q .. 4q+3 of the accumulators of one sub-tile as one finished float4: P::sum, the one add in front of the epilogue.
template <class P>
__device__ inline float4 dense_sum4(const f32x16 (&acc)[P::NACC], int q) {
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a[P::NACC];
#pragma unroll
    for (int c = 0; c < P::NACC; ++c) a[c] = acc[c][4 * q + e];
    v[e] = P::sum(a);
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------------------------------
// out[m][n] = epilogue( sum_k A[m][k] B[k][n] ) over the pieces of P,  B = W^T with W stored [N][K] (WKN = false: nn.Linear's weight,
// the forward) or B = W stored [K][N] (WKN = true: the data gradient dX = dY W).
//
// Block = 4 waves as 2 x 2, tile (64 MI) x (64 NI); wave (wm, wn) owns MI x NI 32 x 32 sub-tiles.  NP LDS images per operand,
// [piece][row][k] bf16; the next step's global loads are issued before this step's MFMAs (register staging, the pairs_gemm_bf16 pipeline).
// Rows past M and columns past N load clamped, always-valid addresses and are never stored.
// AF says where A's rows live and what the epilogue does: DenseRows is the (M, K) matrix with dense_epilogue<EPI>, DensePatches the
// patch embedding's unfold of an image, DenseTapRows the token buffer behind its leading rows.  Nothing else here depends on it, so
// every form sums the same products in the same order.
// ---------------------------------------------------------------------------------------
template <class P, int MI, int NI, int EPI, bool WKN, class AF>
__global__ __launch_bounds__(256, P::MIN_BLOCKS) void dense_gemm_kernel(const AF af, const float *__restrict__ W, const float *__restrict__ bias,
                                                                        const float *__restrict__ pre_in, int64_t M, int N, int K,
                                                                        float *__restrict__ out, float *__restrict__ pre_out) {
  using S = DenseStage<P>;
  constexpr int BM = 64 * MI, BN = 64 * NI;
  constexpr int AP = S::passes(BM);   // float4 of A per thread and step
  constexpr int BP = S::passes(BN);   // the same count for B in either orientation
  constexpr int BQ = S::pair_items(BN);
  static_assert(BP == 2 * BQ, "either orientation of W is the same number of float4");
  constexpr int AIMG = BM * P::STRIDE, BIMG = BN * P::STRIDE;
  __shared__ __attribute__((aligned(16))) __bf16 As[P::NP * AIMG];   // [piece][m][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[P::NP * BIMG];   // [piece][n][k]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  // row-major staging (A, and W stored [N][K]): pass p covers rows ROWS p .. ROWS p + ROWS - 1
  const int srow = tid / S::F4, sk4 = (tid % S::F4) * 4;
  const float *arow[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    int64_t r = m0 + p * S::ROWS + srow;
    arow[p] = af.row(r < M ? r : M - 1);
  }
  const float *brow[BP];
  // WKN: item e = (k pair kp, column float4 n4); two float4 per item (rows 2kp, 2kp+1), stored as packed k pairs
  int bkp[WKN ? BQ : 1], bn4[WKN ? BQ : 1];
  if constexpr (!WKN) {
#pragma unroll
    for (int p = 0; p < BP; ++p) {
      int r = n0 + p * S::ROWS + srow;
      brow[p] = W + (int64_t)(r < N ? r : N - 1) * K + sk4;
    }
  } else {
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const int e = q * 256 + tid;
      bn4[q] = (e % (BN / 4)) * 4;
      bkp[q] = e / (BN / 4);
      int n = n0 + bn4[q];
      brow[2 * q] = W + (int64_t)(2 * bkp[q]) * N + (n + 4 <= N ? n : N - 4);
      brow[2 * q + 1] = brow[2 * q] + N;
    }
  }

  f32x16 acc[MI][NI][P::NACC];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int c = 0; c < P::NACC; ++c)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[i][j][c][g] = 0.f;

  float4 ra[AP], rb[BP];
  auto load_step = [&](int c0) {
    const int64_t ak = af.koff(c0 + sk4);   // where the form keeps reduction index c0 + sk4 of a row
#pragma unroll
    for (int p = 0; p < AP; ++p) ra[p] = *(const float4 *)(arow[p] + ak);
    if constexpr (!WKN) {
#pragma unroll
      for (int p = 0; p < BP; ++p) rb[p] = *(const float4 *)(brow[p] + c0);
    } else {
#pragma unroll
      for (int p = 0; p < BP; ++p) rb[p] = *(const float4 *)(brow[p] + (int64_t)c0 * N);
    }
  };
  // the ONE place the operands become bf16 (P::pieces): fp32 registers -> the LDS images
  auto store_step = [&]() {
#pragma unroll
    for (int p = 0; p < AP; ++p) dense_store_row<P>(As, AIMG, (p * S::ROWS + srow) * P::STRIDE + sk4, ra[p]);
    if constexpr (!WKN) {
#pragma unroll
      for (int p = 0; p < BP; ++p) dense_store_row<P>(Bs, BIMG, (p * S::ROWS + srow) * P::STRIDE + sk4, rb[p]);
    } else {
#pragma unroll
      for (int q = 0; q < BQ; ++q) dense_store_pairs<P>(Bs, BIMG, bn4[q], bkp[q], rb[2 * q], rb[2 * q + 1]);
    }
  };

  const __bf16 *ap = &As[(wm * 32 * MI + l31) * P::STRIDE + 8 * half];
  const __bf16 *bp = &Bs[(wn * 32 * NI + l31) * P::STRIDE + 8 * half];
  load_step(0);
  for (int c0 = 0; c0 < K; c0 += P::BK) {
    store_step();
    __syncthreads();
    if (c0 + P::BK < K) load_step(c0 + P::BK);   // the next step's global loads fly under this step's MFMAs
#pragma unroll
    for (int s = 0; s < P::BK / 16; ++s) {
      bf16x8 af[P::NP][MI], bf[P::NP][NI];
#pragma unroll
      for (int c = 0; c < P::NP; ++c) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[c][i] = *(const bf16x8 *)(ap + c * AIMG + i * 32 * P::STRIDE + 16 * s);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf[c][j] = *(const bf16x8 *)(bp + c * BIMG + j * 32 * P::STRIDE + 16 * s);
      }
      // P::PROD[t] = (W piece, A piece, accumulator).  rows: n, columns (lanes): m.  The MI x NI sub-tiles between two uses of one
      // accumulator hide the MFMA's latency.
#pragma unroll
      for (int t = 0; t < P::NPROD; ++t)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j][P::PROD[t][2]] = mfma_bf16(bf[P::PROD[t][0]][j], af[P::PROD[t][1]][i], acc[i][j][P::PROD[t][2]]);
    }
    __syncthreads();
  }

  // lane (l31, half) of sub-tile (i, j): output row m, columns n .. n+3 in registers 4q .. 4q+3
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int64_t m = m0 + wm * 32 * MI + i * 32 + l31;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 32 * NI + j * 32 + 8 * q + 4 * half;
        if (n >= N) continue;
        af.template store<EPI>(dense_sum4<P>(acc[i][j], q), m, n, N, bias, pre_in, out, pre_out);
      }
  }
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[n][k] = sum_m G[m][n] X[m][k] over the pieces of P     (G = dY [M][N], X [M][K], both row-major over the reduction
// index m)
//
// Block = (128-column tile of k, 128-row tile of n, split s of the rows); 4 waves as 2 x 2, each 64 x 64.  Each step stages P::BK rows:
// float4 loads along the channels, stored TRANSPOSED as m-contiguous bf16 images [piece][channel][m] with two rows packed per 32-bit LDS
// write (the register stage of pairs_wgrad_bf16_kernel).  Rows past the split are zeroed on the block-uniform last step.
// A split count of 1 writes dW directly; otherwise each split writes its own (N x K) partial and dense_wgrad_reduce_kernel adds them.
// ---------------------------------------------------------------------------------------
// GF and XF say where the rows of G and X live (the forms above); nothing else here depends on them, so every pair of forms sums the
// same products in the same order as the plain entry on materialised operands.
template <class P, class GF, class XF>
__global__ __launch_bounds__(256, P::MIN_BLOCKS) void dense_wgrad_kernel(const GF gf, const XF xf, int64_t M, int N, int K, int64_t split_len,
                                                                         float *__restrict__ part, float *__restrict__ dW) {
  constexpr int T = kDenseDwTile;
  constexpr int ITEMS = DenseStage<P>::pair_items(T);   // (row pair, float4) items per thread and operand
  constexpr int IMG = T * P::STRIDE;
  __shared__ __attribute__((aligned(16))) __bf16 Gt[P::NP * IMG];   // [piece][n][m]
  __shared__ __attribute__((aligned(16))) __bf16 Xt[P::NP * IMG];   // [piece][k][m]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;   // wm: k half, wn: n half
  const int k0 = blockIdx.x * T, n0 = blockIdx.y * T;
  const int64_t lo = (int64_t)blockIdx.z * split_len;
  const int64_t hi = lo + split_len < M ? lo + split_len : M;

  int rp[ITEMS], c4[ITEMS], gcol[ITEMS], xcol[ITEMS];
#pragma unroll
  for (int q = 0; q < ITEMS; ++q) {
    const int e = q * 256 + tid;
    c4[q] = (e % (T / 4)) * 4;
    rp[q] = e / (T / 4);
    gcol[q] = n0 + c4[q] + 4 <= N ? n0 + c4[q] : N - 4;   // clamped columns reach only image rows that are never stored
    xcol[q] = k0 + c4[q] + 4 <= K ? k0 + c4[q] : K - 4;
  }

  f32x16 acc[2][2][P::NACC];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < P::NACC; ++c)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[i][j][c][g] = 0.f;

  float4 rg[ITEMS][2], rx[ITEMS][2];
  auto load_step = [&](int64_t r0) {
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int64_t r = r0 + 2 * rp[q] + h;
        r = r < M ? r : M - 1;
        rg[q][h] = dense_load4(gf, r, gcol[q]);
        rx[q][h] = dense_load4(xf, r, xcol[q]);
      }
  };
  auto store_step = [&](int64_t r0) {
    if (r0 + P::BK > hi) {   // block-uniform: the split's last step
#pragma unroll
      for (int q = 0; q < ITEMS; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (r0 + 2 * rp[q] + h >= hi) rg[q][h] = rx[q][h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the ONE place the operands become bf16 (P::pieces)
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
      dense_store_pairs<P>(Gt, IMG, c4[q], rp[q], rg[q][0], rg[q][1]);
      dense_store_pairs<P>(Xt, IMG, c4[q], rp[q], rx[q][0], rx[q][1]);
    }
  };

  const __bf16 *xp = &Xt[(wm * 64 + l31) * P::STRIDE + 8 * half];
  const __bf16 *gp = &Gt[(wn * 64 + l31) * P::STRIDE + 8 * half];
  load_step(lo);
  for (int64_t r0 = lo; r0 < hi; r0 += P::BK) {
    store_step(r0);
    __syncthreads();
    if (r0 + P::BK < hi) load_step(r0 + P::BK);
#pragma unroll
    for (int s = 0; s < P::BK / 16; ++s) {
      bf16x8 xf[P::NP][2], gf[P::NP][2];
#pragma unroll
      for (int c = 0; c < P::NP; ++c) {
#pragma unroll
        for (int i = 0; i < 2; ++i) xf[c][i] = *(const bf16x8 *)(xp + c * IMG + i * 32 * P::STRIDE + 16 * s);
#pragma unroll
        for (int j = 0; j < 2; ++j) gf[c][j] = *(const bf16x8 *)(gp + c * IMG + j * 32 * P::STRIDE + 16 * s);
      }
      // P::PROD[t] = (X piece, G piece, accumulator): the GEMM's list.  rows: k, columns (lanes): n
#pragma unroll
      for (int t = 0; t < P::NPROD; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j][P::PROD[t][2]] = mfma_bf16(xf[P::PROD[t][0]][i], gf[P::PROD[t][1]][j], acc[i][j][P::PROD[t][2]]);
    }
    __syncthreads();
  }

  float *dst = gridDim.z == 1 ? dW : part + (int64_t)blockIdx.z * N * K;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + l31;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + wm * 64 + i * 32 + 8 * q + 4 * half;
        if (k < K) *(float4 *)&dst[(int64_t)n * K + k] = dense_sum4<P>(acc[i][j], q);
      }
  }
}

// ---------------------------------------------------------------------------------------
// host: the entries, generic over a family F: its description (above) and the names of its entries.  Every launch is 256 threads.
// ---------------------------------------------------------------------------------------
struct DenseGemmArgs {
  const float *A, *W, *bias, *pre_in;
  int64_t M;
  int N, K;
  float *out, *pre_out;
};

template <class F, int MI, int NI, int EPI, bool WKN, class AF>
void dense_launch(dim3 grid, hipStream_t st, const AF &af, const DenseGemmArgs &a) {
  dense_gemm_kernel<F, MI, NI, EPI, WKN, AF><<<grid, 256, 0, st>>>(af, a.W, a.bias, a.pre_in, a.M, a.N, a.K, a.out, a.pre_out);
}

template <class F, int MI, int NI, bool WKN>
void dense_launch_epi(int epi, dim3 grid, hipStream_t st, const DenseGemmArgs &a) {
  const DenseRows rows = {a.A, a.K};
  switch (epi) {
    case FTX_EPI_NONE: dense_launch<F, MI, NI, FTX_EPI_NONE, WKN>(grid, st, rows, a); break;
    case FTX_EPI_BIAS: dense_launch<F, MI, NI, FTX_EPI_BIAS, WKN>(grid, st, rows, a); break;
    case FTX_EPI_BIAS_GELU: dense_launch<F, MI, NI, FTX_EPI_BIAS_GELU, WKN>(grid, st, rows, a); break;
    default: dense_launch<F, MI, NI, FTX_EPI_DGELU, WKN>(grid, st, rows, a); break;
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

// A GEMM on a form other than DenseRows: W (n, k) as nn.Linear stores it (or, WKN, stored (k, n): a data gradient), the form's own
// epilogue, the tile of dense_gemm_tile(m, n).
template <class F, class Form, int EPI = FTX_EPI_BIAS, bool WKN = false>
void dense_launch_form(const Form &form, const DenseGemmArgs &a, hipStream_t st) {
  int mi, ni;
  dense_gemm_tile(a.M, a.N, &mi, &ni);
  const dim3 grid((unsigned)ceil_div(a.N, 64 * ni), (unsigned)ceil_div(a.M, 64 * mi));
  if (mi == 2) dense_launch<F, 2, 2, EPI, WKN>(grid, st, form, a);
  else if (ni == 2) dense_launch<F, 1, 2, EPI, WKN>(grid, st, form, a);
  else dense_launch<F, 1, 1, EPI, WKN>(grid, st, form, a);
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

// The weight gradient on a pair of forms, m >= 1 rows: the split rule of dense_wgrad_split_len(m, n, k); `part` holds
// dense_wgrad_partial_bytes of it (unused with one split).
template <class F, class GF, class XF>
void dense_wgrad_launch(const GF &gf, const XF &xf, int64_t m, int n, int k, float *dW, float *part, hipStream_t st) {
  int splits;
  const int64_t len = dense_wgrad_split_len(m, n, k, &splits);
  const dim3 grid((unsigned)ceil_div(k, kDenseDwTile), (unsigned)ceil_div(n, kDenseDwTile), (unsigned)splits);
  dense_wgrad_kernel<F, GF, XF><<<grid, 256, 0, st>>>(gf, xf, m, n, k, len, part, dW);
  if (splits > 1) dense_wgrad_reduce(part, splits, (int64_t)n * k / 4, dW, st);
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
  dense_wgrad_split_len(m, n, k, &splits);
  const size_t need = dense_wgrad_partial_bytes(splits, n, k);
  if (need > 0 && (!workspace || workspace_bytes < need)) return workspace_short(me, workspace_bytes, need);
  dense_wgrad_launch<F>(DenseRows{G, n}, DenseRows{X, k}, m, n, k, dW, (float *)workspace, st);
  return check_launch(me);
}

// ---------------------------------------------------------------------------------------
// host: the training forms of the patch embedding and the tap stems (include/ftx.h states the contracts).  Each entry validates all
// of its arguments, its workspace included, before its first launch; the pieces of a workspace start on 256-byte boundaries.
// ---------------------------------------------------------------------------------------
// dpos (t0 + g, dim) = the sum over the frames, ascending, of dtokens (b, t0 + g, dim); rows 0 and 1 also to dcls and ddist
void dense_frames_sum(const float *dtokens, int b, int t0, int g, int dim, float *dpos, float *dcls, float *ddist, hipStream_t st);
// gm (m, n) = g where y > 0, else 0: DenseReluMaskedRows, materialised
void dense_relu_mask(const float *g, const float *y, int64_t elems, float *gm, hipStream_t st);
// dtokens (b, t0 + g, dim): rows t0.. of every frame from src (b g, dim), the t0 leading rows zero
void dense_strip_store(const float *src, int b, int t0, int g, int dim, float *dtokens, hipStream_t st);

struct PatchBwdWorkspace {
  int64_t partial, colsum, end;
};
inline PatchBwdWorkspace dense_patch_bwd_workspace(int64_t b, int64_t g, int dim, int k) {
  Offsets256 o;
  int splits;
  dense_wgrad_split_len(b * g, dim, k, &splits);
  PatchBwdWorkspace w;
  w.partial = o.take((int64_t)dense_wgrad_partial_bytes(splits, dim, k));
  w.colsum = o.take((int64_t)ftx_colsum_workspace_bytes(g, dim));
  w.end = o.end > 256 ? o.end : 256;
  return w;
}
size_t dense_patch_bwd_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t p, int32_t dim);

// ftx_vit_patch_embed_bwd_<family>
template <class F>
int dense_patch_embed_bwd_entry(const float *dtokens, const float *img, const float *W, int32_t b, int32_t c, int32_t h, int32_t w, int32_t p,
                                int32_t dim, int32_t t0, float *dW, float *dbias, float *dcls, float *ddist, float *dpos, float *dimg,
                                void *workspace, size_t workspace_bytes, void *stream) {
  const char *me = F::patch_bwd_name;
  FTX_REQUIRE(b >= 1 && c >= 1 && h >= 1 && w >= 1 && p >= 1 && dim >= 4, "%s: bad size (b=%d c=%d h=%d w=%d patch=%d dim=%d)", me, b, c, h, w, p, dim);
  FTX_REQUIRE(t0 == 1 || t0 == 2, "%s: t0 must be 1 or 2 (t0=%d)", me, t0);
  FTX_REQUIRE(p % 4 == 0, "%s: patch must be a multiple of 4 (patch=%d)", me, p);
  FTX_REQUIRE(h % p == 0 && w % p == 0, "%s: the image must be whole patches (h=%d w=%d patch=%d)", me, h, w, p);
  FTX_REQUIRE(dim % 4 == 0, "%s: dim must be a multiple of 4 (dim=%d)", me, dim);
  const int64_t k = (int64_t)c * p * p, g = (int64_t)(h / p) * (w / p);
  FTX_REQUIRE(k % kDenseGranule == 0, "%s: c * patch * patch must be a multiple of %d (%lld)", me, kDenseGranule, (long long)k);
  FTX_REQUIRE(!dimg || dim % kDenseGranule == 0, "%s: dim must be a multiple of %d for the image gradient (dim=%d)", me, kDenseGranule, dim);
  FTX_REQUIRE((int64_t)b * g <= 0x7fffffff / 2 && k * dim <= 0x7fffffff / 8 && (int64_t)b * c * h * w <= 0x7fffffff && (g + t0) * dim <= 0x7fffffff,
              "%s: too large", me);
  FTX_REQUIRE(dtokens && img && dW && dbias && dcls && dpos && workspace, "%s: null pointer", me);
  FTX_REQUIRE(ddist || t0 == 1, "%s: null pointer (ddist with t0 = 2)", me);
  FTX_REQUIRE(W || !dimg, "%s: null pointer (W with dimg)", me);
  FTX_REQUIRE(aligned16(dtokens) && aligned16(img) && aligned16(W) && aligned16(dW) && aligned16(dbias) && aligned16(dcls) && aligned16(ddist) &&
                  aligned16(dpos) && aligned16(dimg) && aligned16(workspace),
              "%s: pointers must be 16-byte aligned", me);
  const PatchBwdWorkspace ws = dense_patch_bwd_workspace(b, g, dim, (int)k);
  if (workspace_bytes < (size_t)ws.end) return workspace_short(me, workspace_bytes, (size_t)ws.end);
  const hipStream_t st = (hipStream_t)stream;
  char *base = (char *)workspace;
  const int64_t m = (int64_t)b * g;
  // dW = dY^T unfold(img): G the strip rows of dtokens, X the unfold
  const DenseTapRows gform = {dtokens, nullptr, nullptr, nullptr, nullptr, 0.f, dim, (int)g, t0};
  const DensePatches xform = {img, nullptr, c, h, w, p, w / p, (int)g, t0};
  dense_wgrad_launch<F>(gform, xform, m, dim, (int)k, dW, (float *)(base + ws.partial), st);
  // dpos, dcls, ddist, then dbias = the column sums of dpos' patch rows
  dense_frames_sum(dtokens, b, t0, (int)g, dim, dpos, dcls, ddist, st);
  const int rc = ftx_colsum(dpos + (int64_t)t0 * dim, g, dim, dbias, base + ws.colsum, (size_t)(ws.end - ws.colsum), stream);
  if (rc != FTX_OK) return rc;
  if (dimg) {   // dimg = fold(dY W)
    const DenseStripFold form = {dtokens, dim, c, h, w, p, w / p, (int)g, t0};
    const DenseGemmArgs a = {nullptr, W, nullptr, nullptr, m, (int)k, dim, dimg, nullptr};
    dense_launch_form<F, DenseStripFold, FTX_EPI_NONE, true>(form, a, st);
  }
  return check_launch(me);
}

// ftx_vit_tap_stem_train_fwd_<family>: rows (b g, co) = ReLU(tokens[:, t0:] W^T + bias)
template <class F>
int dense_tap_stem_train_fwd_entry(const float *tokens, const float *W, const float *bias, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co,
                                   float *rows, void *stream) {
  const char *me = F::tap_fwd_name;
  FTX_REQUIRE(b >= 0 && g >= 1 && dim >= kDenseGranule && co >= 4, "%s: bad size (b=%d g=%d dim=%d co=%d)", me, b, g, dim, co);
  FTX_REQUIRE(t0 >= 0 && t0 <= 2, "%s: t0 must be 0, 1 or 2 (t0=%d)", me, t0);
  FTX_REQUIRE(dim % kDenseGranule == 0, "%s: dim must be a multiple of %d (dim=%d)", me, kDenseGranule, dim);
  FTX_REQUIRE(co % 4 == 0, "%s: co must be a multiple of 4 (co=%d)", me, co);
  FTX_REQUIRE((int64_t)b * (g + t0) <= 0x7fffffff / 2 && (int64_t)co * dim <= 0x7fffffff, "%s: too large", me);
  if (b == 0) return FTX_OK;
  FTX_REQUIRE(tokens && W && bias && rows, "%s: null pointer", me);
  FTX_REQUIRE(aligned16(tokens) && aligned16(W) && aligned16(bias) && aligned16(rows), "%s: pointers must be 16-byte aligned", me);
  const DenseTapReluRows form = {tokens, dim, g, t0};
  const DenseGemmArgs a = {nullptr, W, bias, nullptr, (int64_t)b * g, co, dim, rows, nullptr};
  dense_launch_form<F>(form, a, (hipStream_t)stream);
  return check_launch(me);
}

struct TapBwdWorkspace {
  int64_t masked, product, partial, colsum, end;
};
inline TapBwdWorkspace dense_tap_bwd_workspace(int64_t b, int64_t g, int dim, int co) {
  Offsets256 o;
  int splits;
  dense_wgrad_split_len(b * g, co, dim, &splits);
  TapBwdWorkspace w;
  w.masked = o.take((int64_t)sizeof(float) * b * g * co);
  w.product = o.take((int64_t)sizeof(float) * b * g * dim);
  w.partial = o.take((int64_t)dense_wgrad_partial_bytes(splits, co, dim));
  w.colsum = o.take((int64_t)ftx_colsum_workspace_bytes(b * g, co));
  w.end = o.end > 256 ? o.end : 256;
  return w;
}
size_t dense_tap_bwd_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co);

// ftx_vit_tap_stem_bwd_<family>
template <class F>
int dense_tap_stem_bwd_entry(const float *drows, const float *rows, const float *tokens, const float *W, int32_t b, int32_t g, int32_t t0, int32_t dim,
                             int32_t co, float *dW, float *dbias, float *dtokens, void *workspace, size_t workspace_bytes, void *stream) {
  const char *me = F::tap_bwd_name;
  FTX_REQUIRE(b >= 1 && g >= 1 && dim >= kDenseGranule && co >= 4, "%s: bad size (b=%d g=%d dim=%d co=%d)", me, b, g, dim, co);
  FTX_REQUIRE(t0 >= 0 && t0 <= 2, "%s: t0 must be 0, 1 or 2 (t0=%d)", me, t0);
  FTX_REQUIRE(dim % kDenseGranule == 0, "%s: dim must be a multiple of %d (dim=%d)", me, kDenseGranule, dim);
  FTX_REQUIRE(co % 4 == 0, "%s: co must be a multiple of 4 (co=%d)", me, co);
  FTX_REQUIRE((int64_t)b * (g + t0) <= 0x7fffffff / 2 && (int64_t)co * dim <= 0x7fffffff / 8 && (int64_t)b * (g + t0) * dim <= ((int64_t)1 << 40),
              "%s: too large", me);
  FTX_REQUIRE(drows && rows && tokens && W && dW && dbias && dtokens && workspace, "%s: null pointer", me);
  FTX_REQUIRE(aligned16(drows) && aligned16(rows) && aligned16(tokens) && aligned16(W) && aligned16(dW) && aligned16(dbias) && aligned16(dtokens) &&
                  aligned16(workspace),
              "%s: pointers must be 16-byte aligned", me);
  const TapBwdWorkspace ws = dense_tap_bwd_workspace(b, g, dim, co);
  if (workspace_bytes < (size_t)ws.end) return workspace_short(me, workspace_bytes, (size_t)ws.end);
  const hipStream_t st = (hipStream_t)stream;
  char *base = (char *)workspace;
  const int64_t m = (int64_t)b * g;
  float *gm = (float *)(base + ws.masked), *prod = (float *)(base + ws.product);
  // dW = (masked drows)^T tokens[:, t0:]: the mask in G's load, the strip in X's rows
  const DenseReluMaskedRows gform = {drows, rows, co};
  const DenseTapRows xform = {tokens, nullptr, nullptr, nullptr, nullptr, 0.f, dim, g, t0};
  dense_wgrad_launch<F>(gform, xform, m, co, dim, dW, (float *)(base + ws.partial), st);
  // the masked gradient once in memory: dbias = its column sums, and the rows GEMM reads it
  dense_relu_mask(drows, rows, m * co, gm, st);
  int rc = ftx_colsum(gm, m, co, dbias, base + ws.colsum, (size_t)(ws.end - ws.colsum), stream);
  if (rc != FTX_OK) return rc;
  // dtokens[:, t0:] = masked drows . W  (reduction co: the rows GEMM, which takes any multiple of 4), then the strip store
  rc = F::rows_gemm(gm, m, W, 0, nullptr, co, dim, prod, stream);
  if (rc != FTX_OK) return rc;
  dense_strip_store(prod, b, t0, g, dim, dtokens, st);
  return check_launch(me);
}

}  // namespace ftx
