// fp32-accurate dense GEMMs of the ViT trunk's Linears (qkv, proj, fc1, fc2) on the bf16 MFMA: every fp32 operand is split into three
// bf16 pieces as it is staged and six of the nine piece products are summed in fp32 (vit_linear_impl = "ftx_split").  The forward /
// data-gradient GEMM with the bf16 kernels' fused bias and GELU epilogues, and the weight gradient, on v_mfma_f32_32x32x16_bf16.
//
// Precision contract (include/ftx.h states it for callers):
//   split     x -> h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), round-to-nearest-even, both subtractions in fp32 (exact).
//             x == h + m + l for finite |x| < 2^127 whose pieces stay at or above 2^-126; h not finite: m = l = 0.
//   products  hh, hm, mh, hl, lh, mm (first letter: the A / dY piece).  ml, lm, ll are dropped: each below 2.01 * 2^-24 |a b|.
//   order     TWO accumulators per output element (the form that shipped): `hh` takes the hh products alone, k ascending; `corr` takes,
//             per 16-wide k-step, mm, hl, lh, hm, mh in that order (smallest first).  out = hh + corr, one fp32 add in the epilogue,
//             then bias / GELU / GELU derivative exactly as ftx_dense_bf16.hip.  The corrections are 2^-8 of the result and smaller, so
//             their chain's rounding is far below the hh chain's, which is that of a bf16-operand GEMM's fp32 accumulator.
//             No atomics; the partial tiles of a split weight gradient are added by dense_split_reduce_kernel in split order.
//
// LDS: three bf16 images per operand.  The stage is 32 reduction elements deep with a 40-element (80 B) row stride: 6 x 128 x 80 B
// = 61 440 B at the 128 x 128 tile, under the 64 KB a static __shared__ array may take without a function attribute, two blocks per CU.
// (The 64-deep stage of the bf16 kernels would need 110 592 B.)  80 B rows keep the ds_read_b128 fragment reads conflict-free: the 16
// rows of a quarter wave start at 16 distinct multiples of four banks.  __launch_bounds__(256, 2) keeps the 128 x 128 kernels at or
// under 256 registers so that two blocks do share a CU (measured: 13 % less time per block of Linears at batch 4 than one block per CU).
//
// Operand maps, tiles and the epilogue are those of ftx_dense_bf16.hip: lane (r = lane & 31, h = lane >> 5) holds row r, k = 8h + j of
// both fragments of a 16-wide k-step; mfma(F1, F2) leaves C[row of F1][row of F2] with F2's row on the lane and four consecutive F1
// rows in accumulator registers 4q..4q+3, so every store is a float4 along the output row.
#include "ftx_common.h"

using namespace ftx;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

namespace {

struct Pieces4 {
  bf16x4 h, m, l;
};

// the ONE definition of the split: h + m + l == x for finite x in range; h = inf / NaN keeps m = l = 0
__device__ inline void split1(float x, __bf16 &h, __bf16 &m, __bf16 &l) {
  h = (__bf16)x;
  const float hf = (float)h;
  const bool finite = (__float_as_uint(hf) & 0x7f800000u) != 0x7f800000u;
  const float r = finite ? x - hf : 0.f;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

__device__ inline Pieces4 split4(float4 v) {
  Pieces4 p;
  __bf16 h, m, l;
  split1(v.x, h, m, l); p.h[0] = h; p.m[0] = m; p.l[0] = l;
  split1(v.y, h, m, l); p.h[1] = h; p.m[1] = m; p.l[1] = l;
  split1(v.z, h, m, l); p.h[2] = h; p.m[2] = m; p.l[2] = l;
  split1(v.w, h, m, l); p.h[3] = h; p.m[3] = m; p.l[3] = l;
  return p;
}

__device__ inline f32x16 mfma_bf16(const bf16x8 &a, const bf16x8 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// nn.GELU() (approximate="none") and its derivative, in fp32: the expressions of ftx_dense_bf16.hip
__device__ inline float gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ inline float dgelu(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * (0.39894228040143268f * expf(-0.5f * x * x));
}

constexpr int DS_BK = 32;       // reduction elements staged per step: two k-steps of 16
constexpr int DS_STRIDE = 40;   // bf16 per LDS row (80 B): conflict-free ds_read_b128
constexpr int DS_KALIGN = 64;   // the reduction must be a multiple of this (the bf16 twins' rule, kept so both take the same shapes)

}  // namespace

// ---------------------------------------------------------------------------------------
// out[m][n] = epilogue( sum_k A[m][k] B[k][n] ) with the six-product split,  B = W^T with W stored [N][K] (WKN = false: nn.Linear's
// weight, the forward) or B = W stored [K][N] (WKN = true: the data gradient dX = dY W).
//
// Block = 4 waves as 2 x 2, tile (64 MI) x (64 NI); wave (wm, wn) owns MI x NI 32 x 32 sub-tiles.  Three LDS images per operand,
// [piece][row][k] bf16; the next step's global loads are issued before this step's MFMAs (register staging).
// Rows past M and columns past N load clamped, always-valid addresses and are never stored.
// ---------------------------------------------------------------------------------------
template <int MI, int NI, int EPI, bool WKN>
__global__ __launch_bounds__(256, 2) void dense_gemm_split_kernel(const float *__restrict__ A, const float *__restrict__ W, const float *__restrict__ bias,
                                                               const float *__restrict__ pre_in, int64_t M, int N, int K, float *__restrict__ out,
                                                               float *__restrict__ pre_out) {
  constexpr int BM = 64 * MI, BN = 64 * NI;
  constexpr int AP = BM / 32;   // float4 of A per thread and step: 32 rows x 8 float4 per pass
  constexpr int BP = BN / 32;   // the same count for B in either orientation
  constexpr int AIMG = BM * DS_STRIDE, BIMG = BN * DS_STRIDE;
  __shared__ __attribute__((aligned(16))) __bf16 As[3 * AIMG];   // [piece h, m, l][m][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * BIMG];   // [piece h, m, l][n][k]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  // row-major staging (A, and W stored [N][K]): pass p covers rows 32p .. 32p+31, thread -> (row tid/8, float4 tid%8)
  const int srow = tid >> 3, sk4 = (tid & 7) * 4;
  const float *arow[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    int64_t r = m0 + p * 32 + srow;
    arow[p] = A + (r < M ? r : M - 1) * K + sk4;
  }
  const float *brow[BP];
  // WKN: item e = (k pair kp, column float4 n4); two float4 per item (rows 2kp, 2kp+1), stored as packed k pairs
  int bkp[WKN ? BN / 64 : 1], bn4[WKN ? BN / 64 : 1];
  if constexpr (!WKN) {
#pragma unroll
    for (int p = 0; p < BP; ++p) {
      int r = n0 + p * 32 + srow;
      brow[p] = W + (int64_t)(r < N ? r : N - 1) * K + sk4;
    }
  } else {
#pragma unroll
    for (int q = 0; q < BN / 64; ++q) {
      const int e = q * 256 + tid;
      bn4[q] = (e % (BN / 4)) * 4;
      bkp[q] = e / (BN / 4);   // 0 .. 15
      int n = n0 + bn4[q];
      brow[2 * q] = W + (int64_t)(2 * bkp[q]) * N + (n + 4 <= N ? n : N - 4);
      brow[2 * q + 1] = brow[2 * q] + N;
    }
  }

  f32x16 hh[MI][NI], corr[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) hh[i][j][g] = corr[i][j][g] = 0.f;

  float4 ra[AP], rb[BP];
  auto load_step = [&](int c0) {
#pragma unroll
    for (int p = 0; p < AP; ++p) ra[p] = *(const float4 *)(arow[p] + c0);
    if constexpr (!WKN) {
#pragma unroll
      for (int p = 0; p < BP; ++p) rb[p] = *(const float4 *)(brow[p] + c0);
    } else {
#pragma unroll
      for (int p = 0; p < BP; ++p) rb[p] = *(const float4 *)(brow[p] + (int64_t)c0 * N);
    }
  };
  // the ONE place the operands are split: fp32 registers -> three bf16 LDS images
  auto store_step = [&]() {
#pragma unroll
    for (int p = 0; p < AP; ++p) {
      const Pieces4 s = split4(ra[p]);
      const int o = (p * 32 + srow) * DS_STRIDE + sk4;
      *(bf16x4 *)&As[o] = s.h;
      *(bf16x4 *)&As[AIMG + o] = s.m;
      *(bf16x4 *)&As[2 * AIMG + o] = s.l;
    }
    if constexpr (!WKN) {
#pragma unroll
      for (int p = 0; p < BP; ++p) {
        const Pieces4 s = split4(rb[p]);
        const int o = (p * 32 + srow) * DS_STRIDE + sk4;
        *(bf16x4 *)&Bs[o] = s.h;
        *(bf16x4 *)&Bs[BIMG + o] = s.m;
        *(bf16x4 *)&Bs[2 * BIMG + o] = s.l;
      }
    } else {
#pragma unroll
      for (int q = 0; q < BN / 64; ++q) {
        const Pieces4 x0 = split4(rb[2 * q]), x1 = split4(rb[2 * q + 1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = (bn4[q] + e) * DS_STRIDE + 2 * bkp[q];
          *(bf16x2 *)&Bs[o] = (bf16x2){x0.h[e], x1.h[e]};
          *(bf16x2 *)&Bs[BIMG + o] = (bf16x2){x0.m[e], x1.m[e]};
          *(bf16x2 *)&Bs[2 * BIMG + o] = (bf16x2){x0.l[e], x1.l[e]};
        }
      }
    }
  };

  const __bf16 *ap = &As[(wm * 32 * MI + l31) * DS_STRIDE + 8 * half];
  const __bf16 *bp = &Bs[(wn * 32 * NI + l31) * DS_STRIDE + 8 * half];
  load_step(0);
  for (int c0 = 0; c0 < K; c0 += DS_BK) {
    store_step();
    __syncthreads();
    if (c0 + DS_BK < K) load_step(c0 + DS_BK);   // the next step's global loads fly under this step's MFMAs
#pragma unroll
    for (int s = 0; s < DS_BK / 16; ++s) {
      bf16x8 af[3][MI], bf[3][NI];   // [piece h, m, l]
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[c][i] = *(const bf16x8 *)(ap + c * AIMG + i * 32 * DS_STRIDE + 16 * s);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf[c][j] = *(const bf16x8 *)(bp + c * BIMG + j * 32 * DS_STRIDE + 16 * s);
      }
      // (A piece, B piece) in the documented order: the five corrections smallest first, then hh into its own accumulator.
      // rows: n, columns (lanes): m.  The MI x NI sub-tiles between two uses of one accumulator hide the MFMA's latency.
      constexpr int ORDER[5][2] = {{1, 1}, {0, 2}, {2, 0}, {0, 1}, {1, 0}};   // mm, hl, lh, hm, mh
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) corr[i][j] = mfma_bf16(bf[ORDER[t][1]][j], af[ORDER[t][0]][i], corr[i][j]);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) hh[i][j] = mfma_bf16(bf[0][j], af[0][i], hh[i][j]);
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
        float4 v = make_float4(hh[i][j][4 * q] + corr[i][j][4 * q], hh[i][j][4 * q + 1] + corr[i][j][4 * q + 1],
                               hh[i][j][4 * q + 2] + corr[i][j][4 * q + 2], hh[i][j][4 * q + 3] + corr[i][j][4 * q + 3]);
        const int64_t o = m * N + n;
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
  }
}

// Tile per shape: the largest of 128 x 128, 64 x 128, 64 x 64 that still gives one block per CU (256 tiles); else 64 x 64 (the bf16
// kernels' rule).  A function of the shape alone; ftx_dense_split_tile reports it.
constexpr int DENSE_SPLIT_CUS = 256;   // MI355X; a constant of the tiling, not a device query
static void split_gemm_tile(int64_t M, int N, int *mi, int *ni) {
  static const int cand[3][2] = {{2, 2}, {1, 2}, {1, 1}};
  for (const auto &c : cand) {
    if (ceil_div(M, 64 * c[0]) * ceil_div(N, 64 * c[1]) >= DENSE_SPLIT_CUS) {
      *mi = c[0];
      *ni = c[1];
      return;
    }
  }
  *mi = 1;
  *ni = 1;
}

template <int MI, int NI, bool WKN>
static void launch_split_epi(int epi, dim3 grid, hipStream_t st, const float *A, const float *W, const float *bias, const float *pre_in, int64_t M, int N,
                             int K, float *out, float *pre_out) {
  switch (epi) {
    case FTX_EPI_NONE: dense_gemm_split_kernel<MI, NI, FTX_EPI_NONE, WKN><<<grid, 256, 0, st>>>(A, W, bias, pre_in, M, N, K, out, pre_out); break;
    case FTX_EPI_BIAS: dense_gemm_split_kernel<MI, NI, FTX_EPI_BIAS, WKN><<<grid, 256, 0, st>>>(A, W, bias, pre_in, M, N, K, out, pre_out); break;
    case FTX_EPI_BIAS_GELU: dense_gemm_split_kernel<MI, NI, FTX_EPI_BIAS_GELU, WKN><<<grid, 256, 0, st>>>(A, W, bias, pre_in, M, N, K, out, pre_out); break;
    default: dense_gemm_split_kernel<MI, NI, FTX_EPI_DGELU, WKN><<<grid, 256, 0, st>>>(A, W, bias, pre_in, M, N, K, out, pre_out); break;
  }
}

template <int MI, int NI>
static void launch_split(int w_kn, int epi, dim3 grid, hipStream_t st, const float *A, const float *W, const float *bias, const float *pre_in, int64_t M,
                         int N, int K, float *out, float *pre_out) {
  if (w_kn) launch_split_epi<MI, NI, true>(epi, grid, st, A, W, bias, pre_in, M, N, K, out, pre_out);
  else launch_split_epi<MI, NI, false>(epi, grid, st, A, W, bias, pre_in, M, N, K, out, pre_out);
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int ftx_dense_gemm_split(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n,
                                    int32_t k, int32_t epilogue, float *out, float *pre_out, void *stream) {
  FTX_REQUIRE(m >= 0 && n >= 4 && k >= DS_KALIGN, "ftx_dense_gemm_split: bad size (m=%lld n=%d k=%d)", (long long)m, n, k);
  FTX_REQUIRE(k % DS_KALIGN == 0, "ftx_dense_gemm_split: k must be a multiple of 64 (k=%d)", k);
  FTX_REQUIRE(n % 4 == 0, "ftx_dense_gemm_split: n must be a multiple of 4 (n=%d)", n);
  FTX_REQUIRE(w_kn == 0 || w_kn == 1, "ftx_dense_gemm_split: w_kn must be 0 or 1");
  FTX_REQUIRE(epilogue >= FTX_EPI_NONE && epilogue <= FTX_EPI_DGELU, "ftx_dense_gemm_split: unknown epilogue %d", epilogue);
  FTX_REQUIRE(m <= 0x7fffffff / 2 && (int64_t)n * k <= 0x7fffffff, "ftx_dense_gemm_split: too large");
  if (m == 0) return FTX_OK;
  FTX_REQUIRE(A && W && out, "ftx_dense_gemm_split: null pointer");
  FTX_REQUIRE(epilogue == FTX_EPI_NONE || epilogue == FTX_EPI_DGELU || bias, "ftx_dense_gemm_split: null pointer (bias)");
  FTX_REQUIRE(epilogue != FTX_EPI_BIAS_GELU || pre_out, "ftx_dense_gemm_split: null pointer (pre_out)");
  FTX_REQUIRE(epilogue != FTX_EPI_DGELU || pre_in, "ftx_dense_gemm_split: null pointer (pre_in)");
  FTX_REQUIRE(aligned16(A) && aligned16(W) && aligned16(out) && aligned16(bias) && aligned16(pre_in) && aligned16(pre_out),
              "ftx_dense_gemm_split: pointers must be 16-byte aligned");
  int mi, ni;
  split_gemm_tile(m, n, &mi, &ni);
  dim3 grid((unsigned)ceil_div(n, 64 * ni), (unsigned)ceil_div(m, 64 * mi));
  hipStream_t st = (hipStream_t)stream;
  if (mi == 2) launch_split<2, 2>(w_kn, epilogue, grid, st, A, W, bias, pre_in, m, n, k, out, pre_out);
  else if (ni == 2) launch_split<1, 2>(w_kn, epilogue, grid, st, A, W, bias, pre_in, m, n, k, out, pre_out);
  else launch_split<1, 1>(w_kn, epilogue, grid, st, A, W, bias, pre_in, m, n, k, out, pre_out);
  return check_launch("ftx_dense_gemm_split");
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[n][k] = sum_m G[m][n] X[m][k] with the six-product split (G = dY [M][N], X [M][K], both row-major over the
// reduction index m; first piece letter: G's)
//
// Block = (128-column tile of k, 128-row tile of n, split s of the rows); 4 waves as 2 x 2, each 64 x 64.  Each step stages DSW_BR rows:
// float4 loads along the channels, split, and stored TRANSPOSED as m-contiguous bf16 images [piece][channel][m] with two rows packed per
// 32-bit LDS write (the register stage of dense_wgrad_bf16_kernel).  Rows past the split are zeroed on the block-uniform last step.
// A split count of 1 writes dW directly; otherwise each split writes its own (N x K) partial and dense_split_reduce_kernel adds them.
// ---------------------------------------------------------------------------------------
constexpr int DSW_BR = 32;    // rows (reduction) staged per step: two k-steps of 16
constexpr int DSW_T = 128;    // dW tile side
constexpr int DSW_LEN = 64;   // a split's length is a multiple of this (the bf16 twin's rule)

__global__ __launch_bounds__(256, 2) void dense_wgrad_split_kernel(const float *__restrict__ G, const float *__restrict__ X, int64_t M, int N, int K,
                                                                int64_t split_len, float *__restrict__ part, float *__restrict__ dW) {
  constexpr int ITEMS = (DSW_BR / 2) * (DSW_T / 4) / 256;   // (row pair, float4) items per thread and operand: 2
  constexpr int IMG = DSW_T * DS_STRIDE;
  __shared__ __attribute__((aligned(16))) __bf16 Gt[3 * IMG];   // [piece][n][m]
  __shared__ __attribute__((aligned(16))) __bf16 Xt[3 * IMG];   // [piece][k][m]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;   // wm: k half, wn: n half
  const int k0 = blockIdx.x * DSW_T, n0 = blockIdx.y * DSW_T;
  const int64_t lo = (int64_t)blockIdx.z * split_len;
  const int64_t hi = lo + split_len < M ? lo + split_len : M;

  int rp[ITEMS], c4[ITEMS], gcol[ITEMS], xcol[ITEMS];
#pragma unroll
  for (int q = 0; q < ITEMS; ++q) {
    const int e = q * 256 + tid;
    c4[q] = (e % (DSW_T / 4)) * 4;
    rp[q] = e / (DSW_T / 4);   // 0 .. 15
    gcol[q] = n0 + c4[q] + 4 <= N ? n0 + c4[q] : N - 4;   // clamped columns reach only image rows that are never stored
    xcol[q] = k0 + c4[q] + 4 <= K ? k0 + c4[q] : K - 4;
  }

  f32x16 hh[2][2], corr[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) hh[i][j][g] = corr[i][j][g] = 0.f;

  float4 rg[ITEMS][2], rx[ITEMS][2];
  auto load_step = [&](int64_t r0) {
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int64_t r = r0 + 2 * rp[q] + h;
        r = r < M ? r : M - 1;
        rg[q][h] = *(const float4 *)&G[r * N + gcol[q]];
        rx[q][h] = *(const float4 *)&X[r * K + xcol[q]];
      }
  };
  auto store_step = [&](int64_t r0) {
    if (r0 + DSW_BR > hi) {   // block-uniform: the split's last step
#pragma unroll
      for (int q = 0; q < ITEMS; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (r0 + 2 * rp[q] + h >= hi) rg[q][h] = rx[q][h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the ONE place the operands are split
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
      const Pieces4 g0 = split4(rg[q][0]), g1 = split4(rg[q][1]);
      const Pieces4 x0 = split4(rx[q][0]), x1 = split4(rx[q][1]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int o = (c4[q] + e) * DS_STRIDE + 2 * rp[q];
        *(bf16x2 *)&Gt[o] = (bf16x2){g0.h[e], g1.h[e]};
        *(bf16x2 *)&Gt[IMG + o] = (bf16x2){g0.m[e], g1.m[e]};
        *(bf16x2 *)&Gt[2 * IMG + o] = (bf16x2){g0.l[e], g1.l[e]};
        *(bf16x2 *)&Xt[o] = (bf16x2){x0.h[e], x1.h[e]};
        *(bf16x2 *)&Xt[IMG + o] = (bf16x2){x0.m[e], x1.m[e]};
        *(bf16x2 *)&Xt[2 * IMG + o] = (bf16x2){x0.l[e], x1.l[e]};
      }
    }
  };

  const __bf16 *xp = &Xt[(wm * 64 + l31) * DS_STRIDE + 8 * half];
  const __bf16 *gp = &Gt[(wn * 64 + l31) * DS_STRIDE + 8 * half];
  load_step(lo);
  for (int64_t r0 = lo; r0 < hi; r0 += DSW_BR) {
    store_step(r0);
    __syncthreads();
    if (r0 + DSW_BR < hi) load_step(r0 + DSW_BR);
#pragma unroll
    for (int s = 0; s < DSW_BR / 16; ++s) {
      bf16x8 xf[3][2], gf[3][2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < 2; ++i) xf[c][i] = *(const bf16x8 *)(xp + c * IMG + i * 32 * DS_STRIDE + 16 * s);
#pragma unroll
        for (int j = 0; j < 2; ++j) gf[c][j] = *(const bf16x8 *)(gp + c * IMG + j * 32 * DS_STRIDE + 16 * s);
      }
      constexpr int ORDER[5][2] = {{1, 1}, {0, 2}, {2, 0}, {0, 1}, {1, 0}};   // (G piece, X piece): mm, hl, lh, hm, mh
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) corr[i][j] = mfma_bf16(xf[ORDER[t][1]][i], gf[ORDER[t][0]][j], corr[i][j]);   // rows: k, columns (lanes): n
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) hh[i][j] = mfma_bf16(xf[0][i], gf[0][j], hh[i][j]);
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
        if (k < K)
          *(float4 *)&dst[(int64_t)n * K + k] = make_float4(hh[i][j][4 * q] + corr[i][j][4 * q], hh[i][j][4 * q + 1] + corr[i][j][4 * q + 1],
                                                            hh[i][j][4 * q + 2] + corr[i][j][4 * q + 2], hh[i][j][4 * q + 3] + corr[i][j][4 * q + 3]);
      }
  }
}

// dW = part[0] + part[1] + ... + part[S-1], added in split order: a fixed summation order, bit-reproducible.
__global__ __launch_bounds__(256) void dense_split_reduce_kernel(const float *__restrict__ part, int splits, int64_t n4, float *__restrict__ dW) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    float4 s = ((const float4 *)part)[e];
    for (int t = 1; t < splits; ++t) {
      const float4 v = ((const float4 *)part)[t * n4 + e];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    ((float4 *)dW)[e] = s;
  }
}

// Splits of the rows: enough (N/128 x K/128 x S) blocks for one per CU, at least 256 rows per split, at most 8 splits; the split length
// a multiple of DSW_LEN.  A function of the shape alone; ftx_dense_split_tile reports it.
static int64_t split_wgrad_len(int64_t M, int N, int K, int *splits) {
  const int64_t tiles = ceil_div(N, DSW_T) * ceil_div(K, DSW_T);
  int64_t s = ceil_div(DENSE_SPLIT_CUS, tiles);
  int64_t cap = M / 256;
  if (cap > 8) cap = 8;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  int64_t len = ceil_div(ceil_div(M, s), DSW_LEN) * DSW_LEN;
  if (len < DSW_LEN) len = DSW_LEN;
  *splits = (int)ceil_div(M, len);
  if (*splits < 1) *splits = 1;
  return len;
}

extern "C" size_t ftx_dense_wgrad_split_workspace_bytes(int64_t m, int32_t n, int32_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return 256;
  int splits;
  split_wgrad_len(m, n, k, &splits);
  const size_t need = splits > 1 ? sizeof(float) * (size_t)splits * n * k : 0;
  return need > 256 ? need : 256;
}

extern "C" int ftx_dense_wgrad_split(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  FTX_REQUIRE(m >= 0 && n >= 4 && k >= 4, "ftx_dense_wgrad_split: bad size (m=%lld n=%d k=%d)", (long long)m, n, k);
  FTX_REQUIRE(n % 4 == 0 && k % 4 == 0, "ftx_dense_wgrad_split: n and k must be multiples of 4 (n=%d k=%d)", n, k);
  FTX_REQUIRE((int64_t)n * k <= 0x7fffffff / 8 && m <= 0x7fffffff / 2, "ftx_dense_wgrad_split: too large");
  FTX_REQUIRE(dW, "ftx_dense_wgrad_split: null pointer (dW)");
  FTX_REQUIRE(aligned16(dW) && aligned16(G) && aligned16(X) && aligned16(workspace), "ftx_dense_wgrad_split: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (m == 0) {
    if (hipMemsetAsync(dW, 0, sizeof(float) * (size_t)n * k, st) != hipSuccess) return check_launch("ftx_dense_wgrad_split memset");
    return FTX_OK;
  }
  FTX_REQUIRE(G && X, "ftx_dense_wgrad_split: null pointer");
  int splits;
  const int64_t len = split_wgrad_len(m, n, k, &splits);
  const size_t need = splits > 1 ? sizeof(float) * (size_t)splits * n * k : 0;
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("ftx_dense_wgrad_split: workspace %zu < required %zu", workspace_bytes, need);
    return FTX_EWORKSPACE;
  }
  float *part = (float *)workspace;
  dim3 grid((unsigned)ceil_div(k, DSW_T), (unsigned)ceil_div(n, DSW_T), (unsigned)splits);
  dense_wgrad_split_kernel<<<grid, 256, 0, st>>>(G, X, m, n, k, len, part, dW);
  if (splits > 1) {
    const int64_t n4 = (int64_t)n * k / 4;
    dense_split_reduce_kernel<<<grid_for(n4, 256), 256, 0, st>>>(part, splits, n4, dW);
  }
  return check_launch("ftx_dense_wgrad_split");
}

extern "C" int ftx_dense_split_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  FTX_REQUIRE(tile_m_host && tile_n_host && split_host, "ftx_dense_split_tile: null pointer");
  FTX_REQUIRE(m >= 1 && n >= 4 && k >= 4, "ftx_dense_split_tile: bad size (m=%lld n=%d k=%d)", (long long)m, n, k);
  if (form == 0) {
    int mi, ni;
    split_gemm_tile(m, n, &mi, &ni);
    *tile_m_host = 64 * mi;
    *tile_n_host = 64 * ni;
    *split_host = 1;
    return FTX_OK;
  }
  FTX_REQUIRE(form == 1, "ftx_dense_split_tile: form must be 0 (GEMM) or 1 (weight gradient)");
  int splits;
  split_wgrad_len(m, n, k, &splits);
  *tile_m_host = DSW_T;
  *tile_n_host = DSW_T;
  *split_host = splits;
  return FTX_OK;
}
