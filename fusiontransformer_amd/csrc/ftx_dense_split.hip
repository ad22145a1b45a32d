// fp32-accurate dense GEMMs of the ViT trunk's Linears (qkv, proj, fc1, fc2) on the bf16 MFMA: every fp32 operand is split into three
// bf16 pieces as it is staged and six of the nine piece products are summed in fp32 (vit_linear_impl = "ftx_split").  The forward /
// data-gradient GEMM with the bf16 kernels' fused bias and GELU epilogues, and the weight gradient, on v_mfma_f32_32x32x16_bf16.
//
// Precision contract (include/ftx.h states it for callers):
//   split     x -> h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), round-to-nearest-even, both subtractions in fp32 (exact).
//             x == h + m + l for finite |x| < 2^127 whose pieces stay at or above 2^-126; h not finite: m = l = 0.
//   products  hh, hm, mh, hl, lh, mm (first letter: the A / dY piece).  ml, lm, ll are dropped: each below 2.01 * 2^-24 |a b|.
//   order     TWO accumulators per output element (the form that shipped): `hh` takes the hh products alone, k ascending; `corr` takes,
//             per 16-wide k-step, mm, hl, lh, hm, mh in that order (smallest first).  out = hh + corr, one fp32 add after the last k-step,
//             then bias / GELU / GELU derivative by dense_epilogue (ftx_dense_common.h).  The corrections are 2^-8 of the result and smaller, so
//             their chain's rounding is far below the hh chain's, which is that of a bf16-operand GEMM's fp32 accumulator.
//             No atomics; the partial tiles of a split weight gradient are added by dense_wgrad_reduce_kernel in split order.
//
// LDS: three bf16 images per operand.  The stage is 32 reduction elements deep with a 40-element (80 B) row stride: 6 x 128 x 80 B
// = 61 440 B at the 128 x 128 tile, under the 64 KB a static __shared__ array may take without a function attribute, two blocks per CU.
// (The 64-deep stage of the bf16 kernels would need 110 592 B.)  80 B rows keep the ds_read_b128 fragment reads conflict-free: the 16
// rows of a quarter wave start at 16 distinct multiples of four banks.  __launch_bounds__(256, 2) keeps the 128 x 128 kernels at or
// under 256 registers so that two blocks do share a CU (measured: 13 % less time per block of Linears at batch 4 than one block per CU).
//
// The operand maps are those of ftx_dense_bf16.hip: lane (r = lane & 31, h = lane >> 5) holds row r, k = 8h + j of
// both fragments of a 16-wide k-step; mfma(F1, F2) leaves C[row of F1][row of F2] with F2's row on the lane and four consecutive F1
// rows in accumulator registers 4q..4q+3, so every store is a float4 along the output row.
//
// The epilogue, the tile and split rules and the host layer are shared with ftx_dense_bf16.hip: ftx_dense_common.h.
#include "ftx_dense_common.h"

using namespace ftx;

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

constexpr int DS_BK = 32;       // reduction elements staged per step: two k-steps of 16
constexpr int DS_STRIDE = 40;   // bf16 per LDS row (80 B): conflict-free ds_read_b128
static_assert(kDenseGranule % DS_BK == 0, "the entry admits every multiple of kDenseGranule as the reduction");

}  // namespace

// ---------------------------------------------------------------------------------------
// out[m][n] = epilogue( sum_k A[m][k] B[k][n] ) with the six-product split,  B = W^T with W stored [N][K] (WKN = false: nn.Linear's
// weight, the forward) or B = W stored [K][N] (WKN = true: the data gradient dX = dY W).
//
// Block = 4 waves as 2 x 2, tile (64 MI) x (64 NI); wave (wm, wn) owns MI x NI 32 x 32 sub-tiles.  Three LDS images per operand,
// [piece][row][k] bf16; the next step's global loads are issued before this step's MFMAs (register staging).
// Rows past M and columns past N load clamped, always-valid addresses and are never stored.
// AF (ftx_dense_common.h) says where A's rows live and what the epilogue does: DenseRows is the (M, K) matrix with dense_epilogue<EPI>,
// DensePatches the patch embedding's unfold of an image, DenseTapRows the token buffer behind its leading rows.  Nothing else here
// depends on it, so every form sums the same products in the same order.
// ---------------------------------------------------------------------------------------
template <int MI, int NI, int EPI, bool WKN, class AF>
__global__ __launch_bounds__(256, 2) void dense_gemm_split_kernel(const AF af, const float *__restrict__ W, const float *__restrict__ bias,
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
    arow[p] = af.row(r < M ? r : M - 1);
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
        af.template store<EPI>(make_float4(hh[i][j][4 * q] + corr[i][j][4 * q], hh[i][j][4 * q + 1] + corr[i][j][4 * q + 1],
                                           hh[i][j][4 * q + 2] + corr[i][j][4 * q + 2], hh[i][j][4 * q + 3] + corr[i][j][4 * q + 3]),
                               m, n, N, bias, pre_in, out, pre_out);
      }
  }
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[n][k] = sum_m G[m][n] X[m][k] with the six-product split (G = dY [M][N], X [M][K], both row-major over the
// reduction index m; first piece letter: G's)
//
// Block = (128-column tile of k, 128-row tile of n, split s of the rows); 4 waves as 2 x 2, each 64 x 64.  Each step stages DSW_BR rows:
// float4 loads along the channels, split, and stored TRANSPOSED as m-contiguous bf16 images [piece][channel][m] with two rows packed per
// 32-bit LDS write (the register stage of dense_wgrad_bf16_kernel).  Rows past the split are zeroed on the block-uniform last step.
// A split count of 1 writes dW directly; otherwise each split writes its own (N x K) partial and dense_wgrad_reduce_kernel adds them.
// ---------------------------------------------------------------------------------------
constexpr int DSW_BR = 32;    // rows (reduction) staged per step: two k-steps of 16
constexpr int DSW_T = kDenseDwTile;

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

struct DenseSplit {
  static constexpr const char *gemm_name = "ftx_dense_gemm_split", *wgrad_name = "ftx_dense_wgrad_split";
  static constexpr const char *patch_name = "ftx_vit_patch_embed_split", *tap_name = "ftx_vit_tap_stem_split";
  template <int MI, int NI, int EPI, bool WKN, class AF>
  static void gemm(dim3 grid, hipStream_t st, const AF &af, const DenseGemmArgs &a) {
    dense_gemm_split_kernel<MI, NI, EPI, WKN, AF><<<grid, 256, 0, st>>>(af, a.W, a.bias, a.pre_in, a.M, a.N, a.K, a.out, a.pre_out);
  }
  static void wgrad(dim3 grid, hipStream_t st, const float *G, const float *X, int64_t M, int N, int K, int64_t len, float *part, float *dW) {
    dense_wgrad_split_kernel<<<grid, 256, 0, st>>>(G, X, M, N, K, len, part, dW);
  }
};

extern "C" int ftx_dense_gemm_split(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n,
                                    int32_t k, int32_t epilogue, float *out, float *pre_out, void *stream) {
  return dense_gemm_entry<DenseSplit>(A, W, w_kn, bias, pre_in, m, n, k, epilogue, out, pre_out, stream);
}

extern "C" int ftx_vit_patch_embed_split(const float *img, const float *W, const float *bias, const float *cls, const float *dist, const float *pos,
                                       int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *tokens, void *stream) {
  return dense_patch_embed_entry<DenseSplit>(img, W, bias, cls, dist, pos, b, c, h, w, patch, dim, t0, tokens, stream);
}

extern "C" int ftx_vit_tap_stem_split(const float *tokens, const float *W, const float *bias, const float *gamma, const float *beta,
                                    const float *running_mean, const float *running_var, float eps, int32_t b, int32_t g, int32_t t0, int32_t dim,
                                    int32_t co, float *out, void *stream) {
  return dense_tap_stem_entry<DenseSplit>(tokens, W, bias, gamma, beta, running_mean, running_var, eps, b, g, t0, dim, co, out, stream);
}

extern "C" size_t ftx_dense_wgrad_split_workspace_bytes(int64_t m, int32_t n, int32_t k) { return dense_wgrad_workspace_bytes(m, n, k); }

extern "C" int ftx_dense_wgrad_split(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  return dense_wgrad_entry<DenseSplit>(G, X, m, n, k, dW, workspace, workspace_bytes, stream);
}

extern "C" int ftx_dense_split_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  return dense_tile_entry("ftx_dense_split_tile", form, m, n, k, tile_m_host, tile_n_host, split_host);
}
