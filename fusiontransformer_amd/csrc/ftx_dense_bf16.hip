// bf16-operand dense GEMMs of the ViT trunk's Linears (qkv, proj, fc1, fc2): the forward / data-gradient GEMM with fused bias and GELU
// epilogues, and the weight gradient, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
//
// Precision contract (include/ftx.h states it for callers):
//   operands  A, W (GEMM) and dY, X (weight gradient) stay fp32 in HBM; each element is rounded to bf16 (round-to-nearest-even, a plain
//             cast: v_cvt_pk_bf16_f32, NaN stays NaN) from its stored value when it is written to LDS.
//   products  a bf16 x bf16 product is exact in fp32; the sums run in the MFMA's fp32 accumulators, k in ascending order per tile.
//   storage   out, the pre-activation and dW are fp32; bias, the GELU and its derivative are applied in fp32 to the fp32 sum.
//   order     no atomics; the partial tiles of a split weight gradient are added by dense_wgrad_reduce_kernel in split order.
//
// Operand maps (ftx_spconv_bf16.hip, cdna_hip_programming.md section 3): lane (r = lane & 31, h = lane >> 5) holds row r, k = 8h + j of
// both fragments of a 16-wide k-step, read with one ds_read_b128 from a bf16 LDS image whose rows are k-contiguous.  mfma(F1, F2)
// leaves C[row of F1][row of F2] with F2's row on the lane and four consecutive F1 rows in accumulator registers 4q..4q+3
// ((g&3) + 8(g>>2) + 4h), so every store below is a float4 along the output row.
//
// The epilogue, the tile and split rules and the host layer are shared with ftx_dense_split.hip: ftx_dense_common.h.  This file also
// holds the one definition of what that header only declares (the last section).
#include "ftx_dense_common.h"

using namespace ftx;

namespace {

__device__ inline bf16x4 round4(float4 v) { return (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w}; }

constexpr int DB_BK = 64;       // reduction elements staged per step: four k-steps of 16
constexpr int DB_STRIDE = 72;   // bf16 per LDS row (144 B): conflict-free ds_read_b128 (WB_STRIDE of ftx_spconv_bf16.hip)
static_assert(kDenseGranule % DB_BK == 0, "the entry admits every multiple of kDenseGranule as the reduction");

}  // namespace

// ---------------------------------------------------------------------------------------
// out[m][n] = epilogue( sum_k bf16(A[m][k]) bf16(B[k][n]) ),  B = W^T with W stored [N][K] (WKN = false: nn.Linear's weight, the
// forward) or B = W stored [K][N] (WKN = true: the data gradient dX = dY W).
//
// Block = 4 waves as 2 x 2, tile (64 MI) x (64 NI); wave (wm, wn) owns MI x NI 32 x 32 sub-tiles.  One LDS image per operand,
// [row][k] bf16; the next step's global loads are issued before this step's MFMAs (register staging, the pairs_gemm_bf16 pipeline).
// Rows past M and columns past N load clamped, always-valid addresses and are never stored.
// AF (ftx_dense_common.h) says where A's rows live and what the epilogue does: DenseRows is the (M, K) matrix with dense_epilogue<EPI>,
// DensePatches the patch embedding's unfold of an image, DenseTapRows the token buffer behind its leading rows.  Nothing else here
// depends on it, so every form sums the same products in the same order.
// ---------------------------------------------------------------------------------------
template <int MI, int NI, int EPI, bool WKN, class AF>
__global__ __launch_bounds__(256) void dense_gemm_bf16_kernel(const AF af, const float *__restrict__ W, const float *__restrict__ bias,
                                                              const float *__restrict__ pre_in, int64_t M, int N, int K, float *__restrict__ out,
                                                              float *__restrict__ pre_out) {
  constexpr int BM = 64 * MI, BN = 64 * NI;
  constexpr int AP = BM / 16;   // float4 of A per thread and step: 16 rows x 16 float4 per pass
  constexpr int BP = BN / 16;   // the same count for B in either orientation
  __shared__ __attribute__((aligned(16))) __bf16 As[BM * DB_STRIDE];   // [m][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[BN * DB_STRIDE];   // [n][k]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  // row-major staging (A, and W stored [N][K]): pass p covers rows 16p .. 16p+15, thread -> (row tid/16, float4 tid%16)
  const int srow = tid >> 4, sk4 = (tid & 15) * 4;
  const float *arow[AP];
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    int64_t r = m0 + p * 16 + srow;
    arow[p] = af.row(r < M ? r : M - 1);
  }
  const float *brow[BP];
  // WKN: item e = (k pair kp, column float4 n4); two float4 per item (rows 2kp, 2kp+1), stored as packed k pairs
  int bkp[WKN ? BN / 32 : 1], bn4[WKN ? BN / 32 : 1];
  if constexpr (!WKN) {
#pragma unroll
    for (int p = 0; p < BP; ++p) {
      int r = n0 + p * 16 + srow;
      brow[p] = W + (int64_t)(r < N ? r : N - 1) * K + sk4;
    }
  } else {
#pragma unroll
    for (int q = 0; q < BN / 32; ++q) {
      const int e = q * 256 + tid;
      bn4[q] = (e % (BN / 4)) * 4;
      bkp[q] = e / (BN / 4);
      int n = n0 + bn4[q];
      brow[2 * q] = W + (int64_t)(2 * bkp[q]) * N + (n + 4 <= N ? n : N - 4);
      brow[2 * q + 1] = brow[2 * q] + N;
    }
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;

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
  // the ONE place the operands are rounded: fp32 registers -> bf16 LDS images
  auto store_step = [&]() {
#pragma unroll
    for (int p = 0; p < AP; ++p) *(bf16x4 *)&As[(p * 16 + srow) * DB_STRIDE + sk4] = round4(ra[p]);
    if constexpr (!WKN) {
#pragma unroll
      for (int p = 0; p < BP; ++p) *(bf16x4 *)&Bs[(p * 16 + srow) * DB_STRIDE + sk4] = round4(rb[p]);
    } else {
#pragma unroll
      for (int q = 0; q < BN / 32; ++q) {
        const bf16x4 x0 = round4(rb[2 * q]), x1 = round4(rb[2 * q + 1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) *(bf16x2 *)&Bs[(bn4[q] + e) * DB_STRIDE + 2 * bkp[q]] = (bf16x2){x0[e], x1[e]};
      }
    }
  };

  const __bf16 *ap = &As[(wm * 32 * MI + l31) * DB_STRIDE + 8 * half];
  const __bf16 *bp = &Bs[(wn * 32 * NI + l31) * DB_STRIDE + 8 * half];
  load_step(0);
  for (int c0 = 0; c0 < K; c0 += DB_BK) {
    store_step();
    __syncthreads();
    if (c0 + DB_BK < K) load_step(c0 + DB_BK);   // the next step's global loads fly under this step's MFMAs
#pragma unroll
    for (int s = 0; s < DB_BK / 16; ++s) {
      bf16x8 af[MI], bf[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = *(const bf16x8 *)(ap + i * 32 * DB_STRIDE + 16 * s);
#pragma unroll
      for (int j = 0; j < NI; ++j) bf[j] = *(const bf16x8 *)(bp + j * 32 * DB_STRIDE + 16 * s);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma_bf16(bf[j], af[i], acc[i][j]);   // rows: n, columns (lanes): m
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
        af.template store<EPI>(make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]), m, n, N, bias,
                               pre_in, out, pre_out);
      }
  }
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[n][k] = sum_m bf16(G[m][n]) bf16(X[m][k])     (G = dY [M][N], X [M][K], both row-major over the reduction index m)
//
// Block = (128-column tile of k, 128-row tile of n, split s of the rows); 4 waves as 2 x 2, each 64 x 64.  Each step stages DW_BR rows:
// float4 loads along the channels, stored TRANSPOSED as m-contiguous bf16 images [channel][m] with two rows packed per 32-bit LDS
// write (the register stage of pairs_wgrad_bf16_kernel).  Rows past the split are zeroed on the block-uniform last step.
// A split count of 1 writes dW directly; otherwise each split writes its own (N x K) partial and dense_wgrad_reduce_kernel adds them.
// ---------------------------------------------------------------------------------------
constexpr int DW_BR = 64;    // rows (reduction) staged per step: four k-steps of 16
constexpr int DW_T = kDenseDwTile;

__global__ __launch_bounds__(256) void dense_wgrad_bf16_kernel(const float *__restrict__ G, const float *__restrict__ X, int64_t M, int N, int K,
                                                               int64_t split_len, float *__restrict__ part, float *__restrict__ dW) {
  constexpr int ITEMS = (DW_BR / 2) * (DW_T / 4) / 256;   // (row pair, float4) items per thread and operand: 4
  __shared__ __attribute__((aligned(16))) __bf16 Gt[DW_T * DB_STRIDE];   // [n][m]
  __shared__ __attribute__((aligned(16))) __bf16 Xt[DW_T * DB_STRIDE];   // [k][m]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;   // wm: k half, wn: n half
  const int k0 = blockIdx.x * DW_T, n0 = blockIdx.y * DW_T;
  const int64_t lo = (int64_t)blockIdx.z * split_len;
  const int64_t hi = lo + split_len < M ? lo + split_len : M;

  int rp[ITEMS], c4[ITEMS], gcol[ITEMS], xcol[ITEMS];
#pragma unroll
  for (int q = 0; q < ITEMS; ++q) {
    const int e = q * 256 + tid;
    c4[q] = (e % (DW_T / 4)) * 4;
    rp[q] = e / (DW_T / 4);
    gcol[q] = n0 + c4[q] + 4 <= N ? n0 + c4[q] : N - 4;   // clamped columns reach only image rows that are never stored
    xcol[q] = k0 + c4[q] + 4 <= K ? k0 + c4[q] : K - 4;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;

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
    if (r0 + DW_BR > hi) {   // block-uniform: the split's last step
#pragma unroll
      for (int q = 0; q < ITEMS; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (r0 + 2 * rp[q] + h >= hi) rg[q][h] = rx[q][h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the ONE place the operands are rounded
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
      const bf16x4 g0 = round4(rg[q][0]), g1 = round4(rg[q][1]);
      const bf16x4 x0 = round4(rx[q][0]), x1 = round4(rx[q][1]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *(bf16x2 *)&Gt[(c4[q] + e) * DB_STRIDE + 2 * rp[q]] = (bf16x2){g0[e], g1[e]};
        *(bf16x2 *)&Xt[(c4[q] + e) * DB_STRIDE + 2 * rp[q]] = (bf16x2){x0[e], x1[e]};
      }
    }
  };

  const __bf16 *xp = &Xt[(wm * 64 + l31) * DB_STRIDE + 8 * half];
  const __bf16 *gp = &Gt[(wn * 64 + l31) * DB_STRIDE + 8 * half];
  load_step(lo);
  for (int64_t r0 = lo; r0 < hi; r0 += DW_BR) {
    store_step(r0);
    __syncthreads();
    if (r0 + DW_BR < hi) load_step(r0 + DW_BR);
#pragma unroll
    for (int s = 0; s < DW_BR / 16; ++s) {
      bf16x8 xf[2], gf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = *(const bf16x8 *)(xp + i * 32 * DB_STRIDE + 16 * s);
#pragma unroll
      for (int j = 0; j < 2; ++j) gf[j] = *(const bf16x8 *)(gp + j * 32 * DB_STRIDE + 16 * s);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16(xf[i], gf[j], acc[i][j]);   // rows: k, columns (lanes): n
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
        if (k < K) *(float4 *)&dst[(int64_t)n * K + k] = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
      }
  }
}

struct DenseBf16 {
  static constexpr const char *gemm_name = "ftx_dense_gemm_bf16", *wgrad_name = "ftx_dense_wgrad_bf16";
  static constexpr const char *patch_name = "ftx_vit_patch_embed_bf16", *tap_name = "ftx_vit_tap_stem_bf16";
  template <int MI, int NI, int EPI, bool WKN, class AF>
  static void gemm(dim3 grid, hipStream_t st, const AF &af, const DenseGemmArgs &a) {
    dense_gemm_bf16_kernel<MI, NI, EPI, WKN, AF><<<grid, 256, 0, st>>>(af, a.W, a.bias, a.pre_in, a.M, a.N, a.K, a.out, a.pre_out);
  }
  static void wgrad(dim3 grid, hipStream_t st, const float *G, const float *X, int64_t M, int N, int K, int64_t len, float *part, float *dW) {
    dense_wgrad_bf16_kernel<<<grid, 256, 0, st>>>(G, X, M, N, K, len, part, dW);
  }
};

extern "C" int ftx_dense_gemm_bf16(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n,
                                   int32_t k, int32_t epilogue, float *out, float *pre_out, void *stream) {
  return dense_gemm_entry<DenseBf16>(A, W, w_kn, bias, pre_in, m, n, k, epilogue, out, pre_out, stream);
}

extern "C" int ftx_vit_patch_embed_bf16(const float *img, const float *W, const float *bias, const float *cls, const float *dist, const float *pos,
                                       int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *tokens, void *stream) {
  return dense_patch_embed_entry<DenseBf16>(img, W, bias, cls, dist, pos, b, c, h, w, patch, dim, t0, tokens, stream);
}

extern "C" int ftx_vit_tap_stem_bf16(const float *tokens, const float *W, const float *bias, const float *gamma, const float *beta,
                                    const float *running_mean, const float *running_var, float eps, int32_t b, int32_t g, int32_t t0, int32_t dim,
                                    int32_t co, float *out, void *stream) {
  return dense_tap_stem_entry<DenseBf16>(tokens, W, bias, gamma, beta, running_mean, running_var, eps, b, g, t0, dim, co, out, stream);
}

extern "C" size_t ftx_dense_wgrad_bf16_workspace_bytes(int64_t m, int32_t n, int32_t k) { return dense_wgrad_workspace_bytes(m, n, k); }

extern "C" int ftx_dense_wgrad_bf16(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                                    void *stream) {
  return dense_wgrad_entry<DenseBf16>(G, X, m, n, k, dW, workspace, workspace_bytes, stream);
}

extern "C" int ftx_dense_bf16_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  return dense_tile_entry("ftx_dense_bf16_tile", form, m, n, k, tile_m_host, tile_n_host, split_host);
}

// ---------------------------------------------------------------------------------------
// The one definition of what ftx_dense_common.h declares for both families.
// ---------------------------------------------------------------------------------------
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
