// bf16-operand sparse convolution: the pair-list GEMM and the weight gradient of ftx_spconv.hip with every product on
// v_mfma_f32_32x32x16_bf16 (16x the rate of v_mfma_f32_32x32x2_f32) and fp32 accumulation.
//
// Precision contract (include/ftx.h states it for callers):
//   operands  A, W (pair GEMM) and A, G (weight gradient) stay fp32 in HBM; each element is rounded to bf16 (round-to-nearest-even,
//             a plain cast: v_cvt_pk_bf16_f32, NaN stays NaN) from its stored value when it is written to LDS.
//   products  a bf16 x bf16 product is exact in fp32; the sums run in the MFMA's fp32 accumulators.
//   storage   tmp, out, bias and dW are fp32; tmp has the layout of ftx_spconv_pairs_gemm, so ftx_spconv_reduce /
//             ftx_spconv_reduce_stats consume it unchanged and the sum over offsets keeps its fixed order.
//   order     no atomics; weight-gradient partial tiles are added by the fixed-order wgrad_reduce_kernel: deterministic.
//
// Operand maps of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md section 3): lane (r = lane & 31, h = lane >> 5) holds A[row r][k]
// and B[k][col r] for k = 8h + j, j = 0..7, of each 16-wide k-step; accumulator register g of the lane is C[(g&3) + 8(g>>2) + 4h][r],
// the same layout as the f32 MFMA, so the pair GEMM is one kernel body and one epilogue for both families (ftx_spconv_common.h, with
// everything else the two families have in common).  Both operands are staged as bf16 LDS images in which the reduction index is contiguous: one
// ds_read_b128 per operand and k-step.
#include "ftx_spconv_common.h"

using namespace ftx;

// ---------------------------------------------------------------------------------------
// tmp[p,:] = bf16(A[gather[p],:]) @ bf16(Wk(p))      (tiles of 128 pairs of one offset; the forms of the fp32 family):
// pairs_gemm_kernel<SpconvBf16, NT> of ftx_spconv_common.h, the body that both families instantiate
// ---------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------
// weight gradient: dW[k] = sum_{p in k} bf16(A[idx_a[p],:])^T @ bf16(G[idx_g[p],:])
//
// Block = (tile of `tile_len` consecutive pairs of ONE offset, M tile, N tile) -> one (TM x TN) partial of dW[k], summed per offset by
// wgrad_reduce_kernel (an offset that fits one tile is written straight into dW[k]) -- the scheme of pairs_wgrad_kernel.  The reduction
// index is the PAIR, so a lane needs 8 consecutive pairs of one channel: each step gathers WB_BR pairs row-major ([pair][channel]
// float4 loads, two pairs per thread) and stores them transposed as k-contiguous bf16 images [channel][pair], two pairs packed per
// 32-bit LDS write.  Wave (wm, wn) owns MI x NI 32 x 32 sub-tiles: a-channels m0 + 32 (wm MI + i) + l31, g-channels m0 + 32 (wn NI + j)
// + row; KS = 4 / (WMG WNG) wave groups split the k-steps of a stage and are summed through LDS in a fixed order.
// ---------------------------------------------------------------------------------------
constexpr int WB_BR = 64;       // pairs staged per step: four k-steps of 16
constexpr int WB_STRIDE = 72;   // bf16 per image row (144 B): conflict-free ds_read_b128

template <int MI, int NI, int WMG, int WNG>
__global__ __launch_bounds__(256) void pairs_wgrad_bf16_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ idx_a,
                                                               const float *__restrict__ G, int64_t rows_g, const int32_t *__restrict__ idx_g,
                                                               const int32_t *__restrict__ koff, int ca, int cg, int kvol, int tile_len,
                                                               float *__restrict__ part, float *__restrict__ dW, int n_dense) {
  // idx_a == nullptr: dense mode, rows [0, n_dense) of A and G pair up one to one (kvol = 1)
  constexpr int TM = 32 * MI * WMG, TN = 32 * NI * WNG, KS = 4 / (WMG * WNG);
  constexpr int STAGE_B = (TM + TN) * WB_STRIDE * 2;                          // bytes
  constexpr int RED_B = KS > 1 ? MI * NI * 1024 * WMG * WNG * 4 : 0;          // bytes: one KS group's accumulators
  constexpr int LDS_B = STAGE_B > RED_B ? STAGE_B : RED_B;
  __shared__ __attribute__((aligned(16))) char lds[LDS_B];
  __shared__ int32_t s_ia[kWgradRound], s_ig[kWgradRound];
  __shared__ uint8_t s_ok[kWgradRound];
  __shared__ int s_tile[4];
  __shared__ int s_bad;
  __bf16 *At = (__bf16 *)lds, *Gt = At + TM * WB_STRIDE;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wq = wave % (WMG * WNG), ks = wave / (WMG * WNG);
  const int wm = wq % WMG, wn = wq / WMG;
  pair_tile_scan<true>(koff, kvol, tile_len, n_dense, s_tile);   // tile -> (offset, pair range)
  __syncthreads();
  const int k = s_tile[0];
  if (k < 0) return;  // surplus block of the upper-bound grid
  const int m0 = blockIdx.y * TM, n0 = blockIdx.z * TN;
  const int lo = s_tile[1], hi = s_tile[2];
  const bool single = s_tile[3] == 1;   // the only tile of its offset: the result IS dW[k]

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;

  // Staging item = (pair pair pp, 4 channels c4): two float4 gathers, stored as 4 packed bf16 pairs.  TX / 32 items per thread.
  // Loads are unconditional from always-valid addresses: indices clamped to real rows, channels to the last float4 of a row (what a
  // channel >= ca (cg) brings in only reaches accumulator rows / columns the epilogue never stores); pairs past the end of the tile
  // and malformed pairs are zeroed at store time on a block-uniform slow path.
  constexpr int QA = TM / 32, QG = TN / 32;
  float4 ra[QA][2], rg[QG][2];
  int pa[QA], pg[QG], ca_off[QA], cg_off[QG], ra_row[QA], rg_row[QG];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    int e = q * 256 + tid;
    pa[q] = 2 * (e / (TM / 4));
    ra_row[q] = (e % (TM / 4)) * 4;
    int c = m0 + ra_row[q];
    ca_off[q] = c + 4 <= ca ? c : ca - 4;
  }
#pragma unroll
  for (int q = 0; q < QG; ++q) {
    int e = q * 256 + tid;
    pg[q] = 2 * (e / (TN / 4));
    rg_row[q] = (e % (TN / 4)) * 4;
    int c = n0 + rg_row[q];
    cg_off[q] = c + 4 <= cg ? c : cg - 4;
  }
  int rbase = lo, rend = lo;
  auto load_step = [&](int p0) {
    const int o = p0 - rbase;
#pragma unroll
    for (int q = 0; q < QA; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) ra[q][h] = *(const float4 *)(A + ((int64_t)s_ia[o + pa[q] + h] * ca + ca_off[q]));
#pragma unroll
    for (int q = 0; q < QG; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) rg[q][h] = *(const float4 *)(G + ((int64_t)s_ig[o + pg[q] + h] * cg + cg_off[q]));
  };
  auto store_step = [&](int p0) {
    if (p0 + WB_BR > rend || s_bad) {   // block-uniform: last step of the tile (or a malformed pair list)
#pragma unroll
      for (int q = 0; q < QA; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int p = p0 + pa[q] + h;
          if (p >= rend || s_ok[p - rbase] == 0) ra[q][h] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
      for (int q = 0; q < QG; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int p = p0 + pg[q] + h;
          if (p >= rend || s_ok[p - rbase] == 0) rg[q][h] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // the ONE place the operands are rounded
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const bf16x4 x0 = round4(ra[q][0]), x1 = round4(ra[q][1]);
#pragma unroll
      for (int e = 0; e < 4; ++e) *(bf16x2 *)&At[(ra_row[q] + e) * WB_STRIDE + pa[q]] = (bf16x2){x0[e], x1[e]};
    }
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      const bf16x4 x0 = round4(rg[q][0]), x1 = round4(rg[q][1]);
#pragma unroll
      for (int e = 0; e < 4; ++e) *(bf16x2 *)&Gt[(rg_row[q] + e) * WB_STRIDE + pg[q]] = (bf16x2){x0[e], x1[e]};
    }
  };
  const __bf16 *ap = At + (wm * MI * 32 + l31) * WB_STRIDE + 8 * half;
  const __bf16 *gp = Gt + (wn * NI * 32 + l31) * WB_STRIDE + 8 * half;
  auto mfma_step = [&]() {
#pragma unroll
    for (int it = 0; it < 4 / KS; ++it) {
      const int s = it * KS + ks;
      bf16x8 af[MI], gf[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = *(const bf16x8 *)(ap + i * 32 * WB_STRIDE + 16 * s);
#pragma unroll
      for (int j = 0; j < NI; ++j) gf[j] = *(const bf16x8 *)(gp + j * 32 * WB_STRIDE + 16 * s);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma_bf16(gf[j], af[i], acc[i][j]);   // rows: g-channel, cols: a-channel
    }
  };

  for (rbase = lo; rbase < hi; rbase += kWgradRound) {
    rend = (rbase + kWgradRound < hi) ? rbase + kWgradRound : hi;
    wgrad_stage_indices(idx_a, rows_a, idx_g, rows_g, rbase, rend, s_ia, s_ig, s_ok, &s_bad);
    load_step(rbase);
    for (int p0 = rbase; p0 < rend; p0 += WB_BR) {
      store_step(p0);
      __syncthreads();
      if (p0 + WB_BR < rend) load_step(p0 + WB_BR);   // next step's gathers fly under this step's MFMAs
      mfma_step();
      __syncthreads();
    }
  }

  wgrad_ks_reduce<MI, NI, KS>(acc, (float *)lds, wq, ks, lane);   // the k-step subsets of the KS wave groups (the staging images are free now)

  if (ks == 0) {
    const int64_t mat = (int64_t)ca * cg;
    float *dst = single ? dW + (int64_t)k * mat : part + (int64_t)blockIdx.x * mat;   // tiles are numbered in offset order
    // accumulator registers 4q..4q+3 of lane (l31, half) in sub-tile (i, j): a-channel row, g-channels col .. col+3
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + (wm * MI + i) * 32 + l31;
      if (row < ca) {
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int col = n0 + (wn * NI + j) * 32 + 8 * q + 4 * half;
            if (col < cg)
              *(float4 *)&dst[(int64_t)row * cg + col] = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// the family's description and entries (ftx_spconv_common.h): the tile rules of the fp32 family with this family's table and step
// ---------------------------------------------------------------------------------------
struct SpconvBf16 {
  static constexpr const char *pairs_name = "ftx_spconv_pairs_gemm_bf16", *scatter_name = "ftx_spconv_pairs_gemm_scatter_bf16",
                              *rows_name = "ftx_rows_gemm_bf16", *wgrad_name = "ftx_spconv_pairs_wgrad_bf16";
  // .vgpr_count 64 / 100-104 / 136-152 / 188-244 / 312
  static constexpr int wgrad_blocks[4][4] = {{8, 4, 3, 3}, {4, 3, 2, 2}, {3, 2, 1, 2}, {3, 2, 2, 2}};
  static constexpr int wgrad_step = 2 * WB_BR;
  using gemm_lds_t = __bf16;
  static constexpr int gemm_stride = 40;   // bf16 per LDS row (80 B): the 16 lanes of one ds_read_b128 phase cover 16 disjoint bank quads
  static constexpr bool gemm_frag_ptrs_first = true;
  template <int NT>
  static void gemm(dim3 grid, hipStream_t st, const PairsGemmArgs &a) {
    pairs_gemm_kernel<SpconvBf16, NT><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.gather, a.W, a.w_transposed, a.koff, a.ca, a.co, a.kvol, a.out, a.bias,
                                                            a.n_dense, a.scatter, a.rows_out);
  }
  template <int MI, int NI, int WMG, int WNG>
  static void wgrad(dim3 grid, hipStream_t st, const PairsWgradArgs &a) {
    pairs_wgrad_bf16_kernel<MI, NI, WMG, WNG><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.idx_a, a.G, a.rows_g, a.idx_g, a.koff, a.ca, a.cg, a.kvol,
                                                                    a.tile_len, a.part, a.dW, a.n_dense);
  }
};

extern "C" int32_t ftx_spconv_gemm_bf16_block_cols(int32_t co, int64_t n_pairs, int32_t kvol) { return spconv_gemm_block_cols(co, n_pairs, kvol); }

extern "C" int ftx_spconv_pairs_gemm_bf16(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed,
                                          const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream) {
  return spconv_pairs_entry<SpconvBf16>(false, A, rows_a, gather, nullptr, W, w_transposed, koff, n_pairs, ca, co, kvol, tmp, 0, stream);
}

extern "C" int ftx_spconv_pairs_gemm_scatter_bf16(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W,
                                                  int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol,
                                                  float *out, int64_t rows_out, void *stream) {
  return spconv_pairs_entry<SpconvBf16>(true, A, rows_a, gather, scatter, W, w_transposed, koff, n_pairs, ca, co, kvol, out, rows_out, stream);
}

extern "C" int ftx_rows_gemm_bf16(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co,
                                  float *out, void *stream) {
  return spconv_rows_entry<SpconvBf16>(A, n, W, w_transposed, bias, ca, co, out, stream);
}

extern "C" int32_t ftx_spconv_wgrad_bf16_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng) {
  return spconv_wgrad_table_blocks<SpconvBf16>(mi, wmg, ni, wng);
}

extern "C" size_t ftx_spconv_pairs_wgrad_bf16_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol) {
  return spconv_wgrad_workspace_bytes<SpconvBf16>(n_pairs, ca, cg, kvol);
}

extern "C" int ftx_spconv_pairs_wgrad_bf16(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g,
                                           const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace,
                                           size_t workspace_bytes, void *stream) {
  return spconv_wgrad_entry<SpconvBf16>(A, rows_a, idx_a, G, rows_g, idx_g, koff, n_pairs, ca, cg, kvol, dW, workspace, workspace_bytes, stream);
}
