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
// the same layout as the f32 MFMA, so both kernels keep the epilogues of their fp32 twins.  Both operands are staged as bf16 LDS images
// in which the reduction index is contiguous: one ds_read_b128 per operand and k-step.
#include "ftx_common.h"
#include "ftx_mfma.h"
#include "ftx_spconv_wgrad_reduce.h"

using namespace ftx;

namespace {

__device__ inline bf16x4 round4(float4 v) { return (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w}; }

// Tile -> (offset, first pair, pair count) of an upper-bound grid of `tile`-pair tiles: wave 0 scans the per-offset tile counts
// (the scan of pairs_gemm_kernel).  s_tile[0] = -1 for a surplus block.
__device__ inline void gemm_tile_scan(const int32_t *__restrict__ koff, int kvol, int tile, int64_t n_dense, bool dense, int *s_tile) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  if (dense) {
    if (tid == 0) {
      int64_t left = n_dense - (int64_t)b * tile;
      s_tile[0] = left > 0 ? 0 : -1;
      s_tile[1] = b * tile;
      s_tile[2] = left > tile ? tile : (int)left;
    }
    return;
  }
  if (tid >= 64) return;
  int c = (tid < kvol) ? koff[tid + 1] - koff[tid] : 0;
  int nt = (c + tile - 1) / tile;
  int incl = nt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int v = __shfl_up(incl, off, 64);
    if (tid >= off) incl += v;
  }
  int excl = incl - nt;
  bool mine = (tid < kvol) && b >= excl && b < incl;
  unsigned long long m = __ballot(mine);
  if (mine) {
    int t = b - excl;
    int left = c - t * tile;
    s_tile[0] = tid;
    s_tile[1] = koff[tid] + t * tile;
    s_tile[2] = left > tile ? tile : left;
  }
  if (m == 0ull && tid == 0) s_tile[0] = -1;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// tmp[p,:] = bf16(A[gather[p],:]) @ bf16(Wk(p))      (tiles of 128 pairs of one offset; the forms of pairs_gemm_kernel)
// ---------------------------------------------------------------------------------------
constexpr int GB_BK = 32;       // channels of the reduction staged per step: two k-steps of 16
constexpr int GB_STRIDE = 40;   // bf16 per LDS row (80 B): the 16 lanes of one ds_read_b128 phase cover 16 disjoint bank quads
constexpr int GB_TILE = 128;    // pairs per tile: 4 waves x 32 pairs

// NT = 32-column tiles per block.  W is the MFMA's row operand (rows = output channels, columns = pairs), as in the fp32 kernel.
template <int NT>
__global__ __launch_bounds__(256) void pairs_gemm_bf16_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ gather,
                                                              const float *__restrict__ W, int w_transposed, const int32_t *__restrict__ koff,
                                                              int ca, int co, int kvol, float *__restrict__ tmp, const float *__restrict__ bias,
                                                              int64_t n_dense, const int32_t *__restrict__ scatter, int64_t rows_out) {
  constexpr int BN = 32 * NT;
  constexpr int A_PASSES = 4;      // GB_TILE * GB_BK / 4 float4 = 4 per thread
  constexpr int B_PASSES = NT;     // GB_BK * BN / 4 float4 = NT * 256
  __shared__ __attribute__((aligned(16))) __bf16 As[GB_TILE * GB_STRIDE];   // [pair][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[BN * GB_STRIDE];        // [n][k]
  __shared__ int s_tile[3];

  const int tid = threadIdx.x;
  gemm_tile_scan(koff, kvol, GB_TILE, n_dense, gather == nullptr, s_tile);
  __syncthreads();
  const int k = s_tile[0];
  if (k < 0) return;  // surplus block of the upper-bound grid
  const int p0 = s_tile[1], cnt = s_tile[2];

  const int wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int n0 = blockIdx.y * BN;
  const int arow = tid >> 3, acol = (tid & 7) * 4;

  // Gather rules of pairs_gemm_kernel: unconditional loads from always-valid addresses (rows past the tile and malformed indices read
  // row 0 and land in accumulator columns the epilogue never stores, or zeroes); a reduction dimension that is not a multiple of
  // GB_BK (the 4-channel stem) is zero-filled on a uniform slow path.
  const bool kfull = (ca % GB_BK) == 0;
  int32_t src[A_PASSES];
#pragma unroll
  for (int p = 0; p < A_PASSES; ++p) {
    int r = p * 32 + arow;
    int32_t s = 0;
    if (r < cnt) s = gather ? gather[p0 + r] : p0 + r;
    if (s < 0 || s >= rows_a) s = 0;
    src[p] = s;
  }
  const float *Wk = W + (int64_t)k * ca * co;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;

  float4 ra[A_PASSES], rb[B_PASSES];
  auto load_chunk = [&](int c0) {
    if (kfull) {
#pragma unroll
      for (int p = 0; p < A_PASSES; ++p) ra[p] = *(const float4 *)&A[(int64_t)src[p] * ca + c0 + acol];
#pragma unroll
      for (int q = 0; q < B_PASSES; ++q) {
        if (!w_transposed) {  // W[k] stored (ca, co): 16 bytes along co
          int kk = ((tid >> 6) << 3) + (tid & 7), n4 = n0 + (q * 8 + ((tid >> 3) & 7)) * 4;
          n4 = n4 + 4 <= co ? n4 : co - 4;
          rb[q] = *(const float4 *)&Wk[(int64_t)(c0 + kk) * co + n4];
        } else {              // W[k] stored (co, ca): 16 bytes along ca
          int e = q * 256 + tid;
          int nn = n0 + (e >> 3), k4 = (e & 7) * 4;
          nn = nn < co ? nn : co - 1;
          rb[q] = *(const float4 *)&Wk[(int64_t)nn * ca + c0 + k4];
        }
      }
      return;
    }
#pragma unroll
    for (int p = 0; p < A_PASSES; ++p) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + acol < ca) v = *(const float4 *)&A[(int64_t)src[p] * ca + c0 + acol];
      ra[p] = v;
    }
#pragma unroll
    for (int q = 0; q < B_PASSES; ++q) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!w_transposed) {
        int kk = ((tid >> 6) << 3) + (tid & 7), n4 = (q * 8 + ((tid >> 3) & 7)) * 4;
        if (c0 + kk < ca && n0 + n4 < co) v = *(const float4 *)&Wk[(int64_t)(c0 + kk) * co + n0 + n4];
      } else {
        int e = q * 256 + tid;
        int nn = e >> 3, k4 = (e & 7) * 4;
        if (n0 + nn < co && c0 + k4 < ca) v = *(const float4 *)&Wk[(int64_t)(n0 + nn) * ca + c0 + k4];
      }
      rb[q] = v;
    }
  };
  // the ONE place the operands are rounded: fp32 registers -> bf16 LDS images
  auto store_chunk = [&]() {
#pragma unroll
    for (int p = 0; p < A_PASSES; ++p) *(bf16x4 *)&As[(p * 32 + arow) * GB_STRIDE + acol] = round4(ra[p]);
#pragma unroll
    for (int q = 0; q < B_PASSES; ++q) {
      if (!w_transposed) {  // transposing store
        int kk = ((tid >> 6) << 3) + (tid & 7), n4 = (q * 8 + ((tid >> 3) & 7)) * 4;
        const bf16x4 v = round4(rb[q]);
        Bs[(n4 + 0) * GB_STRIDE + kk] = v[0];
        Bs[(n4 + 1) * GB_STRIDE + kk] = v[1];
        Bs[(n4 + 2) * GB_STRIDE + kk] = v[2];
        Bs[(n4 + 3) * GB_STRIDE + kk] = v[3];
      } else {
        int e = q * 256 + tid;
        int nn = e >> 3, k4 = (e & 7) * 4;
        *(bf16x4 *)&Bs[nn * GB_STRIDE + k4] = round4(rb[q]);
      }
    }
  };

  const __bf16 *ap = &As[(wave * 32 + l31) * GB_STRIDE + 8 * half];
  const __bf16 *bp = &Bs[l31 * GB_STRIDE + 8 * half];
  load_chunk(0);
  for (int c0 = 0; c0 < ca; c0 += GB_BK) {
    store_chunk();
    __syncthreads();
    if (c0 + GB_BK < ca) load_chunk(c0 + GB_BK);  // next chunk's global loads fly under the MFMAs
#pragma unroll
    for (int s = 0; s < GB_BK / 16; ++s) {
      const bf16x8 a = *(const bf16x8 *)(ap + 16 * s);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = mfma_bf16(*(const bf16x8 *)(bp + j * 32 * GB_STRIDE + 16 * s), a, acc[j]);
    }
    __syncthreads();
  }

  // epilogue of pairs_gemm_kernel: lane (pair l31, half) holds 4 consecutive output channels in every 4 accumulator registers
  const bool nfull = n0 + BN <= co;
  const int row = wave * 32 + l31;
  int64_t drow = row < cnt ? p0 + row : -1;
  bool zero = false;   // a pair whose source index is out of range contributes a zero row
  if (gather != nullptr && drow >= 0) {
    const int32_t sidx = gather[drow];
    zero = sidx < 0 || sidx >= rows_a;
  }
  if (scatter != nullptr && drow >= 0) {
    drow = scatter[drow];
    if (drow >= rows_out) drow = -1;
  }
  if (drow >= 0) {
    float *dst = tmp + drow * co;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = n0 + j * 32 + 8 * q + 4 * half;
        if (nfull || col < co) {
          float4 v = make_float4(acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]);
          if (zero) v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (bias) {
            const float4 bv = *(const float4 *)&bias[col];
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
          }
          *(float4 *)&dst[col] = v;
        }
      }
  }
}

static void launch_pairs_gemm_bf16(int nt, dim3 grid, hipStream_t st, const float *A, int64_t rows_a, const int32_t *gather, const float *W, int wT,
                                   const int32_t *koff, int ca, int co, int kvol, float *tmp, const float *bias, int64_t n_dense,
                                   const int32_t *scatter = nullptr, int64_t rows_out = 0) {
  switch (nt) {
    case 1: pairs_gemm_bf16_kernel<1><<<grid, 256, 0, st>>>(A, rows_a, gather, W, wT, koff, ca, co, kvol, tmp, bias, n_dense, scatter, rows_out); break;
    case 2: pairs_gemm_bf16_kernel<2><<<grid, 256, 0, st>>>(A, rows_a, gather, W, wT, koff, ca, co, kvol, tmp, bias, n_dense, scatter, rows_out); break;
    case 3: pairs_gemm_bf16_kernel<3><<<grid, 256, 0, st>>>(A, rows_a, gather, W, wT, koff, ca, co, kvol, tmp, bias, n_dense, scatter, rows_out); break;
    default: pairs_gemm_bf16_kernel<4><<<grid, 256, 0, st>>>(A, rows_a, gather, W, wT, koff, ca, co, kvol, tmp, bias, n_dense, scatter, rows_out); break;
  }
}

// Column tiles per block as a function of the arguments only: the fp32 rule (gemm_nt in ftx_spconv.hip) -- 128 columns where there
// are enough pair tiles to fill the chip, 64 on the two deepest levels, 96 for multiples of 96.
static int gemm_bf16_nt(int co, int64_t row_tiles) {
  int nt = co >= 128 ? 4 : (co + 31) / 32;
  if (co > 128 && co % 96 == 0 && co % 128 != 0) nt = 3;
  if (nt == 4 && row_tiles * ceil_div(co, 128) <= 400) nt = 2;
  return nt;
}

extern "C" int32_t ftx_spconv_gemm_bf16_block_cols(int32_t co, int64_t n_pairs, int32_t kvol) {
  if (co < 4 || co % 4 != 0 || n_pairs < 0 || kvol < 0) return -1;
  return 32 * gemm_bf16_nt(co, ceil_div(n_pairs, GB_TILE) + kvol);
}

extern "C" int ftx_spconv_pairs_gemm_bf16(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed,
                                          const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream) {
  FTX_REQUIRE(n_pairs >= 0 && rows_a >= 0 && kvol >= 1 && kvol <= 64, "ftx_spconv_pairs_gemm_bf16: bad size");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && co >= 4 && co % 4 == 0, "ftx_spconv_pairs_gemm_bf16: channels must be multiples of 4 (ca=%d co=%d)", ca, co);
  if (n_pairs == 0) return FTX_OK;
  FTX_REQUIRE(A && gather && W && koff && tmp && rows_a >= 1, "ftx_spconv_pairs_gemm_bf16: null pointer or empty operand");
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles_ub = ceil_div(n_pairs, GB_TILE) + kvol;   // sum_k ceil(cnt_k/tile) <= P/tile + kvol
  const int nt = gemm_bf16_nt(co, tiles_ub);
  dim3 grid((unsigned)tiles_ub, (unsigned)ceil_div(co, 32 * nt));
  launch_pairs_gemm_bf16(nt, grid, st, A, rows_a, gather, W, w_transposed, koff, ca, co, kvol, tmp, nullptr, 0);
  return check_launch("ftx_spconv_pairs_gemm_bf16");
}

extern "C" int ftx_spconv_pairs_gemm_scatter_bf16(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W,
                                                  int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol,
                                                  float *out, int64_t rows_out, void *stream) {
  FTX_REQUIRE(n_pairs >= 0 && rows_a >= 0 && rows_out >= 0 && kvol >= 1 && kvol <= 64, "ftx_spconv_pairs_gemm_scatter_bf16: bad size");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && co >= 4 && co % 4 == 0, "ftx_spconv_pairs_gemm_scatter_bf16: channels must be multiples of 4 (ca=%d co=%d)", ca, co);
  if (n_pairs == 0) return FTX_OK;
  FTX_REQUIRE(A && gather && scatter && W && koff && out && rows_a >= 1, "ftx_spconv_pairs_gemm_scatter_bf16: null pointer or empty operand");
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles_ub = ceil_div(n_pairs, GB_TILE) + kvol;
  const int nt = gemm_bf16_nt(co, tiles_ub);
  dim3 grid((unsigned)tiles_ub, (unsigned)ceil_div(co, 32 * nt));
  launch_pairs_gemm_bf16(nt, grid, st, A, rows_a, gather, W, w_transposed, koff, ca, co, kvol, out, nullptr, 0, scatter, rows_out);
  return check_launch("ftx_spconv_pairs_gemm_scatter_bf16");
}

extern "C" int ftx_rows_gemm_bf16(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co,
                                  float *out, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_rows_gemm_bf16: n < 0");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && co >= 4 && co % 4 == 0, "ftx_rows_gemm_bf16: channels must be multiples of 4 (ca=%d co=%d)", ca, co);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(A && W && out, "ftx_rows_gemm_bf16: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int nt = gemm_bf16_nt(co, ceil_div(n, GB_TILE));
  dim3 grid((unsigned)ceil_div(n, GB_TILE), (unsigned)ceil_div(co, 32 * nt));
  launch_pairs_gemm_bf16(nt, grid, st, A, n, nullptr, W, w_transposed, nullptr, ca, co, 1, out, bias, n);
  return check_launch("ftx_rows_gemm_bf16");
}

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
constexpr int WB_ROUND = 1024;  // pair indices kept in LDS at a time

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
  __shared__ int32_t s_ia[WB_ROUND], s_ig[WB_ROUND];
  __shared__ uint8_t s_ok[WB_ROUND];
  __shared__ int s_tile[4];
  __shared__ int s_bad;
  __bf16 *At = (__bf16 *)lds, *Gt = At + TM * WB_STRIDE;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wq = wave % (WMG * WNG), ks = wave / (WMG * WNG);
  const int wm = wq % WMG, wn = wq / WMG;
  if (tid < 64) {   // tile -> (offset, pair range), as pairs_wgrad_kernel
    const int b = blockIdx.x;
    int c = 0;
    if (tid < kvol) c = koff ? koff[tid + 1] - koff[tid] : n_dense;
    int nt = (c + tile_len - 1) / tile_len;
    int incl = nt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      int v = __shfl_up(incl, off, 64);
      if (tid >= off) incl += v;
    }
    int excl = incl - nt;
    bool mine = (tid < kvol) && b >= excl && b < incl;
    unsigned long long msk = __ballot(mine);
    if (mine) {
      int t = b - excl;
      int first = (koff ? koff[tid] : 0) + t * tile_len;
      int left = c - t * tile_len;
      s_tile[0] = tid;
      s_tile[1] = first;
      s_tile[2] = first + (left > tile_len ? tile_len : left);
      s_tile[3] = nt;
    }
    if (msk == 0ull && tid == 0) s_tile[0] = -1;
  }
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

  for (rbase = lo; rbase < hi; rbase += WB_ROUND) {
    rend = (rbase + WB_ROUND < hi) ? rbase + WB_ROUND : hi;
    __syncthreads();  // previous round's gathers are done with s_ia / s_ig
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int t = tid; t < WB_ROUND; t += 256) {
      // every slot gets a loadable row: slots past the end repeat row 0, malformed pairs are flagged and zeroed at store time
      int32_t ia = 0, ig = 0;
      uint8_t ok = 0;
      if (t < rend - rbase) {
        ia = idx_a ? idx_a[rbase + t] : rbase + t;
        ig = idx_g ? idx_g[rbase + t] : rbase + t;
        ok = 1;
        if (ia < 0 || ia >= rows_a || ig < 0 || ig >= rows_g) {
          ia = ig = 0;
          ok = 0;
          s_bad = 1;
        }
      }
      s_ia[t] = ia;
      s_ig[t] = ig;
      s_ok[t] = ok;
    }
    __syncthreads();
    load_step(rbase);
    for (int p0 = rbase; p0 < rend; p0 += WB_BR) {
      store_step(p0);
      __syncthreads();
      if (p0 + WB_BR < rend) load_step(p0 + WB_BR);   // next step's gathers fly under this step's MFMAs
      mfma_step();
      __syncthreads();
    }
  }

  if (KS > 1) {  // sum the k-step subsets of the KS wave groups, fixed order (the staging images are free now)
    float *red = (float *)lds;
    for (int r = 1; r < KS; ++r) {
      if (ks == r) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) red[(((wq * MI + i) * NI + j) * 16 + g) * 64 + lane] = acc[i][j][g];
      }
      __syncthreads();
      if (ks == 0) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][j][g] += red[(((wq * MI + i) * NI + j) * 16 + g) * 64 + lane];
      }
      __syncthreads();
    }
  }

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

// Tile shape per channel count: the sides of wgrad_config (ftx_spconv.hip) -- M side 32 / 64 / 96 (multiples of 96 that are not
// multiples of 128) / 128, N side the same; 96 x 96 becomes 128 x 96.
struct WgradBf16Cfg { int mi, wmg, ni, wng; };
static WgradBf16Cfg wgrad_bf16_config(int ca, int cg) {
  WgradBf16Cfg c;
  if (ca <= 32) { c.mi = 1; c.wmg = 1; }
  else if (ca <= 64) { c.mi = 2; c.wmg = 1; }
  else if (ca % 96 == 0 && ca % 128 != 0) { c.mi = 3; c.wmg = 1; }
  else { c.mi = 2; c.wmg = 2; }
  if (cg <= 32) { c.ni = 1; c.wng = 1; }
  else if (cg <= 64) { c.ni = 2; c.wng = 1; }
  else if (cg % 96 == 0 && cg % 128 != 0) { c.ni = 3; c.wng = 1; }
  else { c.ni = 2; c.wng = 2; }
  if (c.mi == 3 && c.ni == 3) { c.mi = 2; c.wmg = 2; }
  return c;
}

// Resident blocks per CU of each instantiation, as a TABLE (the tile length, the workspace and the summation tree must be functions of
// the arguments alone): min(8, 512 / VGPRs rounded up to 8, 160 KiB / LDS) from the gfx950 code object (llvm-readelf --notes: .vgpr_count
// 64 / 100-104 / 136-152 / 188-244 / 312).  tests/test_spconv_bf16_host.py recomputes them from the built object.
static int wgrad_bf16_occ(const WgradBf16Cfg &c) {
  // rows: M side (mi, wmg) = (1,1) (2,1) (3,1) (2,2); columns: N side (ni, wng) in the same order
  static const int occ[4][4] = {{8, 4, 3, 3}, {4, 3, 2, 2}, {3, 2, 1, 2}, {3, 2, 2, 2}};
  auto side = [](int i, int w) { return w == 2 ? 3 : i - 1; };
  return occ[side(c.mi, c.wmg)][side(c.ni, c.wng)];
}
// (mi, wmg, ni, wng) -> table value, for the build-time check of the table against the code object
extern "C" int32_t ftx_spconv_wgrad_bf16_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng) {
  if (!((mi >= 1 && mi <= 3 && wmg == 1) || (mi == 2 && wmg == 2)) || !((ni >= 1 && ni <= 3 && wng == 1) || (ni == 2 && wng == 2))) return -1;
  WgradBf16Cfg c{mi, wmg, ni, wng};
  return wgrad_bf16_occ(c);
}
constexpr int WGRAD_BF16_CUS = 256;   // MI355X; a constant of the tiling, not a device query

// Pairs per tile: R full rounds of CUs x resident blocks, R as small as keeps a tile <= 4096 pairs (the rule of wgrad_tile_len).
static int wgrad_bf16_tile_len(int64_t n_pairs, int ca, int cg, int kvol) {
  const WgradBf16Cfg c = wgrad_bf16_config(ca, cg);
  const int64_t mn_tiles = ceil_div(ca, 32 * c.mi * c.wmg) * ceil_div(cg, 32 * c.ni * c.wng);
  const int64_t slots = (int64_t)WGRAD_BF16_CUS * wgrad_bf16_occ(c);
  int64_t len = 256;
  for (int rounds = 1; rounds <= 64; ++rounds) {
    int64_t tiles = (slots * rounds * 15 / 16) / mn_tiles - (kvol + 1) / 2;
    if (tiles < 1) tiles = 1;
    len = ceil_div(ceil_div(n_pairs, tiles), 2 * WB_BR) * 2 * WB_BR;
    if (len <= 4096) break;
  }
  if (len < 256) len = 256;
  return (int)len;
}

extern "C" size_t ftx_spconv_pairs_wgrad_bf16_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol) {
  if (n_pairs <= 0 || ca <= 0 || cg <= 0 || kvol <= 0) return 256;
  const int len = wgrad_bf16_tile_len(n_pairs, ca, cg, kvol);
  return sizeof(float) * (size_t)(ceil_div(n_pairs, len) + kvol) * ca * cg;
}

template <int MI, int WMG>
static void launch_wgrad_bf16_n(const WgradBf16Cfg &c, dim3 grid, hipStream_t st, const float *A, int64_t rows_a, const int32_t *idx_a, const float *G,
                                int64_t rows_g, const int32_t *idx_g, const int32_t *koff, int ca, int cg, int kvol, int tl, float *part, float *dW, int n_dense) {
  if (c.ni == 1)
    pairs_wgrad_bf16_kernel<MI, 1, WMG, 1><<<grid, 256, 0, st>>>(A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tl, part, dW, n_dense);
  else if (c.ni == 3)
    pairs_wgrad_bf16_kernel<MI, 3, WMG, 1><<<grid, 256, 0, st>>>(A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tl, part, dW, n_dense);
  else if (c.wng == 1)
    pairs_wgrad_bf16_kernel<MI, 2, WMG, 1><<<grid, 256, 0, st>>>(A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tl, part, dW, n_dense);
  else
    pairs_wgrad_bf16_kernel<MI, 2, WMG, 2><<<grid, 256, 0, st>>>(A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tl, part, dW, n_dense);
}

extern "C" int ftx_spconv_pairs_wgrad_bf16(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g,
                                           const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace,
                                           size_t workspace_bytes, void *stream) {
  FTX_REQUIRE(n_pairs >= 0 && rows_a >= 0 && rows_g >= 0 && kvol >= 1 && kvol <= 64, "ftx_spconv_pairs_wgrad_bf16: bad size");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && cg >= 4 && cg % 4 == 0, "ftx_spconv_pairs_wgrad_bf16: channels must be multiples of 4 (ca=%d cg=%d)", ca, cg);
  FTX_REQUIRE(dW, "ftx_spconv_pairs_wgrad_bf16: null dW");
  hipStream_t st = (hipStream_t)stream;
  const int64_t mat = (int64_t)ca * cg;
  if (n_pairs == 0) {
    if (hipMemsetAsync(dW, 0, sizeof(float) * kvol * mat, st) != hipSuccess) return check_launch("ftx_spconv_pairs_wgrad_bf16 memset");
    return FTX_OK;
  }
  FTX_REQUIRE(A && G && rows_a >= 1 && rows_g >= 1, "ftx_spconv_pairs_wgrad_bf16: null pointer or empty operand");
  const bool dense = (idx_a == nullptr && idx_g == nullptr && koff == nullptr);
  FTX_REQUIRE(dense || (idx_a && idx_g && koff), "ftx_spconv_pairs_wgrad_bf16: idx_a, idx_g and koff must be all set or all null (dense rows)");
  FTX_REQUIRE(!dense || (kvol == 1 && n_pairs <= rows_a && n_pairs <= rows_g), "ftx_spconv_pairs_wgrad_bf16: dense mode needs kvol == 1 and n_pairs rows in A and G");
  FTX_REQUIRE(n_pairs < 0x7fffffff, "ftx_spconv_pairs_wgrad_bf16: too many pairs");
  const int tile_len = wgrad_bf16_tile_len(n_pairs, ca, cg, kvol);
  const int64_t tiles = ceil_div(n_pairs, tile_len) + kvol;
  const size_t need = sizeof(float) * (size_t)tiles * mat;
  if (!workspace || workspace_bytes < need) {
    set_error("ftx_spconv_pairs_wgrad_bf16: workspace %zu < required %zu", workspace_bytes, need);
    return FTX_EWORKSPACE;
  }
  float *part = (float *)workspace;
  const WgradBf16Cfg c = wgrad_bf16_config(ca, cg);
  dim3 grid((unsigned)tiles, (unsigned)ceil_div(ca, 32 * c.mi * c.wmg), (unsigned)ceil_div(cg, 32 * c.ni * c.wng));
  if (c.mi == 1)
    launch_wgrad_bf16_n<1, 1>(c, grid, st, A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tile_len, part, dW, (int)n_pairs);
  else if (c.mi == 3)
    launch_wgrad_bf16_n<3, 1>(c, grid, st, A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tile_len, part, dW, (int)n_pairs);
  else if (c.wmg == 1)
    launch_wgrad_bf16_n<2, 1>(c, grid, st, A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tile_len, part, dW, (int)n_pairs);
  else
    launch_wgrad_bf16_n<2, 2>(c, grid, st, A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tile_len, part, dW, (int)n_pairs);
  launch_wgrad_reduce(part, koff, kvol, tile_len, (int)n_pairs, mat, tiles, dW, st);
  return check_launch("ftx_spconv_pairs_wgrad_bf16");
}
