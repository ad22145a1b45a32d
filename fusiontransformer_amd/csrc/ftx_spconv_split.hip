// fp32-accurate sparse convolution on the bf16 MFMA: the pair-list GEMM, the dense rows and the weight gradient of ftx_spconv.hip with
// every fp32 operand split into three bf16 pieces as it is staged and six of the nine piece products summed in fp32 on
// v_mfma_f32_32x32x16_bf16 (cfg.MODEL.lidar_split; the dense twin is ftx_dense_split.hip).  Opt-in: the default path stays the exact
// fp32 MFMA of ftx_spconv.hip.
//
// Precision contract (include/ftx.h states it for callers; it is the dense split family's):
//   split     x -> h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), round-to-nearest-even, both subtractions in fp32 (exact): split1 of
//             ftx_split.h, the one definition both families use.  h not finite: m = l = 0.
//   products  hh, hm, mh, hl, lh, mm (first letter: the piece of the gathered operand -- A of the pair GEMM and the dense rows, A of the
//             weight gradient; second: W, or G).  ml, lm, ll are dropped: each below 2.01 * 2^-24 |a b|.
//   order     TWO accumulators per output element: `hh` takes the hh products alone, reduction index ascending; `corr` takes, per
//             16-wide k-step, mm, hl, lh, hm, mh in that order (smallest first).  out = hh + corr: one fp32 add after the last k-step,
//             then the bias.  In the weight gradient the waves of a block that share a sub-tile form wave groups, as in the other
//             families; a group takes one of the two k-steps of a stage, and where there are four groups also one half of the step's
//             products in the order above (mm hl lh | hm mh hh).  Every group adds its two accumulators once, after its last k-step;
//             the group sums are added in group order (wgrad_ks_reduce), the tiles of an offset in tile order (wgrad_reduce_kernel).
//   storage   A, W, G, tmp, out, bias and dW are fp32; tmp has the layout of ftx_spconv_pairs_gemm, so ftx_spconv_reduce, _reduce_stats and
//             _reduce_bn_eval consume it unchanged.
//   No atomics: results are deterministic.  They are not the bits of the fp32 family (another summation tree).
//
// Operand maps of v_mfma_f32_32x32x16_bf16 as in ftx_spconv_bf16.hip: lane (r = lane & 31, h = lane >> 5) holds row r, k = 8h + j of
// each 16-wide k-step; accumulator register g is C[(g&3) + 8(g>>2) + 4h][r].  Both operands are staged as bf16 LDS images with the
// reduction index contiguous, THREE images per operand (h, m, l), 80-byte rows: one conflict-free ds_read_b128 per piece and k-step.
//
// The host layer (validation, tile rules, launches) is ftx_spconv_common.h's, unchanged.  The pair GEMM is a kernel of this family
// and not a third instantiation of pairs_gemm_kernel: that body's instruction placement is measured for the fp32 and bf16 families
// (see its header) and three images with two accumulators are a different stream.
#include "ftx_spconv_common.h"
#include "ftx_split.h"

using namespace ftx;

namespace {

constexpr int kPieces = 3;        // h, m, l
constexpr int kSplitStride = 40;  // bf16 per LDS image row of 32 reduction elements (80 B): the 16 rows of a quarter wave start at 16 distinct
                                  // multiples of four banks, so ds_read_b128 is conflict-free (the dense split family's stride)

// (piece of the MFMA's first operand: W / G, piece of its second: A, accumulator) in the documented order: the five corrections
// smallest first into accumulator 1 (the contract names the A piece first: mm, hl, lh, hm, mh), then hh into accumulator 0
constexpr int kProd[6][3] = {{1, 1, 1}, {2, 0, 1}, {0, 2, 1}, {1, 0, 1}, {0, 1, 1}, {0, 0, 0}};

struct Pieces4 {
  bf16x4 p[kPieces];
};
// the ONE place this family's operands are split
__device__ __forceinline__ Pieces4 split4(float4 v) {
  Pieces4 s;
  __bf16 h, m, l;
  split1(v.x, h, m, l); s.p[0][0] = h; s.p[1][0] = m; s.p[2][0] = l;
  split1(v.y, h, m, l); s.p[0][1] = h; s.p[1][1] = m; s.p[2][1] = l;
  split1(v.z, h, m, l); s.p[0][2] = h; s.p[1][2] = m; s.p[2][2] = l;
  split1(v.w, h, m, l); s.p[0][3] = h; s.p[1][3] = m; s.p[2][3] = l;
  return s;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// tmp[p,:] = A[gather[p],:] @ Wk(p) from the six piece products: the tile of the other families (kPairTile pairs of one offset x 32 NT
// columns, kPairBK channels per step, 4 waves x 32 pairs), their tile scan, gather rule, chunk loads and epilogue; the forms of
// pairs_gemm_kernel (dense rows, scatter list, both orientations of W, the zero-filled reduction of ca % kPairBK != 0).
// LDS: 3 x (128 + 32 NT) rows x 80 B = 61 440 B at NT = 4, under the 64 KB a static array may take; two blocks per CU, and
// __launch_bounds__(256, 2) keeps the kernel at 256 registers so that two do fit.
// ---------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256, 2) void pairs_gemm_split_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ gather,
                                                                  const float *__restrict__ W, int w_transposed, const int32_t *__restrict__ koff,
                                                                  int ca, int co, int kvol, float *__restrict__ tmp, const float *__restrict__ bias,
                                                                  int64_t n_dense, const int32_t *__restrict__ scatter, int64_t rows_out) {
  constexpr int BN = 32 * NT;
  constexpr int STRIDE = kSplitStride;
  constexpr int A_IMG = kPairTile * STRIDE, B_IMG = BN * STRIDE;   // elements per piece image
  constexpr int A_PASSES = kPairAPasses;
  constexpr int B_PASSES = NT;

  __shared__ __attribute__((aligned(16))) __bf16 As[kPieces * A_IMG];   // [piece][pair][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[kPieces * B_IMG];   // [piece][n][k]
  __shared__ int s_tile[3];

  const int tid = threadIdx.x;
  gemm_tile_scan(koff, kvol, n_dense, gather == nullptr, s_tile);
  __syncthreads();
  const int k = s_tile[0];
  if (k < 0) return;  // surplus block of the upper-bound grid
  const int p0 = s_tile[1], cnt = s_tile[2];

  const int wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int n0 = blockIdx.y * BN;
  const int arow = tid >> 3, acol = (tid & 7) * 4;

  const bool kfull = (ca % kPairBK) == 0;
  int32_t src[A_PASSES];
  pair_gather_rows(gather, p0, cnt, rows_a, src);
  const float *Wk = W + (int64_t)k * ca * co;

  f32x16 acc[NT][2];   // [.][0]: hh, [.][1]: the corrections
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[j][c][g] = 0.f;

  float4 ra[A_PASSES], rb[B_PASSES];
  // the chunk loads of pairs_gemm_kernel: unconditional from always-valid addresses where ca is a multiple of kPairBK, zero-filled on a
  // uniform slow path where it is not (the 4-channel stem).  A COPY of that kernel's lambda (ftx_spconv_common.h says why it stays a
  // lambda inside each kernel): the clamping and zero-fill rules keep every load inside its operand, so the two copies change together.
  auto load_chunk = [&](int c0) {
    if (kfull) {
#pragma unroll
      for (int p = 0; p < A_PASSES; ++p) ra[p] = *(const float4 *)&A[(int64_t)src[p] * ca + c0 + acol];
#pragma unroll
      for (int q = 0; q < B_PASSES; ++q) {
        if (!w_transposed) {  // W[k] stored (ca, co): 16 bytes along co; a wave covers 8 k-rows x 128 B
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
  // registers -> the three LDS images of each operand
  auto store_chunk = [&]() {
#pragma unroll
    for (int p = 0; p < A_PASSES; ++p) {
      const Pieces4 s = split4(ra[p]);
#pragma unroll
      for (int c = 0; c < kPieces; ++c) *(bf16x4 *)&As[c * A_IMG + (p * 32 + arow) * STRIDE + acol] = s.p[c];
    }
#pragma unroll
    for (int q = 0; q < B_PASSES; ++q) {
      const Pieces4 s = split4(rb[q]);
      if (!w_transposed) {  // transposing store
        int kk = ((tid >> 6) << 3) + (tid & 7), n4 = (q * 8 + ((tid >> 3) & 7)) * 4;
#pragma unroll
        for (int c = 0; c < kPieces; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) Bs[c * B_IMG + (n4 + e) * STRIDE + kk] = s.p[c][e];
      } else {
        int e = q * 256 + tid;
        int nn = e >> 3, k4 = (e & 7) * 4;
#pragma unroll
        for (int c = 0; c < kPieces; ++c) *(bf16x4 *)&Bs[c * B_IMG + nn * STRIDE + k4] = s.p[c];
      }
    }
  };

  // a lane's fragment rows: pair row wave * 32 + l31 of As, W row l31 of every 32-column tile of Bs, from its half's 8 elements on
  const __bf16 *ap = &As[(wave * 32 + l31) * STRIDE + 8 * half];
  const __bf16 *bp = &Bs[l31 * STRIDE + 8 * half];
  load_chunk(0);
  for (int c0 = 0; c0 < ca; c0 += kPairBK) {
    store_chunk();
    __syncthreads();
    if (c0 + kPairBK < ca) load_chunk(c0 + kPairBK);  // next chunk's global loads fly under the MFMAs
#pragma unroll
    for (int s = 0; s < kPairBK / 16; ++s) {   // a chunk is two k-steps of 16: one ds_read_b128 per piece, operand row and k-step
      bf16x8 af[kPieces];
#pragma unroll
      for (int c = 0; c < kPieces; ++c) af[c] = *(const bf16x8 *)(ap + c * A_IMG + 16 * s);
      // two column tiles at a time, product outermost: the MFMAs between two uses of one accumulator are independent, and the
      // fragments of two tiles (24 registers) keep the NT = 4 kernel within 256 registers without scratch; the order into each
      // accumulator is the documented one either way
#pragma unroll
      for (int j0 = 0; j0 < NT; j0 += 2) {
        constexpr int JN = 2;
        bf16x8 bf[JN][kPieces];
#pragma unroll
        for (int jj = 0; jj < JN; ++jj)
#pragma unroll
          for (int c = 0; c < kPieces; ++c)
            if (j0 + jj < NT) bf[jj][c] = *(const bf16x8 *)(bp + c * B_IMG + (j0 + jj) * 32 * STRIDE + 16 * s);
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int jj = 0; jj < JN; ++jj)
            if (j0 + jj < NT) acc[j0 + jj][kProd[t][2]] = mfma_bf16(bf[jj][kProd[t][0]], af[kProd[t][1]], acc[j0 + jj][kProd[t][2]]);
      }
    }
    __syncthreads();
  }
  f32x16 sum[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) sum[j] = acc[j][0] + acc[j][1];   // the one fp32 add of the two accumulators
  pair_gemm_epilogue<NT>(sum, p0, cnt, n0, gather, rows_a, scatter, rows_out, bias, co, tmp);
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[k] = sum_{p in k} A[idx_a[p],:]^T @ G[idx_g[p],:] from the six piece products
//
// The scheme of pairs_wgrad_bf16_kernel: block = (tile of `tile_len` consecutive pairs of ONE offset, M tile, N tile) -> one (TM x TN)
// partial of dW[k]; each step gathers kWsBR pairs row-major and stores them transposed as k-contiguous bf16 images [channel][pair], two
// pairs packed per 32-bit LDS write, here three images per operand.
//
// LDS budget.  Three 32-pair-deep images of a 128 x 128 tile are 3 x 256 x 80 B = 61 440 B, and with the 9 KB index round of the other
// families (kWgradRound = 1024 pairs) that passes the 64 KB a static array may take.  Of the three ways out this family takes the
// SMALLER INDEX ROUND, kWsRound = 256 pairs (2 304 B; 63 764 B in all at 128 x 128):
//   * a 16-deep stage (one k-step) would halve the MFMA work between two barriers on every tile shape, the small ones included;
//   * dynamic LDS with the function attribute would keep the round but costs a host call per instantiation that can fail, and a tile
//     above 80 KB leaves one block per CU;
//   * a round of 256 pairs costs three more barriers per 256 pairs (8 stages), on every tile, and nothing else: the round is not
//     part of any sum, so tile length, workspace and summation tree keep the other families' rules.
// The stage stays 32 deep, so wgrad_step (two staged steps) is 64, the fp32 family's.
// The 80-byte row is chosen for the READ side (conflict-free ds_read_b128).  The transposed 32-bit stores pay for it: the four channels
// of an item are 20 banks apart and consecutive items 80, so a wave's store hits some banks several times (the bf16 family's 144-byte
// row is the stride picked for its stores).  That cost has not been measured on its own; the kernel's time as a whole is in DESIGN section 5.
//
// A stage is two k-steps, so the KS = 4 / (WMG WNG) wave groups cannot all take a k-step of their own where KS = 4 (tiles of one wave):
// group ks takes k-step ks & 1 and half ks >> 1 of its six products (mm hl lh | hm mh hh), three MFMAs per sub-tile each.
// __launch_bounds__(256, 2) on the tiles of up to four sub-tiles per wave keeps them at 256 registers (they took 260-264 without it,
// one block per CU where LDS admits two); no instantiation uses scratch.
// ---------------------------------------------------------------------------------------
constexpr int kWsBR = 32;       // pairs staged per step: two k-steps of 16
constexpr int kWsRound = 256;   // pair indices kept in LDS at a time

template <int MI, int NI, int WMG, int WNG>
__global__ __launch_bounds__(256, MI * NI <= 4 ? 2 : 1) void pairs_wgrad_split_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ idx_a,
                                                                const float *__restrict__ G, int64_t rows_g, const int32_t *__restrict__ idx_g,
                                                                const int32_t *__restrict__ koff, int ca, int cg, int kvol, int tile_len,
                                                                float *__restrict__ part, float *__restrict__ dW, int n_dense) {
  // idx_a == nullptr: dense mode, rows [0, n_dense) of A and G pair up one to one (kvol = 1)
  constexpr int TM = 32 * MI * WMG, TN = 32 * NI * WNG, KS = 4 / (WMG * WNG);
  constexpr int STRIDE = kSplitStride;
  constexpr int A_IMG = TM * STRIDE, G_IMG = TN * STRIDE;                     // elements per piece image
  constexpr int STAGE_B = kPieces * (TM + TN) * STRIDE * 2;                   // bytes
  constexpr int RED_B = KS > 1 ? MI * NI * 1024 * WMG * WNG * 4 : 0;          // bytes: one KS group's sums
  constexpr int LDS_B = STAGE_B > RED_B ? STAGE_B : RED_B;
  static_assert(kWsRound % kWsBR == 0 && kWsBR == 32, "a round is whole stages of two k-steps");
  __shared__ __attribute__((aligned(16))) char lds[LDS_B];
  __shared__ int32_t s_ia[kWsRound], s_ig[kWsRound];
  __shared__ uint8_t s_ok[kWsRound];
  __shared__ int s_tile[4];
  __shared__ int s_bad;
  __bf16 *At = (__bf16 *)lds, *Gt = At + kPieces * A_IMG;

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

  f32x16 acc[MI][NI][2];   // [.][.][0]: hh, [.][.][1]: the corrections
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[i][j][c][g] = 0.f;

  // Staging item = (pair pair pp, 4 channels c4): two float4 gathers, stored as 4 packed bf16 pairs per piece.  A stage holds
  // (T / 4) x 16 items per operand, T / 64 per thread: with a 32- or 96-channel side the last pass has items for half the threads
  // only, the others repeat item 0's loads and store nothing.  Loads are unconditional from always-valid addresses: indices clamped
  // to real rows, channels to the last float4 of a row (what a channel >= ca (cg) brings in only reaches accumulator rows / columns
  // the epilogue never stores); pairs past the end of the tile and malformed pairs are zeroed at store time on a block-uniform slow
  // path.
  constexpr int QA = (TM + 63) / 64, QG = (TN + 63) / 64;
  float4 ra[QA][2], rg[QG][2];
  int pa[QA], pg[QG], ca_off[QA], cg_off[QG], ra_row[QA], rg_row[QG];
  bool a_on[QA], g_on[QG];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    int e = q * 256 + tid;
    a_on[q] = e < 4 * TM;
    if (!a_on[q]) e = 0;
    pa[q] = 2 * (e / (TM / 4));
    ra_row[q] = (e % (TM / 4)) * 4;
    int c = m0 + ra_row[q];
    ca_off[q] = c + 4 <= ca ? c : ca - 4;
  }
#pragma unroll
  for (int q = 0; q < QG; ++q) {
    int e = q * 256 + tid;
    g_on[q] = e < 4 * TN;
    if (!g_on[q]) e = 0;
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
    if (p0 + kWsBR > rend || s_bad) {   // block-uniform: last step of the tile (or a malformed pair list)
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
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      if (!a_on[q]) continue;
      const Pieces4 x0 = split4(ra[q][0]), x1 = split4(ra[q][1]);
#pragma unroll
      for (int c = 0; c < kPieces; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) *(bf16x2 *)&At[c * A_IMG + (ra_row[q] + e) * STRIDE + pa[q]] = (bf16x2){x0.p[c][e], x1.p[c][e]};
    }
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      if (!g_on[q]) continue;
      const Pieces4 x0 = split4(rg[q][0]), x1 = split4(rg[q][1]);
#pragma unroll
      for (int c = 0; c < kPieces; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) *(bf16x2 *)&Gt[c * G_IMG + (rg_row[q] + e) * STRIDE + pg[q]] = (bf16x2){x0.p[c][e], x1.p[c][e]};
    }
  };
  const __bf16 *ap = At + (wm * MI * 32 + l31) * STRIDE + 8 * half;
  const __bf16 *gp = Gt + (wn * NI * 32 + l31) * STRIDE + 8 * half;
  // products [T0, T1) of kProd on k-step s of the stage; rows: g-channel, cols: a-channel
  auto k_step = [&](int s, auto T0, auto T1) {
    bf16x8 af[MI][kPieces], gf[NI][kPieces];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int c = 0; c < kPieces; ++c) af[i][c] = *(const bf16x8 *)(ap + c * A_IMG + i * 32 * STRIDE + 16 * s);
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int c = 0; c < kPieces; ++c) gf[j][c] = *(const bf16x8 *)(gp + c * G_IMG + j * 32 * STRIDE + 16 * s);
#pragma unroll
    for (int t = decltype(T0)::value; t < decltype(T1)::value; ++t)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j][kProd[t][2]] = mfma_bf16(gf[j][kProd[t][0]], af[i][kProd[t][1]], acc[i][j][kProd[t][2]]);
  };
  using std::integral_constant;
  auto mfma_step = [&]() {
    if constexpr (KS == 1) {
      k_step(0, integral_constant<int, 0>{}, integral_constant<int, 6>{});
      k_step(1, integral_constant<int, 0>{}, integral_constant<int, 6>{});
    } else if constexpr (KS == 2) {
      k_step(ks, integral_constant<int, 0>{}, integral_constant<int, 6>{});
    } else {
      if ((ks >> 1) == 0) k_step(ks & 1, integral_constant<int, 0>{}, integral_constant<int, 3>{});
      else k_step(ks & 1, integral_constant<int, 3>{}, integral_constant<int, 6>{});
    }
  };

  for (rbase = lo; rbase < hi; rbase += kWsRound) {
    rend = (rbase + kWsRound < hi) ? rbase + kWsRound : hi;
    wgrad_stage_indices<kWsRound>(idx_a, rows_a, idx_g, rows_g, rbase, rend, s_ia, s_ig, s_ok, &s_bad);
    load_step(rbase);
    for (int p0 = rbase; p0 < rend; p0 += kWsBR) {
      store_step(p0);
      __syncthreads();
      if (p0 + kWsBR < rend) load_step(p0 + kWsBR);   // next step's gathers fly under this step's MFMAs
      mfma_step();
      __syncthreads();
    }
  }

  f32x16 sum[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) sum[i][j] = acc[i][j][0] + acc[i][j][1];   // the one fp32 add of the group's two accumulators
  wgrad_ks_reduce<MI, NI, KS>(sum, (float *)lds, wq, ks, lane);   // the KS wave groups, in group order (the staging images are free now)

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
              *(float4 *)&dst[(int64_t)row * cg + col] = make_float4(sum[i][j][4 * q], sum[i][j][4 * q + 1], sum[i][j][4 * q + 2], sum[i][j][4 * q + 3]);
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// the family's description and entries (ftx_spconv_common.h): the tile rules of the other families with this family's table and step
// ---------------------------------------------------------------------------------------
struct SpconvSplit {
  static constexpr const char *pairs_name = "ftx_spconv_pairs_gemm_split", *scatter_name = "ftx_spconv_pairs_gemm_scatter_split",
                              *rows_name = "ftx_rows_gemm_split", *wgrad_name = "ftx_spconv_pairs_wgrad_split";
  // .vgpr_count 92 / 126-130 / 156-194 / 230-232 / 388-392; the 128 x 128 tile: 2 by LDS (63 764 B) and by registers
  static constexpr int wgrad_blocks[4][4] = {{5, 4, 2, 3}, {3, 2, 1, 2}, {2, 1, 1, 1}, {3, 2, 1, 2}};
  static constexpr int wgrad_step = 2 * kWsBR;
  template <int NT>
  static void gemm(dim3 grid, hipStream_t st, const PairsGemmArgs &a) {
    pairs_gemm_split_kernel<NT><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.gather, a.W, a.w_transposed, a.koff, a.ca, a.co, a.kvol, a.out, a.bias,
                                                      a.n_dense, a.scatter, a.rows_out);
  }
  template <int MI, int NI, int WMG, int WNG>
  static void wgrad(dim3 grid, hipStream_t st, const PairsWgradArgs &a) {
    pairs_wgrad_split_kernel<MI, NI, WMG, WNG><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.idx_a, a.G, a.rows_g, a.idx_g, a.koff, a.ca, a.cg, a.kvol,
                                                                     a.tile_len, a.part, a.dW, a.n_dense);
  }
};

extern "C" int32_t ftx_spconv_gemm_split_block_cols(int32_t co, int64_t n_pairs, int32_t kvol) { return spconv_gemm_block_cols(co, n_pairs, kvol); }

extern "C" int ftx_spconv_pairs_gemm_split(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed,
                                           const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream) {
  return spconv_pairs_entry<SpconvSplit>(false, A, rows_a, gather, nullptr, W, w_transposed, koff, n_pairs, ca, co, kvol, tmp, 0, stream);
}

extern "C" int ftx_spconv_pairs_gemm_scatter_split(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W,
                                                   int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol,
                                                   float *out, int64_t rows_out, void *stream) {
  return spconv_pairs_entry<SpconvSplit>(true, A, rows_a, gather, scatter, W, w_transposed, koff, n_pairs, ca, co, kvol, out, rows_out, stream);
}

extern "C" int ftx_rows_gemm_split(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co,
                                   float *out, void *stream) {
  return spconv_rows_entry<SpconvSplit>(A, n, W, w_transposed, bias, ca, co, out, stream);
}

extern "C" int32_t ftx_spconv_wgrad_split_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng) {
  return spconv_wgrad_table_blocks<SpconvSplit>(mi, wmg, ni, wng);
}

extern "C" size_t ftx_spconv_pairs_wgrad_split_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol) {
  return spconv_wgrad_workspace_bytes<SpconvSplit>(n_pairs, ca, cg, kvol);
}

extern "C" int ftx_spconv_pairs_wgrad_split(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g,
                                            const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace,
                                            size_t workspace_bytes, void *stream) {
  return spconv_wgrad_entry<SpconvSplit>(A, rows_a, idx_a, G, rows_g, idx_g, koff, n_pairs, ca, cg, kvol, dW, workspace, workspace_bytes, stream);
}
