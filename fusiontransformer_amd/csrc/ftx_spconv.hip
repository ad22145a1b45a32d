// Sparse convolution on gfx950 as  pair-list gather-GEMM  +  ordered reduce.
//
// A kernel map is stored as ONE compacted pair list, sorted by (offset k, output row):
//   pair_in[p], pair_out[p]            rows of the input / output tensor joined by pair p
//   koff[k] .. koff[k+1]               the pairs of offset k
//   pos[k, o] / pos_t[k, i]            position of the pair (k,o) / (k,i) in the list, or -1
//
//   forward      tmp[p]  = in[pair_in[p]]   @ W[k(p)]        out[o] = sum_k tmp[pos[k,o]]
//   data grad    tmp[p]  = gout[pair_out[p]] @ W[k(p)]^T     gin[i] = sum_k tmp[pos_t[k,i]]
//   weight grad  dW[k]   = sum_{p in k} in[pair_in[p]]^T @ gout[pair_out[p]]
//
// Only real (in,out) pairs reach the matrix cores (an output-stationary implicit GEMM spends
// ~80% of its MFMAs on absent neighbours: a voxel has ~5-9 of 27), every tile of 128 pairs
// shares one W[k], and the reduce adds each row's <= 27 partial rows in fixed k order: no float
// atomics anywhere, results are bit-reproducible.  tmp costs one extra streamed write + read of
// P x co floats, which is cheaper than the atomic rate (1.3 TB/s) by ~4x.
//
// MFMA: exact-fp32 v_mfma_f32_32x32x2_f32.  Operand maps (cdna_hip_programming.md §3): A operand
// lane l holds A[i=l&31][k=l>>5], B operand lane l holds B[k=l>>5][j=l&31]; accumulator reg g of
// lane l is C[row=(g&3)+8*(g>>2)+4*(l>>5)][col=l&31].  The reduction index may be permuted as
// long as A and B agree: lane half h consumes k = 8t+4h+s for MFMA s of group t, so the A fragment
// of four MFMAs is ONE ds_read_b128 (row stride 36 floats -> conflict-free).
#include <cstring>
#include <cstdlib>
#include "ftx_bn_eval_op.h"
#include "ftx_index_ops.h"
#include "ftx_lastblock.h"
#include "ftx_spconv_common.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

using namespace ftx;

// ---------------------------------------------------------------------------------------
// pair lists
// ---------------------------------------------------------------------------------------
struct IsValid {
  __host__ __device__ int32_t operator()(int32_t v) const { return v >= 0 ? 1 : 0; }
};

extern "C" size_t ftx_kernel_map_count_workspace_bytes(int64_t n_out, int32_t k) {
  if (n_out <= 0 || k <= 0) return 256;
  size_t bytes = 0;
  const int32_t *in = nullptr;
  int32_t *out = nullptr;
  auto it = rocprim::make_transform_iterator(in, IsValid());
  if (rocprim::exclusive_scan(nullptr, bytes, it, out, 0, (size_t)(n_out * k), rocprim::plus<int32_t>()) != hipSuccess) return 0;
  return bytes + 256;
}

__global__ void koff_kernel(const int32_t *__restrict__ nbr, const int32_t *__restrict__ scan, int64_t n_out, int k, int32_t *__restrict__ koff) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t <= k) koff[t] = koff_entry(nbr, scan, n_out, k, t, 0);
}

extern "C" int ftx_kernel_map_count(const int32_t *nbr, int64_t n_out, int32_t k, int32_t *pos, int32_t *koff, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  FTX_REQUIRE(n_out >= 0 && k >= 1, "ftx_kernel_map_count: bad size");
  FTX_REQUIRE(koff, "ftx_kernel_map_count: null koff");
  hipStream_t st = (hipStream_t)stream;
  if (n_out == 0) {
    if (hipMemsetAsync(koff, 0, sizeof(int32_t) * (k + 1), st) != hipSuccess) return check_launch("ftx_kernel_map_count memset");
    return FTX_OK;
  }
  FTX_REQUIRE(nbr && pos && workspace, "ftx_kernel_map_count: null pointer");
  FTX_REQUIRE(n_out * k < 0x7fffffff, "ftx_kernel_map_count: map too large for int32 positions");
  size_t need = ftx_kernel_map_count_workspace_bytes(n_out, k);
  if (workspace_bytes < need) return workspace_short("ftx_kernel_map_count", workspace_bytes, need);
  size_t bytes = workspace_bytes;
  auto it = rocprim::make_transform_iterator(nbr, IsValid());
  // pos temporarily holds the exclusive scan of the validity flags (k-major = sorted by (k, row))
  if (rocprim::exclusive_scan(workspace, bytes, it, pos, 0, (size_t)(n_out * k), rocprim::plus<int32_t>(), st) != hipSuccess) {
    set_error("ftx_kernel_map_count: scan failed");
    return FTX_ELAUNCH;
  }
  koff_kernel<<<1, 64, 0, st>>>(nbr, pos, n_out, k, koff);
  return check_launch("ftx_kernel_map_count");
}

__global__ void fill_m1_kernel(int32_t *__restrict__ p, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = -1;
}

__global__ void pairs_scatter_kernel(const int32_t *__restrict__ nbr, int64_t n_out, int64_t n_in, int k, int32_t *__restrict__ pos,
                                     int32_t *__restrict__ pos_t, int32_t *__restrict__ pair_in, int32_t *__restrict__ pair_out,
                                     int64_t cap) {
  const int64_t total = n_out * k;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    // pos[e] is this map's own scan, never negative, and already the position where there is a pair
    if (pair_entry(nbr[e], pos[e], e, n_out, n_in, cap, pair_in, pair_out, pos_t) < 0) pos[e] = -1;
  }
}

extern "C" int ftx_kernel_map_pairs(const int32_t *nbr, int64_t n_out, int64_t n_in, int32_t k, int32_t *pos, int32_t *pos_t, int32_t *pair_in,
                                    int32_t *pair_out, int64_t n_pairs, void *stream) {
  FTX_REQUIRE(n_out >= 0 && n_in >= 0 && k >= 1 && n_pairs >= 0, "ftx_kernel_map_pairs: bad size");
  hipStream_t st = (hipStream_t)stream;
  if (n_in > 0) {
    FTX_REQUIRE(pos_t, "ftx_kernel_map_pairs: null pos_t");
    fill_m1_kernel<<<grid_for(n_in * k, 256), 256, 0, st>>>(pos_t, n_in * k);
  }
  if (n_out == 0) return check_launch("ftx_kernel_map_pairs");
  FTX_REQUIRE(nbr && pos && (n_pairs == 0 || (pair_in && pair_out)), "ftx_kernel_map_pairs: null pointer");
  pairs_scatter_kernel<<<grid_for(n_out * k, 256), 256, 0, st>>>(nbr, n_out, n_in, k, pos, pos_t, pair_in, pair_out, n_pairs);
  return check_launch("ftx_kernel_map_pairs");
}

// ---------------------------------------------------------------------------------------
// phase 1: tmp[p,:] = A[gather[p],:] @ Wk(p)        (tiles of 128 pairs of one offset)
// ---------------------------------------------------------------------------------------
// pairs_gemm_kernel<SpconvF32, NT> of ftx_spconv_common.h, the body that both families instantiate.  One pair-GEMM kernel ships: the
// LDS-DMA, producer / consumer and bf16x3 variants of rounds 1-2 each tied or lost against it
// (DESIGN.md section 8); their sources live under tools/probes/spconv_variants/ and are not part of libftx.so.

// ---------------------------------------------------------------------------------------
// phase 2: out[r,:] = sum_k tmp[pos[k,r],:]   (fixed k order; rows without pairs become 0)
// ---------------------------------------------------------------------------------------
// Channels j .. j+3 of output row r: the rows tmp[pos[k, r]] of its pairs, added in ascending k.  KVOL > 0 is the offset count at
// compile time (all positions are read first, then the valid rows), KVOL == 0 takes it from `kvol`.
template <int KVOL>
__device__ __forceinline__ float4 reduce_row(const float *__restrict__ tmp, const int32_t *__restrict__ pos, int64_t n, int co, int kvol,
                                             int64_t r, int j) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (KVOL > 0) {
    int32_t p[KVOL > 0 ? KVOL : 1];
#pragma unroll
    for (int k = 0; k < KVOL; ++k) p[k] = pos[(int64_t)k * n + r];
#pragma unroll
    for (int k = 0; k < KVOL; ++k) {
      if (p[k] >= 0) {
        float4 v = *(const float4 *)&tmp[(int64_t)p[k] * co + j];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  } else {
    for (int k = 0; k < kvol; ++k) {
      int32_t q = pos[(int64_t)k * n + r];
      if (q >= 0) {
        float4 v = *(const float4 *)&tmp[(int64_t)q * co + j];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  }
  return acc;
}

template <int KVOL>
__global__ void spconv_reduce_kernel(const float *__restrict__ tmp, const int32_t *__restrict__ pos, int64_t n, int co, int kvol,
                                     float *__restrict__ out) {
  const int cv = co >> 2;
  const int64_t total = n * cv;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = e / cv;
    int j = (int)(e - r * cv) * 4;
    const float4 acc = reduce_row<KVOL>(tmp, pos, n, co, kvol, r, j);
    *(float4 *)&out[r * co + j] = acc;
  }
}

// Grid of the two plain reduces: one thread per float4 of the output, at most 8192 blocks of 256.
static unsigned reduce_grid(int64_t n, int co) {
  int64_t g = ceil_div(n * (co / 4), 256);
  if (g > 8192) g = 8192;
  return (unsigned)g;
}

extern "C" int ftx_spconv_reduce(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, float *out, void *stream) {
  FTX_REQUIRE(n >= 0 && kvol >= 1 && co >= 4 && co % 4 == 0, "ftx_spconv_reduce: bad size");
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(pos && out, "ftx_spconv_reduce: null pointer");
  const unsigned g = reduce_grid(n, co);
  hipStream_t st = (hipStream_t)stream;
  if (kvol == 27)
    spconv_reduce_kernel<27><<<g, 256, 0, st>>>(tmp, pos, n, co, kvol, out);
  else if (kvol == 8)
    spconv_reduce_kernel<8><<<g, 256, 0, st>>>(tmp, pos, n, co, kvol, out);
  else
    spconv_reduce_kernel<0><<<g, 256, 0, st>>>(tmp, pos, n, co, kvol, out);
  return check_launch("ftx_spconv_reduce");
}

// The same reduce with the eval-mode BatchNorm (+ residual) (+ ReLU) applied to the row before its one store: what ftx_spconv_reduce
// followed by ftx_bn_eval_fwd computes, bit for bit (positions first, then the valid rows in ascending k, then bn_eval_elem on the
// four sums), in one launch and without the (n, co) round trip through memory.
template <int KVOL>
__global__ void spconv_reduce_bn_eval_kernel(const float *__restrict__ tmp, const int32_t *__restrict__ pos, int64_t n, int co,
                                             const float *__restrict__ res, const float *__restrict__ gamma, const float *__restrict__ beta,
                                             const float *__restrict__ rm, const float *__restrict__ rv, float eps, int relu,
                                             float *__restrict__ out) {
  const int cv = co >> 2;
  const int64_t total = n * cv;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = e / cv;
    int j = (int)(e - r * cv) * 4;
    const float4 acc = reduce_row<KVOL>(tmp, pos, n, co, KVOL, r, j);
    *(float4 *)&out[r * co + j] = bn_eval_apply4(acc, res, r * co + j, rm, rv, eps, gamma, beta, j, relu);
  }
}

extern "C" int ftx_spconv_reduce_bn_eval(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, const float *residual,
                                         const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                                         float eps, int32_t relu, float *out, void *stream) {
  FTX_REQUIRE(n >= 0 && co >= 4 && co % 4 == 0, "ftx_spconv_reduce_bn_eval: bad size (n=%lld, co=%d must be a multiple of 4)", (long long)n, co);
  FTX_REQUIRE(kvol == 27 || kvol == 8, "ftx_spconv_reduce_bn_eval: kvol must be 8 or 27, got %d", kvol);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(pos && out && gamma && beta && running_mean && running_var, "ftx_spconv_reduce_bn_eval: null pointer");
  const unsigned g = reduce_grid(n, co);
  hipStream_t st = (hipStream_t)stream;
  if (kvol == 27)
    spconv_reduce_bn_eval_kernel<27><<<g, 256, 0, st>>>(tmp, pos, n, co, residual, gamma, beta, running_mean, running_var, eps, relu, out);
  else
    spconv_reduce_bn_eval_kernel<8><<<g, 256, 0, st>>>(tmp, pos, n, co, residual, gamma, beta, running_mean, running_var, eps, relu, out);
  return check_launch("ftx_spconv_reduce_bn_eval");
}

// The same reduce, also producing the BatchNorm statistics of its output (sum and sum of squares per channel, float64) as
// per-block partials: the BatchNorm that follows every convolution (models/spvcnn.py:22-35,53-79) then needs no pass of its own
// over `out`.  Block = (256 / (co/4)) rows x co/4 float4 columns over a contiguous row range; a thread keeps one column, so its
// eight float64 sums stay in registers; rows of a block are summed in a fixed order and blocks are combined in block order by
// ftx_lastblock.h (then one apply launch, ftx_bn_train_fwd_totals): the statistics do not depend on the launch geometry beyond `nb`, and are bit-reproducible.
template <int KVOL>
__global__ __launch_bounds__(256) void spconv_reduce_stats_kernel(const float *__restrict__ tmp, const int32_t *__restrict__ pos, int64_t n, int co,
                                                                  int kvol, float *__restrict__ out, double *part, StreamScratch sc) {
  extern __shared__ double sh[];  // [2][RL][co]
  const auto [cv, RL] = row_lanes(co);
  const int tid = threadIdx.x;
  const int cg = tid % cv, rl = tid / cv;
  const int64_t rows_per_block = ceil_div(n, (int64_t)gridDim.x);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (rl < RL) {
    const int j = cg * 4;
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      const float4 acc = reduce_row<KVOL>(tmp, pos, n, co, kvol, r, j);
      *(float4 *)&out[r * co + j] = acc;
      s0[0] += (double)acc.x; s1[0] += (double)acc.x * (double)acc.x;
      s0[1] += (double)acc.y; s1[1] += (double)acc.y * (double)acc.y;
      s0[2] += (double)acc.z; s1[2] += (double)acc.z * (double)acc.z;
      s0[3] += (double)acc.w; s1[3] += (double)acc.w * (double)acc.w;
    }
  }
  colstats_block_tail(s0, s1, rl, cg, RL, co, sh, part, sc);
}

extern "C" int32_t ftx_spconv_reduce_stats_blocks(int64_t n, int32_t co) {
  if (n <= 0 || co < 4) return 1;
  int64_t b = ceil_div(n, 2 * row_lanes(co).RL);   // ~2 rows per thread
  if (b > 2048) b = 2048;
  return (int32_t)(b < 1 ? 1 : b);
}

extern "C" int ftx_spconv_reduce_stats(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, float *out, double *part,
                                       int32_t nb, void *stream) {
  FTX_REQUIRE(n >= 1 && kvol >= 1 && co >= 4 && co % 4 == 0 && co <= 512, "ftx_spconv_reduce_stats: bad size (co must be a multiple of 4 in [4, 512])");
  FTX_REQUIRE(pos && out && part, "ftx_spconv_reduce_stats: null pointer");
  FTX_REQUIRE(nb == ftx_spconv_reduce_stats_blocks(n, co), "ftx_spconv_reduce_stats: nb must come from ftx_spconv_reduce_stats_blocks");
  hipStream_t st = (hipStream_t)stream;
  const StreamScratch sc = stream_scratch(st);
  if (!sc.counters) return FTX_ELAUNCH;
  const size_t lds = colstats_lds_bytes(co);
  if (kvol == 27)
    spconv_reduce_stats_kernel<27><<<nb, 256, lds, st>>>(tmp, pos, n, co, kvol, out, part, sc);
  else if (kvol == 8)
    spconv_reduce_stats_kernel<8><<<nb, 256, lds, st>>>(tmp, pos, n, co, kvol, out, part, sc);
  else
    spconv_reduce_stats_kernel<0><<<nb, 256, lds, st>>>(tmp, pos, n, co, kvol, out, part, sc);
  return check_launch("ftx_spconv_reduce_stats");
}

// ---------------------------------------------------------------------------------------
// weight gradient: dW[k] = sum_{p in k} A[idx_a[p],:]^T @ G[idx_g[p],:]
//
// Block = (tile of `tile_len` consecutive pairs of ONE offset, M tile, N tile) -> one (TM x TN) partial of dW[k]; the partials of
// an offset are summed by an ordered second pass (an offset that fits one tile is written straight into dW[k]).
//
// The reduction index is the PAIR, so the gathered rows are staged row-major ([pair][channel], 16-byte stores) and used as they
// are: a wave's (32 MI) x (32 NI) piece of the tile takes channels  base + MI*i + mi  /  base + NI*j + ni  for MFMA index i / j,
// i.e. the MI (NI) sub-tiles interleave.  One lane then needs MI (NI) CONSECUTIVE floats of a staged row per reduction step: a
// single ds_read_b64 / b128 per operand feeds MI*NI MFMAs (the previous kernel fed every MFMA from its own ds_read_b32), and the
// accumulator registers of a lane hold 4*NI consecutive g-channels of MI a-channel rows, so the epilogue is 16-byte stores.
// Waves: WMG x WNG x KS = 4; KS > 1 splits the pairs of each step and sums the KS groups through LDS in a fixed order.
// ---------------------------------------------------------------------------------------
constexpr int WG_BR = 32;       // pairs staged per step

template <int N> struct FragLoad;
template <> struct FragLoad<1> { static __device__ __forceinline__ void ld(const float *p, float (&f)[1]) { f[0] = *p; } };
template <> struct FragLoad<2> { static __device__ __forceinline__ void ld(const float *p, float (&f)[2]) { float2 v = *(const float2 *)p; f[0] = v.x; f[1] = v.y; } };
template <> struct FragLoad<3> { static __device__ __forceinline__ void ld(const float *p, float (&f)[3]) { f[0] = p[0]; f[1] = p[1]; f[2] = p[2]; } };
template <> struct FragLoad<4> { static __device__ __forceinline__ void ld(const float *p, float (&f)[4]) { float4 v = *(const float4 *)p; f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; } };

template <int MI, int NI, int WMG, int WNG>
__global__ __launch_bounds__(256) void pairs_wgrad_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ idx_a,
                                                          const float *__restrict__ G, int64_t rows_g, const int32_t *__restrict__ idx_g,
                                                          const int32_t *__restrict__ koff, int ca, int cg, int kvol, int tile_len,
                                                          float *__restrict__ part, float *__restrict__ dW, int n_dense) {
  // idx_a == nullptr: dense mode, rows [0, n_dense) of A and G pair up one to one (kvol = 1)
  constexpr int TM = 32 * MI * WMG, TN = 32 * NI * WNG, KS = 4 / (WMG * WNG);
  constexpr int STAGE = WG_BR * (TM + TN);                 // floats
  constexpr int RED = KS > 1 ? MI * NI * 1024 * WMG * WNG : 0;  // floats: one KS group's accumulators
  constexpr int LDSF = STAGE > RED ? STAGE : RED;
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  __shared__ int32_t s_ia[kWgradRound], s_ig[kWgradRound];
  __shared__ uint8_t s_ok[kWgradRound];
  __shared__ int s_tile[4];
  __shared__ int s_bad;
  float *As = lds, *Gs = lds + WG_BR * TM;

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

  // Two register stages: the gathers of step s+2 are issued while step s is in the matrix cores, so a block hides its own load
  // latency (blocks of one CU start together and stay in lockstep, so relying on the other resident blocks does not work).
  //
  // The gathers are UNCONDITIONAL loads from addresses that are always valid: the staged indices are clamped to real rows and the
  // channel offset to the last float4 of a row.  What such a load brings in for a channel >= ca (cg) only ever reaches
  // accumulator rows / columns >= ca (cg), which the epilogue never stores, so padded channels need no masking at all; pairs past
  // the end of the tile (and pairs with an out-of-range index) are zeroed at LDS-store time, on a block-uniform slow path that a
  // tile enters for its last step only.  (With a branch per load, as before, every load waited for its own index read:
  // ~16 serialised LDS round trips per step.)
  constexpr int QA = TM / 32, QG = TN / 32;   // float4 per thread per step and operand
  float4 ra0[QA], rg0[QG], ra1[QA], rg1[QG];
  int rbase = lo, rend = lo;
  int pra[QA], prg[QG], ca_off[QA], cg_off[QG];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    int e = q * 256 + tid;
    pra[q] = e / (TM / 4);
    int c = m0 + (e - pra[q] * (TM / 4)) * 4;
    ca_off[q] = c + 4 <= ca ? c : ca - 4;
  }
#pragma unroll
  for (int q = 0; q < QG; ++q) {
    int e = q * 256 + tid;
    prg[q] = e / (TN / 4);
    int c = n0 + (e - prg[q] * (TN / 4)) * 4;
    cg_off[q] = c + 4 <= cg ? c : cg - 4;
  }
  auto load_step = [&](int p0, float4 (&ra)[QA], float4 (&rg)[QG]) {
    const int o = p0 - rbase;
    if (o >= kWgradRound) return;   // past this round's indices: the step is never consumed
    int32_t ia[QA], ig[QG];
#pragma unroll
    for (int q = 0; q < QA; ++q) ia[q] = s_ia[(o + pra[q]) & (kWgradRound - 1)];
#pragma unroll
    for (int q = 0; q < QG; ++q) ig[q] = s_ig[(o + prg[q]) & (kWgradRound - 1)];
#pragma unroll
    for (int q = 0; q < QA; ++q) ra[q] = *(const float4 *)(A + ((int64_t)ia[q] * ca + ca_off[q]));
#pragma unroll
    for (int q = 0; q < QG; ++q) rg[q] = *(const float4 *)(G + ((int64_t)ig[q] * cg + cg_off[q]));
  };
  auto store_step = [&](int p0, float4 (&ra)[QA], float4 (&rg)[QG]) {
    if (p0 + WG_BR > rend || s_bad) {   // block-uniform: last step of the tile (or a malformed pair list)
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        const int p = p0 + pra[q];
        if (p >= rend || s_ok[(p - rbase) & (kWgradRound - 1)] == 0) ra[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < QG; ++q) {
        const int p = p0 + prg[q];
        if (p >= rend || s_ok[(p - rbase) & (kWgradRound - 1)] == 0) rg[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int q = 0; q < QA; ++q) *(float4 *)&As[(q * 256 + tid) * 4] = ra[q];   // row-major [pair][TM]: e*4 == pr*TM + c4
#pragma unroll
    for (int q = 0; q < QG; ++q) *(float4 *)&Gs[(q * 256 + tid) * 4] = rg[q];
  };
  const float *ap = As + wm * 32 * MI + MI * l31, *gp = Gs + wn * 32 * NI + NI * l31;
  auto mfma_step = [&]() {
    constexpr int ITS = WG_BR / 2 / KS;
    float af[2][MI], gf[2][NI];
    auto frag = [&](int buf, int it) {
      const int kk = 2 * (it * KS + ks) + half;
      FragLoad<MI>::ld(ap + kk * TM, af[buf]);
      FragLoad<NI>::ld(gp + kk * TN, gf[buf]);
    };
    frag(0, 0);
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      if (it + 1 < ITS) frag((it + 1) & 1, it + 1);   // next fragments in flight under this step's MFMAs
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[it & 1][j], af[it & 1][i], acc[i][j], 0, 0, 0);  // rows: g-channel, cols: a-channel
    }
  };

  for (rbase = lo; rbase < hi; rbase += kWgradRound) {
    rend = (rbase + kWgradRound < hi) ? rbase + kWgradRound : hi;
    wgrad_stage_indices(idx_a, rows_a, idx_g, rows_g, rbase, rend, s_ia, s_ig, s_ok, &s_bad);
    load_step(rbase, ra0, rg0);
    load_step(rbase + WG_BR, ra1, rg1);
    for (int p0 = rbase; p0 < rend; p0 += 2 * WG_BR) {
      store_step(p0, ra0, rg0);
      __syncthreads();
      load_step(p0 + 2 * WG_BR, ra0, rg0);
      mfma_step();
      __syncthreads();
      if (p0 + WG_BR >= rend) break;
      store_step(p0 + WG_BR, ra1, rg1);
      __syncthreads();
      load_step(p0 + 3 * WG_BR, ra1, rg1);
      mfma_step();
      __syncthreads();
    }
  }

  wgrad_ks_reduce<MI, NI, KS>(acc, lds, wq, ks, lane);   // the pair-subsets of the KS wave groups (the staging buffers are free now)

  if (ks == 0) {
    const int64_t mat = (int64_t)ca * cg;
    float *dst = single ? dW + (int64_t)k * mat : part + (int64_t)blockIdx.x * mat;   // tiles are numbered in offset order
    // accumulator register 4q + e of lane (l31, half) is g-row 8q + 4*half + e of sub-tile (i, j): g-channel gb + NI*(8q+4half+e) + j,
    // a-channel ab + MI*l31 + i.  For fixed (i, q) the NI*4 values over (e, j) are consecutive g-channels: 16-byte stores.
    const int ab = m0 + wm * 32 * MI + MI * l31, gb = n0 + wn * 32 * NI;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = ab + i;
      if (row < ca) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4 * NI];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < NI; ++j) v[e * NI + j] = acc[i][j][4 * q + e];
          const int col = gb + NI * (8 * q + 4 * half);
#pragma unroll
          for (int t = 0; t < NI; ++t)
            if (col + 4 * t < cg) *(float4 *)&dst[(int64_t)row * cg + col + 4 * t] = make_float4(v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// the family's description and entries (ftx_spconv_common.h)
// ---------------------------------------------------------------------------------------
struct SpconvF32 {
  static constexpr const char *pairs_name = "ftx_spconv_pairs_gemm", *scatter_name = "ftx_spconv_pairs_gemm_scatter", *rows_name = "ftx_rows_gemm",
                              *wgrad_name = "ftx_spconv_pairs_wgrad";
  // registers decide (a block is one wave per SIMD, a SIMD has 512 vector registers; LDS never binds first):
  // .vgpr_count 60 / 96-104 / 128-136 / 156 / 184-236 / 316
  static constexpr int wgrad_blocks[4][4] = {{8, 4, 3, 3}, {5, 3, 2, 2}, {4, 2, 1, 2}, {3, 2, 2, 2}};
  static constexpr int wgrad_step = 2 * WG_BR;
  using gemm_lds_t = float;
  static constexpr int gemm_stride = 36;   // floats per LDS row: a lane's four-MFMA fragment is ONE ds_read_b128, conflict-free
  static constexpr bool gemm_frag_ptrs_first = false;
  template <int NT>
  static void gemm(dim3 grid, hipStream_t st, const PairsGemmArgs &a) {
    pairs_gemm_kernel<SpconvF32, NT><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.gather, a.W, a.w_transposed, a.koff, a.ca, a.co, a.kvol, a.out, a.bias,
                                                           a.n_dense, a.scatter, a.rows_out);
  }
  template <int MI, int NI, int WMG, int WNG>
  static void wgrad(dim3 grid, hipStream_t st, const PairsWgradArgs &a) {
    pairs_wgrad_kernel<MI, NI, WMG, WNG><<<grid, 256, 0, st>>>(a.A, a.rows_a, a.idx_a, a.G, a.rows_g, a.idx_g, a.koff, a.ca, a.cg, a.kvol, a.tile_len,
                                                               a.part, a.dW, a.n_dense);
  }
};

extern "C" int32_t ftx_spconv_gemm_block_cols(int32_t co, int64_t n_pairs, int32_t kvol) { return spconv_gemm_block_cols(co, n_pairs, kvol); }

extern "C" int ftx_spconv_pairs_gemm(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed,
                                     const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream) {
  return spconv_pairs_entry<SpconvF32>(false, A, rows_a, gather, nullptr, W, w_transposed, koff, n_pairs, ca, co, kvol, tmp, 0, stream);
}

extern "C" int ftx_spconv_pairs_gemm_scatter(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W,
                                             int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol,
                                             float *out, int64_t rows_out, void *stream) {
  return spconv_pairs_entry<SpconvF32>(true, A, rows_a, gather, scatter, W, w_transposed, koff, n_pairs, ca, co, kvol, out, rows_out, stream);
}

extern "C" int ftx_rows_gemm(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co,
                             float *out, void *stream) {
  return spconv_rows_entry<SpconvF32>(A, n, W, w_transposed, bias, ca, co, out, stream);
}

extern "C" int32_t ftx_spconv_wgrad_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng) {
  return spconv_wgrad_table_blocks<SpconvF32>(mi, wmg, ni, wng);
}
extern "C" int32_t ftx_spconv_wgrad_resident_blocks(int32_t ca, int32_t cg) { return spconv_wgrad_occ<SpconvF32>(spconv_wgrad_config(ca, cg)); }

extern "C" size_t ftx_spconv_pairs_wgrad_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol) {
  return spconv_wgrad_workspace_bytes<SpconvF32>(n_pairs, ca, cg, kvol);
}

extern "C" int ftx_spconv_pairs_wgrad(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g,
                                      const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  return spconv_wgrad_entry<SpconvF32>(A, rows_a, idx_a, G, rows_g, idx_g, koff, n_pairs, ca, cg, kvol, dW, workspace, workspace_bytes, stream);
}
