// What the two sparse-convolution families share (ftx_spconv.hip: exact fp32 MFMA; ftx_spconv_bf16.hip: bf16 operands): the tile scan,
// the whole pair-GEMM kernel (one body, the family's few lines in place under `if constexpr`), the index staging and wave-group reduce of
// the weight gradient, its ordered second pass, and the host layer behind the extern "C" entries.  The weight-gradient kernels stay two:
// their staging differs by design (fp32: row-major rows, interleaved sub-tiles, two register stages; bf16: transposed k-contiguous
// images, one stage), and one body would be two kernels under one name.  A family brings exactly: its weight-gradient kernel, and a
// description (SpconvF32, SpconvBf16) with the entry names that front its messages, the pair GEMM's LDS element type, row stride and
// fragment-pointer placement, the weight gradient's occupancy table and tile-length step, and two launch hooks.  The third family
// (ftx_spconv_split.hip, SpconvSplit: three bf16 pieces per operand, fp32-class results) takes everything here but the pair-GEMM body:
// its `gemm` hook launches a kernel of its own, so it brings no GEMM LDS type, stride or pointer placement.  Nothing here is
// selected by process-wide mutable state or by a device query: tile shapes, workspace sizes and summation trees are functions of the
// arguments alone.
#pragma once
#include "ftx_common.h"
#include "ftx_mfma.h"

namespace ftx {

constexpr int kPairTile = 128;      // pairs per GEMM tile: 4 waves x 32 pairs
constexpr int kPairBK = 32;         // channels of the GEMM's reduction staged per step
constexpr int kPairAPasses = 4;     // kPairTile * kPairBK / 4 float4 of gathered rows per thread and step
constexpr int kWgradRound = 1024;   // pair indices a weight-gradient block keeps in LDS at a time
constexpr int kWgradCUs = 256;      // MI355X; a constant of the tiling, not a device query (see spconv_wgrad_occ)

// ---------------------------------------------------------------------------------------
// device: block -> tile
// ---------------------------------------------------------------------------------------
// Tile = `tile` consecutive pairs of ONE offset.  Offsets differ a lot in pair count (the centre offset of a submanifold map has one
// pair per voxel, ~7x the others), so tiles are cut from the pair list, not per offset: wave 0 scans the per-offset tile counts and
// maps the block of an upper-bound grid to s_tile = {offset, first pair, pair count}, or with RANGE (the weight gradient's form, which
// walks [first, end) and treats the only tile of an offset specially) {offset, first pair, end pair, tiles of the offset}; offset -1
// marks a surplus block.  koff == nullptr is one "offset" of n_dense rows.  (The end pair is stored, not left to the caller to add:
// added after the LDS read it cost the 32 x 32 weight-gradient kernels 10-14 VGPRs and an occupancy step.)
template <bool RANGE>
__device__ __forceinline__ void pair_tile_scan(const int32_t *__restrict__ koff, int kvol, int tile, int n_dense, int *s_tile) {
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid >= 64) return;
  int c = 0;
  if (tid < kvol) c = koff ? koff[tid + 1] - koff[tid] : n_dense;
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
    int first = (koff ? koff[tid] : 0) + t * tile;
    s_tile[0] = tid;
    s_tile[1] = first;
    s_tile[2] = (RANGE ? first : 0) + (left > tile ? tile : left);
    if (RANGE) s_tile[3] = nt;
  }
  if (m == 0ull && tid == 0) s_tile[0] = -1;
}

// The GEMM's tiles of kPairTile pairs; `dense` (no gather list) is rows [0, n_dense) in order, which may pass 2^31.
__device__ __forceinline__ void gemm_tile_scan(const int32_t *__restrict__ koff, int kvol, int64_t n_dense, bool dense, int *s_tile) {
  if (!dense) {
    __builtin_assume(koff != nullptr);   // the entries require it with a gather list; keeps the scan's dense form out of the GEMM
    return pair_tile_scan<false>(koff, kvol, kPairTile, 0, s_tile);
  }
  if (threadIdx.x == 0) {
    int64_t left = n_dense - (int64_t)blockIdx.x * kPairTile;
    s_tile[0] = left > 0 ? 0 : -1;
    s_tile[1] = blockIdx.x * kPairTile;
    s_tile[2] = left > kPairTile ? kPairTile : (int)left;
  }
}

// ---------------------------------------------------------------------------------------
// device: the gathered rows of the pair GEMM.  Thread tid holds float4 (row p * 32 + (tid >> 3), channels (tid & 7) * 4) of the A
// chunk; the chunk loader that uses these rows is a lambda of the kernel (see there).
//
// Gathers are unconditional loads from addresses that are always valid: rows past the end of the tile (and malformed indices) read
// row 0 -- what they produce lands in accumulator columns the epilogue never stores (or zeroes) -- and a column tile that sticks out
// of W re-reads W's last float4.  Only a reduction dimension that is not a multiple of kPairBK (the 4-channel stem) needs zero fill,
// on a uniform slow path.  (A branch per load kept every load behind its own compare.)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_gather_rows(const int32_t *__restrict__ gather, int p0, int cnt, int64_t rows_a, int32_t (&src)[kPairAPasses]) {
  const int arow = threadIdx.x >> 3;
#pragma unroll
  for (int p = 0; p < kPairAPasses; ++p) {
    int r = p * 32 + arow;
    int32_t s = 0;
    if (r < cnt) s = gather ? gather[p0 + r] : p0 + r;
    if (s < 0 || s >= rows_a) s = 0;
    src[p] = s;
  }
}

// ---------------------------------------------------------------------------------------
// device: the epilogue of the pair GEMM.  W is the MFMA's row operand, so lane (pair l31, half) of wave w holds row w * 32 + l31 of
// the tile, 4 consecutive output channels in every 4 consecutive accumulator registers: 16-byte stores, each pair row receives 32
// contiguous bytes per instruction (dword stores of the (pair, channel) orientation took 17k cycles per tile here, these take 6k).
// The row goes to row p of `out`, or to row scatter[p] (< rows_out) where there is a scatter list.
// ---------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void pair_gemm_epilogue(const f32x16 (&acc)[NT], int p0, int cnt, int n0, const int32_t *__restrict__ gather, int64_t rows_a,
                                          const int32_t *__restrict__ scatter, int64_t rows_out, const float *__restrict__ bias, int co,
                                          float *__restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const bool nfull = n0 + 32 * NT <= co;
  const int row = wave * 32 + l31;
  int64_t drow = row < cnt ? p0 + row : -1;
  bool zero = false;   // a pair whose source index is out of range contributes a zero row, as if it gathered zeros
  if (gather != nullptr && drow >= 0) {
    const int32_t sidx = gather[drow];
    zero = sidx < 0 || sidx >= rows_a;
  }
  if (scatter != nullptr && drow >= 0) {
    drow = scatter[drow];
    if (drow >= rows_out) drow = -1;
  }
  if (drow < 0) return;
  float *dst = out + drow * co;
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

}  // namespace ftx

// ---------------------------------------------------------------------------------------
// device: the pair GEMM of both families.  tmp[p,:] = A[gather[p],:] @ Wk(p) over tiles of kPairTile pairs of one offset; the fp32
// family multiplies the stored values on v_mfma_f32_32x32x2_f32, the bf16 family rounds both operands to bf16 on their way into LDS
// and multiplies on v_mfma_f32_32x32x16_bf16.  The lines that differ sit in place under `if constexpr`.  F brings
//   F::gemm_lds_t           element type of the two LDS images (float / __bf16)
//   F::gemm_stride          elements per LDS row of kPairBK channels
//   F::gemm_frag_ptrs_first whether a lane's fragment pointers are formed before the first chunk load or inside the chunk loop: the
//                           same values either way, but the placement decides how the compiler orders the stream, and each family
//                           keeps the one its kernel was measured with (profiles/spconv_one_gemm_body.txt)
// NT = 32-column tiles per wave; a wave owns one 32-pair row tile of the block's kPairTile pairs.  W is the MFMA's row operand (rows =
// output channels, columns = pairs) in both families.
// Measured on MI355X (profiles/r01_spconv_layer_micro.txt workload): 256-pair tiles (RT = 2 row tiles per wave) are 5-30 % SLOWER than
// 128-pair tiles on every layer -- the extra accumulators cut occupancy to 1-2 waves per SIMD and the kernel is latency-, not
// W-traffic-bound: RT = 1 everywhere, so the kernel has no such parameter.
// ---------------------------------------------------------------------------------------
template <class F, int NT>
__global__ __launch_bounds__(256) void pairs_gemm_kernel(const float *__restrict__ A, int64_t rows_a, const int32_t *__restrict__ gather,
                                                         const float *__restrict__ W, int w_transposed, const int32_t *__restrict__ koff,
                                                         int ca, int co, int kvol, float *__restrict__ tmp, const float *__restrict__ bias,
                                                         int64_t n_dense, const int32_t *__restrict__ scatter, int64_t rows_out) {
  using namespace ftx;
  // gather == nullptr: dense mode, tmp[r,:] = A[r,:] @ W (+ bias) for r < n_dense (kvol = 1)
  // scatter != nullptr: the result row of pair p goes to row scatter[p] of `tmp` (rows_out rows) instead of row p: for maps in
  // which every destination row receives exactly ONE pair the convolution is this one launch, with no tmp and no reduce pass
  using T = typename F::gemm_lds_t;
  constexpr bool BF16 = std::is_same<T, __bf16>::value;
  constexpr int BN = 32 * NT;
  constexpr int STRIDE = F::gemm_stride;       // both images: the W chunk is kept as Bs[n][k], the reduction index is contiguous for BOTH operands
  constexpr int FRAG = 16 / sizeof(T);         // elements of one ds_read_b128
  constexpr int A_PASSES = kPairAPasses;
  constexpr int B_PASSES = NT;                 // kPairBK * BN / 4 float4 per W chunk = NT * 256

  __shared__ __attribute__((aligned(16))) T As[kPairTile * STRIDE];   // [pair][k]
  __shared__ __attribute__((aligned(16))) T Bs[BN * STRIDE];          // [n][k]
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

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;

  float4 ra[A_PASSES], rb[B_PASSES];
  // The chunk loader is a lambda of the kernel and must stay one: as a function of this header the compiler ordered its instructions
  // differently and the 32 -> 32 layers ran 4-5 % slower (profiles/spconv_shared_host.txt, section 1).
  // pairs_gemm_split_kernel (ftx_spconv_split.hip) holds a copy of it for the same reason: the clamping and zero-fill rules below are
  // what keeps every load inside its operand, so the two copies change together.
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
  // registers -> LDS images; in the bf16 family the ONE place the operands are rounded
  auto store_chunk = [&]() {
#pragma unroll
    for (int p = 0; p < A_PASSES; ++p) {
      if constexpr (BF16) *(bf16x4 *)&As[(p * 32 + arow) * STRIDE + acol] = round4(ra[p]);
      else *(float4 *)&As[(p * 32 + arow) * STRIDE + acol] = ra[p];
    }
#pragma unroll
    for (int q = 0; q < B_PASSES; ++q) {
      if (!w_transposed) {  // transposing store; fp32: (n4i * 144 + kl) mod 64 banks: 2-way conflicts at worst
        int kk = ((tid >> 6) << 3) + (tid & 7), n4 = (q * 8 + ((tid >> 3) & 7)) * 4;
        if constexpr (BF16) {
          const bf16x4 v = round4(rb[q]);
          Bs[(n4 + 0) * STRIDE + kk] = v[0];
          Bs[(n4 + 1) * STRIDE + kk] = v[1];
          Bs[(n4 + 2) * STRIDE + kk] = v[2];
          Bs[(n4 + 3) * STRIDE + kk] = v[3];
        } else {
          Bs[(n4 + 0) * STRIDE + kk] = rb[q].x;
          Bs[(n4 + 1) * STRIDE + kk] = rb[q].y;
          Bs[(n4 + 2) * STRIDE + kk] = rb[q].z;
          Bs[(n4 + 3) * STRIDE + kk] = rb[q].w;
        }
      } else {
        int e = q * 256 + tid;
        int nn = e >> 3, k4 = (e & 7) * 4;
        if constexpr (BF16) *(bf16x4 *)&Bs[nn * STRIDE + k4] = round4(rb[q]);
        else *(float4 *)&Bs[nn * STRIDE + k4] = rb[q];
      }
    }
  };

  // a lane's fragment rows: pair row wave * 32 + l31 of As, W row l31 of every 32-column tile of Bs, from its half's FRAG elements on
  const T *ap = nullptr, *bp = nullptr;
  if constexpr (F::gemm_frag_ptrs_first) {
    ap = &As[(wave * 32 + l31) * STRIDE + FRAG * half];
    bp = &Bs[l31 * STRIDE + FRAG * half];
  }
  load_chunk(0);
  for (int c0 = 0; c0 < ca; c0 += kPairBK) {
    store_chunk();
    __syncthreads();
    if (c0 + kPairBK < ca) load_chunk(c0 + kPairBK);  // next chunk's global loads fly under the MFMAs
    if constexpr (!F::gemm_frag_ptrs_first) {
      ap = &As[(wave * 32 + l31) * STRIDE + FRAG * half];
      bp = &Bs[l31 * STRIDE + FRAG * half];
    }
    if constexpr (BF16) {   // a chunk of kPairBK channels is two k-steps of 16: one ds_read_b128 per operand and k-step
#pragma unroll
      for (int s = 0; s < kPairBK / 16; ++s) {
        const bf16x8 a = *(const bf16x8 *)(ap + 16 * s);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = mfma_bf16(*(const bf16x8 *)(bp + j * 32 * STRIDE + 16 * s), a, acc[j]);
      }
    } else {
      // lane (l31, half) owns k = 8t + 4*half + s of both operands: one ds_read_b128 per operand row feeds 4 MFMAs.
      // The fragments of step t+1 are in flight while the MFMAs of step t issue.
      float af[2][4], bf[2][NT][4];
      auto load_frag = [&](int buf, int t) {
        float4 a = *(const float4 *)(ap + 8 * t);
        af[buf][0] = a.x; af[buf][1] = a.y; af[buf][2] = a.z; af[buf][3] = a.w;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          float4 b = *(const float4 *)(bp + j * 32 * STRIDE + 8 * t);
          bf[buf][j][0] = b.x; bf[buf][j][1] = b.y; bf[buf][j][2] = b.z; bf[buf][j][3] = b.w;
        }
      };
      load_frag(0, 0);
#pragma unroll
      for (int t = 0; t < kPairBK / 8; ++t) {
        if (t + 1 < kPairBK / 8) load_frag((t + 1) & 1, t + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[t & 1][j][s], af[t & 1][s], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  pair_gemm_epilogue<NT>(acc, p0, cnt, n0, gather, rows_a, scatter, rows_out, bias, co, tmp);
}

namespace ftx {

// ---------------------------------------------------------------------------------------
// device: weight gradient
// ---------------------------------------------------------------------------------------
// One round of a tile: the indices of pairs [rbase, rend), rend - rbase <= ROUND, into LDS (idx_a == nullptr: pair p joins row p
// of A and G).  Every slot gets a loadable row: slots past the end repeat row 0, malformed pairs are flagged in s_ok and s_bad and
// zeroed at store time.  ROUND is kWgradRound unless a family's LDS budget asks for less (ftx_spconv_split.hip).
template <int ROUND = kWgradRound>
__device__ __forceinline__ void wgrad_stage_indices(const int32_t *__restrict__ idx_a, int64_t rows_a, const int32_t *__restrict__ idx_g, int64_t rows_g,
                                           int rbase, int rend, int32_t *s_ia, int32_t *s_ig, uint8_t *s_ok, int *s_bad) {
  __syncthreads();  // previous round's gathers are done with s_ia / s_ig
  if (threadIdx.x == 0) *s_bad = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < ROUND; t += 256) {
    int32_t ia = 0, ig = 0;
    uint8_t ok = 0;
    if (t < rend - rbase) {
      ia = idx_a ? idx_a[rbase + t] : rbase + t;
      ig = idx_g ? idx_g[rbase + t] : rbase + t;
      ok = 1;
      if (ia < 0 || ia >= rows_a || ig < 0 || ig >= rows_g) {
        ia = ig = 0;
        ok = 0;
        *s_bad = 1;
      }
    }
    s_ia[t] = ia;
    s_ig[t] = ig;
    s_ok[t] = ok;
  }
  __syncthreads();
}

// Sums the accumulators of the KS wave groups (group ks, wave wq of its group) into group 0 through `red` (the staging buffers, free
// by now), in group order: a fixed summation tree.
template <int MI, int NI, int KS>
__device__ __forceinline__ void wgrad_ks_reduce(f32x16 (&acc)[MI][NI], float *red, int wq, int ks, int lane) {
  for (int r = 1; r < KS; ++r) {
    if (ks == r) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const f32x16 v = acc[i][j];
#pragma unroll
          for (int g = 0; g < 16; ++g) red[(((wq * MI + i) * NI + j) * 16 + g) * 64 + lane] = v[g];
        }
    }
    __syncthreads();
    if (ks == 0) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          f32x16 v = acc[i][j];
#pragma unroll
          for (int g = 0; g < 16; ++g) v[g] += red[(((wq * MI + i) * NI + j) * 16 + g) * 64 + lane];
          acc[i][j] = v;
        }
    }
    __syncthreads();
  }
}

}  // namespace ftx

// Ordered second pass of the weight gradient: both families leave one (ca x cg) partial per tile of `tile_len` pairs in `part`, tiles
// numbered in offset order.  dW[k] = sum of the partial tiles of offset k; an offset with ONE tile was written by the main kernel
// itself.  Block = (256/TL) float4 columns x TL tile lanes; lane l sums tiles l, l+TL, ... and the TL lane sums are added in lane
// order through LDS: a fixed summation tree, bit-reproducible.
template <int TL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, const int32_t *__restrict__ koff, int kvol,
                                                           int tile_len, int n_dense, int64_t mat, float *__restrict__ dW) {
  constexpr int COLS = 256 / TL;
  __shared__ float4 sh[TL][COLS];
  const int k = blockIdx.y;
  int first = 0, cnt = 0;
  for (int q = 0; q <= k; ++q) {
    int c = koff ? koff[q + 1] - koff[q] : n_dense;
    int nt = (c + tile_len - 1) / tile_len;
    if (q < k) first += nt; else cnt = nt;
  }
  if (cnt == 1) return;   // written directly by the main kernel (block-uniform exit)
  const int col = threadIdx.x % COLS, tl = threadIdx.x / COLS;
  const int64_t chunks = ftx::ceil_div(mat / 4, COLS);
  // a block walks several column chunks: thousands of 4-KB blocks are bound by workgroup dispatch, not by bytes
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t e = (chunk * COLS + col) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < mat) {
      const float *src = part + (int64_t)first * mat + e;
      int t = tl;
      for (; t + 3 * TL < cnt; t += 4 * TL) {   // four independent loads in flight, added in tile order
        float4 v0 = *(const float4 *)&src[(int64_t)t * mat], v1 = *(const float4 *)&src[(int64_t)(t + TL) * mat];
        float4 v2 = *(const float4 *)&src[(int64_t)(t + 2 * TL) * mat], v3 = *(const float4 *)&src[(int64_t)(t + 3 * TL) * mat];
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
        s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
        s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
        s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
      }
      for (; t < cnt; t += TL) {
        float4 v = *(const float4 *)&src[(int64_t)t * mat];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
    }
    if (TL > 1) {
      sh[tl][col] = s;
      __syncthreads();
      if (tl == 0) {
#pragma unroll
        for (int l = 1; l < TL; ++l) {
          float4 v = sh[l][col];
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
      }
      __syncthreads();
    }
    if (tl == 0 && e < mat) *(float4 *)&dW[(int64_t)k * mat + e] = s;
  }
}

namespace ftx {

// Launches wgrad_reduce_kernel over the `tiles` partials (upper bound of the tile count) of a kvol-offset weight gradient.
inline void launch_wgrad_reduce(const float *part, const int32_t *koff, int kvol, int tile_len, int n_dense, int64_t mat, int64_t tiles, float *dW,
                                hipStream_t st) {
  // the centre offset of a submanifold map holds ~6x the average pair count: size the tile lanes for it, not for the average
  const int64_t big_tiles = kvol > 1 ? 6 * tiles / kvol : tiles;
  const int64_t want_blocks = ceil_div(1024, kvol);   // ~4 blocks per CU over all offsets
  auto rgrid = [&](int cols) { int64_t c = ceil_div(mat / 4, cols); return dim3((unsigned)(c < want_blocks ? c : want_blocks), (unsigned)kvol); };
  if (big_tiles <= 4)
    wgrad_reduce_kernel<1><<<rgrid(256), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
  else if (big_tiles <= 32)
    wgrad_reduce_kernel<4><<<rgrid(64), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
  else
    wgrad_reduce_kernel<16><<<rgrid(16), 256, 0, st>>>(part, koff, kvol, tile_len, n_dense, mat, dW);
}

// ---------------------------------------------------------------------------------------
// host: the pair GEMM's entries, generic over a family F:
//   F::pairs_name, F::scatter_name, F::rows_name, F::wgrad_name   the entries' names, as they front every message
//   F::gemm_lds_t, F::gemm_stride, F::gemm_frag_ptrs_first       what pairs_gemm_kernel<F, NT> takes from the family (see there)
//   F::gemm<NT>(grid, st, args)                 launches pairs_gemm_kernel<F, NT>: NT 32-column tiles per block
//   F::wgrad<MI, NI, WMG, WNG>(grid, st, args)  launches the weight-gradient kernel of that tile shape
//   F::wgrad_blocks, F::wgrad_step              the weight gradient's occupancy table and tile-length step (below)
// ---------------------------------------------------------------------------------------
struct PairsGemmArgs {
  const float *A;
  int64_t rows_a;
  const int32_t *gather;
  const float *W;
  int w_transposed;
  const int32_t *koff;
  int ca, co, kvol;
  float *out;
  const float *bias;
  int64_t n_dense;
  const int32_t *scatter;
  int64_t rows_out;
};

// 32-column tiles per block as a function of the arguments: 128 columns per block where there are enough pair tiles to fill the chip,
// 64 where there are not (the two deepest levels: 159-445 tiles -- 372 blocks of 128 columns took 42.0 us on the 256 -> 256 layer of
// level 16, 744 blocks of 64 take 34.5; with 472 blocks and more the wider tile wins by 2-5 %, it reads every gathered row once).
// A column split changes no sum: the results are the same bits either way.
inline int spconv_gemm_nt(int co, int64_t row_tiles) {
  int nt = co >= 128 ? 4 : (co + 31) / 32;
  if (co > 128 && co % 96 == 0 && co % 128 != 0) nt = 3;
  if (nt == 4 && row_tiles * ceil_div(co, 128) <= 400) nt = 2;
  return nt;
}

// Column-block width (32 * nt) that the launches below pick, for tests that must know which tile shape they reach:
// kvol >= 1 is a pair list of n_pairs pairs (the pairs and scatter entries), kvol == 0 dense rows (the rows entry, n_pairs rows).
inline int32_t spconv_gemm_block_cols(int32_t co, int64_t n_pairs, int32_t kvol) {
  if (co < 4 || co % 4 != 0 || n_pairs < 0 || kvol < 0) return -1;
  return 32 * spconv_gemm_nt(co, ceil_div(n_pairs, kPairTile) + kvol);
}

// row_tiles blocks of kPairTile rows x the column blocks of spconv_gemm_nt
template <class F>
void spconv_launch_gemm(int64_t row_tiles, hipStream_t st, const PairsGemmArgs &a) {
  const int nt = spconv_gemm_nt(a.co, row_tiles);
  const dim3 grid((unsigned)row_tiles, (unsigned)ceil_div(a.co, 32 * nt));
  switch (nt) {
    case 1: F::template gemm<1>(grid, st, a); break;
    case 2: F::template gemm<2>(grid, st, a); break;
    case 3: F::template gemm<3>(grid, st, a); break;
    default: F::template gemm<4>(grid, st, a); break;
  }
}

// tmp[p,:] = A[gather[p],:] @ Wk(p), or with a scatter list the one-launch convolution out[scatter[p],:] = A[gather[p],:] @ Wk(p) for
// maps whose destination side is a bijection of the pair list.  The strided 2^3 convolution joins every fine voxel to exactly one
// (coarse voxel, offset), so its data gradient and the transposed convolution built on the same map (models/spvcnn.py:38-50) write
// every fine row exactly once: no tmp, no reduce.  The caller guarantees that `scatter` is injective (rows it does not name are left
// untouched).
template <class F>
int spconv_pairs_entry(bool scattered, const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W,
                       int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *out, int64_t rows_out,
                       void *stream) {
  // `scattered` says which entry this is: it picks the name and makes the scatter list mandatory; the pairs entry passes
  // scatter = nullptr and rows_out = 0, so the rows_out check below cannot fire for it
  const char *me = scattered ? F::scatter_name : F::pairs_name;
  FTX_REQUIRE(n_pairs >= 0 && rows_a >= 0 && rows_out >= 0 && kvol >= 1 && kvol <= 64, "%s: bad size", me);
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && co >= 4 && co % 4 == 0, "%s: channels must be multiples of 4 (ca=%d co=%d)", me, ca, co);
  if (n_pairs == 0) return FTX_OK;
  FTX_REQUIRE(A && gather && (scatter || !scattered) && W && koff && out && rows_a >= 1, "%s: null pointer or empty operand", me);
  const PairsGemmArgs a = {A, rows_a, gather, W, w_transposed, koff, ca, co, kvol, out, nullptr, 0, scatter, rows_out};
  spconv_launch_gemm<F>(ceil_div(n_pairs, kPairTile) + kvol, (hipStream_t)stream, a);   // sum_k ceil(cnt_k/tile) <= P/tile + kvol
  return check_launch(me);
}

// Dense rows: out[r,:] = A[r,:] @ W (+ bias) on the same tile code (identity gather, one "offset").
// The point-branch Linear layers, the 1x1x1 convolutions and the heads are skinny GEMMs
// (81k rows x 20..256 columns, K = 32..256) that are HBM-bound: rows in, rows out, W from L2.
template <class F>
int spconv_rows_entry(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co, float *out,
                      void *stream) {
  const char *me = F::rows_name;
  FTX_REQUIRE(n >= 0, "%s: n < 0", me);
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && co >= 4 && co % 4 == 0, "%s: channels must be multiples of 4 (ca=%d co=%d)", me, ca, co);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(A && W && out, "%s: null pointer", me);
  const PairsGemmArgs a = {A, n, nullptr, W, w_transposed, nullptr, ca, co, 1, out, bias, n, nullptr, 0};
  spconv_launch_gemm<F>(ceil_div(n, kPairTile), (hipStream_t)stream, a);
  return check_launch(me);
}

// ---------------------------------------------------------------------------------------
// host: the weight gradient's rules and entry
// ---------------------------------------------------------------------------------------
struct PairsWgradArgs {
  const float *A;
  int64_t rows_a;
  const int32_t *idx_a;
  const float *G;
  int64_t rows_g;
  const int32_t *idx_g, *koff;
  int ca, cg, kvol, tile_len;
  float *part, *dW;
  int n_dense;
};

// Tile shape per channel count.  M side: 32 / 64 / 96 (multiples of 96 that are not multiples of 128: 96, 192) / 128;
// N side: 32 / 64 / 96 / 128.
struct WgradCfg { int mi, wmg, ni, wng; };
inline WgradCfg spconv_wgrad_config(int ca, int cg) {
  WgradCfg c;
  if (ca <= 32) { c.mi = 1; c.wmg = 1; }
  else if (ca <= 64) { c.mi = 2; c.wmg = 1; }
  else if (ca % 96 == 0 && ca % 128 != 0) { c.mi = 3; c.wmg = 1; }
  else { c.mi = 2; c.wmg = 2; }
  if (cg <= 32) { c.ni = 1; c.wng = 1; }
  else if (cg <= 64) { c.ni = 2; c.wng = 1; }
  else if (cg % 96 == 0 && cg % 128 != 0) { c.ni = 3; c.wng = 1; }
  else { c.ni = 2; c.wng = 2; }
  // a 96 x 96 tile per wave is 9 accumulators (144 registers): one wave per SIMD.  96 -> 96 layers take a 128 x 96 tile instead
  // (2 x 3 accumulators per wave, the last 32 M rows are padding).
  if (c.mi == 3 && c.ni == 3) { c.mi = 2; c.wmg = 2; }
  return c;
}

// Resident blocks per CU of the instantiation a layer uses, as the family's TABLE F::wgrad_blocks -- rows: M side (mi, wmg) = (1,1)
// (2,1) (3,1) (2,2); columns: N side (ni, wng) in the same order.  Values = min(8, 512 / VGPRs rounded up to 8, 160 KiB / LDS) read
// from the gfx950 code object (llvm-readelf --notes); tests/test_cabi.py and tests/test_spconv_bf16_host.py recompute them from the
// built object and fail when a table is stale.  A table and not hipOccupancyMaxActiveBlocksPerMultiprocessor: the tile length, the
// workspace size and the summation tree of the weight gradient (hence its bits) must be functions of the arguments alone, the same on
// every host and device (round 2 asked the runtime, with a fallback of 2 where there was no device to ask).
template <class F>
int spconv_wgrad_occ(const WgradCfg &c) {
  auto side = [](int i, int w) { return w == 2 ? 3 : i - 1; };
  return F::wgrad_blocks[side(c.mi, c.wmg)][side(c.ni, c.wng)];
}
// (mi, wmg, ni, wng) -> table value, for the build-time check of the table against the code object
template <class F>
int32_t spconv_wgrad_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng) {
  if (!((mi >= 1 && mi <= 3 && wmg == 1) || (mi == 2 && wmg == 2)) || !((ni >= 1 && ni <= 3 && wng == 1) || (ni == 2 && wng == 2))) return -1;
  return spconv_wgrad_occ<F>(WgradCfg{mi, wmg, ni, wng});
}

// Pairs per tile.  All blocks of a launch should be resident together: a launch of 1.2x the resident slots takes as long as one of 2x
// (measured: 620 blocks on 512 slots ran 1.7x longer than 820).  So the tile length is chosen for R full rounds of
// slots = CUs x resident blocks per CU, R as small as keeps a tile <= 4096 pairs; every offset adds about half a tile of rounding.
// F::wgrad_step (two staged steps of the family's kernel) is what a tile length is a multiple of.
template <class F>
int spconv_wgrad_tile_len(int64_t n_pairs, int ca, int cg, int kvol) {
  const WgradCfg c = spconv_wgrad_config(ca, cg);
  const int64_t mn_tiles = ceil_div(ca, 32 * c.mi * c.wmg) * ceil_div(cg, 32 * c.ni * c.wng);
  const int64_t slots = (int64_t)kWgradCUs * spconv_wgrad_occ<F>(c);
  int64_t len = 256;
  for (int rounds = 1; rounds <= 64; ++rounds) {
    int64_t tiles = (slots * rounds * 15 / 16) / mn_tiles - (kvol + 1) / 2;   // 1/16 of head room: an overshoot costs a whole round
    if (tiles < 1) tiles = 1;
    len = ceil_div(ceil_div(n_pairs, tiles), F::wgrad_step) * F::wgrad_step;
    if (len <= 4096) break;
  }
  if (len < 256) len = 256;
  return (int)len;
}

inline int64_t spconv_wgrad_tiles_ub(int64_t n_pairs, int tile_len, int kvol) { return ceil_div(n_pairs, tile_len) + kvol; }

template <class F>
size_t spconv_wgrad_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol) {
  if (n_pairs <= 0 || ca <= 0 || cg <= 0 || kvol <= 0) return 256;
  const int len = spconv_wgrad_tile_len<F>(n_pairs, ca, cg, kvol);
  return sizeof(float) * (size_t)spconv_wgrad_tiles_ub(n_pairs, len, kvol) * ca * cg;
}

template <class F, int MI, int WMG>
void spconv_launch_wgrad_n(const WgradCfg &c, dim3 grid, hipStream_t st, const PairsWgradArgs &a) {
  if (c.ni == 1) F::template wgrad<MI, 1, WMG, 1>(grid, st, a);
  else if (c.ni == 3) F::template wgrad<MI, 3, WMG, 1>(grid, st, a);
  else if (c.wng == 1) F::template wgrad<MI, 2, WMG, 1>(grid, st, a);
  else F::template wgrad<MI, 2, WMG, 2>(grid, st, a);
}

template <class F>
int spconv_wgrad_entry(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g,
                       const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace,
                       size_t workspace_bytes, void *stream) {
  const char *me = F::wgrad_name;
  FTX_REQUIRE(n_pairs >= 0 && rows_a >= 0 && rows_g >= 0 && kvol >= 1 && kvol <= 64, "%s: bad size", me);
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && cg >= 4 && cg % 4 == 0, "%s: channels must be multiples of 4 (ca=%d cg=%d)", me, ca, cg);
  FTX_REQUIRE(dW, "%s: null dW", me);
  hipStream_t st = (hipStream_t)stream;
  const int64_t mat = (int64_t)ca * cg;
  if (n_pairs == 0) {
    if (hipMemsetAsync(dW, 0, sizeof(float) * kvol * mat, st) != hipSuccess) {
      char what[64];
      snprintf(what, sizeof(what), "%s memset", me);
      return check_launch(what);
    }
    return FTX_OK;
  }
  FTX_REQUIRE(A && G && rows_a >= 1 && rows_g >= 1, "%s: null pointer or empty operand", me);
  const bool dense = (idx_a == nullptr && idx_g == nullptr && koff == nullptr);
  FTX_REQUIRE(dense || (idx_a && idx_g && koff), "%s: idx_a, idx_g and koff must be all set or all null (dense rows)", me);
  FTX_REQUIRE(!dense || (kvol == 1 && n_pairs <= rows_a && n_pairs <= rows_g), "%s: dense mode needs kvol == 1 and n_pairs rows in A and G", me);
  FTX_REQUIRE(n_pairs < 0x7fffffff, "%s: too many pairs", me);
  const int tile_len = spconv_wgrad_tile_len<F>(n_pairs, ca, cg, kvol);
  const int64_t tiles = spconv_wgrad_tiles_ub(n_pairs, tile_len, kvol);
  const size_t need = sizeof(float) * (size_t)tiles * mat;
  if (!workspace || workspace_bytes < need) return workspace_short(me, workspace_bytes, need);
  const PairsWgradArgs a = {A, rows_a, idx_a, G, rows_g, idx_g, koff, ca, cg, kvol, tile_len, (float *)workspace, dW, (int)n_pairs};
  const WgradCfg c = spconv_wgrad_config(ca, cg);
  const dim3 grid((unsigned)tiles, (unsigned)ceil_div(ca, 32 * c.mi * c.wmg), (unsigned)ceil_div(cg, 32 * c.ni * c.wng));
  if (c.mi == 1) spconv_launch_wgrad_n<F, 1, 1>(c, grid, st, a);
  else if (c.mi == 3) spconv_launch_wgrad_n<F, 3, 1>(c, grid, st, a);
  else if (c.wmg == 1) spconv_launch_wgrad_n<F, 2, 1>(c, grid, st, a);
  else spconv_launch_wgrad_n<F, 2, 2>(c, grid, st, a);
  launch_wgrad_reduce(a.part, koff, kvol, tile_len, (int)n_pairs, mat, tiles, dW, st);
  return check_launch(me);
}

}  // namespace ftx
