// ViT self-attention (timm Attention.forward, reached at models/transformers.py:36-37):
//   out = softmax(Q K^T * scale) V     per (batch, head), T tokens (578), head dim 64, fp32 in HBM.
// Flash-style: the T x T score matrix is never written.  Two precisions of the products, one set of kernel bodies:
//   AttnF32   exact-fp32 MFMA (v_mfma_f32_32x32x2_f32)                          ftx_attn_fwd / ftx_attn_bwd [_tiled]
//   AttnBf16  bf16 operands, fp32 accumulation (v_mfma_f32_32x32x16_bf16)       ftx_attn_fwd_bf16 / ftx_attn_bwd_bf16
//   AttnSplit every operand in three bf16 pieces, six piece products, fp32-class ftx_attn_fwd_split / ftx_attn_bwd_split
// A precision is an operand description (below): the lane fragment and its loader, the staging registers with prefetch and store, the
// LDS images of a staged tile, the two products, and where scale * log2(e) enters.  The forward, dK/dV, dQ and delta bodies
// (attn_*_body) are written once over that description and <QW, SPLIT>; the __global__ kernels are wrappers that keep their names, and
// the host entries are one forward and one backward entry over a family description (the entry names and the kernels).
//
// Layout trick (cdna_hip_programming.md "accumulator tile as the next MFMA's operand"): a 32x32
// accumulator has its COLUMN on the lane and 16 ROWS in registers (row(g,h) = (g&3)+8(g>>2)+4h,
// h = lane>>5).  A following MFMA that sums over the tile's ROW index can take it as the B operand
// with no lane movement.  So each product is oriented so that the index summed next is the row:
//   forward   S^T[key][q] = K Q^T      -> softmax state per lane (one q per lane)
//             O^T[dv][q] += V^T P^T    (sums over keys = rows of P^T)
//   dK/dV     S[q][key]   = Q K^T,  dP[q][key] = dO V^T
//             dV^T[dv][key] += dO^T P, dK^T[d][key] += Q^T dS      (sum over q = rows)
//   dQ        S^T, dP^T as in the forward orientation;  dQ^T[d][q] += K^T dS^T  (sum over keys)
// The reduction index of the first products is permuted (fp32: lane half h takes d = 8t+4h+s) so operand
// fragments are one ds_read_b128 / one 16-byte global load per 4 MFMAs.
#include "ftx_common.h"
#include "ftx_mfma.h"
#include "ftx_split.h"   // split1: the ONE definition of the split

using namespace ftx;

constexpr int HD = 64;          // head dim (fixed)
constexpr int TS = 68;          // LDS row stride in floats (16-byte aligned, conflict-free b128)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ inline int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// 2^x as the bare v_exp_f32: every argument in these kernels is <= 0 up to rounding (a score minus its row maximum / log-sum-exp)
// or -inf (a masked key), so exp2f()'s range fix-ups -- a compare, two selects and an ldexp per call, 5 of the 6 instructions --
// have nothing to fix; results below 2^-126 flush to zero, which is what a softmax weight of that size is worth.
__device__ inline float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }

// qkv (b, t, 3, nh, 64): row of tensor `which` (0 q, 1 k, 2 v) for token t, head hd; tokens are 3 * nh * 64 floats apart
__device__ inline const float *qkv_row(const float *qkv, int b, int t, int which, int hd, int T, int nh) {
  return qkv + ((((int64_t)b * T + t) * 3 + which) * nh + hd) * HD;
}

// ---------------------------------------------------------------------------------------
// Operand descriptions.  What the bodies ask of a precision P:
//   Frag, load_frag        this lane's fragment of a 64-float global row (the B operand of the first products)
//   fold / score / dO      where scale * log2(e) enters, and how the delta kernel reads dO
//   Stage<NT>, prefetch,   registers that hold a 32-token x 64-float tile on its way to LDS: rows t0.. of tensor `which` of qkv
//   prefetch_o             (prefetch) or of a (b, t, nh*64) tensor, out / grad_out (prefetch_o); tokens >= T are zero.  NT = threads
//                          of the staging group (one key / query group of a block), tid in [0, NT).  How a row's address is formed
//                          stays per precision: each form was measured slower in the other's kernels
//   tile_floats, store     the LDS images of a staged tile; <ROW, COL> say which products read it: ROW = a first product (A operand
//                          by token rows), COL = a product on an accumulator tile (A operand by columns)
//   first                  acc[row][col=lane] += sum_d Tile[row][d] * frag[d]
//   X, operand, second     out[r][col=lane] += sum over the 32 rows j of x of Tile[j][col_off + r] * x[j][col]   (x = an accumulator
//                          tile as the B operand, in the form `operand` gives it)
// ---------------------------------------------------------------------------------------
struct AttnF32 {
  using Frag = float[32];
  template <int NT> using Stage = float4[512 / NT];
  using X = f32x16;
  // one image [token][64] with stride TS serves both kinds of product
  static constexpr int tile_floats(bool row, bool col) { return 32 * TS; }

  // Load this lane's permuted 32-float fragment of a 64-float row: elements 8t+4h+s.
  __device__ static void load_frag(const float *row, int h, bool valid, Frag &f) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) v = *(const float4 *)(row + 8 * t + 4 * h);
      f[4 * t + 0] = v.x; f[4 * t + 1] = v.y; f[4 * t + 2] = v.z; f[4 * t + 3] = v.w;
    }
  }
  // scale * log2(e) folded into the Q (K) fragment once: S comes out of the MFMAs in the exp2 domain.  Only S uses that fragment.
  __device__ static void fold(Frag &f, float sl2) {
#pragma unroll
    for (int i = 0; i < 32; ++i) f[i] *= sl2;
  }
  __device__ static float score(float s, float sl2) { return s; }
  __device__ static float dO(float g) { return g; }

  // Each row's address from its token index; the base-and-stride form of AttnBf16 costs the one-wave forward 0.4 us of 20 (batch 1).
  template <int NT>
  __device__ static void prefetch(const float *qkv, int b, int hd, int which, int t0, int T, int nh, int tid, Stage<NT> &r) {
#pragma unroll
    for (int q = 0; q < 512 / NT; ++q) {
      int e = q * NT + tid;
      int row = e >> 4, c4 = (e & 15) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t0 + row < T) v = *(const float4 *)(qkv_row(qkv, b, t0 + row, which, hd, T, nh) + c4);
      r[q] = v;
    }
  }
  template <int NT>
  __device__ static void prefetch_o(const float *o, int b, int hd, int t0, int T, int nh, int tid, Stage<NT> &r) {
#pragma unroll
    for (int q = 0; q < 512 / NT; ++q) {
      int e = q * NT + tid;
      int row = e >> 4, c4 = (e & 15) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t0 + row < T) v = *(const float4 *)(o + (((int64_t)b * T + t0 + row) * nh + hd) * HD + c4);
      r[q] = v;
    }
  }
  template <int NT, bool ROW, bool COL>
  __device__ static void store(float *tile, int tid, const Stage<NT> &r) {
#pragma unroll
    for (int q = 0; q < 512 / NT; ++q) {
      int e = q * NT + tid;
      int row = e >> 4, c4 = (e & 15) * 4;
      *(float4 *)&tile[row * TS + c4] = r[q];
    }
  }
  __device__ static void first(const float *tile, int l31, int h, const Frag &frag, f32x16 &acc) {
    const float *rp = tile + l31 * TS + 4 * h;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float4 a = *(const float4 *)(rp + 8 * t);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, frag[4 * t + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, frag[4 * t + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, frag[4 * t + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, frag[4 * t + 3], acc, 0, 0, 0);
    }
  }
  __device__ static const X &operand(const f32x16 &x) { return x; }
  template <bool ROW>
  __device__ static void second(const float *tile, int col_off, int l31, int h, const X &x, f32x16 &out) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      float a = tile[acc_row(g, h) * TS + col_off + l31];
      out = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[g], out, 0, 0, 0);
    }
  }
};

// =======================================================================================
// bf16-operand attention (ftx_attn_fwd_bf16 / ftx_attn_bwd_bf16): the same three bodies, the same orientation and the same
// (QW, SPLIT) scheme, with every product on v_mfma_f32_32x32x16_bf16 (16x the f32-MFMA rate) and fp32 accumulation.
//
// Precision contract (include/ftx.h states it for callers):
//   storage   qkv, out, lse, grad_out and grad_qkv stay fp32 in HBM.
//   scores    Q, K, V, dO are rounded to bf16 (round-to-nearest-even) from their stored fp32 values; the score comes out of the MFMA in
//             fp32 (a bf16 x bf16 product is exact in fp32) and scale * log2(e) is applied to it in fp32 -- never folded into Q first.
//   softmax   running max, row sum l and lse use the unrounded fp32 exponentials; P is rounded to bf16 only as the P.V operand.
//   backward  P is recomputed from lse; dP = dO V^T on bf16 operands; delta = rowsum(bf16(dO) * O) in fp32 (attn_delta_bf16_kernel); dS is rounded
//             to bf16 only as the operand of the dK and dQ products; every gradient is accumulated and written in fp32.
//   order     no atomics; the key (query) groups merge through the fixed tree of merge_sum: deterministic for a given tiling.
//
// Operand maps of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md section 3): lane (r = lane & 31, h = lane >> 5) holds A[row r][k] and
// B[k][col r] for k = 8h + j, j = 0..7, of each 16-wide k-step.  Two LDS images per staged 32-token tile, both bf16, converted once when
// stored:
//   row image  [token][64]  (stride RS): A operand of the first products (S, dP), k = the head dim: step s, element j <-> d = 16s + 8h + j,
//              one ds_read_b128; the lane's own fragment (the B operand) is loaded in the same order.
//   col image  [64][token]  (stride CS): A operand of the products that take an accumulator tile X as the B operand: registers 8s..8s+7
//              of X, converted pairwise, are k-step s with element j <-> row 16s + 8(j>>2) + 4h + (j&3) of X, so the A element j is read
//              from those tokens: two ds_read_b64.
// =======================================================================================
constexpr int RS = 72;   // row image stride in bf16 (144 B: 16-byte aligned, conflict-free ds_read_b128)
constexpr int CS = 36;   // col image stride in bf16 (72 B: 8-byte aligned, conflict-free ds_read_b64 over 32 lanes)
constexpr int IMG = 32 * RS;   // bf16 per image (32 * RS == 64 * CS)
static_assert(32 * RS == 64 * CS, "row and col images are the same size");

__device__ inline bf16x4 cvt4(float4 v) { return (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w}; }

struct AttnBf16 {
  using Frag = bf16x8[4];
  // Staging of a 32-token x 64-float tile in 4 x 4 micro-blocks (4 tokens x 4 floats, 128 per tile): four float4 loads per micro-block
  // (16 lanes read one 256-byte row segment), stored as 4 rows of the row image and / or 4 columns of the col image, 8 bytes each.
  // With NT = 256 half the threads stage.
  template <int NT> static constexpr int stage_mb() { return (128 + NT - 1) / NT; }
  template <int NT> using Stage = float4[4 * stage_mb<NT>()];
  struct X { bf16x8 s[2]; };
  // the row image, then the col image, of those the tile's products read
  static constexpr int tile_floats(bool row, bool col) { return (row + col) * IMG / 2; }

  // The lane's fragment of a 64-float global row, rounded to bf16: f[s][j] = row[16s + 8h + j].
  __device__ static void load_frag(const float *row, int h, bool valid, Frag &f) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (valid) {
        a = *(const float4 *)(row + 16 * s + 8 * h);
        b = *(const float4 *)(row + 16 * s + 8 * h + 4);
      }
      f[s] = __builtin_shufflevector(cvt4(a), cvt4(b), 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }
  // Q (K) is rounded from its stored value, no scale folded in; the fp32 score goes into the exp2 domain
  __device__ static void fold(Frag &, float) {}
  __device__ static float score(float s, float sl2) { return s * sl2; }
  // dO enters the bf16 backward as its rounded value everywhere, in delta too, so that sum_key dS = P (dP - delta) stays ~0 per query.
  // With the fp32 dO a saturated softmax row (P ~ 1 on one key) would keep dS = (bf16(dO) - dO) . V * scale on that key instead of ~0.
  __device__ static float dO(float g) { return (float)(__bf16)g; }

  // src = token 0 of the tile's tensor, rstride = floats between tokens: an address per row as in AttnF32 costs these kernels 5-15 %
  // (batch 1 forward 10.5 -> 11.1 us, batch 4 19.4 -> 21.0)
  template <int NT>
  __device__ static void prefetch(const float *qkv, int b, int hd, int which, int t0, int T, int nh, int tid, Stage<NT> &r) {
    prefetch_rows<NT>(qkv_row(qkv, b, 0, which, hd, T, nh), 3 * nh * HD, t0, T, tid, r);
  }
  template <int NT>
  __device__ static void prefetch_o(const float *o, int b, int hd, int t0, int T, int nh, int tid, Stage<NT> &r) {
    prefetch_rows<NT>(o + ((int64_t)b * T * nh + hd) * HD, nh * HD, t0, T, tid, r);
  }
  template <int NT>
  __device__ static void prefetch_rows(const float *src, int64_t rstride, int t0, int T, int tid, Stage<NT> &r) {
#pragma unroll
    for (int q = 0; q < stage_mb<NT>(); ++q) {
      const int e = q * NT + tid, tq = (e >> 4) & 7, c4 = (e & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * tq + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((NT <= 128 || e < 128) && t < T) v = *(const float4 *)(src + t * rstride + c4);
        r[4 * q + i] = v;
      }
    }
  }
  template <int NT, bool ROW, bool COL>
  __device__ static void store(float *tile, int tid, const Stage<NT> &r) {
    __bf16 *rowimg = (__bf16 *)tile, *colimg = rowimg + (ROW ? IMG : 0);
#pragma unroll
    for (int q = 0; q < stage_mb<NT>(); ++q) {
      const int e = q * NT + tid, tq = e >> 4, c4 = (e & 15) * 4;
      if (NT > 128 && e >= 128) continue;
      if (ROW) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *(bf16x4 *)(rowimg + (4 * tq + i) * RS + c4) = cvt4(r[4 * q + i]);
      }
      if (COL) {
        *(bf16x4 *)(colimg + (c4 + 0) * CS + 4 * tq) = (bf16x4){(__bf16)r[4 * q].x, (__bf16)r[4 * q + 1].x, (__bf16)r[4 * q + 2].x, (__bf16)r[4 * q + 3].x};
        *(bf16x4 *)(colimg + (c4 + 1) * CS + 4 * tq) = (bf16x4){(__bf16)r[4 * q].y, (__bf16)r[4 * q + 1].y, (__bf16)r[4 * q + 2].y, (__bf16)r[4 * q + 3].y};
        *(bf16x4 *)(colimg + (c4 + 2) * CS + 4 * tq) = (bf16x4){(__bf16)r[4 * q].z, (__bf16)r[4 * q + 1].z, (__bf16)r[4 * q + 2].z, (__bf16)r[4 * q + 3].z};
        *(bf16x4 *)(colimg + (c4 + 3) * CS + 4 * tq) = (bf16x4){(__bf16)r[4 * q].w, (__bf16)r[4 * q + 1].w, (__bf16)r[4 * q + 2].w, (__bf16)r[4 * q + 3].w};
      }
    }
  }
  __device__ static void first(const float *tile, int l31, int h, const Frag &frag, f32x16 &acc) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma_bf16(*(const bf16x8 *)((const __bf16 *)tile + l31 * RS + 16 * s + 8 * h), frag[s], acc);
  }
  // an accumulator tile as a B operand: k-step s = registers 8s..8s+7 (rounded to bf16 here, and only here)
  __device__ static X operand(const f32x16 &x) {
    X r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r.s[0][j] = (__bf16)x[j];
      r.s[1][j] = (__bf16)x[8 + j];
    }
    return r;
  }
  template <bool ROW>
  __device__ static void second(const float *tile, int col_off, int l31, int h, const X &x, f32x16 &out) {
    const __bf16 *colimg = (const __bf16 *)tile + (ROW ? IMG : 0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const __bf16 *p = colimg + (col_off + l31) * CS + 16 * s + 4 * h;
      out = mfma_bf16(__builtin_shufflevector(*(const bf16x4 *)p, *(const bf16x4 *)(p + 8), 0, 1, 2, 3, 4, 5, 6, 7), x.s[s], out);
    }
  }
};

// =======================================================================================
// fp32-accurate attention on the bf16 MFMA (ftx_attn_fwd_split / ftx_attn_bwd_split): the same bodies once more, every product from
// three bf16 pieces per operand (ftx_split.h: x = h + m + l) and the six piece products of tests/split_ref.py.
//
// Precision contract (include/ftx.h states it for callers):
//   storage   qkv, out, lse, grad_out and grad_qkv stay fp32 in HBM.
//   operands  every MFMA operand is split by ftx::split1: Q, K, V, dO from their stored fp32 values (a staged tile when it is stored to
//             LDS, a lane's own fragment when it is loaded), and the accumulator tiles P (forward, dK/dV) and dS (dK/dV, dQ) from their
//             fp32 registers (operand).  Nothing is rounded to one bf16.
//   products  a product is mm, hl, lh, hm, mh, hh (first letter: the staged tile's piece) on v_mfma_f32_32x32x16_bf16, per 16-wide
//             k-step in that order.  Grouping: within one call of first / second the five corrections run in an accumulator of their
//             own that starts at zero, hh runs in the caller's accumulator, and the corrections are added to it once at the end of the
//             call -- once per 32 x 32 x 64 (first) or 32 x 32 x 32 (second) product, i.e. once per staged tile.
//   scale     scale * log2(e) multiplies the fp32 score (as in AttnBf16), it is not folded into an operand.
//   dO        exact: P::dO(g) = g, so attn_delta_split_kernel is the fp32 delta kernel in arithmetic.
//   softmax   running max, row sum, lse, rescale and the P rebuilt from lse are fp32, as in the other families.
//   order     no atomics; merge_sum's fixed tree: deterministic for a given tiling.
//
// LDS: the bf16 family's two images per staged tile (row image, col image: see AttnBf16), three times -- one per piece -- split once
// when the tile is stored, so the QW waves of a block share the split's VALU work as they share the tile (one fp32 image split at
// fragment-read time was built first: every wave then splits every tile it reads, and at (4,2) the kernels only matched the fp32
// family's time).  The images' layout and the fragment order are AttnBf16's; the staging is the family's own (prefetch_rows below).  A
// key group costs 27 KB in the forward, 55 KB in dK/dV and
// 41 KB in dQ, so on a 160 KB CU the forward fits every tiling but (1,8) and the backward those with two groups: built() below.  The
// lane's own fragments are split once, when loaded, and held as pieces in registers (48 VGPRs each).
// =======================================================================================
struct Pieces8 { bf16x8 h, m, l; };
struct Pieces4 { bf16x4 h, m, l; };
__device__ inline void split8(const float (&v)[8], Pieces8 &p) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 h, m, l;
    split1(v[j], h, m, l);
    p.h[j] = h; p.m[j] = m; p.l[j] = l;
  }
}
__device__ inline Pieces4 split4(float a, float b, float c, float d) {
  const float v[4] = {a, b, c, d};
  Pieces4 p;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    __bf16 h, m, l;
    split1(v[j], h, m, l);
    p.h[j] = h; p.m[j] = m; p.l[j] = l;
  }
  return p;
}
// one k-step of a product: the five corrections, smallest first, into `corr`, hh into `main`.  a = the staged tile's pieces
__device__ inline void six_products(const Pieces8 &a, const Pieces8 &b, f32x16 &corr, f32x16 &main) {
  corr = mfma_bf16(a.m, b.m, corr);
  corr = mfma_bf16(a.h, b.l, corr);
  corr = mfma_bf16(a.l, b.h, corr);
  corr = mfma_bf16(a.h, b.m, corr);
  corr = mfma_bf16(a.m, b.h, corr);
  main = mfma_bf16(a.h, b.h, main);
}

struct AttnSplit : AttnBf16 {
  using Frag = Pieces8[4];
  struct X { Pieces8 s[2]; };
  // the row images of h, m, l, then the col images of h, m, l, of those the tile's products read
  static constexpr int tile_floats(bool row, bool col) { return 3 * (row + col) * IMG / 2; }
  // What fits a 160 KB CU (LDS of a block: forward 27 KB x SPLIT, dK/dV 55 KB x SPLIT, dQ 41 KB x SPLIT); the kernels of the other
  // tilings are empty and never launched.
  static constexpr bool built(int qw, int split, bool backward) { return backward ? split == 2 : split <= 4; }

  // The lane's fragment of a 64-float global row, split: f[s] piece [j] = piece of row[16s + 8h + j].
  __device__ static void load_frag(const float *row, int h, bool valid, Frag &f) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (valid) {
        a = *(const float4 *)(row + 16 * s + 8 * h);
        b = *(const float4 *)(row + 16 * s + 8 * h + 4);
      }
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      split8(v, f[s]);
    }
  }
  __device__ static void fold(Frag &, float) {}
  __device__ static float dO(float g) { return g; }

  // Staging in units of TOK tokens x 4 floats, 16 units across a token row: 4 x 4 micro-blocks as AttnBf16 up to 128 threads, 2 x 4 with
  // 256, so that every thread of the group stages -- and splits -- its share (with micro-blocks half of them would do it all) and a
  // lane holds 2 float4 per tile in flight, not 4.
  template <int NT> static constexpr int tok() { return NT > 128 ? 2 : 4; }
  template <int NT> static constexpr int units() { return (32 / tok<NT>()) * 16 / NT; }
  template <int NT> using Stage = float4[tok<NT>() * units<NT>()];
  template <int NT>
  __device__ static void prefetch(const float *qkv, int b, int hd, int which, int t0, int T, int nh, int tid, Stage<NT> &r) {
    prefetch_rows<NT>(qkv_row(qkv, b, 0, which, hd, T, nh), 3 * nh * HD, t0, T, tid, r);
  }
  template <int NT>
  __device__ static void prefetch_o(const float *o, int b, int hd, int t0, int T, int nh, int tid, Stage<NT> &r) {
    prefetch_rows<NT>(o + ((int64_t)b * T * nh + hd) * HD, nh * HD, t0, T, tid, r);
  }
  template <int NT>
  __device__ static void prefetch_rows(const float *src, int64_t rstride, int t0, int T, int tid, Stage<NT> &r) {
    constexpr int TOK = tok<NT>();
#pragma unroll
    for (int q = 0; q < units<NT>(); ++q) {
      const int e = q * NT + tid, tq = e >> 4, c4 = (e & 15) * 4;
#pragma unroll
      for (int i = 0; i < TOK; ++i) {
        const int t = t0 + TOK * tq + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T) v = *(const float4 *)(src + t * rstride + c4);
        r[TOK * q + i] = v;
      }
    }
  }
  // the ONE place a staged tile is split: each unit once, its pieces written to the row and / or col images
  template <int NT, bool ROW, bool COL>
  __device__ static void store(float *tile, int tid, const Stage<NT> &r) {
    constexpr int TOK = tok<NT>();
    __bf16 *rowimg = (__bf16 *)tile, *colimg = rowimg + (ROW ? 3 * IMG : 0);
#pragma unroll
    for (int q = 0; q < units<NT>(); ++q) {
      const int e = q * NT + tid, tq = e >> 4, c4 = (e & 15) * 4;
      Pieces4 p[TOK];   // p[i]: token TOK tq + i, columns c4 .. c4 + 3
#pragma unroll
      for (int i = 0; i < TOK; ++i) p[i] = split4(r[TOK * q + i].x, r[TOK * q + i].y, r[TOK * q + i].z, r[TOK * q + i].w);
      if (ROW) {
#pragma unroll
        for (int i = 0; i < TOK; ++i) {
          __bf16 *d = rowimg + (TOK * tq + i) * RS + c4;
          *(bf16x4 *)d = p[i].h;
          *(bf16x4 *)(d + IMG) = p[i].m;
          *(bf16x4 *)(d + 2 * IMG) = p[i].l;
        }
      }
      if (COL) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          __bf16 *d = colimg + (c4 + c) * CS + TOK * tq;
          if constexpr (TOK == 4) {
            *(bf16x4 *)d = (bf16x4){p[0].h[c], p[1].h[c], p[2].h[c], p[3].h[c]};
            *(bf16x4 *)(d + IMG) = (bf16x4){p[0].m[c], p[1].m[c], p[2].m[c], p[3].m[c]};
            *(bf16x4 *)(d + 2 * IMG) = (bf16x4){p[0].l[c], p[1].l[c], p[2].l[c], p[3].l[c]};
          } else {
            *(bf16x2 *)d = (bf16x2){p[0].h[c], p[1].h[c]};
            *(bf16x2 *)(d + IMG) = (bf16x2){p[0].m[c], p[1].m[c]};
            *(bf16x2 *)(d + 2 * IMG) = (bf16x2){p[0].l[c], p[1].l[c]};
          }
        }
      }
    }
  }
  __device__ static void first(const float *tile, int l31, int h, const Frag &frag, f32x16 &acc) {
    const __bf16 *rp = (const __bf16 *)tile + l31 * RS + 8 * h;
    f32x16 corr;
#pragma unroll
    for (int g = 0; g < 16; ++g) corr[g] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const Pieces8 t = {*(const bf16x8 *)(rp + 16 * s), *(const bf16x8 *)(rp + 16 * s + IMG), *(const bf16x8 *)(rp + 16 * s + 2 * IMG)};
      six_products(t, frag[s], corr, acc);
    }
    acc += corr;
  }
  // an accumulator tile as a B operand: k-step s = registers 8s..8s+7, split here, and only here
  __device__ static X operand(const f32x16 &x) {
    X r;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = x[8 * s + j];
      split8(v, r.s[s]);
    }
    return r;
  }
  template <bool ROW>
  __device__ static void second(const float *tile, int col_off, int l31, int h, const X &x, f32x16 &out) {
    const __bf16 *cp = (const __bf16 *)tile + (ROW ? 3 * IMG : 0) + (col_off + l31) * CS + 4 * h;
    f32x16 corr;
#pragma unroll
    for (int g = 0; g < 16; ++g) corr[g] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Pieces8 t;
      const __bf16 *p = cp + 16 * s;
      t.h = __builtin_shufflevector(*(const bf16x4 *)p, *(const bf16x4 *)(p + 8), 0, 1, 2, 3, 4, 5, 6, 7);
      t.m = __builtin_shufflevector(*(const bf16x4 *)(p + IMG), *(const bf16x4 *)(p + IMG + 8), 0, 1, 2, 3, 4, 5, 6, 7);
      t.l = __builtin_shufflevector(*(const bf16x4 *)(p + 2 * IMG), *(const bf16x4 *)(p + 2 * IMG + 8), 0, 1, 2, 3, 4, 5, 6, 7);
      six_products(t, x.s[s], corr, out);
    }
    out += corr;
  }
};

// ---------------------------------------------------------------------------------------
// All three bodies: block = QW waves of 32 queries (or keys) x SPLIT groups.  Group g walks the inner tiles g, g+SPLIT, ... with
// its own LDS tiles; the groups' partial results are merged pairwise through LDS at the end (a fixed tree: 0<-1, 2<-3, ..., 0<-2,
// ..., so the result depends on (QW, SPLIT) only, never on timing).  578 tokens give 19 wave-tiles per (frame, head): 228 per layer at
// batch 1, 912 at batch 4, for 1024 SIMDs -- so the launcher picks (QW, SPLIT) from the number of wave-tiles: few of them => one wave
// per group and up to 8 key groups (the serial key loop, which is what bounds a small launch, gets 4x shorter), many => 4 waves
// sharing each staged tile.  With QW = 1 a group is one wave, which orders its own LDS traffic: no block barrier in the loop.
// ---------------------------------------------------------------------------------------
template <int QW>
__device__ inline void group_sync() {
  if (QW == 1) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}
constexpr int cmax(int a, int b) { return a > b ? a : b; }
// floats of LDS: SPLIT groups of GROUP floats (the staged tiles + per-tile row statistics), reused after the loop for SPLIT/2 merge slots
// of QW x NREG x 64 floats
template <int QW, int SPLIT, int NREG, int GROUP>
constexpr int smem_floats() { return cmax(SPLIT * GROUP, cmax(SPLIT / 2, 1) * QW * NREG * 64); }

// Sum the groups' accumulator tiles into group 0: tree over the groups, fixed order.
template <int QW, int SPLIT, int NTILES>
__device__ inline void merge_sum(float *smem, int grp, int wave, int lane, f32x16 (&acc)[NTILES]) {
  if (SPLIT == 1) return;
#pragma unroll
  for (int s = 1; s < SPLIT; s <<= 1) {
    float *cw = smem + ((grp / (2 * s)) * QW + wave) * (16 * NTILES) * 64 + lane;
    __syncthreads();   // tiles (round 1) / the slot's previous contents are dead
    if ((grp & (2 * s - 1)) == s) {
#pragma unroll
      for (int t = 0; t < NTILES; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) cw[(t * 16 + g) * 64] = acc[t][g];
    }
    __syncthreads();
    if ((grp & (2 * s - 1)) == 0 && grp + s < SPLIT) {
#pragma unroll
      for (int t = 0; t < NTILES; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[t][g] += cw[(t * 16 + g) * 64];
    }
  }
}

// forward: wave = 32 queries; loop over 32-key tiles.  K is read by rows (S^T = K Q^T), V by columns (O^T += V^T P^T).
template <class P, int QW, int SPLIT>
__device__ inline void attn_fwd_body(const float *__restrict__ qkv, int T, int nh, float scale, float *__restrict__ out, float *__restrict__ lse) {
  constexpr int NT = 64 * QW, KF = P::tile_floats(true, false), GROUP = KF + P::tile_floats(false, true);
  __shared__ __attribute__((aligned(16))) float smem[smem_floats<QW, SPLIT, 34, GROUP>()];
  const int tid = threadIdx.x % NT, grp = threadIdx.x / NT;
  float *Ks = smem + grp * GROUP, *Vs = Ks + KF;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * (32 * QW) + wave * 32 + l31;   // this lane's query (the accumulator column)
  const bool qv = q < T;
  // 578 tokens = 18 wave-tiles + 2 rows: with 4 waves per block the 20th wave-tile holds no query at all.  Such a wave still stages
  // tiles and keeps the barriers, but skips its MFMAs and softmax (wave-uniform), leaving the SIMD to the waves beside it.
  const bool wave_live = blockIdx.x * (32 * QW) + wave * 32 < T;
  const float sl2 = scale * LOG2E;

  typename P::Frag qf;
  P::load_frag(qkv_row(qkv, b, qv ? q : 0, 0, hd, T, nh), h, qv, qf);
  P::fold(qf, sl2);

  f32x16 o0, o1;
#pragma unroll
  for (int g = 0; g < 16; ++g) o0[g] = o1[g] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int ntiles = (T + 31) / 32;
  const int iters = (ntiles + SPLIT - 1) / SPLIT;
  typename P::template Stage<NT> rk, rv;
  P::template prefetch<NT>(qkv, b, hd, 1, grp * 32, T, nh, tid, rk);
  P::template prefetch<NT>(qkv, b, hd, 2, grp * 32, T, nh, tid, rv);
  for (int it = 0; it < iters; ++it) {
    const int kt = it * SPLIT + grp;
    P::template store<NT, true, false>(Ks, tid, rk);
    P::template store<NT, false, true>(Vs, tid, rv);
    group_sync<QW>();
    if (it + 1 < iters) {
      P::template prefetch<NT>(qkv, b, hd, 1, (kt + SPLIT) * 32, T, nh, tid, rk);
      P::template prefetch<NT>(qkv, b, hd, 2, (kt + SPLIT) * 32, T, nh, tid, rv);
    }
    if (kt < ntiles && wave_live) {
      // S^T[key][q] * scale * log2(e): rows = keys of this tile, column = this lane's query
      f32x16 st;
#pragma unroll
      for (int g = 0; g < 16; ++g) st[g] = 0.f;
      P::first(Ks, l31, h, qf, st);
#pragma unroll
      for (int g = 0; g < 16; ++g) st[g] = P::score(st[g], sl2);
      if (kt == ntiles - 1) {   // only the last tile has keys past T (wave-uniform branch)
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if (kt * 32 + acc_row(g, h) >= T) st[g] = -INFINITY;
      }
      float mx = fmaxf(fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])), fmaxf(fmaxf(st[4], st[5]), fmaxf(st[6], st[7])));
      mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(st[8], st[9]), fmaxf(st[10], st[11])), fmaxf(fmaxf(st[12], st[13]), fmaxf(st[14], st[15]))));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));     // the other 16 keys of the tile live in the partner half
      const float m_new = fmaxf(m, mx);
      float rs = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float p = exp2_raw(st[g] - m_new);
        st[g] = p;
        rs += p;   // l sums the unrounded exponentials
      }
      rs += __shfl_xor(rs, 32, 64);
      if (__any(m_new != m)) {   // the running maximum moved for some query of this wave: rescale (a factor of exactly 1 is skipped)
        const float alpha = exp2_raw(m - m_new);
        l *= alpha;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          o0[g] *= alpha;
          o1[g] *= alpha;
        }
      }
      l += rs;
      m = m_new;
      // O^T[dv][q] += sum_key V[key][dv] * P^T[key][q]
      const typename P::X pb = P::operand(st);
      P::template second<false>(Vs, 0, l31, h, pb, o0);
      P::template second<false>(Vs, 32, l31, h, pb, o1);
    }
    group_sync<QW>();
  }
  if (SPLIT > 1) {   // merge the groups' (m, l, O): tree in fixed order
#pragma unroll
    for (int s = 1; s < SPLIT; s <<= 1) {
      float *cw = smem + ((grp / (2 * s)) * QW + wave) * 34 * 64 + lane;
      __syncthreads();
      if ((grp & (2 * s - 1)) == s) {
        cw[0] = m;
        cw[64] = l;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          cw[(2 + g) * 64] = o0[g];
          cw[(18 + g) * 64] = o1[g];
        }
      }
      __syncthreads();
      if ((grp & (2 * s - 1)) == 0 && grp + s < SPLIT) {
        const float m1 = cw[0], l1 = cw[64];
        const float mt = fmaxf(m, m1);
        const float a0 = (m == -INFINITY) ? 0.f : exp2f(m - mt), a1 = (m1 == -INFINITY) ? 0.f : exp2f(m1 - mt);
        l = l * a0 + l1 * a1;
        m = mt;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          o0[g] = o0[g] * a0 + cw[(2 + g) * 64] * a1;
          o1[g] = o1[g] * a0 + cw[(18 + g) * 64] * a1;
        }
      }
    }
  }
  if (qv && grp == 0) {
    const float inv = 1.f / l;
    float *op = out + (((int64_t)b * T + q) * nh + hd) * HD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      int r = acc_row(4 * g4, h);
      *(float4 *)(op + r) = make_float4(o0[4 * g4] * inv, o0[4 * g4 + 1] * inv, o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv);
      *(float4 *)(op + 32 + r) = make_float4(o1[4 * g4] * inv, o1[4 * g4 + 1] * inv, o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv);
    }
    if (h == 0) lse[((int64_t)b * nh + hd) * T + q] = (m + log2f(l)) * LN2;   // ln sum_k exp(scale * s)
  }
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
// delta[b,h,t] = sum_dv dO[b,t,h,dv] * O[b,t,h,dv] in fp32, dO as the precision's products read it (P::dO)
template <class P>
__device__ inline void attn_delta_body(const float *__restrict__ o, const float *__restrict__ go, int64_t rows, int T, int nh, float *__restrict__ delta) {
  // one 16-lane group per (b, t, h) row of 64 floats
  const int64_t gid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  if (gid >= rows) return;
  float4 a = *(const float4 *)(o + gid * HD + sub * 4);
  float4 g = *(const float4 *)(go + gid * HD + sub * 4);
  float s = a.x * P::dO(g.x) + a.y * P::dO(g.y) + a.z * P::dO(g.z) + a.w * P::dO(g.w);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
  if (sub == 0) {
    int64_t bt = gid / nh;
    int hd = (int)(gid - bt * nh);
    int64_t bb = bt / T;
    int t = (int)(bt - bb * T);
    delta[(bb * nh + hd) * T + t] = s;
  }
}

// dK, dV: wave = 32 keys; loop over 32-query tiles.  Q and dO are read by rows (S = Q K^T, dP = dO V^T) and by columns (dK^T += Q^T dS,
// dV^T += dO^T P).
template <class P, int QW, int SPLIT>
__device__ inline void attn_bwd_kv_body(const float *__restrict__ qkv, const float *__restrict__ go, const float *__restrict__ lse,
                                        const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  constexpr int NT = 64 * QW, TF = P::tile_floats(true, true), GROUP = 2 * TF + 64;   // floats per group: two tiles + lse / delta of the tile
  __shared__ __attribute__((aligned(16))) float smem[smem_floats<QW, SPLIT, 64, GROUP>()];
  const int tid = threadIdx.x % NT, grp = threadIdx.x / NT;
  float *Qs = smem + grp * GROUP, *Gs = Qs + TF, *s_lse = Gs + TF, *s_delta = s_lse + 32;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int key = blockIdx.x * (32 * QW) + wave * 32 + l31;   // accumulator column = this lane's key
  const bool kv = key < T;
  const bool wave_live = blockIdx.x * (32 * QW) + wave * 32 < T;   // a wave-tile with no key at all skips its products (see attn_fwd_body)
  const float sl2 = scale * LOG2E;

  typename P::Frag kf, vf;
  P::load_frag(qkv_row(qkv, b, kv ? key : 0, 1, hd, T, nh), h, kv, kf);
  P::load_frag(qkv_row(qkv, b, kv ? key : 0, 2, hd, T, nh), h, kv, vf);
  P::fold(kf, sl2);

  f32x16 acc[4];   // dV^T tile 0/1, dK^T tile 0/1
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;

  const int ntiles = (T + 31) / 32;
  const int iters = (ntiles + SPLIT - 1) / SPLIT;
  typename P::template Stage<NT> rq, rg;
  P::template prefetch<NT>(qkv, b, hd, 0, grp * 32, T, nh, tid, rq);
  P::template prefetch_o<NT>(go, b, hd, grp * 32, T, nh, tid, rg);
  for (int it = 0; it < iters; ++it) {
    const int qt = it * SPLIT + grp;
    P::template store<NT, true, true>(Qs, tid, rq);
    P::template store<NT, true, true>(Gs, tid, rg);
    if (tid < 32) {
      int t = qt * 32 + tid;
      s_lse[tid] = t < T ? lse[((int64_t)b * nh + hd) * T + t] * LOG2E : 0.f;
      s_delta[tid] = t < T ? delta[((int64_t)b * nh + hd) * T + t] : 0.f;
    }
    group_sync<QW>();
    if (it + 1 < iters) {
      P::template prefetch<NT>(qkv, b, hd, 0, (qt + SPLIT) * 32, T, nh, tid, rq);
      P::template prefetch_o<NT>(go, b, hd, (qt + SPLIT) * 32, T, nh, tid, rg);
    }
    if (qt < ntiles && wave_live) {
      // S[q][key] and dP[q][key]: rows = queries of the tile, column = this lane's key
      f32x16 s, dp;
#pragma unroll
      for (int g = 0; g < 16; ++g) s[g] = dp[g] = 0.f;
      P::first(Qs, l31, h, kf, s);
      P::first(Gs, l31, h, vf, dp);
      // P = exp2(S - lse), dS = P (dP - delta) scale.  A key lane past T holds zero K / V fragments: its column is finite garbage
      // that is never stored; query rows past T exist in the last tile only (wave-uniform branch).
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int r = acc_row(g, h);
        const float p = exp2_raw(P::score(s[g], sl2) - s_lse[r]);
        s[g] = p;                                            // P
        dp[g] = p * (dp[g] - s_delta[r]) * scale;             // dS
      }
      if (qt == ntiles - 1) {
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if (qt * 32 + acc_row(g, h) >= T) s[g] = dp[g] = 0.f;
      }
      // dV^T[dv][key] += sum_q dO[q][dv] P[q][key];  dK^T[d][key] += sum_q Q[q][d] dS[q][key]
      const typename P::X pb = P::operand(s), db = P::operand(dp);
      P::template second<true>(Gs, 0, l31, h, pb, acc[0]);
      P::template second<true>(Gs, 32, l31, h, pb, acc[1]);
      P::template second<true>(Qs, 0, l31, h, db, acc[2]);
      P::template second<true>(Qs, 32, l31, h, db, acc[3]);
    }
    group_sync<QW>();
  }
  merge_sum<QW, SPLIT, 4>(smem, grp, wave, lane, acc);
  if (kv && grp == 0) {
    float *kp = gqkv + ((((int64_t)b * T + key) * 3 + 1) * nh + hd) * HD;
    float *vp = gqkv + ((((int64_t)b * T + key) * 3 + 2) * nh + hd) * HD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      int r = acc_row(4 * g4, h);
      *(float4 *)(vp + r) = make_float4(acc[0][4 * g4], acc[0][4 * g4 + 1], acc[0][4 * g4 + 2], acc[0][4 * g4 + 3]);
      *(float4 *)(vp + 32 + r) = make_float4(acc[1][4 * g4], acc[1][4 * g4 + 1], acc[1][4 * g4 + 2], acc[1][4 * g4 + 3]);
      *(float4 *)(kp + r) = make_float4(acc[2][4 * g4], acc[2][4 * g4 + 1], acc[2][4 * g4 + 2], acc[2][4 * g4 + 3]);
      *(float4 *)(kp + 32 + r) = make_float4(acc[3][4 * g4], acc[3][4 * g4 + 1], acc[3][4 * g4 + 2], acc[3][4 * g4 + 3]);
    }
  }
}

// dQ: wave = 32 queries; loop over 32-key tiles.  K is read by rows (S^T) and by columns (dQ^T += K^T dS^T), V by rows (dP^T = V dO^T).
template <class P, int QW, int SPLIT>
__device__ inline void attn_bwd_q_body(const float *__restrict__ qkv, const float *__restrict__ go, const float *__restrict__ lse,
                                       const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  constexpr int NT = 64 * QW, KF = P::tile_floats(true, true), GROUP = KF + P::tile_floats(true, false);
  __shared__ __attribute__((aligned(16))) float smem[smem_floats<QW, SPLIT, 32, GROUP>()];
  const int tid = threadIdx.x % NT, grp = threadIdx.x / NT;
  float *Ks = smem + grp * GROUP, *Vs = Ks + KF;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * (32 * QW) + wave * 32 + l31;
  const bool qv = q < T;
  const bool wave_live = blockIdx.x * (32 * QW) + wave * 32 < T;   // a wave-tile with no query at all skips its products (see attn_fwd_body)
  const float sl2 = scale * LOG2E;

  typename P::Frag qf, gf;
  P::load_frag(qkv_row(qkv, b, qv ? q : 0, 0, hd, T, nh), h, qv, qf);
  P::fold(qf, sl2);
  P::load_frag(go + (((int64_t)b * T + (qv ? q : 0)) * nh + hd) * HD, h, qv, gf);
  const float my_lse = qv ? lse[((int64_t)b * nh + hd) * T + q] * LOG2E : 0.f;
  const float my_delta = qv ? delta[((int64_t)b * nh + hd) * T + q] : 0.f;

  f32x16 acc[2];
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[0][g] = acc[1][g] = 0.f;

  const int ntiles = (T + 31) / 32;
  const int iters = (ntiles + SPLIT - 1) / SPLIT;
  typename P::template Stage<NT> rk, rv;
  P::template prefetch<NT>(qkv, b, hd, 1, grp * 32, T, nh, tid, rk);
  P::template prefetch<NT>(qkv, b, hd, 2, grp * 32, T, nh, tid, rv);
  for (int it = 0; it < iters; ++it) {
    const int kt = it * SPLIT + grp;
    P::template store<NT, true, true>(Ks, tid, rk);
    P::template store<NT, true, false>(Vs, tid, rv);
    group_sync<QW>();
    if (it + 1 < iters) {
      P::template prefetch<NT>(qkv, b, hd, 1, (kt + SPLIT) * 32, T, nh, tid, rk);
      P::template prefetch<NT>(qkv, b, hd, 2, (kt + SPLIT) * 32, T, nh, tid, rv);
    }
    if (kt < ntiles && wave_live) {
      // S^T[key][q], dP^T[key][q]
      f32x16 st, dpt;
#pragma unroll
      for (int g = 0; g < 16; ++g) st[g] = dpt[g] = 0.f;
      P::first(Ks, l31, h, qf, st);
      P::first(Vs, l31, h, gf, dpt);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float p = exp2_raw(P::score(st[g], sl2) - my_lse);
        dpt[g] = p * (dpt[g] - my_delta) * scale;   // dS^T
      }
      if (kt == ntiles - 1) {   // key rows past T: only in the last tile (their K rows are zero, so P would be exp2(-lse), not 0)
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if (kt * 32 + acc_row(g, h) >= T) dpt[g] = 0.f;
      }
      // dQ^T[d][q] += sum_key K[key][d] dS^T[key][q]
      const typename P::X db = P::operand(dpt);
      P::template second<true>(Ks, 0, l31, h, db, acc[0]);
      P::template second<true>(Ks, 32, l31, h, db, acc[1]);
    }
    group_sync<QW>();
  }
  merge_sum<QW, SPLIT, 2>(smem, grp, wave, lane, acc);
  if (qv && grp == 0) {
    float *qp = gqkv + ((((int64_t)b * T + q) * 3 + 0) * nh + hd) * HD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      int r = acc_row(4 * g4, h);
      *(float4 *)(qp + r) = make_float4(acc[0][4 * g4], acc[0][4 * g4 + 1], acc[0][4 * g4 + 2], acc[0][4 * g4 + 3]);
      *(float4 *)(qp + 32 + r) = make_float4(acc[1][4 * g4], acc[1][4 * g4 + 1], acc[1][4 * g4 + 2], acc[1][4 * g4 + 3]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// The kernels: the names that profiles and tools key on, one wrapper per body and precision.
// ---------------------------------------------------------------------------------------
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_fwd_kernel(const float *__restrict__ qkv, int T, int nh, float scale, float *__restrict__ out,
    float *__restrict__ lse) {
  attn_fwd_body<AttnF32, QW, SPLIT>(qkv, T, nh, scale, out, lse);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_kv_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  attn_bwd_kv_body<AttnF32, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_q_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  attn_bwd_q_body<AttnF32, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
__global__ void attn_delta_kernel(const float *__restrict__ o, const float *__restrict__ go, int64_t rows, int T, int nh, float *__restrict__ delta) {
  attn_delta_body<AttnF32>(o, go, rows, T, nh, delta);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_fwd_bf16_kernel(const float *__restrict__ qkv, int T, int nh, float scale, float *__restrict__ out,
    float *__restrict__ lse) {
  attn_fwd_body<AttnBf16, QW, SPLIT>(qkv, T, nh, scale, out, lse);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_kv_bf16_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  attn_bwd_kv_body<AttnBf16, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_q_bf16_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  attn_bwd_q_body<AttnBf16, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
__global__ void attn_delta_bf16_kernel(const float *__restrict__ o, const float *__restrict__ go, int64_t rows, int T, int nh, float *__restrict__ delta) {
  attn_delta_body<AttnBf16>(o, go, rows, T, nh, delta);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_fwd_split_kernel(const float *__restrict__ qkv, int T, int nh, float scale, float *__restrict__ out,
    float *__restrict__ lse) {
  if constexpr (AttnSplit::built(QW, SPLIT, false)) attn_fwd_body<AttnSplit, QW, SPLIT>(qkv, T, nh, scale, out, lse);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_kv_split_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  if constexpr (AttnSplit::built(QW, SPLIT, true)) attn_bwd_kv_body<AttnSplit, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
template <int QW, int SPLIT>
__global__ __launch_bounds__(64 * QW * SPLIT) void attn_bwd_q_split_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
    const float *__restrict__ lse, const float *__restrict__ delta, int T, int nh, float scale, float *__restrict__ gqkv) {
  if constexpr (AttnSplit::built(QW, SPLIT, true)) attn_bwd_q_body<AttnSplit, QW, SPLIT>(qkv, go, lse, delta, T, nh, scale, gqkv);
}
__global__ void attn_delta_split_kernel(const float *__restrict__ o, const float *__restrict__ go, int64_t rows, int T, int nh, float *__restrict__ delta) {
  attn_delta_body<AttnSplit>(o, go, rows, T, nh, delta);
}

// ---------------------------------------------------------------------------------------
// host: a family = the entry names that front its messages, its three kernels and its delta kernel
// ---------------------------------------------------------------------------------------
struct AttnF32Family {
  static constexpr const char *fwd_name = "ftx_attn_fwd", *bwd_name = "ftx_attn_bwd", *tiled = "_tiled";   // "ftx_attn_fwd_tiled: (..) is not .."
  template <int QW, int SPLIT> static constexpr auto fwd = attn_fwd_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_kv = attn_bwd_kv_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_q = attn_bwd_q_kernel<QW, SPLIT>;
  static constexpr auto delta = attn_delta_kernel;
  static bool built(int qw, int split, bool backward);
  static void config(int b, int t, int h, bool backward, int &qw, int &split);
};
struct AttnBf16Family {
  static constexpr const char *fwd_name = "ftx_attn_fwd_bf16", *bwd_name = "ftx_attn_bwd_bf16", *tiled = "";
  template <int QW, int SPLIT> static constexpr auto fwd = attn_fwd_bf16_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_kv = attn_bwd_kv_bf16_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_q = attn_bwd_q_bf16_kernel<QW, SPLIT>;
  static constexpr auto delta = attn_delta_bf16_kernel;
  static bool built(int qw, int split, bool backward);
  static void config(int b, int t, int h, bool backward, int &qw, int &split);
};
struct AttnSplitFamily {
  static constexpr const char *fwd_name = "ftx_attn_fwd_split", *bwd_name = "ftx_attn_bwd_split", *tiled = "";
  template <int QW, int SPLIT> static constexpr auto fwd = attn_fwd_split_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_kv = attn_bwd_kv_split_kernel<QW, SPLIT>;
  template <int QW, int SPLIT> static constexpr auto bwd_q = attn_bwd_q_split_kernel<QW, SPLIT>;
  static constexpr auto delta = attn_delta_split_kernel;
  static bool built(int qw, int split, bool backward);
  static void config(int b, int t, int h, bool backward, int &qw, int &split);
};

static int attn_check(const char *who, int b, int t, int h, int d) {
  FTX_REQUIRE(b >= 1 && t >= 1 && h >= 1, "%s: bad size", who);
  FTX_REQUIRE(d == HD, "%s: head dim must be 64 (got %d)", who, d);
  FTX_REQUIRE(b <= 65535 && h <= 65535, "%s: batch / heads exceed the grid limits", who);
  return FTX_OK;
}

// (QW, SPLIT) of a launch: an explicit, built tiling from the caller (ftx_attn_fwd_tiled / ftx_attn_bwd_tiled: tests and tools/bench_attn.py
// walk them), or (0, 0) = chosen here from the number of 32-row wave-tiles against the SIMDs of an MI355X (256 CUs x 4; a constant, not a
// device query: the choice -- hence nothing a caller can observe but time -- must not depend on the environment).  No process-wide state.
// Measured at 578 tokens x 12 heads (tools/bench_attn.py, us fwd / bwd): batch 1 (228 wave-tiles) (4,2) 52 / 170, (1,8) 21 / 75,
// (1,4) 23 / 70; batch 2 (4,2) 52 / 170, (2,4) 34 / 103; batch 4 (4,2) 54 / 174, (2,4) 65 / 199; batch 8 (4,2) 106 / 342, others slower.
// Both families build this set and share attn_config's choice (measured for bf16: see DESIGN section 4).
static bool attn_tiling_built(int qw, int split) {
  return (qw == 0 && split == 0) || (qw == 4 && split == 2) || (qw == 2 && (split == 2 || split == 4)) ||
         (qw == 1 && (split == 2 || split == 4 || split == 8));
}
static void attn_config(int b, int t, int h, bool backward, int &qw, int &split) {
  if (qw != 0) return;   // explicit
  const int64_t wave_tiles = (int64_t)ceil_div(t, 32) * h * b;
  const int64_t simds = 4 * 256;
  if (wave_tiles * 4 <= simds) { qw = 1; split = backward ? 4 : 8; }   // a quarter of the SIMDs or fewer: shortest key loop
  else if (wave_tiles * 2 <= simds) { qw = 2; split = 4; }
  else { qw = 4; split = 2; }
}

bool AttnF32Family::built(int qw, int split, bool) { return attn_tiling_built(qw, split); }
bool AttnBf16Family::built(int qw, int split, bool) { return attn_tiling_built(qw, split); }
void AttnF32Family::config(int b, int t, int h, bool backward, int &qw, int &split) { attn_config(b, t, h, backward, qw, split); }
void AttnBf16Family::config(int b, int t, int h, bool backward, int &qw, int &split) { attn_config(b, t, h, backward, qw, split); }

// The split family's own set and choice: the tilings whose blocks fit the LDS (AttnSplit::built).  Forward: attn_config's thresholds
// with the nearest built tiling -- one wave per group up to a quarter of the SIMDs, two up to half, four above.  Backward: (2,2) at every
// size.  (4,2) is built and is the faster backward from batch 4 up at 578 tokens x 12 heads (154 us against 184), but
// its dK/dV kernel keeps 80 bytes of scratch per lane (two fragments in pieces, four gradient tiles and two split accumulator tiles
// are 256 registers before anything else), and the automatic choice keeps to kernels without scratch; (1,2) runs one block of two
// waves per CU (111 KB of LDS) and loses to (2,2) at every size measured.
bool AttnSplitFamily::built(int qw, int split, bool backward) {
  return attn_tiling_built(qw, split) && ((qw == 0 && split == 0) || AttnSplit::built(qw, split, backward));
}
void AttnSplitFamily::config(int b, int t, int h, bool backward, int &qw, int &split) {
  if (qw != 0) return;   // explicit
  if (backward) { qw = 2; split = 2; return; }
  const int64_t wave_tiles = (int64_t)ceil_div(t, 32) * h * b;
  const int64_t simds = 4 * 256;
  qw = wave_tiles * 4 <= simds ? 1 : wave_tiles * 2 <= simds ? 2 : 4;
  split = qw == 4 ? 2 : 4;
}
extern "C" int32_t ftx_attn_split_tiling_built(int32_t qw, int32_t split, int32_t backward) {
  return (qw != 0 || split != 0) && AttnSplitFamily::built(qw, split, backward != 0);
}

#define ATTN_DISPATCH(KERNEL, ...)                                                                               \
  do {                                                                                                           \
    dim3 grid((unsigned)ceil_div(t, 32 * qw), (unsigned)h, (unsigned)b);                                         \
    if (qw == 4) KERNEL<4, 2><<<grid, 512, 0, st>>>(__VA_ARGS__);                                                \
    else if (qw == 2 && split == 2) KERNEL<2, 2><<<grid, 256, 0, st>>>(__VA_ARGS__);                             \
    else if (qw == 2) KERNEL<2, 4><<<grid, 512, 0, st>>>(__VA_ARGS__);                                           \
    else if (split == 2) KERNEL<1, 2><<<grid, 128, 0, st>>>(__VA_ARGS__);                                        \
    else if (split == 4) KERNEL<1, 4><<<grid, 256, 0, st>>>(__VA_ARGS__);                                        \
    else KERNEL<1, 8><<<grid, 512, 0, st>>>(__VA_ARGS__);                                                        \
  } while (0)

template <class F>
static int attn_fwd_entry(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw, int32_t split,
                          void *stream) {
  const char *me = F::fwd_name;
  int rc = attn_check(me, b, t, h, d);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(qkv && out && lse, "%s: null pointer", me);
  FTX_REQUIRE(F::built(qw, split, false), "%s%s: (%d, %d) is not a built tiling", me, F::tiled, qw, split);
  hipStream_t st = (hipStream_t)stream;
  F::config(b, t, h, false, qw, split);
  ATTN_DISPATCH(F::template fwd, qkv, t, h, scale, out, lse);
  return check_launch(me);
}

extern "C" size_t ftx_attn_bwd_workspace_bytes(int32_t b, int32_t t, int32_t h) {
  if (b <= 0 || t <= 0 || h <= 0) return 256;
  return sizeof(float) * (size_t)b * t * h + 256;
}

template <class F>
static int attn_bwd_entry(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h, int32_t d,
                          float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split, void *stream) {
  const char *me = F::bwd_name;
  int rc = attn_check(me, b, t, h, d);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(qkv && out && grad_out && lse && grad_qkv && workspace, "%s: null pointer", me);
  FTX_REQUIRE(F::built(qw, split, true), "%s%s: (%d, %d) is not a built tiling", me, F::tiled, qw, split);
  if (workspace_bytes < ftx_attn_bwd_workspace_bytes(b, t, h)) return workspace_short(me, workspace_bytes, ftx_attn_bwd_workspace_bytes(b, t, h));
  hipStream_t st = (hipStream_t)stream;
  float *delta = (float *)workspace;
  const int64_t rows = (int64_t)b * t * h;
  F::delta<<<(unsigned)ceil_div(rows * 16, 256), 256, 0, st>>>(out, grad_out, rows, t, h, delta);
  F::config(b, t, h, true, qw, split);
  ATTN_DISPATCH(F::template bwd_kv, qkv, grad_out, lse, delta, t, h, scale, grad_qkv);
  ATTN_DISPATCH(F::template bwd_q, qkv, grad_out, lse, delta, t, h, scale, grad_qkv);
  return check_launch(me);
}

extern "C" int ftx_attn_fwd_tiled(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw,
                                  int32_t split, void *stream) {
  return attn_fwd_entry<AttnF32Family>(qkv, b, t, h, d, scale, out, lse, qw, split, stream);
}
extern "C" int ftx_attn_fwd(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, void *stream) {
  return attn_fwd_entry<AttnF32Family>(qkv, b, t, h, d, scale, out, lse, 0, 0, stream);
}
extern "C" int ftx_attn_fwd_bf16(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw,
                                 int32_t split, void *stream) {
  return attn_fwd_entry<AttnBf16Family>(qkv, b, t, h, d, scale, out, lse, qw, split, stream);
}
extern "C" int ftx_attn_bwd_tiled(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h,
                                  int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split,
                                  void *stream) {
  return attn_bwd_entry<AttnF32Family>(qkv, out, grad_out, lse, b, t, h, d, scale, grad_qkv, workspace, workspace_bytes, qw, split, stream);
}
extern "C" int ftx_attn_bwd(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h,
                            int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, void *stream) {
  return attn_bwd_entry<AttnF32Family>(qkv, out, grad_out, lse, b, t, h, d, scale, grad_qkv, workspace, workspace_bytes, 0, 0, stream);
}
extern "C" int ftx_attn_bwd_bf16(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h,
                                 int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split,
                                 void *stream) {
  return attn_bwd_entry<AttnBf16Family>(qkv, out, grad_out, lse, b, t, h, d, scale, grad_qkv, workspace, workspace_bytes, qw, split, stream);
}
extern "C" int ftx_attn_fwd_split(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw,
                                  int32_t split, void *stream) {
  return attn_fwd_entry<AttnSplitFamily>(qkv, b, t, h, d, scale, out, lse, qw, split, stream);
}
extern "C" int ftx_attn_bwd_split(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h,
                                  int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split,
                                  void *stream) {
  return attn_bwd_entry<AttnSplitFamily>(qkv, out, grad_out, lse, b, t, h, d, scale, grad_qkv, workspace, workspace_bytes, qw, split, stream);
}
