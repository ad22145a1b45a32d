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
// The kernels (dense_gemm_kernel, dense_wgrad_kernel), the epilogue, the tile and split rules and the host layer are shared with
// ftx_dense_bf16.hip: ftx_dense_common.h.  This file says what is the split family's own, the description DenseSplit, and holds its entries.
#include "ftx_dense_common.h"
#include "ftx_split.h"   // split1: the ONE definition of the split, shared with ftx_spconv_split.hip

using namespace ftx;

struct DenseSplit {
  static constexpr const char *gemm_name = "ftx_dense_gemm_split", *wgrad_name = "ftx_dense_wgrad_split";
  static constexpr const char *patch_name = "ftx_vit_patch_embed_split", *tap_name = "ftx_vit_tap_stem_split";
  static constexpr const char *patch_bwd_name = "ftx_vit_patch_embed_bwd_split", *tap_fwd_name = "ftx_vit_tap_stem_train_fwd_split";
  static constexpr const char *tap_bwd_name = "ftx_vit_tap_stem_bwd_split";
  // the rows GEMM of the family's mode: the tap stem's data gradient, whose reduction (co = 96) is no multiple of kDenseGranule
  static constexpr auto rows_gemm = &ftx_rows_gemm_split;

  // LDS: three bf16 images per operand.  The stage is 32 reduction elements deep with a 40-element (80 B) row stride: 6 x 128 x 80 B
  // = 61 440 B at the 128 x 128 tile, under the 64 KB a static __shared__ array may take without a function attribute, two blocks per CU.
  // (The 64-deep stage of the bf16 kernels would need 110 592 B.)  80 B rows keep the ds_read_b128 fragment reads conflict-free: the 16
  // rows of a quarter wave start at 16 distinct multiples of four banks.  __launch_bounds__(256, 2) keeps the 128 x 128 kernels at or
  // under 256 registers so that two blocks do share a CU (measured: 13 % less time per block of Linears at batch 4 than one block per CU).
  static constexpr int NP = 3;           // pieces h, m, l
  static constexpr int BK = 32;          // reduction elements (rows, in the weight gradient) staged per step: two k-steps of 16
  static constexpr int STRIDE = 40;      // bf16 per LDS row (80 B): conflict-free ds_read_b128
  static constexpr int MIN_BLOCKS = 2;

  struct Pieces4 {
    bf16x4 p[NP];   // h, m, l
  };
  // the ONE place the operands are split
  static __device__ Pieces4 pieces(float4 v) {
    Pieces4 s;
    __bf16 h, m, l;
    split1(v.x, h, m, l); s.p[0][0] = h; s.p[1][0] = m; s.p[2][0] = l;
    split1(v.y, h, m, l); s.p[0][1] = h; s.p[1][1] = m; s.p[2][1] = l;
    split1(v.z, h, m, l); s.p[0][2] = h; s.p[1][2] = m; s.p[2][2] = l;
    split1(v.w, h, m, l); s.p[0][3] = h; s.p[1][3] = m; s.p[2][3] = l;
    return s;
  }

  // (piece of the MFMA's first operand: W / X, piece of its second: A / dY, accumulator) in the documented order: the five
  // corrections smallest first into `corr` (mm, lh, hl, mh, hm here; the contract names the A / dY piece first: mm, hl, lh, hm, mh),
  // then hh into its own accumulator.  out = hh + corr.
  static constexpr int NACC = 2, NPROD = 6;   // accumulator 0: hh, 1: corr
  static constexpr int PROD[NPROD][3] = {{1, 1, 1}, {2, 0, 1}, {0, 2, 1}, {1, 0, 1}, {0, 1, 1}, {0, 0, 0}};
  static __device__ float sum(const float (&a)[NACC]) { return a[0] + a[1]; }
};

// the staging constants the split kernels were written with fall out of DenseStage's formula
static_assert(DenseStage<DenseSplit>::ROWS == 32 && DenseStage<DenseSplit>::F4 == 8, "32 rows x 8 float4 per pass");
static_assert(DenseStage<DenseSplit>::pair_items(128) == 128 / 64 && DenseStage<DenseSplit>::pair_items(64) == 64 / 64, "W [K][N]: BN / 64 items");
static_assert(DenseStage<DenseSplit>::pair_items(kDenseDwTile) == 2, "weight gradient: 2 (row pair, float4) items per thread and operand");

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

extern "C" size_t ftx_vit_patch_embed_bwd_split_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim) {
  return dense_patch_bwd_workspace_bytes(b, c, h, w, patch, dim);
}

extern "C" int ftx_vit_patch_embed_bwd_split(const float *dtokens, const float *img, const float *W, int32_t b, int32_t c, int32_t h, int32_t w,
                                           int32_t patch, int32_t dim, int32_t t0, float *dW, float *dbias, float *dcls, float *ddist, float *dpos,
                                           float *dimg, void *workspace, size_t workspace_bytes, void *stream) {
  return dense_patch_embed_bwd_entry<DenseSplit>(dtokens, img, W, b, c, h, w, patch, dim, t0, dW, dbias, dcls, ddist, dpos, dimg, workspace, workspace_bytes,
                                              stream);
}

extern "C" int ftx_vit_tap_stem_train_fwd_split(const float *tokens, const float *W, const float *bias, int32_t b, int32_t g, int32_t t0, int32_t dim,
                                              int32_t co, float *rows, void *stream) {
  return dense_tap_stem_train_fwd_entry<DenseSplit>(tokens, W, bias, b, g, t0, dim, co, rows, stream);
}

extern "C" size_t ftx_vit_tap_stem_bwd_split_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co) {
  return dense_tap_bwd_workspace_bytes(b, g, dim, co);
}

extern "C" int ftx_vit_tap_stem_bwd_split(const float *drows, const float *rows, const float *tokens, const float *W, int32_t b, int32_t g, int32_t t0,
                                        int32_t dim, int32_t co, float *dW, float *dbias, float *dtokens, void *workspace, size_t workspace_bytes,
                                        void *stream) {
  return dense_tap_stem_bwd_entry<DenseSplit>(drows, rows, tokens, W, b, g, t0, dim, co, dW, dbias, dtokens, workspace, workspace_bytes, stream);
}

extern "C" size_t ftx_dense_wgrad_split_workspace_bytes(int64_t m, int32_t n, int32_t k) { return dense_wgrad_workspace_bytes(m, n, k); }

extern "C" int ftx_dense_wgrad_split(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  return dense_wgrad_entry<DenseSplit>(G, X, m, n, k, dW, workspace, workspace_bytes, stream);
}

extern "C" int ftx_dense_split_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  return dense_tile_entry("ftx_dense_split_tile", form, m, n, k, tile_m_host, tile_n_host, split_host);
}
