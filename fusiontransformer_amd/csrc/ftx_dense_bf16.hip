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
// The kernels (dense_gemm_kernel, dense_wgrad_kernel), the epilogue, the tile and split rules and the host layer are shared with
// ftx_dense_split.hip: ftx_dense_common.h.  This file says what is the bf16 family's own, the description DenseBf16, and holds its entries.
#include "ftx_dense_common.h"

using namespace ftx;

struct DenseBf16 {
  static constexpr const char *gemm_name = "ftx_dense_gemm_bf16", *wgrad_name = "ftx_dense_wgrad_bf16";
  static constexpr const char *patch_name = "ftx_vit_patch_embed_bf16", *tap_name = "ftx_vit_tap_stem_bf16";
  static constexpr const char *patch_bwd_name = "ftx_vit_patch_embed_bwd_bf16", *tap_fwd_name = "ftx_vit_tap_stem_train_fwd_bf16";
  static constexpr const char *tap_bwd_name = "ftx_vit_tap_stem_bwd_bf16";
  // the rows GEMM of the family's mode: the tap stem's data gradient, whose reduction (co = 96) is no multiple of kDenseGranule
  static constexpr auto rows_gemm = &ftx_rows_gemm_bf16;

  static constexpr int NP = 1;           // one bf16 image per operand
  static constexpr int BK = 64;          // reduction elements (rows, in the weight gradient) staged per step: four k-steps of 16
  static constexpr int STRIDE = 72;      // bf16 per LDS row (144 B): conflict-free ds_read_b128 (WB_STRIDE of ftx_spconv_bf16.hip)
  static constexpr int MIN_BLOCKS = 1;   // no demand: every kernel keeps the registers it had without one (profiles/dense_shared_bodies.txt)

  struct Pieces4 {
    bf16x4 p[NP];
  };
  // the ONE place the operands are rounded
  static __device__ Pieces4 pieces(float4 v) { return {{round4(v)}}; }

  // one product per k-step into one accumulator, which is the sum
  static constexpr int NACC = 1, NPROD = 1;
  static constexpr int PROD[NPROD][3] = {{0, 0, 0}};
  static __device__ float sum(const float (&a)[NACC]) { return a[0]; }
};

// the staging constants the bf16 kernels were written with fall out of DenseStage's formula
static_assert(DenseStage<DenseBf16>::ROWS == 16 && DenseStage<DenseBf16>::F4 == 16, "16 rows x 16 float4 per pass");
static_assert(DenseStage<DenseBf16>::pair_items(128) == 128 / 32 && DenseStage<DenseBf16>::pair_items(64) == 64 / 32, "W [K][N]: BN / 32 items");
static_assert(DenseStage<DenseBf16>::pair_items(kDenseDwTile) == 4, "weight gradient: 4 (row pair, float4) items per thread and operand");

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

extern "C" size_t ftx_vit_patch_embed_bwd_bf16_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim) {
  return dense_patch_bwd_workspace_bytes(b, c, h, w, patch, dim);
}

extern "C" int ftx_vit_patch_embed_bwd_bf16(const float *dtokens, const float *img, const float *W, int32_t b, int32_t c, int32_t h, int32_t w,
                                           int32_t patch, int32_t dim, int32_t t0, float *dW, float *dbias, float *dcls, float *ddist, float *dpos,
                                           float *dimg, void *workspace, size_t workspace_bytes, void *stream) {
  return dense_patch_embed_bwd_entry<DenseBf16>(dtokens, img, W, b, c, h, w, patch, dim, t0, dW, dbias, dcls, ddist, dpos, dimg, workspace, workspace_bytes,
                                              stream);
}

extern "C" int ftx_vit_tap_stem_train_fwd_bf16(const float *tokens, const float *W, const float *bias, int32_t b, int32_t g, int32_t t0, int32_t dim,
                                              int32_t co, float *rows, void *stream) {
  return dense_tap_stem_train_fwd_entry<DenseBf16>(tokens, W, bias, b, g, t0, dim, co, rows, stream);
}

extern "C" size_t ftx_vit_tap_stem_bwd_bf16_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co) {
  return dense_tap_bwd_workspace_bytes(b, g, dim, co);
}

extern "C" int ftx_vit_tap_stem_bwd_bf16(const float *drows, const float *rows, const float *tokens, const float *W, int32_t b, int32_t g, int32_t t0,
                                        int32_t dim, int32_t co, float *dW, float *dbias, float *dtokens, void *workspace, size_t workspace_bytes,
                                        void *stream) {
  return dense_tap_stem_bwd_entry<DenseBf16>(drows, rows, tokens, W, b, g, t0, dim, co, dW, dbias, dtokens, workspace, workspace_bytes, stream);
}

extern "C" size_t ftx_dense_wgrad_bf16_workspace_bytes(int64_t m, int32_t n, int32_t k) { return dense_wgrad_workspace_bytes(m, n, k); }

extern "C" int ftx_dense_wgrad_bf16(const float *G, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes,
                                    void *stream) {
  return dense_wgrad_entry<DenseBf16>(G, X, m, n, k, dW, workspace, workspace_bytes, stream);
}

extern "C" int ftx_dense_bf16_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host) {
  return dense_tile_entry("ftx_dense_bf16_tile", form, m, n, k, tile_m_host, tile_n_host, split_host);
}
