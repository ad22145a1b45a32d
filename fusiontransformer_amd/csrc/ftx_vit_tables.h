// The host tables of the ViT image branch's executors (layouts documented in include/ftx.h) and the one checker of them: ftx_vit_eval
// (ftx_exec_vit.hip) and ftx_vit_train_fwd / _bwd (ftx_exec_vit_train.hip) read the same model and block records and refuse the same
// records with the same texts, `who` being the entry that was called.  Host code only.
#pragma once
#include "ftx_common.h"

namespace ftx {
namespace vit {

struct Model {
  const float *patch_w, *patch_b, *cls, *dist, *pos;
  int32_t dim, heads, hidden, patch, grid, t0, in_chans;
  float eps;
};
struct Block {
  const float *norm1_w, *norm1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct Tap {
  const float *stem_w, *stem_b, *gamma, *beta, *mean, *var;
  int32_t block, co;
  float eps;
  int32_t reserved;
};
static_assert(sizeof(Model) == 72 && sizeof(Block) == 96 && sizeof(Tap) == 64, "table records are packed");

constexpr int kMaxBlocks = 64;
constexpr int kMaxBatch = 4096;

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline int check_model(const char *who, const Model *M, int32_t n_blocks, int32_t b) {
  FTX_REQUIRE(M, "%s: null model record", who);
  FTX_REQUIRE(n_blocks >= 1 && n_blocks <= kMaxBlocks, "%s: block count %d outside [1, %d]", who, n_blocks, kMaxBlocks);
  FTX_REQUIRE(b >= 0 && b <= kMaxBatch, "%s: batch %d outside [0, %d]", who, b, kMaxBatch);
  FTX_REQUIRE(M->dim == 256 || M->dim == 512 || M->dim == 768 || M->dim == 1024, "%s: dim %d is not one the LayerNorm kernel takes (256, 512, 768, 1024)", who,
              M->dim);
  FTX_REQUIRE(M->heads >= 1 && M->heads * 64 == M->dim, "%s: heads * 64 != dim (heads=%d dim=%d)", who, M->heads, M->dim);
  FTX_REQUIRE(M->hidden >= 64 && M->hidden % 64 == 0 && M->hidden <= 16384, "%s: hidden must be a multiple of 64 (hidden=%d)", who, M->hidden);
  FTX_REQUIRE(M->t0 == 1 || M->t0 == 2, "%s: t0 must be 1 or 2 (t0=%d)", who, M->t0);
  FTX_REQUIRE(M->patch >= 4 && M->patch % 4 == 0 && M->patch <= 64 && M->grid >= 1 && M->grid <= 256 && M->in_chans >= 1 && M->in_chans <= 64,
              "%s: patch %d (a multiple of 4), grid %d or channels %d out of range", who, M->patch, M->grid, M->in_chans);
  return FTX_OK;
}

// the block range and the two execution modes of a call
inline int check_range(const char *who, const Block *blocks, int32_t n_blocks, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode) {
  FTX_REQUIRE(blocks, "%s: null block table", who);
  FTX_REQUIRE(block_first >= 0 && block_first <= block_last && block_last < n_blocks, "%s: blocks [%d, %d] outside 0..%d", who, block_first, block_last,
              n_blocks - 1);
  FTX_REQUIRE(linear_mode == 0 || linear_mode == 1, "%s: linear_mode must be 0 (split) or 1 (bf16)", who);
  FTX_REQUIRE(attn_mode >= 0 && attn_mode <= 2, "%s: attn_mode must be 0 (fp32), 1 (bf16) or 2 (split)", who);
  return FTX_OK;
}

// every pointer of the records [block_first, block_last] is there and 16-byte aligned; `what`: "parameter" or "gradient"
inline int check_blocks(const char *who, const Block *blocks, int32_t block_first, int32_t block_last, const char *what = "parameter") {
  for (int i = block_first; i <= block_last; ++i) {
    const Block &B = blocks[i];
    FTX_REQUIRE(B.norm1_w && B.norm1_b && B.qkv_w && B.qkv_b && B.proj_w && B.proj_b && B.norm2_w && B.norm2_b && B.fc1_w && B.fc1_b && B.fc2_w && B.fc2_b,
                "%s: block %d: null %s", who, i, what);
    FTX_REQUIRE(al16(B.norm1_w) && al16(B.norm1_b) && al16(B.qkv_w) && al16(B.qkv_b) && al16(B.proj_w) && al16(B.proj_b) && al16(B.norm2_w) && al16(B.norm2_b) &&
                    al16(B.fc1_w) && al16(B.fc1_b) && al16(B.fc2_w) && al16(B.fc2_b),
                "%s: block %d: %ss must be 16-byte aligned", who, i, what);
  }
  return FTX_OK;
}

// tokens per frame and token rows of a batch
inline int64_t tokens_of(const Model &M) { return M.t0 + (int64_t)M.grid * M.grid; }

}  // namespace vit
}  // namespace ftx
