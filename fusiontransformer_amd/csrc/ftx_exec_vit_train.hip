// Native training executor of the ViT image branch (include/ftx.h: ftx_vit_train_fwd / ftx_vit_train_bwd).
//
// The unit is a trunk segment: blocks [block_first, block_last] from one materialised token tensor x_in to one materialised token
// tensor x_out = r + (m + fc2_b), which is transformers._TrunkSegment.forward without the embedding.  The forward issues per block what
// ftx_vit_eval issues, into per-block regions of the caller's arena that the backward reads; the backward walks the blocks in reverse and
// issues, through the library's own entry points with the same arguments, what the autograd nodes of the package issue
// (_Materialize, _VitMlp, _AddLayerNorm, _VitLinear, _Attention, _LayerNorm of functional.py and models/transformers.py), so every
// result has the bits of that path.  The model and block records are ftx_vit_eval's, checked by the same checker (ftx_vit_tables.h).
// Nothing here synchronises or allocates; the one thing kept beyond a call is a host-side note per arena address of which forward it
// holds and whether its backward has run (ftx_vit_train_release drops it).
#include <algorithm>
#include <mutex>
#include <string>
#include <unordered_map>
#include "ftx_vit_tables.h"

using namespace ftx;
using namespace ftx::vit;

namespace {

// Where everything lives, in bytes from the arena's start.  A function of (model sizes, b, blocks in the segment) alone.
struct Saved {   // of one block: what its backward reads
  int64_t s, stats1, h, qkv, att, lse, s2, stats2, h2, pre, act;
};
struct Plan {
  int64_t rows = 0, tokens = 0;
  Saved blk[kMaxBlocks];
  int64_t g[3] = {0, 0, 0}, dpre = 0, gqkv = 0, ws = 0, stage = 0, total = 0;
  size_t ws_attn = 0, ws_ln = 0, ws_col_d = 0, ws_col_h = 0, ws_col_q = 0;
  size_t ws_w2[2] = {0, 0}, ws_w1[2] = {0, 0}, ws_wp[2] = {0, 0}, ws_wq[2] = {0, 0};   // weight-gradient workspaces by linear_mode
};

void make_plan(const Model &M, int32_t b, int32_t n_seg, Plan &P) {
  P.tokens = tokens_of(M);
  P.rows = (int64_t)b * P.tokens;
  const int64_t rows = P.rows;
  const int32_t D = M.dim, H = M.hidden;
  const int64_t row = align256(4 * rows * D), wide = align256(4 * rows * H);
  const int64_t stats = align256(8 * rows), lse = align256(4 * (int64_t)b * M.heads * P.tokens);
  Offsets256 off;
  for (int k = 0; k < n_seg; ++k) {
    Saved &S = P.blk[k];
    S.s = k ? off.take(row) : -1;   // the first block's LayerNorm input is x_in itself
    S.stats1 = off.take(stats);
    S.h = off.take(row);
    S.qkv = off.take(3 * row);
    S.att = off.take(row);
    S.lse = off.take(lse);
    S.s2 = off.take(row);
    S.stats2 = off.take(stats);
    S.h2 = off.take(row);
    S.pre = off.take(wide);
    S.act = off.take(wide);
  }
  // the shared temporaries: three token-sized buffers the gradients flow through (the forward keeps the MLP and the proj output in
  // the first two), fc1's output gradient, the attention's input gradient, one workspace for whichever op runs, the LayerNorm's
  // parameter gradients where the caller's three buffers are not consecutive
  for (int j = 0; j < 3; ++j) P.g[j] = off.take(row);
  P.dpre = off.take(wide);
  P.gqkv = off.take(3 * row);
  P.ws_attn = ftx_attn_bwd_workspace_bytes(b, (int32_t)P.tokens, M.heads);
  P.ws_ln = ftx_layernorm_bwd_workspace_bytes(rows, D);
  P.ws_col_d = ftx_colsum_workspace_bytes(rows, D);
  P.ws_col_h = ftx_colsum_workspace_bytes(rows, H);
  P.ws_col_q = ftx_colsum_workspace_bytes(rows, 3 * D);
  P.ws_w2[0] = ftx_dense_wgrad_split_workspace_bytes(rows, D, H);
  P.ws_w2[1] = ftx_dense_wgrad_bf16_workspace_bytes(rows, D, H);
  P.ws_w1[0] = ftx_dense_wgrad_split_workspace_bytes(rows, H, D);
  P.ws_w1[1] = ftx_dense_wgrad_bf16_workspace_bytes(rows, H, D);
  P.ws_wp[0] = ftx_dense_wgrad_split_workspace_bytes(rows, D, D);
  P.ws_wp[1] = ftx_dense_wgrad_bf16_workspace_bytes(rows, D, D);
  P.ws_wq[0] = ftx_dense_wgrad_split_workspace_bytes(rows, 3 * D, D);
  P.ws_wq[1] = ftx_dense_wgrad_bf16_workspace_bytes(rows, 3 * D, D);
  size_t ws = std::max({P.ws_attn, P.ws_ln, P.ws_col_d, P.ws_col_h, P.ws_col_q});
  for (int j = 0; j < 2; ++j) ws = std::max({ws, P.ws_w2[j], P.ws_w1[j], P.ws_wp[j], P.ws_wq[j]});
  P.ws = off.take((int64_t)ws);
  P.stage = off.take(4 * 3 * (int64_t)D);
  P.total = off.end < 256 ? 256 : off.end;
}

// which forward an arena holds (host side; what the backward reads is device memory inside the arena)
struct Note {
  int32_t b, first, last, linear_mode, attn_mode, dim, tokens;
  bool backward_ran;
};
std::mutex g_mu;
std::unordered_map<const void *, Note> g_note;

int fail(const char *who, const char *what, int block, int rc) {
  const std::string inner = ftx_last_error();
  set_error("%s: block %d (%s): %s", who, block, what, inner.c_str());
  return rc;
}

// what both directions check of a call before anything is launched
int check_call(const char *who, const Model *Mp, const Block *blocks, int32_t n_blocks, int32_t b, int32_t block_first, int32_t block_last,
               int32_t linear_mode, int32_t attn_mode) {
  int rc = check_model(who, Mp, n_blocks, b);
  if (rc != FTX_OK) return rc;
  rc = check_range(who, blocks, n_blocks, block_first, block_last, linear_mode, attn_mode);
  if (rc != FTX_OK) return rc;
  return check_blocks(who, blocks, block_first, block_last);
}

int check_arena(const char *who, const void *arena, size_t arena_bytes, const Plan &P) {
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "%s: the arena must be a 256-byte aligned device buffer", who);
  if (arena_bytes < (size_t)P.total) {
    set_error("%s: arena %zu < required %zu (ftx_vit_train_arena_bytes)", who, arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  return FTX_OK;
}

}  // namespace

extern "C" int32_t ftx_vit_train_block_bytes(void) { return (int32_t)sizeof(Block); }

// Drops the note about `arena`: for a caller that frees or hands on an arena.  Host only.
extern "C" int ftx_vit_train_release(const void *arena) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_note.erase(arena);
  return FTX_OK;
}

extern "C" size_t ftx_vit_train_arena_bytes(const void *model_host, int32_t n_blocks, int32_t block_first, int32_t block_last, int32_t b) {
  const char *who = "ftx_vit_train_arena_bytes";
  const Model *M = (const Model *)model_host;
  if (check_model(who, M, n_blocks, b) != FTX_OK) return 0;
  if (!(block_first >= 0 && block_first <= block_last && block_last < n_blocks)) {
    set_error("%s: blocks [%d, %d] outside 0..%d", who, block_first, block_last, n_blocks - 1);
    return 0;
  }
  Plan P;
  make_plan(*M, b, block_last - block_first + 1, P);
  return (size_t)P.total;
}

#define RUN(what, call)                              \
  do {                                               \
    rc = (call);                                     \
    if (rc != FTX_OK) return fail(who, what, i, rc); \
  } while (0)

extern "C" int ftx_vit_train_fwd(const void *model_host, const void *blocks_host, int32_t n_blocks, int32_t b, const float *x_in, int32_t block_first,
                                 int32_t block_last, int32_t linear_mode, int32_t attn_mode, float *x_out, void *arena, size_t arena_bytes, void *stream) {
  const char *who = "ftx_vit_train_fwd";
  const Model *Mp = (const Model *)model_host;
  const Block *blocks = (const Block *)blocks_host;
  int rc = check_call(who, Mp, blocks, n_blocks, b, block_first, block_last, linear_mode, attn_mode);
  if (rc != FTX_OK) return rc;
  const Model &M = *Mp;
  FTX_REQUIRE(b == 0 || (x_in && x_out), "%s: null x_in or x_out", who);
  FTX_REQUIRE(al16(x_in) && al16(x_out), "%s: x_in and x_out must be 16-byte aligned", who);
  FTX_REQUIRE((int64_t)b * tokens_of(M) <= 0x7fffffff / 2, "%s: too large", who);
  if (b == 0) return FTX_OK;
  Plan P;
  make_plan(M, b, block_last - block_first + 1, P);
  rc = check_arena(who, arena, arena_bytes, P);
  if (rc != FTX_OK) return rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    g_note.erase(arena);   // a call that fails half-way leaves no forward behind
  }
  char *base = (char *)arena;
  auto at = [&](int64_t off) { return (float *)(base + off); };
  const int64_t rows = P.rows;
  const int T = (int)P.tokens, dim = M.dim;
  auto gemm = linear_mode ? ftx_dense_gemm_bf16 : ftx_dense_gemm_split;
  auto attn = attn_mode == 2 ? ftx_attn_fwd_split : attn_mode == 1 ? ftx_attn_fwd_bf16 : ftx_attn_fwd_tiled;
  float *m = at(P.g[0]), *proj = at(P.g[1]);
  // everything above answered on the host; from here on launches only
  const float *r = x_in;   // the stream is (r, m, fc2 bias of the previous block) behind the first block, just r in front of it
  for (int i = block_first; i <= block_last; ++i) {
    const Block &B = blocks[i];
    const Saved &S = P.blk[i - block_first];
    float *mean1 = at(S.stats1), *mean2 = at(S.stats2);
    const float *s = r;
    if (i == block_first) {
      RUN("norm1", ftx_add_layernorm_fwd(r, nullptr, nullptr, B.norm1_w, B.norm1_b, M.eps, rows, dim, nullptr, at(S.h), mean1, mean1 + rows, stream));
    } else {
      RUN("norm1", ftx_add_layernorm_fwd(r, m, blocks[i - 1].fc2_b, B.norm1_w, B.norm1_b, M.eps, rows, dim, at(S.s), at(S.h), mean1, mean1 + rows, stream));
      s = at(S.s);
    }
    RUN("qkv", gemm(at(S.h), B.qkv_w, 0, B.qkv_b, nullptr, rows, 3 * dim, dim, FTX_EPI_BIAS, at(S.qkv), nullptr, stream));
    RUN("attention", attn(at(S.qkv), b, T, M.heads, 64, 0.125f, at(S.att), at(S.lse), 0, 0, stream));
    RUN("proj", gemm(at(S.att), B.proj_w, 0, nullptr, nullptr, rows, dim, dim, FTX_EPI_NONE, proj, nullptr, stream));
    RUN("norm2", ftx_add_layernorm_fwd(s, proj, B.proj_b, B.norm2_w, B.norm2_b, M.eps, rows, dim, at(S.s2), at(S.h2), mean2, mean2 + rows, stream));
    RUN("fc1", gemm(at(S.h2), B.fc1_w, 0, B.fc1_b, nullptr, rows, M.hidden, dim, FTX_EPI_BIAS_GELU, at(S.act), at(S.pre), stream));
    RUN("fc2", gemm(at(S.act), B.fc2_w, 0, nullptr, nullptr, rows, dim, M.hidden, FTX_EPI_NONE, m, nullptr, stream));
    r = at(S.s2);
  }
  {
    const int i = block_last;
    RUN("materialise", ftx_rows_add_bias(r, m, blocks[i].fc2_b, rows, dim, x_out, stream));
  }
  {
    std::lock_guard<std::mutex> lock(g_mu);
    g_note[arena] = Note{b, block_first, block_last, linear_mode, attn_mode, dim, (int32_t)P.tokens, false};
  }
  return FTX_OK;
}

extern "C" int ftx_vit_train_bwd(const void *model_host, const void *blocks_host, const void *grads_host, int32_t n_blocks, int32_t b, const float *x_in,
                                 const float *grad_out, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode, float *grad_in,
                                 void *arena, size_t arena_bytes, void *stream) {
  const char *who = "ftx_vit_train_bwd";
  const Model *Mp = (const Model *)model_host;
  const Block *blocks = (const Block *)blocks_host;
  const Block *grads = (const Block *)grads_host;   // the gradient table: a block record whose pointers are written
  int rc = check_call(who, Mp, blocks, n_blocks, b, block_first, block_last, linear_mode, attn_mode);
  if (rc != FTX_OK) return rc;
  const Model &M = *Mp;
  FTX_REQUIRE(grads, "%s: null gradient table", who);
  rc = check_blocks(who, grads, block_first, block_last, "gradient");
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(b == 0 || (x_in && grad_out && grad_in), "%s: null x_in, grad_out or grad_in", who);
  FTX_REQUIRE(al16(x_in) && al16(grad_out) && al16(grad_in), "%s: x_in, grad_out and grad_in must be 16-byte aligned", who);
  FTX_REQUIRE((int64_t)b * tokens_of(M) <= 0x7fffffff / 2, "%s: too large", who);
  if (b == 0) return FTX_OK;
  Plan P;
  make_plan(M, b, block_last - block_first + 1, P);
  rc = check_arena(who, arena, arena_bytes, P);
  if (rc != FTX_OK) return rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    const auto it = g_note.find(arena);
    const bool match = it != g_note.end() && it->second.b == b && it->second.first == block_first && it->second.last == block_last &&
                       it->second.linear_mode == linear_mode && it->second.attn_mode == attn_mode && it->second.dim == M.dim &&
                       it->second.tokens == (int32_t)P.tokens;
    FTX_REQUIRE(match, "%s: no forward of b = %d, blocks [%d, %d], linear_mode %d, attn_mode %d ran on this arena", who, b, block_first, block_last, linear_mode,
                attn_mode);
    FTX_REQUIRE(!it->second.backward_ran, "%s: the backward of this forward has run already (a second backward needs a second forward)", who);
    it->second.backward_ran = true;   // the temporaries are overwritten from the first launch on
  }
  char *base = (char *)arena;
  auto at = [&](int64_t off) { return (float *)(base + off); };
  const int64_t rows = P.rows;
  const int T = (int)P.tokens, dim = M.dim, hid = M.hidden;
  const int lm = linear_mode;
  auto gemm = lm ? ftx_dense_gemm_bf16 : ftx_dense_gemm_split;
  auto wgrad = lm ? ftx_dense_wgrad_bf16 : ftx_dense_wgrad_split;
  auto attn = attn_mode == 2 ? ftx_attn_bwd_split : attn_mode == 1 ? ftx_attn_bwd_bf16 : ftx_attn_bwd_tiled;
  float *ga = at(P.g[0]), *gb = at(P.g[1]), *gc = at(P.g[2]), *dpre = at(P.dpre), *gqkv = at(P.gqkv), *stage = at(P.stage);
  void *ws = at(P.ws);
  // The LayerNorm backward writes d gamma, d beta (, d y_bias) as one (2 or 3, dim) array: straight into the caller's buffers where
  // they are consecutive, else into the arena and from there, row by row, with the copy form of ftx_rows_add_bias.
  auto together = [&](const float *g0, const float *g1, const float *g2) { return g1 == g0 + dim && (!g2 || g2 == g1 + dim); };
  // everything above answered on the host; from here on launches only
  {
    const int i = block_last;   // _Materialize.backward: the last fc2 bias
    RUN("fc2 bias gradient", ftx_colsum(grad_out, rows, dim, (float *)grads[i].fc2_b, ws, P.ws_col_d, stream));
  }
  const float *gs = grad_out;   // the gradient of the block's s2 and of its MLP output
  for (int i = block_last; i >= block_first; --i) {
    const Block &B = blocks[i];
    const Block &G = grads[i];
    const Saved &S = P.blk[i - block_first];
    const bool first = i == block_first;
    const float *s = first ? x_in : at(S.s);
    const float *mean1 = at(S.stats1), *mean2 = at(S.stats2);
    // _VitMlp.backward
    RUN("fc2 data gradient", gemm(gs, B.fc2_w, 1, nullptr, at(S.pre), rows, hid, dim, FTX_EPI_DGELU, dpre, nullptr, stream));
    RUN("fc2 weight gradient", wgrad(gs, at(S.act), rows, dim, hid, (float *)G.fc2_w, ws, P.ws_w2[lm], stream));
    RUN("fc1 data gradient", gemm(dpre, B.fc1_w, 1, nullptr, nullptr, rows, dim, hid, FTX_EPI_NONE, gb, nullptr, stream));
    RUN("fc1 weight gradient", wgrad(dpre, at(S.h2), rows, hid, dim, (float *)G.fc1_w, ws, P.ws_w1[lm], stream));
    RUN("fc1 bias gradient", ftx_colsum(dpre, rows, hid, (float *)G.fc1_b, ws, P.ws_col_h, stream));
    // _AddLayerNorm.backward at norm2, with the proj bias gradient
    {
      const bool direct = together(G.norm2_w, G.norm2_b, G.proj_b);
      float *gp = direct ? (float *)G.norm2_w : stage;
      RUN("norm2 backward", ftx_add_layernorm_bwd(gb, gs, at(S.s2), B.norm2_w, mean2, mean2 + rows, rows, dim, 1, gc, gp, ws, P.ws_ln, stream));
      if (!direct) {
        RUN("norm2 weight gradient", ftx_rows_add_bias(stage, nullptr, nullptr, 1, dim, (float *)G.norm2_w, stream));
        RUN("norm2 bias gradient", ftx_rows_add_bias(stage + dim, nullptr, nullptr, 1, dim, (float *)G.norm2_b, stream));
        RUN("proj bias gradient", ftx_rows_add_bias(stage + 2 * dim, nullptr, nullptr, 1, dim, (float *)G.proj_b, stream));
      }
    }
    // _VitLinear.backward of proj (its bias went with norm2), _Attention.backward, _VitLinear.backward of qkv
    RUN("proj data gradient", gemm(gc, B.proj_w, 1, nullptr, nullptr, rows, dim, dim, FTX_EPI_NONE, ga, nullptr, stream));
    RUN("proj weight gradient", wgrad(gc, at(S.att), rows, dim, dim, (float *)G.proj_w, ws, P.ws_wp[lm], stream));
    RUN("attention backward", attn(at(S.qkv), at(S.att), ga, at(S.lse), b, T, M.heads, 64, 0.125f, gqkv, ws, P.ws_attn, 0, 0, stream));
    RUN("qkv data gradient", gemm(gqkv, B.qkv_w, 1, nullptr, nullptr, rows, dim, 3 * dim, FTX_EPI_NONE, gb, nullptr, stream));
    RUN("qkv weight gradient", wgrad(gqkv, at(S.h), rows, 3 * dim, dim, (float *)G.qkv_w, ws, P.ws_wq[lm], stream));
    RUN("qkv bias gradient", ftx_colsum(gqkv, rows, 3 * dim, (float *)G.qkv_b, ws, P.ws_col_q, stream));
    // norm1: _AddLayerNorm.backward with the previous block's fc2 bias gradient, or _LayerNorm.backward in front of the segment
    {
      float *gprev = first ? nullptr : (float *)grads[i - 1].fc2_b;
      const bool direct = together(G.norm1_w, G.norm1_b, gprev);
      float *gp = direct ? (float *)G.norm1_w : stage;
      RUN("norm1 backward", ftx_add_layernorm_bwd(gb, first ? nullptr : gc, s, B.norm1_w, mean1, mean1 + rows, rows, dim, first ? 0 : 1, ga, gp, ws, P.ws_ln, stream));
      if (!direct) {
        RUN("norm1 weight gradient", ftx_rows_add_bias(stage, nullptr, nullptr, 1, dim, (float *)G.norm1_w, stream));
        RUN("norm1 bias gradient", ftx_rows_add_bias(stage + dim, nullptr, nullptr, 1, dim, (float *)G.norm1_b, stream));
        if (gprev) RUN("fc2 bias gradient", ftx_rows_add_bias(stage + 2 * dim, nullptr, nullptr, 1, dim, gprev, stream));
      }
    }
    // x_in feeds norm1 and the residual: its two gradients, the one of norm2's addend and the one of norm1's input, are one fp32 add
    if (first) RUN("input gradient", ftx_rows_add(gc, ga, rows, dim, grad_in, stream));
    gs = ga;
  }
  return FTX_OK;
}
#undef RUN
