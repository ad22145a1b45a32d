// Native eval-mode executor of the ViT image branch (include/ftx.h: ftx_vit_eval).  Where the Python path uses torch (the residual
// stream as one tensor, transformers._materialize) it issues ftx_rows_add_bias (ftx_rows.hip).
//
// The trunk is three host tables (model, blocks, taps; fusiontransformer_amd/native_image.py writes them from the module tree).  This
// file validates them, places every intermediate in the caller's arena and issues, per block, exactly what transformers.Block.chain
// issues through the library's own entry points: add + LayerNorm, qkv, attention, proj, add + LayerNorm, fc1 + GELU, fc2.  The residual
// stream stays (r, p, pb) with value r + (p + pb) from block to block and becomes one tensor only at a tap.  Nothing here synchronises
// or allocates; the one thing kept beyond a call is a host-side note per arena address of which blocks its residual state has seen
// (ftx_vit_eval_release drops it).
#include <mutex>
#include <string>
#include <unordered_map>
#include "ftx_vit_tables.h"

using namespace ftx;
using namespace ftx::vit;   // the records and their checker, shared with the training executor (ftx_vit_tables.h)

namespace {

// Where everything lives, in bytes from the arena's start.  A function of (model sizes, b) alone.
struct Plan {
  int64_t rows = 0, tokens = 0;
  int64_t r[2] = {0, 0}, m = 0, h = 0, qkv = 0, att = 0, proj = 0, pre = 0, act = 0, x = 0, lse = 0, stats = 0, total = 0;
};

void make_plan(const Model &M, int32_t b, Plan &P) {
  P.tokens = tokens_of(M);
  P.rows = (int64_t)b * P.tokens;
  const int64_t row = align256(4 * P.rows * M.dim), wide = align256(4 * P.rows * M.hidden);
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = off;
    off += bytes;
    return at;
  };
  P.r[0] = take(row);
  P.r[1] = take(row);
  P.m = take(row);
  P.h = take(row);
  P.qkv = take(3 * row);
  P.att = take(row);
  P.proj = take(row);
  P.pre = take(wide);
  P.act = take(wide);
  P.x = take(row);
  P.lse = take(align256(4 * (int64_t)b * M.heads * P.tokens));
  P.stats = take(align256(8 * P.rows));
  P.total = off < 256 ? 256 : off;
}

// which blocks the residual state of an arena has seen (host side; the state itself is device memory inside the arena)
struct State {
  int32_t b, dim, tokens, next, r;
};
std::mutex g_mu;
std::unordered_map<const void *, State> g_state;

int fail(const char *what, int block, int rc) {
  const std::string inner = ftx_last_error();
  set_error("ftx_vit_eval: block %d (%s): %s", block, what, inner.c_str());
  return rc;
}

}  // namespace

extern "C" int32_t ftx_vit_model_bytes(void) { return (int32_t)sizeof(Model); }
extern "C" int32_t ftx_vit_block_bytes(void) { return (int32_t)sizeof(Block); }
extern "C" int32_t ftx_vit_tap_bytes(void) { return (int32_t)sizeof(Tap); }

// Drops the note about `arena`: for a caller that frees or hands on an arena.  Host only.
extern "C" int ftx_vit_eval_release(const void *arena) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_state.erase(arena);
  return FTX_OK;
}

extern "C" size_t ftx_vit_eval_arena_bytes(const void *model_host, int32_t n_blocks, int32_t b) {
  const Model *M = (const Model *)model_host;
  if (check_model("ftx_vit_eval_arena_bytes", M, n_blocks, b) != FTX_OK) return 0;
  Plan P;
  make_plan(*M, b, P);
  return (size_t)P.total;
}

extern "C" int ftx_vit_eval(const void *model_host, const void *blocks_host, int32_t n_blocks, const void *taps_host, int32_t n_taps, int32_t b,
                            const float *img, const float *tokens_in, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode,
                            float *const *tap_out_host, void *arena, size_t arena_bytes, void *stream) {
  const char *who = "ftx_vit_eval";
  const Model *Mp = (const Model *)model_host;
  const Block *blocks = (const Block *)blocks_host;
  const Tap *taps = (const Tap *)taps_host;
  int rc = check_model(who, Mp, n_blocks, b);
  if (rc != FTX_OK) return rc;
  const Model &M = *Mp;
  rc = check_range(who, blocks, n_blocks, block_first, block_last, linear_mode, attn_mode);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n_taps >= 0 && n_taps <= kMaxBlocks && (taps || !n_taps) && (tap_out_host || !n_taps), "%s: null tap table or tap count outside [0, %d]", who,
              kMaxBlocks);
  for (int i = 0; i < n_taps; ++i) {
    const Tap &T = taps[i];
    FTX_REQUIRE(T.block >= 0 && (i == 0 || T.block > taps[i - 1].block), "%s: tap %d: taps must be ascending by block (block=%d)", who, i, T.block);
    FTX_REQUIRE(T.block <= block_last, "%s: tap %d: block %d is past block_last %d", who, i, T.block, block_last);
    FTX_REQUIRE(T.co >= 4 && T.co % 4 == 0, "%s: tap %d: co must be a multiple of 4 (co=%d)", who, i, T.co);
    if (T.block < block_first) continue;   // an earlier call on this arena produced it
    FTX_REQUIRE(T.stem_w && T.stem_b && T.gamma && T.beta && T.mean && T.var, "%s: tap %d: null parameter", who, i);
    FTX_REQUIRE(b == 0 || tap_out_host[i], "%s: tap %d: null output", who, i);
    FTX_REQUIRE(al16(T.stem_w) && al16(T.stem_b) && al16(tap_out_host[i]), "%s: tap %d: stem weight, bias and output must be 16-byte aligned", who, i);
  }
  rc = check_blocks(who, blocks, block_first, block_last);
  if (rc != FTX_OK) return rc;
  if (block_first > 0)
    FTX_REQUIRE(blocks[block_first - 1].fc2_b && al16(blocks[block_first - 1].fc2_b), "%s: block %d: null or misaligned parameter (fc2 bias)", who,
                block_first - 1);
  if (block_first == 0 && !tokens_in) {
    FTX_REQUIRE(b == 0 || img, "%s: block_first = 0 needs the image or tokens_in", who);
    FTX_REQUIRE(M.patch_w && M.patch_b && M.cls && M.pos && (M.dist || M.t0 == 1), "%s: null parameter in the model record", who);
    FTX_REQUIRE(((int64_t)M.in_chans * M.patch * M.patch) % 64 == 0, "%s: in_chans * patch * patch must be a multiple of 64", who);
    FTX_REQUIRE(al16(M.patch_w) && al16(M.patch_b) && al16(M.cls) && al16(M.dist) && al16(M.pos), "%s: the model record's pointers must be 16-byte aligned", who);
  }
  FTX_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)tokens_in & 15) == 0, "%s: pointers must be 16-byte aligned", who);
  Plan P;
  make_plan(M, b, P);
  FTX_REQUIRE(P.rows <= 0x7fffffff / 2, "%s: too large", who);
  if (b == 0) return FTX_OK;
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "%s: the arena must be a 256-byte aligned device buffer", who);
  if (arena_bytes < (size_t)P.total) {
    set_error("%s: arena %zu < required %zu (ftx_vit_eval_arena_bytes)", who, arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  int cur = 0;   // which of the two residual buffers holds r
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (block_first > 0) {
      const auto it = g_state.find(arena);
      FTX_REQUIRE(it != g_state.end() && it->second.b == b && it->second.dim == M.dim && it->second.tokens == (int32_t)P.tokens,
                  "%s: block_first = %d, but the arena holds no residual state for b = %d", who, block_first, b);
      FTX_REQUIRE(it->second.next == block_first, "%s: block_first = %d, but the arena's residual state is in front of block %d", who, block_first,
                  it->second.next);
      cur = it->second.r;
    }
    g_state.erase(arena);   // a call that fails half-way leaves no state behind
  }

  char *base = (char *)arena;
  auto at = [&](int64_t off) { return (float *)(base + off); };
  float *h = at(P.h), *qkv = at(P.qkv), *att = at(P.att), *proj = at(P.proj), *pre = at(P.pre), *act = at(P.act), *m = at(P.m), *x = at(P.x);
  float *lse = at(P.lse), *mean = at(P.stats), *rstd = at(P.stats) + P.rows;
  const int64_t rows = P.rows;
  const int T = (int)P.tokens, G = M.grid * M.grid, dim = M.dim;
  auto gemm = linear_mode ? ftx_dense_gemm_bf16 : ftx_dense_gemm_split;
#define RUN(what, call)                      \
  do {                                       \
    rc = (call);                             \
    if (rc != FTX_OK) return fail(what, i, rc); \
  } while (0)
  // everything above answered on the host; from here on launches only
  const float *r = nullptr;
  bool have_m = block_first > 0;   // the stream is (r, m, fc2 bias of the previous block); else just r
  int next_tap = 0;
  while (next_tap < n_taps && taps[next_tap].block < block_first) ++next_tap;
  if (block_first == 0) {
    const int i = -1;
    if (tokens_in) {
      r = tokens_in;
    } else {
      const int side = M.grid * M.patch;
      RUN("patch embedding", (linear_mode ? ftx_vit_patch_embed_bf16 : ftx_vit_patch_embed_split)(img, M.patch_w, M.patch_b, M.cls, M.dist, M.pos, b, M.in_chans,
                                                                                                 side, side, M.patch, dim, M.t0, at(P.r[0]), stream));
      r = at(P.r[0]);
      cur = 0;
    }
  } else {
    r = at(P.r[cur]);
  }
  for (int i = block_first; i <= block_last; ++i) {
    const Block &B = blocks[i];
    const float *s = r;
    if (have_m) {
      float *s_out = at(P.r[r == at(P.r[0]) ? 1 : 0]);
      RUN("norm1", ftx_add_layernorm_fwd(r, m, blocks[i - 1].fc2_b, B.norm1_w, B.norm1_b, M.eps, rows, dim, s_out, h, mean, rstd, stream));
      s = s_out;
    } else {
      RUN("norm1", ftx_add_layernorm_fwd(r, nullptr, nullptr, B.norm1_w, B.norm1_b, M.eps, rows, dim, nullptr, h, mean, rstd, stream));
    }
    RUN("qkv", gemm(h, B.qkv_w, 0, B.qkv_b, nullptr, rows, 3 * dim, dim, FTX_EPI_BIAS, qkv, nullptr, stream));
    if (attn_mode == 2) RUN("attention", ftx_attn_fwd_split(qkv, b, T, M.heads, 64, 0.125f, att, lse, 0, 0, stream));
    else if (attn_mode == 1) RUN("attention", ftx_attn_fwd_bf16(qkv, b, T, M.heads, 64, 0.125f, att, lse, 0, 0, stream));
    else RUN("attention", ftx_attn_fwd_tiled(qkv, b, T, M.heads, 64, 0.125f, att, lse, 0, 0, stream));
    RUN("proj", gemm(att, B.proj_w, 0, nullptr, nullptr, rows, dim, dim, FTX_EPI_NONE, proj, nullptr, stream));
    float *s2 = at(P.r[s == at(P.r[0]) ? 1 : 0]);
    RUN("norm2", ftx_add_layernorm_fwd(s, proj, B.proj_b, B.norm2_w, B.norm2_b, M.eps, rows, dim, s2, h, mean, rstd, stream));
    RUN("fc1", gemm(h, B.fc1_w, 0, B.fc1_b, nullptr, rows, M.hidden, dim, FTX_EPI_BIAS_GELU, act, pre, stream));
    RUN("fc2", gemm(act, B.fc2_w, 0, nullptr, nullptr, rows, dim, M.hidden, FTX_EPI_NONE, m, nullptr, stream));
    r = s2;
    have_m = true;
    if (next_tap < n_taps && taps[next_tap].block == i) {
      const Tap &Tp = taps[next_tap];
      RUN("materialise", ftx_rows_add_bias(r, m, B.fc2_b, rows, dim, x, stream));
      RUN("tap stem", (linear_mode ? ftx_vit_tap_stem_bf16 : ftx_vit_tap_stem_split)(x, Tp.stem_w, Tp.stem_b, Tp.gamma, Tp.beta, Tp.mean, Tp.var, Tp.eps, b, G,
                                                                                    M.t0, dim, Tp.co, tap_out_host[next_tap], stream));
      ++next_tap;
    }
  }
#undef RUN
  {
    std::lock_guard<std::mutex> lock(g_mu);
    g_state[arena] = State{b, dim, (int32_t)P.tokens, block_last + 1, r == at(P.r[0]) ? 0 : 1};
  }
  return FTX_OK;
}
