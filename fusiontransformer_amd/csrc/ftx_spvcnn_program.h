// What the two SPVCNN executors (ftx_exec.hip: eval, ftx_exec_train.hip: training) share on the host: the view of the tables of one
// call, the rule for the two sides of a kernel map, the table of a precision family's sparse-convolution entries, and the ONE checker of the op program against the model and batch tables.
// Nothing here places memory or launches; each executor places its own arena from the facts the checker leaves.  Where the two
// executors ask different things of the same program the checker says so in a `train` / eval branch at that point.
#pragma once
#include <string.h>
#include <string>
#include <vector>
#include "ftx_common.h"
#include "ftx_spvcnn_tables.h"

namespace ftx {

using Layer = SpvcnnLayer;
using Op = SpvcnnOp;
using Map = SpvcnnMap;
using PV = SpvcnnPV;

constexpr int kLevels = 6;        // five voxel levels + the point set
constexpr int kMaxSlots = 256;
constexpr int kMaxOps = 4096;
constexpr int kMaxSegments = 8;   // of the training program; the eval program has the three of FTX_SPVCNN_SEG_*
constexpr int64_t kOstatMaxRows = 64 * 4096;
constexpr const char *kKindName[] = {"?", "conv_bn", "linear_bn", "voxelize", "devoxelize", "concat", "add", "add_ext", "dropout"};

// the tables of one call, as the entry points are given them (layouts documented in include/ftx.h); groutes is the training executor's
struct SpvcnnTables {
  const Layer *layers;
  int32_t n_layers;
  const Op *ops;
  int32_t n_ops;
  const int64_t *rows;
  const Map *maps;
  int32_t n_maps;
  const PV *pvs;
  int32_t n_pvs;
  const int32_t *routes, *groutes;
};
inline SpvcnnTables spvcnn_tables(const void *layers, int32_t n_layers, const void *ops, int32_t n_ops, const int64_t *rows, const void *maps, int32_t n_maps,
                                  const void *pvs, int32_t n_pvs, const int32_t *routes, const int32_t *groutes = nullptr) {
  return {(const Layer *)layers, n_layers, (const Op *)ops, n_ops, rows, (const Map *)maps, n_maps, (const PV *)pvs, n_pvs, routes, groutes};
}

// Per pair the row a layer reads (`gather`) and the row it writes (`scatter`), and per side the (kvol, rows) table of each row's
// pairs: the forward reduces through dst_pos, the data gradient gathers `scatter`, scatters to `gather` and reduces through src_pos.
// A transposed layer swaps the two sides of the map.  This is functional._map_sides.
struct MapSides {
  const int32_t *gather, *scatter, *dst_pos, *src_pos;
};
inline MapSides map_sides(const Layer &L, const Map &M) {
  if (L.transposed) return {M.pair_out, M.pair_in, M.pos_t, M.pos};
  return {M.pair_in, M.pair_out, M.pos, M.pos_t};
}

// The four sparse-convolution entries of a layer's precision family (include/ftx.h): the ONE place the executors pick between the
// fp32 entries (operand mode 0), their bf16 twins (1) and their three-piece split twins (2); check_program admits no other mode.
struct SpconvEntries {
  decltype(&ftx_spconv_pairs_gemm) pairs;
  decltype(&ftx_spconv_pairs_gemm_scatter) scatter;
  decltype(&ftx_rows_gemm) rows;
  decltype(&ftx_spconv_pairs_wgrad) wgrad;
};
inline SpconvEntries spconv_entries(const Layer &L) {
  if (L.bf16 == 2) return {ftx_spconv_pairs_gemm_split, ftx_spconv_pairs_gemm_scatter_split, ftx_rows_gemm_split, ftx_spconv_pairs_wgrad_split};
  if (L.bf16) return {ftx_spconv_pairs_gemm_bf16, ftx_spconv_pairs_gemm_scatter_bf16, ftx_rows_gemm_bf16, ftx_spconv_pairs_wgrad_bf16};
  return {ftx_spconv_pairs_gemm, ftx_spconv_pairs_gemm_scatter, ftx_rows_gemm, ftx_spconv_pairs_wgrad};
}

// What the checker found out about the program, for the placement of either executor.
struct SlotFacts {
  struct PerOp {
    int second;          // the second slot the op reads (residual, concat / add operand), or -1
    int grad_to[2];      // the slots its backward sends a gradient to, by operand, or -1
    int64_t temp_rows;   // of a layer: rows of its one temporary in eval mode (pair rows on the pairs / empty routes, else output rows)
  };
  int level[kMaxSlots], ch[kMaxSlots], def[kMaxSlots];   // per slot: level, channels, the op that writes it (-1: none)
  std::vector<PerOp> op;
  // training only
  int uses[kMaxSlots], galias[kMaxSlots];   // gradient contributions; the slot whose gradient buffer IS this slot's (operand of an add)
  int n_segments = 0, in_slot[kMaxSegments], out_slot[kMaxSegments];
};

// p of a DROPOUT op: reserved0 holds its IEEE bits
inline float dropout_p(const Op &o) {
  float p;
  memcpy(&p, &o.reserved0, sizeof p);
  return p;
}

// an executor's error at op i, around the text of the per-op entry point that refused
inline int fail(const char *entry, int i, const Op &o, int rc) {
  const std::string inner = ftx_last_error();
  set_error("%s: op %d (%s, layer %d): %s", entry, i, kKindName[o.kind], o.kind <= FTX_SPVCNN_OP_LINEAR_BN ? o.layer : -1, inner.c_str());
  return rc;
}

// Validates the program against the tables.  Host only.  Conditions are met in program order and the first one that fails gives
// the text, so their order is part of the contract; the training executor runs a backward over the same program and an empty level
// has no batch statistics, so it asks more (and in places something else) than the eval executor: every `train` below.  Each executor
// calls this once with a constant `train`; static, so that each gets its own copy with the other's branches folded away.
static inline int check_program(const SpvcnnTables &T, bool train, SlotFacts &F) {
  const char *who = train ? "ftx_spvcnn_train" : "ftx_spvcnn_eval";
  const Layer *layers = T.layers;
  const Op *ops = T.ops;
  const int64_t *rows = T.rows;
  const Map *maps = T.maps;
  const int32_t n_ops = T.n_ops;
  FTX_REQUIRE(ops && rows && T.routes && (!train || T.groutes) && n_ops >= 1 && n_ops <= kMaxOps, "%s: null table or op count outside [1, %d]", who, kMaxOps);
  FTX_REQUIRE(T.n_layers >= 0 && T.n_maps >= 0 && T.n_pvs >= 0 && (layers || !T.n_layers) && (maps || !T.n_maps) && (T.pvs || !T.n_pvs), "%s: null table", who);
  for (int l = 0; l < kLevels; ++l) {
    if (train)   // the eval executor sizes and runs an empty batch
      FTX_REQUIRE(rows[l] >= 1 && rows[l] < (1ll << 31), "%s: rows[%d] = %lld (the training BatchNorm needs at least one row on every level)", who, l,
                  (long long)rows[l]);
    else
      FTX_REQUIRE(rows[l] >= 0 && rows[l] < (1ll << 31), "%s: rows[%d] = %lld out of range", who, l, (long long)rows[l]);
  }
  for (int m = 0; m < T.n_maps; ++m)
    FTX_REQUIRE(maps[m].n_pairs >= 0 && maps[m].n_in >= 0 && maps[m].n_out >= 0 && maps[m].n_pairs < (1ll << 31), "%s: map %d has a negative or huge count", who, m);
  for (int s = 0; s < kMaxSlots; ++s) {
    F.level[s] = F.ch[s] = F.def[s] = -1;
    if (train) {
      F.galias[s] = -1;
      F.uses[s] = 0;
    }
  }
  F.op.assign(n_ops, {-1, {-1, -1}, 0});
  F.level[FTX_SPVCNN_SLOT_INPUT] = 0;   // the voxelised input features; channel count fixed by its first reader
  F.def[FTX_SPVCNN_SLOT_INPUT] = 0;
  int seg = 0;
  auto slot_ok = [](int s) { return s >= 0 && s < kMaxSlots; };
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    FTX_REQUIRE(o.kind >= FTX_SPVCNN_OP_CONV_BN && o.kind <= FTX_SPVCNN_OP_DROPOUT, "%s: op %d: unknown kind %d", who, i, o.kind);
    const char *kn = kKindName[o.kind];
    if (train)   // one autograd node per segment: any number of them, none skipped
      FTX_REQUIRE((o.segment == seg || o.segment == seg + 1) && o.segment < kMaxSegments && (i > 0 || o.segment == 0),
                  "%s: op %d (%s): segments are numbered from 0 without a gap, ascending, at most %d", who, i, kn, kMaxSegments);
    else
      FTX_REQUIRE(o.segment >= seg && o.segment <= 2, "%s: op %d (%s): segments must be 0..2 and ascending", who, i, kn);
    seg = o.segment;
    FTX_REQUIRE(slot_ok(o.src) && slot_ok(o.dst) && F.def[o.src] >= 0, "%s: op %d (%s): source slot %d is not written before it is read", who, i, kn, o.src);
    FTX_REQUIRE(o.level >= 0 && o.level < kLevels, "%s: op %d (%s): level %d", who, i, kn, o.level);
    FTX_REQUIRE(o.channels >= 4 && o.channels % 4 == 0 && o.channels <= 1024, "%s: op %d (%s): channel count %d is not a multiple of 4 in [4, 1024]", who, i,
                kn, o.channels);
    const int64_t n_dst = rows[o.level];
    auto need_src = [&](int s, int c) {      // the input slot takes the channel count of its first reader
      if (F.ch[s] < 0) F.ch[s] = c;
      return F.ch[s] == c;
    };
    int &second = F.op[i].second;
    int *grad_to = F.op[i].grad_to;          // the input features need no gradient
    switch (o.kind) {
      case FTX_SPVCNN_OP_CONV_BN:
      case FTX_SPVCNN_OP_LINEAR_BN: {
        FTX_REQUIRE(o.layer >= 0 && o.layer < T.n_layers, "%s: op %d (%s): layer %d out of range", who, i, kn, o.layer);
        const Layer &L = layers[o.layer];
        const bool conv = o.kind == FTX_SPVCNN_OP_CONV_BN;
        FTX_REQUIRE(L.kind == (conv ? FTX_SPVCNN_LAYER_CONV_BN : FTX_SPVCNN_LAYER_LINEAR_BN), "%s: op %d (%s): layer %d is of another kind", who, i, kn, o.layer);
        // train: the statistics kernels of the training BatchNorm take up to 512 channels
        FTX_REQUIRE(L.ca >= 4 && L.ca % 4 == 0 && L.co >= 4 && L.co % 4 == 0 && (!train || L.co <= 512),
                    "%s: op %d (%s) layer %d: channels must be multiples of 4 (ca=%d co=%d)", who, i, kn, o.layer, L.ca, L.co);
        FTX_REQUIRE(L.co == o.channels && need_src(o.src, L.ca), "%s: op %d (%s) layer %d: channel counts do not match the slots", who, i, kn, o.layer);
        FTX_REQUIRE(L.weight && L.gamma && L.beta && L.mean && L.var, "%s: op %d (%s) layer %d: null parameter", who, i, kn, o.layer);
        FTX_REQUIRE(L.bf16 >= 0 && L.bf16 <= 2, "%s: op %d (%s) layer %d: operand mode %d is not 0 (fp32), 1 (bf16) or 2 (split)", who, i, kn, o.layer, L.bf16);
        const int r = T.routes[i];
        F.op[i].temp_rows = n_dst;
        if (o.src != FTX_SPVCNN_SLOT_INPUT) grad_to[0] = o.src;
        if (!conv || L.kvol == 1) {
          FTX_REQUIRE(r == FTX_SPVCNN_ROUTE_ROWS, "%s: op %d (%s) layer %d: a dense layer takes the rows route, got %d", who, i, kn, o.layer, r);
          FTX_REQUIRE(L.ca <= 512 && L.co <= 512 && (conv ? L.stride == 1 && !L.transposed : L.kvol == 0), "%s: op %d (%s) layer %d: unsupported dense layer",
                      who, i, kn, o.layer);
          FTX_REQUIRE(F.level[o.src] == o.level, "%s: op %d (%s): a dense layer keeps its rows", who, i, kn);
        } else {
          FTX_REQUIRE(L.kvol == 8 || L.kvol == 27, "%s: op %d (%s) layer %d: kernel volume %d (1, 8 or 27)", who, i, kn, o.layer, L.kvol);
          FTX_REQUIRE(o.map >= 0 && o.map < T.n_maps && maps[o.map].kvol == L.kvol, "%s: op %d (%s) layer %d: kernel map %d missing or of another volume", who, i,
                      kn, o.layer, o.map);
          const Map &M = maps[o.map];
          const int64_t m_in = L.transposed ? M.n_out : M.n_in, m_out = L.transposed ? M.n_in : M.n_out;
          const int64_t n_src = rows[F.level[o.src]];
          FTX_REQUIRE(n_src == m_in && n_dst == m_out, "%s: op %d (%s) layer %d: kernel map %d is (%lld -> %lld), the slots hold (%lld -> %lld)", who, i, kn,
                      o.layer, o.map, (long long)m_in, (long long)m_out, (long long)n_src, (long long)n_dst);
          const MapSides side = map_sides(L, M);
          if (train) {   // whatever the route: the weight gradient reads both pair lists.  Eval asks per route for what that route reads
            FTX_REQUIRE(M.koff, "%s: op %d (%s): null offset table in map %d", who, i, kn, o.map);
            FTX_REQUIRE(!M.n_pairs || (M.pair_in && M.pair_out), "%s: op %d (%s): null pair list in map %d (the weight gradient reads both sides)", who, i, kn, o.map);
          }
          if (r == FTX_SPVCNN_ROUTE_DIRECT) {
            FTX_REQUIRE(M.fine_bijective && M.n_pairs == n_dst && L.transposed, "%s: op %d (%s) layer %d: the direct route needs a transposed layer on a "
                        "map whose pairs cover every output row once", who, i, kn, o.layer);
            if (!train) FTX_REQUIRE(!M.n_pairs || (M.pair_in && M.pair_out && M.koff), "%s: op %d (%s): null pair list in map %d", who, i, kn, o.map);
          } else if (r == FTX_SPVCNN_ROUTE_OSTAT) {
            // eval: the kernel needs a row on either side; train (no empty level): the route's statistics epilogue needs a pair
            // the kernel is exact fp32: that is mode 0, and it meets mode 2's fp32-class contract; a bf16 layer never takes it
            FTX_REQUIRE(L.bf16 != 1 && !L.transposed && ftx_spconv_ostat_supported(L.ca, L.co, L.kvol, 0) && n_dst <= kOstatMaxRows &&
                            (train ? M.n_pairs > 0 : n_dst >= 1 && m_in >= 1),
                        "%s: op %d (%s) layer %d: the output-stationary route does not take this layer", who, i, kn, o.layer);
            FTX_REQUIRE(M.nbr, "%s: op %d (%s): null neighbour table in map %d", who, i, kn, o.map);
          } else if (r == FTX_SPVCNN_ROUTE_PAIRS || r == FTX_SPVCNN_ROUTE_EMPTY) {
            if (train) {   // functional._conv_route gives the empty route to a map without pairs and to no other
              FTX_REQUIRE((r == FTX_SPVCNN_ROUTE_PAIRS) == (M.n_pairs > 0), "%s: op %d (%s) layer %d: the empty route is for a map without pairs, and only for it",
                          who, i, kn, o.layer);
              FTX_REQUIRE(side.dst_pos, "%s: op %d (%s): null position table in map %d", who, i, kn, o.map);
            } else {       // the pairs route also runs a map without pairs or rows; tables nothing will read may be null
              FTX_REQUIRE(r == FTX_SPVCNN_ROUTE_PAIRS || M.n_pairs == 0 || n_dst == 0, "%s: op %d (%s) layer %d: the empty route on a map with pairs", who, i, kn,
                          o.layer);
              FTX_REQUIRE(!n_dst || side.dst_pos, "%s: op %d (%s): null position table in map %d", who, i, kn, o.map);
              FTX_REQUIRE(!M.n_pairs || (side.gather && M.koff), "%s: op %d (%s): null pair list in map %d", who, i, kn, o.map);
              F.op[i].temp_rows = M.n_pairs;
            }
          } else {
            FTX_REQUIRE(false, "%s: op %d (%s) layer %d: route %d is not one this entry point takes", who, i, kn, o.layer, r);
          }
          if (train && grad_to[0] >= 0) {   // the data gradient: functional._conv_route(grad=True)
            const int gr = T.groutes[i];
            if (gr == FTX_SPVCNN_ROUTE_EMPTY)
              FTX_REQUIRE(M.n_pairs == 0, "%s: op %d (%s) layer %d: the empty gradient route on a map with pairs", who, i, kn, o.layer);
            else if (gr == FTX_SPVCNN_ROUTE_DIRECT)
              FTX_REQUIRE(M.fine_bijective && !L.transposed && M.n_pairs == n_src, "%s: op %d (%s) layer %d: the direct gradient route needs a strided layer on "
                          "a map whose pairs cover every input row once", who, i, kn, o.layer);
            else if (gr == FTX_SPVCNN_ROUTE_PAIRS)
              FTX_REQUIRE(M.n_pairs > 0 && side.src_pos, "%s: op %d (%s) layer %d: the pair-list gradient route needs pairs and the position "
                          "table of the input side", who, i, kn, o.layer);
            else
              FTX_REQUIRE(false, "%s: op %d (%s) layer %d: gradient route %d is not one this entry point takes", who, i, kn, o.layer, gr);
          }
        }
        if (conv && o.src2 >= 0) {   // train: the input features take no gradient
          FTX_REQUIRE(slot_ok(o.src2) && F.def[o.src2] >= 0 && F.level[o.src2] == o.level && need_src(o.src2, o.channels) &&
                          (!train || o.src2 != FTX_SPVCNN_SLOT_INPUT),
                      "%s: op %d (%s): the residual slot does not match the output", who, i, kn);
          second = grad_to[1] = o.src2;
        }
        break;
      }
      case FTX_SPVCNN_OP_VOXELIZE:
      case FTX_SPVCNN_OP_DEVOXELIZE: {
        const bool vox = o.kind == FTX_SPVCNN_OP_VOXELIZE;
        FTX_REQUIRE(o.map >= 0 && o.map < T.n_pvs, "%s: op %d (%s): point-voxel index %d out of range", who, i, kn, o.map);
        const PV &V = T.pvs[o.map];
        const int vlev = vox ? o.level : F.level[o.src], plev = vox ? F.level[o.src] : o.level;
        FTX_REQUIRE(plev == kLevels - 1 && vlev == V.level && V.level >= 0 && V.level < kLevels - 1 && rows[vlev] == V.n_vox,
                    "%s: op %d (%s): point-voxel index %d does not join these slots", who, i, kn, o.map);
        FTX_REQUIRE(need_src(o.src, o.channels) && (!train || o.src != FTX_SPVCNN_SLOT_INPUT), "%s: op %d (%s): channel counts differ", who, i, kn);
        if (train) {   // the backward of a voxelise reads the unsorted index; the forward takes the sorted segments where there are any
          if (vox)
            FTX_REQUIRE(V.vox_idx && V.vox_counts, "%s: op %d (%s): null voxel index in index %d (the backward reads it)", who, i, kn, o.map);
          else
            FTX_REQUIRE(V.devox_idx && V.devox_weights, "%s: op %d (%s): null corner table in index %d", who, i, kn, o.map);
        } else {       // the forward alone, on the sorted segments; tables of an empty side may be null
          if (vox)
            FTX_REQUIRE(!V.n_vox || (V.vox_seg_off && (V.vox_order || !rows[plev])), "%s: op %d (%s): null sorted segments in index %d", who, i, kn, o.map);
          else
            FTX_REQUIRE(!rows[plev] || (V.devox_idx && V.devox_weights), "%s: op %d (%s): null corner table in index %d", who, i, kn, o.map);
        }
        grad_to[0] = o.src;
        break;
      }
      case FTX_SPVCNN_OP_CONCAT:
      case FTX_SPVCNN_OP_ADD: {   // train: two gradients to two distinct arena slots
        FTX_REQUIRE(slot_ok(o.src2) && F.def[o.src2] >= 0 && F.level[o.src] == o.level && F.level[o.src2] == o.level &&
                        (!train || (o.src != o.src2 && o.src != FTX_SPVCNN_SLOT_INPUT && o.src2 != FTX_SPVCNN_SLOT_INPUT)),
                    "%s: op %d (%s): operands of different levels", who, i, kn);
        FTX_REQUIRE(F.ch[o.src] > 0 && F.ch[o.src2] > 0 && (o.kind == FTX_SPVCNN_OP_ADD ? (F.ch[o.src] == o.channels && F.ch[o.src2] == o.channels)
                                                                                         : F.ch[o.src] + F.ch[o.src2] == o.channels),
                    "%s: op %d (%s): channel counts do not add up", who, i, kn);
        second = o.src2;
        grad_to[0] = o.src;
        grad_to[1] = o.src2;
        break;
      }
      case FTX_SPVCNN_OP_ADD_EXT:
        FTX_REQUIRE(o.dst == o.src && (o.layer == 0 || o.layer == 1) && F.level[o.src] == o.level && F.ch[o.src] == o.channels && o.src >= FTX_SPVCNN_SLOT_FIRST,
                    "%s: op %d (%s): the fusion addend is added in place to an arena slot (layer = 0 early, 1 middle)", who, i, kn);
        if (train)
          FTX_REQUIRE(F.uses[o.src] == 0, "%s: op %d (%s): slot %d is read before the addend reaches it, and the backward would read it after", who, i, kn, o.src);
        break;
      case FTX_SPVCNN_OP_DROPOUT: {   // train only: in place like ADD_EXT; no gradient goes anywhere, the backward scales the slot's gradient in place
        FTX_REQUIRE(train, "%s: op %d (%s): the eval program has no Dropout (it is the identity in eval mode)", who, i, kn);
        FTX_REQUIRE(o.dst == o.src && o.layer >= 0 && F.level[o.src] == o.level && F.ch[o.src] == o.channels && o.src >= FTX_SPVCNN_SLOT_FIRST,
                    "%s: op %d (%s): Dropout works in place on an arena slot (layer = its site number >= 0)", who, i, kn);
        FTX_REQUIRE(F.uses[o.src] == 0, "%s: op %d (%s): slot %d is read before the Dropout reaches it, and the backward would read it after", who, i, kn, o.src);
        const float p = dropout_p(o);
        FTX_REQUIRE(p >= 0.0f && p < 1.0f, "%s: op %d (%s): p = %g outside [0, 1)", who, i, kn, (double)p);
        break;
      }
    }
    if (o.kind != FTX_SPVCNN_OP_ADD_EXT && o.kind != FTX_SPVCNN_OP_DROPOUT) {
      FTX_REQUIRE(o.dst != FTX_SPVCNN_SLOT_INPUT && F.def[o.dst] < 0, "%s: op %d (%s): slot %d is written twice", who, i, kn, o.dst);
      FTX_REQUIRE(o.dst != FTX_SPVCNN_SLOT_OUTPUT || o.level == kLevels - 1, "%s: op %d (%s): the output slot holds point rows", who, i, kn);
      if (train)
        FTX_REQUIRE(o.dst != FTX_SPVCNN_SLOT_OUTPUT || (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN),
                    "%s: op %d (%s): a layer may not write the output slot (its backward reads its result, which the backward is not given)", who, i, kn);
      F.def[o.dst] = i;
      F.level[o.dst] = o.level;
      F.ch[o.dst] = o.channels;
    }
    if (!train) continue;
    for (int k = 0; k < 2; ++k)
      if (grad_to[k] >= 0)
        FTX_REQUIRE(++F.uses[grad_to[k]] <= 2, "%s: op %d (%s): slot %d would receive more than two gradient contributions", who, i, kn, grad_to[k]);
    if (o.kind == FTX_SPVCNN_OP_ADD)   // both operands take the gradient of the sum as it is
      F.galias[o.src] = F.galias[o.src2] = o.dst;
  }
  if (!train) return FTX_OK;
  // the training program ends in the output slot, and every slot's gradient has one well-defined source
  F.n_segments = seg + 1;
  for (int i = 0; i < n_ops; ++i) F.out_slot[ops[i].segment] = ops[i].dst;
  for (int s = 0; s < F.n_segments; ++s) F.in_slot[s] = s ? F.out_slot[s - 1] : FTX_SPVCNN_SLOT_INPUT;
  FTX_REQUIRE(F.out_slot[F.n_segments - 1] == FTX_SPVCNN_SLOT_OUTPUT && F.def[FTX_SPVCNN_SLOT_OUTPUT] >= 0, "%s: the last op writes the output slot", who);
  for (int i = 0; i < n_ops; ++i) {   // the backward of a Dropout scales its slot's gradient buffer in place: that buffer is the slot's own, inside the arena
    const Op &o = ops[i];
    if (o.kind != FTX_SPVCNN_OP_DROPOUT) continue;
    FTX_REQUIRE(F.galias[o.src] < 0 && F.out_slot[o.segment] != o.src, "%s: op %d (dropout): slot %d is an operand of an add or the result of its segment: "
                "its gradient is another buffer's", who, i, o.src);
  }
  for (int s = FTX_SPVCNN_SLOT_OUTPUT; s < kMaxSlots; ++s) {
    if (F.def[s] < 0) continue;
    if (F.galias[s] >= 0) FTX_REQUIRE(F.uses[s] == 1, "%s: slot %d is an operand of an add and of another op: its gradient would need a copy", who, s);
    FTX_REQUIRE(F.uses[s] >= 1 || s == FTX_SPVCNN_SLOT_OUTPUT, "%s: slot %d is never read: its producer would take an undefined gradient", who, s);
    FTX_REQUIRE(s != FTX_SPVCNN_SLOT_OUTPUT || F.uses[s] == 0, "%s: the output slot is read inside the program", who);
  }
  return FTX_OK;
}

}  // namespace ftx
