// Native training executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_train_fwd / _bwd).  Where the Python path slices a
// gradient its backward issues ftx_rows_split (ftx_rows.hip, the backward of ftx_rows_concat).
//
// The program, the model table and the batch tables are the eval executor's (ftx_exec.hip), and one checker validates them for both
// (ftx_spvcnn_program.h: check_program, which also says where this executor asks more of a program); the forward issues the train-mode form of
// every op and the backward walks the same program in reverse, issuing for every op what its autograd node issues on the Python path
// (functional._ConvBNTrain, _BatchNormTrain, _RowsLinear, _RowsMatmul, _Voxelize, _Devoxelize) through the library's own per-op entry
// points.  Everything the backward reads stays in the caller's arena: no buffer is shared between two slots, so nothing is
// overwritten while a run is alive.  No state outlives a call; nothing here synchronises or allocates.
#include <vector>
#include "ftx_spvcnn_program.h"

using namespace ftx;

// ---------------------------------------------------------------- plan
namespace {

using TrainLayer = ftx::SpvcnnTrainLayer;
using TrainPV = ftx::SpvcnnTrainPV;

// Workspace of the weight gradient over n pairs.  The library's own size follows its tile length (>= 256 pairs) and is not monotone in
// n; this bound on it is: a tile per 256 pairs plus one per offset.
inline int64_t wgrad_ws_bytes(int64_t n_pairs, int ca, int cg, int kvol) { return 4 * (ceil_div(n_pairs, 256) + kvol) * (int64_t)ca * cg; }

// Where everything lies in the arena, and which contribution to a slot's gradient arrives first.
struct Plan {
  int first_op[kMaxSlots], first_operand[kMaxSlots], read_lo[kMaxSlots], read_hi[kMaxSlots];   // per slot
  int64_t f_off[kMaxSlots], g_off[kMaxSlots];                                                  // per slot: forward buffer, gradient buffer
  std::vector<int64_t> x_off, stats_off;                                                       // per op: convolution / GEMM output, (mean, invstd)
  int64_t temp_off = 0, temp_bytes = 0, total = 0;
};

// the temporaries of one op: consecutive 256-byte aligned pieces of the shared region (base 0: sizes only)
struct Carve {
  uintptr_t base = 0;
  int64_t off = 0;
  void *take(int64_t bytes) {
    void *p = (void *)(base + (uintptr_t)off);
    off += align256(bytes);
    return p;
  }
};

struct Exec {
  const SpvcnnTables T;
  const SlotFacts &S;
  const Plan &P;
  const TrainLayer *tlayers = nullptr;
  uintptr_t base = 0;
  const float *seg_in = nullptr;
  int in_slot = -1;
  void *stream = nullptr;
  bool launch = false;      // false: carve only (the size query)
  // the forward's
  const float *add[2] = {nullptr, nullptr};
  float *out = nullptr;
  // the backward's
  const TrainPV *tpvs = nullptr;
  const float *grad_out = nullptr;
  int gout_slot = -1;
  // the _rng entries': the random stream of the program's DROPOUT ops (site s draws call_base + s)
  uint64_t seed = 0, call_base = 0;

  float *F(int s) const {
    if (s == in_slot) return const_cast<float *>(seg_in);
    if (s == FTX_SPVCNN_SLOT_OUTPUT) return out;
    return (float *)(base + (uintptr_t)P.f_off[s]);
  }
  int gslot(int s) const {
    while (S.galias[s] >= 0) s = S.galias[s];
    return s;
  }
  float *G(int s) const {
    s = gslot(s);
    if (s == gout_slot) return const_cast<float *>(grad_out);
    return (float *)(base + (uintptr_t)P.g_off[s]);
  }
  int64_t slot_bytes(int s) const { return 4 * T.rows[S.level[s]] * (int64_t)S.ch[s]; }

  // where operand `operand` of op i writes its gradient contribution to slot s: the slot's gradient buffer when it is the first one to
  // arrive (the slot's last reader), else a temporary that `commit` adds to it
  struct Target {
    float *ptr, *sum;
  };
  Target target(int i, int operand, int s, Carve &cv) const {
    if (P.first_op[s] == i && P.first_operand[s] == operand) return {launch ? G(s) : nullptr, nullptr};
    float *t = (float *)cv.take(slot_bytes(s));
    return {t, launch ? G(s) : nullptr};
  }
  int commit(const Target &t, int s) const {
    if (!t.sum || !launch) return FTX_OK;
    return ftx_rows_add(t.sum, t.ptr, T.rows[S.level[s]], S.ch[s], t.sum, stream);
  }

  int fwd_op(int i, Carve &cv) const;
  int bwd_op(int i, Carve &cv) const;
};

#define RUN(call)                  \
  do {                             \
    if (launch) {                  \
      const int rc_ = (call);      \
      if (rc_ != FTX_OK) return rc_; \
    }                              \
  } while (0)

int Exec::fwd_op(int i, Carve &cv) const {
  const Op &o = T.ops[i];
  const int64_t n = T.rows[o.level];
  switch (o.kind) {
    case FTX_SPVCNN_OP_CONV_BN:
    case FTX_SPVCNN_OP_LINEAR_BN: {
      const Layer &L = T.layers[o.layer];
      const SpconvEntries E = spconv_entries(L);
      const bool linear = o.kind == FTX_SPVCNN_OP_LINEAR_BN;
      const float momentum = launch ? tlayers[o.layer].momentum : 0.f;
      float *x = (float *)(base + (uintptr_t)P.x_off[i]);
      float *mean = (float *)(base + (uintptr_t)P.stats_off[i]), *invstd = mean + L.co;
      float *rm = const_cast<float *>(L.mean), *rv = const_cast<float *>(L.var);
      const float *src = launch ? F(o.src) : nullptr;
      const float *res = (launch && !linear && o.src2 >= 0) ? F(o.src2) : nullptr;
      float *y = launch ? F(o.dst) : nullptr;
      const int r = T.routes[i];
      const int64_t bn_ws_bytes = (int64_t)ftx_bn_workspace_bytes(n, L.co);
      if (r == FTX_SPVCNN_ROUTE_ROWS) {
        void *ws = cv.take(bn_ws_bytes);
        RUN(E.rows(src, n, L.weight, linear ? 1 : 0, linear ? L.bias : nullptr, L.ca, L.co, x, stream));
        RUN(ftx_bn_train_fwd(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, ws, (size_t)bn_ws_bytes, stream));
        break;
      }
      const Map &M = T.maps[o.map];
      const int64_t rows_a = T.rows[S.level[o.src]];
      const MapSides side = map_sides(L, M);
      if (r == FTX_SPVCNN_ROUTE_OSTAT || r == FTX_SPVCNN_ROUTE_PAIRS) {
        // the convolution leaves the statistics (nb partial rows + the totals row, float64), then the one apply pass
        const int32_t nb = r == FTX_SPVCNN_ROUTE_OSTAT ? ftx_spconv_ostat_blocks(n) : ftx_spconv_reduce_stats_blocks(n, L.co);
        float *tmp = (float *)cv.take(r == FTX_SPVCNN_ROUTE_PAIRS ? 4 * M.n_pairs * (int64_t)L.co : 0);
        double *part = (double *)cv.take(16 * ((int64_t)nb + 1) * L.co);
        const double *totals = part + (int64_t)nb * 2 * L.co;
        if (r == FTX_SPVCNN_ROUTE_OSTAT) {
          RUN(ftx_spconv_ostat(src, rows_a, M.nbr, n, L.weight, 0, 0, L.ca, L.co, L.kvol, x, part, nb, stream));
        } else {
          RUN(E.pairs(src, rows_a, side.gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce_stats(tmp, side.dst_pos, n, L.co, L.kvol, x, part, nb, stream));
        }
        RUN(ftx_bn_train_fwd_totals(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, totals, stream));
      } else {
        // scatter epilogue or empty map: the plain convolution, then the BatchNorm's own statistics pass
        float *tmp = (float *)cv.take(r == FTX_SPVCNN_ROUTE_EMPTY ? 4 * M.n_pairs * (int64_t)L.co : 0);
        void *ws = cv.take(bn_ws_bytes);
        if (r == FTX_SPVCNN_ROUTE_DIRECT) {
          RUN(E.scatter(src, rows_a, side.gather, side.scatter, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, x, n, stream));
        } else {
          RUN(E.pairs(src, rows_a, side.gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce(tmp, side.dst_pos, n, L.co, L.kvol, x, stream));
        }
        RUN(ftx_bn_train_fwd(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, ws, (size_t)bn_ws_bytes, stream));
      }
      break;
    }
    case FTX_SPVCNN_OP_VOXELIZE: {
      if (!launch) break;
      const PV &V = T.pvs[o.map];
      if (V.vox_order && V.vox_seg_off)
        RUN(ftx_voxelize_fwd_sorted(F(o.src), V.vox_order, V.vox_seg_off, T.rows[kLevels - 1], o.channels, n, F(o.dst), stream));
      else
        RUN(ftx_voxelize_fwd(F(o.src), V.vox_idx, V.vox_counts, T.rows[kLevels - 1], o.channels, n, F(o.dst), stream));
      break;
    }
    case FTX_SPVCNN_OP_DEVOXELIZE: {
      if (!launch) break;
      const PV &V = T.pvs[o.map];
      RUN(ftx_devoxelize_fwd(F(o.src), V.devox_idx, V.devox_weights, n, o.channels, V.n_vox, F(o.dst), stream));
      break;
    }
    case FTX_SPVCNN_OP_CONCAT:
      if (launch) RUN(ftx_rows_concat(F(o.src), S.ch[o.src], F(o.src2), S.ch[o.src2], n, F(o.dst), stream));
      break;
    case FTX_SPVCNN_OP_ADD:
      if (launch) RUN(ftx_rows_add(F(o.src), F(o.src2), n, o.channels, F(o.dst), stream));
      break;
    case FTX_SPVCNN_OP_ADD_EXT:
      if (launch && add[o.layer]) RUN(ftx_rows_add(F(o.src), add[o.layer], n, o.channels, F(o.dst), stream));
      break;
    case FTX_SPVCNN_OP_DROPOUT:
      if (launch) RUN(ftx_dropout(F(o.src), n * o.channels, dropout_p(o), seed, call_base + (uint64_t)o.layer, 0, F(o.dst), stream));
      break;
  }
  return FTX_OK;
}

// What the op's autograd node issues on the Python path, in that node's order.
int Exec::bwd_op(int i, Carve &cv) const {
  const Op &o = T.ops[i];
  const int64_t n = T.rows[o.level];
  const float *gy = launch ? G(o.dst) : nullptr;
  switch (o.kind) {
    case FTX_SPVCNN_OP_CONV_BN:
    case FTX_SPVCNN_OP_LINEAR_BN: {
      const Layer &L = T.layers[o.layer];
      const SpconvEntries E = spconv_entries(L);
      const bool linear = o.kind == FTX_SPVCNN_OP_LINEAR_BN;
      const bool has_res = !linear && o.src2 >= 0;
      const bool need_data = o.src != FTX_SPVCNN_SLOT_INPUT;
      const int64_t n_src = T.rows[S.level[o.src]];
      TrainLayer TL = {nullptr, nullptr, nullptr, nullptr, 0.f, 0};
      if (launch) TL = tlayers[o.layer];
      const float *x = (const float *)(base + (uintptr_t)P.x_off[i]);
      const float *mean = (const float *)(base + (uintptr_t)P.stats_off[i]), *invstd = mean + L.co;
      const float *src = launch ? F(o.src) : nullptr;
      const float *y = launch ? F(o.dst) : nullptr;
      // BatchNorm half: gx = d loss / d (convolution output) is a temporary, consumed by the calls below
      const int64_t bn_ws_bytes = (int64_t)ftx_bn_workspace_bytes(n, L.co);
      void *bn_ws = cv.take(bn_ws_bytes);
      float *gx = (float *)cv.take(4 * n * (int64_t)L.co);
      Target tres = {nullptr, nullptr};
      if (has_res) tres = target(i, 1, o.src2, cv);
      RUN(ftx_bn_train_bwd(gy, x, y, L.gamma, L.beta, mean, invstd, n, L.co, o.relu, gx, tres.ptr, TL.dgamma, TL.dbeta, bn_ws, (size_t)bn_ws_bytes, stream));
      if (has_res) RUN(commit(tres, o.src2));
      Target tsrc = {nullptr, nullptr};
      if (need_data) tsrc = target(i, 0, o.src, cv);
      if (T.routes[i] == FTX_SPVCNN_ROUTE_ROWS) {
        void *wg_ws = cv.take(wgrad_ws_bytes(n, L.ca, L.co, 1));
        const size_t wg_bytes = (size_t)wgrad_ws_bytes(n, L.ca, L.co, 1);
        if (linear) {   // weight (co, ca): gx @ W, dW = gx^T x, dbias = column sums of gx
          if (need_data) RUN(E.rows(gx, n, L.weight, 0, nullptr, L.co, L.ca, tsrc.ptr, stream));
          RUN(E.wgrad(gx, n, nullptr, src, n, nullptr, nullptr, n, L.co, L.ca, 1, TL.dweight, wg_ws, wg_bytes, stream));
          if (L.bias) {
            const int64_t cs_bytes = (int64_t)ftx_colsum_workspace_bytes(n, L.co);
            void *cs_ws = cv.take(cs_bytes);
            RUN(ftx_colsum(gx, n, L.co, TL.dbias, cs_ws, (size_t)cs_bytes, stream));
          }
        } else {        // kernel (ca, co): gx @ W^T, dW = x^T gx
          if (need_data) RUN(E.rows(gx, n, L.weight, 1, nullptr, L.co, L.ca, tsrc.ptr, stream));
          RUN(E.wgrad(src, n, nullptr, gx, n, nullptr, nullptr, n, L.ca, L.co, 1, TL.dweight, wg_ws, wg_bytes, stream));
        }
      } else {
        const Map &M = T.maps[o.map];
        const MapSides side = map_sides(L, M);
        const int gr = need_data ? T.groutes[i] : -1;
        float *tmp = (float *)cv.take(gr == FTX_SPVCNN_ROUTE_PAIRS ? 4 * M.n_pairs * (int64_t)L.ca : 0);
        const int64_t wg_bytes = wgrad_ws_bytes(M.n_pairs, L.ca, L.co, L.kvol);
        void *wg_ws = cv.take(wg_bytes);
        if (gr == FTX_SPVCNN_ROUTE_EMPTY) {
          if (launch && n_src > 0 && hipMemsetAsync(tsrc.ptr, 0, sizeof(float) * n_src * L.ca, (hipStream_t)stream) != hipSuccess)
            return check_launch("ftx_spvcnn_train_bwd memset");
        } else if (gr == FTX_SPVCNN_ROUTE_DIRECT) {
          RUN(E.scatter(gx, n, side.scatter, side.gather, L.weight, 1, M.koff, M.n_pairs, L.co, L.ca, L.kvol, tsrc.ptr, n_src,
                        stream));
        } else if (gr == FTX_SPVCNN_ROUTE_PAIRS) {
          RUN(E.pairs(gx, n, side.scatter, L.weight, 1, M.koff, M.n_pairs, L.co, L.ca, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce(tmp, side.src_pos, n_src, L.ca, L.kvol, tsrc.ptr, stream));
        }
        RUN(E.wgrad(src, n_src, side.gather, gx, n, side.scatter, M.koff, M.n_pairs, L.ca, L.co, L.kvol, TL.dweight, wg_ws, (size_t)wg_bytes,
                    stream));
      }
      if (need_data) RUN(commit(tsrc, o.src));
      break;
    }
    case FTX_SPVCNN_OP_VOXELIZE: {
      const Target t = target(i, 0, o.src, cv);
      if (!launch) break;
      const PV &V = T.pvs[o.map];
      RUN(ftx_voxelize_bwd(gy, V.vox_idx, V.vox_counts, T.rows[kLevels - 1], o.channels, n, t.ptr, stream));
      RUN(commit(t, o.src));
      break;
    }
    case FTX_SPVCNN_OP_DEVOXELIZE: {
      const Target t = target(i, 0, o.src, cv);
      if (!launch) break;
      const PV &V = T.pvs[o.map];
      const TrainPV &TV = tpvs[o.map];
      if (TV.devox_order && TV.devox_seg_off)
        RUN(ftx_devoxelize_bwd_sorted(gy, V.devox_weights, TV.devox_order, TV.devox_seg_off, n, o.channels, V.n_vox, t.ptr, stream));
      else
        RUN(ftx_devoxelize_bwd(gy, V.devox_idx, V.devox_weights, n, o.channels, V.n_vox, t.ptr, stream));
      RUN(commit(t, o.src));
      break;
    }
    case FTX_SPVCNN_OP_CONCAT: {
      const Target ta = target(i, 0, o.src, cv), tb = target(i, 1, o.src2, cv);
      RUN(ftx_rows_split(gy, n, S.ch[o.src], S.ch[o.src2], ta.ptr, tb.ptr, stream));
      RUN(commit(ta, o.src));
      RUN(commit(tb, o.src2));
      break;
    }
    case FTX_SPVCNN_OP_ADD:       // both operands take the gradient of the sum as it is: their gradient buffers ARE the sum's
    case FTX_SPVCNN_OP_ADD_EXT:   // in place: the slot's gradient is also the addend's
      break;
    case FTX_SPVCNN_OP_DROPOUT: {   // the same mask, recomputed, on the slot's gradient in place (check_program: the buffer is the slot's own)
      float *g = launch ? G(o.src) : nullptr;
      RUN(ftx_dropout(g, n * o.channels, dropout_p(o), seed, call_base + (uint64_t)o.layer, 0, g, stream));
      break;
    }
  }
  return FTX_OK;
}
#undef RUN

// Validates the program against the tables (check_program) and places every buffer.  Host only.
int make_plan(const SpvcnnTables &T, SlotFacts &F, Plan &P) {
  const int rc = check_program(T, true, F);
  if (rc != FTX_OK) return rc;
  const Op *ops = T.ops;
  const int n_ops = T.n_ops;
  for (int s = 0; s < kMaxSlots; ++s) {
    P.first_op[s] = P.first_operand[s] = P.read_lo[s] = P.read_hi[s] = -1;
    P.f_off[s] = P.g_off[s] = -1;
  }
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    for (int k = 0; k < 2; ++k) {
      const int s = F.op[i].grad_to[k];
      if (s < 0) continue;
      P.first_op[s] = i;       // the last reader in program order is the first to contribute in the backward
      P.first_operand[s] = k;
    }
    for (int s : {o.src, F.op[i].second}) {
      if (s < 0) continue;
      if (P.read_lo[s] < 0) P.read_lo[s] = o.segment;
      P.read_hi[s] = o.segment;
    }
  }
  // placement: one region per slot, per slot gradient, per layer output and statistics -- nothing is shared, so nothing the backward
  // reads has a later writer -- then the shared region of the per-op temporaries
  int64_t off = 0;
  for (int s = FTX_SPVCNN_SLOT_FIRST; s < kMaxSlots; ++s) {
    if (F.def[s] < 0) continue;
    const int64_t b = align256(4 * T.rows[F.level[s]] * (int64_t)F.ch[s]);
    P.f_off[s] = off;
    off += b;
    if (F.galias[s] < 0) {
      P.g_off[s] = off;
      off += b;
    }
  }
  P.x_off.assign(n_ops, -1);
  P.stats_off.assign(n_ops, -1);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    if (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN) continue;
    P.x_off[i] = off;
    off += align256(4 * T.rows[o.level] * (int64_t)o.channels);
    P.stats_off[i] = off;
    off += align256(8 * (int64_t)o.channels);
  }
  P.temp_off = off;
  const Exec E{T, F, P};   // carve only
  for (int i = 0; i < n_ops; ++i) {
    Carve f, b;
    (void)E.fwd_op(i, f);
    (void)E.bwd_op(i, b);
    if (f.off > P.temp_bytes) P.temp_bytes = f.off;
    if (b.off > P.temp_bytes) P.temp_bytes = b.off;
  }
  P.total = off + P.temp_bytes;
  if (P.total < 256) P.total = 256;
  return FTX_OK;
}

// what both directions check after the plan: the segment range, the arena, the buffer that stands for the first segment's input
int check_call(const char *entry, const SpvcnnTables &T, const SlotFacts &F, const Plan &P, int32_t first, int32_t last, const void *seg_in, const void *arena,
               size_t arena_bytes) {
  FTX_REQUIRE(first >= 0 && first <= last && last < F.n_segments, "%s: segments [%d, %d] outside 0..%d", entry, first, last, F.n_segments - 1);
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "%s: the arena must be a 256-byte aligned device buffer", entry);
  if (arena_bytes < (size_t)P.total) {
    set_error("%s: arena %zu < required %zu (ftx_spvcnn_train_arena_bytes)", entry, arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  const int in = F.in_slot[first];
  FTX_REQUIRE(seg_in, "%s: null input of segment %d", entry, first);
  FTX_REQUIRE(((uintptr_t)seg_in & 15) == 0, "%s: the input of segment %d must be 16-byte aligned", entry, first);
  if (in >= FTX_SPVCNN_SLOT_FIRST && (P.read_lo[in] != first || P.read_hi[in] != first))
    FTX_REQUIRE((const char *)seg_in == (const char *)arena + P.f_off[in], "%s: the input of segment %d is also read by another segment: it must be the buffer "
                "the previous segment returned", entry, first);
  for (int i = 0; i < T.n_ops; ++i) {   // a segment other than the first reads the input features or another segment's replaced input
    const Op &o = T.ops[i];
    if (o.segment < first || o.segment > last) continue;
    FTX_REQUIRE(first == 0 || (o.src != FTX_SPVCNN_SLOT_INPUT && o.src2 != FTX_SPVCNN_SLOT_INPUT), "%s: op %d reads the input features outside segment 0", entry, i);
  }
  return FTX_OK;
}

}  // namespace

extern "C" int32_t ftx_spvcnn_train_layer_bytes(void) { return (int32_t)sizeof(TrainLayer); }
extern "C" int32_t ftx_spvcnn_train_pv_bytes(void) { return (int32_t)sizeof(TrainPV); }

extern "C" size_t ftx_spvcnn_train_arena_bytes(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host,
                                               const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host,
                                               const int32_t *grad_routes_host) {
  SlotFacts F;
  Plan P;
  if (make_plan(spvcnn_tables(layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs, routes_host, grad_routes_host), F, P) != FTX_OK)
    return 0;
  return (size_t)P.total;
}

namespace {

// The plain entries have no random stream: they refuse a program with a DROPOUT op, before the first launch.
int check_rng(const char *entry, const SpvcnnTables &T, bool rng) {
  for (int i = 0; i < T.n_ops && !rng; ++i)
    FTX_REQUIRE(T.ops[i].kind != FTX_SPVCNN_OP_DROPOUT, "%s: op %d is a Dropout, which draws from the random stream: call %s_rng with (seed, call_base)", entry, i,
                entry);
  return FTX_OK;
}

int train_fwd(const char *entry, bool rng, uint64_t seed, uint64_t call_base, const void *layers_host, const void *train_layers_host, int32_t n_layers,
              const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs,
              const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment, const float *seg_in,
              const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out, float **seg_out, void *stream) {
  const SpvcnnTables T = spvcnn_tables(layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs, routes_host, grad_routes_host);
  SlotFacts F;
  Plan P;
  int rc = make_plan(T, F, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(train_layers_host || !n_layers, "%s: null train table", entry);
  rc = check_rng(entry, T, rng);
  if (rc != FTX_OK) return rc;
  rc = check_call(entry, T, F, P, first_segment, last_segment, seg_in, arena, arena_bytes);
  if (rc != FTX_OK) return rc;
  const int out_slot = F.out_slot[last_segment];
  FTX_REQUIRE(out_slot != FTX_SPVCNN_SLOT_OUTPUT || out, "%s: null output", entry);
  Exec E{T, F, P, (const TrainLayer *)train_layers_host, (uintptr_t)arena, seg_in, F.in_slot[first_segment], stream, true};
  E.add[0] = add_early;
  E.add[1] = add_middle;
  E.out = out;
  E.seed = seed;
  E.call_base = call_base;
  // everything above answered on the host; from here on launches only
  for (int i = 0; i < n_ops; ++i) {
    if (T.ops[i].segment < first_segment || T.ops[i].segment > last_segment) continue;
    Carve cv;
    cv.base = E.base + (uintptr_t)P.temp_off;
    rc = E.fwd_op(i, cv);
    if (rc != FTX_OK) return fail(entry, i, T.ops[i], rc);
  }
  if (seg_out) *seg_out = E.F(out_slot);
  return FTX_OK;
}

int train_bwd(const char *entry, bool rng, uint64_t seed, uint64_t call_base, const void *layers_host, const void *train_layers_host, int32_t n_layers,
              const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host,
              const void *train_pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment,
              int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in, void *stream) {
  const SpvcnnTables T = spvcnn_tables(layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs, routes_host, grad_routes_host);
  const TrainLayer *tl = (const TrainLayer *)train_layers_host;
  SlotFacts F;
  Plan P;
  int rc = make_plan(T, F, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE((tl || !n_layers) && (train_pvs_host || !n_pvs), "%s: null train table", entry);
  rc = check_rng(entry, T, rng);
  if (rc != FTX_OK) return rc;
  rc = check_call(entry, T, F, P, first_segment, last_segment, seg_in, arena, arena_bytes);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(grad_out && ((uintptr_t)grad_out & 15) == 0, "%s: null or misaligned output gradient", entry);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = T.ops[i];
    if (o.segment < first_segment || o.segment > last_segment || (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN)) continue;
    const TrainLayer &G = tl[o.layer];
    FTX_REQUIRE(G.dweight && G.dgamma && G.dbeta && (G.dbias || !T.layers[o.layer].bias), "%s: op %d, layer %d: null gradient destination", entry, i, o.layer);
  }
  Exec E{T, F, P, tl, (uintptr_t)arena, seg_in, F.in_slot[first_segment], stream, true};
  E.tpvs = (const TrainPV *)train_pvs_host;
  E.grad_out = grad_out;
  E.gout_slot = F.out_slot[last_segment];
  E.seed = seed;
  E.call_base = call_base;
  for (int i = n_ops - 1; i >= 0; --i) {
    if (T.ops[i].segment < first_segment || T.ops[i].segment > last_segment) continue;
    Carve cv;
    cv.base = E.base + (uintptr_t)P.temp_off;
    rc = E.bwd_op(i, cv);
    if (rc != FTX_OK) return fail(entry, i, T.ops[i], rc);
  }
  if (grad_in) *grad_in = first_segment ? E.G(E.in_slot) : nullptr;
  return FTX_OK;
}

}  // namespace

extern "C" int ftx_spvcnn_train_fwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                    const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs,
                                    const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment,
                                    const float *seg_in, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out,
                                    float **seg_out, void *stream) {
  return train_fwd("ftx_spvcnn_train_fwd", false, 0, 0, layers_host, train_layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs,
                   routes_host, grad_routes_host, first_segment, last_segment, seg_in, add_early, add_middle, arena, arena_bytes, out, seg_out, stream);
}

extern "C" int ftx_spvcnn_train_fwd_rng(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                        const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs,
                                        const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment,
                                        const float *seg_in, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out,
                                        float **seg_out, void *stream, uint64_t seed, uint64_t call_base) {
  return train_fwd("ftx_spvcnn_train_fwd_rng", true, seed, call_base, layers_host, train_layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps,
                   pvs_host, n_pvs, routes_host, grad_routes_host, first_segment, last_segment, seg_in, add_early, add_middle, arena, arena_bytes, out, seg_out,
                   stream);
}

extern "C" int ftx_spvcnn_train_bwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                    const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, const void *train_pvs_host,
                                    int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment,
                                    int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in,
                                    void *stream) {
  return train_bwd("ftx_spvcnn_train_bwd", false, 0, 0, layers_host, train_layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host,
                   train_pvs_host, n_pvs, routes_host, grad_routes_host, first_segment, last_segment, seg_in, grad_out, arena, arena_bytes, grad_in, stream);
}

extern "C" int ftx_spvcnn_train_bwd_rng(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                        const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, const void *train_pvs_host,
                                        int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment,
                                        int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in,
                                        void *stream, uint64_t seed, uint64_t call_base) {
  return train_bwd("ftx_spvcnn_train_bwd_rng", true, seed, call_base, layers_host, train_layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps,
                   pvs_host, train_pvs_host, n_pvs, routes_host, grad_routes_host, first_segment, last_segment, seg_in, grad_out, arena, arena_bytes, grad_in,
                   stream);
}
