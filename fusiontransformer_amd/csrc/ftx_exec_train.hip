// Native training executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_train_fwd / _bwd) and the row kernel its backward
// needs where the Python path slices a gradient (ftx_rows_split, the backward of ftx_rows_concat).
//
// The program, the model table and the batch tables are the eval executor's (ftx_exec.hip); the forward issues the train-mode form of
// every op and the backward walks the same program in reverse, issuing for every op what its autograd node issues on the Python path
// (functional._ConvBNTrain, _BatchNormTrain, _RowsLinear, _RowsMatmul, _Voxelize, _Devoxelize) through the library's own per-op entry
// points.  Everything the backward reads stays in the caller's arena: no buffer is shared between two slots, so nothing is
// overwritten while a run is alive.  No state outlives a call; nothing here synchronises or allocates.
#include <string>
#include <vector>
#include "ftx_common.h"
#include "ftx_spvcnn_tables.h"

using namespace ftx;

// ---------------------------------------------------------------- row kernel
// a[r], b[r] = in[r][:ca], in[r][ca:] (the backward of the channel concatenation); ca, cb multiples of 4, 16-byte accesses
__global__ void rows_split_kernel(const float *__restrict__ in, int64_t n, int ca, int cb, float *__restrict__ a, float *__restrict__ b) {
  const int cv = (ca + cb) >> 2, av = ca >> 2;
  const int64_t total = n * cv;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cv;
    const int j = (int)(e - r * cv);
    const float4 v = *(const float4 *)&in[e * 4];
    if (j < av)
      *(float4 *)&a[r * ca + 4 * j] = v;
    else
      *(float4 *)&b[r * cb + 4 * (j - av)] = v;
  }
}

extern "C" int ftx_rows_split(const float *in, int64_t n, int32_t ca, int32_t cb, float *a, float *b, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_rows_split: n < 0");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && cb >= 4 && cb % 4 == 0, "ftx_rows_split: channels must be multiples of 4 (ca=%d cb=%d)", ca, cb);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(in && a && b, "ftx_rows_split: null pointer");
  FTX_REQUIRE((((uintptr_t)in | (uintptr_t)a | (uintptr_t)b) & 15) == 0, "ftx_rows_split: pointers must be 16-byte aligned");
  rows_split_kernel<<<grid_for(n * ((ca + cb) / 4), 256), 256, 0, (hipStream_t)stream>>>(in, n, ca, cb, a, b);
  return check_launch("ftx_rows_split");
}

// ---------------------------------------------------------------- plan
namespace {

using Layer = ftx::SpvcnnLayer;
using Op = ftx::SpvcnnOp;
using Map = ftx::SpvcnnMap;
using PV = ftx::SpvcnnPV;
using TrainLayer = ftx::SpvcnnTrainLayer;
using TrainPV = ftx::SpvcnnTrainPV;

constexpr int kLevels = 6;        // five voxel levels + the point set
constexpr int kMaxSlots = 256;
constexpr int kMaxOps = 4096;
constexpr int kMaxSegments = 8;
constexpr int64_t kOstatMaxRows = 64 * 4096;
const char *const kKindName[] = {"?", "conv_bn", "linear_bn", "voxelize", "devoxelize", "concat", "add", "add_ext"};
const char *const kWho = "ftx_spvcnn_train";

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Workspace of the weight gradient over n pairs.  The library's own size follows its tile length (>= 256 pairs) and is not monotone in
// n; this bound on it is: a tile per 256 pairs plus one per offset.
inline int64_t wgrad_ws_bytes(int64_t n_pairs, int ca, int cg, int kvol) { return 4 * (ceil_div(n_pairs, 256) + kvol) * (int64_t)ca * cg; }

struct Plan {
  int n_segments = 0;
  std::vector<int> level, ch, def, uses, first_op, first_operand, galias, read_lo, read_hi;   // per slot
  std::vector<int> in_slot, out_slot;                                                          // per segment
  std::vector<int64_t> f_off, g_off;                                                           // per slot: forward buffer, gradient buffer
  std::vector<int64_t> x_off, stats_off;                                                       // per op: convolution / GEMM output, (mean, invstd)
  int64_t temp_off = 0, temp_bytes = 0, total = 0;
};

#define PLAN_REQUIRE(cond, ...)        \
  do {                                 \
    if (!(cond)) {                     \
      set_error(__VA_ARGS__);          \
      return FTX_EINVAL;               \
    }                                  \
  } while (0)

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
  const Layer *layers = nullptr;
  const TrainLayer *tlayers = nullptr;
  const Op *ops = nullptr;
  const int64_t *rows = nullptr;
  const Map *maps = nullptr;
  const PV *pvs = nullptr;
  const TrainPV *tpvs = nullptr;
  const int32_t *routes = nullptr, *groutes = nullptr;
  const Plan *P = nullptr;
  uintptr_t base = 0;
  const float *seg_in = nullptr;
  int in_slot = -1;
  const float *add[2] = {nullptr, nullptr};
  float *out = nullptr;
  const float *grad_out = nullptr;
  int gout_slot = -1;
  void *stream = nullptr;
  bool launch = false;      // false: carve only (the size query)

  float *F(int s) const {
    if (s == in_slot) return const_cast<float *>(seg_in);
    if (s == FTX_SPVCNN_SLOT_OUTPUT) return out;
    return (float *)(base + (uintptr_t)P->f_off[s]);
  }
  int gslot(int s) const {
    while (P->galias[s] >= 0) s = P->galias[s];
    return s;
  }
  float *G(int s) const {
    s = gslot(s);
    if (s == gout_slot) return const_cast<float *>(grad_out);
    return (float *)(base + (uintptr_t)P->g_off[s]);
  }
  int64_t slot_bytes(int s) const { return 4 * rows[P->level[s]] * (int64_t)P->ch[s]; }

  // where operand `operand` of op i writes its gradient contribution to slot s: the slot's gradient buffer when it is the first one to
  // arrive (the slot's last reader), else a temporary that `commit` adds to it
  struct Target {
    float *ptr, *sum;
  };
  Target target(int i, int operand, int s, Carve &cv) const {
    if (P->first_op[s] == i && P->first_operand[s] == operand) return {launch ? G(s) : nullptr, nullptr};
    float *t = (float *)cv.take(slot_bytes(s));
    return {t, launch ? G(s) : nullptr};
  }
  int commit(const Target &t, int s) const {
    if (!t.sum || !launch) return FTX_OK;
    return ftx_rows_add(t.sum, t.ptr, rows[P->level[s]], P->ch[s], t.sum, stream);
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
  const Op &o = ops[i];
  const int64_t n = rows[o.level];
  switch (o.kind) {
    case FTX_SPVCNN_OP_CONV_BN:
    case FTX_SPVCNN_OP_LINEAR_BN: {
      const Layer &L = layers[o.layer];
      const bool linear = o.kind == FTX_SPVCNN_OP_LINEAR_BN;
      const float momentum = launch ? tlayers[o.layer].momentum : 0.f;
      float *x = (float *)(base + (uintptr_t)P->x_off[i]);
      float *mean = (float *)(base + (uintptr_t)P->stats_off[i]), *invstd = mean + L.co;
      float *rm = const_cast<float *>(L.mean), *rv = const_cast<float *>(L.var);
      const float *src = launch ? F(o.src) : nullptr;
      const float *res = (launch && !linear && o.src2 >= 0) ? F(o.src2) : nullptr;
      float *y = launch ? F(o.dst) : nullptr;
      const int r = routes[i];
      const int64_t bn_ws_bytes = (int64_t)ftx_bn_workspace_bytes(n, L.co);
      if (r == FTX_SPVCNN_ROUTE_ROWS) {
        void *ws = cv.take(bn_ws_bytes);
        RUN((L.bf16 ? ftx_rows_gemm_bf16 : ftx_rows_gemm)(src, n, L.weight, linear ? 1 : 0, linear ? L.bias : nullptr, L.ca, L.co, x, stream));
        RUN(ftx_bn_train_fwd(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, ws, (size_t)bn_ws_bytes, stream));
        break;
      }
      const Map &M = maps[o.map];
      const int64_t rows_a = rows[P->level[o.src]];
      const int32_t *gather = L.transposed ? M.pair_out : M.pair_in, *scatter = L.transposed ? M.pair_in : M.pair_out;
      const int32_t *dst_pos = L.transposed ? M.pos_t : M.pos;
      if (r == FTX_SPVCNN_ROUTE_OSTAT || r == FTX_SPVCNN_ROUTE_PAIRS) {
        // the convolution leaves the statistics (nb partial rows + the totals row, float64), then the one apply pass
        const int32_t nb = r == FTX_SPVCNN_ROUTE_OSTAT ? ftx_spconv_ostat_blocks(n) : ftx_spconv_reduce_stats_blocks(n, L.co);
        float *tmp = (float *)cv.take(r == FTX_SPVCNN_ROUTE_PAIRS ? 4 * M.n_pairs * (int64_t)L.co : 0);
        double *part = (double *)cv.take(16 * ((int64_t)nb + 1) * L.co);
        const double *totals = part + (int64_t)nb * 2 * L.co;
        if (r == FTX_SPVCNN_ROUTE_OSTAT) {
          RUN(ftx_spconv_ostat(src, rows_a, M.nbr, n, L.weight, 0, 0, L.ca, L.co, L.kvol, x, part, nb, stream));
        } else {
          RUN((L.bf16 ? ftx_spconv_pairs_gemm_bf16 : ftx_spconv_pairs_gemm)(src, rows_a, gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce_stats(tmp, dst_pos, n, L.co, L.kvol, x, part, nb, stream));
        }
        RUN(ftx_bn_train_fwd_totals(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, totals, stream));
      } else {
        // scatter epilogue or empty map: the plain convolution, then the BatchNorm's own statistics pass
        float *tmp = (float *)cv.take(r == FTX_SPVCNN_ROUTE_EMPTY ? 4 * M.n_pairs * (int64_t)L.co : 0);
        void *ws = cv.take(bn_ws_bytes);
        if (r == FTX_SPVCNN_ROUTE_DIRECT) {
          RUN((L.bf16 ? ftx_spconv_pairs_gemm_scatter_bf16 : ftx_spconv_pairs_gemm_scatter)(src, rows_a, gather, scatter, L.weight, 0, M.koff, M.n_pairs, L.ca,
                                                                                            L.co, L.kvol, x, n, stream));
        } else {
          RUN((L.bf16 ? ftx_spconv_pairs_gemm_bf16 : ftx_spconv_pairs_gemm)(src, rows_a, gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce(tmp, dst_pos, n, L.co, L.kvol, x, stream));
        }
        RUN(ftx_bn_train_fwd(x, res, L.gamma, L.beta, rm, rv, momentum, L.eps, n, L.co, o.relu, y, mean, invstd, ws, (size_t)bn_ws_bytes, stream));
      }
      break;
    }
    case FTX_SPVCNN_OP_VOXELIZE: {
      if (!launch) break;
      const PV &V = pvs[o.map];
      if (V.vox_order && V.vox_seg_off)
        RUN(ftx_voxelize_fwd_sorted(F(o.src), V.vox_order, V.vox_seg_off, rows[kLevels - 1], o.channels, n, F(o.dst), stream));
      else
        RUN(ftx_voxelize_fwd(F(o.src), V.vox_idx, V.vox_counts, rows[kLevels - 1], o.channels, n, F(o.dst), stream));
      break;
    }
    case FTX_SPVCNN_OP_DEVOXELIZE: {
      if (!launch) break;
      const PV &V = pvs[o.map];
      RUN(ftx_devoxelize_fwd(F(o.src), V.devox_idx, V.devox_weights, n, o.channels, V.n_vox, F(o.dst), stream));
      break;
    }
    case FTX_SPVCNN_OP_CONCAT:
      if (launch) RUN(ftx_rows_concat(F(o.src), P->ch[o.src], F(o.src2), P->ch[o.src2], n, F(o.dst), stream));
      break;
    case FTX_SPVCNN_OP_ADD:
      if (launch) RUN(ftx_rows_add(F(o.src), F(o.src2), n, o.channels, F(o.dst), stream));
      break;
    case FTX_SPVCNN_OP_ADD_EXT:
      if (launch && add[o.layer]) RUN(ftx_rows_add(F(o.src), add[o.layer], n, o.channels, F(o.dst), stream));
      break;
  }
  return FTX_OK;
}

// What the op's autograd node issues on the Python path, in that node's order.
int Exec::bwd_op(int i, Carve &cv) const {
  const Op &o = ops[i];
  const int64_t n = rows[o.level];
  const float *gy = launch ? G(o.dst) : nullptr;
  switch (o.kind) {
    case FTX_SPVCNN_OP_CONV_BN:
    case FTX_SPVCNN_OP_LINEAR_BN: {
      const Layer &L = layers[o.layer];
      const bool linear = o.kind == FTX_SPVCNN_OP_LINEAR_BN;
      const bool has_res = !linear && o.src2 >= 0;
      const bool need_data = o.src != FTX_SPVCNN_SLOT_INPUT;
      const int64_t n_src = rows[P->level[o.src]];
      TrainLayer T = {nullptr, nullptr, nullptr, nullptr, 0.f, 0};
      if (launch) T = tlayers[o.layer];
      const float *x = (const float *)(base + (uintptr_t)P->x_off[i]);
      const float *mean = (const float *)(base + (uintptr_t)P->stats_off[i]), *invstd = mean + L.co;
      const float *src = launch ? F(o.src) : nullptr;
      const float *y = launch ? F(o.dst) : nullptr;
      // BatchNorm half: gx = d loss / d (convolution output) is a temporary, consumed by the calls below
      const int64_t bn_ws_bytes = (int64_t)ftx_bn_workspace_bytes(n, L.co);
      void *bn_ws = cv.take(bn_ws_bytes);
      float *gx = (float *)cv.take(4 * n * (int64_t)L.co);
      Target tres = {nullptr, nullptr};
      if (has_res) tres = target(i, 1, o.src2, cv);
      RUN(ftx_bn_train_bwd(gy, x, y, L.gamma, L.beta, mean, invstd, n, L.co, o.relu, gx, tres.ptr, T.dgamma, T.dbeta, bn_ws, (size_t)bn_ws_bytes, stream));
      if (has_res) RUN(commit(tres, o.src2));
      Target tsrc = {nullptr, nullptr};
      if (need_data) tsrc = target(i, 0, o.src, cv);
      if (routes[i] == FTX_SPVCNN_ROUTE_ROWS) {
        void *wg_ws = cv.take(wgrad_ws_bytes(n, L.ca, L.co, 1));
        const size_t wg_bytes = (size_t)wgrad_ws_bytes(n, L.ca, L.co, 1);
        auto gemm = L.bf16 ? ftx_rows_gemm_bf16 : ftx_rows_gemm;
        auto wgrad = L.bf16 ? ftx_spconv_pairs_wgrad_bf16 : ftx_spconv_pairs_wgrad;
        if (linear) {   // weight (co, ca): gx @ W, dW = gx^T x, dbias = column sums of gx
          if (need_data) RUN(gemm(gx, n, L.weight, 0, nullptr, L.co, L.ca, tsrc.ptr, stream));
          RUN(wgrad(gx, n, nullptr, src, n, nullptr, nullptr, n, L.co, L.ca, 1, T.dweight, wg_ws, wg_bytes, stream));
          if (L.bias) {
            const int64_t cs_bytes = (int64_t)ftx_colsum_workspace_bytes(n, L.co);
            void *cs_ws = cv.take(cs_bytes);
            RUN(ftx_colsum(gx, n, L.co, T.dbias, cs_ws, (size_t)cs_bytes, stream));
          }
        } else {        // kernel (ca, co): gx @ W^T, dW = x^T gx
          if (need_data) RUN(gemm(gx, n, L.weight, 1, nullptr, L.co, L.ca, tsrc.ptr, stream));
          RUN(wgrad(src, n, nullptr, gx, n, nullptr, nullptr, n, L.ca, L.co, 1, T.dweight, wg_ws, wg_bytes, stream));
        }
      } else {
        const Map &M = maps[o.map];
        // per pair the row the convolution reads (src side) and the row it writes (dst side): functional._map_sides
        const int32_t *ps = L.transposed ? M.pair_out : M.pair_in, *pd = L.transposed ? M.pair_in : M.pair_out;
        const int32_t *src_pos = L.transposed ? M.pos : M.pos_t;
        const int gr = need_data ? groutes[i] : -1;
        float *tmp = (float *)cv.take(gr == FTX_SPVCNN_ROUTE_PAIRS ? 4 * M.n_pairs * (int64_t)L.ca : 0);
        const int64_t wg_bytes = wgrad_ws_bytes(M.n_pairs, L.ca, L.co, L.kvol);
        void *wg_ws = cv.take(wg_bytes);
        if (gr == FTX_SPVCNN_ROUTE_EMPTY) {
          if (launch && n_src > 0 && hipMemsetAsync(tsrc.ptr, 0, sizeof(float) * n_src * L.ca, (hipStream_t)stream) != hipSuccess)
            return check_launch("ftx_spvcnn_train_bwd memset");
        } else if (gr == FTX_SPVCNN_ROUTE_DIRECT) {
          RUN((L.bf16 ? ftx_spconv_pairs_gemm_scatter_bf16 : ftx_spconv_pairs_gemm_scatter)(gx, n, pd, ps, L.weight, 1, M.koff, M.n_pairs, L.co, L.ca, L.kvol,
                                                                                            tsrc.ptr, n_src, stream));
        } else if (gr == FTX_SPVCNN_ROUTE_PAIRS) {
          RUN((L.bf16 ? ftx_spconv_pairs_gemm_bf16 : ftx_spconv_pairs_gemm)(gx, n, pd, L.weight, 1, M.koff, M.n_pairs, L.co, L.ca, L.kvol, tmp, stream));
          RUN(ftx_spconv_reduce(tmp, src_pos, n_src, L.ca, L.kvol, tsrc.ptr, stream));
        }
        RUN((L.bf16 ? ftx_spconv_pairs_wgrad_bf16 : ftx_spconv_pairs_wgrad)(src, n_src, ps, gx, n, pd, M.koff, M.n_pairs, L.ca, L.co, L.kvol, T.dweight, wg_ws,
                                                                            (size_t)wg_bytes, stream));
      }
      if (need_data) RUN(commit(tsrc, o.src));
      break;
    }
    case FTX_SPVCNN_OP_VOXELIZE: {
      const Target t = target(i, 0, o.src, cv);
      if (!launch) break;
      const PV &V = pvs[o.map];
      RUN(ftx_voxelize_bwd(gy, V.vox_idx, V.vox_counts, rows[kLevels - 1], o.channels, n, t.ptr, stream));
      RUN(commit(t, o.src));
      break;
    }
    case FTX_SPVCNN_OP_DEVOXELIZE: {
      const Target t = target(i, 0, o.src, cv);
      if (!launch) break;
      const PV &V = pvs[o.map];
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
      RUN(ftx_rows_split(gy, n, P->ch[o.src], P->ch[o.src2], ta.ptr, tb.ptr, stream));
      RUN(commit(ta, o.src));
      RUN(commit(tb, o.src2));
      break;
    }
    case FTX_SPVCNN_OP_ADD:       // both operands take the gradient of the sum as it is: their gradient buffers ARE the sum's
    case FTX_SPVCNN_OP_ADD_EXT:   // in place: the slot's gradient is also the addend's
      break;
  }
  return FTX_OK;
}
#undef RUN

// Validates the program against the tables and places every buffer.  Host only.
int make_plan(const Layer *layers, int32_t n_layers, const Op *ops, int32_t n_ops, const int64_t *rows, const Map *maps, int32_t n_maps, const PV *pvs,
              int32_t n_pvs, const int32_t *routes, const int32_t *groutes, Plan &P) {
  const char *who = kWho;
  PLAN_REQUIRE(ops && rows && routes && groutes && n_ops >= 1 && n_ops <= kMaxOps, "%s: null table or op count outside [1, %d]", who, kMaxOps);
  PLAN_REQUIRE(n_layers >= 0 && n_maps >= 0 && n_pvs >= 0 && (layers || !n_layers) && (maps || !n_maps) && (pvs || !n_pvs), "%s: null table", who);
  for (int l = 0; l < kLevels; ++l)
    PLAN_REQUIRE(rows[l] >= 1 && rows[l] < (1ll << 31), "%s: rows[%d] = %lld (the training BatchNorm needs at least one row on every level)", who, l,
                 (long long)rows[l]);
  for (int m = 0; m < n_maps; ++m)
    PLAN_REQUIRE(maps[m].n_pairs >= 0 && maps[m].n_in >= 0 && maps[m].n_out >= 0 && maps[m].n_pairs < (1ll << 31), "%s: map %d has a negative or huge count", who, m);
  for (auto *v : {&P.level, &P.ch, &P.def, &P.first_op, &P.first_operand, &P.galias, &P.read_lo, &P.read_hi}) v->assign(kMaxSlots, -1);
  P.uses.assign(kMaxSlots, 0);
  P.f_off.assign(kMaxSlots, -1);
  P.g_off.assign(kMaxSlots, -1);
  P.x_off.assign(n_ops, -1);
  P.stats_off.assign(n_ops, -1);
  P.level[FTX_SPVCNN_SLOT_INPUT] = 0;   // the voxelised input features; channel count fixed by its first reader
  P.def[FTX_SPVCNN_SLOT_INPUT] = 0;
  int seg = 0;
  auto slot_ok = [](int s) { return s >= 0 && s < kMaxSlots; };
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    PLAN_REQUIRE(o.kind >= FTX_SPVCNN_OP_CONV_BN && o.kind <= FTX_SPVCNN_OP_ADD_EXT, "%s: op %d: unknown kind %d", who, i, o.kind);
    const char *kn = kKindName[o.kind];
    PLAN_REQUIRE((o.segment == seg || o.segment == seg + 1) && o.segment < kMaxSegments && (i > 0 || o.segment == 0),
                 "%s: op %d (%s): segments are numbered from 0 without a gap, ascending, at most %d", who, i, kn, kMaxSegments);
    seg = o.segment;
    PLAN_REQUIRE(slot_ok(o.src) && slot_ok(o.dst) && P.def[o.src] >= 0, "%s: op %d (%s): source slot %d is not written before it is read", who, i, kn, o.src);
    PLAN_REQUIRE(o.level >= 0 && o.level < kLevels, "%s: op %d (%s): level %d", who, i, kn, o.level);
    PLAN_REQUIRE(o.channels >= 4 && o.channels % 4 == 0 && o.channels <= 1024, "%s: op %d (%s): channel count %d is not a multiple of 4 in [4, 1024]", who, i,
                 kn, o.channels);
    const int64_t n_dst = rows[o.level];
    auto need_src = [&](int s, int c) {      // the input slot takes the channel count of its first reader
      if (P.ch[s] < 0) P.ch[s] = c;
      return P.ch[s] == c;
    };
    int grad_to[2] = {-1, -1};               // the slots this op's backward sends a gradient to, by operand
    int second = -1;
    switch (o.kind) {
      case FTX_SPVCNN_OP_CONV_BN:
      case FTX_SPVCNN_OP_LINEAR_BN: {
        PLAN_REQUIRE(o.layer >= 0 && o.layer < n_layers, "%s: op %d (%s): layer %d out of range", who, i, kn, o.layer);
        const Layer &L = layers[o.layer];
        const bool conv = o.kind == FTX_SPVCNN_OP_CONV_BN;
        PLAN_REQUIRE(L.kind == (conv ? FTX_SPVCNN_LAYER_CONV_BN : FTX_SPVCNN_LAYER_LINEAR_BN), "%s: op %d (%s): layer %d is of another kind", who, i, kn, o.layer);
        PLAN_REQUIRE(L.ca >= 4 && L.ca % 4 == 0 && L.co >= 4 && L.co % 4 == 0 && L.co <= 512, "%s: op %d (%s) layer %d: channels must be multiples of 4 (ca=%d co=%d)",
                     who, i, kn, o.layer, L.ca, L.co);
        PLAN_REQUIRE(L.co == o.channels && need_src(o.src, L.ca), "%s: op %d (%s) layer %d: channel counts do not match the slots", who, i, kn, o.layer);
        PLAN_REQUIRE(L.weight && L.gamma && L.beta && L.mean && L.var, "%s: op %d (%s) layer %d: null parameter", who, i, kn, o.layer);
        const int r = routes[i];
        if (o.src != FTX_SPVCNN_SLOT_INPUT) grad_to[0] = o.src;
        if (!conv || L.kvol == 1) {
          PLAN_REQUIRE(r == FTX_SPVCNN_ROUTE_ROWS, "%s: op %d (%s) layer %d: a dense layer takes the rows route, got %d", who, i, kn, o.layer, r);
          PLAN_REQUIRE(L.ca <= 512 && L.co <= 512 && (conv ? L.stride == 1 && !L.transposed : L.kvol == 0), "%s: op %d (%s) layer %d: unsupported dense layer",
                       who, i, kn, o.layer);
          PLAN_REQUIRE(P.level[o.src] == o.level, "%s: op %d (%s): a dense layer keeps its rows", who, i, kn);
        } else {
          PLAN_REQUIRE(L.kvol == 8 || L.kvol == 27, "%s: op %d (%s) layer %d: kernel volume %d (1, 8 or 27)", who, i, kn, o.layer, L.kvol);
          PLAN_REQUIRE(o.map >= 0 && o.map < n_maps && maps[o.map].kvol == L.kvol, "%s: op %d (%s) layer %d: kernel map %d missing or of another volume", who, i,
                       kn, o.layer, o.map);
          const Map &M = maps[o.map];
          const int64_t m_in = L.transposed ? M.n_out : M.n_in, m_out = L.transposed ? M.n_in : M.n_out;
          const int64_t n_src = rows[P.level[o.src]];
          PLAN_REQUIRE(n_src == m_in && n_dst == m_out, "%s: op %d (%s) layer %d: kernel map %d is (%lld -> %lld), the slots hold (%lld -> %lld)", who, i, kn,
                       o.layer, o.map, (long long)m_in, (long long)m_out, (long long)n_src, (long long)n_dst);
          PLAN_REQUIRE(M.koff, "%s: op %d (%s): null offset table in map %d", who, i, kn, o.map);
          PLAN_REQUIRE(!M.n_pairs || (M.pair_in && M.pair_out), "%s: op %d (%s): null pair list in map %d (the weight gradient reads both sides)", who, i, kn, o.map);
          if (r == FTX_SPVCNN_ROUTE_DIRECT) {
            PLAN_REQUIRE(M.fine_bijective && M.n_pairs == n_dst && L.transposed, "%s: op %d (%s) layer %d: the direct route needs a transposed layer on a "
                         "map whose pairs cover every output row once", who, i, kn, o.layer);
          } else if (r == FTX_SPVCNN_ROUTE_OSTAT) {
            PLAN_REQUIRE(!L.bf16 && !L.transposed && ftx_spconv_ostat_supported(L.ca, L.co, L.kvol, 0) && n_dst <= kOstatMaxRows && M.n_pairs > 0,
                         "%s: op %d (%s) layer %d: the output-stationary route does not take this layer", who, i, kn, o.layer);
            PLAN_REQUIRE(M.nbr, "%s: op %d (%s): null neighbour table in map %d", who, i, kn, o.map);
          } else if (r == FTX_SPVCNN_ROUTE_PAIRS || r == FTX_SPVCNN_ROUTE_EMPTY) {
            PLAN_REQUIRE((r == FTX_SPVCNN_ROUTE_PAIRS) == (M.n_pairs > 0), "%s: op %d (%s) layer %d: the empty route is for a map without pairs, and only for it",
                         who, i, kn, o.layer);
            PLAN_REQUIRE(L.transposed ? M.pos_t : M.pos, "%s: op %d (%s): null position table in map %d", who, i, kn, o.map);
          } else {
            PLAN_REQUIRE(false, "%s: op %d (%s) layer %d: route %d is not one this entry point takes", who, i, kn, o.layer, r);
          }
          if (grad_to[0] >= 0) {   // the data gradient: functional._conv_route(grad=True)
            const int gr = groutes[i];
            if (gr == FTX_SPVCNN_ROUTE_EMPTY)
              PLAN_REQUIRE(M.n_pairs == 0, "%s: op %d (%s) layer %d: the empty gradient route on a map with pairs", who, i, kn, o.layer);
            else if (gr == FTX_SPVCNN_ROUTE_DIRECT)
              PLAN_REQUIRE(M.fine_bijective && !L.transposed && M.n_pairs == n_src, "%s: op %d (%s) layer %d: the direct gradient route needs a strided layer on "
                           "a map whose pairs cover every input row once", who, i, kn, o.layer);
            else if (gr == FTX_SPVCNN_ROUTE_PAIRS)
              PLAN_REQUIRE(M.n_pairs > 0 && (L.transposed ? M.pos : M.pos_t), "%s: op %d (%s) layer %d: the pair-list gradient route needs pairs and the position "
                           "table of the input side", who, i, kn, o.layer);
            else
              PLAN_REQUIRE(false, "%s: op %d (%s) layer %d: gradient route %d is not one this entry point takes", who, i, kn, o.layer, gr);
          }
        }
        if (conv && o.src2 >= 0) {
          PLAN_REQUIRE(slot_ok(o.src2) && P.def[o.src2] >= 0 && P.level[o.src2] == o.level && need_src(o.src2, o.channels) && o.src2 != FTX_SPVCNN_SLOT_INPUT,
                       "%s: op %d (%s): the residual slot does not match the output", who, i, kn);
          second = grad_to[1] = o.src2;
        }
        break;
      }
      case FTX_SPVCNN_OP_VOXELIZE:
      case FTX_SPVCNN_OP_DEVOXELIZE: {
        const bool vox = o.kind == FTX_SPVCNN_OP_VOXELIZE;
        PLAN_REQUIRE(o.map >= 0 && o.map < n_pvs, "%s: op %d (%s): point-voxel index %d out of range", who, i, kn, o.map);
        const PV &V = pvs[o.map];
        const int vlev = vox ? o.level : P.level[o.src], plev = vox ? P.level[o.src] : o.level;
        PLAN_REQUIRE(plev == kLevels - 1 && vlev == V.level && V.level >= 0 && V.level < kLevels - 1 && rows[vlev] == V.n_vox,
                     "%s: op %d (%s): point-voxel index %d does not join these slots", who, i, kn, o.map);
        PLAN_REQUIRE(need_src(o.src, o.channels) && o.src != FTX_SPVCNN_SLOT_INPUT, "%s: op %d (%s): channel counts differ", who, i, kn);
        if (vox)
          PLAN_REQUIRE(V.vox_idx && V.vox_counts, "%s: op %d (%s): null voxel index in index %d (the backward reads it)", who, i, kn, o.map);
        else
          PLAN_REQUIRE(V.devox_idx && V.devox_weights, "%s: op %d (%s): null corner table in index %d", who, i, kn, o.map);
        grad_to[0] = o.src;
        break;
      }
      case FTX_SPVCNN_OP_CONCAT:
      case FTX_SPVCNN_OP_ADD: {
        PLAN_REQUIRE(slot_ok(o.src2) && P.def[o.src2] >= 0 && P.level[o.src] == o.level && P.level[o.src2] == o.level && o.src != o.src2 &&
                     o.src != FTX_SPVCNN_SLOT_INPUT && o.src2 != FTX_SPVCNN_SLOT_INPUT, "%s: op %d (%s): operands of different levels", who, i, kn);
        PLAN_REQUIRE(P.ch[o.src] > 0 && P.ch[o.src2] > 0 && (o.kind == FTX_SPVCNN_OP_ADD ? (P.ch[o.src] == o.channels && P.ch[o.src2] == o.channels)
                                                                                          : P.ch[o.src] + P.ch[o.src2] == o.channels),
                     "%s: op %d (%s): channel counts do not add up", who, i, kn);
        second = o.src2;
        grad_to[0] = o.src;
        grad_to[1] = o.src2;
        break;
      }
      case FTX_SPVCNN_OP_ADD_EXT:
        PLAN_REQUIRE(o.dst == o.src && (o.layer == 0 || o.layer == 1) && P.level[o.src] == o.level && P.ch[o.src] == o.channels && o.src >= FTX_SPVCNN_SLOT_FIRST,
                     "%s: op %d (%s): the fusion addend is added in place to an arena slot (layer = 0 early, 1 middle)", who, i, kn);
        PLAN_REQUIRE(P.uses[o.src] == 0, "%s: op %d (%s): slot %d is read before the addend reaches it, and the backward would read it after", who, i, kn, o.src);
        break;
    }
    if (o.kind != FTX_SPVCNN_OP_ADD_EXT) {
      PLAN_REQUIRE(o.dst != FTX_SPVCNN_SLOT_INPUT && P.def[o.dst] < 0, "%s: op %d (%s): slot %d is written twice", who, i, kn, o.dst);
      PLAN_REQUIRE(o.dst != FTX_SPVCNN_SLOT_OUTPUT || o.level == kLevels - 1, "%s: op %d (%s): the output slot holds point rows", who, i, kn);
      PLAN_REQUIRE(o.dst != FTX_SPVCNN_SLOT_OUTPUT || (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN),
                   "%s: op %d (%s): a layer may not write the output slot (its backward reads its result, which the backward is not given)", who, i, kn);
      P.def[o.dst] = i;
      P.level[o.dst] = o.level;
      P.ch[o.dst] = o.channels;
    }
    for (int k = 0; k < 2; ++k) {
      const int s = grad_to[k];
      if (s < 0) continue;
      PLAN_REQUIRE(++P.uses[s] <= 2, "%s: op %d (%s): slot %d would receive more than two gradient contributions", who, i, kn, s);
      P.first_op[s] = i;       // the last reader in program order is the first to contribute in the backward
      P.first_operand[s] = k;
    }
    for (int s : {o.src, second}) {
      if (s < 0) continue;
      if (P.read_lo[s] < 0) P.read_lo[s] = o.segment;
      P.read_hi[s] = o.segment;
    }
    if (o.kind == FTX_SPVCNN_OP_ADD) {
      P.galias[o.src] = o.dst;
      P.galias[o.src2] = o.dst;
    }
  }
  P.n_segments = seg + 1;
  P.in_slot.assign(P.n_segments, -1);
  P.out_slot.assign(P.n_segments, -1);
  for (int i = 0; i < n_ops; ++i) P.out_slot[ops[i].segment] = ops[i].dst;
  for (int s = 0; s < P.n_segments; ++s) P.in_slot[s] = s ? P.out_slot[s - 1] : FTX_SPVCNN_SLOT_INPUT;
  PLAN_REQUIRE(P.out_slot[P.n_segments - 1] == FTX_SPVCNN_SLOT_OUTPUT && P.def[FTX_SPVCNN_SLOT_OUTPUT] >= 0, "%s: the last op writes the output slot", who);
  for (int s = FTX_SPVCNN_SLOT_OUTPUT; s < kMaxSlots; ++s) {
    if (P.def[s] < 0) continue;
    if (P.galias[s] >= 0) PLAN_REQUIRE(P.uses[s] == 1, "%s: slot %d is an operand of an add and of another op: its gradient would need a copy", who, s);
    PLAN_REQUIRE(P.uses[s] >= 1 || s == FTX_SPVCNN_SLOT_OUTPUT, "%s: slot %d is never read: its producer would take an undefined gradient", who, s);
    PLAN_REQUIRE(s != FTX_SPVCNN_SLOT_OUTPUT || P.uses[s] == 0, "%s: the output slot is read inside the program", who);
  }
  // placement: one region per slot, per slot gradient, per layer output and statistics -- nothing is shared, so nothing the backward
  // reads has a later writer -- then the shared region of the per-op temporaries
  int64_t off = 0;
  for (int s = FTX_SPVCNN_SLOT_FIRST; s < kMaxSlots; ++s) {
    if (P.def[s] < 0) continue;
    const int64_t b = align256(4 * rows[P.level[s]] * (int64_t)P.ch[s]);
    P.f_off[s] = off;
    off += b;
    if (P.galias[s] < 0) {
      P.g_off[s] = off;
      off += b;
    }
  }
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    if (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN) continue;
    P.x_off[i] = off;
    off += align256(4 * rows[o.level] * (int64_t)o.channels);
    P.stats_off[i] = off;
    off += align256(8 * (int64_t)o.channels);
  }
  P.temp_off = off;
  Exec E;
  E.layers = layers;
  E.ops = ops;
  E.rows = rows;
  E.maps = maps;
  E.pvs = pvs;
  E.routes = routes;
  E.groutes = groutes;
  E.P = &P;
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

int fail(const char *entry, int i, const Op &o, int rc) {
  const std::string inner = ftx_last_error();
  set_error("%s: op %d (%s, layer %d): %s", entry, i, kKindName[o.kind], o.kind <= FTX_SPVCNN_OP_LINEAR_BN ? o.layer : -1, inner.c_str());
  return rc;
}

// what both directions check after the plan: the segment range, the arena, the buffer that stands for the first segment's input
int check_call(const char *entry, const Plan &P, const Op *ops, int32_t n_ops, int32_t first, int32_t last, const void *seg_in, const void *arena,
               size_t arena_bytes) {
  FTX_REQUIRE(first >= 0 && first <= last && last < P.n_segments, "%s: segments [%d, %d] outside 0..%d", entry, first, last, P.n_segments - 1);
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "%s: the arena must be a 256-byte aligned device buffer", entry);
  if (arena_bytes < (size_t)P.total) {
    set_error("%s: arena %zu < required %zu (ftx_spvcnn_train_arena_bytes)", entry, arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  const int in = P.in_slot[first];
  FTX_REQUIRE(seg_in, "%s: null input of segment %d", entry, first);
  FTX_REQUIRE(((uintptr_t)seg_in & 15) == 0, "%s: the input of segment %d must be 16-byte aligned", entry, first);
  if (in >= FTX_SPVCNN_SLOT_FIRST && (P.read_lo[in] != first || P.read_hi[in] != first))
    FTX_REQUIRE((const char *)seg_in == (const char *)arena + P.f_off[in], "%s: the input of segment %d is also read by another segment: it must be the buffer "
                "the previous segment returned", entry, first);
  for (int i = 0; i < n_ops; ++i) {   // a segment other than the first reads the input features or another segment's replaced input
    const Op &o = ops[i];
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
  Plan P;
  if (make_plan((const Layer *)layers_host, n_layers, (const Op *)ops_host, n_ops, rows_host, (const Map *)maps_host, n_maps, (const PV *)pvs_host, n_pvs,
                routes_host, grad_routes_host, P) != FTX_OK)
    return 0;
  return (size_t)P.total;
}

extern "C" int ftx_spvcnn_train_fwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                    const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs,
                                    const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment,
                                    const float *seg_in, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out,
                                    float **seg_out, void *stream) {
  const char *entry = "ftx_spvcnn_train_fwd";
  const Op *ops = (const Op *)ops_host;
  Plan P;
  int rc = make_plan((const Layer *)layers_host, n_layers, ops, n_ops, rows_host, (const Map *)maps_host, n_maps, (const PV *)pvs_host, n_pvs, routes_host,
                     grad_routes_host, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(train_layers_host || !n_layers, "%s: null train table", entry);
  rc = check_call(entry, P, ops, n_ops, first_segment, last_segment, seg_in, arena, arena_bytes);
  if (rc != FTX_OK) return rc;
  const int out_slot = P.out_slot[last_segment];
  FTX_REQUIRE(out_slot != FTX_SPVCNN_SLOT_OUTPUT || out, "%s: null output", entry);
  Exec E;
  E.layers = (const Layer *)layers_host;
  E.tlayers = (const TrainLayer *)train_layers_host;
  E.ops = ops;
  E.rows = rows_host;
  E.maps = (const Map *)maps_host;
  E.pvs = (const PV *)pvs_host;
  E.routes = routes_host;
  E.groutes = grad_routes_host;
  E.P = &P;
  E.base = (uintptr_t)arena;
  E.seg_in = seg_in;
  E.in_slot = P.in_slot[first_segment];
  E.add[0] = add_early;
  E.add[1] = add_middle;
  E.out = out;
  E.stream = stream;
  E.launch = true;
  // everything above answered on the host; from here on launches only
  for (int i = 0; i < n_ops; ++i) {
    if (ops[i].segment < first_segment || ops[i].segment > last_segment) continue;
    Carve cv;
    cv.base = E.base + (uintptr_t)P.temp_off;
    rc = E.fwd_op(i, cv);
    if (rc != FTX_OK) return fail(entry, i, ops[i], rc);
  }
  if (seg_out) *seg_out = E.F(out_slot);
  return FTX_OK;
}

extern "C" int ftx_spvcnn_train_bwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops,
                                    const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, const void *train_pvs_host,
                                    int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment,
                                    int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in,
                                    void *stream) {
  const char *entry = "ftx_spvcnn_train_bwd";
  const Op *ops = (const Op *)ops_host;
  const Layer *layers = (const Layer *)layers_host;
  const TrainLayer *tl = (const TrainLayer *)train_layers_host;
  Plan P;
  int rc = make_plan(layers, n_layers, ops, n_ops, rows_host, (const Map *)maps_host, n_maps, (const PV *)pvs_host, n_pvs, routes_host, grad_routes_host, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE((tl || !n_layers) && (train_pvs_host || !n_pvs), "%s: null train table", entry);
  rc = check_call(entry, P, ops, n_ops, first_segment, last_segment, seg_in, arena, arena_bytes);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(grad_out && ((uintptr_t)grad_out & 15) == 0, "%s: null or misaligned output gradient", entry);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    if (o.segment < first_segment || o.segment > last_segment || (o.kind != FTX_SPVCNN_OP_CONV_BN && o.kind != FTX_SPVCNN_OP_LINEAR_BN)) continue;
    const TrainLayer &T = tl[o.layer];
    FTX_REQUIRE(T.dweight && T.dgamma && T.dbeta && (T.dbias || !layers[o.layer].bias), "%s: op %d, layer %d: null gradient destination", entry, i, o.layer);
  }
  Exec E;
  E.layers = layers;
  E.tlayers = tl;
  E.ops = ops;
  E.rows = rows_host;
  E.maps = (const Map *)maps_host;
  E.pvs = (const PV *)pvs_host;
  E.tpvs = (const TrainPV *)train_pvs_host;
  E.routes = routes_host;
  E.groutes = grad_routes_host;
  E.P = &P;
  E.base = (uintptr_t)arena;
  E.seg_in = seg_in;
  E.in_slot = P.in_slot[first_segment];
  E.grad_out = grad_out;
  E.gout_slot = P.out_slot[last_segment];
  E.stream = stream;
  E.launch = true;
  for (int i = n_ops - 1; i >= 0; --i) {
    if (ops[i].segment < first_segment || ops[i].segment > last_segment) continue;
    Carve cv;
    cv.base = E.base + (uintptr_t)P.temp_off;
    rc = E.bwd_op(i, cv);
    if (rc != FTX_OK) return fail(entry, i, ops[i], rc);
  }
  if (grad_in) *grad_in = first_segment ? E.G(E.in_slot) : nullptr;
  return FTX_OK;
}
