// Native eval-mode executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_eval).  Where the Python path uses torch (channel
// concatenation, row-wise add) it issues the row kernels of ftx_rows.hip.
//
// The network is a static op program that the host emits once per model (fusiontransformer_amd/native_eval.py) over numbered buffers
// ("slots"); it is validated against the model and batch tables by the checker both SPVCNN executors share (ftx_spvcnn_program.h);
// this file places every slot and every per-op temporary in the caller's arena and issues the ops of the requested segments through
// the library's own per-op entry points -- the same launch code and the same order as the Python path, minus the Python.  No state
// outlives a call; nothing here synchronises or allocates.
#include <vector>
#include "ftx_spvcnn_program.h"

using namespace ftx;

// ---------------------------------------------------------------- plan (the checker of the program: ftx_spvcnn_program.h)
namespace {

// Where every slot and every per-op temporary lies in the arena.
struct Plan {
  int last[kMaxSlots], region[kMaxSlots];   // per slot: its last reader, its region
  std::vector<int64_t> region_bytes, region_off, op_temp;
  int64_t temp_off = 0, temp_bytes = 0, total = 0;
};

// Validates the program against the tables (check_program) and places slots and temporaries.  Host only.  Regions are shared by
// slots of the same level whose lifetimes do not overlap; which slots share is decided by the program alone, a region is as large as
// its largest tenant, so the total never shrinks when a row or pair count grows.
int make_plan(const SpvcnnTables &T, SlotFacts &F, Plan &P) {
  const int rc = check_program(T, false, F);
  if (rc != FTX_OK) return rc;
  const int n_ops = T.n_ops;
  for (int s = 0; s < kMaxSlots; ++s) P.last[s] = P.region[s] = -1;
  P.op_temp.assign(n_ops, 0);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = T.ops[i];
    if (o.kind <= FTX_SPVCNN_OP_LINEAR_BN) P.op_temp[i] = align256(4 * F.op[i].temp_rows * (int64_t)T.layers[o.layer].co);
    P.last[o.src] = i;
    if (F.op[i].second >= 0) P.last[F.op[i].second] = i;
    if (P.last[o.dst] < i) P.last[o.dst] = i;
  }
  // regions: per level, the lowest-numbered free one; a slot's region is free again after its last reader
  std::vector<std::vector<int>> free_regions(kLevels);
  std::vector<std::vector<int>> dying(n_ops);
  for (int s = FTX_SPVCNN_SLOT_FIRST; s < kMaxSlots; ++s)
    if (F.def[s] >= 0) dying[P.last[s]].push_back(s);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = T.ops[i];
    if (o.kind != FTX_SPVCNN_OP_ADD_EXT && o.dst >= FTX_SPVCNN_SLOT_FIRST) {
      auto &fr = free_regions[o.level];
      int reg;
      if (fr.empty()) {
        reg = (int)P.region_bytes.size();
        P.region_bytes.push_back(0);
      } else {
        size_t best = 0;
        for (size_t k = 1; k < fr.size(); ++k)
          if (fr[k] < fr[best]) best = k;
        reg = fr[best];
        fr.erase(fr.begin() + best);
      }
      P.region[o.dst] = reg;
      const int64_t b = align256(4 * T.rows[o.level] * (int64_t)o.channels);
      if (b > P.region_bytes[reg]) P.region_bytes[reg] = b;
    }
    for (int s : dying[i]) free_regions[F.level[s]].push_back(P.region[s]);
    if (P.op_temp[i] > P.temp_bytes) P.temp_bytes = P.op_temp[i];
  }
  int64_t off = 0;
  P.region_off.resize(P.region_bytes.size());
  for (size_t r = 0; r < P.region_bytes.size(); ++r) {
    P.region_off[r] = off;
    off += P.region_bytes[r];
  }
  P.temp_off = off;
  P.total = off + P.temp_bytes;
  if (P.total < 256) P.total = 256;
  return FTX_OK;
}

}  // namespace

extern "C" int32_t ftx_spvcnn_layer_bytes(void) { return (int32_t)sizeof(Layer); }
extern "C" int32_t ftx_spvcnn_op_bytes(void) { return (int32_t)sizeof(Op); }
extern "C" int32_t ftx_spvcnn_map_bytes(void) { return (int32_t)sizeof(Map); }
extern "C" int32_t ftx_spvcnn_pv_bytes(void) { return (int32_t)sizeof(PV); }

extern "C" size_t ftx_spvcnn_eval_arena_bytes(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host,
                                              const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host) {
  SlotFacts F;
  Plan P;
  if (make_plan(spvcnn_tables(layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs, routes_host), F, P) != FTX_OK) return 0;
  return (size_t)P.total;
}

extern "C" int ftx_spvcnn_eval(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host,
                               const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const float *x0,
                               int32_t first_segment, int32_t last_segment, const float *add_early, const float *add_middle, void *arena,
                               size_t arena_bytes, float *out, void *stream) {
  const SpvcnnTables T = spvcnn_tables(layers_host, n_layers, ops_host, n_ops, rows_host, maps_host, n_maps, pvs_host, n_pvs, routes_host);
  const Op *ops = T.ops;
  const int64_t *rows = T.rows;
  SlotFacts F;
  Plan P;
  int rc = make_plan(T, F, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(first_segment >= 0 && first_segment <= last_segment && last_segment <= 2, "ftx_spvcnn_eval: segments [%d, %d] outside 0..2", first_segment,
              last_segment);
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "ftx_spvcnn_eval: the arena must be a 256-byte aligned device buffer");
  if (arena_bytes < (size_t)P.total) {
    set_error("ftx_spvcnn_eval: arena %zu < required %zu (ftx_spvcnn_eval_arena_bytes)", arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  bool reads_input = false, writes_output = false;
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    if (o.segment < first_segment || o.segment > last_segment) continue;
    reads_input |= o.src == FTX_SPVCNN_SLOT_INPUT || ((o.kind == FTX_SPVCNN_OP_CONV_BN || o.kind == FTX_SPVCNN_OP_CONCAT || o.kind == FTX_SPVCNN_OP_ADD) &&
                                                      o.src2 == FTX_SPVCNN_SLOT_INPUT);
    writes_output |= o.dst == FTX_SPVCNN_SLOT_OUTPUT;
  }
  FTX_REQUIRE(!reads_input || x0 || rows[0] == 0, "ftx_spvcnn_eval: null input features");
  FTX_REQUIRE(!writes_output || out || rows[kLevels - 1] == 0, "ftx_spvcnn_eval: null output");
  char *base = (char *)arena;
  float *temp = (float *)(base + P.temp_off);
  auto at = [&](int s) -> float * {
    if (s == FTX_SPVCNN_SLOT_INPUT) return const_cast<float *>(x0);
    if (s == FTX_SPVCNN_SLOT_OUTPUT) return out;
    return (float *)(base + P.region_off[P.region[s]]);
  };
#define RUN(call)                                              \
  do {                                                         \
    rc = (call);                                               \
    if (rc != FTX_OK) return fail("ftx_spvcnn_eval", i, o, rc); \
  } while (0)
  // everything above answered on the host; from here on launches only
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    if (o.segment < first_segment || o.segment > last_segment) continue;
    const int64_t n = rows[o.level];
    const float *src = at(o.src);
    float *dst = at(o.dst);
    switch (o.kind) {
      case FTX_SPVCNN_OP_CONV_BN: {
        const Layer &L = T.layers[o.layer];
        const SpconvEntries E = spconv_entries(L);
        const float *res = o.src2 >= 0 ? at(o.src2) : nullptr;
        const int64_t rows_a = rows[F.level[o.src]];
        if (L.kvol == 1) {
          RUN(E.rows(src, n, L.weight, 0, nullptr, L.ca, L.co, temp, stream));
          RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
          break;
        }
        const Map &M = T.maps[o.map];
        const MapSides side = map_sides(L, M);
        switch (T.routes[i]) {
          case FTX_SPVCNN_ROUTE_DIRECT:
            RUN(E.scatter(src, rows_a, side.gather, side.scatter, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, temp, n,
                          stream));
            RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
            break;
          case FTX_SPVCNN_ROUTE_OSTAT:
            RUN(ftx_spconv_ostat(src, rows_a, M.nbr, n, L.weight, 0, 0, L.ca, L.co, L.kvol, temp, nullptr, 0, stream));
            RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
            break;
          default:   // pairs, or the empty map (no pair rows: every output row reduces to zero before the BatchNorm)
            RUN(E.pairs(src, rows_a, side.gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, temp, stream));
            RUN(ftx_spconv_reduce_bn_eval(temp, side.dst_pos, n, L.co, L.kvol, res, L.gamma, L.beta, L.mean, L.var, L.eps, o.relu, dst, stream));
            break;
        }
        break;
      }
      case FTX_SPVCNN_OP_LINEAR_BN: {
        const Layer &L = T.layers[o.layer];
        const SpconvEntries E = spconv_entries(L);
        RUN(E.rows(src, n, L.weight, 1, L.bias, L.ca, L.co, temp, stream));
        RUN(ftx_bn_eval_fwd(temp, nullptr, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_VOXELIZE: {
        const PV &V = T.pvs[o.map];
        RUN(ftx_voxelize_fwd_sorted(src, V.vox_order, V.vox_seg_off, rows[kLevels - 1], o.channels, n, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_DEVOXELIZE: {
        const PV &V = T.pvs[o.map];
        RUN(ftx_devoxelize_fwd(src, V.devox_idx, V.devox_weights, n, o.channels, V.n_vox, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_CONCAT:
        RUN(ftx_rows_concat(src, F.ch[o.src], at(o.src2), F.ch[o.src2], n, dst, stream));
        break;
      case FTX_SPVCNN_OP_ADD:
        RUN(ftx_rows_add(src, at(o.src2), n, o.channels, dst, stream));
        break;
      case FTX_SPVCNN_OP_ADD_EXT: {
        const float *addend = o.layer == 0 ? add_early : add_middle;
        if (addend) RUN(ftx_rows_add(src, addend, n, o.channels, dst, stream));
        break;
      }
    }
  }
#undef RUN
  return FTX_OK;
}
