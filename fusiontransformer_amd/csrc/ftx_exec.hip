// Native eval-mode executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_eval) and the two row kernels it needs where the
// Python path uses torch (channel concatenation, row-wise add).
//
// The network is a static op program that the host emits once per model (fusiontransformer_amd/native_eval.py) over numbered buffers
// ("slots"); this file validates it against the model and batch tables, places every slot and every per-op temporary in the caller's
// arena, and issues the ops of the requested segments through the library's own per-op entry points -- the same launch code and the
// same order as the Python path, minus the Python.  No state outlives a call; nothing here synchronises or allocates.
#include <string>
#include <vector>
#include "ftx_common.h"
#include "ftx_spvcnn_tables.h"

using namespace ftx;

// ---------------------------------------------------------------- row kernels
// out[r] = a[r] ++ b[r] (channel concatenation); ca, cb multiples of 4, 16-byte accesses
__global__ void rows_concat_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n, int ca, int cb, float *__restrict__ out) {
  const int cv = (ca + cb) >> 2, av = ca >> 2;
  const int64_t total = n * cv;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cv;
    const int j = (int)(e - r * cv);
    const float4 v = j < av ? *(const float4 *)&a[r * ca + 4 * j] : *(const float4 *)&b[r * cb + 4 * (j - av)];
    *(float4 *)&out[e * 4] = v;
  }
}

extern "C" int ftx_rows_concat(const float *a, int32_t ca, const float *b, int32_t cb, int64_t n, float *out, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_rows_concat: n < 0");
  FTX_REQUIRE(ca >= 4 && ca % 4 == 0 && cb >= 4 && cb % 4 == 0, "ftx_rows_concat: channels must be multiples of 4 (ca=%d cb=%d)", ca, cb);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(a && b && out, "ftx_rows_concat: null pointer");
  rows_concat_kernel<<<grid_for(n * ((ca + cb) / 4), 256), 256, 0, (hipStream_t)stream>>>(a, b, n, ca, cb, out);
  return check_launch("ftx_rows_concat");
}

// out = a + b over (n, c) rows, one fp32 add per element; out may be a or b (every element is read before it is written, by its own thread)
__global__ void rows_add_kernel(const float *a, const float *b, int64_t total4, float *out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total4; e += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = *(const float4 *)&a[e * 4];
    const float4 y = *(const float4 *)&b[e * 4];
    *(float4 *)&out[e * 4] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
  }
}

extern "C" int ftx_rows_add(const float *a, const float *b, int64_t n, int32_t c, float *out, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_rows_add: n < 0");
  FTX_REQUIRE(c >= 4 && c % 4 == 0, "ftx_rows_add: channels must be a multiple of 4 (c=%d)", c);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(a && b && out, "ftx_rows_add: null pointer");
  rows_add_kernel<<<grid_for(n * (c / 4), 256), 256, 0, (hipStream_t)stream>>>(a, b, n * (c / 4), out);
  return check_launch("ftx_rows_add");
}

// ---------------------------------------------------------------- tables (layouts documented in include/ftx.h)
namespace {

using Layer = ftx::SpvcnnLayer;   // ftx_spvcnn_tables.h: shared with the training executor
using Op = ftx::SpvcnnOp;
using Map = ftx::SpvcnnMap;   // ftx_spvcnn_tables.h: shared with the index builder that writes them
using PV = ftx::SpvcnnPV;
static_assert(sizeof(Layer) == 80 && sizeof(Op) == 48 && sizeof(Map) == 80 && sizeof(PV) == 64, "table records are packed");

constexpr int kLevels = 6;        // five voxel levels + the point set
constexpr int kMaxSlots = 256;
constexpr int kMaxOps = 4096;
constexpr int64_t kOstatMaxRows = 64 * 4096;
const char *const kKindName[] = {"?", "conv_bn", "linear_bn", "voxelize", "devoxelize", "concat", "add", "add_ext"};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Plan {
  int n_slots = 0;
  std::vector<int> level, ch, def, last, region;
  std::vector<int64_t> region_bytes, region_off, op_temp;
  int64_t temp_off = 0, temp_bytes = 0, total = 0;
};

#define PLAN_REQUIRE(cond, ...)        \
  do {                                 \
    if (!(cond)) {                     \
      set_error(__VA_ARGS__);          \
      return FTX_EINVAL;               \
    }                                  \
  } while (0)

// Validates the program against the tables and places slots and temporaries.  Host only.  Regions are shared by slots of the same
// level whose lifetimes do not overlap; which slots share is decided by the program alone, a region is as large as its largest
// tenant, so the total never shrinks when a row or pair count grows.
int make_plan(const Layer *layers, int32_t n_layers, const Op *ops, int32_t n_ops, const int64_t *rows, const Map *maps, int32_t n_maps,
              const PV *pvs, int32_t n_pvs, const int32_t *routes, Plan &P) {
  const char *who = "ftx_spvcnn_eval";
  PLAN_REQUIRE(ops && rows && routes && n_ops >= 1 && n_ops <= kMaxOps, "%s: null table or op count outside [1, %d]", who, kMaxOps);
  PLAN_REQUIRE(n_layers >= 0 && n_maps >= 0 && n_pvs >= 0 && (layers || !n_layers) && (maps || !n_maps) && (pvs || !n_pvs), "%s: null table", who);
  for (int l = 0; l < kLevels; ++l) PLAN_REQUIRE(rows[l] >= 0 && rows[l] < (1ll << 31), "%s: rows[%d] = %lld out of range", who, l, (long long)rows[l]);
  for (int m = 0; m < n_maps; ++m)
    PLAN_REQUIRE(maps[m].n_pairs >= 0 && maps[m].n_in >= 0 && maps[m].n_out >= 0 && maps[m].n_pairs < (1ll << 31), "%s: map %d has a negative or huge count", who, m);
  P.level.assign(kMaxSlots, -1);
  P.ch.assign(kMaxSlots, -1);
  P.def.assign(kMaxSlots, -1);
  P.last.assign(kMaxSlots, -1);
  P.region.assign(kMaxSlots, -1);
  P.op_temp.assign(n_ops, 0);
  P.level[FTX_SPVCNN_SLOT_INPUT] = 0;   // the voxelised input features; channel count fixed by its first reader
  P.def[FTX_SPVCNN_SLOT_INPUT] = 0;
  int seg = 0;
  auto slot_ok = [](int s) { return s >= 0 && s < kMaxSlots; };
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
    PLAN_REQUIRE(o.kind >= FTX_SPVCNN_OP_CONV_BN && o.kind <= FTX_SPVCNN_OP_ADD_EXT, "%s: op %d: unknown kind %d", who, i, o.kind);
    const char *kn = kKindName[o.kind];
    PLAN_REQUIRE(o.segment >= seg && o.segment <= 2, "%s: op %d (%s): segments must be 0..2 and ascending", who, i, kn);
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
    int second = -1;
    switch (o.kind) {
      case FTX_SPVCNN_OP_CONV_BN:
      case FTX_SPVCNN_OP_LINEAR_BN: {
        PLAN_REQUIRE(o.layer >= 0 && o.layer < n_layers, "%s: op %d (%s): layer %d out of range", who, i, kn, o.layer);
        const Layer &L = layers[o.layer];
        const bool conv = o.kind == FTX_SPVCNN_OP_CONV_BN;
        PLAN_REQUIRE(L.kind == (conv ? FTX_SPVCNN_LAYER_CONV_BN : FTX_SPVCNN_LAYER_LINEAR_BN), "%s: op %d (%s): layer %d is of another kind", who, i, kn, o.layer);
        PLAN_REQUIRE(L.ca >= 4 && L.ca % 4 == 0 && L.co >= 4 && L.co % 4 == 0, "%s: op %d (%s) layer %d: channels must be multiples of 4 (ca=%d co=%d)", who, i,
                     kn, o.layer, L.ca, L.co);
        PLAN_REQUIRE(L.co == o.channels && need_src(o.src, L.ca), "%s: op %d (%s) layer %d: channel counts do not match the slots", who, i, kn, o.layer);
        PLAN_REQUIRE(L.weight && L.gamma && L.beta && L.mean && L.var, "%s: op %d (%s) layer %d: null parameter", who, i, kn, o.layer);
        const int r = routes[i];
        int64_t temp_rows = n_dst;
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
          PLAN_REQUIRE(rows[P.level[o.src]] == m_in && n_dst == m_out, "%s: op %d (%s) layer %d: kernel map %d is (%lld -> %lld), the slots hold (%lld -> %lld)", who,
                       i, kn, o.layer, o.map, (long long)m_in, (long long)m_out, (long long)rows[P.level[o.src]], (long long)n_dst);
          if (r == FTX_SPVCNN_ROUTE_DIRECT) {
            PLAN_REQUIRE(M.fine_bijective && M.n_pairs == n_dst && L.transposed, "%s: op %d (%s) layer %d: the direct route needs a transposed layer on a "
                         "map whose pairs cover every output row once", who, i, kn, o.layer);
            PLAN_REQUIRE(!M.n_pairs || (M.pair_in && M.pair_out && M.koff), "%s: op %d (%s): null pair list in map %d", who, i, kn, o.map);
          } else if (r == FTX_SPVCNN_ROUTE_OSTAT) {
            PLAN_REQUIRE(!L.bf16 && !L.transposed && ftx_spconv_ostat_supported(L.ca, L.co, L.kvol, 0) && n_dst <= kOstatMaxRows && n_dst >= 1 && m_in >= 1,
                         "%s: op %d (%s) layer %d: the output-stationary route does not take this layer", who, i, kn, o.layer);
            PLAN_REQUIRE(M.nbr, "%s: op %d (%s): null neighbour table in map %d", who, i, kn, o.map);
          } else if (r == FTX_SPVCNN_ROUTE_PAIRS || r == FTX_SPVCNN_ROUTE_EMPTY) {
            PLAN_REQUIRE(r == FTX_SPVCNN_ROUTE_PAIRS || M.n_pairs == 0 || n_dst == 0, "%s: op %d (%s) layer %d: the empty route on a map with pairs", who, i, kn,
                         o.layer);
            PLAN_REQUIRE(!n_dst || (L.transposed ? M.pos_t : M.pos), "%s: op %d (%s): null position table in map %d", who, i, kn, o.map);
            PLAN_REQUIRE(!M.n_pairs || ((L.transposed ? M.pair_out : M.pair_in) && M.koff), "%s: op %d (%s): null pair list in map %d", who, i, kn, o.map);
            temp_rows = M.n_pairs;
          } else {
            PLAN_REQUIRE(false, "%s: op %d (%s) layer %d: route %d is not one this entry point takes", who, i, kn, o.layer, r);
          }
        }
        P.op_temp[i] = align256(4 * temp_rows * (int64_t)L.co);
        if (conv && o.src2 >= 0) {
          PLAN_REQUIRE(slot_ok(o.src2) && P.def[o.src2] >= 0 && P.level[o.src2] == o.level && need_src(o.src2, o.channels),
                       "%s: op %d (%s): the residual slot does not match the output", who, i, kn);
          second = o.src2;
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
        PLAN_REQUIRE(need_src(o.src, o.channels), "%s: op %d (%s): channel counts differ", who, i, kn);
        if (vox)
          PLAN_REQUIRE(!V.n_vox || (V.vox_seg_off && (V.vox_order || !rows[plev])), "%s: op %d (%s): null sorted segments in index %d", who, i, kn, o.map);
        else
          PLAN_REQUIRE(!rows[plev] || (V.devox_idx && V.devox_weights), "%s: op %d (%s): null corner table in index %d", who, i, kn, o.map);
        break;
      }
      case FTX_SPVCNN_OP_CONCAT:
      case FTX_SPVCNN_OP_ADD: {
        PLAN_REQUIRE(slot_ok(o.src2) && P.def[o.src2] >= 0 && P.level[o.src] == o.level && P.level[o.src2] == o.level, "%s: op %d (%s): operands of different levels",
                     who, i, kn);
        PLAN_REQUIRE(P.ch[o.src] > 0 && P.ch[o.src2] > 0 && (o.kind == FTX_SPVCNN_OP_ADD ? (P.ch[o.src] == o.channels && P.ch[o.src2] == o.channels)
                                                                                          : P.ch[o.src] + P.ch[o.src2] == o.channels),
                     "%s: op %d (%s): channel counts do not add up", who, i, kn);
        second = o.src2;
        break;
      }
      case FTX_SPVCNN_OP_ADD_EXT:
        PLAN_REQUIRE(o.dst == o.src && (o.layer == 0 || o.layer == 1) && P.level[o.src] == o.level && P.ch[o.src] == o.channels && o.src >= FTX_SPVCNN_SLOT_FIRST,
                     "%s: op %d (%s): the fusion addend is added in place to an arena slot (layer = 0 early, 1 middle)", who, i, kn);
        break;
    }
    if (o.kind != FTX_SPVCNN_OP_ADD_EXT) {
      PLAN_REQUIRE(o.dst != FTX_SPVCNN_SLOT_INPUT && P.def[o.dst] < 0, "%s: op %d (%s): slot %d is written twice", who, i, kn, o.dst);
      PLAN_REQUIRE(o.dst != FTX_SPVCNN_SLOT_OUTPUT || o.level == kLevels - 1, "%s: op %d (%s): the output slot holds point rows", who, i, kn);
      P.def[o.dst] = i;
      P.level[o.dst] = o.level;
      P.ch[o.dst] = o.channels;
    }
    P.last[o.src] = i;
    if (second >= 0) P.last[second] = i;
    if (P.last[o.dst] < i) P.last[o.dst] = i;
  }
  // regions: per level, the lowest-numbered free one; a slot's region is free again after its last reader
  std::vector<std::vector<int>> free_regions(kLevels);
  std::vector<std::vector<int>> dying(n_ops);
  for (int s = FTX_SPVCNN_SLOT_FIRST; s < kMaxSlots; ++s)
    if (P.def[s] >= 0) dying[P.last[s]].push_back(s);
  for (int i = 0; i < n_ops; ++i) {
    const Op &o = ops[i];
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
      const int64_t b = align256(4 * rows[o.level] * (int64_t)o.channels);
      if (b > P.region_bytes[reg]) P.region_bytes[reg] = b;
    }
    for (int s : dying[i]) free_regions[P.level[s]].push_back(P.region[s]);
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

int fail(int i, const Op &o, int rc) {
  const std::string inner = ftx_last_error();
  set_error("ftx_spvcnn_eval: op %d (%s, layer %d): %s", i, kKindName[o.kind], o.kind <= FTX_SPVCNN_OP_LINEAR_BN ? o.layer : -1, inner.c_str());
  return rc;
}

}  // namespace

extern "C" int32_t ftx_spvcnn_layer_bytes(void) { return (int32_t)sizeof(Layer); }
extern "C" int32_t ftx_spvcnn_op_bytes(void) { return (int32_t)sizeof(Op); }
extern "C" int32_t ftx_spvcnn_map_bytes(void) { return (int32_t)sizeof(Map); }
extern "C" int32_t ftx_spvcnn_pv_bytes(void) { return (int32_t)sizeof(PV); }

extern "C" size_t ftx_spvcnn_eval_arena_bytes(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host,
                                              const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host) {
  Plan P;
  if (make_plan((const Layer *)layers_host, n_layers, (const Op *)ops_host, n_ops, rows_host, (const Map *)maps_host, n_maps, (const PV *)pvs_host, n_pvs,
                routes_host, P) != FTX_OK)
    return 0;
  return (size_t)P.total;
}

extern "C" int ftx_spvcnn_eval(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host,
                               const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const float *x0,
                               int32_t first_segment, int32_t last_segment, const float *add_early, const float *add_middle, void *arena,
                               size_t arena_bytes, float *out, void *stream) {
  const Layer *layers = (const Layer *)layers_host;
  const Op *ops = (const Op *)ops_host;
  const Map *maps = (const Map *)maps_host;
  const PV *pvs = (const PV *)pvs_host;
  Plan P;
  int rc = make_plan(layers, n_layers, ops, n_ops, rows_host, maps, n_maps, pvs, n_pvs, routes_host, P);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(first_segment >= 0 && first_segment <= last_segment && last_segment <= 2, "ftx_spvcnn_eval: segments [%d, %d] outside 0..2", first_segment,
              last_segment);
  FTX_REQUIRE(arena && ((uintptr_t)arena & 255) == 0, "ftx_spvcnn_eval: the arena must be a 256-byte aligned device buffer");
  if (arena_bytes < (size_t)P.total) {
    set_error("ftx_spvcnn_eval: arena %zu < required %zu (ftx_spvcnn_eval_arena_bytes)", arena_bytes, (size_t)P.total);
    return FTX_EWORKSPACE;
  }
  const int64_t *rows = rows_host;
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
#define RUN(call)                           \
  do {                                      \
    rc = (call);                            \
    if (rc != FTX_OK) return fail(i, o, rc); \
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
        const Layer &L = layers[o.layer];
        const float *res = o.src2 >= 0 ? at(o.src2) : nullptr;
        const int64_t rows_a = rows[P.level[o.src]];
        if (L.kvol == 1) {
          RUN((L.bf16 ? ftx_rows_gemm_bf16 : ftx_rows_gemm)(src, n, L.weight, 0, nullptr, L.ca, L.co, temp, stream));
          RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
          break;
        }
        const Map &M = maps[o.map];
        const int32_t *gather = L.transposed ? M.pair_out : M.pair_in, *scatter = L.transposed ? M.pair_in : M.pair_out;
        const int32_t *dst_pos = L.transposed ? M.pos_t : M.pos;
        switch (routes_host[i]) {
          case FTX_SPVCNN_ROUTE_DIRECT:
            RUN((L.bf16 ? ftx_spconv_pairs_gemm_scatter_bf16 : ftx_spconv_pairs_gemm_scatter)(src, rows_a, gather, scatter, L.weight, 0, M.koff, M.n_pairs, L.ca,
                                                                                              L.co, L.kvol, temp, n, stream));
            RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
            break;
          case FTX_SPVCNN_ROUTE_OSTAT:
            RUN(ftx_spconv_ostat(src, rows_a, M.nbr, n, L.weight, 0, 0, L.ca, L.co, L.kvol, temp, nullptr, 0, stream));
            RUN(ftx_bn_eval_fwd(temp, res, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
            break;
          default:   // pairs, or the empty map (no pair rows: every output row reduces to zero before the BatchNorm)
            RUN((L.bf16 ? ftx_spconv_pairs_gemm_bf16 : ftx_spconv_pairs_gemm)(src, rows_a, gather, L.weight, 0, M.koff, M.n_pairs, L.ca, L.co, L.kvol, temp,
                                                                              stream));
            RUN(ftx_spconv_reduce_bn_eval(temp, dst_pos, n, L.co, L.kvol, res, L.gamma, L.beta, L.mean, L.var, L.eps, o.relu, dst, stream));
            break;
        }
        break;
      }
      case FTX_SPVCNN_OP_LINEAR_BN: {
        const Layer &L = layers[o.layer];
        RUN((L.bf16 ? ftx_rows_gemm_bf16 : ftx_rows_gemm)(src, n, L.weight, 1, L.bias, L.ca, L.co, temp, stream));
        RUN(ftx_bn_eval_fwd(temp, nullptr, L.gamma, L.beta, L.mean, L.var, L.eps, n, L.co, o.relu, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_VOXELIZE: {
        const PV &V = pvs[o.map];
        RUN(ftx_voxelize_fwd_sorted(src, V.vox_order, V.vox_seg_off, rows[kLevels - 1], o.channels, n, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_DEVOXELIZE: {
        const PV &V = pvs[o.map];
        RUN(ftx_devoxelize_fwd(src, V.devox_idx, V.devox_weights, n, o.channels, V.n_vox, dst, stream));
        break;
      }
      case FTX_SPVCNN_OP_CONCAT:
        RUN(ftx_rows_concat(src, P.ch[o.src], at(o.src2), P.ch[o.src2], n, dst, stream));
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
