// Native index build of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_index_levels / _maps / _pairs): everything of a batch that
// depends on its coordinates only -- what SPVCNN._index_steps(ahead=True) chains together from ~20 entry points -- in three calls with
// one host read between them (all level sizes, then the five submanifold pair counts).
//
// The per-level entry points launch a handful of latency-bound kernels per level, five (or nine, or three) times over.  Here every
// repeated step is ONE launch over all its instances: a descriptor passed by value (kernel arguments; at most twelve instances, so no
// table has to be copied to the device) gives each instance its pointers, sizes and the first element it owns in the launch's
// flat index space.  The dependent chain then has the depth of one level.  The arithmetic of every step is the per-level kernel's
// (ftx_index.hip, ftx_spconv.hip, ftx_pointvoxel.hip) because both call the same element functions (ftx_index_ops.h), so the outputs
// are equal bit for bit: smallest row wins for duplicate keys in the hash table, pair lists are in (k, o) order.  What is this
// file's own is which instance an element belongs to, where its arrays lie, and the validity scan over all maps at once.
//
// Memory: three caller-owned arenas, one per phase, each sized by a host-only function from the values known when the phase is
// issued (A: n; B: n, c_in and the level sizes; C: the level sizes and the pair counts).  Every region is 256-byte aligned.
// Temporaries (sort and scan workspaces) are the tail of arenas A and B.
#include <cstring>
#include "ftx_index_ops.h"
#include "ftx_spvcnn_tables.h"
#include <rocprim/device/device_radix_sort.hpp>

using namespace ftx;

namespace {

constexpr int kNL = 5;                        // voxel levels, strides 1, 2, 4, 8, 16
constexpr int kNM = 9;                        // kernel maps: the 3^3 map of every level, then the strided 2^3 map between consecutive levels
constexpr int kNPV = 3;                       // strides at which points and voxels exchange features
constexpr int kStride[kNL] = {1, 2, 4, 8, 16};
constexpr int kPvLevel[kNPV] = {0, 4, 2};     // strides 1, 16, 4: the order of native_eval.PV_STRIDES
constexpr int kScanChunk = 4096;              // elements per block of the validity scan (256 threads x 16)
constexpr int kLayoutWords = 105;

struct Lay {
  int64_t n = 0, c = 0;
  int64_t nl[kNL] = {}, off[kNL + 1] = {}, cap[kNL] = {}, pairs[kNL] = {};
  // arena A
  int64_t a_coords = 0, a_points = 0, a_uniq = 0, a_first = 0, a_skeys = 0, a_order = 0, a_level_off = 0, a_ws = 0, a_ws_bytes = 0, a_total = 0;
  // arena B
  int64_t b_coords[kNL] = {}, b_tkeys[kNL] = {}, b_tvals[kNL] = {}, b_x0 = 0;
  int64_t map_start[kNM + 1] = {}, map_nout[kNM] = {}, map_nin[kNM] = {};   // element offsets of every map in the nbr / pos regions
  int map_k[kNM] = {};
  int64_t b_nbr = 0, b_pos = 0, b_koff[kNM] = {}, b_mapbase = 0, b_paircounts = 0;
  int64_t b_pos_t2 = 0, b_pos_t2_bytes = 0, pos_t2[4] = {}, pair_in2[4] = {}, pair_out2[4] = {};
  int64_t vidx[kNPV] = {}, b_vcnt = 0, b_vcnt_bytes = 0, vcnt[kNPV] = {}, vseg[kNPV] = {}, didx[kNPV] = {}, dw[kNPV] = {}, dorder[kNPV] = {}, dseg[kNPV] = {};
  int64_t b_bsum = 0, n_blocks = 0, b_skin = 0, b_skout = 0, b_svin = 0, b_stmp = 0, b_stmp_bytes = 0, b_total = 0;
  // arena C
  int64_t c_pos_t = 0, c_pos_t_bytes = 0, pos_t3[kNL] = {}, pair_in3[kNL] = {}, pair_out3[kNL] = {}, c_total = 0;
};

#define LAY_REQUIRE(cond, ...)   \
  do {                           \
    if (!(cond)) {               \
      set_error(__VA_ARGS__);    \
      return FTX_EINVAL;         \
    }                            \
  } while (0)

// Host only.  `off` (6 level offsets as phase A reports them) and `pairs` (5 pair counts as phase B reports them) may be null: the
// arenas that depend on them are then left out.
int make_layout(const char *who, int64_t n, int32_t c_in, const int32_t *off, const int32_t *pairs, int with_bwd, Lay &L) {
  LAY_REQUIRE(n >= 1, "%s: n < 1", who);
  LAY_REQUIRE(n * 24 < 0x7fffffff, "%s: n = %lld is too large for int32 rows", who, (long long)n);
  L.n = n;
  L.c = c_in;
  Offsets256 o;
  const int64_t m = n * kNL;
  L.a_coords = o.take(16 * n);
  L.a_points = o.take(16 * n);
  L.a_uniq = o.take(8 * m);
  L.a_first = o.take(4 * m);
  L.a_skeys = o.take(8 * m);
  L.a_order = o.take(4 * m);
  L.a_level_off = o.take(256);
  // ftx_levels_unique's workspace: keys, sorted keys, two value arrays (24 B per key) and the sort / unique temporaries, which no host-only
  // formula gives exactly; this bound is checked against ftx_levels_workspace_bytes when the phase is issued (FTX_EWORKSPACE if it falls short)
  L.a_ws_bytes = align256(40 * m + (4 << 20));
  L.a_ws = o.take(L.a_ws_bytes);
  L.a_total = o.end;
  if (!off) return FTX_OK;

  LAY_REQUIRE(c_in >= 4 && c_in % 4 == 0 && c_in <= 1024, "%s: c_in = %d must be a multiple of 4 in [4, 1024]", who, c_in);
  LAY_REQUIRE(off[0] == 0, "%s: level offsets must start at 0", who);
  for (int l = 0; l < kNL; ++l) {
    const int64_t sz = (int64_t)off[l + 1] - off[l];
    LAY_REQUIRE(sz >= 1 && sz <= n, "%s: level %d has %lld voxels (1 .. n = %lld)", who, l, (long long)sz, (long long)n);
    LAY_REQUIRE(l == 0 || sz <= L.nl[l - 1], "%s: level %d has more voxels (%lld) than the finer level (%lld)", who, l, (long long)sz, (long long)L.nl[l - 1]);
    L.nl[l] = sz;
    L.off[l] = off[l];
    L.cap[l] = ftx_hashtable_capacity(sz);
  }
  L.off[kNL] = off[kNL];
  o = Offsets256();
  for (int l = 0; l < kNL; ++l) {
    L.b_coords[l] = o.take(16 * L.nl[l]);
    L.b_tkeys[l] = o.take(8 * L.cap[l]);
    L.b_tvals[l] = o.take(4 * L.cap[l]);
  }
  L.b_x0 = o.take(4 * L.nl[0] * c_in);
  int64_t e = 0;
  for (int mi = 0; mi < kNM; ++mi) {
    const bool sub = mi < kNL;
    L.map_k[mi] = sub ? 27 : 8;
    L.map_nin[mi] = sub ? L.nl[mi] : L.nl[mi - kNL];
    L.map_nout[mi] = sub ? L.nl[mi] : L.nl[mi - kNL + 1];
    L.map_start[mi] = e;
    e += (L.map_k[mi] * L.map_nout[mi] + 63) & ~(int64_t)63;   // every map starts on a 256-byte boundary; the padding is "no neighbour"
  }
  L.map_start[kNM] = e;
  LAY_REQUIRE(e < 0x7fffffff, "%s: the kernel maps have too many entries for int32 positions", who);
  L.b_nbr = o.take(4 * e);
  L.b_pos = o.take(4 * e);
  for (int mi = 0; mi < kNM; ++mi) L.b_koff[mi] = o.take(4 * (L.map_k[mi] + 1));
  L.b_mapbase = o.take(4 * 16);
  L.b_paircounts = o.take(4 * 16);
  L.b_pos_t2 = o.end;
  for (int i = 0; i < 4; ++i) L.pos_t2[i] = o.take(4 * 8 * L.nl[i]);
  L.b_pos_t2_bytes = o.end - L.b_pos_t2;
  for (int i = 0; i < 4; ++i) {
    L.pair_in2[i] = o.take(4 * L.nl[i]);
    L.pair_out2[i] = o.take(4 * L.nl[i]);
  }
  for (int j = 0; j < kNPV; ++j) L.vidx[j] = o.take(4 * n);
  L.b_vcnt = o.end;
  for (int j = 0; j < kNPV; ++j) L.vcnt[j] = o.take(4 * L.nl[kPvLevel[j]]);
  L.b_vcnt_bytes = o.end - L.b_vcnt;
  for (int j = 0; j < kNPV; ++j) {
    L.vseg[j] = o.take(4 * (L.nl[kPvLevel[j]] + 1));
    L.didx[j] = o.take(32 * n);
    L.dw[j] = o.take(32 * n);
  }
  if (with_bwd) {
    const int64_t d = o.take(4 * 8 * n * kNPV);      // the three sorted entry lists back to back: one sort writes them
    for (int j = 0; j < kNPV; ++j) {
      L.dorder[j] = d + 32 * n * j;
      L.dseg[j] = o.take(4 * (L.nl[kPvLevel[j]] + 1));
    }
  }
  L.n_blocks = ceil_div(e, kScanChunk);
  L.b_bsum = o.take(4 * L.n_blocks);
  if (with_bwd) {
    const int64_t ne = 8 * n * kNPV;
    L.b_skin = o.take(4 * ne);
    L.b_skout = o.take(4 * ne);
    L.b_svin = o.take(4 * ne);
    // radix sort temporaries: bounded like arena A's, checked against rocprim's own figure when the phase is issued
    L.b_stmp_bytes = align256(12 * ne + (4 << 20));
    L.b_stmp = o.take(L.b_stmp_bytes);
  }
  L.b_total = o.end;
  if (!pairs) return FTX_OK;

  o = Offsets256();
  for (int l = 0; l < kNL; ++l) {
    LAY_REQUIRE(pairs[l] >= 0 && pairs[l] <= 27 * L.nl[l], "%s: level %d: %d pairs is outside 0 .. 27 * %lld", who, l, pairs[l], (long long)L.nl[l]);
    L.pairs[l] = pairs[l];
  }
  L.c_pos_t = o.end;
  for (int l = 0; l < kNL; ++l) L.pos_t3[l] = o.take(4 * 27 * L.nl[l]);
  L.c_pos_t_bytes = o.end - L.c_pos_t;
  for (int l = 0; l < kNL; ++l) {
    L.pair_in3[l] = o.take(4 * L.pairs[l]);
    L.pair_out3[l] = o.take(4 * L.pairs[l]);
  }
  L.c_total = o.end < 256 ? 256 : o.end;
  return FTX_OK;
}

void export_layout(const Lay &L, int64_t *w) {
  int i = 0;
  w[i++] = L.a_total; w[i++] = L.b_total; w[i++] = L.c_total;
  w[i++] = L.a_coords; w[i++] = L.a_points; w[i++] = L.a_uniq; w[i++] = L.a_first; w[i++] = L.a_skeys; w[i++] = L.a_order;
  for (int l = 0; l < kNL; ++l) { w[i++] = L.b_coords[l]; w[i++] = L.b_tkeys[l]; w[i++] = L.b_tvals[l]; w[i++] = L.cap[l]; }
  w[i++] = L.b_x0;
  for (int m = 0; m < kNM; ++m) { w[i++] = L.b_nbr + 4 * L.map_start[m]; w[i++] = L.b_pos + 4 * L.map_start[m]; w[i++] = L.b_koff[m]; }
  for (int m = 0; m < 4; ++m) { w[i++] = L.pos_t2[m]; w[i++] = L.pair_in2[m]; w[i++] = L.pair_out2[m]; }
  for (int j = 0; j < kNPV; ++j) { w[i++] = L.vidx[j]; w[i++] = L.vcnt[j]; w[i++] = L.vseg[j]; w[i++] = L.didx[j]; w[i++] = L.dw[j]; w[i++] = L.dorder[j]; w[i++] = L.dseg[j]; }
  for (int l = 0; l < kNL; ++l) { w[i++] = L.pos_t3[l]; w[i++] = L.pair_in3[l]; w[i++] = L.pair_out3[l]; }
  static_assert(3 + 6 + 4 * kNL + 1 + 3 * kNM + 12 + 7 * kNPV + 3 * kNL == kLayoutWords, "layout words");
}

// ---------------------------------------------------------------- phase A: rescale + floor
// new_float_coord of initial_voxelize: (x * init_res) / after_res in float32, where the division by a host scalar is the multiplication
// by its float32 reciprocal that the tensor library performs; then floor_coords(., 1)
__global__ void nx_rescale_floor_kernel(const float4 *__restrict__ pc, int64_t n, int rescale, float mul, float inv, float4 *__restrict__ zc,
                                        int4 *__restrict__ pts) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float4 p = pc[i];
    if (rescale) {
      p.x = __fmul_rn(__fmul_rn(p.x, mul), inv);
      p.y = __fmul_rn(__fmul_rn(p.y, mul), inv);
      p.z = __fmul_rn(__fmul_rn(p.z, mul), inv);
      zc[i] = p;
    }
    pts[i] = floor_point(p, 1);
  }
}

// ---------------------------------------------------------------- phase B kernels
struct LevelsDesc {
  const int4 *pts;
  const int32_t *first;     // first-occurrence point rows of all levels back to back (ftx_levels_unique)
  const int64_t *uniq;      // their hashes, same order
  int4 *coords[kNL];
  int64_t *tk[kNL];
  int32_t *tv[kNL];
  int64_t cap[kNL];
  int64_t off[kNL + 1];     // first voxel of each level in the concatenation
  int64_t cap_off[kNL + 1]; // first slot of each level's table in the concatenation of all tables
  int32_t stride[kNL];
  int32_t n_points;
};

__device__ inline int nx_find(const int64_t *starts, int count, int64_t e) {
  int l = 0;
  for (int i = 1; i < count; ++i) l += e >= starts[i] ? 1 : 0;
  return l;
}

__global__ void nx_table_init_kernel(LevelsDesc D) {
  const int64_t total = D.cap_off[kNL];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = nx_find(D.cap_off, kNL, e);
    const int64_t s = e - D.cap_off[l];
    D.tk[l][s] = kEmptyKey;
    D.tv[l][s] = 0x7fffffff;
  }
}

// per voxel of every level: its coordinates (level_coords_kernel) and its entry in the level's hash table (table_insert_kernel)
__global__ void nx_levels_kernel(LevelsDesc D) {
  const int64_t total = D.off[kNL];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = nx_find(D.off, kNL, e);
    const int64_t r = e - D.off[l];
    const int stride = D.stride[l];
    int32_t f = D.first[e];
    f = f < 0 ? 0 : (f >= D.n_points ? D.n_points - 1 : f);   // a true first-occurrence row is inside; offsets that are not phase A's must not read outside
    D.coords[l][r] = level_coord(D.pts[f], stride);
    table_insert(D.uniq[e], (int32_t)r, D.tk[l], D.tv[l], D.cap[l]);
  }
}

struct PvDesc {
  const float4 *zc;
  int64_t n;
  const int64_t *tk[kNPV];
  const int32_t *tv[kNPV];
  int64_t cap[kNPV], m[kNPV];
  int32_t stride[kNPV], level[kNPV];
  int32_t *vidx[kNPV], *vcnt[kNPV], *vseg[kNPV], *didx[kNPV];
  float *dw[kNPV];
  const int64_t *skeys[kNPV];   // the level's row of ftx_levels_unique's sorted keys
  const int64_t *uniq[kNPV];    // the level's hashes
  int64_t seg_start[kNPV + 1];  // first element of each instance among the sum of (m + 1) segment offsets
  // backward segments
  int32_t *keys_in, *vals_in;
  const int32_t *keys_out;
  int32_t *dseg[kNPV];
  int64_t kbase[kNPV];
};

// point -> voxel row at every stride (sphash(floor_coords) + hash query) and the points per voxel (ftx_count; the counts are zeroed before)
__global__ void nx_point_query_kernel(PvDesc D) {
  const int64_t total = D.n * kNPV;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / D.n);
    const int64_t i = e - (int64_t)j * D.n;
    const int4 c = floor_point(D.zc[i], D.stride[j]);
    const int32_t r = table_lookup(fnv_hash4(c.x, c.y, c.z, c.w), D.tk[j], D.tv[j], D.cap[j]);
    D.vidx[j][i] = r;
    if (r >= 0 && r < D.m[j]) atomicAdd(&D.vcnt[j][r], 1);
  }
}

// level_segments_kernel for the three strides
__global__ void nx_level_segments_kernel(PvDesc D) {
  const int64_t total = D.seg_start[kNPV];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = nx_find(D.seg_start, kNPV, e);
    const int64_t v = e - D.seg_start[j], m = D.m[j];
    if (v == m) { D.vseg[j][m] = (int32_t)D.n; continue; }
    D.vseg[j][v] = (int32_t)lower_bound(D.skeys[j], D.n, level_key(D.level[j], D.uniq[j][v]));
  }
}

// One neighbour table per instance (kernel_map_kernel): the 3^3 map of every level, the 2^3 map between consecutive levels, and the
// 8 corner rows of every point at the three strides (written point-major, the transposed form voxel_to_point keeps).
struct NbrInst {
  const void *src;          // int4 rows (maps) or float4 points (corners)
  const int64_t *tk;
  const int32_t *tv;
  int32_t *out;
  int64_t cap, rows, start, valid;   // `valid` = k * rows entries, the rest up to the next instance's start is padding
  int32_t k, stride, corners, reserved;
};
struct NbrDesc {
  NbrInst inst[kNM + kNPV];
  int64_t starts[kNM + kNPV + 1];
};

__global__ void nx_nbr_kernel(NbrDesc D) {
  const int64_t total = D.starts[kNM + kNPV];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int t = nx_find(D.starts, kNM + kNPV, e);
    const NbrInst &I = D.inst[t];
    const int64_t loc = e - I.start;
    if (loc >= I.valid) { I.out[loc] = -1; continue; }
    int kk;
    int4 c;
    if (I.corners) {
      kk = (int)(loc & 7);
      c = floor_point(((const float4 *)I.src)[loc >> 3], I.stride);
    } else {
      kk = (int)(loc / I.rows);
      c = ((const int4 *)I.src)[loc - (int64_t)kk * I.rows];
    }
    int dx, dy, dz;
    kernel_offset(I.k, kk, I.stride, dx, dy, dz);
    I.out[loc] = table_lookup(fnv_hash4(c.x + dx, c.y + dy, c.z + dz, c.w), I.tk, I.tv, I.cap);
  }
}

// trilinear_kernel for the three strides
__global__ void nx_trilinear_kernel(PvDesc D) {
  const int64_t total = D.n * kNPV;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / D.n);
    const int64_t i = e - (int64_t)j * D.n;
    trilinear_row(D.zc[i], D.didx[j] + i * 8, D.stride[j], D.dw[j] + i * 8);
  }
}

// ---- validity scan over the nine neighbour tables laid end to end: pos[e] = number of present neighbours before e.  Integer sums, so
// the three-kernel form (block totals, their scan, the scan inside each block) gives what one exclusive scan per map gives, shifted by
// the map's base pos[map_start], which nx_koff_kernel records and the compaction takes off again.
__global__ __launch_bounds__(256) void nx_scan_totals_kernel(const int32_t *__restrict__ nbr, int64_t total, int32_t *__restrict__ bsum) {
  __shared__ int s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + threadIdx.x * 16;
  int cnt = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t at = base + g * 4;
    if (at + 4 <= total) {
      const int4 v = *(const int4 *)&nbr[at];
      cnt += (v.x >= 0) + (v.y >= 0) + (v.z >= 0) + (v.w >= 0);
    }
  }
  atomicAdd(&s_sum, cnt);
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_sum;
}

// exclusive scan of 256 values held one per thread; returns the exclusive prefix, *total gets the sum
__device__ inline int nx_block_exclusive(int v, int *lds, int *total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const int incl = lds[t];
  *total = lds[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void nx_scan_blocks_kernel(int32_t *__restrict__ bsum, int64_t nb) {
  __shared__ int lds[256];
  int carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t at = base + threadIdx.x;
    const int v = at < nb ? bsum[at] : 0;
    int tot;
    const int ex = nx_block_exclusive(v, lds, &tot);
    if (at < nb) bsum[at] = carry + ex;
    carry += tot;
  }
}

__global__ __launch_bounds__(256) void nx_scan_write_kernel(const int32_t *__restrict__ nbr, int64_t total, const int32_t *__restrict__ bsum,
                                                            int32_t *__restrict__ pos) {
  __shared__ int lds[256];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + threadIdx.x * 16;
  int4 v[4];
  int cnt = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t at = base + g * 4;
    v[g] = at + 4 <= total ? *(const int4 *)&nbr[at] : make_int4(-1, -1, -1, -1);
    cnt += (v[g].x >= 0) + (v[g].y >= 0) + (v[g].z >= 0) + (v[g].w >= 0);
  }
  int tot;
  int run = bsum[blockIdx.x] + nx_block_exclusive(cnt, lds, &tot);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t at = base + g * 4;
    int4 p;
    p.x = run; run += v[g].x >= 0;
    p.y = run; run += v[g].y >= 0;
    p.z = run; run += v[g].z >= 0;
    p.w = run; run += v[g].w >= 0;
    if (at + 4 <= total) *(int4 *)&pos[at] = p;
  }
}

struct MapsDesc {
  const int32_t *nbr;       // all maps, map m from element start[m]
  int32_t *pos;
  int32_t *koff[kNM];
  int32_t *pos_t[kNM], *pair_in[kNM], *pair_out[kNM];
  int64_t start[kNM + 1], n_out[kNM], n_in[kNM], cap[kNM];
  int32_t k[kNM];
  int32_t *mapbase;         // [kNM] pos at the first element of each map
  int32_t *paircounts;      // [kNL] pairs of the five 3^3 maps, read back by the host
};

// koff_kernel for all maps, relative to each map's base
__global__ void nx_koff_kernel(MapsDesc D) {
  const int t = threadIdx.x;
  const int m = t / 28, kk = t - m * 28;
  if (m >= kNM || kk > D.k[m]) return;
  const int64_t s = D.start[m];
  const int32_t base = D.pos[s];
  const int32_t v = koff_entry(D.nbr + s, D.pos + s, D.n_out[m], D.k[m], kk, base);
  D.koff[m][kk] = v;
  if (kk == 0) D.mapbase[m] = base;
  if (kk == D.k[m] && m < kNL) D.paircounts[m] = v;
}

// pairs_scatter_kernel for maps [first, first + count): pos turns from the scan into the position in the map's own pair list (or -1)
__global__ void nx_pairs_kernel(MapsDesc D, int first, int count) {
  const int64_t begin = D.start[first], total = D.start[first + count];
  for (int64_t e = begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int m = first + nx_find(D.start + first, count, e);
    const int64_t loc = e - D.start[m], n_out = D.n_out[m], n_in = D.n_in[m];
    if (loc >= D.k[m] * n_out) continue;      // padding
    D.pos[e] = pair_entry(D.nbr[e], D.pos[e] - D.mapbase[m], loc, n_out, n_in, D.cap[m], D.pair_in[m], D.pair_out[m], D.pos_t[m]);
  }
}

// ---- the devoxelise backward's segments: the (point, corner) entries of each stride sorted by voxel, zero-weight corners dropped
// (devoxelize_segments + ftx_segment_build).  The three key sets are shifted into disjoint ranges and sorted in one stable radix sort;
// seg_off is the lower bound of every voxel in its instance's sorted keys (= the exclusive scan of the per-voxel counts).
__global__ void nx_dseg_prepare_kernel(PvDesc D) {
  const int64_t per = D.n * 8, total = per * kNPV;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / per);
    const int64_t i = e - (int64_t)j * per;
    const int32_t k = D.dw[j][i] != 0.f ? D.didx[j][i] : -1;
    D.keys_in[e] = (int32_t)(D.kbase[j] + segment_key(k, D.m[j]));   // dropped entries sort to the end of their instance
    D.vals_in[e] = (int32_t)i;
  }
}

__global__ void nx_dseg_offsets_kernel(PvDesc D) {
  const int64_t total = D.seg_start[kNPV], per = D.n * 8;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = nx_find(D.seg_start, kNPV, e);
    const int64_t v = e - D.seg_start[j];
    D.dseg[j][v] = (int32_t)lower_bound(D.keys_out + (int64_t)j * per, per, (int32_t)(D.kbase[j] + v));
  }
}

bool aligned256(const void *p) { return p && ((uintptr_t)p & 255) == 0; }

unsigned dseg_bits(const Lay &L) {
  int64_t range = 0;
  for (int j = 0; j < kNPV; ++j) range += L.nl[kPvLevel[j]] + 1;
  unsigned bits = 1;
  while ((1ll << bits) <= range - 1) ++bits;
  return bits;
}

}  // namespace

// ---------------------------------------------------------------- host-only size and layout queries
extern "C" int32_t ftx_spvcnn_index_layout_words(void) { return kLayoutWords; }

extern "C" int ftx_spvcnn_index_layout(int64_t n, int32_t c_in, const int32_t *level_off_host, const int32_t *pair_counts_host,
                                       int32_t with_backward_segments, int64_t *words_host) {
  FTX_REQUIRE(words_host, "ftx_spvcnn_index_layout: null output");
  FTX_REQUIRE(level_off_host || !pair_counts_host, "ftx_spvcnn_index_layout: pair counts without level offsets");
  Lay L;
  int rc = make_layout("ftx_spvcnn_index_layout", n, c_in, level_off_host, pair_counts_host, with_backward_segments, L);
  if (rc != FTX_OK) return rc;
  export_layout(L, words_host);
  return FTX_OK;
}

extern "C" size_t ftx_spvcnn_index_levels_arena_bytes(int64_t n) {
  Lay L;
  if (make_layout("ftx_spvcnn_index_levels_arena_bytes", n, 4, nullptr, nullptr, 0, L) != FTX_OK) return 0;
  return (size_t)L.a_total;
}

extern "C" size_t ftx_spvcnn_index_maps_arena_bytes(int64_t n, int32_t c_in, const int32_t *level_off_host, int32_t with_backward_segments) {
  Lay L;
  if (!level_off_host) {
    set_error("ftx_spvcnn_index_maps_arena_bytes: null level offsets");
    return 0;
  }
  if (make_layout("ftx_spvcnn_index_maps_arena_bytes", n, c_in, level_off_host, nullptr, with_backward_segments, L) != FTX_OK) return 0;
  return (size_t)L.b_total;
}

extern "C" size_t ftx_spvcnn_index_pairs_arena_bytes(int64_t n, const int32_t *level_off_host, const int32_t *pair_counts_host) {
  Lay L;
  if (!level_off_host || !pair_counts_host) {
    set_error("ftx_spvcnn_index_pairs_arena_bytes: null level offsets / pair counts");
    return 0;
  }
  if (make_layout("ftx_spvcnn_index_pairs_arena_bytes", n, 4, level_off_host, pair_counts_host, 0, L) != FTX_OK) return 0;
  return (size_t)L.c_total;
}

// ---------------------------------------------------------------- phase A
extern "C" int ftx_spvcnn_index_levels(const float *coords, int64_t n, float init_res, float after_res, void *arena_a, size_t arena_a_bytes,
                                       int32_t *level_off_pinned, void *stream) {
  const char *who = "ftx_spvcnn_index_levels";
  Lay L;
  int rc = make_layout(who, n, 4, nullptr, nullptr, 0, L);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(coords && level_off_pinned, "%s: null pointer", who);
  FTX_REQUIRE(((uintptr_t)coords & 15) == 0, "%s: the coordinates must be 16-byte aligned", who);
  FTX_REQUIRE(init_res > 0.f && after_res > 0.f, "%s: resolutions must be positive", who);
  FTX_REQUIRE(aligned256(arena_a), "%s: the arena must be a 256-byte aligned device buffer", who);
  if (arena_a_bytes < (size_t)L.a_total) {
    set_error("%s: arena %zu < required %zu (ftx_spvcnn_index_levels_arena_bytes)", who, arena_a_bytes, (size_t)L.a_total);
    return FTX_EWORKSPACE;
  }
  const size_t ws_need = ftx_levels_workspace_bytes(n, kNL);
  if (ws_need == 0 || ws_need > (size_t)L.a_ws_bytes) {
    set_error("%s: the level sort needs %zu workspace bytes, the arena reserves %zu", who, ws_need, (size_t)L.a_ws_bytes);
    return FTX_EWORKSPACE;
  }
  // everything above answered on the host; from here on launches only
  hipStream_t st = (hipStream_t)stream;
  char *A = (char *)arena_a;
  const int rescale = init_res != after_res;
  nx_rescale_floor_kernel<<<grid_for(n, 256), 256, 0, st>>>((const float4 *)coords, n, rescale, init_res, 1.0f / after_res, (float4 *)(A + L.a_coords),
                                                           (int4 *)(A + L.a_points));
  int32_t strides[kNL];
  for (int l = 0; l < kNL; ++l) strides[l] = kStride[l];
  int32_t *level_off = (int32_t *)(A + L.a_level_off);
  rc = ftx_levels_unique((const int32_t *)(A + L.a_points), n, strides, kNL, (int64_t *)(A + L.a_uniq), (int32_t *)(A + L.a_first), level_off,
                         (int64_t *)(A + L.a_skeys), (int32_t *)(A + L.a_order), A + L.a_ws, (size_t)L.a_ws_bytes, stream);
  if (rc != FTX_OK) return rc;
  if (hipMemcpyAsync(level_off_pinned, level_off, sizeof(int32_t) * (kNL + 1), hipMemcpyDeviceToHost, st) != hipSuccess) return check_launch(who);
  return check_launch(who);
}

// ---------------------------------------------------------------- phase B
extern "C" int ftx_spvcnn_index_maps(const float *coords, int64_t n, float init_res, float after_res, const float *feats, int32_t c_in,
                                     const int32_t *level_off_host, int32_t with_backward_segments, void *arena_a, size_t arena_a_bytes,
                                     void *arena_b, size_t arena_b_bytes, int32_t *pair_counts_pinned, void *stream) {
  const char *who = "ftx_spvcnn_index_maps";
  FTX_REQUIRE(level_off_host, "%s: null level offsets", who);
  Lay L;
  int rc = make_layout(who, n, c_in, level_off_host, nullptr, with_backward_segments, L);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(coords && feats && pair_counts_pinned, "%s: null pointer", who);
  FTX_REQUIRE((((uintptr_t)coords | (uintptr_t)feats) & 15) == 0, "%s: coordinates and features must be 16-byte aligned", who);
  FTX_REQUIRE(init_res > 0.f && after_res > 0.f, "%s: resolutions must be positive", who);
  FTX_REQUIRE(aligned256(arena_a) && aligned256(arena_b), "%s: the arenas must be 256-byte aligned device buffers", who);
  if (arena_a_bytes < (size_t)L.a_total || arena_b_bytes < (size_t)L.b_total) {
    set_error("%s: arena A %zu / B %zu < required %zu / %zu (ftx_spvcnn_index_*_arena_bytes)", who, arena_a_bytes, arena_b_bytes, (size_t)L.a_total,
              (size_t)L.b_total);
    return FTX_EWORKSPACE;
  }
  const int64_t ne = 8 * n * kNPV;
  const unsigned bits = dseg_bits(L);
  size_t sort_bytes = 0;
  if (with_backward_segments) {
    int32_t *kp = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, kp, kp, kp, kp, (size_t)ne, 0u, bits) != hipSuccess || sort_bytes > (size_t)L.b_stmp_bytes) {
      set_error("%s: the segment sort needs %zu workspace bytes, the arena reserves %zu", who, sort_bytes, (size_t)L.b_stmp_bytes);
      return FTX_EWORKSPACE;
    }
  }
  // everything above answered on the host; from here on launches only
  hipStream_t st = (hipStream_t)stream;
  char *A = (char *)arena_a, *B = (char *)arena_b;
  const float4 *zc = init_res != after_res ? (const float4 *)(A + L.a_coords) : (const float4 *)coords;

  LevelsDesc LD;
  LD.pts = (const int4 *)(A + L.a_points);
  LD.first = (const int32_t *)(A + L.a_first);
  LD.uniq = (const int64_t *)(A + L.a_uniq);
  LD.n_points = (int32_t)n;
  int64_t cap_off = 0;
  for (int l = 0; l < kNL; ++l) {
    LD.coords[l] = (int4 *)(B + L.b_coords[l]);
    LD.tk[l] = (int64_t *)(B + L.b_tkeys[l]);
    LD.tv[l] = (int32_t *)(B + L.b_tvals[l]);
    LD.cap[l] = L.cap[l];
    LD.off[l] = L.off[l];
    LD.cap_off[l] = cap_off;
    cap_off += L.cap[l];
    LD.stride[l] = kStride[l];
  }
  LD.off[kNL] = L.off[kNL];
  LD.cap_off[kNL] = cap_off;
  nx_table_init_kernel<<<grid_for(cap_off, 256), 256, 0, st>>>(LD);
  nx_levels_kernel<<<grid_for(L.off[kNL], 256), 256, 0, st>>>(LD);

  PvDesc PD;
  memset(&PD, 0, sizeof(PD));
  PD.zc = zc;
  PD.n = n;
  int64_t seg_start = 0, kbase = 0;
  for (int j = 0; j < kNPV; ++j) {
    const int l = kPvLevel[j];
    PD.tk[j] = LD.tk[l];
    PD.tv[j] = LD.tv[l];
    PD.cap[j] = L.cap[l];
    PD.m[j] = L.nl[l];
    PD.stride[j] = kStride[l];
    PD.level[j] = l;
    PD.vidx[j] = (int32_t *)(B + L.vidx[j]);
    PD.vcnt[j] = (int32_t *)(B + L.vcnt[j]);
    PD.vseg[j] = (int32_t *)(B + L.vseg[j]);
    PD.didx[j] = (int32_t *)(B + L.didx[j]);
    PD.dw[j] = (float *)(B + L.dw[j]);
    PD.skeys[j] = (const int64_t *)(A + L.a_skeys) + (int64_t)l * n;
    PD.uniq[j] = LD.uniq + L.off[l];
    PD.seg_start[j] = seg_start;
    seg_start += L.nl[l] + 1;
    PD.kbase[j] = kbase;
    kbase += L.nl[l] + 1;
    PD.dseg[j] = with_backward_segments ? (int32_t *)(B + L.dseg[j]) : nullptr;
  }
  PD.seg_start[kNPV] = seg_start;
  PD.keys_in = (int32_t *)(B + L.b_skin);
  PD.vals_in = (int32_t *)(B + L.b_svin);
  PD.keys_out = (const int32_t *)(B + L.b_skout);
  if (hipMemsetAsync(B + L.b_vcnt, 0, (size_t)L.b_vcnt_bytes, st) != hipSuccess) return check_launch(who);
  nx_point_query_kernel<<<grid_for(n * kNPV, 256), 256, 0, st>>>(PD);
  nx_level_segments_kernel<<<grid_for(seg_start, 256), 256, 0, st>>>(PD);
  rc = ftx_voxelize_fwd_sorted(feats, (const int32_t *)(A + L.a_order), PD.vseg[0], n, c_in, L.nl[0], (float *)(B + L.b_x0), stream);
  if (rc != FTX_OK) return rc;

  NbrDesc ND;
  memset(&ND, 0, sizeof(ND));
  int32_t *nbr = (int32_t *)(B + L.b_nbr), *pos = (int32_t *)(B + L.b_pos);
  for (int m = 0; m < kNM; ++m) {
    NbrInst &I = ND.inst[m];
    const int lin = m < kNL ? m : m - kNL, lout = m < kNL ? m : m - kNL + 1;
    I.src = LD.coords[lout];
    I.tk = LD.tk[lin];
    I.tv = LD.tv[lin];
    I.cap = L.cap[lin];
    I.out = nbr + L.map_start[m];
    I.rows = L.map_nout[m];
    I.k = L.map_k[m];
    I.stride = kStride[lin];
    I.start = L.map_start[m];
    I.valid = (int64_t)I.k * I.rows;
    ND.starts[m] = I.start;
  }
  int64_t e = L.map_start[kNM];
  for (int j = 0; j < kNPV; ++j) {
    NbrInst &I = ND.inst[kNM + j];
    I.src = zc;
    I.tk = PD.tk[j];
    I.tv = PD.tv[j];
    I.cap = PD.cap[j];
    I.out = PD.didx[j];
    I.rows = n;
    I.k = 8;
    I.stride = PD.stride[j];
    I.corners = 1;
    I.start = e;
    I.valid = 8 * n;
    ND.starts[kNM + j] = e;
    e += 8 * n;
  }
  ND.starts[kNM + kNPV] = e;
  nx_nbr_kernel<<<grid_for(e, 256), 256, 0, st>>>(ND);
  nx_trilinear_kernel<<<grid_for(n * kNPV, 256), 256, 0, st>>>(PD);

  MapsDesc MD;
  memset(&MD, 0, sizeof(MD));
  MD.nbr = nbr;
  MD.pos = pos;
  MD.mapbase = (int32_t *)(B + L.b_mapbase);
  MD.paircounts = (int32_t *)(B + L.b_paircounts);
  for (int m = 0; m < kNM; ++m) {
    MD.koff[m] = (int32_t *)(B + L.b_koff[m]);
    MD.start[m] = L.map_start[m];
    MD.n_out[m] = L.map_nout[m];
    MD.n_in[m] = L.map_nin[m];
    MD.k[m] = L.map_k[m];
    if (m >= kNL) {
      MD.pos_t[m] = (int32_t *)(B + L.pos_t2[m - kNL]);
      MD.pair_in[m] = (int32_t *)(B + L.pair_in2[m - kNL]);
      MD.pair_out[m] = (int32_t *)(B + L.pair_out2[m - kNL]);
      MD.cap[m] = L.map_nin[m];       // a strided 2^3 map joins every fine voxel to exactly one (parent, offset)
    }
  }
  MD.start[kNM] = L.map_start[kNM];
  const int64_t total = L.map_start[kNM];
  int32_t *bsum = (int32_t *)(B + L.b_bsum);
  nx_scan_totals_kernel<<<(unsigned)L.n_blocks, 256, 0, st>>>(nbr, total, bsum);
  nx_scan_blocks_kernel<<<1, 256, 0, st>>>(bsum, L.n_blocks);
  nx_scan_write_kernel<<<(unsigned)L.n_blocks, 256, 0, st>>>(nbr, total, bsum, pos);
  nx_koff_kernel<<<1, 256, 0, st>>>(MD);
  if (hipMemcpyAsync(pair_counts_pinned, MD.paircounts, sizeof(int32_t) * kNL, hipMemcpyDeviceToHost, st) != hipSuccess) return check_launch(who);
  if (hipMemsetAsync(B + L.b_pos_t2, 0xFF, (size_t)L.b_pos_t2_bytes, st) != hipSuccess) return check_launch(who);
  nx_pairs_kernel<<<grid_for(L.map_start[kNM] - L.map_start[kNL], 256), 256, 0, st>>>(MD, kNL, kNM - kNL);

  if (with_backward_segments) {
    nx_dseg_prepare_kernel<<<grid_for(ne, 256), 256, 0, st>>>(PD);
    size_t tb = (size_t)L.b_stmp_bytes;
    if (rocprim::radix_sort_pairs(B + L.b_stmp, tb, (const int32_t *)PD.keys_in, (int32_t *)(B + L.b_skout), (const int32_t *)PD.vals_in,
                                  (int32_t *)(B + L.dorder[0]), (size_t)ne, 0u, bits, st) != hipSuccess) {
      set_error("%s: segment sort failed", who);
      return FTX_ELAUNCH;
    }
    nx_dseg_offsets_kernel<<<grid_for(seg_start, 256), 256, 0, st>>>(PD);
  }
  return check_launch(who);
}

// ---------------------------------------------------------------- phase C
extern "C" int ftx_spvcnn_index_pairs(int64_t n, int32_t c_in, const int32_t *level_off_host, int32_t with_backward_segments,
                                      const int32_t *pair_counts_host, void *arena_a, void *arena_b, size_t arena_b_bytes, void *arena_c,
                                      size_t arena_c_bytes, int64_t *rows_host, void *maps_host, void *pvs_host, const float **x0, void *stream) {
  const char *who = "ftx_spvcnn_index_pairs";
  FTX_REQUIRE(level_off_host && pair_counts_host, "%s: null level offsets / pair counts", who);
  Lay L;
  int rc = make_layout(who, n, c_in, level_off_host, pair_counts_host, with_backward_segments, L);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(rows_host && maps_host && pvs_host, "%s: null table", who);
  FTX_REQUIRE(aligned256(arena_a) && aligned256(arena_b) && aligned256(arena_c), "%s: the arenas must be 256-byte aligned device buffers", who);
  if (arena_b_bytes < (size_t)L.b_total || arena_c_bytes < (size_t)L.c_total) {
    set_error("%s: arena B %zu / C %zu < required %zu / %zu (ftx_spvcnn_index_*_arena_bytes)", who, arena_b_bytes, arena_c_bytes, (size_t)L.b_total,
              (size_t)L.c_total);
    return FTX_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char *A = (char *)arena_a, *B = (char *)arena_b, *C = (char *)arena_c;
  MapsDesc MD;
  memset(&MD, 0, sizeof(MD));
  MD.nbr = (const int32_t *)(B + L.b_nbr);
  MD.pos = (int32_t *)(B + L.b_pos);
  MD.mapbase = (int32_t *)(B + L.b_mapbase);
  MD.paircounts = (int32_t *)(B + L.b_paircounts);
  SpvcnnMap *maps = (SpvcnnMap *)maps_host;
  for (int m = 0; m < kNM; ++m) {
    MD.koff[m] = (int32_t *)(B + L.b_koff[m]);
    MD.start[m] = L.map_start[m];
    MD.n_out[m] = L.map_nout[m];
    MD.n_in[m] = L.map_nin[m];
    MD.k[m] = L.map_k[m];
    const bool sub = m < kNL;
    MD.pos_t[m] = (int32_t *)(sub ? C + L.pos_t3[m] : B + L.pos_t2[m - kNL]);
    MD.pair_in[m] = (int32_t *)(sub ? C + L.pair_in3[m] : B + L.pair_in2[m - kNL]);
    MD.pair_out[m] = (int32_t *)(sub ? C + L.pair_out3[m] : B + L.pair_out2[m - kNL]);
    MD.cap[m] = sub ? L.pairs[m] : L.map_nin[m];
    SpvcnnMap &M = maps[m];
    M.nbr = MD.nbr + L.map_start[m];
    M.pos = MD.pos + L.map_start[m];
    M.pos_t = MD.pos_t[m];
    M.pair_in = MD.pair_in[m];
    M.pair_out = MD.pair_out[m];
    M.koff = MD.koff[m];
    M.n_pairs = MD.cap[m];
    M.n_in = L.map_nin[m];
    M.n_out = L.map_nout[m];
    M.kvol = L.map_k[m];
    M.fine_bijective = sub ? 0 : 1;
  }
  MD.start[kNM] = L.map_start[kNM];
  for (int l = 0; l < kNL; ++l) rows_host[l] = L.nl[l];
  rows_host[kNL] = n;
  SpvcnnPV *pvs = (SpvcnnPV *)pvs_host;
  for (int j = 0; j < kNPV; ++j) {
    const int l = kPvLevel[j];
    SpvcnnPV &V = pvs[j];
    V.vox_idx = (const int32_t *)(B + L.vidx[j]);
    V.vox_counts = (const int32_t *)(B + L.vcnt[j]);
    V.vox_order = (const int32_t *)(A + L.a_order) + (int64_t)l * n;
    V.vox_seg_off = (const int32_t *)(B + L.vseg[j]);
    V.devox_idx = (const int32_t *)(B + L.didx[j]);
    V.devox_weights = (const float *)(B + L.dw[j]);
    V.n_vox = L.nl[l];
    V.level = l;
    V.reserved = 0;
  }
  if (x0) *x0 = (const float *)(B + L.b_x0);
  if (hipMemsetAsync(C + L.c_pos_t, 0xFF, (size_t)L.c_pos_t_bytes, st) != hipSuccess) return check_launch(who);
  nx_pairs_kernel<<<grid_for(L.map_start[kNL], 256), 256, 0, st>>>(MD, 0, kNL);
  return check_launch(who);
}
