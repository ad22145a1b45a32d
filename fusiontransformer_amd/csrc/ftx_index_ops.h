// The per-element arithmetic of the sparse-voxel index build, shared by the per-level entry points (ftx_index.hip, the pair lists of
// ftx_spconv.hip, the sorted segments of ftx_pointvoxel.hip) and by the native builder that does the same work in three calls
// (ftx_native_index.hip).  One expression, written once: the native builder's arrays equal the per-level build bit for bit because both
// kernel families call these functions, and what pins one family to the oracle pins the other.  The float expressions (floor_point,
// trilinear_row) are order-sensitive: do not reorder, re-associate or pre-divide them.  No function here knows which family calls it;
// where the callers differ, the difference is a parameter or stays in the caller.
//
//   function        per-level kernel                                                  native kernel
//   floor_div       (through level_coord)                                             (through level_coord)
//   floor_point     floor_coords_kernel                                               nx_rescale_floor_, nx_point_query_, nx_nbr_kernel (corners)
//   level_coord     downsample_, level_coords_, levels_hash_kernel                    nx_levels_kernel
//   level_key       levels_hash_, levels_offsets_, level_segments_, levels_strip_     nx_level_segments_kernel
//   trilinear_row   trilinear_kernel                                                  nx_trilinear_kernel
//   table_insert    table_insert_kernel                                               nx_levels_kernel
//   table_lookup    table_query_, kernel_map_kernel                                   nx_point_query_, nx_nbr_kernel
//   lower_bound     sorted_rank_, levels_offsets_, level_segments_kernel              nx_level_segments_, nx_dseg_offsets_kernel
//   kernel_offset   (functional.kernel_offsets hands the table in)                    nx_nbr_kernel
//   koff_entry      koff_kernel                                                       nx_koff_kernel
//   pair_entry      pairs_scatter_kernel                                              nx_pairs_kernel
//   segment_key     seg_prepare_kernel                                                nx_dseg_prepare_kernel
#pragma once
#include "ftx_common.h"

namespace ftx {

// ---------------------------------------------------------------- coordinates
__host__ __device__ __forceinline__ int floor_div(int a, int b) {
  int q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// voxel of a float point at `stride`: floor(p / s) * s per axis, the batch column cast
__device__ __forceinline__ int4 floor_point(float4 p, int stride) {
  const float s = (float)stride;
  int4 o;
  o.x = (int)floorf(p.x / s) * stride;
  o.y = (int)floorf(p.y / s) * stride;
  o.z = (int)floorf(p.z / s) * stride;
  o.w = (int)p.w;
  return o;
}

// voxel of an integer point at `stride`: floor_div(p, s) * s per axis, batch column kept
__host__ __device__ __forceinline__ int4 level_coord(int4 v, int stride) {
  v.x = floor_div(v.x, stride) * stride;
  v.y = floor_div(v.y, stride) * stride;
  v.z = floor_div(v.z, stride) * stride;
  return v;
}

// (level tag | hash): hashes are 60-bit, the tag lives in bits 60..62, so one sort orders every level's voxels level by level
constexpr int64_t kLevelHashMask = 0x0FFFFFFFFFFFFFFFLL;
__host__ __device__ __forceinline__ int64_t level_key(int64_t level, int64_t hash) { return (level << 60) | hash; }

// The 8 trilinear weights of point p for the corner rows idx8 (corner order (bx,by,bz), z fastest = KernelRegion(2, s, 1) offsets).
// float32 throughout, in upstream's operation order (torchsparse calc_ti_weights works in the dtype of `pc`, float32):
// three-factor product, division by scale^3, zero for absent corners, sum of the 8, division by (sum + 1e-8)
__device__ __forceinline__ void trilinear_row(float4 p, const int32_t *idx8, int scale, float *w8) {
  const float s = (float)scale;
  float fx, fy, fz;
  if (scale != 1) {
    fx = floorf(p.x / s) * s; fy = floorf(p.y / s) * s; fz = floorf(p.z / s) * s;
  } else {
    fx = floorf(p.x); fy = floorf(p.y); fz = floorf(p.z);
  }
  float cx = fx + s, cy = fy + s, cz = fz + s;
  const float lo[3] = {p.x - fx, p.y - fy, p.z - fz};
  const float hi[3] = {cx - p.x, cy - p.y, cz - p.z};
  float ws[8];
  float sum = 0.f;
  const float inv = s * s * s;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int bx = (c >> 2) & 1, by = (c >> 1) & 1, bz = c & 1;
    float v = ((bx ? lo[0] : hi[0]) * (by ? lo[1] : hi[1])) * (bz ? lo[2] : hi[2]);
    if (scale != 1) v = v / inv;
    if (idx8[c] < 0) v = 0.f;
    ws[c] = v;
    sum += v;
  }
  const float den = sum + 1e-8f;
#pragma unroll
  for (int c = 0; c < 8; ++c) w8[c] = ws[c] / den;
}

// ---------------------------------------------------------------- hash table (open addressing, capacity a power of two)
// the smallest row wins among duplicate keys
__device__ __forceinline__ void table_insert(int64_t key, int32_t row, int64_t *tk, int32_t *tv, int64_t cap) {
  const uint64_t mask = (uint64_t)cap - 1;
  uint64_t slot = slot_mix((uint64_t)key) & mask;
  for (int64_t probe = 0; probe < cap; ++probe) {
    unsigned long long prev = atomicCAS((unsigned long long *)&tk[slot], (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == (unsigned long long)kEmptyKey || prev == (unsigned long long)key) {
      atomicMin(&tv[slot], row);
      break;
    }
    slot = (slot + 1) & mask;
  }
}

__device__ __forceinline__ int32_t table_lookup(int64_t key, const int64_t *__restrict__ tk, const int32_t *__restrict__ tv, int64_t cap) {
  const uint64_t mask = (uint64_t)cap - 1;
  uint64_t slot = slot_mix((uint64_t)key) & mask;
  for (int64_t probe = 0; probe < cap; ++probe) {
    int64_t cur = tk[slot];
    if (cur == key) return tv[slot];
    if (cur == kEmptyKey) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

// first position of sorted[0 .. n) (ascending) whose key is not below `want`
template <typename K>
__host__ __device__ __forceinline__ int64_t lower_bound(const K *sorted, int64_t n, K want) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- kernel maps and pair lists
// Offset kk of the 3^3 (ks = 27) or 2^3 (ks = 8) kernel at `stride`: the library's one statement of the enumeration order, which must
// agree with functional.kernel_offsets (torchsparse KernelRegion: odd kernels enumerate x fastest, even kernels z fastest).
__host__ __device__ __forceinline__ void kernel_offset(int ks, int kk, int stride, int &dx, int &dy, int &dz) {
  if (ks == 27) {           // offsets -stride / 0 / +stride
    dx = (kk % 3 - 1) * stride; dy = ((kk / 3) % 3 - 1) * stride; dz = (kk / 9 - 1) * stride;
  } else {                  // offsets 0 / +stride
    dx = ((kk >> 2) & 1) * stride; dy = ((kk >> 1) & 1) * stride; dz = (kk & 1) * stride;
  }
}

// koff[kk] of one (k, n_out) neighbour table `nbr` from `scan`, the exclusive scan of its validity flags shifted by `base`: the first
// pair of offset kk, and for kk == k the number of pairs
__device__ __forceinline__ int32_t koff_entry(const int32_t *nbr, const int32_t *scan, int64_t n_out, int k, int kk, int32_t base) {
  if (kk < k) return scan[(int64_t)kk * n_out] - base;
  const int64_t last = (int64_t)k * n_out - 1;
  return scan[last] + (nbr[last] >= 0 ? 1 : 0) - base;
}

// entry e = kk * n_out + o of a (k, n_out) neighbour table with input row i and scan position p: records the pair and returns its
// position in the list, or -1 where there is no pair (absent neighbour, or a row / position outside the arrays).  The division is
// for real pairs only: most entries of a table are absent neighbours.
__device__ __forceinline__ int32_t pair_entry(int32_t i, int32_t p, int64_t e, int64_t n_out, int64_t n_in, int64_t cap, int32_t *pair_in,
                                              int32_t *pair_out, int32_t *pos_t) {
  if (i >= 0 && i < n_in && p >= 0 && p < cap) {
    int kk = (int)(e / n_out);
    int64_t o = e - (int64_t)kk * n_out;
    pair_in[p] = i;
    pair_out[p] = (int32_t)o;
    pos_t[(int64_t)kk * n_in + i] = p;
    return p;
  }
  return -1;
}

// sort key of an entry bound for row k of m: invalid entries sort to the end
__host__ __device__ __forceinline__ int32_t segment_key(int32_t k, int64_t m) { return (k >= 0 && k < m) ? k : (int32_t)m; }

}  // namespace ftx
