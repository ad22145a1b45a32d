// Shared helpers for libftx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/ftx.h"

namespace ftx {

void set_error(const char *fmt, ...);

inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return FTX_ELAUNCH;
  }
  return FTX_OK;
}

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Arena pieces start on 256-byte boundaries.
inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Consecutive pieces of an arena or workspace: take(bytes) is the offset of the next piece, `end` the size so far.
struct Offsets256 {
  int64_t end = 0;
  int64_t take(int64_t bytes) {
    const int64_t at = end;
    end += align256(bytes);
    return at;
  }
};

// Grid for a grid-stride elementwise kernel: enough blocks to fill 256 CUs x 8, no more.
inline unsigned grid_for(int64_t work, int block) {
  int64_t g = ceil_div(work, block);
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (unsigned)g;
}

#define FTX_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      ftx::set_error(__VA_ARGS__);             \
      return FTX_EINVAL;                       \
    }                                          \
  } while (0)

// The refusal of a workspace that is too small: `if (workspace_bytes < need) return workspace_short(who, workspace_bytes, need);`
inline int workspace_short(const char *who, size_t have, size_t need) {
  set_error("%s: workspace %zu < required %zu", who, have, need);
  return FTX_EWORKSPACE;
}

// nn.Upsample(size) nearest source index in float32, exactly as ATen computes it:
// src = min((int)floorf(dst * ((float)n_in / (float)n_out)), n_in - 1).
__device__ inline int nearest_src(int dst, int n_in, int n_out) {
  float scale = (float)n_in / (float)n_out;
  int s = (int)floorf((float)dst * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

// FNV-1a over the four int32 words of a coordinate row, folded to 60 bits
// (torchsparse v1.1.0 hash kernel; call sites models/utils.py:19,74-78).
__host__ __device__ inline int64_t fnv_hash4(int32_t x, int32_t y, int32_t z, int32_t b) {
  uint64_t h = 14695981039346656037ULL;
  h ^= (uint32_t)x; h *= 1099511628211ULL;
  h ^= (uint32_t)y; h *= 1099511628211ULL;
  h ^= (uint32_t)z; h *= 1099511628211ULL;
  h ^= (uint32_t)b; h *= 1099511628211ULL;
  h = (h >> 60) ^ (h & 0x0FFFFFFFFFFFFFFFULL);
  return (int64_t)h;
}

// Slot hash for the open-addressing table (murmur3 finaliser).
__device__ inline uint64_t slot_mix(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

constexpr int64_t kEmptyKey = -1;  // hashes are 60-bit non-negative, so -1 never collides

}  // namespace ftx
