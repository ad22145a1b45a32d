// Counter-based Dropout (include/ftx.h: ftx_dropout / ftx_dropout_mask).  The mask is a pure function of (seed, call, logical element
// index): Philox4x32-10 keyed by the seed, counter (q lo, q hi, call lo, call hi) with q = g >> 2, word g & 3 of the ten-round output
// against a 32-bit threshold.  Nothing is stored: the backward is the same call on the gradient.
//
// Memory-bound streaming: 8 bytes of traffic and ~25 integer VALU operations per element on the fast path (one Philox block per four
// consecutive elements, one 16-byte load and one 16-byte store per lane), grid capped at 2048 blocks of 256 lanes as the other
// streaming kernels of the library (ftx_common.h: grid_for), grid-stride beyond the cap.  Elements in front of the first multiple of
// four of the logical index (head), behind the last (tail), and every element of a buffer whose 16-byte alignment does not fall on such
// a multiple take the scalar path: one Philox block per element, word g & 3 of it -- the same bits.
#include "ftx_common.h"

using namespace ftx;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMulA = 0xD2511F53u, kMulB = 0xCD9E8D57u, kKeyA = 0x9E3779B9u, kKeyB = 0xBB67AE85u;

struct Stream {          // what the host hands every lane: the key, the high counter words, the threshold and the scale
  uint32_t k0, k1, c2, c3, thr;
  float scale;
};

struct U4 {
  uint32_t w[4];
};

__device__ inline U4 philox4x32_10(uint64_t q, const Stream &s) {
  uint32_t c0 = (uint32_t)q, c1 = (uint32_t)(q >> 32), c2 = s.c2, c3 = s.c3, k0 = s.k0, k1 = s.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kMulA, c0), lo0 = kMulA * c0;
    const uint32_t hi1 = __umulhi(kMulB, c2), lo1 = kMulB * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kKeyA;
    k1 += kKeyB;
  }
  return {{c0, c1, c2, c3}};
}

// The n elements of a call that starts at logical index elem0 are `items` work items: `head` scalar elements up to the first multiple
// of four, n4 vectors of four, and the scalar tail; a buffer the vector path cannot take is all tail (head = n4 = 0).
// item w < n4: the vector of elements head + 4 w ..; else scalar element number w - n4 of head ++ tail
__device__ inline int64_t scalar_index(int64_t w, int64_t head, int64_t n4) {
  const int64_t s = w - n4;
  return s < head ? s : s + 4 * n4;
}

// y = x * (keep ? scale : 0): a product, so that NaN and Inf of a dropped element give NaN.  y may be x: every element is read and
// written by one lane, the read first.
__global__ __launch_bounds__(kBlock) void dropout_kernel(const float *x, float *y, int64_t head, int64_t n4, int64_t items, uint64_t elem0, Stream s) {
  for (int64_t w = blockIdx.x * (int64_t)kBlock + threadIdx.x; w < items; w += (int64_t)gridDim.x * kBlock) {
    if (w < n4) {
      const int64_t i = head + 4 * w;
      const U4 u = philox4x32_10((elem0 + (uint64_t)i) >> 2, s);
      const float4 v = *(const float4 *)&x[i];
      *(float4 *)&y[i] = make_float4(v.x * (u.w[0] >= s.thr ? s.scale : 0.0f), v.y * (u.w[1] >= s.thr ? s.scale : 0.0f),
                                     v.z * (u.w[2] >= s.thr ? s.scale : 0.0f), v.w * (u.w[3] >= s.thr ? s.scale : 0.0f));
    } else {
      const int64_t i = scalar_index(w, head, n4);
      const uint64_t g = elem0 + (uint64_t)i;
      const U4 u = philox4x32_10(g >> 2, s);
      const uint32_t j = (uint32_t)g & 3u;
      const uint32_t r = j == 0 ? u.w[0] : j == 1 ? u.w[1] : j == 2 ? u.w[2] : u.w[3];
      y[i] = x[i] * (r >= s.thr ? s.scale : 0.0f);
    }
  }
}

__global__ __launch_bounds__(kBlock) void dropout_mask_kernel(uint8_t *keep, int64_t head, int64_t n4, int64_t items, uint64_t elem0, Stream s) {
  for (int64_t w = blockIdx.x * (int64_t)kBlock + threadIdx.x; w < items; w += (int64_t)gridDim.x * kBlock) {
    if (w < n4) {
      const int64_t i = head + 4 * w;
      const U4 u = philox4x32_10((elem0 + (uint64_t)i) >> 2, s);
      *(uchar4 *)&keep[i] = make_uchar4(u.w[0] >= s.thr, u.w[1] >= s.thr, u.w[2] >= s.thr, u.w[3] >= s.thr);
    } else {
      const int64_t i = scalar_index(w, head, n4);
      const uint64_t g = elem0 + (uint64_t)i;
      const U4 u = philox4x32_10(g >> 2, s);
      const uint32_t j = (uint32_t)g & 3u;
      const uint32_t r = j == 0 ? u.w[0] : j == 1 ? u.w[1] : j == 2 ? u.w[2] : u.w[3];
      keep[i] = r >= s.thr;
    }
  }
}

// threshold and scale on the host, as include/ftx.h states them
inline Stream make_stream(float p, uint64_t seed, uint64_t call) {
  const double scaled = (double)p * 4294967296.0;      // p < 1 as a float: below 2^32
  return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)(uint64_t)scaled, (float)(1.0 / (1.0 - (double)p))};
}

}  // namespace

extern "C" int64_t ftx_dropout_sweep_elements(void) { return (int64_t)2048 * kBlock * 4; }

extern "C" int ftx_dropout(const float *x, int64_t n, float p, uint64_t seed, uint64_t call, uint64_t elem0, float *y, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_dropout: n < 0");
  FTX_REQUIRE(p >= 0.0f && p < 1.0f, "ftx_dropout: p = %g outside [0, 1)", (double)p);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(x && y, "ftx_dropout: null pointer");
  FTX_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0, "ftx_dropout: pointers must be 4-byte aligned");
  FTX_REQUIRE(n <= (int64_t)1 << 60, "ftx_dropout: n too large");
  const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y, bytes = (uintptr_t)n * 4;
  FTX_REQUIRE(xa == ya || xa + bytes <= ya || ya + bytes <= xa, "ftx_dropout: x and y overlap without being the same buffer (in place is y == x)");
  int64_t head = (int64_t)((4 - (elem0 & 3)) & 3);
  if (head > n) head = n;
  int64_t n4 = (((xa + 4 * (uintptr_t)head) | (ya + 4 * (uintptr_t)head)) & 15) == 0 ? (n - head) >> 2 : 0;
  if (n4 == 0) head = 0;
  const int64_t items = n4 + (n - 4 * n4);
  dropout_kernel<<<grid_for(items, kBlock), kBlock, 0, (hipStream_t)stream>>>(x, y, head, n4, items, elem0, make_stream(p, seed, call));
  return check_launch("ftx_dropout");
}

extern "C" int ftx_dropout_mask(int64_t n, float p, uint64_t seed, uint64_t call, uint64_t elem0, uint8_t *keep, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_dropout_mask: n < 0");
  FTX_REQUIRE(p >= 0.0f && p < 1.0f, "ftx_dropout_mask: p = %g outside [0, 1)", (double)p);
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(keep, "ftx_dropout_mask: null pointer");
  int64_t head = (int64_t)((4 - (elem0 & 3)) & 3);
  if (head > n) head = n;
  int64_t n4 = (((uintptr_t)keep + (uintptr_t)head) & 3) == 0 ? (n - head) >> 2 : 0;
  if (n4 == 0) head = 0;
  const int64_t items = n4 + (n - 4 * n4);
  dropout_mask_kernel<<<grid_for(items, kBlock), kBlock, 0, (hipStream_t)stream>>>(keep, head, n4, items, elem0, make_stream(p, seed, call));
  return check_launch("ftx_dropout_mask");
}
