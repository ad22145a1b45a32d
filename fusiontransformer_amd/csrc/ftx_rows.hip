// General kernels over the rows of an (n, c) float32 matrix, where the Python path uses torch: channel concatenation and its backward,
// the row-wise add, and the ViT residual stream as one tensor.  The native executors (ftx_exec.hip, ftx_exec_train.hip, ftx_exec_vit.hip)
// issue them through these entries.  Channels are multiples of 4; every access is 16 bytes.
#include "ftx_common.h"

using namespace ftx;

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

// out = r + (p + pb), pb (c) broadcast over the rows: two fp32 adds per element in that order; p == NULL: out = r
// (the ViT residual stream as one tensor, transformers._materialize)
__global__ __launch_bounds__(256) void rows_add_bias_kernel(const float *__restrict__ r, const float *__restrict__ p, const float *__restrict__ pb,
                                                            int64_t total4, int c4, float *__restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total4; e += (int64_t)gridDim.x * blockDim.x) {
    float4 x = *(const float4 *)&r[e * 4];
    if (p) {
      const float4 y = *(const float4 *)&p[e * 4];
      const float4 b = *(const float4 *)&pb[(e % c4) * 4];
      x = make_float4(x.x + (y.x + b.x), x.y + (y.y + b.y), x.z + (y.z + b.z), x.w + (y.w + b.w));
    }
    *(float4 *)&out[e * 4] = x;
  }
}

extern "C" int ftx_rows_add_bias(const float *r, const float *p, const float *pb, int64_t n, int32_t c, float *out, void *stream) {
  FTX_REQUIRE(n >= 0, "ftx_rows_add_bias: n < 0");
  FTX_REQUIRE(c >= 4 && c % 4 == 0, "ftx_rows_add_bias: channels must be a multiple of 4 (c=%d)", c);
  FTX_REQUIRE((p == nullptr) == (pb == nullptr), "ftx_rows_add_bias: p and pb are given together or not at all");
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(r && out, "ftx_rows_add_bias: null pointer");
  FTX_REQUIRE((((uintptr_t)r | (uintptr_t)p | (uintptr_t)pb | (uintptr_t)out) & 15) == 0, "ftx_rows_add_bias: pointers must be 16-byte aligned");
  rows_add_bias_kernel<<<grid_for(n * (c / 4), 256), 256, 0, (hipStream_t)stream>>>(r, p, pb, n * (c / 4), c / 4, out);
  return check_launch("ftx_rows_add_bias");
}
