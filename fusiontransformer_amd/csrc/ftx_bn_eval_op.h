// The per-element arithmetic of the eval-mode BatchNorm (+ residual) (+ ReLU), shared by the stand-alone apply kernel
// (ftx_bn.hip: bn_apply_eval_kernel) and by the sparse-conv reduce that carries it in its epilogue (ftx_spconv.hip:
// spconv_reduce_bn_eval_kernel).  One expression, written once: the compiler contracts it the same way in both kernels, which is what
// makes the fused kernel bit-identical to reduce + apply.  Do not reorder or re-associate it.
#pragma once
#include <hip/hip_runtime.h>

namespace ftx {

__device__ __forceinline__ float bn_eval_elem(float x, float rm, float rv, float eps, float gamma, float beta, float rr, int relu) {
  float is = (float)(1.0 / sqrt((double)rv + (double)eps));
  float t = (x - rm) * is * gamma + beta + rr;
  return (relu && !(t > 0.f)) ? 0.f : t;
}

// bn_eval_elem on the four channels [col, col + 4) of one row: xv holds the row's four values, the residual (optional) is read at res[off].
__device__ __forceinline__ float4 bn_eval_apply4(float4 xv, const float *__restrict__ res, int64_t off, const float *__restrict__ rm,
                                                 const float *__restrict__ rv, float eps, const float *__restrict__ gamma,
                                                 const float *__restrict__ beta, int col, int relu) {
  float o[4] = {xv.x, xv.y, xv.z, xv.w};
  float rr[4] = {0, 0, 0, 0};
  if (res) {
    float4 t = *(const float4 *)&res[off];
    rr[0] = t.x; rr[1] = t.y; rr[2] = t.z; rr[3] = t.w;
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) o[v] = bn_eval_elem(o[v], rm[col + v], rv[col + v], eps, gamma[col + v], beta[col + v], rr[v], relu);
  return make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace ftx
