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

}  // namespace ftx
