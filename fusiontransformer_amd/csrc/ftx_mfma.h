// The MFMA vocabulary shared by the kernels of libftx: the accumulator and bf16 fragment vector types, v_mfma_f32_32x32x16_bf16, and
// the fp32 -> bf16 rounding of a float4.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ inline f32x16 mfma_bf16(const bf16x8 &a, const bf16x8 &b, const f32x16 &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// round-to-nearest-even, a plain cast (v_cvt_pk_bf16_f32; NaN stays NaN)
__device__ inline bf16x4 round4(float4 v) { return (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w}; }
