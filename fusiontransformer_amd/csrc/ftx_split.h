// The three-piece operand split of the fp32-accurate families on the bf16 MFMA (ftx_dense_split.hip: the ViT Linears;
// ftx_spconv_split.hip: the sparse convolution), defined once.  include/ftx.h states the contract for callers.
#pragma once
#include "ftx_mfma.h"

namespace ftx {

// the ONE definition of the split: h + m + l == x for finite x in range; h = inf / NaN keeps m = l = 0
__device__ inline void split1(float x, __bf16 &h, __bf16 &m, __bf16 &l) {
  h = (__bf16)x;
  const float hf = (float)h;
  const bool finite = (__float_as_uint(hf) & 0x7f800000u) != 0x7f800000u;
  const float r = finite ? x - hf : 0.f;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

}  // namespace ftx
