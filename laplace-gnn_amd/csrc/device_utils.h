// Small device helpers shared by the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/laplace_gnn_hip.h"

namespace lgnn {

__device__ __forceinline__ float act_apply(float x, int act) {
  return act == LGNN_ACT_RELU ? fmaxf(x, 0.f) : tanhf(x);
}
// derivative of the activation expressed through its OUTPUT h (relu: h > 0 <=> pre > 0)
__device__ __forceinline__ float act_deriv_from_out(float h, int act) {
  return act == LGNN_ACT_RELU ? (h > 0.f ? 1.f : 0.f) : (1.f - h * h);
}

// sum over the wave's 64 lanes, in every lane (xor butterfly: the same summation order wherever it is used)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace lgnn
