// The lane layout of v_mfma_f32_32x32x2_f32 and the LDS tile step built on it, written down once.
//
// One instruction multiplies a 32 x 2 slice of A by a 2 x 32 slice of B into a wave's 32 x 32 fp32 accumulator.  Lane l
// supplies operand row l & 31 at k = kk + (l >> 5); the result of lane l is column l & 31, rows
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) for the accumulator registers r = 0 .. 15.
//
// The helpers take LDS tile pointers and scalars, never structs: the loops they replace keep their scalar loads.  A form is
// here when two kernels share it; a kernel whose operands come from registers (the Gram accumulators of gram256.h, the path
// route, diag.hip, eigh.hip, train.hip) or that reads a tile in a form of its own (ggn_tn_kernel's transposed product, the
// 128 x 128 block step of gemm_kernel and its two copies) issues the instruction itself.
#pragma once
#include <hip/hip_runtime.h>

namespace lgnn {

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ void acc_zero(f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// Row of accumulator register r in this lane, counted from the row `base` of the wave's 32 x 32 block; the column is
// lane & 31.  The pieces are added to `base` one by one in its own type: what the callers wrote out before.
template <class T>
__device__ __forceinline__ T acc_row(T base, int lane, int r) {
  return base + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// acc += A[arow0 .. arow0 + 32, 0 .. K) B[brow0 .. brow0 + 32, 0 .. K)^T for two K-contiguous LDS tiles of row stride LD
// (one wave's 32 x 32 block of a 64 x 64 workgroup tile: arow0 = 32 (wave >> 1), brow0 = 32 (wave & 1))
template <int K, int LD>
__device__ __forceinline__ void tile_nt_step(const float* __restrict__ As, int arow0, const float* __restrict__ Bs, int brow0,
                                             int lane, f32x16& acc) {
  static_assert(K % 2 == 0, "two k per instruction");
  const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < K; kk += 2) {
    const float a = As[(arow0 + l31) * LD + kk + lh];
    const float b = Bs[(brow0 + l31) * LD + kk + lh];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
}

}  // namespace lgnn
