// Streaming Gram: S += Y^T Y for rows of `width` floats (129 .. 256) in HBM -- the wide case of launch_gram_batched
// (kernels.hip) and the second half of the path route's overflow (paths_overflow.hip).  One persistent 512-thread workgroup per
// CU, ALL EIGHT waves on the matrix pipes (fp32 MFMA bound): the 4 tile groups of gram256.h (9 sub-tiles each) go to the two
// waves that share a SIMD (hardware waves g and g + 4), 5 + 4 sub-tiles.  Blocks of 32 rows arrive by LDS-DMA, issued by the MFMA
// waves themselves, into a 3-slot ring: one raw s_barrier and one counted vmcnt wait per block.
#include "gram256.h"
#include "lgnn_internal.h"

namespace lgnn {
namespace {

template <int W, int LO, int HI> __device__ __forceinline__ constexpr bool part_uses(int b) {
  for (int s = LO; s < HI; ++s)
    if (Tiles256<W>::si[s] == b || Tiles256<W>::sj[s] == b) return true;
  return false;
}
template <int W, int LO, int HI>
__device__ __forceinline__ void part_load(const float* __restrict__ p, float (&x)[8]) {
#pragma unroll
  for (int b = 0; b < 8; ++b) x[b] = part_uses<W, LO, HI>(b) ? p[b * 32] : 0.f;
}
template <int W, int LO, int HI>
__device__ __forceinline__ void part_mfma(const float (&x)[8], f32x16 (&acc)[HI - LO]) {
#pragma unroll
  for (int s = LO; s < HI; ++s)
    acc[s - LO] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[Tiles256<W>::si[s]], x[Tiles256<W>::sj[s]], acc[s - LO], 0, 0, 0);
}

constexpr int kSlots = 3;
constexpr int kBlockRows = 32;

__device__ float g_stream_zeros[256];  // (zero initialised) the source of copies past a row's end / past the last row

struct GramStreamArgs {
  const float* Y;       // [rows][ld], `width` floats used per row
  int64_t rows;
  int64_t ld;
  int width;
  const float* zeros;   // >= 16 bytes of zeros: the source of lanes past the row's end and of rows past the last
  float* scratch;       // [width][width], upper sub-tiles, float atomics
  const int32_t* gate;  // optional: run only if *gate > gate_cap (the overflow route of the path kernels)
  int64_t gate_cap;
};

// the 4 LDS-DMA row copies of block `blk` that this wave issues (rows 4 hw .. 4 hw + 3 of the block) into slot `slot`
__device__ __forceinline__ void issue_block(const GramStreamArgs& a, float* tiles, int64_t blk, int slot, int hw, int lane,
                                            bool lane_ok) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 4 * hw + q;
    const int64_t row = blk * kBlockRows + r;
    const float* src = (lane_ok && row < a.rows) ? a.Y + row * a.ld + 4 * lane : a.zeros;
    float* dst = tiles + (slot * kBlockRows + r) * 256;  // wave-uniform LDS base; lane l lands at + 4 l floats
    __builtin_amdgcn_global_load_lds(src, reinterpret_cast<__attribute__((address_space(3))) void*>(
                                              reinterpret_cast<uintptr_t>(dst)), 16, 0, 0);
  }
}

template <int W, int LO, int HI>
__device__ __forceinline__ void stream_wave(const GramStreamArgs& a, float* tiles, int64_t nb, int hw, int lane) {
  constexpr int NT = HI - LO;
  f32x16 acc[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  const bool lane_ok = 4 * lane < a.width;  // width % 4 == 0 (launcher)
  const int64_t stride = gridDim.x;
  // prologue: blocks 0 and 1 of this workgroup are in flight before the loop
  issue_block(a, tiles, blockIdx.x, 0, hw, lane, lane_ok);
  issue_block(a, tiles, blockIdx.x + stride, 1, hw, lane, lane_ok);
  for (int64_t i = 0; i < nb; ++i) {
    // all but this wave's 4 youngest copies (block i + 1) have landed => its rows of block i are in LDS; the barrier then
    // says so for every wave's rows, and that everybody is done reading block i - 1, whose slot block i + 2 reuses
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_block(a, tiles, blockIdx.x + (i + 2) * stride, int((i + 2) % kSlots), hw, lane, lane_ok);
    const float* __restrict__ base = tiles + int(i % kSlots) * kBlockRows * 256 + (lane >> 5) * 256 + (lane & 31);
    float xa[8], xb[8];
    part_load<W, LO, HI>(base, xa);
#pragma unroll 2
    for (int kk = 0; kk < kBlockRows / 2; kk += 2) {
      part_load<W, LO, HI>(base + (kk + 1) * 512, xb);
      __builtin_amdgcn_sched_barrier(0);
      part_mfma<W, LO, HI>(xa, acc);
      __builtin_amdgcn_sched_barrier(0);
      if (kk + 2 < kBlockRows / 2) part_load<W, LO, HI>(base + (kk + 2) * 512, xa);
      __builtin_amdgcn_sched_barrier(0);
      part_mfma<W, LO, HI>(xb, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two look-ahead blocks past the end (zeros) before the LDS dies
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t D = a.width;
#pragma unroll
  for (int s = LO; s < HI; ++s) {
    const int64_t j = Tiles256<W>::sj[s] * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t i = Tiles256<W>::si[s] * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      if (i < D && j < D) atomicAdd(&a.scratch[i * D + j], acc[s - LO][r]);
    }
  }
}

__global__ __launch_bounds__(512, 2) void gram256_stream_kernel(GramStreamArgs a) {
  __shared__ float tiles[kSlots * kBlockRows * 256];  // 96 KiB: ONE LDS object (a second one makes hipcc drain vmcnt)
  if (a.gate != nullptr && int64_t(*a.gate) <= a.gate_cap) return;  // (the overflow route of the path kernels)
  const int lane = threadIdx.x & 63;
  const int hw = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t nblocks = (a.rows + kBlockRows - 1) / kBlockRows;
  const int64_t nb = nblocks > int64_t(blockIdx.x) ? (nblocks - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  // hardware waves g and g + 4 share a SIMD (waves are dealt round-robin to the CU's four SIMDs)
  switch (hw) {
    case 0: stream_wave<0, 0, 5>(a, tiles, nb, hw, lane); break;
    case 4: stream_wave<0, 5, 9>(a, tiles, nb, hw, lane); break;
    case 1: stream_wave<1, 0, 5>(a, tiles, nb, hw, lane); break;
    case 5: stream_wave<1, 5, 9>(a, tiles, nb, hw, lane); break;
    case 2: stream_wave<2, 0, 5>(a, tiles, nb, hw, lane); break;
    case 6: stream_wave<2, 5, 9>(a, tiles, nb, hw, lane); break;
    case 3: stream_wave<3, 0, 5>(a, tiles, nb, hw, lane); break;
    default: stream_wave<3, 5, 9>(a, tiles, nb, hw, lane); break;
  }
}

}  // namespace

int launch_gram256_stream(const float* Y, int64_t ld, int64_t rows, int64_t width, float* scratch, hipStream_t s,
                          const int32_t* gate, int64_t gate_cap) {
  LGNN_REQUIRE(width > 128 && width <= 256 && width % 4 == 0 && ld % 4 == 0 && ld >= width, "internal: streaming Gram width");
  if (rows <= 0) return 0;
  static const float* zeros = nullptr;  // address of the device-side zero block (per process; one device per process)
  if (zeros == nullptr) {
    void* p = nullptr;
    LGNN_HIP_CHECK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_stream_zeros)));
    zeros = static_cast<const float*>(p);
  }
  GramStreamArgs g{Y, rows, ld, int(width), zeros, scratch, gate, gate_cap};
  const int64_t nblocks = cdiv(rows, kBlockRows);
  hipLaunchKernelGGL(gram256_stream_kernel, dim3(unsigned(std::min<int64_t>(nblocks, 256))), dim3(512), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn
