// The path route of a batch whose path list does not fit its buffer (or LGNN_PATH_LIST_CAP): ybuild_kernel enumerates every
// node's paths on the fly and streams Y to HBM as class planes, the streaming Gram (gram_stream.hip) contracts them.  Both
// launches are gated on the device by the list's length: they return at once when it did fit.
#include "gram256.h"
#include "paths.h"

namespace lgnn {
namespace {

constexpr int kPathWindow = 128; // paths staged in LDS per accumulation window

// Paths staged per window.  26.6 % of the arxiv-shaped nodes have more than 16 paths, 12 % more than 20 (mean 13.7): every
// further window of a node is restaged in place, two barriers and an exposed copy.  20 x (2 x 1 KiB table rows + 768 B
// coefficients + 32 B mask) = 55.6 KiB per window; two of them and a 40-row Y tile fill the 160 KiB of a CU.
constexpr int kWin = 20;
constexpr int kCoefLds = 3 * kCoefStride;  // floats of a coefficient row that are staged (the table's rows are 1 KiB apart)

struct YWin {
  float bg[kWin][2][256];       // rows b_m, g_m as they sit in the table (the mask is applied when they are read)
  float coef[kWin][kCoefLds];   // (alpha | -beta | -gamma) of the path's sample (the path weight is applied when read)
  uint32_t mask[kWin][8];       // ReLU bits of the path's middle node v
};
struct YMeta {                  // the window's triples
  int32_t m[kWin], v[kWin];
  float w[kWin];
};

__device__ __forceinline__ void lds_dma16(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, reinterpret_cast<__attribute__((address_space(3))) void*>(
                                            reinterpret_cast<uintptr_t>(lds_dst)), 16, 0, 0);
}

// Start the LDS-DMA copies of a window of kw <= kWin paths (triples in `mt`): three 1 KiB pieces per path (row b_m, row g_m,
// the coefficient row), one wave instruction each, no data registers.  Asynchronous: the consumer waits on vmcnt + a barrier.
__device__ __forceinline__ void stage_dma(const YArgs& a, YWin& win, const YMeta& mt, int kw, int wave, int nwaves, int lane) {
  const int kw2 = (kw + 1) & ~1;  // the last MFMA step reads an even number of paths: the odd one out is staged as zeros
  const bool lane_ok = 4 * lane < a.H;
  const int npieces = kw2 * 3;
  for (int q = wave; q < npieces; q += nwaves) {   // q, j, kind are wave uniform
    const int j = q / 3, kind = q - 3 * j;
    const float* src = a.zeros;
    float* dst = kind < 2 ? &win.bg[j][kind][0] : &win.coef[j][0];
    if (j < kw) {
      const int64_t mj = __builtin_amdgcn_readfirstlane(mt.m[j]);
      if (kind == 2) src = a.coef + mj * kCoefRow + 4 * lane;
      else if (lane_ok && !a.no_bg) src = a.bg + ((kind ? a.M : 0) + mj) * a.H + 4 * lane;
    }
    // (a coefficient row is 768 bytes in LDS: 48 lanes copy, the others would land in the next path's row)
    if (kind < 2 || lane < kCoefLds / 4) lds_dma16(src, dst);
  }
}
// the mask word (j = tid >> 3, word = tid & 7) of the window's paths, for threads tid < 8 * kw2
__device__ __forceinline__ uint32_t load_mask_word(const YArgs& a, const YMeta& mt, int kw, int tid) {
  const int j = tid >> 3, wd = tid & 7;
  return (j < kw && wd < a.mask_words) ? a.mask[int64_t(mt.v[j]) * a.mask_words + wd] : 0u;
}

// The three products of one staged window: wave (rt, cg), lane l: A row i = l & 31 (class), B column = l & 31, k = l >> 5.
// The LDS operands of step ks + 1 are read before the six MFMAs of step ks are issued (their latency hides behind 384 cycles
// of matrix work instead of stalling every step).
struct YOps { float aa, ab, ag, mf[2], bb[2], gg[2]; };
__device__ __forceinline__ void y_load_ops(const YWin& win, const YMeta& mt, int kw, int ks, int half, int cls,
                                           const int (&colv)[2], const bool (&col_ok)[2], YOps& o) {
  const int j = min(2 * ks + half, kWin - 1);   // (past the window's end: a valid row, weight 0)
  const float wj = 2 * ks + half < kw ? mt.w[j] : 0.f;
  o.aa = wj * win.coef[j][cls]; o.ab = wj * win.coef[j][kCoefStride + cls]; o.ag = wj * win.coef[j][2 * kCoefStride + cls];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const uint32_t word = win.mask[j][colv[ct] >> 5];
    o.mf[ct] = (col_ok[ct] && 2 * ks + half < kw && ((word >> (colv[ct] & 31)) & 1u)) ? 1.f : 0.f;
    o.bb[ct] = o.mf[ct] * win.bg[j][0][colv[ct]];
    o.gg[ct] = o.mf[ct] * win.bg[j][1][colv[ct]];
  }
}
__device__ __forceinline__ void y_mfma_ops(const YOps& o, bool no_bg, f32x16 (&t1)[2], f32x16 (&y2)[2]) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    t1[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.aa, o.mf[ct], t1[ct], 0, 0, 0);
    if (!no_bg) {
      y2[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.ab, o.bb[ct], y2[ct], 0, 0, 0);
      y2[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.ag, o.gg[ct], y2[ct], 0, 0, 0);
    }
  }
}
__device__ __forceinline__ void mfma_window(const YWin& win, const YMeta& mt, int kw, int cls, const int (&colv)[2],
                                            const bool (&col_ok)[2], int half, bool no_bg, f32x16 (&t1)[2], f32x16 (&y2)[2]) {
  const int nks = (kw + 1) >> 1;
  if (nks == 0) return;
  YOps oa, ob;
  y_load_ops(win, mt, kw, 0, half, cls, colv, col_ok, oa);
  for (int ks = 0; ks < nks; ks += 2) {
    y_load_ops(win, mt, kw, ks + 1, half, cls, colv, col_ok, ob);  // (a step past the end multiplies zeros)
    __builtin_amdgcn_sched_barrier(0);
    y_mfma_ops(oa, no_bg, t1, y2);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 1 < nks) {
      y_load_ops(win, mt, kw, ks + 2, half, cls, colv, col_ok, oa);
      __builtin_amdgcn_sched_barrier(0);
      y_mfma_ops(ob, no_bg, t1, y2);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Role of a wave: (rt, cg) owns the 32-class row tile rt (classes c0 + 32 rt ...) and the columns [64 cg, 64 cg + 64) of
// Y[n]: two 32 x 32 accumulator tiles for the alpha product and two for the beta / gamma products; waves w and w + 4 (the
// two row tiles of one column group) share a SIMD.
struct YRole {
  int lane, li, half, wave, nwaves, cg, rt, cls;
  int colv[2];
  bool col_ok[2];
};
__device__ __forceinline__ YRole y_role(const YArgs& a) {
  YRole r;
  const int tid = threadIdx.x;
  r.lane = tid & 63; r.li = r.lane & 31; r.half = r.lane >> 5;
  r.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  r.nwaves = blockDim.x >> 6;
  const int ncg = (a.H + 63) >> 6;
  r.cg = r.wave % ncg; r.rt = r.wave / ncg;
  // class of this lane's A-operand row (i = lane & 31), clamped into the zero-padded coefficient row; rows past the class
  // range are computed on whatever sits there and never stored
  r.cls = coef_slot(min(a.c0 - a.cb + 32 * r.rt + r.li, kCoefStride - 1));
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    r.colv[ct] = 64 * r.cg + 32 * ct + r.li;
    r.col_ok[ct] = r.colv[ct] < a.H;
    if (!r.col_ok[ct]) r.colv[ct] = 0;
  }
  return r;
}

// The fallback when the batch's path list does not fit its buffer (very large batches on hub-heavy graphs): a grid-stride loop
// over nodes, the paths enumerated here -- block scan over the neighbours' R lists, up to kPathWindow triples at a time in
// LDS, staged kWin at a time.  Same arithmetic, no overlap; its launch returns at once when the list did fit.
__global__ __launch_bounds__(512, 4) void ybuild_kernel(YArgs a) {
  __shared__ struct {
    YWin win;
    YMeta meta;
    int32_t fm[kPathWindow], fv[kPathWindow];
    float fw[kPathWindow];
    int32_t scan[8];
  } sh;
  if (int64_t(a.pptr[a.N]) <= a.cap) return;
  const YRole ro = y_role(a);
  const int tid = threadIdx.x, lane = ro.lane, wave = ro.wave, H = a.H;
  const int nthreads = blockDim.x, nwaves = ro.nwaves;
  const bool no_bg = a.no_bg != 0;
  for (int64_t n = a.n0 + blockIdx.x; n < a.n1; n += gridDim.x) {
    f32x16 t1[2], y2[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) { t1[ct][r] = 0.f; y2[ct][r] = 0.f; }
    const int32_t rs = a.rowptr[n], re = a.rowptr[n + 1];
    for (int32_t base = rs; base < re; base += nthreads) {
      // ---- this thread's neighbour v and the extent of its batch list R[v]
      int32_t v = 0, r0 = 0, cnt = 0;
      float pv = 0.f;
      if (base + tid < re) {
        v = a.col[base + tid];
        pv = a.val[base + tid];
        r0 = a.rptr[v];
        cnt = a.rptr[v + 1] - r0;
      }
      // ---- block-wide exclusive scan of cnt
      int incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      __syncthreads();  // sh.scan / the triples of the previous chunk are still being read
      if (lane == 63) sh.scan[wave] = incl;
      __syncthreads();
      int woff = 0, total = 0;
      for (int w = 0; w < nwaves; ++w) {
        const int sw = sh.scan[w];
        if (w < wave) woff += sw;
        total += sw;
      }
      const int off = woff + incl - cnt;
      for (int wb = 0; wb < total; wb += kPathWindow) {
        __syncthreads();
        const int lo = max(off, wb), hi = min(off + cnt, wb + kPathWindow);
        for (int j = lo; j < hi; ++j) {
          const int k = j - off;
          sh.fm[j - wb] = a.r_m[r0 + k];
          sh.fw[j - wb] = pv * a.r_w[r0 + k];
          sh.fv[j - wb] = v;
        }
        __syncthreads();
        const int kall = min(kPathWindow, total - wb);
        for (int sb = 0; sb < kall; sb += kWin) {
          const int kw = min(kWin, kall - sb);
          if (sb > 0) __syncthreads();
          if (tid < kw) { sh.meta.m[tid] = sh.fm[sb + tid]; sh.meta.v[tid] = sh.fv[sb + tid]; sh.meta.w[tid] = sh.fw[sb + tid]; }
          __syncthreads();
          stage_dma(a, sh.win, sh.meta, kw, wave, nwaves, lane);
          if (tid < 8 * kWin) sh.win.mask[tid >> 3][tid & 7] = load_mask_word(a, sh.meta, kw, tid);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          mfma_window(sh.win, sh.meta, kw, ro.cls, ro.colv, ro.col_ok, ro.half, no_bg, t1, y2);
        }
      }
    }
    // ---- Y[n][c - c0][col] = W_1[c][col] * T1 + Y2
    // (32-bit offsets from two uniform bases; `late` ties the address arithmetic to this point of the program -- hipcc
    //  otherwise computes all 64 addresses at the top of the kernel and spills them around the products)
    int late = 0;
    asm volatile("v_mov_b32 %0, 0" : "=v"(late));
    float* __restrict__ yn = a.Y + n * int64_t(a.R) * H;
    const float* __restrict__ w1p = a.W1 + int64_t(a.c0) * H;
    const int row0 = 32 * ro.rt + 4 * ro.half + late;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int colc = 64 * ro.cg + 32 * ct + ro.li;
      const bool cok = colc < H;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        const int o = row * H + colc;
        if (cok && row < a.R) yn[o] = w1p[o] * t1[ct][r] + y2[ct][r];
      }
    }
    __syncthreads();  // the next node restages the shared buffers
  }
}

}  // namespace

int launch_paths_overflow(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s) {
  const int64_t N = y.N, H = y.H, nb = y.n0, ne = y.n1;
  const int64_t per_class = std::max<int64_t>(N * H * 4, 1);  // planes in HBM, under the workspace cap
  const int64_t cc_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ce - cb, 64), h->ws_limit / per_class));
  LGNN_CALL(h->ws.planes_a.reserve(size_t(cc_max) * N * H * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  y.Y = h->ws.planes_a.as<float>(); y.list = nullptr; y.n_list = nullptr;
  for (int64_t c0 = cb; c0 < ce; c0 += cc_max) {
    const int64_t R = std::min(cc_max, ce - c0);
    y.c0 = int(c0); y.R = int(R);
    const unsigned threads = unsigned(64 * cdiv(H, 64) * cdiv(R, 32));  // (column groups) x (32-class row tiles) waves
    hipLaunchKernelGGL(ybuild_kernel, dim3(unsigned(std::min<int64_t>(ne - nb, 1024))), dim3(threads), 0, s, y);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(launch_gram256_stream(y.Y + nb * R * H, H, (ne - nb) * R, H, scratch, s, y.pptr + N, y.cap));
  }
  return 0;
}

}  // namespace lgnn
