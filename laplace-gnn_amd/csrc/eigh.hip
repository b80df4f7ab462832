// Batched symmetric eigendecomposition of the Kronecker factors (the step right after the accumulation inside
// KronLaplace.fit: laplace/baselaplace.py:1610 -> laplace/utils/matrix.py:118-145 -> utils.py:193-226).
//
// The reference calls torch.linalg.eigh once per factor; on this stack that is one rocSOLVER syevd per matrix, each a
// chain of ~100 single-workgroup kernels (tridiagonalisation panels, divide and conquer): ~3.3 ms per 256 x 256 factor,
// 13 ms for the four distinct factors of the arxiv-shaped model -- strictly serial and using one CU.  Batched through ONE
// strided-batched syevd the decomposition costs what the largest factor costs (5.0 ms), 4 ms of it the Householder
// tridiagonalisation: 64 panel steps of seven tiny launches each plus a 2 ms single-workgroup tail kernel.
//
// n <= 256 (every factor of the BASELINE models) therefore takes a hand-written path:
//   tridiag256_kernel   one 1024-thread workgroup per matrix, the whole matrix in REGISTERS (thread (r, q) owns 64 entries
//                       of row r), the Householder vector / A v / w through 4 KB of LDS, four barriers per column and
//                       no launch in between: A = Q T Q^T, reflectors to a workspace                       (~0.5 ms)
//   tridiag_dc_kernel   divide and conquer on T (eigenvectors of the tridiagonal matrix), again one 1024-thread workgroup per
//                       matrix and no launch in between (the library's sstedc is a chain of ~75 tiny kernels per factor)
//   backtransform_kernel  y = H_0 H_1 ... H_{n-2} z, one wave per eigenvector, reflectors streamed from L2
// (The caller pads smaller factors to the common size with a decoupled negative diagonal block, see matrix.py: a column
// whose off-diagonal part is exactly zero gets tau = 0 and costs one barrier, and a split with e = 0 is a pure sort.)
// 256 < n <= 512 (n % 4 == 0) keeps rocsolver_sstedc between the hand-written tridiagonalisation and back-transform; larger
// factors (or n % 4 != 0 above 256) take the library's syevd.
#include <cstdio>

#include <rocsolver/rocsolver.h>

#include "gram256.h"  // f32x16
#include "lgnn_internal.h"

namespace lgnn {
namespace {
rocblas_handle g_handle = nullptr;
// The library path (factors above 256 rows) has a handle and a workspace of its own: KronLaplace runs it on a side stream
// while the caller's stream still executes queued batches that use g_handle (rocBLAS handles are not meant to serve two
// streams at once: they carry the solver's device workspace).
rocblas_handle g_eig_handle = nullptr;
struct EighScratch {
  DevBuf e_large;  // off-diagonal workspace of the library path [batch, n]
  DevBuf e;    // off-diagonal workspace [batch, n]
  DevBuf v;    // Householder vectors [batch][n][256]
  DevBuf tau;  // [batch][n]
  DevBuf d;    // diagonal of T in, eigenvalues out [batch][n]
  DevBuf z;    // eigenvectors of T [batch][n][n]
  DevBuf z2;   // tridiag_dc_kernel's second eigenvector buffer [batch][n][n]
  DevBuf info; // [batch]
};
// never deleted, like the handles: a hipFree at static destruction could run after the HIP runtime is gone
EighScratch& scratch() {
  static auto* s = new EighScratch;
  return *s;
}

// 256 < n <= 512 only: the library's divide and conquer calls of the factors are independent chains of ~75 tiny kernels each
// (launch after launch on one CU): each factor's chain goes to a side stream of its own (own rocBLAS handle and
// workspace), forked off and joined back into the caller's stream with events, so the chains run side by side.
// (Capturing the chains into a hipGraph was tried first: the solver performs an operation that is not permitted while a
// stream is capturing, so the fork / join is done with plain streams.)
constexpr int kBranches = 8;
rocblas_handle g_bh[kBranches] = {};
hipStream_t g_side[kBranches] = {};
hipEvent_t g_fork = nullptr, g_join[kBranches] = {};
constexpr int TN = 256;

__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Thread (r = tid / 4, q = tid % 4) holds a[4 g + i] = A[r][16 g + 4 q + i], g < 16, i < 4: the four threads of a row read
// 64 contiguous bytes of an LDS vector per step (no bank conflict, rows of a wave broadcast).
// (nfull, off, vld: the matrix is the trailing n x n block at offset `off` of an nfull x nfull matrix whose first `off` columns
//  tridiag_stream_kernel has eliminated; reflector k goes to row off + k of V [nfull][vld] at coordinates off..off + n.
//  Stand-alone use: nfull = n, off = 0, vld = TN.)
__global__ __launch_bounds__(1024) void tridiag256_kernel(const float* __restrict__ A, int n, float* __restrict__ D,
                                                          float* __restrict__ E, float* __restrict__ V,
                                                          float* __restrict__ tau, int nfull, int off, int vld) {
  __shared__ __attribute__((aligned(16))) float xs[TN], vs[TN], ps[TN], ws[TN];
  const int tid = threadIdx.x, lane = tid & 63, r = tid >> 2, q = tid & 3;
  const int64_t b = blockIdx.x;
  const float* __restrict__ Ab = A + b * int64_t(nfull) * nfull + int64_t(off) * nfull + off;
  float* __restrict__ Db = D + b * int64_t(nfull) + off;
  float* __restrict__ Eb = E + b * int64_t(nfull) + off;
  float* __restrict__ Vb = V + b * int64_t(nfull) * vld + int64_t(off) * vld + off;
  float* __restrict__ tb = tau + b * int64_t(nfull) + off;
  float a[64];
#pragma unroll
  for (int g = 0; g < 16; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * g + 4 * q + i;
      a[4 * g + i] = (r < n && c < n) ? Ab[int64_t(r) * nfull + c] : 0.f;
    }
  for (int k = 0; k < n - 1; ++k) {
    const int g0 = (k + 1) >> 4;  // column groups below hold columns <= k only
    if (r == k) {
#pragma unroll
      for (int g = 0; g < 16; ++g)
        *reinterpret_cast<float4*>(&xs[16 * g + 4 * q]) = make_float4(a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]);
    }
    __syncthreads();
    // every wave: sigma = sum_{c > k+1} x_c^2 (identical in all waves: same data, same order)
    float sg = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      const float x = xs[c];
      sg += c > k + 1 ? x * x : 0.f;
    }
    sg = wsum64(sg);
    const float alpha = xs[k + 1];
    if (tid == 0) Db[k] = xs[k];
    if (sg == 0.f) {  // nothing to eliminate: H = I
      if (tid == 0) { Eb[k] = alpha; tb[k] = 0.f; }
      __syncthreads();  // xs is rewritten by the next column
      continue;
    }
    const float nrm = sqrtf(alpha * alpha + sg);
    const float beta = alpha >= 0.f ? -nrm : nrm;
    const float t = (beta - alpha) / beta;
    const float inv = 1.f / (alpha - beta);
    if (tid < TN) {
      const float v = tid <= k ? 0.f : (tid == k + 1 ? 1.f : xs[tid] * inv);
      vs[tid] = v;
      Vb[int64_t(k) * vld + tid] = v;  // (embedded use: n == TN, so off + tid < nfull)
    }
    if (tid == 0) { Eb[k] = beta; tb[k] = t; }
    __syncthreads();
    // p = tau A v on the trailing rows
    if (r > k) {
      float part = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if (g >= g0) {
          const float4 v4 = *reinterpret_cast<const float4*>(&vs[16 * g + 4 * q]);
          part = fmaf(a[4 * g], v4.x, part); part = fmaf(a[4 * g + 1], v4.y, part);
          part = fmaf(a[4 * g + 2], v4.z, part); part = fmaf(a[4 * g + 3], v4.w, part);
        }
      part += __shfl_xor(part, 1);
      part += __shfl_xor(part, 2);
      if (q == 0) ps[r] = t * part;
    } else if (q == 0) {
      ps[r] = 0.f;
    }
    __syncthreads();
    // w = p - (tau / 2) (p^T v) v
    float ds = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ds += ps[lane + 64 * j] * vs[lane + 64 * j];
    ds = wsum64(ds);
    const float hd = 0.5f * t * ds;
    if (tid < TN) ws[tid] = ps[tid] - hd * vs[tid];
    __syncthreads();
    // A -= v w^T + w v^T on the trailing block
    if (r > k) {
      const float vr = vs[r], wr = ws[r];
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if (g >= g0) {
          const float4 v4 = *reinterpret_cast<const float4*>(&vs[16 * g + 4 * q]);
          const float4 w4 = *reinterpret_cast<const float4*>(&ws[16 * g + 4 * q]);
          a[4 * g] -= vr * w4.x + wr * v4.x; a[4 * g + 1] -= vr * w4.y + wr * v4.y;
          a[4 * g + 2] -= vr * w4.z + wr * v4.z; a[4 * g + 3] -= vr * w4.w + wr * v4.w;
        }
    }
    // (the next column's row goes to xs, which nobody reads after the second barrier of this step)
  }
  if (r == n - 1) {
#pragma unroll
    for (int g = 0; g < 16; ++g)
      *reinterpret_cast<float4*>(&xs[16 * g + 4 * q]) = make_float4(a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]);
  }
  __syncthreads();
  if (tid == 0) { Db[n - 1] = xs[n - 1]; Eb[n - 1] = 0.f; tb[n - 1] = 0.f; }
}

// Row j of Z (memory row = eigenvector j of T, the solver's column j) -> Q z = H_0 (H_1 (... H_{n-2} z)) into row j of the
// caller's matrix; one wave per eigenvector, lane = 4 coordinates.  Also hands the eigenvalues and the status over.
__global__ __launch_bounds__(256) void backtransform_kernel(const float* __restrict__ Z, int n, const float* __restrict__ V,
                                                            const float* __restrict__ tau, const float* __restrict__ lam,
                                                            const int32_t* __restrict__ info_in, float* __restrict__ out,
                                                            float* __restrict__ W, int32_t* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t b = blockIdx.y;
  if (j >= n) return;
  if (lane == 0) {
    W[b * n + j] = lam[b * n + j];
    if (j == 0) info[b] = info_in[b];
  }
  const float* __restrict__ zr = Z + (b * n + j) * int64_t(n);
  float* __restrict__ orow = out + (b * n + j) * int64_t(n);
  const float* __restrict__ Vb = V + b * int64_t(n) * TN;
  const float* __restrict__ tb = tau + b * int64_t(n);
  float z[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = 4 * lane + i < n ? zr[4 * lane + i] : 0.f;
  for (int k = n - 2; k >= 0; --k) {
    const float t = tb[k];
    if (t == 0.f) continue;
    const float4 v = *reinterpret_cast<const float4*>(Vb + int64_t(k) * TN + 4 * lane);
    float d = v.x * z[0] + v.y * z[1] + v.z * z[2] + v.w * z[3];
    d = wsum64(d) * t;
    z[0] -= d * v.x; z[1] -= d * v.y; z[2] -= d * v.z; z[3] -= d * v.w;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * lane + i < n) orow[4 * lane + i] = z[i];
}

// ---- 256 < n <= 512 (n % 4 == 0): the first n - 256 columns ---------------------------------------------------------------
// 512 x 512 floats are two CUs' register files, so the register-resident kernel above cannot hold the matrix.  One 1024-thread
// workgroup per matrix eliminates the first n - 256 columns with the matrix in global memory (1 MB: L2 resident) by the blocked
// scheme of LAPACK's latrd: panels of 32 columns whose reflectors V and companions W live in LDS ([32][n] each, 128 KiB at
// n = 512), the trailing matrix is READ once per column (p = A v, every thread owns four columns and an eighth of the rows:
// row-contiguous 16-byte loads, no cross-lane reduction) and WRITTEN once per panel (A -= V W^T + W V^T).  The trailing 256 x 256
// block then goes to tridiag256_kernel.  Per column: x = A[k, :] - (V W^T + W V^T)[k, :]; Householder v, tau;
// w = tau (A v - V (W^T v) - W (V^T v)), w -= (tau / 2)(w^T v) v.
constexpr int SNB = 32;   // panel width
constexpr int SRG = 8;    // row groups of the matrix-vector product
__global__ __launch_bounds__(1024) void tridiag_stream_kernel(float* __restrict__ A, int n, int ncols, float* __restrict__ D,
                                                              float* __restrict__ E, float* __restrict__ V,
                                                              float* __restrict__ tau) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* __restrict__ Vp = sm;                    // [SNB][n]
  float* __restrict__ Wp = Vp + SNB * n;          // [SNB][n]
  float* __restrict__ pp = Wp + SNB * n;          // [SRG][n] partial products
  float* __restrict__ xs = pp + SRG * n;          // [n]
  float* __restrict__ vs = xs + n;                // [n]
  float* __restrict__ ps = vs + n;                // [n]
  float* __restrict__ tv = ps + n;                // [SNB] W^T v
  float* __restrict__ tw = tv + SNB;              // [SNB] V^T v
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = tid & 127, rg = tid >> 7, c4 = 4 * cg;
  const int64_t b = blockIdx.x;
  float* __restrict__ Ab = A + b * int64_t(n) * n;
  float* __restrict__ Db = D + b * int64_t(n);
  float* __restrict__ Eb = E + b * int64_t(n);
  float* __restrict__ Vb = V + b * int64_t(n) * n;
  float* __restrict__ tb = tau + b * int64_t(n);
  const int per_lane = (n + 63) >> 6;
  for (int k0 = 0; k0 < ncols; k0 += SNB) {
    const int jn = min(SNB, ncols - k0);
    for (int j = 0; j < jn; ++j) {
      const int k = k0 + j;
      // (1) the current column with the panel's pending update applied (row k of the symmetric matrix: contiguous)
      if (tid < n) {
        float val = 0.f;
        if (tid >= k) {
          val = Ab[int64_t(k) * n + tid];
          float v2 = 0.f;  // (two chains, unrolled: the LDS reads of several panel columns are in flight together)
#pragma unroll 4
          for (int i = 0; i < j; ++i) {
            val -= Vp[i * n + tid] * Wp[i * n + k];
            v2 += Wp[i * n + tid] * Vp[i * n + k];
          }
          val -= v2;
        }
        xs[tid] = val;
      }
      __syncthreads();
      // (2) Householder vector (every wave: the same data in the same order)
      float sg = 0.f;
      for (int q = 0; q < per_lane; ++q) {
        const int c = lane + 64 * q;
        const float x = c < n ? xs[c] : 0.f;
        sg += c > k + 1 ? x * x : 0.f;
      }
      sg = wsum64(sg);
      const float alpha = xs[k + 1];
      float t = 0.f, beta = alpha, inv = 0.f;
      if (sg != 0.f) {
        const float nrm = sqrtf(alpha * alpha + sg);
        beta = alpha >= 0.f ? -nrm : nrm;
        t = (beta - alpha) / beta;
        inv = 1.f / (alpha - beta);
      }
      if (tid < n) {
        const float v = (sg == 0.f || tid <= k) ? 0.f : (tid == k + 1 ? 1.f : xs[tid] * inv);
        vs[tid] = v;
        Vp[j * n + tid] = v;
        Vb[int64_t(k) * n + tid] = v;
      }
      if (tid == 0) { Db[k] = xs[k]; Eb[k] = beta; tb[k] = t; }
      __syncthreads();
      if (sg == 0.f) {  // H = I: w = 0
        if (tid < n) Wp[j * n + tid] = 0.f;
        __syncthreads();
        continue;
      }
      // (3) p = A v over the trailing block (rows and columns > k), W^T v and V^T v of the panel's earlier columns
      {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 + 3 > k && c4 < n) {
          int r = k + 1 + rg;
          // eight rows per step: the loads of a step are all in flight before the first product (the loop is bound by the
          // L2 latency otherwise: four loads per thread gave 91 GB/s into the CU)
          for (; r + 7 * SRG < n; r += 8 * SRG) {
            float4 a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const float4*>(Ab + int64_t(r + u * SRG) * n + c4);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const float vv = vs[r + u * SRG];
              acc.x += a[u].x * vv; acc.y += a[u].y * vv; acc.z += a[u].z * vv; acc.w += a[u].w * vv;
            }
          }
          for (; r < n; r += SRG) {
            const float4 a0 = *reinterpret_cast<const float4*>(Ab + int64_t(r) * n + c4);
            const float v0 = vs[r];
            acc.x += a0.x * v0; acc.y += a0.y * v0; acc.z += a0.z * v0; acc.w += a0.w * v0;
          }
        }
        if (c4 < n) *reinterpret_cast<float4*>(pp + rg * n + c4) = acc;
        for (int i = wave; i < j; i += 16) {
          float s1 = 0.f, s2 = 0.f;
          for (int q = 0; q < per_lane; ++q) {
            const int c = lane + 64 * q;
            if (c < n) { const float v = vs[c]; s1 += Wp[i * n + c] * v; s2 += Vp[i * n + c] * v; }
          }
          s1 = wsum64(s1); s2 = wsum64(s2);
          if (lane == 0) { tv[i] = s1; tw[i] = s2; }
        }
      }
      __syncthreads();
      if (tid < n) {
        float p = 0.f;
        if (tid > k) {
#pragma unroll
          for (int g = 0; g < SRG; ++g) p += pp[g * n + tid];
          float p2 = 0.f;
#pragma unroll 4
          for (int i = 0; i < j; ++i) {
            p -= Vp[i * n + tid] * tv[i];
            p2 += Wp[i * n + tid] * tw[i];
          }
          p -= p2;
        }
        ps[tid] = t * p;
      }
      __syncthreads();
      // (4) w = p - (tau / 2)(p^T v) v
      float ds = 0.f;
      for (int q = 0; q < per_lane; ++q) {
        const int c = lane + 64 * q;
        if (c < n) ds += ps[c] * vs[c];
      }
      ds = wsum64(ds);
      const float hd = 0.5f * t * ds;
      if (tid < n) Wp[j * n + tid] = ps[tid] - hd * vs[tid];
      __syncthreads();
    }
    // trailing update A -= V W^T + W V^T = [V | W] [W | V]^T on rows / columns >= kb: a rank-64 product on the matrix cores
    // (v_mfma_f32_32x32x2_f32, both operands straight from the LDS panels: lanes along rows resp. columns are consecutive
    // addresses), 32 x 32 output tiles dealt to the 16 waves, read-modify-write of the L2-resident matrix.  (As VALU code with
    // the panel operands re-read from LDS per row this update was bound by the LDS pipe: 200 us per panel.)
    const int kb = k0 + jn;
    if (jn < SNB) {  // a partial last panel: the unused panel columns multiply as zeros
      for (int q = tid; q < (SNB - jn) * n; q += 1024) { Vp[jn * n + q] = 0.f; Wp[jn * n + q] = 0.f; }
      __syncthreads();
    }
    {
      const int base = kb & ~31;
      const int nt = (n - base + 31) >> 5;
      const int l31 = lane & 31, lhi = lane >> 5;
      for (int tile = wave; tile < nt * nt; tile += 16) {
        const int tr = tile / nt, tc = tile - tr * nt;
        const int row = base + 32 * tr + l31, col = base + 32 * tc + l31;
        const int rr = row < n ? row : n - 1, cc = col < n ? col : n - 1;  // (clamped: out-of-range lanes are not stored)
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < SNB / 2; ++kk) {
          const int i = 2 * kk + lhi;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vp[i * n + rr], Wp[i * n + cc], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Wp[i * n + rr], Vp[i * n + cc], acc, 0, 0, 0);
        }
        if (col < n) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int r = base + 32 * tr + (q & 3) + 8 * (q >> 2) + 4 * lhi;
            if (r < n) Ab[int64_t(r) * n + col] -= acc[q];
          }
        }
      }
    }
    __syncthreads();
  }
}

// the back-transform for n <= 512: lane holds coordinates 4 lane + 256 q + i, q < 2
__global__ __launch_bounds__(256) void backtransform512_kernel(const float* __restrict__ Z, int n, const float* __restrict__ V,
                                                               const float* __restrict__ tau, const float* __restrict__ lam,
                                                               const int32_t* __restrict__ info_in, float* __restrict__ out,
                                                               float* __restrict__ W, int32_t* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t b = blockIdx.y;
  if (j >= n) return;
  if (lane == 0) {
    W[b * n + j] = lam[b * n + j];
    if (j == 0) info[b] = info_in[b];
  }
  const float* __restrict__ zr = Z + (b * n + j) * int64_t(n);
  float* __restrict__ orow = out + (b * n + j) * int64_t(n);
  const float* __restrict__ Vb = V + b * int64_t(n) * n;
  const float* __restrict__ tb = tau + b * int64_t(n);
  const bool hi = 256 + 4 * lane < n;  // (n % 4 == 0)
  const bool lo = 4 * lane < n;
  float4 z0 = lo ? *reinterpret_cast<const float4*>(zr + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 z1 = hi ? *reinterpret_cast<const float4*>(zr + 256 + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = n - 2; k >= 0; --k) {
    const float t = tb[k];
    if (t == 0.f) continue;
    const float* __restrict__ vk = Vb + int64_t(k) * n;
    const float4 v0 = lo ? *reinterpret_cast<const float4*>(vk + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v1 = hi ? *reinterpret_cast<const float4*>(vk + 256 + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    float d = v0.x * z0.x + v0.y * z0.y + v0.z * z0.z + v0.w * z0.w + v1.x * z1.x + v1.y * z1.y + v1.z * z1.z + v1.w * z1.w;
    d = wsum64(d) * t;
    z0.x -= d * v0.x; z0.y -= d * v0.y; z0.z -= d * v0.z; z0.w -= d * v0.w;
    z1.x -= d * v1.x; z1.y -= d * v1.y; z1.z -= d * v1.z; z1.w -= d * v1.w;
  }
  if (lo) *reinterpret_cast<float4*>(orow + 4 * lane) = z0;
  if (hi) *reinterpret_cast<float4*>(orow + 256 + 4 * lane) = z1;
}

// ---- divide and conquer on the tridiagonal matrix, n <= 256 ---------------------------------------------------------------
// Cuppen's method with the Gu-Eisenstat vector fix, bottom-up in ONE 1024-thread workgroup per matrix (a barrier between the
// phases of a level, no other workgroup involved); tests/test_gpu_tridiag_eig.py::merge_f32 restates one merge in numpy.
// The node i of depth k covers the indices [(i n) >> k, ((i + 1) n) >> k); leaves have size 1, so every off-diagonal entry is the
// split of exactly one node and all of them are torn up front: d_j -= |e_{j-1}| + |e_j|.  Level by level (deepest first) every
// node of two or more indices merges its children: z = [last row of Q_1; sign(e) first row of Q_2] scaled to unit norm,
// a stable rank sort of D, deflation with LAPACK's tolerance 8 eps max(|D|max, |z|max) (tiny components in parallel; the
// close-pair recurrence only in a node where some neighbouring pair meets the criterion, one lane per such node), the secular
// roots by 32 bisection steps on the offset from the nearer pole (four lanes per root), the update vector recomputed from the
// roots, and Q_new = Q U on v_mfma_f32_32x32x2_f32 with U generated on the fly.  The eigenvectors are the ROWS of two n x n
// global buffers used alternately (L2 resident), entries outside a node's block stay the identity's; the eigenvalues and all
// the vectors of a level live in LDS.  Every loop has a fixed trip count; no atomics: two calls give the same bits.
constexpr int DCN = 256;
constexpr float DC_EPS = 5.9604645e-8f;  // LAPACK's slamch('E')
constexpr int DC_BISECT = 32;

struct DcNode { int lo, hi, mid; };
__device__ __forceinline__ DcNode dc_node(int node, int k, int n) {
  return {(node * n) >> k, ((node + 1) * n) >> k, ((2 * node + 1) * n) >> (k + 1)};
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// The secular roots of a level: thread (g = tid / 4, sub = tid % 4), g the absolute index lo + q of root q of its node.  The poles'
// offsets from the origin and the squared weights stay in registers for the first R of a lane's C chunks of 4 (128 VGPRs do not hold
// all 64 pairs beside the rest of the kernel), the other chunks come from d2n / z2n in every step (float4 reads of the node's
// padded slots: poles 1e30, weights 0).
template <int C, int R>
__device__ __forceinline__ void dc_secular(bool active, int lo, int q, int kk, float rho, int sub, const float* __restrict__ dsv,
                                           const float* __restrict__ z2n, const float* __restrict__ d2n,
                                           float* __restrict__ mu, float* __restrict__ lam, float* __restrict__ dov, int g) {
  float dr[4 * R], zr[4 * R];
  const bool last = q == kk - 1;
  const float dj = active ? dsv[lo + q] : 0.f;
  const float dn = (active && !last) ? dsv[lo + q + 1] : dj;
  const float gap = last ? rho : dn - dj;
  const float half = 0.5f * gap;
  float dorg = dj;
  auto load = [&]() {
#pragma unroll
    for (int c = 0; c < R; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = 16 * c + 4 * sub + i;
        dr[4 * c + i] = (active && t < kk) ? dsv[lo + t] - dorg : 1e30f;
      }
  };
  auto eval = [&](float m) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 4 * R; ++c) s = fmaf(zr[c], __builtin_amdgcn_rcpf(dr[c] - m), s);
#pragma unroll
    for (int c = R; c < C; ++c) {
      const float4 zz = *reinterpret_cast<const float4*>(z2n + 16 * c + 4 * sub);
      const float4 dd = *reinterpret_cast<const float4*>(d2n + 16 * c + 4 * sub);
      s = fmaf(zz.x, __builtin_amdgcn_rcpf((dd.x - dorg) - m), s);
      s = fmaf(zz.y, __builtin_amdgcn_rcpf((dd.y - dorg) - m), s);
      s = fmaf(zz.z, __builtin_amdgcn_rcpf((dd.z - dorg) - m), s);
      s = fmaf(zz.w, __builtin_amdgcn_rcpf((dd.w - dorg) - m), s);
    }
    return 1.f + rho * quad_sum(s);
  };
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const float4 zz = *reinterpret_cast<const float4*>(z2n + 16 * c + 4 * sub);
    zr[4 * c] = zz.x; zr[4 * c + 1] = zz.y; zr[4 * c + 2] = zz.z; zr[4 * c + 3] = zz.w;
  }
  load();
  const bool left = last || eval(half) > 0.f;  // the root lies in the left half of its interval: origin d_j
  if (!left) { dorg = dn; load(); }
  float a = left ? 0.f : -half, b = left ? half : 0.f;
  if (last) b = gap;
  for (int it = 0; it < DC_BISECT; ++it) {
    if (C > R) asm volatile("" ::: "memory");  // the LDS chunks are read again in every step: hoisted, they would not fit the registers
    const float m = 0.5f * (a + b);
    if (m == a || m == b) break;  // the interval is one float wide (the four lanes of a root leave together)
    const bool pos = eval(m) > 0.f;
    b = pos ? m : b;
    a = pos ? a : m;
  }
  if (active && sub == 0) {
    const float m = 0.5f * (a + b);
    mu[g] = m;
    lam[g] = dorg + m;
    dov[g] = dorg;
  }
}

__global__ __launch_bounds__(1024) void tridiag_dc_kernel(float* __restrict__ D, const float* __restrict__ E, int n,
                                                          float* __restrict__ Z, float* __restrict__ Zalt,
                                                          int32_t* __restrict__ info) {
  __shared__ float Dc[DCN], es[DCN], zv[DCN], Ds[DCN], zs[DCN], dsv[DCN], zsv[DCN], mu[DCN], lam[DCN], zh[DCN], invn[DCN], dov[DCN], Dd[DCN];
  __shared__ float rc[DCN], rs[DCN];
  __shared__ int nodeof[DCN];
  __shared__ int srow[DCN], sv[DCN], dl[DCN], l1[DCN], l2[DCN], typ[DCN], svrow[DCN], rpj[DCN], rnj[DCN];
  __shared__ __attribute__((aligned(16))) float z2a[2048], d2a[2048];
  __shared__ float n_rho[DCN / 2], n_tol[DCN / 2];
  __shared__ int n_k[DCN / 2], n_k1[DCN / 2], n_k2[DCN / 2], n_flag[DCN / 2], n_nrot[DCN / 2];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t bi = blockIdx.x;
  float* __restrict__ Db = D + bi * n;
  const float* __restrict__ Eb = E + bi * n;
  float* bufs[2] = {Z + bi * int64_t(n) * n, Zalt + bi * int64_t(n) * n};
  if (tid == 0) bad = 0;
  if (tid < DCN) {  // every index list holds indices below n from the start, whatever a later comparison with an overflowed value does
    srow[tid] = 0; sv[tid] = 0; dl[tid] = 0; l1[tid] = 0; l2[tid] = 0; typ[tid] = 0; svrow[tid] = 0;
    rpj[tid] = 0; rnj[tid] = 0;
  }
  __syncthreads();
  if (tid < n) {
    const float d = Db[tid], e = tid < n - 1 ? Eb[tid] : 0.f;
    if (!(fabsf(d) <= 3.0e38f) || !(fabsf(e) <= 3.0e38f)) bad = 1;
    es[tid] = e;
  }
  __syncthreads();
  if (bad) {  // a NaN or Inf: the caller's fallback takes this matrix
    if (tid == 0) info[bi] = 1;
    return;
  }
  if (tid < n) Dc[tid] = Db[tid] - (tid > 0 ? fabsf(es[tid - 1]) : 0.f) - (tid < n - 1 ? fabsf(es[tid]) : 0.f);
  for (int r = wave; r < n; r += 16)
    for (int c = lane; c < n; c += 64) {
      const float v = r == c ? 1.f : 0.f;
      bufs[0][int64_t(r) * n + c] = v;
      bufs[1][int64_t(r) * n + c] = v;
    }
  int L = 0;
  while ((1 << L) < n) ++L;
  int cur = (L + 1) & 1;  // L merges and the final sort each change the buffer: the result lands in Z
  __syncthreads();

  for (int k = L - 1; k >= 0; --k) {
    const int nodes = 1 << k;
    const int mmax = (n + nodes - 1) >> k;
    int stride = 16;  // a node's slot in z2a: a power of two, nodes * stride <= 2048
    while (stride < mmax) stride <<= 1;
    float* __restrict__ src = bufs[cur];
    float* __restrict__ dst = bufs[cur ^ 1];
    // this thread's index t = tid (tid < n) and its node
    const int t = tid;
    int node = 0;
    DcNode nd = {0, 0, 0};
    bool mine = false;
    if (t < n) {
      node = (((t + 1) << k) - 1) / n;
      nd = dc_node(node, k, n);
      mine = nd.hi - nd.lo >= 2;
      nodeof[t] = node;
    }
    const int lo = nd.lo, mid = nd.mid;
    // (A1) z
    if (mine) {
      const float e = es[mid - 1];
      zv[t] = t < mid ? src[int64_t(t) * n + mid - 1] : (e >= 0.f ? 1.f : -1.f) * src[int64_t(t) * n + mid];
    }
    if (tid < nodes) { n_flag[tid] = 0; n_nrot[tid] = 0; n_k[tid] = 0; }
    for (int q = tid; q < nodes * stride; q += 1024) { z2a[q] = 0.f; d2a[q] = 1e30f; }
    __syncthreads();
    // (A2) norm, tolerance, stable rank sort, the tiny components: four lanes per index g, each a quarter of the node
    {
      const int g = tid >> 2, sub = tid & 3;
      int gnode = 0;
      DcNode b = {0, 0, 0};
      if (g < n) {
        gnode = (((g + 1) << k) - 1) / n;
        b = dc_node(gnode, k, n);
      }
      const bool gmine = b.hi - b.lo >= 2;
      float nrm2 = 0.f, zmax = 0.f, dmax = 0.f;
#pragma unroll 4
      for (int j = b.lo + sub; j < b.hi; j += 4) {
        const float zz = zv[j];
        nrm2 = fmaf(zz, zz, nrm2);
        zmax = fmaxf(zmax, fabsf(zz));
        dmax = fmaxf(dmax, fabsf(Dc[j]));
      }
      nrm2 = quad_sum(nrm2);
      zmax = fmaxf(zmax, __shfl_xor(zmax, 1)); zmax = fmaxf(zmax, __shfl_xor(zmax, 2));
      dmax = fmaxf(dmax, __shfl_xor(dmax, 1)); dmax = fmaxf(dmax, __shfl_xor(dmax, 2));
      const float inv = nrm2 > 0.f ? 1.f / sqrtf(nrm2) : 0.f;
      const float rho = gmine ? fabsf(es[b.mid - 1]) * nrm2 * (inv > 0.f ? 1.f : 0.f) : 0.f;
      const float gtol = 8.f * DC_EPS * fmaxf(dmax, zmax * inv);
      const float myz = gmine ? zv[g] * inv : 0.f, myD = gmine ? Dc[g] : 0.f;
      const bool mytiny = !(rho * fabsf(myz) > gtol);
      int rank = 0, kq = 0, ktot = 0, q1 = 0, k1tot = 0;
#pragma unroll 4
      for (int j = b.lo + sub; j < b.hi; j += 4) {
        const float Dj = Dc[j];
        const bool before = Dj < myD || (Dj == myD && j < g);
        const bool keep = rho * fabsf(zv[j] * inv) > gtol;
        rank += before;
        kq += before && keep;
        ktot += keep;
        q1 += before && keep && j < b.mid;
        k1tot += keep && j < b.mid;
      }
      rank += __shfl_xor(rank, 1); rank += __shfl_xor(rank, 2);
      kq += __shfl_xor(kq, 1); kq += __shfl_xor(kq, 2);
      ktot += __shfl_xor(ktot, 1); ktot += __shfl_xor(ktot, 2);
      q1 += __shfl_xor(q1, 1); q1 += __shfl_xor(q1, 2);
      k1tot += __shfl_xor(k1tot, 1); k1tot += __shfl_xor(k1tot, 2);
      if (gmine && sub == 0) {
        const int p = b.lo + rank;
        Ds[p] = myD; zs[p] = myz; srow[p] = g; typ[p] = g < b.mid ? 1 : 2;
        if (!mytiny) {
          sv[b.lo + kq] = p;
          if (g < b.mid) l1[b.lo + q1] = kq; else l2[b.lo + kq - q1] = kq;
        } else {
          dl[b.lo + rank - kq] = p;
          Dd[b.lo + rank - kq] = myD;
        }
        if (g == b.lo) { n_rho[gnode] = rho; n_tol[gnode] = gtol; n_k[gnode] = ktot; n_k1[gnode] = k1tot; n_k2[gnode] = ktot - k1tot; }
      }
    }
    __syncthreads();
    // (A3) does any neighbouring pair of survivors deflate?
    if (mine) {
      const int q = t - lo;
      if (q >= 1 && q < n_k[node]) {
        const int p = sv[lo + q], pp = sv[lo + q - 1];
        const float s = zs[pp], c = zs[p], tt = Ds[p] - Ds[pp];
        if (fabsf(tt * c * s) <= n_tol[node] * (c * c + s * s)) n_flag[node] = 1;  // |t c s| / tau^2 <= tol
      }
    }
    __syncthreads();
    const int any = __syncthreads_or(tid < nodes && n_flag[tid] != 0);
    if (any) {
      // (B) the close-pair recurrence, one lane per flagged node: rotations recorded, lists rebuilt.  The sorted arrays are only
      // read here and the entry under comparison is carried in registers, so the reads of the next entries do not wait for
      // this entry's stores; the survivors' values go straight to their compact places.
      if (tid < nodes && n_flag[tid]) {
        const DcNode b = dc_node(tid, k, n);
        const float rho = n_rho[tid], btol = n_tol[tid];
        int ks = 0, k1 = 0, k2 = 0, ndef = 0, nr = 0, prev = -1, typrev = 0;
        float zprev = 0.f, dprev = 0.f;
        auto emit = [&]() {
          sv[b.lo + ks] = prev; dsv[b.lo + ks] = dprev; zsv[b.lo + ks] = zprev;
          if (typrev & 1) l1[b.lo + k1++] = ks;
          if (typrev & 2) l2[b.lo + k2++] = ks;
          ++ks;
        };
#pragma unroll 4
        for (int p = b.lo; p < b.hi; ++p) {
          const float zp = zs[p], dp = Ds[p];
          const int tp = typ[p];
          if (!(rho * fabsf(zp) > btol)) { dl[b.lo + ndef] = p; Dd[b.lo + ndef] = dp; ++ndef; continue; }
          if (prev >= 0) {
            const float tt = dp - dprev, tau2 = zp * zp + zprev * zprev;
            if (fabsf(tt * zp * zprev) <= btol * tau2) {  // |t c s| <= tol with c = zp / tau, s = -zprev / tau
              const float tau = sqrtf(tau2), c = zp / tau, s = -zprev / tau;
              rpj[b.lo + nr] = prev; rnj[b.lo + nr] = p; rc[b.lo + nr] = c; rs[b.lo + nr] = s; ++nr;
              dl[b.lo + ndef] = prev; Dd[b.lo + ndef] = dprev * c * c + dp * s * s; ++ndef;
              dprev = dprev * s * s + dp * c * c;
              zprev = tau;
              typrev = typrev != tp ? 3 : tp;  // the rotated vector has entries in both halves
              prev = p;
              continue;
            }
            emit();
          }
          prev = p; zprev = zp; dprev = dp; typrev = tp;
        }
        if (prev >= 0) emit();
        n_k[tid] = ks; n_k1[tid] = k1; n_k2[tid] = k2; n_nrot[tid] = nr;
      }
      __syncthreads();
      // the rotations, in order, on this thread's column of the node's block.  A chain of rotations hands its second row on in
      // a register; the rows a group of four rotations reads have not been written before, so all are loaded first.
      if (mine) {
        const int nr = n_nrot[node];
        float carry = 0.f;
        int last = -1;
        for (int r0 = 0; r0 < nr; r0 += 4) {
          float x[4], y[4];
          int pj[4], nj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = min(r0 + u, nr - 1);
            pj[u] = rpj[lo + r]; nj[u] = rnj[lo + r];
            x[u] = src[int64_t(srow[pj[u]]) * n + t];
            y[u] = src[int64_t(srow[nj[u]]) * n + t];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (r0 + u < nr) {
              const float c = rc[lo + r0 + u], sn = rs[lo + r0 + u];
              float xx = x[u];
              if (pj[u] == last) xx = carry;
              else if (last >= 0) src[int64_t(srow[last]) * n + t] = carry;
              src[int64_t(srow[pj[u]]) * n + t] = c * xx + sn * y[u];
              carry = c * y[u] - sn * xx;
              last = nj[u];
            }
          }
        }
        if (last >= 0) src[int64_t(srow[last]) * n + t] = carry;
      }
      __syncthreads();
    }
    // (C0) the survivors, compact
    const int kk = mine ? n_k[node] : 0;
    if (mine && t - lo < kk) {
      const int p = sv[t];
      const bool scanned = n_flag[node] != 0;  // (B) has written the survivors' values itself
      const float zz = scanned ? zsv[t] : zs[p], dd = scanned ? dsv[t] : Ds[p];
      dsv[t] = dd; zsv[t] = zz; svrow[t] = srow[p];
      z2a[node * stride + (t - lo)] = zz * zz;
      d2a[node * stride + (t - lo)] = dd;
    }
    __syncthreads();
    // (C) secular roots, four lanes per root
    {
      const int g = tid >> 2, sub = tid & 3;
      int gnode = 0, glo = 0, gk = 0;
      bool active = false;
      if (g < n) {
        gnode = (((g + 1) << k) - 1) / n;
        const DcNode b = dc_node(gnode, k, n);
        glo = b.lo;
        gk = b.hi - b.lo >= 2 ? n_k[gnode] : 0;
        active = g - glo < gk;
      }
      const float rho = active ? n_rho[gnode] : 0.f;
      const float* z2n = z2a + (active ? gnode * stride : 0);
      const float* d2n = d2a + (active ? gnode * stride : 0);
      const int q = g - glo;
      if (stride <= 16) dc_secular<1, 1>(active, glo, q, gk, rho, sub, dsv, z2n, d2n, mu, lam, dov, g);
      else if (stride <= 32) dc_secular<2, 2>(active, glo, q, gk, rho, sub, dsv, z2n, d2n, mu, lam, dov, g);
      else if (stride <= 64) dc_secular<4, 4>(active, glo, q, gk, rho, sub, dsv, z2n, d2n, mu, lam, dov, g);
      else if (stride <= 128) dc_secular<8, 4>(active, glo, q, gk, rho, sub, dsv, z2n, d2n, mu, lam, dov, g);
      else dc_secular<16, 4>(active, glo, q, gk, rho, sub, dsv, z2n, d2n, mu, lam, dov, g);
      __syncthreads();
      // (D) the update vector for which these roots are exact: a product of ratios of the same shifted differences
      float prod = 1.f;
      const float di = active ? dsv[g] : 0.f;
#pragma unroll 4
      for (int j = sub; j < (active ? gk : 0); j += 4) {
        const float num = (dov[glo + j] - di) + mu[glo + j];
        const float den = j == q ? 1.f : dsv[glo + j] - di;
        prod *= num / den;
      }
      prod *= __shfl_xor(prod, 1);
      prod *= __shfl_xor(prod, 2);
      if (active && sub == 0) zh[g] = copysignf(sqrtf(fabsf(prod / rho)), zsv[g]);
      __syncthreads();
      // (E) the eigenvectors' norms
      float s2 = 0.f;
      if (active) {
        const float dorg = dov[g], mj = mu[g];
#pragma unroll 4
        for (int i = sub; i < gk; i += 4) {
          const float u = zh[glo + i] / ((dsv[glo + i] - dorg) - mj);
          s2 = fmaf(u, u, s2);
        }
      }
      s2 = quad_sum(s2);
      if (active && sub == 0) invn[g] = 1.f / sqrtf(s2);
      __syncthreads();
    }
    // (F) rows of the new vectors: U^T (kk x kk, generated) times the surviving rows, 32 x 32 tiles dealt to the waves.  A
    // tile whose columns lie in one half only meets the survivors that came from that half (or were rotated across).
    {
      const int l31 = lane & 31, lhi = lane >> 5;
      auto do_tile = [&](const DcNode& b, int bk, int bk1, int bk2, int tr, int tc) {
        const int c0 = b.lo + 32 * tc, c1 = min(c0 + 32, b.hi);
        const int* list = nullptr;
        int cnt = bk;
        if (c1 <= b.mid) { list = l1 + b.lo; cnt = bk1; }
        else if (c0 >= b.mid) { list = l2 + b.lo; cnt = bk2; }
        const int j = 32 * tr + l31;
        const bool rowok = j < bk;
        const int jj = rowok ? j : 0;
        const float dorg = dov[b.lo + jj], mj = mu[b.lo + jj], inj = rowok ? invn[b.lo + jj] : 0.f;
        const int col = c0 + l31;
        const bool colok = col < b.hi;
        const int colc = colok ? col : b.hi - 1;
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int s = 0; s < cnt; s += 8) {  // four steps' operands in flight (steps past the end multiply zeros)
          float av[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int idx = s + 2 * u + lhi;
            const bool ok = idx < cnt;
            const int ic = ok ? idx : 0;
            const int qi = list ? list[ic] : ic;
            const float bb = src[int64_t(svrow[b.lo + qi]) * n + colc];
            const float aa = zh[b.lo + qi] * inj * __builtin_amdgcn_rcpf((dsv[b.lo + qi] - dorg) - mj);
            av[u] = ok ? aa : 0.f;
            bv[u] = (ok && colok) ? bb : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
        if (colok) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int r = 32 * tr + (q & 3) + 8 * (q >> 2) + 4 * lhi;
            if (r < bk) dst[int64_t(b.lo + r) * n + col] = acc[q];
          }
        }
      };
      if (mmax <= 32) {  // one tile per node
        for (int nn = wave; nn < nodes; nn += 16) {
          const DcNode b = dc_node(nn, k, n);
          const int bk = b.hi - b.lo >= 2 ? n_k[nn] : 0;
          if (bk > 0) do_tile(b, bk, bk, bk, 0, 0);  // (the node's own lists are not needed: every tile straddles or is whole)
        }
      } else {
        int item = 0;
        for (int nn = 0; nn < nodes; ++nn) {
          const DcNode b = dc_node(nn, k, n);
          const int bk = n_k[nn], bk1 = n_k1[nn], bk2 = n_k2[nn];
          const int rt = (bk + 31) >> 5, ct = (b.hi - b.lo + 31) >> 5;
          for (int tile = 0; tile < rt * ct; ++tile, ++item)
            if ((item & 15) == wave) do_tile(b, bk, bk1, bk2, tile / ct, tile % ct);
        }
      }
      // the deflated rows, copied; the new eigenvalues
      int sh = 4;
      while ((1 << sh) < stride) ++sh;
#pragma unroll 4
      for (int idx = tid; idx < (n << sh); idx += 1024) {
        const int g = idx >> sh, gnode = nodeof[g];
        const DcNode b = dc_node(gnode, k, n);
        const int c = b.lo + (idx & (stride - 1)), bk = n_k[gnode], q = g - b.lo;
        if (b.hi - b.lo >= 2 && q >= bk && c < b.hi) dst[int64_t(g) * n + c] = src[int64_t(srow[dl[g - bk]]) * n + c];
      }
      if (mine) Dc[t] = t - lo < kk ? lam[t] : Dd[t - kk];
    }
    __syncthreads();
    cur ^= 1;
  }
  // ascending order (stable), rows to Z
  {
    const float* __restrict__ src = bufs[cur];
    float* __restrict__ dst = bufs[cur ^ 1];
    {
      const int g = tid >> 2, sub = tid & 3;
      const float myD = g < n ? Dc[g] : 0.f;
      int rank = 0;
#pragma unroll 4
      for (int j = sub; j < n; j += 4) {
        const float Dj = Dc[j];
        rank += Dj < myD || (Dj == myD && j < g);
      }
      rank += __shfl_xor(rank, 1); rank += __shfl_xor(rank, 2);
      if (g < n && sub == 0) { srow[rank] = g; Db[rank] = myD; }
    }
    __syncthreads();
#pragma unroll 2
    for (int r = wave; r < n; r += 16) {
      const int sr = srow[r];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        if (c < n) dst[int64_t(r) * n + c] = src[int64_t(sr) * n + c];
      }
    }
    if (tid == 0) info[bi] = 0;
  }
}

int stedc_branch(int br, int branches, int64_t n, int64_t batch, hipStream_t st) {
  if (rocblas_set_stream(g_bh[br], st) != rocblas_status_success) { set_error("rocblas_set_stream failed"); return 3; }
  for (int64_t b = br; b < batch; b += branches) {
    const rocblas_status rs = rocsolver_sstedc(g_bh[br], rocblas_evect_tridiagonal, rocblas_int(n), scratch().d.as<float>() + b * n,
                                               scratch().e.as<float>() + b * n, scratch().z.as<float>() + b * n * n, rocblas_int(n),
                                               scratch().info.as<int32_t>() + b);
    if (rs != rocblas_status_success) { set_error("rocsolver_sstedc failed"); return 3; }
  }
  return 0;
}

// eigenpairs of the tridiagonal matrices in scratch().d / scratch().e -> scratch().d (values), scratch().z (vectors), scratch().info; on stream s
int stedc_all(int64_t n, int64_t batch, hipStream_t s) {
  const int branches = int(std::min<int64_t>(batch, kBranches));
  for (int i = 0; i < branches; ++i) {
    if (!g_bh[i] && rocblas_create_handle(&g_bh[i]) != rocblas_status_success) { set_error("rocblas_create_handle failed"); return 3; }
    if (i > 0 && !g_side[i]) LGNN_HIP_CHECK(hipStreamCreateWithFlags(&g_side[i], hipStreamNonBlocking));
    if (!g_join[i]) LGNN_HIP_CHECK(hipEventCreateWithFlags(&g_join[i], hipEventDisableTiming));
  }
  if (!g_fork) LGNN_HIP_CHECK(hipEventCreateWithFlags(&g_fork, hipEventDisableTiming));
  if (branches == 1) {
    for (int i = 0; i < branches; ++i) LGNN_CALL(stedc_branch(i, branches, n, batch, s));
    return 0;
  }
  LGNN_HIP_CHECK(hipEventRecord(g_fork, s));
  for (int i = 0; i < branches; ++i) {
    hipStream_t st = i == 0 ? s : g_side[i];
    if (i > 0) LGNN_HIP_CHECK(hipStreamWaitEvent(st, g_fork, 0));
    LGNN_CALL(stedc_branch(i, branches, n, batch, st));
    if (i > 0) {
      LGNN_HIP_CHECK(hipEventRecord(g_join[i], st));
      LGNN_HIP_CHECK(hipStreamWaitEvent(s, g_join[i], 0));
    }
  }
  return 0;
}
}  // namespace
}  // namespace lgnn

namespace lgnn {
// the process-wide rocBLAS handle, bound to stream `s` (also used by jacobian.hip); nullptr on failure
void* blas_handle(hipStream_t s) {
  if (!g_handle && rocblas_create_handle(&g_handle) != rocblas_status_success) return nullptr;
  if (rocblas_set_stream(g_handle, s) != rocblas_status_success) return nullptr;
  return g_handle;
}
}  // namespace lgnn

using namespace lgnn;

// Eigenpairs of `batch` symmetric tridiagonal matrices of n <= 256 rows (diagonal d [batch][n], off-diagonal e [batch][n], the
// last entry of a row unused): d <- eigenvalues ascending, row j of Z [batch][n][n] <- eigenvector j, info[b] = 1 where d or e
// holds a NaN or Inf (that matrix's d and Z are then left alone), else 0.  Asynchronous on `stream`.
extern "C" int lgnn_tridiag_eig(float* d, float* e, int64_t n, int64_t batch, float* Z, int32_t* info, void* stream) {
  if (!d || !e || !Z || !info) { set_error("null argument"); return 2; }
  LGNN_REQUIRE(n > 0 && n <= DCN && batch > 0 && batch <= 65535, "tridiag_eig: bad shape");
  hipStream_t s = static_cast<hipStream_t>(stream);
  LGNN_CALL(scratch().z2.reserve(size_t(batch) * n * n * 4));
  hipLaunchKernelGGL(tridiag_dc_kernel, dim3(unsigned(batch)), dim3(1024), 0, s, d, e, int(n), Z, scratch().z2.as<float>(), info);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// A: [batch][n][n] fp32, symmetric, overwritten: row j of matrix b = eigenvector j (unit norm) for eigenvalue W[b][j],
// eigenvalues ascending (column-major eigenvector columns of the solver == rows of the row-major view).
// info: device int32 [batch], 0 = converged.  Asynchronous on `stream` (apart from workspace growth on first use).
extern "C" int lgnn_symeig_batched(float* A, int64_t n, int64_t batch, float* W, int32_t* info, void* stream) {
  if (!A || !W || !info) { set_error("null argument"); return 2; }
  LGNN_REQUIRE(n > 0 && n <= 32768 && batch > 0 && batch <= 65535, "symeig: bad shape");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (neither branch touches the shared g_handle: the divide and conquer chains have handles of their own, g_bh, and the
  //  library path g_eig_handle -- queued main-stream work that uses g_handle is never rebound to a side stream from here)
  if (n <= TN && n >= 2) {
    LGNN_CALL(scratch().e.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().v.reserve(size_t(batch) * n * TN * 4));
    LGNN_CALL(scratch().tau.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().d.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().z.reserve(size_t(batch) * n * n * 4));
    LGNN_CALL(scratch().z2.reserve(size_t(batch) * n * n * 4));
    LGNN_CALL(scratch().info.reserve(size_t(batch) * 4));
    hipLaunchKernelGGL(tridiag256_kernel, dim3(unsigned(batch)), dim3(1024), 0, s, A, int(n), scratch().d.as<float>(),
                       scratch().e.as<float>(), scratch().v.as<float>(), scratch().tau.as<float>(), int(n), 0, TN);
    LGNN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tridiag_dc_kernel, dim3(unsigned(batch)), dim3(1024), 0, s, scratch().d.as<float>(), scratch().e.as<float>(),
                       int(n), scratch().z.as<float>(), scratch().z2.as<float>(), scratch().info.as<int32_t>());
    LGNN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(backtransform_kernel, dim3(unsigned(cdiv(n, 4)), unsigned(batch)), dim3(256), 0, s, scratch().z.as<float>(),
                       int(n), scratch().v.as<float>(), scratch().tau.as<float>(), scratch().d.as<float>(), scratch().info.as<int32_t>(), A, W, info);
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  }
  if (n > TN && n <= 2 * TN && n % 4 == 0) {
    // 256 < n <= 512: n - 256 columns by the streaming kernel, the trailing 256 x 256 block by the register-resident one,
    // divide and conquer on the tridiagonal matrix (library), back-transform: four launches + the library's chain
    LGNN_CALL(scratch().e.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().v.reserve(size_t(batch) * n * n * 4));
    LGNN_CALL(scratch().tau.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().d.reserve(size_t(batch) * n * 4));
    LGNN_CALL(scratch().z.reserve(size_t(batch) * n * n * 4));
    LGNN_CALL(scratch().info.reserve(size_t(batch) * 4));
    const size_t smem = size_t(2 * SNB * n + SRG * n + 3 * n + 2 * SNB) * 4;
    LGNN_REQUIRE(smem <= 160 * 1024, "symeig: panel does not fit the LDS");
    LGNN_CALL(lds_opt_in<&tridiag_stream_kernel>(160 * 1024));
    LGNN_HIP_CHECK(hipMemsetAsync(scratch().v.p, 0, size_t(batch) * n * n * 4, s));  // (the trailing block's reflectors start at column n - 256)
    hipLaunchKernelGGL(tridiag_stream_kernel, dim3(unsigned(batch)), dim3(1024), smem, s, A, int(n), int(n - TN),
                       scratch().d.as<float>(), scratch().e.as<float>(), scratch().v.as<float>(), scratch().tau.as<float>());
    LGNN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tridiag256_kernel, dim3(unsigned(batch)), dim3(1024), 0, s, A, TN, scratch().d.as<float>(), scratch().e.as<float>(),
                       scratch().v.as<float>(), scratch().tau.as<float>(), int(n), int(n - TN), int(n));
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(stedc_all(n, batch, s));
    hipLaunchKernelGGL(backtransform512_kernel, dim3(unsigned(cdiv(n, 4)), unsigned(batch)), dim3(256), 0, s, scratch().z.as<float>(),
                       int(n), scratch().v.as<float>(), scratch().tau.as<float>(), scratch().d.as<float>(), scratch().info.as<int32_t>(), A, W, info);
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  }
  if (!g_eig_handle && rocblas_create_handle(&g_eig_handle) != rocblas_status_success) { set_error("rocBLAS handle"); return 3; }
  if (rocblas_set_stream(g_eig_handle, s) != rocblas_status_success) { set_error("rocBLAS stream setup failed"); return 3; }
  LGNN_CALL(scratch().e_large.reserve(size_t(batch) * n * 4));
  const rocblas_status st = rocsolver_ssyevd_strided_batched(
      g_eig_handle, rocblas_evect_original, rocblas_fill_upper, rocblas_int(n), A, rocblas_int(n), rocblas_stride(n * n), W,
      rocblas_stride(n), scratch().e_large.as<float>(), rocblas_stride(n), info, rocblas_int(batch));
  if (st != rocblas_status_success) { set_error("rocsolver_ssyevd_strided_batched failed"); return 3; }
  return 0;
}
