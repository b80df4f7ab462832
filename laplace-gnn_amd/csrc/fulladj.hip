// Full posterior, adjacency gradient: the product of a chunk's Jacobian rows with the dense weighting
//     Gamma = d(1/2 logdet(f H + Delta)) / dH = (f / 2) (f H + Delta)^-1        [P, P], symmetric
// (FullLaplace, laplace/baselaplace.py:1377-1505; the curvature it differentiates: laplace/curvature/curvature.py:374-410 with the
// fork's attached Jacobians, :89-130; the loop that asks for it: gnn/marglik_training.py:197-216 under --hessian_structure full,
// gnn/utils.py:57-59).  One pass over Z = J Gamma gives both inputs of adjgrad_ext.hip's tangent / reverse chain,
//     K_n = (J_n Gamma) J_n^T   [C, C]            R_n = 2 Lambda_n (J_n Gamma)   [C, P],   Lambda_n = diag(p) - p p^T,
// without Z ever reaching memory.
#include "lgnn_internal.h"
#include "mfma_tile.h"  // f32x16

namespace lgnn {
namespace {

constexpr int FBM = 128, FBN = 128, FBK = 32, FHALF = 64;
constexpr int FZLD = FHALF + 1;  // odd stride of the staged accumulator half: row walks and column walks are conflict free

// Z tile = J[rows of whole samples, :] Gamma[:, 128 columns]: gemm_kernel's fp32 MFMA 32x32x2 tile (128 x 128 x 32, A with an
// odd LDS stride).  A row tile holds nsamp = floor(128 / C) whole samples (rt = nsamp * C rows, the rest of the 128 rows stay
// zero), so the finished accumulator can be mixed by Lambda_n inside the workgroup: it goes through LDS in two halves of 64
// columns (the K loop's staging buffers are reused, 33 KB in all), and per half
//   R[q, col]      = 2 p_c (Z[q, col] - sum_k p_k Z[(m, k), col])                      one store per element, q = (m, c)
//   K_n[a, b]     += sum_col Z[(m, a), col] J[(m, b), col]                              one wave reduction per (m, a, b)
// K_n's partial sums over the column blocks are combined with float atomics (as the adjacency gradient's other accumulators): K_n is
// zeroed by the launcher, and the order of the P / 64 additions per entry is not fixed.  R needs the complete K_n only through
// out_bar (diag_ext_sample_kernel, which runs after this kernel), so one pass is enough.  p = softmax of the model's own logits
// at idx, computed as diag_ext_sample_kernel computes it; a sample with an id outside [0, N) gets p = 0 (R = 0).
// Gamma is read as stored (row k, columns of the block); its symmetry is what makes that the same as the column walk.
// Ragged edges: rows past Q, columns past P and k past P are zero-filled at the loads and skipped at the stores.
__global__ __launch_bounds__(256, 2) void full_direction_kernel(const float* __restrict__ J, const float* __restrict__ G,
                                                             const int64_t* __restrict__ idx,
                                                             const float* __restrict__ logits, int64_t N, int64_t Q, int C,
                                                             int64_t P, int rt, int vec, float* __restrict__ R,
                                                             float* __restrict__ Kn) {
  __shared__ float smem[FBM * (FBK + 1) + FBK * FBN];  // As | Bs in the K loop, then Zs [128][65]
  __shared__ float ps[FBM];                            // p of every tile row's (sample, class)
  static_assert(FBM * FZLD <= FBM * (FBK + 1) + FBK * FBN, "the staged half fits the K loop's buffers");
  float (*As)[FBK + 1] = reinterpret_cast<float (*)[FBK + 1]>(smem);
  float (*Bs)[FBN] = reinterpret_cast<float (*)[FBN]>(smem + FBM * (FBK + 1));
  float (*Zs)[FZLD] = reinterpret_cast<float (*)[FZLD]>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t row0 = int64_t(blockIdx.x) * rt, col0 = int64_t(blockIdx.y) * FBN;
  const int rows = int(min(int64_t(rt), Q - row0));  // valid rows of this tile: whole samples (Q is a multiple of C)
  const int nsamp = rows / C;
  const int64_t m_first = row0 / C;

  if (tid < nsamp) {
    const int64_t n = idx[m_first + tid];
    float* p = ps + tid * C;
    if (n < 0 || n >= N) {
      for (int c = 0; c < C; ++c) p[c] = 0.f;
    } else {
      float mx = -INFINITY, sum = 0.f;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, logits[n * C + c]);
      for (int c = 0; c < C; ++c) { p[c] = expf(logits[n * C + c] - mx); sum += p[c]; }
      for (int c = 0; c < C; ++c) p[c] /= sum;
    }
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // The next k step's global loads are issued before this step's MFMAs and stored to LDS after them (register prefetch):
  // A tile 128 rows x 32 k, thread -> (row = tid/8 + 32*it, k4 = (tid%8)*4);  B tile 32 k x 128 cols, thread -> (k = tid/32 +
  // 8*it, c4 = (tid%32)*4)
  float xa[4][4], xb[4][4];
  auto fetch = [&](int64_t k0) {
    const int kvalid = int(min(int64_t(FBK), P - k0));
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = (tid >> 3) + 32 * it, k4 = (tid & 7) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) xa[it][q] = 0.f;
      if (r < rows) {
        const float* src = J + (row0 + r) * P + k0 + k4;
        if (vec && k4 + 4 <= kvalid) {
          const float4 t = *reinterpret_cast<const float4*>(src);
          xa[it][0] = t.x; xa[it][1] = t.y; xa[it][2] = t.z; xa[it][3] = t.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (k4 + q < kvalid) xa[it][q] = src[q];
        }
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int k = (tid >> 5) + 8 * it, c4 = (tid & 31) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) xb[it][q] = 0.f;
      if (k < kvalid) {
        const float* src = G + (k0 + k) * P + col0 + c4;
        if (vec && col0 + c4 + 4 <= P) {
          const float4 t = *reinterpret_cast<const float4*>(src);
          xb[it][0] = t.x; xb[it][1] = t.y; xb[it][2] = t.z; xb[it][3] = t.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (col0 + c4 + q < P) xb[it][q] = src[q];
        }
      }
    }
  };
  fetch(0);
  for (int64_t k0 = 0; k0 < P; k0 += FBK) {
    const int kvalid = int(min(int64_t(FBK), P - k0));
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = (tid >> 3) + 32 * it, k4 = (tid & 7) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) As[r][k4 + q] = xa[it][q];
      const int k = (tid >> 5) + 8 * it, c4 = (tid & 31) * 4;
      *reinterpret_cast<float4*>(&Bs[k][c4]) = make_float4(xb[it][0], xb[it][1], xb[it][2], xb[it][3]);
    }
    __syncthreads();
    if (k0 + FBK < P) fetch(k0 + FBK);
    const int ksteps = (kvalid + 1) >> 1;
    for (int kk = 0; kk < ksteps; ++kk) {
      const int k = kk * 2 + lhi;
      float av[2], bv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) av[m] = As[wr * 64 + m * 32 + l31][k];
#pragma unroll
      for (int n = 0; n < 2; ++n) bv[n] = Bs[k][wc * 64 + n * 32 + l31];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
  }

  for (int half = 0; half < 2; ++half) {
    if (wc == half) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            Zs[wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi][n * 32 + l31] = acc[m][n][r];
    }
    __syncthreads();
    const int64_t col = col0 + half * FHALF + lane;  // this lane's column in both passes
    // R: wave w takes the samples w, w + 4, ...; 64 consecutive columns per store
    if (col < P) {
      for (int sm = wave; sm < nsamp; sm += 4) {
        const float* __restrict__ p = ps + sm * C;
        float zb = 0.f;
        for (int k = 0; k < C; ++k) zb += p[k] * Zs[sm * C + k][lane];
        float* __restrict__ out = R + (row0 + sm * C) * P + col;
        for (int c = 0; c < C; ++c) out[c * P] = 2.f * p[c] * (Zs[sm * C + c][lane] - zb);
      }
    }
    // K_n: wave w takes the tile rows t = (m, b) = w, w + 4, ...; one J value per lane, C reductions
    for (int t = wave; t < rows; t += 4) {
      const int sm = t / C, b = t - sm * C;
      const float jv = col < P ? J[(row0 + t) * P + col] : 0.f;
      float* __restrict__ kout = Kn + (m_first + sm) * C * C + b;
      for (int a = 0; a < C; ++a) {
        float v = Zs[sm * C + a][lane] * jv;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) atomicAdd(&kout[a * C], v);
      }
    }
    __syncthreads();  // the next half overwrites Zs
  }
}

}  // namespace

int launch_full_directions(const float* J, const float* Gamma, const int64_t* idx, const float* logits, int64_t N,
                           int64_t mc, int64_t C, int64_t P, float* R, float* Kn, hipStream_t s) {
  LGNN_REQUIRE(C >= 1 && C <= 127, "adjacency gradient, full posterior: at most 127 classes");
  LGNN_REQUIRE(mc > 0 && P > 0, "adjacency gradient, full posterior: empty chunk");
  const int rt = int(FBM / C * C);
  const int64_t row_tiles = cdiv(mc * C, rt), col_blocks = cdiv(P, FBN);
  LGNN_REQUIRE(row_tiles < (int64_t(1) << 31) && col_blocks < 65536, "adjacency gradient, full posterior: chunk too large");
  const int vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(J) | reinterpret_cast<uintptr_t>(Gamma)) & 15) == 0;
  LGNN_HIP_CHECK(hipMemsetAsync(Kn, 0, size_t(mc) * C * C * 4, s));
  // blockIdx.x walks the row tiles: the workgroups that share a column block of Gamma run next to each other
  hipLaunchKernelGGL(full_direction_kernel, dim3(unsigned(row_tiles), unsigned(col_blocks)), dim3(256), 0, s, J, Gamma, idx,
                     logits, N, mc * C, int(C), P, rt, vec, R, Kn);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn
