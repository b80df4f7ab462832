// Functional (GP) Laplace: the kernel k(x, x') = J(x) J(x')^T of the linearised model and its products with a parameter
// vector, without the Jacobians where the model has a closed form.
//
// Reference: FunctionalLaplace (laplace/baselaplace.py:1922-2960) forms Js [b, C, P] of two batches by jacrev and contracts
// them (_kernel_batch :2684-2715, _kernel_star :2717-2747, _kernel_batch_star :2749-2776): 2 (M C)^2 P flops and M C P floats.
//
// Structured route (1- and 2-layer GCN / GraphSAGE without res / norm).  With the notation of jac_closed_form_kernel
// (jacobian.hip): a = node of sample n, E[u] = [first Linear's input at u | its bias entry], d_u = act'(h_1[u]),
//   GCN        T_n[h, :]  = sum_u P[a, u] d_u[h] E[u, :]
//   GraphSAGE  Ts_n[h, :] = d_a[h] [cat_0[a] | 1],   Tn_n[h, :] = sum_u P[a, u] d_u[h] [cat_0[u] | 1],   W_1 = [Ws | Wn]
//   K[(n, c), (m, e)] = sum_h sum_{al, be} W^al[c, h] W^be[e, h] <T^al_n[h, :], T^be_m[h, :]> + [c == e] (<phi_n, phi_m> + s_n s_m)
// (a) gp_table_kernel writes the tables T [z = (al, h)][n][ld] of a chunk of samples (the first-layer loop of
//     jac_closed_form_kernel without the class scaling) and launch_ll_build_phi (lastlayer_full.hip) the rows [phi_n | s_n];
// (b) gp_nt_gemm_kernel, a batched NT GEMM on the fp32 matrix cores, forms G [z' = (al, be, h)][n][m] and Phi Phi^T;
// (c) launch_gemm (kernels.hip) contracts the classes: Kt [(c, e)][(n, m)] = W_pair [(c, e), z'] G [z', (n, m)];
// (d) the placement kernels write the caller's layout and add the last layer's term.
// G is stored z' major, (n, m) fastest: stage (b) writes it and stage (c) reads it with neighbouring lanes on neighbouring
// floats (the NT kernel's element stride on the output allows the other order; it is not used here).
//
// General route (every other model, and any model under LGNN_GP_FROM_JACOBIANS): chunks of lgnn_jacobians' rows for both
// index lists and the same NT kernel with K = P.
//
// No float atomics anywhere in this file: few-tile, long-K products split K into partial outputs that a second kernel adds
// in slab order, launch_gemm runs with no_atomics.  Two calls on the same input return the same bits.  The fp32 MFMA is
// bit for bit a k-ordered fmaf chain, so <x, y> and <y, x> agree; with the same index pointer on both sides only the upper
// chunk pairs are computed and the lower triangle is a copy of the upper, so K(a, a) is exactly symmetric on every route.
#include "closedform.h"
#include "gpkernel.h"
#include "lgnn_internal.h"

#include <cmath>

#include "device_utils.h"
#include "mfma_tile.h"  // f32x16

namespace lgnn {

namespace {

bool aligned16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- (a) tables --------------------------------------------------------------------------------------------------------
// T[(z * Mc + m) * ld + i], i <= in0 (i == in0: the bias entry), columns (in0, ld) zeroed; GCN: z = h; GraphSAGE: z = h
// (self table), H + h (neighbour table): the entries Ts / Tn of closedform.h.  Samples with an id outside [0, N): zero rows
// and the sticky flag.
__global__ __launch_bounds__(256) void gp_table_kernel(const int64_t* __restrict__ idx, int64_t Mc, LGNN_CF_PARAMS, int64_t ld,
                                                       float* __restrict__ T, int* __restrict__ bad) {
  const ClosedForm cf = LGNN_CF_VIEW;
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  const int64_t H = cf.H;
  const int64_t t0 = int64_t(blockIdx.y) * blockDim.x + threadIdx.x, tstep = int64_t(gridDim.y) * blockDim.x;
  const bool valid = a >= 0 && a < cf.N;
  if (!valid && t0 == 0) bad[1] = 1;
  const int32_t ps = valid ? cf.rowptr[a] : 0, pe = valid ? cf.rowptr[a + 1] : 0;
  for (int64_t t = t0; t < H * ld; t += tstep) {
    const int64_t hh = t / ld, i = t - hh * ld;
    float tn = 0.f, ts = 0.f;
    if (valid && i <= cf.in0) {
      tn = cf_neigh(cf, ps, pe, hh, i);
      if (cf.sage) ts = cf_self(cf, a, hh, i);
    }
    if (cf.sage) {
      T[(hh * Mc + m) * ld + i] = ts;
      T[((H + hh) * Mc + m) * ld + i] = tn;
    } else {
      T[(hh * Mc + m) * ld + i] = tn;
    }
  }
}

// ---- (b) batched NT GEMM -------------------------------------------------------------------------------------------------
// Out_z[i, j] = sum_k A_z[i, k] B_z[j, k], both operands K-contiguous; fp32 MFMA 32x32x2, 128 x 128 block tile, BK = 32, four
// waves of 2 x 2 tiles -- gemm_kernel (kernels.hip) with the B tile loaded the way that kernel loads its A tile: rows x k,
// odd LDS stride, so the per-k column reads of both operands are conflict free.  Any K (a last k-tile is zero filled, an odd
// K pads the last k-pair with zeros), any row counts.
constexpr int TBM = 128, TBN = 128, TBK = 32;

struct NtArgs {
  const float* A; int64_t lda, a_bs;  // A_z = A + z * a_bs: [Ra, K], row stride lda
  const float* B; int64_t ldb, b_bs;  // B_z = B + z * b_bs: [Rb, K], row stride ldb
  float* Out;                          // Out[z * o_bs + sp * o_ss + i * ldo + j * o_es]
  int64_t ldo, o_es, o_bs, o_ss;
  int64_t Ra, Rb, K;
  int64_t k_chunk;                     // split-K: slab sp covers [sp * k_chunk, (sp + 1) * k_chunk); a multiple of TBK
  int splits;                          // blockIdx.z = z * splits + sp
  int vecA, vecB;
  int upper;                           // skip the tiles strictly below the diagonal (the caller mirrors the upper triangle)
};

__device__ __forceinline__ void nt_load_tile(const float* __restrict__ base, int64_t ld, int64_t rows, int64_t row0,
                                             int64_t k0, int kvalid, int vec, float (*dst)[TBK + 1], int tid) {
  // 128 rows x 32 k; thread -> (row = tid / 8 + 32 it, k4 = (tid % 8) * 4)
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = (tid >> 3) + 32 * it, k4 = (tid & 7) * 4;
    const int64_t grow = row0 + r;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (grow < rows) {
      const float* src = base + grow * ld + k0 + k4;
      if (vec && k4 + 4 <= kvalid) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k4 + q < kvalid) x[q] = src[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[r][k4 + q] = x[q];
  }
}

__global__ __launch_bounds__(256) void gp_nt_gemm_kernel(NtArgs g) {
  __shared__ float As[TBM][TBK + 1];
  __shared__ float Bs[TBN][TBK + 1];
  if (g.upper && blockIdx.x > blockIdx.y) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t row0 = int64_t(blockIdx.x) * TBM, col0 = int64_t(blockIdx.y) * TBN;
  const int64_t z = int64_t(blockIdx.z) / g.splits, sp = int64_t(blockIdx.z) - z * g.splits;
  const float* __restrict__ A = g.A + z * g.a_bs;
  const float* __restrict__ B = g.B + z * g.b_bs;

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  const int64_t k_begin = g.splits > 1 ? sp * g.k_chunk : 0;
  const int64_t k_end = g.splits > 1 ? min(g.K, k_begin + g.k_chunk) : g.K;
  for (int64_t k0 = k_begin; k0 < k_end; k0 += TBK) {
    const int kvalid = int(min(int64_t(TBK), k_end - k0));
    nt_load_tile(A, g.lda, g.Ra, row0, k0, kvalid, g.vecA, As, tid);
    nt_load_tile(B, g.ldb, g.Rb, col0, k0, kvalid, g.vecB, Bs, tid);
    __syncthreads();
    const int ksteps = (kvalid + 1) >> 1;
    for (int kk = 0; kk < ksteps; ++kk) {
      const int k = kk * 2 + lhi;
      float av[2], bv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) av[m] = As[wr * 64 + m * 32 + l31][k];
#pragma unroll
      for (int n = 0; n < 2; ++n) bv[n] = Bs[wc * 64 + n * 32 + l31][k];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
  }
  float* __restrict__ out = g.Out + z * g.o_bs + sp * g.o_ss;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int64_t cj = col0 + wc * 64 + n * 32 + l31;
      if (cj >= g.Rb) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t ri = row0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (ri < g.Ra) out[ri * g.ldo + cj * g.o_es] = acc[m][n][r];
      }
    }
  }
}

// second pass of a split-K product: Out[z][i][j] = sum of the slabs' partials in slab order
__global__ __launch_bounds__(256) void gp_splitk_sum_kernel(const float* __restrict__ part, int splits, int64_t Ra, int64_t Rb,
                                                            int64_t batch, float* __restrict__ Out, int64_t ldo, int64_t o_es,
                                                            int64_t o_bs) {
  const int64_t per = Ra * Rb, total = batch * per;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t z = t / per, q = t - z * per, i = q / Rb, j = q - i * Rb;
    const float* __restrict__ p = part + z * splits * per + q;
    float acc = 0.f;
    for (int sp = 0; sp < splits; ++sp) acc += p[sp * per];
    Out[z * o_bs + i * ldo + j * o_es] = acc;
  }
}

// out[z * o_bs + r] = <A_z[r, :], B_z[r, :]>: one wave per (z, r), lanes over k, the xor butterfly's fixed order
__global__ __launch_bounds__(256) void gp_rowdot_kernel(const float* __restrict__ A, int64_t lda, int64_t a_bs,
                                                        const float* __restrict__ B, int64_t ldb, int64_t b_bs, int64_t K,
                                                        int64_t R, int64_t batch, float* __restrict__ out, int64_t o_bs) {
  const int lane = threadIdx.x & 63;
  const int64_t w = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (w >= R * batch) return;
  const int64_t z = w / R, r = w - z * R;
  const float* __restrict__ a = A + z * a_bs + r * lda;
  const float* __restrict__ b = B + z * b_bs + r * ldb;
  float acc = 0.f;
  for (int64_t k = lane; k < K; k += 64) acc = fmaf(a[k], b[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) out[z * o_bs + r] = acc;
}

// ---- (c) class pairs -----------------------------------------------------------------------------------------------------
// Wp[q * ldw + (ab * H + h)] = W^al[c, h] W^be[e, h];  q = c * C + e, or q = c = e with diag_only; GCN: one (al, be);
// GraphSAGE: ab = 2 al + be over the halves [Ws | Wn] of W_1
__global__ void gp_wpair_kernel(const float* __restrict__ W1, int64_t w1_ld, int64_t H, int64_t C, int sage, int diag_only,
                                float* __restrict__ Wp, int64_t ldw) {
  const int64_t nab = sage ? 4 : 1, Zp = nab * H, Q = diag_only ? C : C * C;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= Q * Zp) return;
  const int64_t q = t / Zp, zp = t - q * Zp, ab = zp / H, hh = zp - ab * H;
  const int64_t c = diag_only ? q : q / C, e = diag_only ? q : q - c * C;
  Wp[q * ldw + zp] = W1[c * w1_ld + (ab >> 1) * H + hh] * W1[e * w1_ld + (ab & 1) * H + hh];
}

// ---- (d) placement -------------------------------------------------------------------------------------------------------
// full layout: K[(n C + c) ldk + (m C + e)] = Kt[(c C + e) pairs + n mb + m] + [c == e] S[c s_cs + n mb + m] + Add[(n C + c)
// mb C + m C + e]; one workgroup per (64 columns m, class c, sample n): Kt is read along m and written along (m, e) through an
// LDS transpose of 32 classes e.  S (s_cs = 0: one plane for every class) and Add are the joint GLM predictive's.
__global__ __launch_bounds__(256) void gp_place_full_kernel(const float* __restrict__ Kt /* null: 0 */, int64_t pairs,
                                                            const float* __restrict__ S /* null: 0 */, int64_t s_cs,
                                                            const float* __restrict__ Add /* null: 0 */, int64_t mb, int64_t C,
                                                            float* __restrict__ K, int64_t ldk) {
  __shared__ float tile[32][65];
  const int64_t n = blockIdx.z, c = blockIdx.y, m0 = int64_t(blockIdx.x) * 64;
  const int t = threadIdx.x;
  for (int64_t e0 = 0; e0 < C; e0 += 32) {
    for (int ee = t >> 6; ee < 32; ee += 4) {
      const int mm = t & 63;
      const int64_t e = e0 + ee, m = m0 + mm;
      float v = 0.f;
      if (e < C && m < mb) {
        if (Kt) v = Kt[(c * C + e) * pairs + n * mb + m];
        if (S && e == c) v += S[c * s_cs + n * mb + m];
      }
      tile[ee][mm] = v;
    }
    __syncthreads();
    for (int mm = t >> 5; mm < 64; mm += 8) {
      const int ee = t & 31;
      const int64_t e = e0 + ee, m = m0 + mm;
      if (e < C && m < mb)
        K[(n * C + c) * ldk + m * C + e] = Add ? tile[ee][mm] + Add[(n * C + c) * mb * C + m * C + e] : tile[ee][mm];
    }
    __syncthreads();
  }
}

// independent outputs: K[c plane + n ldk + m] = Kt[c pairs + n mb + m] + S[n mb + m]
__global__ __launch_bounds__(256) void gp_place_planes_kernel(const float* __restrict__ Kt /* null: 0 */, int64_t pairs,
                                                              const float* __restrict__ S, int64_t mb, float* __restrict__ K,
                                                              int64_t ldk, int64_t plane) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, n = blockIdx.y, c = blockIdx.z;
  if (m >= mb) return;
  float v = S[n * mb + m];
  if (Kt) v += Kt[c * pairs + n * mb + m];
  K[c * plane + n * ldk + m] = v;
}

// matched samples: K[n Q + q] = Kt[q M + n] + [q is a diagonal pair] S[n]   (Q = C C, or C with independent outputs)
__global__ void gp_place_matched_kernel(const float* __restrict__ Kt /* null: 0 */, const float* __restrict__ S, int64_t M,
                                        int64_t Q, int64_t C, int diag_only, float* __restrict__ K) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * Q) return;
  const int64_t n = t / Q, q = t - n * Q;
  float v = Kt ? Kt[q * M + n] : 0.f;
  if (diag_only || q / C == q % C) v += S[n];
  K[t] = v;
}

// lower triangle <- upper triangle of `planes` D x D matrices with row stride ld (symmetrize_upper_kernel with a stride)
__global__ __launch_bounds__(256) void gp_mirror_kernel(float* __restrict__ K, int64_t D, int64_t ld, int64_t plane) {
  __shared__ float t[32][33];
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  float* __restrict__ Kp = K + int64_t(blockIdx.z) * plane;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int64_t i = bi * 32 + r, j = bj * 32 + tx;
    t[r][tx] = (i < D && j < D) ? Kp[i * ld + j] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t i = bj * 32 + r, j = bi * 32 + tx;
    if (i < D && j < D && i > j) Kp[i * ld + j] = t[tx][r];
  }
}

// ---- products with a parameter vector -------------------------------------------------------------------------------------
// out[m, c] = sum_z W_1[c, z] <T_m[z, :], theta_0[h(z), :]> + <phi_m, v_Wlast[c, :]> + s_m v_blast[c] for the samples of a
// chunk; theta_0[h, :] = [v_W0[h, :] | v_b0[h]].  One workgroup per sample, a wave per table row, Z floats of dynamic LDS.
__global__ __launch_bounds__(256) void gp_jvp_kernel(const float* __restrict__ T, int64_t Mc, int64_t ld, int64_t in0,
                                                     int64_t H, int64_t Z, const float* __restrict__ W1, int64_t w1_ld,
                                                     const float* __restrict__ Phi, int64_t ldp, int64_t in_last, int64_t C,
                                                     int64_t off_last, const float* __restrict__ v, float* __restrict__ out) {
  extern __shared__ float dz[];
  const int64_t m = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int64_t z = wave; z < Z; z += nw) {
    const int64_t hh = z % H;
    const float* __restrict__ row = T + (z * Mc + m) * ld;
    float acc = 0.f;
    for (int64_t i = lane; i <= in0; i += 64) acc = fmaf(row[i], i < in0 ? v[hh * in0 + i] : v[H * in0 + hh], acc);
    acc = wave_sum(acc);
    if (lane == 0) dz[z] = acc;
  }
  __syncthreads();
  const float* __restrict__ phi = Phi + m * ldp;
  for (int64_t c = threadIdx.x; c < C; c += blockDim.x) {
    float acc = 0.f;
    for (int64_t z = 0; z < Z; ++z) acc = fmaf(W1[c * w1_ld + z], dz[z], acc);
    const float* __restrict__ vw = v + off_last + c * in_last;
    for (int64_t j = 0; j < in_last; ++j) acc = fmaf(phi[j], vw[j], acc);
    out[m * C + c] = fmaf(phi[in_last], v[off_last + C * in_last + c], acc);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
}  // namespace

// Split-K when the output has fewer tiles than the chip has CUs and K is long (the general route: K = P): partial outputs
// [z][slab][Ra][Rb] in ws.gp_part, added in slab order by gp_splitk_sum_kernel.  (NtProblem: lgnn_internal.h; ggnmat.hip
// calls this too.)
int launch_nt_gemm(lgnn_ctx* h, const NtProblem& p, hipStream_t s) {
  if (p.Ra <= 0 || p.Rb <= 0 || p.batch <= 0) return 0;
  LGNN_REQUIRE(p.K > 0, "NT product with empty K");
  NtArgs g{};
  g.A = p.A; g.lda = p.lda; g.a_bs = p.a_bs; g.B = p.B; g.ldb = p.ldb; g.b_bs = p.b_bs;
  g.Ra = p.Ra; g.Rb = p.Rb; g.K = p.K;
  g.upper = (p.upper_only && p.Ra == p.Rb) ? 1 : 0;
  g.vecA = (p.lda % 4 == 0) && (p.a_bs % 4 == 0) && aligned16p(p.A);
  g.vecB = (p.ldb % 4 == 0) && (p.b_bs % 4 == 0) && aligned16p(p.B);
  const int64_t tiles = cdiv(p.Ra, TBM) * cdiv(p.Rb, TBN) * p.batch;
  int64_t splits = 1, k_chunk = 0;
  if (g.upper) {
    // upper tiles only: a long K on few tiles is bound by one tile's time (M C = 2 560, K = 33 792: 210 tiles);
    // slabs of K fill the chip
    const int64_t nt = cdiv(p.Ra, TBM), work = nt * (nt + 1) / 2 * p.batch;
    if (work < 512 && p.K >= 512) {
      const int64_t want = std::min<int64_t>(cdiv(1024, work), cdiv(p.K, 128));
      k_chunk = cdiv(cdiv(p.K, want), TBK) * TBK;
      splits = cdiv(p.K, k_chunk);
    }
  } else if (tiles < 256 && p.K >= 512) {
    const int64_t want = std::min<int64_t>(cdiv(512, tiles), cdiv(p.K, 128));
    k_chunk = cdiv(cdiv(p.K, want), TBK) * TBK;
    splits = cdiv(p.K, k_chunk);
  }
  LGNN_REQUIRE(cdiv(p.Rb, TBN) < 65536 && p.batch * splits < 65536 && cdiv(p.Ra, TBM) < (int64_t(1) << 31),
               "NT product: grid too large");
  const dim3 grid{unsigned(cdiv(p.Ra, TBM)), unsigned(cdiv(p.Rb, TBN)), unsigned(p.batch * splits)};
  if (splits <= 1) {
    g.splits = 1; g.k_chunk = 0;
    g.Out = p.Out; g.ldo = p.ldo; g.o_es = p.o_es; g.o_bs = p.o_bs; g.o_ss = 0;
    hipLaunchKernelGGL(gp_nt_gemm_kernel, grid, dim3(256), 0, s, g);
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  }
  const int64_t per = p.Ra * p.Rb;
  LGNN_CALL(h->ws.gp_part.reserve(size_t(p.batch) * splits * per * 4));
  g.splits = int(splits); g.k_chunk = k_chunk;
  g.Out = h->ws.gp_part.as<float>(); g.ldo = p.Rb; g.o_es = 1; g.o_bs = splits * per; g.o_ss = per;
  hipLaunchKernelGGL(gp_nt_gemm_kernel, grid, dim3(256), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gp_splitk_sum_kernel, dim3(unsigned(std::min<int64_t>(cdiv(p.batch * per, 256), 8192))), dim3(256), 0, s,
                     h->ws.gp_part.as<float>(), int(splits), p.Ra, p.Rb, p.batch, p.Out, p.ldo, p.o_es, p.o_bs);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_wpair(const float* W1, int64_t w1_ld, int64_t H, int64_t C, bool sage, bool diag_only, float* Wp, int64_t ldw,
                 hipStream_t s) {
  const int64_t total = (diag_only ? C : C * C) * (sage ? 4 : 1) * H;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(gp_wpair_kernel, dim3(unsigned(cdiv(total, 256))), dim3(256), 0, s, W1, w1_ld, H, C, sage ? 1 : 0,
                     diag_only ? 1 : 0, Wp, ldw);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_place_full(const float* Kt, int64_t pairs, const float* S, int64_t s_cs, const float* Add, int64_t ma, int64_t mb,
                      int64_t C, float* K, int64_t ldk, hipStream_t s) {
  LGNN_REQUIRE(C < 65536 && ma < 65536, "too many classes");
  hipLaunchKernelGGL(gp_place_full_kernel, dim3(unsigned(cdiv(mb, 64)), unsigned(C), unsigned(ma)), dim3(256), 0, s, Kt, pairs,
                     S, s_cs, Add, mb, C, K, ldk);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

namespace {

int launch_rowdot(const float* A, int64_t lda, int64_t a_bs, const float* B, int64_t ldb, int64_t b_bs, int64_t K, int64_t R,
                  int64_t batch, float* out, int64_t o_bs, hipStream_t s) {
  if (R <= 0 || batch <= 0) return 0;
  LGNN_REQUIRE(cdiv(R * batch, 4) < (int64_t(1) << 31), "row products: too many rows");
  hipLaunchKernelGGL(gp_rowdot_kernel, dim3(unsigned(cdiv(R * batch, 4))), dim3(256), 0, s, A, lda, a_bs, B, ldb, b_bs, K, R,
                     batch, out, o_bs);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_mirror(float* K, int64_t D, int64_t ld, int64_t planes, int64_t plane, hipStream_t s) {
  if (D <= 1) return 0;
  const int64_t nt = cdiv(D, 32);
  LGNN_REQUIRE(nt < 65536 && planes < 65536, "kernel matrix too large to mirror in one launch");
  hipLaunchKernelGGL(gp_mirror_kernel, dim3(unsigned(nt), unsigned(nt), unsigned(planes)), dim3(256), 0, s, K, D, ld, plane);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// the structured route's view of the bound model (GpModel: gpkernel.h)
int gp_model(lgnn_ctx* h, GpModel& g) {
  LGNN_CALL(closed_form_view(h, g.cf));
  const ClosedForm& cf = g.cf;
  g.Z = cf.L == 2 ? (cf.sage ? 2 : 1) * cf.H : 0;
  g.Zp = cf.L == 2 ? (cf.sage ? 4 : 1) * cf.H : 0;
  g.ld = cdiv(cf.in0 + 1, 4) * 4;
  g.ldp = cdiv(cf.in_last + 1, 4) * 4;
  return 0;
}

// tables and [phi | s] rows of the samples idx[0..mc)
int build_tables(lgnn_ctx* h, const GpModel& g, const int64_t* idx, int64_t mc, float* T, float* Phi, hipStream_t s) {
  LGNN_REQUIRE(mc < (int64_t(1) << 31), "too many samples");
  LGNN_CALL(launch_ll_build_phi(idx, mc, g.cf.PhiL, g.ldp, Phi, s));
  // (one-layer model: no table, one wave per sample checks the ids -- nothing else looks at them)
  const unsigned per = g.Z == 0 ? 1u : unsigned(std::max<int64_t>(1, std::min<int64_t>(cdiv(g.cf.H * g.ld, 256), cdiv(2048, mc))));
  hipLaunchKernelGGL(gp_table_kernel, dim3(unsigned(mc), per), dim3(g.Z == 0 ? 64 : 256), 0, s, idx, mc, LGNN_CF_ARGS(g.cf), g.ld, T,
                     h->ws.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

namespace {

int gp_kernel_structured(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags, float* K,
                         int64_t ldk, hipStream_t s) {
  LGNN_CALL(forward_ensure_aux(h, s));
  GpModel g;
  LGNN_CALL(gp_model(h, g));
  const ClosedForm& cf = g.cf;
  const bool indep = (flags & LGNN_GP_INDEPENDENT) != 0, matched = (flags & LGNN_GP_MATCHED) != 0;
  const bool same = idx_a == idx_b && Ma == Mb;
  const int64_t C = cf.C, Q = indep ? C : C * C;
  Workspace& w = h->ws;
  StageTimer tm{h, s};
  if (g.Zp > 0) {
    LGNN_CALL(w.gp_wpair.reserve(size_t(Q) * g.Zp * 4));
    LGNN_CALL(launch_wpair(cf.W1, cf.w1_ld, cf.H, C, cf.sage != 0, indep, w.gp_wpair.as<float>(), g.Zp, s));
  }
  GemmEpilogue ep;
  ep.no_atomics = true;
  const int64_t tab_row = std::max<int64_t>(g.Z, 1) * g.ld + g.ldp;  // floats of tables and phi per sample

  if (matched) {
    // K[n][c][e] = <J_a[n, c, :], J_b[n, e, :]>: row-wise products of the two samples' tables in place of stage (b)
    const int64_t per_sample = (2 * tab_row + g.Zp + Q + 1) * 4;
    const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(Ma, 1 << 20), h->ws_limit / per_sample));
    LGNN_CALL(w.gp_tab_a.reserve(size_t(mc_max) * std::max<int64_t>(g.Z, 1) * g.ld * 4));
    LGNN_CALL(w.gp_phi_a.reserve(size_t(mc_max) * g.ldp * 4));
    if (!same) {
      LGNN_CALL(w.gp_tab_b.reserve(size_t(mc_max) * std::max<int64_t>(g.Z, 1) * g.ld * 4));
      LGNN_CALL(w.gp_phi_b.reserve(size_t(mc_max) * g.ldp * 4));
    }
    LGNN_CALL(w.gp_g.reserve(size_t(mc_max) * std::max<int64_t>(g.Zp, 1) * 4));
    LGNN_CALL(w.gp_kt.reserve(size_t(mc_max) * Q * 4));
    LGNN_CALL(w.gp_s.reserve(size_t(mc_max) * 4));
    for (int64_t m0 = 0; m0 < Ma; m0 += mc_max) {
      const int64_t mc = std::min(mc_max, Ma - m0);
      float* Ta = w.gp_tab_a.as<float>();
      float* Pa = w.gp_phi_a.as<float>();
      float* Tb = same ? Ta : w.gp_tab_b.as<float>();
      float* Pb = same ? Pa : w.gp_phi_b.as<float>();
      LGNN_CALL(tm.mark());
      LGNN_CALL(build_tables(h, g, idx_a + m0, mc, Ta, Pa, s));
      if (!same) LGNN_CALL(build_tables(h, g, idx_b + m0, mc, Tb, Pb, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());
      const int64_t slab = cf.H * mc * g.ld;  // one (al) group of tables
      for (int64_t ab = 0; g.Zp > 0 && ab < (cf.sage ? 4 : 1); ++ab)
        LGNN_CALL(launch_rowdot(Ta + (ab >> 1) * slab, g.ld, mc * g.ld, Tb + (ab & 1) * slab, g.ld, mc * g.ld, cf.in0 + 1, mc, cf.H,
                                w.gp_g.as<float>() + ab * cf.H * mc, mc, s));
      LGNN_CALL(launch_rowdot(Pa, g.ldp, 0, Pb, g.ldp, 0, cf.in_last + 1, mc, 1, w.gp_s.as<float>(), 0, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());
      if (g.Zp > 0)
        LGNN_CALL(launch_gemm(w.gp_wpair.as<float>(), g.Zp, w.gp_g.as<float>(), mc, w.gp_kt.as<float>(), mc, Q, g.Zp, mc, ep, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());
      hipLaunchKernelGGL(gp_place_matched_kernel, dim3(unsigned(cdiv(mc * Q, 256))), dim3(256), 0, s,
                         g.Zp > 0 ? w.gp_kt.as<float>() : nullptr, w.gp_s.as<float>(), mc, Q, C, indep ? 1 : 0, K + m0 * Q);
      LGNN_HIP_CHECK(hipGetLastError());
      LGNN_CALL(tm.mark());
    }
    return 0;
  }

  // chunk pairs: G [Zp][mc x mc] and Kt [Q][mc x mc] under half the workspace limit; launch_gemm's grid bounds the pairs
  const int64_t per_pair = (g.Zp + Q + 1) * 4;
  int64_t mc_max = int64_t(std::sqrt(double(std::max<int64_t>(h->ws_limit / 2, per_pair)) / double(per_pair)));
  mc_max = std::max<int64_t>(1, std::min<int64_t>(mc_max, 2048));
  while (mc_max > 1 && 2 * mc_max * tab_row * 4 > h->ws_limit / 2) mc_max /= 2;
  const int64_t ca = std::min(mc_max, Ma), cb = std::min(mc_max, Mb);
  LGNN_CALL(w.gp_tab_a.reserve(size_t(ca) * std::max<int64_t>(g.Z, 1) * g.ld * 4));
  LGNN_CALL(w.gp_phi_a.reserve(size_t(ca) * g.ldp * 4));
  LGNN_CALL(w.gp_tab_b.reserve(size_t(cb) * std::max<int64_t>(g.Z, 1) * g.ld * 4));
  LGNN_CALL(w.gp_phi_b.reserve(size_t(cb) * g.ldp * 4));
  LGNN_CALL(w.gp_g.reserve(size_t(ca) * cb * std::max<int64_t>(g.Zp, 1) * 4));
  LGNN_CALL(w.gp_kt.reserve(size_t(ca) * cb * Q * 4));
  LGNN_CALL(w.gp_s.reserve(size_t(ca) * cb * 4));
  const int64_t plane = Ma * ldk;
  for (int64_t n0 = 0; n0 < Ma; n0 += ca) {
    const int64_t ma = std::min(ca, Ma - n0);
    bool a_built = false;
    for (int64_t m0 = same ? n0 : 0; m0 < Mb; m0 += cb) {  // same index list: upper chunk pairs only, mirrored below
      const int64_t mb = std::min(cb, Mb - m0);
      const bool diag = same && m0 == n0;
      float* Ta = w.gp_tab_a.as<float>();
      float* Pa = w.gp_phi_a.as<float>();
      float* Tb = diag ? Ta : w.gp_tab_b.as<float>();
      float* Pb = diag ? Pa : w.gp_phi_b.as<float>();
      LGNN_CALL(tm.mark());
      if (!a_built) { LGNN_CALL(build_tables(h, g, idx_a + n0, ma, Ta, Pa, s)); a_built = true; }
      if (!diag) LGNN_CALL(build_tables(h, g, idx_b + m0, mb, Tb, Pb, s));
      LGNN_CALL(tm.mark());
      const int64_t pairs = ma * mb;
      LGNN_CALL(tm.mark());
      for (int64_t ab = 0; g.Zp > 0 && ab < (cf.sage ? 4 : 1); ++ab) {
        NtProblem p{};
        p.A = Ta + (ab >> 1) * cf.H * ma * g.ld; p.lda = g.ld; p.a_bs = ma * g.ld;
        p.B = Tb + (ab & 1) * cf.H * mb * g.ld; p.ldb = g.ld; p.b_bs = mb * g.ld;
        p.Out = w.gp_g.as<float>() + ab * cf.H * pairs; p.ldo = mb; p.o_es = 1; p.o_bs = pairs;
        p.Ra = ma; p.Rb = mb; p.K = cf.in0 + 1; p.batch = cf.H;
        LGNN_CALL(launch_nt_gemm(h, p, s));
      }
      {
        NtProblem p{};
        p.A = Pa; p.lda = g.ldp; p.B = Pb; p.ldb = g.ldp;
        p.Out = w.gp_s.as<float>(); p.ldo = mb; p.o_es = 1;
        p.Ra = ma; p.Rb = mb; p.K = cf.in_last + 1; p.batch = 1;
        LGNN_CALL(launch_nt_gemm(h, p, s));
      }
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());
      if (g.Zp > 0)
        LGNN_CALL(launch_gemm(w.gp_wpair.as<float>(), g.Zp, w.gp_g.as<float>(), pairs, w.gp_kt.as<float>(), pairs, Q, g.Zp, pairs,
                              ep, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());
      const float* Kt = g.Zp > 0 ? w.gp_kt.as<float>() : nullptr;
      if (indep) {
        LGNN_REQUIRE(C < 65536, "too many classes");
        hipLaunchKernelGGL(gp_place_planes_kernel, dim3(unsigned(cdiv(mb, 256)), unsigned(ma), unsigned(C)), dim3(256), 0, s, Kt,
                           pairs, w.gp_s.as<float>(), mb, K + n0 * ldk + m0, ldk, plane);
      } else {
        LGNN_CALL(launch_place_full(Kt, pairs, w.gp_s.as<float>(), 0, nullptr, ma, mb, C, K + n0 * C * ldk + m0 * C, ldk, s));
      }
      LGNN_HIP_CHECK(hipGetLastError());
      LGNN_CALL(tm.mark());
    }
  }
  if (same) LGNN_CALL(indep ? launch_mirror(K, Ma, ldk, C, plane, s) : launch_mirror(K, Ma * C, ldk, 1, 0, s));
  return 0;
}

int gp_kernel_general(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags, float* K,
                      int64_t ldk, hipStream_t s) {
  const bool indep = (flags & LGNN_GP_INDEPENDENT) != 0, matched = (flags & LGNN_GP_MATCHED) != 0;
  const bool same = idx_a == idx_b && Ma == Mb;
  const int64_t C = h->dims[h->L], P = h->n_params;
  Workspace& w = h->ws;
  // two chunks of Jacobian rows under half the workspace limit (the other half is lgnn_jacobians' own)
  const int64_t per_sample = C * P * 4;
  int64_t mc_max = std::max<int64_t>(1, h->ws_limit / 2 / (2 * per_sample));
  mc_max = std::min<int64_t>(mc_max, std::max<int64_t>(1, (int64_t(65535) * TBN) / C));  // grid.y of the NT kernel
  mc_max = std::min<int64_t>(mc_max, 65535);                                             // batch = samples (matched)
  const int64_t ca = std::min(mc_max, Ma), cb = std::min(mc_max, Mb);
  LGNN_CALL(w.gp_jac_a.reserve(size_t(ca) * per_sample));
  if (!same || cb < Mb || matched) LGNN_CALL(w.gp_jac_b.reserve(size_t(cb) * per_sample));
  float* Ja = w.gp_jac_a.as<float>();
  if (matched) {
    const int64_t Q = indep ? C : C * C;
    for (int64_t m0 = 0; m0 < Ma; m0 += ca) {
      const int64_t mc = std::min(ca, Ma - m0);
      LGNN_CALL(jacobians(h, idx_a + m0, mc, Ja, nullptr, s));
      float* Jb = Ja;
      if (!same) { Jb = w.gp_jac_b.as<float>(); LGNN_CALL(jacobians(h, idx_b + m0, mc, Jb, nullptr, s)); }
      if (indep) {
        LGNN_CALL(launch_rowdot(Ja, P, 0, Jb, P, 0, P, mc * C, 1, K + m0 * Q, 0, s));
      } else {
        NtProblem p{};
        p.A = Ja; p.lda = P; p.a_bs = C * P; p.B = Jb; p.ldb = P; p.b_bs = C * P;
        p.Out = K + m0 * Q; p.ldo = C; p.o_es = 1; p.o_bs = Q;
        p.Ra = C; p.Rb = C; p.K = P; p.batch = mc;
        LGNN_CALL(launch_nt_gemm(h, p, s));
      }
    }
    return 0;
  }
  const int64_t plane = Ma * ldk;
  for (int64_t n0 = 0; n0 < Ma; n0 += ca) {
    const int64_t ma = std::min(ca, Ma - n0);
    LGNN_CALL(jacobians(h, idx_a + n0, ma, Ja, nullptr, s));
    for (int64_t m0 = same ? n0 : 0; m0 < Mb; m0 += cb) {
      const int64_t mb = std::min(cb, Mb - m0);
      float* Jb = Ja;
      if (!(same && m0 == n0)) { Jb = w.gp_jac_b.as<float>(); LGNN_CALL(jacobians(h, idx_b + m0, mb, Jb, nullptr, s)); }
      NtProblem p{};
      p.K = P; p.o_es = 1; p.ldo = ldk;
      if (indep) {  // batch C: row c of every sample, row stride C P
        p.A = Ja; p.lda = C * P; p.a_bs = P; p.B = Jb; p.ldb = C * P; p.b_bs = P;
        p.Out = K + n0 * ldk + m0; p.o_bs = plane; p.Ra = ma; p.Rb = mb; p.batch = C;
      } else {
        p.A = Ja; p.lda = P; p.B = Jb; p.ldb = P;
        p.Out = K + n0 * C * ldk + m0 * C; p.Ra = ma * C; p.Rb = mb * C; p.batch = 1;
      }
      LGNN_CALL(launch_nt_gemm(h, p, s));
    }
  }
  if (same) LGNN_CALL(indep ? launch_mirror(K, Ma, ldk, C, plane, s) : launch_mirror(K, Ma * C, ldk, 1, 0, s));
  return 0;
}

}  // namespace

int gp_kernel(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags, float* K, int64_t ldk,
              hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_REQUIRE((flags & ~(LGNN_GP_INDEPENDENT | LGNN_GP_MATCHED | LGNN_GP_FROM_JACOBIANS)) == 0, "unknown flag");
  const int64_t C = h->dims[h->L];
  if (flags & LGNN_GP_MATCHED) LGNN_REQUIRE(Ma == Mb, "LGNN_GP_MATCHED needs as many samples on both sides");
  else LGNN_REQUIRE(ldk >= ((flags & LGNN_GP_INDEPENDENT) ? Mb : Mb * C), "row stride of K too small");
  if (closed_form_model(h) && !(flags & LGNN_GP_FROM_JACOBIANS)) return gp_kernel_structured(h, idx_a, Ma, idx_b, Mb, flags, K, ldk, s);
  return gp_kernel_general(h, idx_a, Ma, idx_b, Mb, flags, K, ldk, s);
}

int gp_jvp(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* v, float* out, hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  Workspace& w = h->ws;
  const int64_t C = h->dims[h->L], P = h->n_params;
  if (!closed_form_model(h)) {  // a chunked matvec over lgnn_jacobians' rows
    const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / 2 / (C * P * 4)));
    LGNN_CALL(w.gp_jac_a.reserve(size_t(mc_max) * C * P * 4));
    for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
      const int64_t mc = std::min(mc_max, M - m0);
      LGNN_CALL(jacobians(h, idx + m0, mc, w.gp_jac_a.as<float>(), nullptr, s));
      LGNN_CALL(launch_rowdot(w.gp_jac_a.as<float>(), P, 0, v, 0, 0, P, mc * C, 1, out + m0 * C, 0, s));
    }
    return 0;
  }
  LGNN_CALL(forward_ensure_aux(h, s));
  GpModel g;
  LGNN_CALL(gp_model(h, g));
  const ClosedForm& cf = g.cf;
  LGNN_REQUIRE(g.Z * 4 <= 48 * 1024, "hidden width exceeds the staging area");
  const int64_t tab_row = std::max<int64_t>(g.Z, 1) * g.ld + g.ldp;
  const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, 1 << 20), h->ws_limit / (tab_row * 4)));
  LGNN_CALL(w.gp_tab_a.reserve(size_t(mc_max) * std::max<int64_t>(g.Z, 1) * g.ld * 4));
  LGNN_CALL(w.gp_phi_a.reserve(size_t(mc_max) * g.ldp * 4));
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(build_tables(h, g, idx + m0, mc, w.gp_tab_a.as<float>(), w.gp_phi_a.as<float>(), s));
    hipLaunchKernelGGL(gp_jvp_kernel, dim3(unsigned(mc)), dim3(256), size_t(std::max<int64_t>(g.Z, 1)) * 4, s,
                       w.gp_tab_a.as<float>(), mc, g.ld, cf.in0, std::max<int64_t>(cf.H, 1), g.Z, cf.W1, cf.w1_ld,
                       w.gp_phi_a.as<float>(), g.ldp, cf.in_last, C, cf.off_last, v, out + m0 * C);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace lgnn

extern "C" int lgnn_gp_kernel(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags,
                              float* K, int64_t ldk, void* stream) {
  if (!h || ((Ma > 0 && Mb > 0) && (!idx_a || !idx_b || !K))) { lgnn::set_error("null argument"); return 2; }
  if (Ma <= 0 || Mb <= 0) return 0;
  return lgnn::gp_kernel(h, idx_a, Ma, idx_b, Mb, flags, K, ldk, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_gp_jvp(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* v, float* out, void* stream) {
  if (!h || (M > 0 && (!idx || !v || !out))) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0) return 0;
  return lgnn::gp_jvp(h, idx, M, v, out, static_cast<hipStream_t>(stream));
}
