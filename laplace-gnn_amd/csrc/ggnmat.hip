// GGN-times-block products: out = J V^T and G += sum_n J_n^T Lambda_n J_n V^T for a block V [k, P] of parameter directions
// (a direction is a contiguous row of P floats, the layout of theta in lgnn_sampled_forward).
//
// Reference: LowRankLaplace (laplace/baselaplace.py:1679-1835) takes its eigenpairs from AsdfghjklHessian.eig_lowrank
// (laplace/curvature/asdfghjkl.py:212-236): power iteration on Hessian-vector products, one vector at a time.  Here the
// curvature is the GGN of lgnn_full_accumulate and the product takes a whole block, never forming the P x P matrix.
//
// Structured route (1- and 2-layer GCN / GraphSAGE, relu or tanh, no res / norm): no Jacobian and no [rows, H k] intermediate
// reaches memory.  Notation of sampled.hip: in0 = [P X | rowsum P] (GCN) or [X | P X | 1] (GraphSAGE), R the needed rows of the
// batch, D = act'(s), W1 = [W1a | W1b] for GraphSAGE (z has Cz = 2 C columns, C for GCN).  Per direction i = (dW0, db0, dW1, db1):
//   forward    q_i[r] = (D[r] . (in0[r] [dW0 | db0]^T)) W1^T + h[r] dW1^T             r in R      first_layer_kernel<FwdArgs>
//              u_i[m] = sum_b P[n_m, b] (q_i[b] + db1)  (GraphSAGE: self half + gathered half + db1)   sampled.hip's gather
//   curvature  w_i[m] = Lambda_m u_i[m]                                                            ggn_lambda_rows_kernel
//   transpose  qbar_i[r] = sum_m P[n_m, r] w_i[m]  (GraphSAGE: and the self half)                     ggn_qbar_kernel
//              g_b1 = sum_m rho_m w_i[m]                                                            ggn_bias_kernel
//              g_W1 = sum_r qbar_i[r]^T h[r]                                                        ggn_tn_kernel, direct
//              sbar_i[r] = D[r] . (qbar_i[r] W1);  [g_W0 | g_b0] = sum_r sbar_i[r]^T in0[r]         ggn_tn_kernel, through W1
// A sample's w depends on its node alone, so the samples of a repeated node enter qbar as (multiplicity) x (the first one's w):
// qbar is a gather over P^T's rows with one writer per element.  One layer is the two outer products alone.
// The forward product is step (b) of sampled.hip linearised, and is that kernel's text (its FwdArgs instance): the k directions
// in the grid, D and the contraction with W1 applied while the 64 x 64 tile is in LDS, the h dW1^T term on the same
// accumulators.  ggn_tn_kernel owns a 64 x 64 output tile per workgroup and walks its share of R's row tiles: it builds sbar
// from qbar and W1 in its prologue (MFMA), multiplies sbar^T in0 on the same MFMA, and writes one partial tile per slab of R;
// ggn_finish_kernel adds the slabs in order into G.  Only q, u, w, qbar (|R| Cz k or M C k floats each), the slab partials
// and the [k, P] output reach memory.  The directions go in chunks so that these stay under the workspace limit.
//
// General route (every other bound model, and any model under LGNN_GGN_FROM_JACOBIANS): chunks of lgnn_jacobians' rows
// J_c [mc C, P] under the workspace limit,
//   (a) U = J_c V^T               launch_nt_gemm (gpkernel.hip: fp32 MFMA 32x32x2, split-K partials added in slab order)
//   (b) W^T[i, (m, c)] = (Lambda_m U[m, :, i])[c]   ggn_lambda_kernel: Lambda = diag(p) - p p^T from the batch prologue's
//                                                   softmax; the identity for regression; zero for an invalid id
//   (c) T = W^T J_c               launch_gemm (kernels.hip) with no_atomics
//   (d) G += T                    ggn_add_kernel
// No float atomics in this file: every output element has one writer and a fixed summation order, so two calls on the same
// input return the same bits.  (The loss is the batch prologue's, shared with every accumulate.)  With kernel timing enabled
// each chunk records four event pairs: general (a)-(d); structured forward + gather, curvature, qbar + bias, outer products +
// finish.  lgnn_jvp_block records one pair per chunk.
//
// lgnn_block_gram: A B^T of two blocks of directions through the same NT GEMM -- the Gram and Rayleigh-Ritz matrices of the
// eigensolver (lowrank.py), bit-reproducible and exactly symmetric for A == B.
#include "closedform.h"
#include "ggn_struct.h"
#include "lgnn_internal.h"

#include <climits>

#include "device_utils.h"
#include "mfma_tile.h"

namespace lgnn {

namespace {

// one thread per (sample, direction): the C values of the pair are read twice (L1), written along W^T's row i
__global__ __launch_bounds__(256) void ggn_lambda_kernel(const float* __restrict__ U, const float* __restrict__ probs,
                                                         const int64_t* __restrict__ idx, int64_t N, int64_t mc, int64_t C,
                                                         int64_t k, int regression, float* __restrict__ Wt, int64_t ldw) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= mc * k) return;
  const int64_t m = t / k, i = t - m * k;
  const int64_t n = idx[m];
  const float* __restrict__ u = U + m * C * k + i;
  float* __restrict__ w = Wt + i * ldw + m * C;
  if (n < 0 || n >= N) {  // flagged by the batch prologue; its probabilities were never written
    for (int64_t c = 0; c < C; ++c) w[c] = 0.f;
    return;
  }
  if (regression) {
    for (int64_t c = 0; c < C; ++c) w[c] = u[c * k];
    return;
  }
  const float* __restrict__ p = probs + m * C;
  float pu = 0.f;
  for (int64_t c = 0; c < C; ++c) pu = fmaf(p[c], u[c * k], pu);
  for (int64_t c = 0; c < C; ++c) w[c] = p[c] * (u[c * k] - pu);
}

__global__ __launch_bounds__(256) void ggn_add_kernel(const float* __restrict__ T, int64_t n, float* __restrict__ G) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += stride) G[t] += T[t];
}

struct PhaseTimer {  // lgnn_enable_kernel_timing: one event pair per phase
  lgnn_ctx* h; hipStream_t s;
  int mark() { return h->timing ? record_event(h, s) : 0; }
};

// samples per chunk: the Jacobian rows, U and W^T under half the workspace limit (the other half is lgnn_jacobians' own)
int64_t chunk_samples(const lgnn_ctx* h, int64_t M, int64_t k) {
  const int64_t C = h->dims[h->L], P = h->n_params;
  const int64_t per_sample = C * (P + 2 * k) * 4;
  int64_t mc = std::max<int64_t>(1, h->ws_limit / 2 / per_sample);
  mc = std::min<int64_t>(mc, (int64_t(1) << 30) / std::max<int64_t>(C, 1));  // rows of a chunk stay below 2^30
  return std::min(mc, M);
}

int jvp_block_general(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* out, hipStream_t s) {
  const int64_t C = h->dims[h->L], P = h->n_params;
  const int64_t mc_max = chunk_samples(h, M, k);
  Workspace& w = h->ws;
  LGNN_CALL(w.ggn_jac.reserve(size_t(mc_max) * C * P * 4));
  PhaseTimer tm{h, s};
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, w.ggn_jac.as<float>(), nullptr, s));
    LGNN_CALL(tm.mark());
    NtProblem p{};
    p.A = w.ggn_jac.as<float>(); p.lda = P; p.B = V; p.ldb = P;
    p.Out = out + m0 * C * k; p.ldo = k; p.o_es = 1;
    p.Ra = mc * C; p.Rb = k; p.K = P; p.batch = 1;
    LGNN_CALL(launch_nt_gemm(h, p, s));
    LGNN_CALL(tm.mark());
  }
  return 0;
}

int ggn_matmat_general(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* G, hipStream_t s) {
  const int64_t C = h->dims[h->L], P = h->n_params;
  const int64_t mc_max = chunk_samples(h, M, k);
  const int64_t ldw = cdiv(mc_max * C, 4) * 4;
  Workspace& w = h->ws;
  LGNN_CALL(w.ggn_jac.reserve(size_t(mc_max) * C * P * 4));
  LGNN_CALL(w.ggn_u.reserve(size_t(mc_max) * C * k * 4));
  LGNN_CALL(w.ggn_wt.reserve(size_t(k) * ldw * 4));
  LGNN_CALL(w.ggn_tmp.reserve(size_t(k) * P * 4));
  float* J = w.ggn_jac.as<float>();
  float* U = w.ggn_u.as<float>();
  float* Wt = w.ggn_wt.as<float>();
  float* T = w.ggn_tmp.as<float>();
  GemmEpilogue ep;
  ep.no_atomics = true;
  PhaseTimer tm{h, s};
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    LGNN_CALL(tm.mark());
    NtProblem p{};
    p.A = J; p.lda = P; p.B = V; p.ldb = P;
    p.Out = U; p.ldo = k; p.o_es = 1;
    p.Ra = mc * C; p.Rb = k; p.K = P; p.batch = 1;
    LGNN_CALL(launch_nt_gemm(h, p, s));
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    hipLaunchKernelGGL(ggn_lambda_kernel, dim3(unsigned(cdiv(mc * k, 256))), dim3(256), 0, s, U,
                       h->ws.probs.as<float>() + m0 * C, idx + m0, h->N, mc, C, k, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, Wt,
                       ldw);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    LGNN_CALL(launch_gemm(Wt, ldw, J, P, T, P, k, mc * C, P, ep, s));
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    hipLaunchKernelGGL(ggn_add_kernel, dim3(unsigned(std::min<int64_t>(cdiv(k * P, 256), 8192))), dim3(256), 0, s, T, k * P, G);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(tm.mark());
  }
  return 0;
}


// ======== structured route ================================================================================================
// w[i][m][:] = Lambda_m u[i][m][:] in place layout [kc][M][C]; one thread per (direction, sample)
__global__ __launch_bounds__(256) void ggn_lambda_rows_kernel(const float* __restrict__ U, const float* __restrict__ probs,
                                                              const int64_t* __restrict__ idx, int64_t N, int64_t M, int64_t C,
                                                              int64_t kc, int regression, float* __restrict__ W) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= kc * M) return;
  const int64_t m = t % M;
  const int64_t n = idx[m];
  const float* __restrict__ u = U + t * C;
  float* __restrict__ w = W + t * C;
  if (n < 0 || n >= N) {
    for (int64_t c = 0; c < C; ++c) w[c] = 0.f;
    return;
  }
  if (regression) {
    for (int64_t c = 0; c < C; ++c) w[c] = u[c];
    return;
  }
  const float* __restrict__ p = probs + m * C;
  float pu = 0.f;
  for (int64_t c = 0; c < C; ++c) pu = fmaf(p[c], u[c], pu);
  for (int64_t c = 0; c < C; ++c) w[c] = p[c] * (u[c] - pu);
}

// qbar[i][t][cz] for the needed rows t < |R|: the gather over P^T's row (one writer, the row's stored order); a repeated node's
// samples enter as multiplicity x the first one's w.  GraphSAGE: columns [0, C) are the row's own samples.
__global__ __launch_bounds__(256) void ggn_qbar_kernel(const float* __restrict__ W, int64_t M, int64_t C, int64_t Cz, int sage,
                                                       const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                       const int32_t* __restrict__ trowptr, const int32_t* __restrict__ tcol,
                                                       const float* __restrict__ tval, const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ count, int64_t rcap, int64_t kc,
                                                       float* __restrict__ qbar) {
  const int64_t cnt = int64_t(*count);
  const int64_t per = cnt * Cz, total = kc * per;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t i = e / per, q = e - i * per, t = q / Cz, cz = q - t * Cz;
    const int64_t c = cz % C;
    const int32_t r = rows[t];
    const float* __restrict__ wi = W + i * M * C;
    float acc = 0.f;
    if (sage && cz < C) {
      const int32_t pm = pos[r];
      if (pm != INT32_MAX) acc = float(mult[pm]) * wi[int64_t(pm) * C + c];
    } else {
      for (int32_t p = trowptr[r]; p < trowptr[r + 1]; ++p) {
        const int32_t pm = pos[tcol[p]];
        if (pm != INT32_MAX) acc = fmaf(tval[p] * float(mult[pm]), wi[int64_t(pm) * C + c], acc);
      }
    }
    qbar[(i * rcap + t) * Cz + cz] = acc;
  }
}

// part[i][offb + c] = sum_m rho_m w[i][m][c]: grid (directions, 64-class windows), 16 groups of 64 lanes stride the samples,
// the groups' sums meet in group order
__global__ __launch_bounds__(1024) void ggn_bias_kernel(const float* __restrict__ W, const int64_t* __restrict__ idx, int64_t N,
                                                        int64_t M, int64_t C, const float* __restrict__ in0, int64_t ldk,
                                                        int64_t Fp, int gcn, float* __restrict__ part, int64_t P, int64_t offb) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t i = blockIdx.x, c = int64_t(blockIdx.y) * 64 + lane;
  const float* __restrict__ wi = W + i * M * C;
  float acc = 0.f;
  if (c < C)
    for (int64_t m = grp; m < M; m += 16) {
      const int64_t n = idx[m];
      if (n < 0 || n >= N) continue;
      const float rho = gcn ? in0[n * ldk + Fp] : 1.f;
      acc = fmaf(rho, wi[m * C + c], acc);
    }
  red[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && c < C) {
    float t = 0.f;
    for (int g2 = 0; g2 < 16; ++g2) t += red[g2][lane];
    part[i * P + offb + c] = t;
  }
}

// 16 consecutive floats of a row into registers (zero where the row is absent or the column is past `cols`)
__device__ __forceinline__ void tn_fetch(float (&v)[16], const float* __restrict__ src, int64_t c0, int64_t cols, bool ok) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int64_t c = c0 + e;
    v[e] = (ok && c < cols) ? src[c] : 0.f;
  }
}
__device__ __forceinline__ void tn_store(float* __restrict__ dst, const float (&v)[16], int srow, int sk) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[srow * SLDT + sk + e] = v[e];
}
// Wh[h][cz] = W1z[cz0 + cz][a0 + h], lanes along h
__device__ __forceinline__ void tn_stage_w1(float* __restrict__ Wh, const TnArgs& g, int64_t cz0, int64_t a0, int wave, int lane) {
  for (int cz = wave; cz < SBM; cz += 4) {
    const int64_t c = cz0 + cz, hh = a0 + lane;
    float v = 0.f;
    if (c < g.acols && hh < g.H) v = g.W1[(c % g.C) * g.ld1 + (c / g.C) * g.H + hh];
    Wh[lane * SLDT + cz] = v;
  }
}

// grid: (slabs of R's row tiles, directions of the chunk, output tiles a x b).  A thread owns 16 consecutive columns of one row
// of the 64 x 64 tiles it stages; the next row tile's id and A values and this tile's B values travel in registers under the
// products.  W1's tile is staged once per workgroup when the classes fit one chunk of 64.
__global__ __launch_bounds__(256) void ggn_tn_kernel(TnArgs g) {
  __shared__ float At[SBM * SLDT];
  __shared__ float Bt[SBM * SLDT];
  __shared__ float Wh[SBM * SLDT];
  __shared__ float bcol[SBM];
  __shared__ int rid[SBM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int srow = tid >> 2, sk = (tid & 3) * 16;
  const int64_t cnt = int64_t(*g.count);
  const int64_t i = blockIdx.y;
  const int64_t at = int64_t(blockIdx.z) / g.btiles, bt = int64_t(blockIdx.z) - at * g.btiles;
  const int64_t a0 = at * SBM, b0 = bt * SBM;
  const bool bias = g.bias_off >= 0 && bt == 0;
  const bool through = g.mode == 1;
  const bool w1_once = through && g.acols <= SBM;
  const int64_t ac0 = through ? 0 : a0;  // first column of A this workgroup reads
  const float* __restrict__ Ai = g.A + i * g.a_ds;
  f32x16 acc;
  acc_zero(acc);
  float bias_acc = 0.f;
  if (w1_once) tn_stage_w1(Wh, g, 0, a0, wave, lane);  // (the first tile's barriers come before its first read)
  int64_t tile = blockIdx.x;
  int32_t r_cur = -1;
  float qa[16];
  if (tile * SBM < cnt) {
    r_cur = g.rows[tile * SBM + srow < cnt ? tile * SBM + srow : cnt - 1];
    if (tile * SBM + srow >= cnt) r_cur = -1;
    tn_fetch(qa, Ai + (tile * SBM + srow) * g.a_ld, ac0 + sk, g.acols, r_cur >= 0);
  }
  for (; tile * SBM < cnt; tile += gridDim.x) {
    const int64_t t0 = tile * SBM;
    const bool rok = r_cur >= 0;
    float pb[16];
    const float* __restrict__ bp = g.b_listed ? g.B + i * g.b_ds + (rok ? t0 + srow : 0) * g.b_ld
                                              : g.B + int64_t(rok ? r_cur : 0) * g.b_ld;
    tn_fetch(pb, bp, b0 + sk, g.bcols, rok);
    const float bc = (rok && bias) ? g.in0[int64_t(r_cur) * g.ldk + g.Fp] : 0.f;
    __syncthreads();  // the previous tile's products have read At / Bt / bcol / rid
    if ((tid & 3) == 0) {
      rid[srow] = r_cur;
      bcol[srow] = bc;
    }
    tn_store(through ? Bt : At, qa, srow, sk);
    if (!through) tn_store(Bt, pb, srow, sk);  // (through W1, Bt holds the A values first and takes B's after the prologue)
    if (through && !w1_once) tn_stage_w1(Wh, g, 0, a0, wave, lane);
    // the next tile of this workgroup: its row and its A values
    {
      const int64_t nt = (tile + gridDim.x) * SBM + srow;
      r_cur = nt < cnt ? g.rows[nt] : -1;
      tn_fetch(qa, Ai + nt * g.a_ld, ac0 + sk, g.acols, r_cur >= 0);
    }
    __syncthreads();
    if (through) {
      const int64_t hh = a0 + wc * 32 + l31;
      float dv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int r2 = rid[acc_row(wr * 32, lane, r)];
        dv[r] = (r2 >= 0 && hh < g.H) ? g.dact[int64_t(r2) * g.H + hh] : 0.f;
      }
      f32x16 sacc;
      acc_zero(sacc);
      tile_nt_step<SBM, SLDT>(Bt, wr * 32, Wh, wc * 32, lane, sacc);
      for (int64_t cz0 = SBM; cz0 < g.acols; cz0 += SBM) {  // more than 64 class columns: the further chunks, staged in place
        __syncthreads();
        float qc[16];
        const int r2 = rid[srow];
        tn_fetch(qc, Ai + (t0 + srow) * g.a_ld, cz0 + sk, g.acols, r2 >= 0);
        tn_store(Bt, qc, srow, sk);
        tn_stage_w1(Wh, g, cz0, a0, wave, lane);
        __syncthreads();
        tile_nt_step<SBM, SLDT>(Bt, wr * 32, Wh, wc * 32, lane, sacc);
      }
      __syncthreads();  // every wave has read Bt (and Wh): Bt takes the B tile
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(wr * 32, lane, r);
        At[row * SLDT + wc * 32 + l31] = dv[r] * sacc[r];
      }
      tn_store(Bt, pb, srow, sk);
      __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < SBM; kk += 2) {
      const float a = At[(kk + lh) * SLDT + wr * 32 + l31];
      const float b = Bt[(kk + lh) * SLDT + wc * 32 + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (bias && tid < SBM)
      for (int t = 0; t < SBM; ++t) bias_acc = fmaf(At[t * SLDT + tid], bcol[t], bias_acc);
  }
  float* __restrict__ out = g.part + (int64_t(blockIdx.x) * g.kc + i) * g.P;
  const int64_t bb = b0 + wc * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t aa = acc_row(a0 + wr * 32, lane, r);
    if (aa < g.adim && bb < g.bcols) out[g.ooff + (aa % g.amod) * g.old + (aa / g.amod) * g.ashift + bb] = acc[r];
  }
  if (bias && tid < SBM && a0 + tid < g.adim) out[g.bias_off + a0 + tid] = bias_acc;
}

// G[i][p] += the slabs' partials in slab order
__global__ __launch_bounds__(256) void ggn_finish_kernel(const float* __restrict__ part, int nslab, int64_t per,
                                                         float* __restrict__ G) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < per; t += stride) {
    float acc = 0.f;
    for (int sl = 0; sl < nslab; ++sl) acc += part[sl * per + t];
    G[t] += acc;
  }
}

// out[(m C + c) k + i0 + i] = u[i][m][c]
__global__ __launch_bounds__(256) void ggn_place_kernel(const float* __restrict__ U, int64_t M, int64_t C, int64_t kc, int64_t k,
                                                        int64_t i0, float* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= kc * M * C) return;
  const int64_t i = t / (M * C), mc = t - i * M * C;
  out[mc * k + i0 + i] = U[t];
}

int struct_model(lgnn_ctx* h, int64_t M, StructModel& m) {
  m.two = h->L == 2; m.sage = h->kind == LGNN_KIND_SAGE;
  m.N = h->N; m.Fp = h->in_dim[0]; m.H = h->dims[1]; m.C = h->dims[h->L];
  m.Cz = m.sage ? 2 * m.C : m.C; m.ld1 = m.sage ? 2 * m.H : m.H;
  m.off1 = m.H * m.Fp + m.H; m.offb = m.two ? m.off1 + m.C * m.ld1 : m.C * m.Fp;
  m.P = h->n_params; m.rcap = m.two ? m.N : M;
  LGNN_REQUIRE(m.P == m.offb + m.C, "parameter count of the bound model");
  if (m.two) LGNN_REQUIRE(h->in_dim[1] == m.ld1 && h->fc.hact_p[0] && h->fc.dact0.p, "internal: second layer's operands");
  return 0;
}

// u [kc][M][C] of the directions V_c[0..kc): forward product and gather
int struct_forward(lgnn_ctx* h, const StructModel& m, const int64_t* idx, int64_t M, const float* Vc, int64_t kc, float* q,
                   float* u, hipStream_t s) {
  SampledState& sf = h->sf;
  FwdArgs a{};
  a.in0 = sf.in0.as<float>(); a.ldk = sf.ldk;
  a.rows = sf.rows.as<int32_t>(); a.count = sf.count.as<int32_t>();
  a.theta = Vc; a.P = m.P;
  a.Fp = m.Fp; a.H = m.two ? m.H : m.C;
  a.dact = m.two ? h->fc.dact0.as<float>() : nullptr;
  a.h1 = m.two ? h->fc.hact_p[0] : nullptr; a.h1_ld = m.two ? h->fc.hact_ld[0] : 0;
  a.W1 = m.two ? h->W[1] : nullptr; a.ld1 = m.ld1; a.off1 = m.off1; a.C = m.C; a.Cz = m.Cz;
  a.z = m.two ? q : u; a.rcap = m.rcap;
  LGNN_CALL(launch_first_layer(a, m.two, kc, s));
  if (m.two) {
    int cw = 1;
    while (cw < 64 && cw < m.C) cw <<= 1;
    GatherArgs g{};
    g.idx = idx; g.M = M; g.N = m.N;
    g.rowptr = h->P.rowptr; g.col = h->P.col; g.val = h->P.val;
    g.rpos = sf.rpos.as<int32_t>();
    g.z = q; g.rcap = m.rcap; g.Cz = m.Cz; g.C = m.C;
    g.sage = m.sage ? 1 : 0; g.cw = cw;
    g.theta = Vc; g.P = m.P; g.offb = m.offb;
    g.ns = kc; g.out = u;
    LGNN_CALL(launch_sampled_gather(g, s));
  }
  return 0;
}

// directions per chunk: q, qbar, u, w and the slab partials under half the workspace limit
int64_t struct_chunk(const lgnn_ctx* h, const StructModel& m, int64_t M, int64_t k, bool with_transpose) {
  int64_t per_dir = M * m.C * 4 + (m.two ? m.rcap * m.Cz * 4 : 0);
  if (with_transpose) per_dir = 2 * per_dir + int64_t(kMaxSlabs) * m.P * 4;
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(k, 32768), h->ws_limit / 2 / per_dir));
}

}  // namespace

int struct_prepare(lgnn_ctx* h, const int64_t* idx, int64_t M, StructModel& m, hipStream_t s) {
  LGNN_CALL(forward_ensure_aux(h, s));
  LGNN_CALL(struct_model(h, M, m));
  LGNN_CALL(sampled_ensure_input(h, s));
  LGNN_CALL(sampled_needed_rows(h, idx, M, s));
  return 0;
}

int struct_slabs(const StructModel& m, int64_t kc, int64_t tiles) {
  return int(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kMaxSlabs, cdiv(m.rcap, SBM)), cdiv(1024, kc * tiles))));
}

int launch_ggn_qbar(lgnn_ctx* h, const StructModel& m, const float* w, int64_t M, int64_t kc, float* qbar, hipStream_t s) {
  const int64_t bound = kc * m.rcap * m.Cz;
  hipLaunchKernelGGL(ggn_qbar_kernel, dim3(unsigned(std::min<int64_t>(cdiv(bound, 256), int64_t(1) << 20))), dim3(256), 0, s, w,
                     M, m.C, m.Cz, m.sage ? 1 : 0, h->ws.pos.as<int32_t>(), h->ws.mult.as<int32_t>(), h->PT.rowptr, h->PT.col,
                     h->PT.val, h->sf.rows.as<int32_t>(), h->sf.count.as<int32_t>(), m.rcap, kc, qbar);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_ggn_tn(const TnArgs& t, int nslab, int64_t atiles, hipStream_t s) {
  hipLaunchKernelGGL(ggn_tn_kernel, dim3(unsigned(nslab), unsigned(t.kc), unsigned(atiles * t.btiles)), dim3(256), 0, s, t);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_ggn_finish(const float* part, int nslab, int64_t per, float* G, hipStream_t s) {
  hipLaunchKernelGGL(ggn_finish_kernel, dim3(unsigned(std::min<int64_t>(cdiv(per, 256), 8192))), dim3(256), 0, s, part, nslab,
                     per, G);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

namespace {

int jvp_block_structured(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* out, hipStream_t s) {
  StructModel m;
  LGNN_CALL(struct_prepare(h, idx, M, m, s));
  Workspace& w = h->ws;
  const int64_t kc_max = struct_chunk(h, m, M, k, false);
  if (m.two) LGNN_CALL(w.ggn_q.reserve(size_t(kc_max) * m.rcap * m.Cz * 4));
  LGNN_CALL(w.ggn_u.reserve(size_t(kc_max) * M * m.C * 4));
  PhaseTimer tm{h, s};
  for (int64_t i0 = 0; i0 < k; i0 += kc_max) {
    const int64_t kc = std::min(kc_max, k - i0);
    LGNN_CALL(tm.mark());
    LGNN_CALL(struct_forward(h, m, idx, M, V + i0 * m.P, kc, w.ggn_q.as<float>(), w.ggn_u.as<float>(), s));
    hipLaunchKernelGGL(ggn_place_kernel, dim3(unsigned(cdiv(kc * M * m.C, 256))), dim3(256), 0, s, w.ggn_u.as<float>(), M, m.C,
                       kc, k, i0, out);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(tm.mark());
  }
  return 0;
}

int ggn_matmat_structured(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* G, hipStream_t s) {
  StructModel m;
  LGNN_CALL(struct_prepare(h, idx, M, m, s));
  Workspace& w = h->ws;
  SampledState& sf = h->sf;
  const int64_t kc_max = struct_chunk(h, m, M, k, true);
  if (m.two) {
    LGNN_CALL(w.ggn_q.reserve(size_t(kc_max) * m.rcap * m.Cz * 4));
    LGNN_CALL(w.ggn_qbar.reserve(size_t(kc_max) * m.rcap * m.Cz * 4));
  }
  LGNN_CALL(w.ggn_u.reserve(size_t(kc_max) * M * m.C * 4));
  LGNN_CALL(w.ggn_wt.reserve(size_t(kc_max) * M * m.C * 4));
  LGNN_CALL(w.ggn_part.reserve(size_t(kMaxSlabs) * kc_max * m.P * 4));
  float* q = w.ggn_q.as<float>();
  float* qbar = w.ggn_qbar.as<float>();
  float* u = w.ggn_u.as<float>();
  float* wv = w.ggn_wt.as<float>();
  float* part = w.ggn_part.as<float>();
  const int64_t big = int64_t(1) << 40;
  PhaseTimer tm{h, s};
  for (int64_t i0 = 0; i0 < k; i0 += kc_max) {
    const int64_t kc = std::min(kc_max, k - i0);
    // slabs of R's row tiles: about 1024 workgroups over the directions and output tiles (a function of the shapes alone)
    const int64_t tiles = m.two ? cdiv(m.H, SBM) * (cdiv(m.Fp, SBM) + cdiv(m.Cz, SBM)) : cdiv(m.C, SBM) * cdiv(m.Fp, SBM);
    const int nslab = int(std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kMaxSlabs, cdiv(m.rcap, SBM)),
                                                                  cdiv(1024, kc * tiles))));
    LGNN_CALL(tm.mark());
    LGNN_CALL(struct_forward(h, m, idx, M, V + i0 * m.P, kc, q, u, s));
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    hipLaunchKernelGGL(ggn_lambda_rows_kernel, dim3(unsigned(cdiv(kc * M, 256))), dim3(256), 0, s, u, h->ws.probs.as<float>(), idx,
                       m.N, M, m.C, kc, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, wv);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    LGNN_HIP_CHECK(hipMemsetAsync(part, 0, size_t(nslab) * kc * m.P * 4, s));
    if (m.two) {
      const int64_t bound = kc * m.rcap * m.Cz;
      hipLaunchKernelGGL(ggn_qbar_kernel, dim3(unsigned(std::min<int64_t>(cdiv(bound, 256), int64_t(1) << 20))), dim3(256), 0, s,
                         wv, M, m.C, m.Cz, m.sage ? 1 : 0, w.pos.as<int32_t>(), w.mult.as<int32_t>(), h->PT.rowptr, h->PT.col,
                         h->PT.val, sf.rows.as<int32_t>(), sf.count.as<int32_t>(), m.rcap, kc, qbar);
      LGNN_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(ggn_bias_kernel, dim3(unsigned(kc), unsigned(cdiv(m.C, 64))), dim3(1024), 0, s, wv, idx, m.N, M, m.C,
                         sf.in0.as<float>(), sf.ldk, m.Fp, m.sage ? 0 : 1, part, m.P, m.offb);
      LGNN_HIP_CHECK(hipGetLastError());
    }
    LGNN_CALL(tm.mark());
    LGNN_CALL(tm.mark());
    TnArgs t{};
    t.rows = sf.rows.as<int32_t>(); t.count = sf.count.as<int32_t>();
    t.in0 = sf.in0.as<float>(); t.ldk = sf.ldk; t.Fp = m.Fp;
    t.part = part; t.P = m.P; t.kc = kc;
    t.W1 = m.two ? h->W[1] : nullptr; t.ld1 = m.ld1; t.C = m.C; t.H = m.H;
    t.dact = m.two ? h->fc.dact0.as<float>() : nullptr;
    if (m.two) {
      // [g_W0 | g_b0] = sum_r sbar^T in0
      t.A = qbar; t.a_ld = m.Cz; t.a_ds = m.rcap * m.Cz; t.acols = m.Cz; t.mode = 1;
      t.B = sf.in0.as<float>(); t.b_ld = sf.ldk; t.bcols = m.Fp;
      t.adim = m.H; t.ooff = 0; t.old = m.Fp; t.amod = big; t.ashift = 0; t.bias_off = m.H * m.Fp;
      t.btiles = int(cdiv(m.Fp, SBM));
      hipLaunchKernelGGL(ggn_tn_kernel, dim3(unsigned(nslab), unsigned(kc), unsigned(cdiv(m.H, SBM) * t.btiles)), dim3(256), 0, s, t);
      LGNN_HIP_CHECK(hipGetLastError());
      // g_W1 = sum_r qbar^T h
      t.mode = 0;
      t.B = h->fc.hact_p[0]; t.b_ld = h->fc.hact_ld[0]; t.bcols = m.H;
      t.adim = m.Cz; t.ooff = m.off1; t.old = m.ld1; t.amod = m.C; t.ashift = m.H; t.bias_off = -1;
      t.btiles = int(cdiv(m.H, SBM));
      hipLaunchKernelGGL(ggn_tn_kernel, dim3(unsigned(nslab), unsigned(kc), unsigned(cdiv(m.Cz, SBM) * t.btiles)), dim3(256), 0, s, t);
      LGNN_HIP_CHECK(hipGetLastError());
    } else {
      // one layer: [g_W | g_b] = sum_m w^T in0 over the batch rows
      t.A = wv; t.a_ld = m.C; t.a_ds = M * m.C; t.acols = m.C; t.mode = 0;
      t.B = sf.in0.as<float>(); t.b_ld = sf.ldk; t.bcols = m.Fp;
      t.adim = m.C; t.ooff = 0; t.old = m.Fp; t.amod = big; t.ashift = 0; t.bias_off = m.C * m.Fp;
      t.btiles = int(cdiv(m.Fp, SBM));
      hipLaunchKernelGGL(ggn_tn_kernel, dim3(unsigned(nslab), unsigned(kc), unsigned(cdiv(m.C, SBM) * t.btiles)), dim3(256), 0, s, t);
      LGNN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ggn_finish_kernel, dim3(unsigned(std::min<int64_t>(cdiv(kc * m.P, 256), 8192))), dim3(256), 0, s, part,
                       nslab, kc * m.P, G + i0 * m.P);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(tm.mark());
  }
  return 0;
}

}  // namespace

int jvp_block(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* out, hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_REQUIRE(k > 0 && k < 65536 && M < (int64_t(1) << 31), "block size or batch size out of range");
  if (closed_form_model(h) && h->X != nullptr) return jvp_block_structured(h, idx, M, V, k, out, s);
  return jvp_block_general(h, idx, M, V, k, out, s);
}

int ggn_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k, int flags, float* G,
               float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_REQUIRE((flags & ~LGNN_GGN_FROM_JACOBIANS) == 0, "unknown flag");
  LGNN_REQUIRE(k > 0 && k < 65536 && M < (int64_t(1) << 31), "block size or batch size out of range");
  LGNN_CALL(forward_ensure(h, s));
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
  const bool structured = closed_form_model(h) && h->X != nullptr && !(flags & LGNN_GGN_FROM_JACOBIANS);
  if (structured) LGNN_CALL(ggn_matmat_structured(h, idx, M, V, k, G, s));
  else LGNN_CALL(ggn_matmat_general(h, idx, M, V, k, G, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn

extern "C" int lgnn_block_gram(lgnn_ctx* h, const float* A, int64_t ka, const float* B, int64_t kb, int64_t P, float* out,
                               void* stream) {
  if (!h || !A || !B || !out) { lgnn::set_error("null argument"); return 2; }
  if (ka <= 0 || kb <= 0 || P <= 0) { lgnn::set_error("empty block"); return 2; }
  lgnn::NtProblem p{};
  p.A = A; p.lda = P; p.B = B; p.ldb = P;
  p.Out = out; p.ldo = kb; p.o_es = 1;
  p.Ra = ka; p.Rb = kb; p.K = P; p.batch = 1;
  return lgnn::launch_nt_gemm(h, p, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_jvp_block(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* out, void* stream) {
  if (!h || (M > 0 && k > 0 && (!idx || !V || !out))) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0 || k <= 0) return 0;
  return lgnn::jvp_block(h, idx, M, V, k, out, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_ggn_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k, int flags,
                               float* G, float* loss_out, void* stream) {
  if (!h || (M > 0 && k > 0 && (!idx || !y || !V || !G || !loss_out))) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0 || k <= 0) return 0;
  return lgnn::ggn_matmat(h, idx, y, M, V, k, flags, G, loss_out, static_cast<hipStream_t>(stream));
}
