// Last-layer Kronecker and diagonal GGN of one mini-batch.
//
// Reference: KronLLLaplace / DiagLLLaplace (laplace/lllaplace.py:381-475, 477-...) fit a KronLaplace / DiagLaplace on the
// final nn.Linear alone, fed with the features the rest of the network produces; their curvature calls are
// CurvlinopsInterface.kron on that head (laplace/curvature/curvlinops.py:77-108: KFAC of one Linear, A rescaled by M / N)
// and GGNInterface.diag on last_layer_jacobians (laplace/curvature/curvature.py:132-167, 412-432).
//
// Per batch sample n the logits are f_n = W phi_n + s_n b (GraphSAGE: phi_n = [h_n | (A_bar h)_n], s_n = 1; GCN:
// phi_n = (A_hat h)_n, s_n = rowsum(A_hat)_n -- feat_views of closedform.h), so with the KFAC seeds V_n [C, C] of kfac_seed.hip
//   A   [D, D] += Phi^T Phi / n_train              (fp32 MFMA Gram of the gathered rows, kernels.hip)
//   B   [C, C] += sum_n V_n V_n^T
//   B_b [C, C] += sum_n s_n^2 V_n V_n^T            (the exact bias block; equals B for GraphSAGE)
//   diag[c D + d] += sum_n Lambda_n[c, c] phi_n[d]^2,   diag[C D + c] += sum_n Lambda_n[c, c] s_n^2
// Every batch row is a sample of its own here (a repeated node id is two samples: the head sees two input rows).
//
// The seed block is diagonal plus rank two (seed_factors of the oracle):  V[k, c] = alpha_c d_kc - beta_c u_k - gamma_c p_k  with
// sp = sqrt(p), t = f - sum_k p_k f_k;  fork exact: alpha = sp (1 + t/2), beta = sp, gamma = sp t / 2, u = p (1 + t);  upstream:
// alpha = beta = sp, gamma = 0, u = p (then V V^T = diag(p) - p p^T).  Hence, with a = alpha beta, g = alpha gamma,
//   (V V^T)[k, k'] = d_kk' alpha_k^2 + u_k r_k' + p_k t'_k' - a_k u_k' - g_k p_k',
//   r = (sum beta^2) u + (sum beta gamma) p - a,   t' = (sum beta gamma) u + (sum gamma^2) p - g
// -- C^2 work per sample from seven C-vectors; no seed block is ever written.
#include <algorithm>

#include "closedform.h"
#include "device_utils.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// softmax of one logits row by one wave; lane l owns the classes l, l + 64, ... of f_s / p_s (nothing is read across lanes).
// Returns logsumexp(f) - f[yy] (0 for a label outside [0, C): the caller flags it) and mbar = sum_k p_k f_k.
__device__ __forceinline__ void ll_softmax_row(const float* __restrict__ row, int C, int64_t yy, int lane, float* f_s,
                                               float* p_s, float& nll, float& mbar) {
  float mx = -INFINITY, fy = 0.f;
  for (int k = lane; k < C; k += 64) {
    const float v = row[k];
    f_s[k] = v;
    mx = fmaxf(mx, v);
    if (k == yy) fy = v;
  }
  mx = wave_max_f(mx);
  fy = wave_sum(fy);
  float se = 0.f;
  for (int k = lane; k < C; k += 64) {
    const float e = expf(f_s[k] - mx);
    p_s[k] = e;
    se += e;
  }
  se = wave_sum(se);
  const float inv = 1.0f / se;
  float mb = 0.f;
  for (int k = lane; k < C; k += 64) {
    const float p = p_s[k] * inv;
    p_s[k] = p;
    mb += p * f_s[k];
  }
  mbar = wave_sum(mb);
  nll = logf(se) + mx - fy;
}

// one atomic per workgroup for the loss; the waves' shares meet in LDS
__device__ __forceinline__ void ll_flush_loss(float loss_acc, float* loss_part, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) loss_part[wave] = loss_acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (loss_part[0] + loss_part[1]) + (loss_part[2] + loss_part[3]));
}

enum { kVecU = 0, kVecP, kVecA, kVecG, kVecR, kVecT, kVecD, kNumVec };  // the seven C-vectors of a sample (see the header)

// B, B_b and the loss of the samples [blockIdx.x * slab, + slab): chunks of SC samples -- the waves write the samples' vectors
// to LDS, then every thread adds the chunk into the entries (k <= k') of the workgroup's LDS accumulators it owns.  One float
// atomic per entry and workgroup at the end (both mirror images).
// LDS: vec [kNumVec][SC][C] | s2 [SC] | accB [C C] | accBb [C C] (only with a bias column: without one B_b = B)
__global__ __launch_bounds__(256) void ll_kron_rows_kernel(const float* __restrict__ logits, int C,
                                                           const int64_t* __restrict__ idx,
                                                           const int64_t* __restrict__ y, int64_t M, int64_t N, int64_t slab,
                                                           int SC, const float* __restrict__ bias_col, int fork_exact,
                                                           float* __restrict__ B_out, float* __restrict__ Bb_out,
                                                           float* __restrict__ loss, int* __restrict__ bad) {
  extern __shared__ float sm[];
  __shared__ float loss_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CC = C * C;
  float* vec = sm;
  float* s2 = vec + size_t(kNumVec) * SC * C;
  float* accB = s2 + SC;
  float* accBb = bias_col ? accB + CC : nullptr;
  for (int q = tid; q < CC; q += 256) {
    accB[q] = 0.f;
    if (accBb) accBb[q] = 0.f;
  }
  const int64_t m_begin = int64_t(blockIdx.x) * slab, m_end = min(M, m_begin + slab);
  float loss_acc = 0.f;
  for (int64_t m0 = m_begin; m0 < m_end; m0 += SC) {
    __syncthreads();  // the previous chunk's vectors have been read (first pass: the accumulators are zeroed)
    for (int j = wave; j < SC; j += 4) {
      const int64_t m = m0 + j;
      float* u_s = vec + (size_t(kVecU) * SC + j) * C;
      float* p_s = vec + (size_t(kVecP) * SC + j) * C;
      float* a_s = vec + (size_t(kVecA) * SC + j) * C;
      float* g_s = vec + (size_t(kVecG) * SC + j) * C;
      float* r_s = vec + (size_t(kVecR) * SC + j) * C;
      float* t_s = vec + (size_t(kVecT) * SC + j) * C;
      float* d_s = vec + (size_t(kVecD) * SC + j) * C;
      const int64_t n = m < m_end ? idx[m] : -1;
      if (n < 0 || n >= N) {  // past the slab, or an invalid id (flagged): the sample adds nothing
        if (m < m_end && lane == 0) bad[1] = 1;
        for (int k = lane; k < C; k += 64) u_s[k] = p_s[k] = a_s[k] = g_s[k] = r_s[k] = t_s[k] = d_s[k] = 0.f;
        if (lane == 0) s2[j] = 0.f;
        continue;
      }
      const int64_t yy = y[m];
      float nll, mb;
      ll_softmax_row(logits + n * C, C, yy, lane, u_s /* holds f until it is overwritten below */, p_s, nll, mb);
      if (lane == 0) {
        if (yy < 0 || yy >= C) *bad = 2;
        else loss_acc += nll;
        const float sn = bias_col ? bias_col[n] : 1.f;
        s2[j] = sn * sn;
      }
      float sbb = 0.f, sbg = 0.f, sgg = 0.f;
      for (int k = lane; k < C; k += 64) {
        const float p = p_s[k], t = fork_exact ? u_s[k] - mb : 0.f;
        const float sp = sqrtf(p);
        const float alpha = sp * (1.f + 0.5f * t), gamma = 0.5f * sp * t;  // beta = sp
        u_s[k] = p * (1.f + t);
        a_s[k] = alpha * sp;
        g_s[k] = alpha * gamma;
        d_s[k] = alpha * alpha;
        sbb += p;
        sbg += sp * gamma;
        sgg += gamma * gamma;
      }
      sbb = wave_sum(sbb);
      sbg = wave_sum(sbg);
      sgg = wave_sum(sgg);
      for (int k = lane; k < C; k += 64) {
        const float u = u_s[k], p = p_s[k];
        r_s[k] = sbb * u + sbg * p - a_s[k];
        t_s[k] = sbg * u + sgg * p - g_s[k];
      }
    }
    __syncthreads();
    for (int q = tid; q < CC; q += 256) {
      const int k = q / C, k2 = q - k * C;
      if (k > k2) continue;
      float acc = 0.f, accb = 0.f;
      for (int j = 0; j < SC; ++j) {
        const float* __restrict__ vj = vec + size_t(j) * C;
        const size_t vs = size_t(SC) * C;
        float v = vj[kVecU * vs + k] * vj[kVecR * vs + k2] + vj[kVecP * vs + k] * vj[kVecT * vs + k2] -
                  vj[kVecA * vs + k] * vj[kVecU * vs + k2] - vj[kVecG * vs + k] * vj[kVecP * vs + k2];
        if (k == k2) v += vj[kVecD * vs + k];
        acc += v;
        accb += s2[j] * v;
      }
      accB[q] += acc;
      if (accBb) accBb[q] += accb;
    }
  }
  // (every thread reads back only the entries it has written itself)
  for (int q = tid; q < CC; q += 256) {
    const int k = q / C, k2 = q - k * C;
    if (k > k2) continue;
    const float vb = accB[q], vbb = accBb ? accBb[q] : vb;
    atomicAdd(&B_out[q], vb);
    atomicAdd(&Bb_out[q], vbb);
    if (k != k2) {
      atomicAdd(&B_out[k2 * C + k], vb);
      atomicAdd(&Bb_out[k2 * C + k], vbb);
    }
  }
  ll_flush_loss(loss_acc, loss_part, loss);
}

constexpr int kDiagSlab = 32;  // samples per workgroup of ll_diag_rows_kernel (their squared features stay in registers)

// diag of the samples [blockIdx.y * 32, + 32) on the columns [blockIdx.x * 256, + 256) of [phi | s]: the waves write the
// samples' Lambda_n[c, c] = p_c (1 - p_c) to LDS (w [32][C]), a thread squares its column of the 32 rows and adds one value per
// class.  The workgroups of the first column chunk also add the loss.
__global__ __launch_bounds__(256) void ll_diag_rows_kernel(const float* __restrict__ logits, int C,
                                                           const int64_t* __restrict__ idx,
                                                           const int64_t* __restrict__ y, int64_t M, FeatView Phi,
                                                           float* __restrict__ diag, float* __restrict__ loss,
                                                           int* __restrict__ bad) {
  extern __shared__ float sm[];
  __shared__ float loss_part[4];
  __shared__ int64_t node[kDiagSlab];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* w = sm;                  // [kDiagSlab][C]
  float* f_s = w + kDiagSlab * C; // [4][C]: a wave's logits row
  const int64_t m_begin = int64_t(blockIdx.y) * kDiagSlab, m_end = min(M, m_begin + kDiagSlab);
  const bool first = blockIdx.x == 0;
  float loss_acc = 0.f;
  for (int j = wave; j < kDiagSlab; j += 4) {
    const int64_t m = m_begin + j;
    const int64_t n = m < m_end ? idx[m] : -1;
    float* w_s = w + j * C;
    if (lane == 0) node[j] = n;
    if (n < 0 || n >= Phi.nrows) {
      if (m < m_end && lane == 0) bad[1] = 1;
      for (int k = lane; k < C; k += 64) w_s[k] = 0.f;
      continue;
    }
    const int64_t yy = y[m];
    float nll, mb;
    ll_softmax_row(logits + n * C, C, yy, lane, f_s + wave * C, w_s, nll, mb);
    if (lane == 0) {
      if (yy < 0 || yy >= C) *bad = 2;
      else if (first) loss_acc += nll;
    }
    for (int k = lane; k < C; k += 64) { const float p = w_s[k]; w_s[k] = p * (1.f - p); }
  }
  __syncthreads();
  const int64_t i = int64_t(blockIdx.x) * 256 + tid;
  if (i <= Phi.width) {
    float ph2[kDiagSlab];
#pragma unroll
    for (int j = 0; j < kDiagSlab; ++j) {
      const float ph = feat(Phi, node[j], i);  // id -1 (past the batch) or out of range: 0
      ph2[j] = ph * ph;
    }
    const int64_t D = Phi.width;
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < kDiagSlab; ++j) acc += w[j * C + c] * ph2[j];
      atomicAdd(i < D ? &diag[int64_t(c) * D + i] : &diag[int64_t(C) * D + c], acc);
    }
  }
  if (first) ll_flush_loss(loss_acc, loss_part, loss);
}

int ll_check(lgnn_ctx* h) {
  LGNN_REQUIRE(h->L >= 1, "no model bound");
  LGNN_REQUIRE(h->lik == LGNN_LIK_CLASSIFICATION, "last-layer Kronecker / diagonal GGN kernels: classification likelihood");
  return 0;
}

}  // namespace

int lastlayer_kron_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train, uint32_t flags,
                              float* A_out, float* B_out, float* Bb_out, float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y && A_out && B_out && Bb_out && loss_out, "empty batch or null pointers");
  LGNN_REQUIRE(n_train > 0, "n_train must be positive");
  LGNN_CALL(ll_check(h));
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t C = h->dims[h->L];
  FeatView Phi;
  feat_views(h, h->L - 1, Phi);
  const int64_t D = Phi.width, ldp = cdiv(D + 1, 4) * 4;
  // A: the batch's rows [phi | s | 0] gathered once, then the fp32 MFMA Gram of their first D columns
  LGNN_CALL(h->ws.planes_a.reserve(size_t(M) * ldp * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* PhiM = h->ws.planes_a.as<float>();
  LGNN_CALL(launch_ll_build_phi(idx, M, Phi, ldp, PhiM, s));
  LGNN_CALL(launch_gram_scaled(PhiM, ldp, M, D, A_out, 1.0f / float(n_train), s));
  LGNN_CALL(launch_symmetrize_upper(A_out, D, s));  // (the lower triangle is rewritten from the upper one: idempotent)
  // B, B_b, loss: one pass over the rows
  const bool has_s = Phi.bias_col != nullptr;
  const size_t acc_bytes = size_t(has_s ? 2 : 1) * C * C * 4;
  int SC = 16;
  auto smem_of = [&](int sc) { return acc_bytes + (size_t(kNumVec) * sc * C + sc) * 4; };
  while (SC > 4 && smem_of(SC) > 158 * 1024) SC /= 2;
  const size_t smem = smem_of(SC);
  LGNN_REQUIRE(smem <= 158 * 1024, "too many classes for the last-layer Kronecker kernel");
  LGNN_CALL(lds_opt_in<&ll_kron_rows_kernel>(158 * 1024));
  // ~512 workgroups (two per CU) of whole chunks: every workgroup ends with C^2 float atomics per factor
  const int64_t slab = cdiv(std::max<int64_t>(SC, cdiv(M, 512)), SC) * SC;
  hipLaunchKernelGGL(ll_kron_rows_kernel, dim3(unsigned(cdiv(M, slab))), dim3(256), smem, s, h->fc.out.as<float>(), int(C),
                     idx, static_cast<const int64_t*>(y), M, h->N, slab, SC, Phi.bias_col,
                     (flags & LGNN_FLAG_FORK_EXACT_SEED) ? 1 : 0, B_out, Bb_out, loss_out, h->ws.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int lastlayer_diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* diag_out, float* loss_out,
                              hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y && diag_out && loss_out, "empty batch or null pointers");
  LGNN_CALL(ll_check(h));
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t C = h->dims[h->L];
  FeatView Phi;
  feat_views(h, h->L - 1, Phi);
  const size_t smem = size_t(kDiagSlab + 4) * C * 4;
  LGNN_REQUIRE(smem <= 60 * 1024, "too many classes for the last-layer diagonal kernel");
  LGNN_REQUIRE(cdiv(M, kDiagSlab) < 65536, "batch too large for one launch of the last-layer diagonal kernel");
  hipLaunchKernelGGL(ll_diag_rows_kernel, dim3(unsigned(cdiv(Phi.width + 1, 256)), unsigned(cdiv(M, kDiagSlab))), dim3(256),
                     smem, s, h->fc.out.as<float>(), int(C), idx, static_cast<const int64_t*>(y), M, Phi, diag_out, loss_out,
                     h->ws.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn
