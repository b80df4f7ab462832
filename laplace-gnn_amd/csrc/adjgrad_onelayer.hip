// Adjacency gradient of the marginal likelihood (adjgrad.hip), one-layer GCN, every posterior.
#include "adjgrad.h"
#include "device_utils.h"

namespace lgnn {

// One-layer GCN (the reference's Banana configurations, gnn/configs/original/stegcn_config.yaml: num_layers 1):
// out = P (X W^T + 1 b^T), f_n = W phi_n + b rho_n with psi_n = [phi_n | rho_n] = [P X | rowsum(P)][n] (the cached E rows),
// J_n[c, (c', j)] = delta_cc' psi_n[j].  Everything lives on the batch rows: no planes, no hidden layer, and the batch
// calls only fill out_bar [N, C] and e_bar [N, F + 1] (the Kronecker posterior: out_bar and the seed SDDMM); the finish adds
// gradP[(a, b)] = <out_bar[a], Z[b]> + <e_bar[a, :F], X[b]> + e_bar[a, F], Z = X W^T + 1 b^T  (DESIGN.md 12.20).
namespace {

// Diagonal posterior, one wave per batch sample m (n = idx[m]); Gamma_c = [gamma_W[c, :] | gamma_b[c]]:
//   kappa_c = sum_j Gamma_c[j] psi[j]^2      pbar_c = (1 - 2 p_c) kappa_c
//   out_bar[n] += p * (pbar - <p, pbar>) + loss_scale (p - onehot(y))      e_bar[n] += 2 psi * sum_c p_c (1 - p_c) Gamma_c
__global__ __launch_bounds__(256) void onelayer_diag_sample_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ y,
                                                                   int64_t M, int64_t N, int64_t C, int64_t F,
                                                                   const float* __restrict__ E, int64_t lde,
                                                                   const float* __restrict__ probs,
                                                                   const float* __restrict__ gamma, float loss_scale,
                                                                   float* __restrict__ out_bar, float* __restrict__ e_bar) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m = int64_t(blockIdx.x) * 4 + wave;
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) return;  // flagged by the batch prologue
  float* __restrict__ pb = sm + size_t(wave) * C;
  const int64_t F1 = F + 1;
  const float* __restrict__ psi = E + n * lde;
  const float* __restrict__ pm = probs + m * C;
  const float* __restrict__ gb = gamma + C * F;
  for (int64_t c = 0; c < C; ++c) {
    float acc = 0.f;
    for (int64_t j = lane; j < F1; j += 64) {
      const float v = psi[j];
      acc += (j < F ? gamma[c * F + j] : gb[c]) * v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) pb[c] = (1.f - 2.f * pm[c]) * acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float dot = 0.f;
  for (int64_t c = lane; c < C; c += 64) dot += pm[c] * pb[c];
  dot = wave_sum(dot);
  const int64_t yy = y[m];
  for (int64_t c = lane; c < C; c += 64) {
    const float p = pm[c];
    atomicAdd(&out_bar[n * C + c], p * (pb[c] - dot) + loss_scale * (p - (c == yy ? 1.f : 0.f)));
  }
  for (int64_t j = lane; j < F1; j += 64) {
    float acc = 0.f;
    for (int64_t c = 0; c < C; ++c) {
      const float p = pm[c];
      acc += p * (1.f - p) * (j < F ? gamma[c * F + j] : gb[c]);
    }
    atomicAdd(&e_bar[n * F1 + j], 2.f * psi[j] * acc);  // (a repeated node id: several samples share the row)
  }
}

// Full posterior: e_bar[n, j] += sum_c R[m][c][pos(c, j)], pos(c, j) = c F + j (weight) / C F + c (bias): the only entries
// of the direction R_m = 2 Lambda_m J_m Gamma that d J_m[c, :] = delta_cc' d psi_n pairs with
__global__ void onelayer_full_ebar_kernel(const int64_t* __restrict__ idx, int64_t mc, int64_t N, int64_t C, int64_t F,
                                          const float* __restrict__ R, float* __restrict__ e_bar) {
  const int64_t F1 = F + 1, P = C * F1;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= mc * F1) return;
  const int64_t m = t / F1, j = t - m * F1;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) return;
  const float* __restrict__ Rm = R + m * C * P;
  float acc = 0.f;
  for (int64_t c = 0; c < C; ++c) acc += Rm[c * P + (j < F ? c * F + j : C * F + c)];
  atomicAdd(&e_bar[n * F1 + j], acc);
}

}  // namespace

int check_model_onelayer(const lgnn_ctx* h) {
  LGNN_REQUIRE(h->L == 1, "internal: one-layer route");
  LGNN_REQUIRE(h->kind == LGNN_KIND_GCN, "adjacency gradient, 1-layer models: GCN (1-layer GraphSAGE is not covered)");
  LGNN_REQUIRE(!h->extras(), "adjacency gradient: models without res / norm");
  LGNN_REQUIRE(h->lik == LGNN_LIK_CLASSIFICATION, "adjacency gradient: classification");
  LGNN_REQUIRE(h->dims[1] <= 256, "adjacency gradient: at most 256 classes");
  return 0;
}

int onelayer_diag_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, float loss_scale,
                                float* out_bar, float* e_bar, hipStream_t s) {
  LGNN_CALL(check_model_onelayer(h));
  LGNN_REQUIRE(M > 0 && idx && y && gamma && out_bar && e_bar, "empty batch or null pointers");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t N = h->N, C = h->dims[1], F = h->dims[0];
  LGNN_REQUIRE(h->n_params == C * F + C, "internal: parameter count");
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, nullptr, s));
  hipLaunchKernelGGL(onelayer_diag_sample_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), size_t(4) * C * 4, s, idx,
                     static_cast<const int64_t*>(y), M, N, C, F, h->fc.prop_in[0].as<float>(), h->fc.prop_ld[0],
                     h->ws.probs.as<float>(), gamma, loss_scale, out_bar, e_bar);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

// K_n and R_n from the closed-form Jacobian rows (jacobian.hip handles L == 1) through fulladj.hip's product kernel, in
// chunks of samples under the workspace cap; chunk_directions also adds the batch's part of out_bar
int onelayer_full_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* Gamma, float loss_scale,
                                float* out_bar, float* e_bar, hipStream_t s) {
  LGNN_CALL(check_model_onelayer(h));
  LGNN_REQUIRE(M > 0 && idx && y && Gamma && out_bar && e_bar, "empty batch or null pointers");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t N = h->N, C = h->dims[1], F = h->dims[0], P = h->n_params;
  LGNN_REQUIRE(P == C * F + C, "internal: parameter count");
  LGNN_REQUIRE(size_t(C * C + C + 4) * 4 <= 64 * 1024, "too many classes");
  const int64_t per_sample = C * 2 * P * 4;  // J and R rows
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / std::max<int64_t>(per_sample, 1)));
  LGNN_REQUIRE(chunk * C < (int64_t(1) << 31), "adjacency gradient, diagonal / full posterior: chunk too large");
  LGNN_CALL(h->ws.jac.reserve(size_t(chunk) * C * P * 4));
  LGNN_CALL(h->ws.adj_dir.reserve(size_t(chunk) * C * P * 4));
  LGNN_CALL(h->ws.probs.reserve(size_t(chunk) * (C + C * C) * 4));
  float* J = h->ws.jac.as<float>();
  float* R = h->ws.adj_dir.as<float>();
  float* probs = h->ws.probs.as<float>();
  float* Kn = probs + chunk * C;
  const int64_t* yy = static_cast<const int64_t*>(y);
  for (int64_t m0 = 0; m0 < M; m0 += chunk) {
    const int64_t mc = std::min(chunk, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    LGNN_CALL(chunk_directions(h, idx + m0, yy + m0, mc, J, nullptr, Gamma, loss_scale, probs, Kn, R, out_bar, s));
    hipLaunchKernelGGL(onelayer_full_ebar_kernel, dim3(unsigned(cdiv(mc * (F + 1), 256))), dim3(256), 0, s, idx + m0, mc, N, C,
                       F, R, e_bar);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// Kronecker posterior: A_0 = X^T X does not depend on the adjacency; B_0 = sum_batches sum_c g_c^T g_c, g_c = P[batch, :]^T V_c
// is the top layer of kfac_adjgrad_batch's chain: gbar = 2 g Gamma_B, the seed SDDMM on the batch rows' entries, the seed
// adjoint into out_bar
int onelayer_kfac_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags, const float* gamma_B,
                                float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a, const int32_t* cand_b,
                                int64_t K, float* grad_cand, hipStream_t s) {
  LGNN_CALL(check_model_onelayer(h));
  LGNN_REQUIRE(M > 0 && idx && y && gamma_B && grad_P && out_bar, "empty batch or null pointers");
  LGNN_CALL(forward_ensure(h, s));
  const int64_t N = h->N, C = h->dims[1], CC = C * C;
  const bool fork_exact = (flags & LGNN_FLAG_FORK_EXACT_SEED) != 0;
  LGNN_CALL(batch_prologue(h, idx, y, M, true, fork_exact, nullptr, s));
  LGNN_CALL(h->ws.top.reserve(size_t(N) * CC * 4 + 16));
  LGNN_CALL(h->ws.active.reserve(size_t(N)));
  float* g = h->ws.top.as<float>();  // planes [C][N][C]
  LGNN_CALL(launch_seed_planes(h, g, s));
  LGNN_CALL(h->ws.jac.reserve(size_t(M) * CC * 4));  // Vbar [M][C][C]
  float* vbar = h->ws.jac.as<float>();
  const int64_t per_class = N * C * 4;
  const int64_t cc_max = std::max<int64_t>(1, std::min<int64_t>(C, h->ws_limit / std::max<int64_t>(per_class, 1)));
  LGNN_CALL(h->ws.planes_b.reserve(size_t(cc_max) * N * C * 4));
  float* GB = h->ws.planes_b.as<float>();
  for (int64_t c0 = 0; c0 < C; c0 += cc_max) {
    const int64_t cc = std::min(cc_max, C - c0);
    LGNN_CALL(sgemm_rm(s, cc * N, C, C, 2.f, g + c0 * N * C, C, gamma_B, C, 0.f, GB, C));
    LGNN_CALL(launch_seed_sddmm(h, idx, M, GB, c0, cc, grad_P, cand_a, cand_b, K, grad_cand, s));
    LGNN_CALL(launch_seed_gather(h, idx, M, GB, c0, cc, vbar, s));
  }
  LGNN_CALL(launch_seed_adjoint(h, idx, y, M, vbar, fork_exact, loss_scale, out_bar, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

// e_bar == null: the Kronecker posterior (no adjoint of [P X | rowsum(P)]: its A factor is X^T X)
int onelayer_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* e_bar, float* grad_P, float* grad_adj,
                            const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, float* grad_cand_adj,
                            hipStream_t s) {
  LGNN_CALL(check_model_onelayer(h));
  LGNN_REQUIRE(K == 0 || (cand_a && cand_b && grad_cand && grad_cand_adj), "candidate pairs without their buffers");
  LGNN_REQUIRE(out_bar && grad_P && grad_adj, "null pointers");
  LGNN_CALL(forward_ensure(h, s));
  LGNN_CALL(ensure_wt(h, s));
  LGNN_CALL(forward_input_view(h, s));
  const int64_t N = h->N, C = h->dims[1], F = h->dims[0];
  // Z = X W^T + b [N, C] (the forward keeps only P Z)
  LGNN_CALL(h->ws.planes_a.reserve(size_t(N) * C * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* Z = h->ws.planes_a.as<float>();
  GemmEpilogue eb;
  eb.bias = h->b[0];
  LGNN_CALL(launch_gemm(h->fc.lin_in_p[0], h->fc.lin_in_ld[0], h->Wt[0].as<float>(), C, Z, C, N, F, C, eb, s));
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, out_bar, C, 0, Z, C, 0, C, 1, grad_P, s));
  LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, out_bar, C, 0, Z, C, 0, C, 1, nullptr, grad_cand, s));
  if (e_bar) {
    const int64_t F1 = F + 1;
    LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, e_bar, F1, 0, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], 0, F, 1, grad_P, s));
    LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, e_bar, F1, 0, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], 0, F, 1, nullptr,
                               grad_cand, s));
    LGNN_CALL(launch_row_const(h, e_bar + F, F1, grad_P, cand_a, K, grad_cand, s));
  }
  return normalize_adj_backward(h, grad_P, grad_adj, cand_a, cand_b, K, grad_cand, grad_cand_adj, s);
}

}  // namespace lgnn
