// Empirical and Monte-Carlo Fisher of one mini-batch from per-sample loss gradients.
//
// Reference: EFInterface (laplace/curvature/curvature.py:435-504) and GGNInterface with stochastic=True (:343-364) take the
// per-sample gradients g_n = J_n^T r_n of the loss (gradients, :169-210) -- r_n = softmax(f_n) - onehot(y_n) resp. f_n - y_n, with
// the true labels (empirical) or labels drawn from the model (Monte Carlo) -- and sum g_n g_n^T or its diagonal.
// Here, with r = resid_scale * (that residual) and the caller's `scale` on every square:
//   * diagonal only, closed-form models: g_n^2 has the form of the diagonal GGN with other weights (q_ef_kernel,
//     ef_last_weights_kernel), so the two kernels of diag.hip run through the launchers of diag.h -- no gradient is formed;
//   * otherwise the rows G [mc, P] of a chunk of samples: from the closed form (ef_grads_closed_form_kernel; M P floats, no
//     Jacobian) or, for deeper models and models with res / norm, contracted from a chunk of lgnn_jacobians' rows;
//     then their squares' column sums (diagonal), G^T G by rocBLAS (full), or the rows themselves (grads_out).
#include <rocblas/rocblas.h>

#include "closedform.h"
#include "diag.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// Empirical Fisher: the per-sample gradient of the first layer is diag(rho_n) T_n (+ diag(rho_s) S_n), rho[j] = sum_k r_k w_kj,
// so its square has the GGN kernel's form with q(neigh,neigh) = scale rho_n^2, q(self,neigh) = scale rho_s rho_n,
// q(self,self) = scale rho_s^2; the last layer's weights are scale r_k^2.
__global__ void q_ef_kernel(const float* __restrict__ r, int64_t M, int64_t C, const float* __restrict__ W1, int64_t ldw,
                            int64_t d, int64_t off_self, int64_t off_neigh, int has_self, float scale, float* __restrict__ q) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * d) return;
  const int64_t m = t / d, j = t - m * d;
  float rn = 0.f, rs = 0.f;
  for (int64_t k = 0; k < C; ++k) {
    const float rk = r[m * C + k];
    rn += rk * W1[k * ldw + off_neigh + j];
    if (has_self) rs += rk * W1[k * ldw + off_self + j];
  }
  q[t] = scale * rn * rn;
  if (has_self) {
    q[M * d + t] = scale * rs * rn;
    q[2 * M * d + t] = scale * rs * rs;
  }
}
__global__ void ef_last_weights_kernel(const float* __restrict__ r, int64_t n, float scale, float* __restrict__ w) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t < n) w[t] = scale * r[t] * r[t];
}
// ---- empirical / Monte-Carlo Fisher from per-sample gradients (EFInterface, laplace/curvature/curvature.py:435-504;
// GGNInterface with stochastic=True, :343-364): G[m, p] = sum_c r[m, c] J[m, c, p] with the functional gradient
// r = resid_scale * (softmax(f) - onehot(y_seed))  resp.  resid_scale * (f - y_seed) for the regression likelihood.
__global__ void ef_resid_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                const int64_t* __restrict__ idx, const void* __restrict__ yseed, int64_t mc, int64_t C,
                                int64_t N, int regression, float resid_scale, float* __restrict__ r, int* __restrict__ bad) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= mc * C) return;
  const int64_t m = t / C, c = t - m * C;
  const int64_t n = idx[m];
  float v = 0.f;
  if (n >= 0 && n < N) {
    if (regression) v = logits[n * C + c] - static_cast<const float*>(yseed)[t];
    else {
      const int64_t ys = static_cast<const int64_t*>(yseed)[m];
      if (ys < 0 || ys >= C) *bad = 2;
      v = probs[t] - (c == ys ? 1.f : 0.f);
    }
  }
  r[t] = resid_scale * v;
}
__global__ __launch_bounds__(256) void grads_from_jac_kernel(const float* __restrict__ J, const float* __restrict__ r,
                                                             int64_t mc, int64_t C, int64_t P, float* __restrict__ G) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t m = blockIdx.y;
  if (p >= P) return;
  const float* __restrict__ Jm = J + m * C * P + p;
  float acc = 0.f;
  for (int64_t c = 0; c < C; ++c) acc += r[m * C + c] * Jm[c * P];
  G[m * P + p] = acc;
}
__global__ __launch_bounds__(256) void sumsq_rows_kernel(const float* __restrict__ G, int64_t mc, int64_t P, float scale,
                                                         float* __restrict__ diag) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t m_begin = int64_t(blockIdx.y) * 32, m_end = min(mc, m_begin + 32);
  float acc = 0.f;
  for (int64_t m = m_begin; m < m_end; ++m) { const float g = G[m * P + p]; acc += g * g; }
  atomicAdd(&diag[p], scale * acc);
}

// out[P, P] += scale * G^T G for row-major G [rows, P] (the full empirical / MC Fisher of a chunk of per-sample gradients)
int gram_rows_sgemm(const float* G, int64_t rows, int64_t P, float scale, float* out, hipStream_t s) {
  rocblas_handle blas = static_cast<rocblas_handle>(blas_handle(s));
  LGNN_REQUIRE(blas != nullptr, "rocBLAS handle");
  const float one = 1.f;
  // column-major view of G: [P, rows] with ld = P;  out = G_cm G_cm^T (symmetric: row / column major coincide)
  const rocblas_status st = rocblas_sgemm(blas, rocblas_operation_none, rocblas_operation_transpose, rocblas_int(P),
                                          rocblas_int(P), rocblas_int(rows), &scale, G, rocblas_int(P), G, rocblas_int(P), &one,
                                          out, rocblas_int(P));
  if (st != rocblas_status_success) { set_error("rocblas_sgemm failed"); return 3; }
  return 0;
}

}  // namespace

// Per-sample loss gradients G[m, :] = sum_c r[m, c] J[m, c, :] of 1- and 2-layer models straight from the closed form
// (closedform.h): with rho_s[h] = sum_c r_c Ws[c, h], rho_n[h] = sum_c r_c Wn[c, h] the first layer's gradient is
// rho_s[h] Ts[h, :] + rho_n[h] Tn[h, :], the last layer's is r (x) phi~_a -- M * P floats instead of the M * C * P of the Jacobians.
// One workgroup row per sample, like jac_closed_form_kernel (jacobian.hip).
__global__ __launch_bounds__(256) void ef_grads_closed_form_kernel(const int64_t* __restrict__ idx, LGNN_CF_PARAMS,
                                                                   const float* __restrict__ r, float* __restrict__ G) {
  const ClosedForm cf = LGNN_CF_VIEW;
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  const int64_t C = cf.C, P = cf.P, H = cf.H, in0 = cf.in0, in_last = cf.in_last;
  float* __restrict__ Gm = G + m * P;
  const float* __restrict__ rm = r + m * C;
  const int64_t t0 = int64_t(blockIdx.y) * blockDim.x + threadIdx.x, tstep = int64_t(gridDim.y) * blockDim.x;
  if (a < 0 || a >= cf.N) {  // flagged by the batch prologue
    for (int64_t t = t0; t < P; t += tstep) Gm[t] = 0.f;
    return;
  }
  for (int64_t t = t0; t < C * in_last + C; t += tstep) {
    float v;
    if (t < C * in_last) { const int64_t k = t / in_last; v = rm[k] * feat_at(cf.PhiL, a, t - k * in_last); }
    else v = rm[t - C * in_last] * feat_at(cf.PhiL, a, in_last);
    Gm[cf.off_last + t] = v;
  }
  if (cf.L == 1) return;
  const int32_t ps = cf.rowptr[a], pe = cf.rowptr[a + 1];
  const int64_t in1 = in0 + 1;
  for (int64_t t = t0; t < H * in1; t += tstep) {
    const int64_t hh = t / in1, i = t - hh * in1;
    float rs = 0.f, rn = 0.f;
    for (int64_t c = 0; c < C; ++c) {
      const float rc = rm[c];
      if (cf.sage) { rs = fmaf(rc, cf.W1[c * cf.w1_ld + hh], rs); rn = fmaf(rc, cf.W1[c * cf.w1_ld + H + hh], rn); }
      else rn = fmaf(rc, cf.W1[c * cf.w1_ld + hh], rn);
    }
    float v = rn * cf_neigh(cf, ps, pe, hh, i);
    if (cf.sage) v = fmaf(rs, cf_self(cf, a, hh, i), v);
    Gm[i < in0 ? hh * in0 + i : H * in0 + hh] = v;
  }
}

static int ef_grads_closed_form(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* r, float* G, hipStream_t s) {
  LGNN_CALL(forward_ensure_aux(h, s));
  ClosedForm cf;
  LGNN_CALL(closed_form_view(h, cf));
  LGNN_REQUIRE(M < (int64_t(1) << 31), "too many samples");
  const unsigned per = unsigned(std::max<int64_t>(1, std::min<int64_t>(cdiv(std::max<int64_t>(cf.H * (cf.in0 + 1), cf.C * cf.in_last + cf.C), 256), cdiv(4096, M))));
  hipLaunchKernelGGL(ef_grads_closed_form_kernel, dim3(unsigned(M), per), dim3(256), 0, s, idx, LGNN_CF_ARGS(cf), r, G);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int ef_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y_seed, const void* y_loss, int64_t M, float resid_scale,
                  float scale, float* diag_out, float* full_out, float* grads_out, float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y_seed, "empty batch or null pointers");
  LGNN_REQUIRE(h->L >= 1, "no model bound");
  LGNN_REQUIRE(diag_out || full_out || grads_out, "nothing to compute");
  LGNN_REQUIRE(!y_loss || loss_out, "loss requested without an output");
  LGNN_CALL(forward_ensure(h, s));
  const int64_t C = h->dims[h->L], P = h->n_params, N = h->N;
  LGNN_CALL(batch_prologue(h, idx, y_loss ? y_loss : y_seed, M, false, false, y_loss ? loss_out : nullptr, s));
  // <= 2 layers: closed forms; deeper models (and LGNN_JAC_PLANES) contract Jacobians
  const bool closed = closed_form_model(h) && getenv("LGNN_JAC_PLANES") == nullptr;
  if (diag_out && !full_out && !grads_out && closed) {
    // diagonal only: the closed form of the diagonal GGN with other weights -- no Jacobians, no gradients
    LGNN_CALL(forward_ensure_aux(h, s));
    const int L = h->L;
    const int64_t H = L == 2 ? h->dims[1] : 0;
    LGNN_CALL(h->ws.misc.reserve(size_t(3) * M * std::max<int64_t>(H, 1) * 4 + size_t(2) * M * C * 4));
    float* q = h->ws.misc.as<float>();
    float* r = q + 3 * M * std::max<int64_t>(H, 1);
    float* wl = r + M * C;
    hipLaunchKernelGGL(ef_resid_kernel, dim3(unsigned(cdiv(M * C, 256))), dim3(256), 0, s, h->ws.probs.as<float>(),
                       h->fc.out.as<float>(), idx, y_seed, M, C, N, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, resid_scale, r,
                       h->ws.flags.as<int>());
    hipLaunchKernelGGL(ef_last_weights_kernel, dim3(unsigned(cdiv(M * C, 256))), dim3(256), 0, s, r, M * C, scale, wl);
    LGNN_HIP_CHECK(hipGetLastError());
    const int64_t slab = diag_slab(h, M, 2048);
    int64_t off = 0;
    if (L == 2) {
      const int has_self = h->kind == LGNN_KIND_SAGE ? 1 : 0;
      hipLaunchKernelGGL(q_ef_kernel, dim3(unsigned(cdiv(M * H, 256))), dim3(256), 0, s, r, M, C, h->W[1], h->in_dim[1], H,
                         int64_t(0), has_self ? H : int64_t(0), has_self, scale, q);
      LGNN_CALL(launch_diag_first_layer_staged(h, idx, M, slab, q, diag_out, s));
      off = H * h->in_dim[0] + H;
    }
    LGNN_CALL(launch_diag_last_layer(h, idx, M, slab, wl, diag_out + off, s));
    LGNN_CALL(batch_epilogue(h, idx, M, s));
    return 0;
  }
  // the gradients come straight from the closed form (M * P floats) or from chunks of Jacobians
  const int64_t jrows = closed ? 0 : C;
  const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(M, (h->ws_limit / 4) / std::max<int64_t>((jrows + 1) * P * 4, 1)));
  LGNN_CALL(h->ws.jac.reserve(size_t(mc_max) * (jrows + 1) * P * 4 + size_t(mc_max) * C * 4));
  float* J = h->ws.jac.as<float>();
  float* G = J + mc_max * jrows * P;
  float* r = G + mc_max * P;
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    if (!closed) LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    const void* ys = h->lik == LGNN_LIK_REGRESSION ? static_cast<const void*>(static_cast<const float*>(y_seed) + m0 * C)
                                                   : static_cast<const void*>(static_cast<const int64_t*>(y_seed) + m0);
    hipLaunchKernelGGL(ef_resid_kernel, dim3(unsigned(cdiv(mc * C, 256))), dim3(256), 0, s, h->ws.probs.as<float>() + m0 * C,
                       h->fc.out.as<float>(), idx + m0, ys, mc, C, N, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, resid_scale, r,
                       h->ws.flags.as<int>());
    if (closed) LGNN_CALL(ef_grads_closed_form(h, idx + m0, mc, r, G, s));
    else hipLaunchKernelGGL(grads_from_jac_kernel, dim3(unsigned(cdiv(P, 256)), unsigned(mc)), dim3(256), 0, s, J, r, mc, C, P, G);
    LGNN_HIP_CHECK(hipGetLastError());
    if (grads_out) LGNN_HIP_CHECK(hipMemcpyAsync(grads_out + m0 * P, G, size_t(mc) * P * 4, hipMemcpyDeviceToDevice, s));
    if (diag_out)
      hipLaunchKernelGGL(sumsq_rows_kernel, dim3(unsigned(cdiv(P, 256)), unsigned(cdiv(mc, 32))), dim3(256), 0, s, G, mc, P,
                         scale, diag_out);
    if (full_out) LGNN_CALL(gram_rows_sgemm(G, mc, P, scale, full_out, s));
    LGNN_HIP_CHECK(hipGetLastError());
  }
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn
