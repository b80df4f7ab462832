// Per-sample Jacobians  J[m][c][:] = d f[idx[m], c] / d theta  for the GLM predictive ("next" row 8(f)-3).
//
// Reference: CurvatureInterface.jacobians (laplace/curvature/curvature.py:89-130): torch.func.jacrev of the whole
// dense-adjacency model, M*C backward passes through autograd, result [M, C, P] with the parameters in
// named_parameters order, each flattened row major (weight [out, in], then bias).
//
// Here the M*C backward passes travel together as planes, exactly like the C class columns of the KFAC path
// (kfac.hip), with the per-layer contraction g_l^T in_l (one strided-batched rocBLAS GEMM per layer, written straight
// into J) in place of the Gram g_l^T g_l:
//     top    g_{L-1}[(m,c)] = P^T-scatter of e_c at node idx[m]          (GraphSAGE: e_c at idx[m] itself)
//     layer  dW_l[(m,c)] = g_l^T in_l   [out_l x in_l]      db_l[(m,c)] = column sums of g_l
//     down   g_{l-1} = P^T (act'(h_l) * (g_l W_l))          (GraphSAGE: act'(h_l) * (dcat[:, :d] + P^T dcat[:, d:]))
// The result is as large as the reference's (M*C*P floats); samples are processed in chunks that fit the workspace cap.
// 1- and 2-layer models without res / norm skip the planes: closed form (closedform.h).  full_accumulate, the all-weights
// full GGN, consumes whole chunks of these rows and sits at the end of the file.
#include <rocblas/rocblas.h>

#include "closedform.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// GCN: planes[(m, c)][v][c] = P[idx[m], v] for the entries v of row idx[m] of P; one wave per sample.
__global__ __launch_bounds__(256) void jac_top_gcn_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int64_t C,
                                                          const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, const float* __restrict__ val,
                                                          float* __restrict__ g, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) { if (lane == 0) bad[1] = 1; return; }
  const int32_t e = rowptr[n + 1];
  for (int32_t p = rowptr[n] + lane; p < e; p += 64) {
    const int64_t v = col[p];
    const float x = val[p];
    for (int64_t c = 0; c < C; ++c) g[((m * C + c) * N + v) * C + c] = x;
  }
}
// GraphSAGE: the last Linear's output is not propagated
__global__ void jac_top_sage_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int64_t C,
                                    float* __restrict__ g, int* __restrict__ bad) {
  const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= M * C) return;
  const int64_t m = q / C, c = q - m * C;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) { bad[1] = 1; return; }
  g[(q * N + n) * C + c] = 1.f;
}

// out[p * out_stride + o] = sum_v g[p][v][o]; one workgroup per plane
__global__ __launch_bounds__(256) void plane_colsum_kernel(const float* __restrict__ g, int64_t N, int64_t D,
                                                           float* __restrict__ out, int64_t out_stride) {
  const int64_t p = blockIdx.x;
  const float* __restrict__ gp = g + p * N * D;
  for (int64_t o = threadIdx.x; o < D; o += blockDim.x) {
    float acc = 0.f;
    for (int64_t v = 0; v < N; ++v) acc += gp[v * D + o];
    out[p * out_stride + o] = acc;
  }
}

}  // namespace

// Closed-form Jacobians of 1- and 2-layer models (closedform.h): no planes over all N nodes, no GEMM with K = N.
// One workgroup row per sample: the entries Ts / Tn [H x (in_0 + 1)] are built once from the ~15 neighbours and every class row
// of J is a row scaling of them -- the kernel is bound by writing J (M * C * P floats, like the reference's).
__global__ __launch_bounds__(256) void jac_closed_form_kernel(const int64_t* __restrict__ idx, LGNN_CF_PARAMS,
                                                              float* __restrict__ J, int* __restrict__ bad) {
  const ClosedForm cf = LGNN_CF_VIEW;
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  const int64_t C = cf.C, P = cf.P, H = cf.H, in0 = cf.in0, in_last = cf.in_last;
  float* __restrict__ Jm = J + m * C * P;
  const int64_t t0 = int64_t(blockIdx.y) * blockDim.x + threadIdx.x, tstep = int64_t(gridDim.y) * blockDim.x;
  if (a < 0 || a >= cf.N) {
    if (t0 == 0) bad[1] = 1;
    for (int64_t t = t0; t < C * P; t += tstep) Jm[t] = 0.f;
    return;
  }
  // last layer: row c of J holds phi_a in its own block, zeros in the other classes' blocks, s_a at its bias entry
  for (int64_t t = t0; t < C * (C * in_last + C); t += tstep) {
    const int64_t c = t / (C * in_last + C), q = t - c * (C * in_last + C);
    float v = 0.f;
    if (q < C * in_last) { if (q / in_last == c) v = feat_at(cf.PhiL, a, q - c * in_last); }
    else if (q - C * in_last == c) v = feat_at(cf.PhiL, a, in_last);
    Jm[c * P + cf.off_last + q] = v;
  }
  if (cf.L == 1) return;
  // first layer: element (h, i) with i <= in0 (i == in0: the bias entry of unit h)
  const int32_t ps = cf.rowptr[a], pe = cf.rowptr[a + 1];
  const int64_t in1 = in0 + 1;
  for (int64_t t = t0; t < H * in1; t += tstep) {
    const int64_t hh = t / in1, i = t - hh * in1;
    const float tn = cf_neigh(cf, ps, pe, hh, i);
    float ts = 0.f;
    if (cf.sage) ts = cf_self(cf, a, hh, i);
    const int64_t dst = i < in0 ? hh * in0 + i : H * in0 + hh;
    for (int64_t c = 0; c < C; ++c) Jm[c * P + dst] = cf_class_row(cf, c, hh, ts, tn);
  }
}

static int jacobians_closed_form(lgnn_ctx* h, const int64_t* idx, int64_t M, float* J, float* f_out, hipStream_t s) {
  LGNN_CALL(forward_ensure_aux(h, s));
  ClosedForm cf;
  LGNN_CALL(closed_form_view(h, cf));
  int* bad = h->ws.flags.as<int>();
  if (f_out) LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), cf.C, cf.N, idx, M, cf.C, f_out, bad + 2, s));
  LGNN_REQUIRE(M < (int64_t(1) << 31), "too many samples");
  // enough workgroups per sample to fill the chip at small M
  const unsigned per = unsigned(std::max<int64_t>(1, std::min<int64_t>(cdiv(std::max<int64_t>(cf.H * (cf.in0 + 1), cf.C * (cf.C * cf.in_last + cf.C)), 256), cdiv(2048, M))));
  hipLaunchKernelGGL(jac_closed_form_kernel, dim3(unsigned(M), per), dim3(256), 0, s, idx, LGNN_CF_ARGS(cf), J, bad);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int jacobians(lgnn_ctx* h, const int64_t* idx, int64_t M, float* J, float* f_out, hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  // 1- and 2-layer models: closed form (LGNN_JAC_PLANES=1 forces the generic plane route, which deeper models use)
  const bool force_planes = getenv("LGNN_JAC_PLANES") != nullptr;
  // (models with res / norm have no closed form: the norm's row-local backward sits between the layers)
  if (closed_form_model(h) && !force_planes) return jacobians_closed_form(h, idx, M, J, f_out, s);
  LGNN_CALL(forward_ensure(h, s));
  const int64_t N = h->N;
  const int L = h->L;
  const int64_t C = h->dims[L];
  const bool gcn = h->kind == LGNN_KIND_GCN;
  int64_t off_w[kMaxLayers], off_b[kMaxLayers], off_rw[kMaxLayers], off_rb[kMaxLayers], P = 0;
  for (int l = 0; l < L; ++l) {
    off_w[l] = P; P += h->dims[l + 1] * h->in_dim[l];
    off_b[l] = P; P += h->dims[l + 1];
  }
  for (int l = 0; h->has_res && l < L - 1; ++l) {  // res.{l}.weight|bias follow all convs.* (named_parameters order)
    off_rw[l] = P; P += h->dims[l + 1] * h->dims[l];
    off_rb[l] = P; P += h->dims[l + 1];
  }
  LGNN_REQUIRE(P == h->n_params, "internal: parameter count");
  int* bad = h->ws.flags.as<int>();
  if (f_out)
    LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), C, N, idx, M, C, f_out, bad + 2, s));

  int64_t maxw = C;
  for (int l = 1; l < L; ++l) maxw = std::max(maxw, h->in_dim[l]);  // d (GCN) or 2 d (GraphSAGE) of the hidden layers
  const int64_t per_sample = C * N * maxw * 4 * 2;                   // two plane buffers
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / std::max<int64_t>(per_sample, 1)));
  LGNN_REQUIRE(chunk * C < (int64_t(1) << 31) && N < (int64_t(1) << 31), "jacobians: chunk too large");
  LGNN_CALL(h->ws.planes_a.reserve(size_t(chunk) * C * N * maxw * 4));
  LGNN_CALL(h->ws.planes_b.reserve(size_t(chunk) * C * N * maxw * 4));
  rocblas_handle blas = static_cast<rocblas_handle>(blas_handle(s));
  LGNN_REQUIRE(blas != nullptr, "rocBLAS handle");
  const float one = 1.f, zero = 0.f;
  const bool gcn_res = gcn && h->has_res;
  if (gcn_res && L > 2) LGNN_CALL(h->ws.planes_c.reserve(size_t(chunk) * C * N * maxw * 4));
  // d f / d res.{l} = u_l^T h_l, column sums of u_l (u_l = gradient at s_l; GraphSAGE: u_l = g_l)
  auto res_block = [&](int l, const float* u, float* Jc, int64_t planes) -> int {
    const int64_t dout = h->dims[l + 1], din = h->dims[l];
    const rocblas_status st = rocblas_sgemm_strided_batched(
        blas, rocblas_operation_none, rocblas_operation_transpose, rocblas_int(din), rocblas_int(dout), rocblas_int(N), &one,
        h->fc.lin_in_p[l], rocblas_int(h->fc.lin_in_ld[l]), 0, u, rocblas_int(dout), rocblas_stride(N * dout), &zero,
        Jc + off_rw[l], rocblas_int(din), rocblas_stride(P), rocblas_int(planes));
    if (st != rocblas_status_success) { set_error("rocblas_sgemm_strided_batched failed"); return 3; }
    hipLaunchKernelGGL(plane_colsum_kernel, dim3(unsigned(planes)), dim3(256), 0, s, u, N, dout, Jc + off_rb[l], P);
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  };
  h->ws.planes_a_zero_ptr = nullptr;  // (the GraphSAGE KFAC path keeps an invariant on this buffer)

  for (int64_t m0 = 0; m0 < M; m0 += chunk) {
    const int64_t mc = std::min(chunk, M - m0);
    const int64_t planes = mc * C;
    float* g = h->ws.planes_a.as<float>();      // g_l, width dims[l+1]
    float* other = h->ws.planes_b.as<float>();  // GEMM output
    float* Jc = J + m0 * C * P;
    LGNN_HIP_CHECK(hipMemsetAsync(g, 0, size_t(planes) * N * C * 4, s));
    if (gcn)
      hipLaunchKernelGGL(jac_top_gcn_kernel, dim3(unsigned(cdiv(mc, 4))), dim3(256), 0, s, idx + m0, mc, N, C, h->P.rowptr,
                         h->P.col, h->P.val, g, bad);
    else
      hipLaunchKernelGGL(jac_top_sage_kernel, dim3(unsigned(cdiv(planes, 256))), dim3(256), 0, s, idx + m0, mc, N, C, g, bad);
    LGNN_HIP_CHECK(hipGetLastError());

    for (int l = L - 1; l >= 0; --l) {
      const int64_t dout = h->dims[l + 1], din = h->in_dim[l];
      // dW (row major [dout, din]) = g^T in_l.  Column major view: C[din, dout] = in_l^T[din, N] * g[N, dout]
      const rocblas_status st = rocblas_sgemm_strided_batched(
          blas, rocblas_operation_none, rocblas_operation_transpose, rocblas_int(din), rocblas_int(dout), rocblas_int(N),
          &one, h->fc.lin_in_p[l], rocblas_int(h->fc.lin_in_ld[l]), 0, g, rocblas_int(dout), rocblas_stride(N * dout), &zero,
          Jc + off_w[l], rocblas_int(din), rocblas_stride(P), rocblas_int(planes));
      if (st != rocblas_status_success) { set_error("rocblas_sgemm_strided_batched failed"); return 3; }
      hipLaunchKernelGGL(plane_colsum_kernel, dim3(unsigned(planes)), dim3(256), 0, s, g, N, dout, Jc + off_b[l], P);
      LGNN_HIP_CHECK(hipGetLastError());
      if (!gcn && h->has_res && l < L - 1) LGNN_CALL(res_block(l, g, Jc, planes));  // GraphSAGE: res.{l} sees g_l too
      if (l == 0) break;
      const int64_t d = h->dims[l];
      if (gcn) {
        // up = act'(h_l) * (g W_l);  g_{l-1} = P^T up      (gnn/models/layers.py:45-46 backward)
        GemmEpilogue ep;
        ep.hact = h->fc.hact_p[l - 1]; ep.hact_ld = h->fc.hact_ld[l - 1]; ep.act = h->act; ep.hact_row_mod = N;
        // res / norm (base_gnn.py:141-149 backwards): below the top level dh_l = g_l W_l + u_l Wr_l with u_l still in
        // `other`; mask and the norm's row-local backward give u_{l-1}, which res.{l-1} sees and P^T propagates
        const bool res_term = gcn_res && l < L - 1;
        if (res_term) {
          GemmEpilogue none;
          LGNN_CALL(launch_gemm(other, dout, h->Wr[l], d, h->ws.planes_c.as<float>(), d, planes * N, dout, d, none, s));
          ep = none;
        }
        LGNN_CALL(launch_gemm(g, dout, h->W[l], d, other, d, planes * N, dout, d, ep, s));
        if (res_term || h->norm != LGNN_NORM_NONE)
          LGNN_CALL(launch_resnorm_backward(h, l - 1, other, d, planes * N, res_term ? h->ws.planes_c.as<float>() : nullptr,
                                            res_term, s));
        if (gcn_res) LGNN_CALL(res_block(l - 1, other, Jc, planes));
        SpmmArgs sa{};
        sa.rowptr = h->PT.rowptr; sa.col = h->PT.col; sa.val = h->PT.val; sa.nrows = N;
        sa.in = other; sa.in_ld = d; sa.in_plane_stride = N * d;
        sa.out = g; sa.out_ld = d; sa.out_plane_stride = N * d; sa.width = d; sa.out_act = -1;
        LGNN_CALL(launch_spmm_ex(sa, planes, s));
      } else {
        // dcat = g W_l [., 2d];  g_{l-1} = act'(h_l) * (dcat[:, :d] + P^T dcat[:, d:])   (layers.py:26-29 backward)
        // (with res: W_l + [Wr_l | 0], the gradient at the Linear's output is res.{l}'s too)
        GemmEpilogue ep;
        LGNN_CALL(launch_gemm(g, dout, h->Wback(l), 2 * d, other, 2 * d, planes * N, dout, 2 * d, ep, s));
        SpmmArgs sa{};
        sa.rowptr = h->PT.rowptr; sa.col = h->PT.col; sa.val = h->PT.val; sa.nrows = N;
        sa.in = other + d; sa.in_ld = 2 * d; sa.in_plane_stride = N * 2 * d;
        sa.self = other; sa.self_ld = 2 * d; sa.self_plane_stride = N * 2 * d;
        sa.hact = h->fc.hact_p[l - 1]; sa.hact_ld = h->fc.hact_ld[l - 1]; sa.act = h->act;
        sa.out = g; sa.out_ld = d; sa.out_plane_stride = N * d; sa.width = d; sa.out_act = -1;
        LGNN_CALL(launch_spmm_ex(sa, planes, s));
        if (h->norm != LGNN_NORM_NONE) LGNN_CALL(launch_resnorm_backward(h, l - 1, g, d, planes * N, nullptr, false, s));
      }
    }
  }
  return 0;
}

// Full GGN over all weights (GGNInterface.full, laplace/curvature/curvature.py:374-410; the reference's default backend
// applies a matrix-free GGN to the P columns of the identity, curvlinops/ggn.py:44-75 via laplace/curvature/
// curvlinops.py:110-140): H = sum_n J_n^T Lambda_n J_n with Lambda_n = S_n S_n^T, S[k, c] = sqrt(p_c) (d_kc - p_k), so
// H = X^T X for the rows X[(n, c), :] = sum_k S_n[k, c] J[n, k, :] = sqrt(p_c) (J[n, c, :] - sum_k p_k J[n, k, :]) -- one
// in-place row mixing pass over a chunk of device Jacobians, then the fp32 MFMA Gram kernel (upper sub-tiles) straight
// into the caller's H.  Regression (H_lik = None): X = J.
__global__ __launch_bounds__(256) void ggn_mix_rows_kernel(float* __restrict__ J, const float* __restrict__ probs,
                                                           int64_t mc, int64_t C, int64_t P) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t m = blockIdx.y;
  if (p >= P) return;
  float* __restrict__ Jm = J + m * C * P + p;
  const float* __restrict__ pm = probs + m * C;
  float t = 0.f;
  for (int64_t k = 0; k < C; ++k) t += pm[k] * Jm[k * P];
  for (int64_t c = 0; c < C; ++c) Jm[c * P] = sqrtf(pm[c]) * (Jm[c * P] - t);
}

int full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* H_out, float* loss_out,
                    hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y && H_out && loss_out, "empty batch or null pointers");
  LGNN_REQUIRE(h->L >= 1, "no model bound");
  LGNN_CALL(forward_ensure(h, s));
  const int64_t C = h->dims[h->L], P = h->n_params;
  LGNN_REQUIRE(P * P < (int64_t(1) << 40), "full GGN: P x P does not fit");
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
  const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(M, (h->ws_limit / 4) / std::max<int64_t>(C * P * 4, 1)));
  LGNN_CALL(h->ws.jac.reserve(size_t(mc_max) * C * P * 4));
  float* J = h->ws.jac.as<float>();
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    if (h->lik != LGNN_LIK_REGRESSION) {
      hipLaunchKernelGGL(ggn_mix_rows_kernel, dim3(unsigned(cdiv(P, 256)), unsigned(mc)), dim3(256), 0, s, J,
                         h->ws.probs.as<float>() + m0 * C, mc, C, P);
      LGNN_HIP_CHECK(hipGetLastError());
    }
    LGNN_CALL(launch_gram(J, P, mc * C, P, H_out, s));
  }
  LGNN_CALL(launch_symmetrize_upper(H_out, P, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn

extern "C" int lgnn_jacobians(lgnn_ctx* h, const int64_t* idx, int64_t M, float* J, float* f_out, void* stream) {
  if (!h || (M > 0 && (!idx || !J))) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0) return 0;
  return lgnn::jacobians(h, idx, M, J, f_out, static_cast<hipStream_t>(stream));
}
