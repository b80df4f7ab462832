// Last-layer full GGN of one mini-batch as weighted Grams over class pairs, and the last layer's feature rows.
//
// Reference: last_layer_jacobians (laplace/curvature/curvature.py:132-167) gives J_n = [I_C (x) phi_n^T | s_n I_C]; GGNInterface.full
// (:374-410) contracts it with Lambda_n = diag(p_n) - p_n p_n^T (:365-372):
//   H = sum_n Lambda_n (x) phi~_n phi~_n^T,  phi~_n = [phi_n | s_n]     (GCN: phi_n = (P h)[n], s_n = rowsum(P)[n]; GraphSAGE: cat[n], 1)
// Block (c, c') of H is the Gram of the batch's feature rows weighted by Lambda[:, c, c'].  The driver builds the rows once
// (ll_build_phi_kernel), the row scales of a chunk of pairs (ll_pair_weights_kernel), runs the batched fp32 MFMA Gram of
// kernels.hip over the D feature columns and one rocBLAS GEMM for the bias column, and keeps the result pair major: S [Q][D][D],
// Sb [Q][D + 1], Q = C (C + 1) / 2.  A fit accumulates every batch there and places the pairs into H once.
#include <rocblas/rocblas.h>

#include "closedform.h"
#include "device_utils.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// ---- last-layer full GGN as weighted Grams over class pairs -----------------------------------------------------
// H = sum_n Lambda_n (x) phi~_n phi~_n^T: block (c, c') of H is the weighted Gram Phi~^T diag(Lambda[:, c, c']) Phi~ -- symmetric
// in (c, c') AND inside the block.  Only the pairs c <= c' and the upper half of every block are computed (a quarter
// of the P x P products; the formulation through Z^T Z, Z = [p_c phi~], computed half).
// pair index q <-> (c, c'), c <= c', row major
__device__ __forceinline__ void pair_of(int64_t q, int64_t C, int64_t& c, int64_t& c2) {
  c = 0;
  while (q >= C - c) { q -= C - c; ++c; }
  c2 = c + q;
}
// Phi[m][j] = phi~ of batch row m (j < D features, j == D bias scale), zero padded to ldp
__global__ void ll_build_phi_kernel(const int64_t* __restrict__ idx, int64_t M, FeatView Phi, int64_t ldp,
                                    float* __restrict__ out) {
  const int64_t total = M * ldp;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t m = t / ldp, j = t - m * ldp;
    out[t] = j <= Phi.width ? feat(Phi, idx[m], j) : 0.f;
  }
}
// w = Lambda[m, c, c'] = [c == c'] p_c - p_c p_c'.  rs[q][m] = sqrt|w| (row scale of the Gram), ws[q][m] = w * s_m (signed,
// times the bias scale of the row: the bias column of a block is sum_m w s_m phi~_m), zsign[q] = +1 (c == c') / -1
__global__ void ll_pair_weights_kernel(const float* __restrict__ probs, const int64_t* __restrict__ idx, FeatView Phi,
                                       int64_t M, int64_t C, int64_t q0, float* __restrict__ rs, float* __restrict__ ws,
                                       float* __restrict__ zsign) {
  const int64_t q = blockIdx.y;  // index inside the chunk of pairs that starts at q0
  int64_t c, c2;
  pair_of(q0 + q, C, c, c2);
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; m < M; m += stride) {
    const float pc = probs[m * C + c], pc2 = probs[m * C + c2];
    const float w = (c == c2 ? pc : 0.f) - pc * pc2;
    rs[q * M + m] = sqrtf(fabsf(w));
    ws[q * M + m] = w * feat(Phi, idx[m], Phi.width);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) zsign[q] = c == c2 ? 1.f : -1.f;
}
// S[q] [D x D] (upper 32 x 32 sub-tiles valid) and Sb[q] [D + 1] (bias column) -> upper triangle of H.
// H index of (class c, column a): a < D -> c * D + a, a == D (bias) -> C * D + c.
// One workgroup per (32 x 32 tile (ti <= tj) of the block, pair): the tile goes through LDS so that the block's (ti, tj)
// part and -- for c < c' or an off-diagonal tile -- its mirror image (tj, ti) are both written with coalesced rows.
__global__ __launch_bounds__(256) void ll_place_tiles_kernel(const float* __restrict__ S, int64_t D, int64_t C, int64_t q0,
                                                             float* __restrict__ Hout) {
  __shared__ float t[32][33];
  const int64_t P = C * D + C;
  int64_t c, c2;
  pair_of(q0 + blockIdx.z, C, c, c2);
  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;
  const float* __restrict__ Sq = S + int64_t(blockIdx.z) * D * D;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int64_t i = ti * 32 + r, j = tj * 32 + tx;
    t[r][tx] = (i < D && j < D) ? Sq[i * D + j] : 0.f;
  }
  __syncthreads();
  // block element (i, j) -> H[c D + i][c2 D + j]   (c <= c2: always in the upper triangle for c < c2; for c == c2 keep i <= j)
  for (int r = ty; r < 32; r += 8) {
    const int64_t i = ti * 32 + r, j = tj * 32 + tx;
    if (i < D && j < D && (c < c2 || i <= j)) Hout[(c * D + i) * P + c2 * D + j] += t[r][tx];
  }
  if (ti < tj && c < c2) {  // the block is symmetric: element (j, i) of it equals (i, j); rows j of H, coalesced over i
    for (int r = ty; r < 32; r += 8) {
      const int64_t j = tj * 32 + r, i = ti * 32 + tx;
      if (i < D && j < D) Hout[(c * D + j) * P + c2 * D + i] += t[tx][r];
    }
  }
}
// bias column of every block: H[(c, a)][(bias c2)] and H[(c2, a)][(bias c)] for a < D, H[bias c][bias c2]
__global__ void ll_place_bias_kernel(const float* __restrict__ Sb, int64_t D, int64_t C, int64_t q0, int64_t nq,
                                     float* __restrict__ Hout) {
  const int64_t D1 = D + 1, P = C * D + C;
  const int64_t total = nq * D1;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t tq = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; tq < total; tq += stride) {
    const int64_t q = tq / D1, a = tq - q * D1;
    int64_t c, c2;
    pair_of(q0 + q, C, c, c2);
    const float v = Sb[tq];
    if (a == D) { Hout[(C * D + c) * P + C * D + c2] += v; continue; }  // (bias c, bias c2), c <= c2
    Hout[(c * D + a) * P + C * D + c2] += v;                            // ((c, a), bias c2): row < column always
    if (c != c2) Hout[(c2 * D + a) * P + C * D + c] += v;               // ((c2, a), bias c)
  }
}

// row major Sb[Q, D1] = Wq[Q, M] * Phi[M, D1] (ld ldp) + beta Sb: the bias column of the pair Grams
int ll_bias_gemm(const float* Wq, const float* Phi, float* Sb, int64_t Q, int64_t M, int64_t D1, int64_t ldp,
                 hipStream_t s, float beta) {
  rocblas_handle blas = static_cast<rocblas_handle>(blas_handle(s));
  LGNN_REQUIRE(blas != nullptr, "rocBLAS handle");
  const float one = 1.f, zero = beta;
  // column-major view: C^T[D1, Q] = B^T[D1, M] * A^T[M, Q]
  const rocblas_status st = rocblas_sgemm(blas, rocblas_operation_none, rocblas_operation_none, rocblas_int(D1),
                                          rocblas_int(Q), rocblas_int(M), &one, Phi, rocblas_int(ldp), Wq, rocblas_int(M),
                                          &zero, Sb, rocblas_int(D1));
  if (st != rocblas_status_success) { set_error("rocblas_sgemm failed"); return 3; }
  return 0;
}

}  // namespace

int launch_ll_build_phi(const int64_t* idx, int64_t M, const FeatView& Phi, int64_t ldp, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ll_build_phi_kernel, dim3(unsigned(std::min<int64_t>(cdiv(M * ldp, 256), 8192))), dim3(256), 0, s, idx, M,
                     Phi, ldp, out);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// phi~ of the batch rows: out [M, D + 1] = [last layer's input features at the node | bias scale]
// (last_layer_jacobians, laplace/curvature/curvature.py:132-167: J_n = [I_C (x) phi_n^T | s_n I_C])
int lastlayer_features(lgnn_ctx* h, const int64_t* idx, int64_t M, float* out, float* f_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && out, "empty batch or null pointers");
  LGNN_CALL(forward_ensure_aux(h, s));
  FeatView Phi;
  feat_views(h, h->L - 1, Phi);
  const int64_t D1 = Phi.width + 1;
  LGNN_CALL(launch_ll_build_phi(idx, M, Phi, D1, out, s));
  if (f_out)
    LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), h->dims[h->L], h->N, idx, M, h->dims[h->L], f_out,
                                 h->ws.flags.as<int>() + 2, s));
  return 0;
}

// Pair-major accumulation: S [Q][D][D] (upper sub-tiles of each block) and Sb [Q][D + 1] are the CALLER's buffers and are
// added to -- a fit accumulates all its batches there and places them into H once (lastlayer_pairs_place), instead of one
// placement (1.2 GB of read-modify-write) + mirror pass per batch; a data-parallel caller all-reduces the pair buffers,
// half the bytes of H.
int lastlayer_pairs_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* S, float* Sb,
                               float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y && S && Sb && loss_out, "empty batch or null pointers");
  LGNN_REQUIRE(h->lik == LGNN_LIK_CLASSIFICATION, "last-layer full GGN kernels: classification likelihood");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int L = h->L;
  const int64_t C = h->dims[L];
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
  const float* probs = h->ws.probs.as<float>();
  FeatView Phi;
  feat_views(h, L - 1, Phi);
  const int64_t D = Phi.width, D1 = D + 1;
  const int64_t Q = C * (C + 1) / 2, ldp = cdiv(D1, 4) * 4;
  // chunks of pairs: the row-scale / weight vectors [qc][M] live in the workspace
  const int64_t per_pair = (2 * M + 1) * 4;
  const int64_t qc_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(Q, 32768), h->ws_limit / per_pair));
  LGNN_CALL(h->ws.planes_a.reserve(size_t(M) * ldp * 4 + size_t(qc_max) * (2 * M + 1) * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* PhiM = h->ws.planes_a.as<float>();
  float* rs = PhiM + M * ldp;
  float* wsg = rs + qc_max * M;
  float* zsign = wsg + qc_max * M;
  LGNN_CALL(launch_ll_build_phi(idx, M, Phi, ldp, PhiM, s));
  for (int64_t q0 = 0; q0 < Q; q0 += qc_max) {
    const int64_t qc = std::min(qc_max, Q - q0);
    hipLaunchKernelGGL(ll_pair_weights_kernel, dim3(unsigned(std::min<int64_t>(cdiv(M, 256), 64)), unsigned(qc)),
                       dim3(256), 0, s, probs, idx, Phi, M, C, q0, rs, wsg, zsign);
    LGNN_HIP_CHECK(hipGetLastError());
    // S[q] += sign_q * (diag(rs_q) Phi)^T (diag(rs_q) Phi) over the D feature columns
    if (h->timing) LGNN_CALL(record_event(h, s));  // dominant kernel of the last-layer path (bench.py roofline)
    LGNN_CALL(launch_gram_batched(PhiM, ldp, M, D, S + q0 * D * D, D * D, qc, rs, zsign, 1.0f, s));
    if (h->timing) { LGNN_CALL(record_event(h, s)); h->ev_planes += qc; }
    // bias column: Sb[q][j] += sum_m w_qm s_m phi~[m][j], one library GEMM [qc x M] * [M x D1]
    LGNN_CALL(ll_bias_gemm(wsg, PhiM, Sb + q0 * D1, qc, M, D1, ldp, s, 1.0f));
  }
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

// H_out [P, P] += the blocks of the pair-major accumulators (upper triangle), then the mirror pass
int lastlayer_pairs_place(lgnn_ctx* h, const float* S, const float* Sb, float* H_out, hipStream_t s) {
  LGNN_REQUIRE(S && Sb && H_out && h->L > 0, "null pointers / no model bound");
  const int64_t C = h->dims[h->L], D = h->in_dim[h->L - 1], P = C * D + C;
  const int64_t Q = C * (C + 1) / 2;
  const unsigned nt = unsigned(cdiv(D, 32));
  for (int64_t q0 = 0; q0 < Q; q0 += 32768) {
    const int64_t qc = std::min<int64_t>(32768, Q - q0);
    hipLaunchKernelGGL(ll_place_tiles_kernel, dim3(nt, nt, unsigned(qc)), dim3(256), 0, s, S + q0 * D * D, D, C, q0, H_out);
  }
  hipLaunchKernelGGL(ll_place_bias_kernel, dim3(unsigned(std::min<int64_t>(cdiv(Q * (D + 1), 256), 4096))), dim3(256), 0, s,
                     Sb, D, C, int64_t(0), Q, H_out);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(launch_symmetrize_upper(H_out, P, s));
  return 0;
}

// One batch straight into H (the entry point of the first round): pair buffers from the workspace, zeroed, accumulated,
// placed and mirrored in this call.
int lastlayer_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* H_out,
                              float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && y && H_out && loss_out, "empty batch or null pointers");
  LGNN_REQUIRE(h->L > 0, "no model bound");
  const int64_t C = h->dims[h->L], D = h->in_dim[h->L - 1], D1 = D + 1, Q = C * (C + 1) / 2;
  LGNN_CALL(h->ws.planes_b.reserve(size_t(Q) * (D * D + D1) * 4));
  float* S = h->ws.planes_b.as<float>();
  float* Sb = S + Q * D * D;
  LGNN_HIP_CHECK(hipMemsetAsync(S, 0, size_t(Q) * (D * D + D1) * 4, s));
  LGNN_CALL(lastlayer_pairs_accumulate(h, idx, y, M, S, Sb, loss_out, s));
  return lastlayer_pairs_place(h, S, Sb, H_out, s);
}

}  // namespace lgnn
