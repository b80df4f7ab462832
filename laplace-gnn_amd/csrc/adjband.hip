// Row bands of the all-pairs adjacency gradient under the diagonal posterior (DiagLaplace.propose_edges): the dense route of
// lora.hip without its [N, N] buffer.  Row a of d(-marglik)/dP on the full grid is the sum of
//   * the per-sample all-pairs term of the samples whose node is a (dense_diag_pair_kernel, lora.hip), and
//   * three bilinear terms over whole-graph adjoints (adjgrad_finish's dense forms, adjgrad.hip):
//       <out_bar[a], Z1[b]> + <Hb[a], Z0[b]> + <e_bar[a, :F], X[b]> + e_bar[a, F],
// so the rows [a0, a1) need the samples of the band and the band's rows of three tile GEMMs -- every sample is visited once
// over all bands.  Entry (a, b) of P = D A^T D is the pair (i = b, j = a) of the adjacency: a band holds d/d adj[i, j] for
// j in [a0, a1) and every i once normalize_adj backward has run on it (band_adj_kernel: dense_adj_finish_kernel's formula
// without the pairing of transposed tiles, which a directed model does not need).
//
// Four calls: lgnn_diag_adjgrad_band_sparse per batch (the sparse pass of lgnn_diag_adjgrad_batch with fixed-order sums),
// lgnn_diag_adjgrad_band_prepare once (Z1, Z0, Hb, the stored-entry gradient completed and the row / column sums behind rt_i),
// then per band lgnn_diag_adjgrad_band_batch and lgnn_diag_adjgrad_band_finish.  One
// writer per element throughout: no float atomics touch the band.
#include "adjgrad.h"
#include "device_utils.h"

namespace lgnn {

namespace {

// Hb = act'(h_1) * (Hb + h1_bar): the first layer's pre-activation adjoint (ReLU: the mask of H_1 > 0)
__global__ void band_hb_kernel(float* __restrict__ hb, const float* __restrict__ h1_bar, const float* __restrict__ h1, int64_t H,
                               int64_t ldh, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride) {
    const int64_t v = q / H, j = q - v * H;
    hb[q] = h1[v * ldh + j] > 0.f ? hb[q] + h1_bar[q] : 0.f;
  }
}

// band[t, i] = d/dP[a0 + t, i]  ->  d/d adj[i, j = a0 + t] = G d_i d_j + rt_i,  rt_i = -1/2 d_i^2 (rs_i + cs_i),
// d = rowsum(A_hat)^-1/2 (the arithmetic of dense_adj_finish_kernel); the diagonal leaves as +inf (never a proposal).
__global__ __launch_bounds__(256) void band_adj_kernel(float* __restrict__ band, int64_t N, int64_t a0, int64_t rows,
                                                       const int32_t* __restrict__ a_rowptr, const float* __restrict__ rs,
                                                       const float* __restrict__ cs) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float di = rsqrtf(float(a_rowptr[i + 1] - a_rowptr[i]));
  const float rti = -0.5f * di * di * (rs[i] + cs[i]);
  for (int64_t t = int64_t(blockIdx.y); t < rows; t += gridDim.y) {
    const int64_t j = a0 + t;
    const float dj = rsqrtf(float(a_rowptr[j + 1] - a_rowptr[j]));
    float* __restrict__ g = band + t * N + i;
    *g = i == j ? INFINITY : fmaf(*g, di * dj, rti);
  }
}

// the stored entries leave as +inf: row a = j of P's pattern lists the i with (i, j) stored in the adjacency.  One wave per row.
__global__ __launch_bounds__(256) void band_mask_kernel(float* __restrict__ band, int64_t N, int64_t a0, int64_t rows,
                                                        const int32_t* __restrict__ p_rowptr, const int32_t* __restrict__ p_col) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (t >= rows) return;
  for (int32_t p = p_rowptr[a0 + t] + lane; p < p_rowptr[a0 + t + 1]; p += 64) band[t * N + p_col[p]] = INFINITY;
}

// rs[v] = sum_b gP[v, b] P[v, b] and cs[v] = sum_a gP[a, v] P[a, v] on the stored entries (gp_rowcol_kernel's sums, adjgrad.hip,
// without its float atomics: the column sum walks row v of P^T and finds each entry in its row of P; sorted columns).  One
// wave per node, a fixed reduction order: the same bits on every run.
__global__ __launch_bounds__(256) void band_rowcol_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ val, const int32_t* __restrict__ t_rowptr,
                                                          const int32_t* __restrict__ t_col, const float* __restrict__ gP, int64_t N,
                                                          float* __restrict__ rs, float* __restrict__ cs) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (v >= N) return;
  float r = 0.f, c = 0.f;
  for (int32_t p = rowptr[v] + lane; p < rowptr[v + 1]; p += 64) r = fmaf(gP[p], val[p], r);
  for (int32_t q = t_rowptr[v] + lane; q < t_rowptr[v + 1]; q += 64) {
    const int64_t a = t_col[q];
    int32_t lo = rowptr[a], hi = rowptr[a + 1];
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (col[mid] < int32_t(v)) lo = mid + 1;
      else hi = mid;
    }
    if (lo < rowptr[a + 1] && col[lo] == int32_t(v)) c = fmaf(gP[lo], val[lo], c);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    r += __shfl_xor(r, o);
    c += __shfl_xor(c, o);
  }
  if (lane == 0) {
    rs[v] = r;
    cs[v] = c;
  }
}

int band_scope(const lgnn_ctx* h, const char* what) {
  if (h->kind != LGNN_KIND_GCN || h->L != 2 || h->extras() || h->sym) {
    set_error(std::string(what) + ": row bands cover plain directed 2-layer GCN models (no res / norm, symmetric=False)");
    return 2;
  }
  return check_model(h);  // ReLU, classification
}

}  // namespace

int diag_adjgrad_band_prepare(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar, float* grad_P, float* Hb, float* Z0,
                              float* Z1, float* rs, float* cs, hipStream_t s) {
  LGNN_CALL(band_scope(h, "lgnn_diag_adjgrad_band_prepare"));
  LGNN_REQUIRE(out_bar && h1_bar && e_bar && grad_P && Hb && Z0 && Z1 && rs && cs, "lgnn_diag_adjgrad_band_prepare: null pointers");
  LGNN_CALL(forward_ensure(h, s));
  LGNN_CALL(ensure_wt(h, s));
  LGNN_CALL(forward_input_view(h, s));
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0], F1 = F + 1;
  LGNN_CALL(h->ws.planes_a.reserve(size_t(N) * C * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* Zb = h->ws.planes_a.as<float>();  // Z1bar = P^T out_bar [N, C]
  // (no split-K that meets in float atomics, no rocBLAS: what the bands are built from is the same bits on every run)
  GemmEpilogue eb1, plain;
  eb1.bias = h->b[1];
  eb1.no_atomics = plain.no_atomics = true;
  LGNN_CALL(launch_gemm(h->fc.hact_p[0], h->fc.hact_ld[0], h->Wt[1].as<float>(), C, Z1, C, N, H, C, eb1, s));
  LGNN_CALL(launch_spmm(h->PT, N, out_bar, C, Zb, C, C, 0, s));
  LGNN_CALL(launch_gemm(Zb, C, h->W[1], H, Hb, H, N, C, H, plain, s));
  hipLaunchKernelGGL(band_hb_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * H, 256), 4096))), dim3(256), 0, s, Hb, h1_bar,
                     h->fc.hact_p[0], H, h->fc.hact_ld[0], N * H);
  LGNN_HIP_CHECK(hipGetLastError());
  GemmEpilogue eb0;
  eb0.bias = h->b[0];
  eb0.no_atomics = true;
  LGNN_CALL(launch_gemm(h->fc.lin_in_p[0], h->fc.lin_in_ld[0], h->Wt[0].as<float>(), H, Z0, H, N, F, H, eb0, s));
  // d/dP on the stored entries, completed as adjgrad_finish completes it (one writer per entry: nplanes = 1 splits nothing)
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, out_bar, C, 0, Z1, C, 0, C, 1, grad_P, s));
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, Hb, H, 0, Z0, H, 0, H, 1, grad_P, s));
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, e_bar, F1, 0, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], 0, F, 1, grad_P, s));
  LGNN_CALL(launch_row_const(h, e_bar + F, F1, grad_P, nullptr, 0, nullptr, s));
  hipLaunchKernelGGL(band_rowcol_kernel, dim3(unsigned(cdiv(N * 64, 256))), dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.val,
                     h->PT.rowptr, h->PT.col, grad_P, N, rs, cs);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int diag_adjgrad_band_finish(lgnn_ctx* h, const float* out_bar, const float* Hb, const float* Z0, const float* Z1,
                             const float* e_bar, const float* rs, const float* cs, int64_t a0, int64_t a1, float* band,
                             hipStream_t s) {
  LGNN_CALL(band_scope(h, "lgnn_diag_adjgrad_band_finish"));
  LGNN_REQUIRE(out_bar && Hb && Z0 && Z1 && e_bar && rs && cs && band, "lgnn_diag_adjgrad_band_finish: null pointers");
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0], F1 = F + 1, rows = a1 - a0;
  LGNN_REQUIRE(a0 >= 0 && rows > 0 && a1 <= N, "lgnn_diag_adjgrad_band_finish: the band must be a non-empty row range of the graph");
  LGNN_CALL(forward_input_view(h, s));
  DenseNtArgs dn;  // the rows [a0, a1) of the dense route's three terms: the left operands start at row a0
  dn.out = band; dn.ldo = N; dn.ncols = N; dn.nrows = rows;
  dn.L = out_bar + a0 * C; dn.l_ld = C; dn.R = Z1; dn.r_ld = C; dn.width = C;
  LGNN_CALL(launch_dense_nt(dn, s));
  dn.L = Hb + a0 * H; dn.l_ld = H; dn.R = Z0; dn.r_ld = H; dn.width = H;
  LGNN_CALL(launch_dense_nt(dn, s));
  dn.L = e_bar + a0 * F1; dn.l_ld = F1; dn.R = h->fc.lin_in_p[0]; dn.r_ld = h->fc.lin_in_ld[0]; dn.width = F;
  dn.rowc = e_bar + a0 * F1 + F; dn.rowc_ld = F1;
  LGNN_CALL(launch_dense_nt(dn, s));
  hipLaunchKernelGGL(band_adj_kernel, dim3(unsigned(cdiv(N, 256)), unsigned(std::min<int64_t>(rows, 1024))), dim3(256), 0, s, band,
                     N, a0, rows, h->A.rowptr, rs, cs);
  hipLaunchKernelGGL(band_mask_kernel, dim3(unsigned(cdiv(rows * 64, 256))), dim3(256), 0, s, band, N, a0, rows, h->P.rowptr,
                     h->P.col);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn

using namespace lgnn;

extern "C" int lgnn_diag_adjgrad_band_sparse(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                             float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                                             void* stream) {
  if (!h) { set_error("null context"); return 2; }
  LGNN_CALL(band_scope(h, "lgnn_diag_adjgrad_band_sparse"));
  return diag_adjgrad_batch_gcn(h, idx, y, M, gamma, loss_scale, grad_P, out_bar, h1_bar, e_bar, nullptr, nullptr, 0, nullptr,
                                static_cast<hipStream_t>(stream), nullptr, 0, 0, true);
}

extern "C" int lgnn_diag_adjgrad_band_prepare(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar,
                                              float* grad_P, float* Hb, float* Z0, float* Z1, float* rs, float* cs, void* stream) {
  if (!h) { set_error("null context"); return 2; }
  return diag_adjgrad_band_prepare(h, out_bar, h1_bar, e_bar, grad_P, Hb, Z0, Z1, rs, cs, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_diag_adjgrad_band_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                            int64_t a0, int64_t a1, float* band, void* stream) {
  if (!h || !band) { set_error("null argument"); return 2; }
  LGNN_CALL(band_scope(h, "lgnn_diag_adjgrad_band_batch"));
  LGNN_REQUIRE(a0 >= 0 && a1 > a0 && a1 <= h->N, "lgnn_diag_adjgrad_band_batch: the band must be a non-empty row range of the graph");
  return diag_adjgrad_batch_gcn(h, idx, y, M, gamma, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                static_cast<hipStream_t>(stream), band, a0, a1);
}

extern "C" int lgnn_diag_adjgrad_band_finish(lgnn_ctx* h, const float* out_bar, const float* Hb, const float* Z0, const float* Z1,
                                             const float* e_bar, const float* rs, const float* cs, int64_t a0, int64_t a1,
                                             float* band, void* stream) {
  if (!h) { set_error("null context"); return 2; }
  return diag_adjgrad_band_finish(h, out_bar, Hb, Z0, Z1, e_bar, rs, cs, a0, a1, band, static_cast<hipStream_t>(stream));
}
