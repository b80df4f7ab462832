// What the translation units of the adjacency gradient share -- adjgrad.hip (shared kernels, finish, dispatchers, C entry points),
// adjgrad_gcn.hip / adjgrad_sage.hip / adjgrad_ext.hip / adjgrad_onelayer.hip (one model family each: its kernels and host
// chains under every posterior), adjgrad_diag.hip (the diagonal posterior's closed form): host helpers and family entry points.
// A kernel lives in exactly one file; another file reaches it through a launcher declared here.
#pragma once
#include "lgnn_internal.h"

namespace lgnn {

// ---- adjgrad.hip: shared launchers and helpers ----------------------------------------------------------------------------------
// out[p] += sum_planes <L_c[a, :], R_c[b, :]> on the stored entries p = (a, b) of m (rows a from an optional device list) ...
int launch_sddmm(const Csr& m, int64_t nrows, const int32_t* rows, const int32_t* nrows_dev, const float* L, int64_t l_ld,
                 int64_t l_stride, const float* R, int64_t r_ld, int64_t r_stride, int64_t width, int64_t nplanes,
                 float* out, hipStream_t s);
// ... and on K candidate pairs (ca[k], cb[k]) (a_active: optional row flags, pairs with an inactive a are skipped)
int launch_sddmm_coo(const int32_t* ca, const int32_t* cb, int64_t K, const float* L, int64_t l_ld, int64_t l_stride,
                     const float* R, int64_t r_ld, int64_t r_stride, int64_t width, int64_t nplanes, const uint8_t* a_active,
                     float* out, hipStream_t s);
// The Kronecker chains' top layer (C = dims[L] classes): g [C][N][C] = P^T scatter(seeds) and the flags ws.active of its rows
int launch_seed_planes(lgnn_ctx* h, float* g, hipStream_t s);
// gradP (stored entries; skipped when null) and grad_cand (K pairs) += <seeds of a batch row a, g1bar[b]>, classes [c0, c0 + cc)
int launch_seed_sddmm(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* g1bar, int64_t c0, int64_t cc, float* grad_P,
                      const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s);
// Vbar[m][c0 + c][:] = (P g1bar_c)[idx[m]]
int launch_seed_gather(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* g1bar, int64_t c0, int64_t cc, float* vbar,
                       hipStream_t s);
// out_bar[idx[m]] += d/df <Vbar_m, V(f)> (fork_exact) + loss_scale (softmax - onehot): the end of every Kronecker batch chain
int launch_seed_adjoint(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* vbar, bool fork_exact,
                        float loss_scale, float* out_bar, hipStream_t s);
// out[(i, j)] = (gA[(i, j)] + gA[(j, i)]) / 2 on a symmetric stored pattern
int launch_adj_grad_symmetrize(const Csr& a, const float* gA, int64_t N, float* out, hipStream_t s);
// gradP[p] += c[a * ld] for every stored entry p of row a;  grad_cand[k] += c[cand_a[k] * ld]
int launch_row_const(lgnn_ctx* h, const float* c, int64_t ld, float* grad_P, const int32_t* cand_a, int64_t K, float* grad_cand,
                     hipStream_t s);
int normalize_adj_backward(lgnn_ctx* h, const float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b,
                           int64_t K, const float* grad_cand, float* grad_cand_adj, hipStream_t s);
int check_model(const lgnn_ctx* h);  // plain 2-layer models

// ---- adjgrad_gcn.hip: plain 2-layer GCN, Kronecker posterior (after the batch prologue; dense: lgnn_kfac_adjgrad_batch_dense) ----
int kfac_adjgrad_batch_gcn(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool fork_exact, const float* gamma_B0,
                           const float* gamma_B1, float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a,
                           const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s, float* dense);

// ---- adjgrad_diag.hip: plain 2-layer GCN, diagonal posterior (closed form) --------------------------------------------------------
// band1 > band0: the per-sample all-pairs term alone, into dense = the rows [band0, band1) of the grid (adjband.hip)
int diag_adjgrad_batch_gcn(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, float loss_scale,
                           float* grad_P, float* out_bar, float* h1_bar, float* e_bar, const int32_t* cand_a,
                           const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s, float* dense, int64_t band0 = 0,
                           int64_t band1 = 0, bool det = false);  // det: the fixed-order kernels (lgnn_diag_adjgrad_band_sparse)

// ---- adjgrad_sage.hip: plain 2-layer GraphSAGE ------------------------------------------------------------------------------------
int sage_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool fork_exact, const float* gamma_B0,
                       const float* gamma_B1, float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a,
                       const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s);
int sage_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* gamma_A0, const float* gamma_A1, float a_scale,
                        float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b, int64_t K,
                        float* grad_cand, float* grad_cand_adj, hipStream_t s, const float* h1_bar = nullptr,
                        const float* px_bar = nullptr, int64_t px_ld = 0);
// per-sample chain under the diagonal (gamma [P]) or the full (Gamma [P, P]) posterior: exactly one of the two is given
int persample_adjgrad_batch_sage(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                 const float* Gamma, float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                                 const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s);

// ---- adjgrad_ext.hip: 2-layer GCN with res / norm; the per-sample planes chain (also the full posterior of plain GCNs) ----------
int check_model_ext(const lgnn_ctx* h);
int sgemm_rm_nt_shared(hipStream_t s, int64_t R, int64_t Nout, int64_t K, const float* A, int64_t lda, const float* B,
                       int64_t strideB, float beta, float* Cm, int64_t strideC, int64_t batch);
int chunk_directions(lgnn_ctx* h, const int64_t* idx, const int64_t* y, int64_t mc, const float* J, const float* gamma,
                     const float* Gamma, float loss_scale, float* probs, float* Kn, float* R, float* out_bar, hipStream_t s);
int kfac_adjgrad_batch_ext(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool fork_exact, const float* gamma_B0,
                           const float* gamma_B1, const float* gamma_Br, float loss_scale, float* grad_P, float* out_bar,
                           const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s);
int persample_adjgrad_batch_ext(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, const float* Gamma,
                                float loss_scale, float* grad_P, float* out_bar, float* h1_bar, const int32_t* cand_a,
                                const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s);

// ---- adjgrad_onelayer.hip: 1-layer GCN -----------------------------------------------------------------------------------------
int check_model_onelayer(const lgnn_ctx* h);
int onelayer_kfac_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags, const float* gamma_B,
                                float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a, const int32_t* cand_b,
                                int64_t K, float* grad_cand, hipStream_t s);
int onelayer_diag_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, float loss_scale,
                                float* out_bar, float* e_bar, hipStream_t s);
int onelayer_full_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* Gamma, float loss_scale,
                                float* out_bar, float* e_bar, hipStream_t s);
int onelayer_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* e_bar, float* grad_P, float* grad_adj,
                            const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, float* grad_cand_adj,
                            hipStream_t s);

}  // namespace lgnn
