// The exact Hessian of the loss as a matrix-free block product: G += R V^T for the part the GGN leaves out.
//
// Reference: CurvlinopsHessian (laplace/curvature/curvlinops.py:182-187) hands the model to curvlinops' HessianLinearOperator
// (curvlinops/hessian.py), which multiplies by double backward, one pass over the data per block.  With the summed loss
//   H = sum_n J_n^T Lambda_n J_n + R,   R = sum_n sum_c r_nc grad^2 f_nc,
// r_n = softmax(f_n) - onehot(y_n) (regression: f_n - y_n, so that GGN + R is the interface's factor 0.5 times the Hessian of
// MSELoss(sum)), the first term is lgnn_ggn_matmat's.  This file is the second, for the models whose second derivative has a
// closed form: plain 1- and 2-layer GCN / GraphSAGE, relu or tanh.  A deeper model or one with res / norm would need second
// derivatives that chunks of Jacobian rows do not hold; it is refused.  One layer is linear in its weights: R = 0.
//
// Notation of ggnmat.hip / sampled.hip: in0 = [P X | rowsum P] or [X | P X | 1], s = in0 [W0 | b0]^T, D = act'(s), D2 = act''(s)
// (0 for ReLU, -2 tanh(s) D for tanh), S [N, C] the residual rows added at the batch's nodes, G = P^T S (GraphSAGE: [S | P^T S]
// against W1 = [W1a | W1b]).  Per direction (dW0, db0, dW1, db1):
//   dS = in0 [dW0 | db0]^T      E = D . dS      T = (G dW1) . D + (G W1) . D2 . dS
//   (RV)_W1 = G^T E             [(RV)_W0 | (RV)_b0] = T^T in0             (RV)_b1 = 0
// Only the rows with a non-zero row of G matter: the batch's needed rows (sampled.hip).  Per call:
//   S's rows [M, C] at each node's first place in the batch: one thread per node adds the rows of its samples in batch order
//     (a repeated id adds; an invalid id or label adds nothing and raises the sticky flag)                    hess_resid_kernel
//   G on the needed rows: ggn_qbar_kernel's gather over P^T's rows on one "direction", one writer per element;
//     G W1 once                                                                                               hess_gw1_kernel
// and per chunk of directions
//   E, T: first_layer_kernel<HessArgs> -- dS on the fp32 MFMA tile, G dW1 on a second accumulator of the same tile, the
//     elementwise epilogue in registers (the ReLU run reads neither h nor G W1)
//   the two outer products through ggn_tn_kernel (slab partials) and ggn_finish_kernel (added in slab order).
// Only the residual rows, G, G W1, E, T (|R| H floats per direction each), the slab partials and the output reach memory.  No
// float atomics: two calls on the same input return the same bits.  The directions go in chunks under the workspace limit.
#include "ggn_struct.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

constexpr const char* kScope = "exact Hessian: closed-form models only (plain 1- and 2-layer GCN / GraphSAGE)";

// S's row of a node, kept at the node's first place in the batch (pos, the batch prologue's): r[m][:] = sum over the samples
// m' of that node, in batch order, of softmax(f_n) - onehot(y_m') (regression: f_n - y_m').  The labels of a repeated node
// differ, so its rows are added here, by the one thread that owns the row, and the gather's multiplicity of that place is
// set to one; the later places hold zero rows.  An invalid id: a zero row (flagged by the prologue); an invalid label: that
// sample adds nothing and the sticky flag is raised.
__global__ __launch_bounds__(256) void hess_resid_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                                         const int64_t* __restrict__ idx, const void* __restrict__ y_,
                                                         int64_t M, int64_t N, int64_t C, int regression,
                                                         const int32_t* __restrict__ pos, int32_t* __restrict__ mult,
                                                         float* __restrict__ r, int* __restrict__ bad) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t n = idx[m];
  float* __restrict__ o = r + m * C;
  for (int64_t c = 0; c < C; ++c) o[c] = 0.f;
  if (n < 0 || n >= N || int64_t(pos[n]) != m) return;
  const int32_t copies = mult[m];
  int32_t seen = 0;
  for (int64_t m2 = m; m2 < M && seen < copies; ++m2) {
    if (idx[m2] != n) continue;
    ++seen;
    if (regression) {
      const float* __restrict__ yr = static_cast<const float*>(y_) + m2 * C;
      for (int64_t c = 0; c < C; ++c) o[c] += logits[n * C + c] - yr[c];
      continue;
    }
    const int64_t yy = static_cast<const int64_t*>(y_)[m2];
    if (yy < 0 || yy >= C) {
      *bad = 2;
      continue;
    }
    for (int64_t c = 0; c < C; ++c) o[c] += probs[m * C + c] - (c == yy ? 1.f : 0.f);
  }
  mult[m] = 1;
}

// GW1[t][h] = sum_cz G[t][cz] W1z[cz][h] for the listed rows, W1z[cz][h] = W1[(cz % C) * ld1 + (cz / C) * H + h]
__global__ __launch_bounds__(256) void hess_gw1_kernel(const float* __restrict__ G, const float* __restrict__ W1, int64_t ld1,
                                                       int64_t C, int64_t Cz, int64_t H, const int32_t* __restrict__ count,
                                                       float* __restrict__ out) {
  const int64_t total = int64_t(*count) * H;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t t = e / H, hh = e - t * H;
    float acc = 0.f;
    for (int64_t cz = 0; cz < Cz; ++cz) acc = fmaf(G[t * Cz + cz], W1[(cz % C) * ld1 + (cz / C) * H + hh], acc);
    out[e] = acc;
  }
}

// directions per chunk: E, T and the slab partials under half the workspace limit
int64_t hess_chunk(const lgnn_ctx* h, const StructModel& m, int64_t k) {
  const int64_t per_dir = 2 * m.rcap * m.H * 4 + int64_t(kMaxSlabs) * m.P * 4;
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(k, 32768), h->ws_limit / 2 / per_dir));
}

}  // namespace

int hessian_resid_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k, float* G,
                         hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_REQUIRE(h->L <= 2 && !h->extras() && h->X, kScope);
  LGNN_REQUIRE(k > 0 && k < 65536 && M < (int64_t(1) << 31), "block size or batch size out of range");
  if (h->L == 1) return 0;  // linear in its weights: R = 0
  LGNN_CALL(forward_ensure(h, s));
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, nullptr, s));
  StructModel m;
  LGNN_CALL(struct_prepare(h, idx, M, m, s));
  Workspace& w = h->ws;
  SampledState& sf = h->sf;
  const int64_t kc_max = hess_chunk(h, m, k);
  LGNN_CALL(w.ggn_wt.reserve(size_t(M) * m.C * 4));
  LGNN_CALL(w.hess_g.reserve(size_t(m.rcap) * m.Cz * 4));
  LGNN_CALL(w.hess_gw1.reserve(size_t(m.rcap) * m.H * 4));
  LGNN_CALL(w.hess_e.reserve(size_t(kc_max) * m.rcap * m.H * 4));
  LGNN_CALL(w.hess_t.reserve(size_t(kc_max) * m.rcap * m.H * 4));
  LGNN_CALL(w.ggn_part.reserve(size_t(kMaxSlabs) * kc_max * m.P * 4));
  float* r = w.ggn_wt.as<float>();
  float* Gr = w.hess_g.as<float>();
  float* GW1 = w.hess_gw1.as<float>();
  float* E = w.hess_e.as<float>();
  float* T = w.hess_t.as<float>();
  float* part = w.ggn_part.as<float>();
  const bool curved = h->act != LGNN_ACT_RELU;
  hipLaunchKernelGGL(hess_resid_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, w.probs.as<float>(), h->fc.out.as<float>(),
                     idx, y, M, m.N, m.C, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, w.pos.as<int32_t>(), w.mult.as<int32_t>(), r,
                     w.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(launch_ggn_qbar(h, m, r, M, 1, Gr, s));
  if (curved) {
    hipLaunchKernelGGL(hess_gw1_kernel, dim3(unsigned(std::min<int64_t>(cdiv(m.rcap * m.H, 256), 8192))), dim3(256), 0, s, Gr,
                       h->W[1], m.ld1, m.C, m.Cz, m.H, sf.count.as<int32_t>(), GW1);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  const int64_t big = int64_t(1) << 40;
  const int64_t htiles = cdiv(m.H, SBM);
  for (int64_t i0 = 0; i0 < k; i0 += kc_max) {
    const int64_t kc = std::min(kc_max, k - i0);
    const int nslab = struct_slabs(m, kc, htiles * (cdiv(m.Fp, SBM) + cdiv(m.Cz, SBM)));
    if (h->timing) LGNN_CALL(record_event(h, s));
    HessArgs a{};
    a.in0 = sf.in0.as<float>(); a.ldk = sf.ldk;
    a.rows = sf.rows.as<int32_t>(); a.count = sf.count.as<int32_t>();
    a.theta = V + i0 * m.P; a.P = m.P;
    a.Fp = m.Fp; a.H = m.H;
    a.dact = h->fc.dact0.as<float>(); a.h1 = h->fc.hact_p[0]; a.h1_ld = h->fc.hact_ld[0]; a.act = h->act;
    a.G = Gr; a.GW1 = GW1;
    a.ld1 = m.ld1; a.off1 = m.off1; a.C = m.C; a.Cz = m.Cz;
    a.E = E; a.T = T; a.rcap = m.rcap;
    LGNN_CALL(launch_first_layer(a, kc, s));
    LGNN_HIP_CHECK(hipMemsetAsync(part, 0, size_t(nslab) * kc * m.P * 4, s));
    TnArgs t{};
    t.rows = sf.rows.as<int32_t>(); t.count = sf.count.as<int32_t>();
    t.in0 = sf.in0.as<float>(); t.ldk = sf.ldk; t.Fp = m.Fp;
    t.part = part; t.P = m.P; t.kc = kc;
    t.ld1 = m.ld1; t.C = m.C; t.H = m.H;
    t.mode = 0;
    // [(RV)_W0 | (RV)_b0] = sum_t T^T in0
    t.A = T; t.a_ld = m.H; t.a_ds = m.rcap * m.H; t.acols = m.H;
    t.B = sf.in0.as<float>(); t.b_ld = sf.ldk; t.bcols = m.Fp;
    t.adim = m.H; t.ooff = 0; t.old = m.Fp; t.amod = big; t.ashift = 0; t.bias_off = m.H * m.Fp;
    t.btiles = int(cdiv(m.Fp, SBM));
    LGNN_CALL(launch_ggn_tn(t, nslab, htiles, s));
    // (RV)_W1 = sum_t G^T E: the same G for every direction, E the direction's, both listed like the rows
    t.A = Gr; t.a_ld = m.Cz; t.a_ds = 0; t.acols = m.Cz;
    t.B = E; t.b_ld = m.H; t.bcols = m.H; t.b_ds = m.rcap * m.H; t.b_listed = 1;
    t.adim = m.Cz; t.ooff = m.off1; t.old = m.ld1; t.amod = m.C; t.ashift = m.H; t.bias_off = -1;
    t.btiles = int(htiles);
    LGNN_CALL(launch_ggn_tn(t, nslab, cdiv(m.Cz, SBM), s));
    LGNN_CALL(launch_ggn_finish(part, nslab, kc * m.P, G + i0 * m.P, s));
    if (h->timing) LGNN_CALL(record_event(h, s));
  }
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn

extern "C" int lgnn_hessian_resid_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k,
                                         float* G, void* stream) {
  if (!h || (M > 0 && k > 0 && (!idx || !y || !V || !G))) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0 || k <= 0) return 0;
  return lgnn::hessian_resid_matmat(h, idx, y, M, V, k, G, static_cast<hipStream_t>(stream));
}
