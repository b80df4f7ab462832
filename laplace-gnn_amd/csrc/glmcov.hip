// Joint GLM predictive: the cross-node covariance K = J(a) P^-1 J(b)^T of the linearised model under a block-diagonal
// Kronecker or diagonal posterior, without the Jacobians where the model has a closed form.
//
// Reference: _glm_predictive_distribution(joint=True) (laplace/baselaplace.py:1123-1158) forms Js [M, C, P] by jacrev and calls
// functional_covariance -- KronLaplace :1638-1644 (posterior_precision.inv_square_form of the [1, M C, P] rows,
// laplace/utils/matrix.py inv_square_form), DiagLaplace :1905-1910, FullLaplace :1491-1494; the joint predictive itself is
// :1223-1242.  That is 2 (M C)^2 P flops after M C P floats of Jacobians and M C P (in + out) flops of rotations.
//
// Per Linear block l (weight [out, in], bias [out]; lgnn_jacobians' order, convs.* then res.*) the caller passes S[l]
// [out, in + 1] (inverse precisions, last column: the bias) and, for a Kronecker posterior, the eigenvectors QA[l] [in, in],
// QB[l] [out, out] in columns: the block of P^-1 is (Q_B (x) Q_A) diag(S) (Q_B (x) Q_A)^T; QA[l] = QB[l] = null: diag(S).
//
// Structured route (1- and 2-layer GCN / GraphSAGE without res / norm), notation of gpkernel.hip:7-11 (tables T^al_n[h, i],
// halves W^al of W_1, last layer's rows [phi_n | s_n]):
//   last layer    phit = phi Q_A1 (diagonal posterior: phi), K_i[n, m] = sum_j S1[i, j] phit_n[j] phit_m[j] + S1[i, in1] s_n s_m
//                 -- the batched NT GEMM with z = i against the b side's rows scaled by S1[i, :] -- and
//                 Cov1[(n, c), (m, e)] = sum_i Q_B1[c, i] Q_B1[e, i] K_i[n, m] (diagonal posterior: [c == e == i]);
//   first layer, diagonal posterior   stages (a) to (c) of gp_kernel_structured with the b side's tables scaled by S0[h, :];
//   first layer, Kronecker posterior  the tables rotated by [Q_A0 0; 0 1] (one NT GEMM, written z fastest),
//                 V_{n, c}[k, :] = sum_{al, h} Q_B0[h, k] W^al[c, h] T~^al_n[h, :] (one NT GEMM per sample against
//                 M [(c, k), (al, h)]), and Cov0 = <V_{n, c}, S0 . V_{m, e}> : one NT GEMM over rows (n, c), K = H (in0 + 1).
// The rows of G that hold the K_i follow the table pairs', so ONE class contraction (launch_gemm, no atomics) gives
// Kt [(c, e)][(n, m)] of both layers; the placement kernel adds Cov0 and writes the caller's layout.  One side is scaled by S,
// never both by its square root.  The chunk length mc of the index lists is the largest whose buffers -- tables, rows, V
// (2 mc C H (in0 + 1) floats), G, Kt and Cov0 (mc^2 (Zp + 2 C^2 + C)) -- stay under half the workspace limit; V is not
// slabbed over k, and a limit below one sample's buffers is a named error.
//   flops  2 (Ma C)(Mb C) H (in0 + 1)  (Cov0; dominates)  + 2 (Ma + Mb) C H Z (in0 + 1)  (V)  + 2 Ma Mb C^2 (Zp + C)  (contraction)
//   bytes  V is written once and read once per chunk pair: 4 (Ma + Mb) C H (in0 + 1) (Ma / mc); K: 4 Ma Mb C^2 written once.
//
// General route (every other model, and any model under LGNN_COV_FROM_JACOBIANS): chunks of lgnn_jacobians' rows for both
// lists; per Kronecker block both sides are rotated into the eigenbasis (two batched NT GEMMs per block: rows x Q_A, Q_B^T x
// rows, and one for the bias), the b side is scaled by S, and the NT GEMM runs with K = P.
//
// No float atomics; every element of K has one writer and a fixed summation order: two calls on the same input return the
// same bits.  With the same index pointer on both sides only the upper chunk pairs are computed, of a diagonal chunk pair's
// long-K product (Cov0, the general route's K = P) only the 128 x 128 tiles on and above the diagonal (NtProblem::upper_only;
// few such tiles: K in slabs, added in slab order), and the lower triangle is a copy of the upper.  Enqueue only: no host
// synchronisation.
#include "closedform.h"
#include "gpkernel.h"
#include "lgnn_internal.h"

#include <algorithm>

namespace lgnn {

namespace {

// QT[j * ldq + k] = Q[k, j] for j, k < n -- the NT GEMM's B operand of a product with Q -- [n][n] = 1 with aug (the bias
// entry passes through), zero elsewhere
__global__ __launch_bounds__(256) void cov_qt_kernel(const float* __restrict__ Q, int64_t n, int64_t ldq, int aug,
                                                     float* __restrict__ QT) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= ldq * ldq) return;
  const int64_t j = t / ldq, k = t - j * ldq;
  float v = 0.f;
  if (j < n && k < n) v = Q[k * n + j];
  else if (aug && j == n && k == n) v = 1.f;
  QT[t] = v;
}

// out[r * ld + q] = S[r * w + q] for q < w, zero in the pad
__global__ __launch_bounds__(256) void cov_pad_kernel(const float* __restrict__ S, int64_t rows, int64_t w, int64_t ld,
                                                      float* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= rows * ld) return;
  const int64_t r = t / ld, q = t - r * ld;
  out[t] = q < w ? S[r * w + q] : 0.f;
}

// the general route's scale of a block: sv[ow + k * in + i] = S[k, i], sv[ob + k] = S[k, in]
__global__ __launch_bounds__(256) void cov_flat_kernel(const float* __restrict__ S, int64_t out_l, int64_t in_l,
                                                       float* __restrict__ sv_w, float* __restrict__ sv_b) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= out_l * (in_l + 1)) return;
  const int64_t k = t / (in_l + 1), i = t - k * (in_l + 1);
  if (i < in_l) sv_w[k * in_l + i] = S[t];
  else sv_b[k] = S[t];
}

// out[r * ld_out + q] = in[ri * ld_in + q] * sv[((r / row_div) % sv_rows) * sv_ld + q], ri = r % in_mod (in_mod = 0: r);
// sv = null: a copy.  in == out is allowed where the rows map onto themselves (no restrict on the two).
__global__ __launch_bounds__(256) void cov_scale_rows_kernel(const float* in, int64_t ld_in, int64_t in_mod, float* out,
                                                             int64_t ld_out, int64_t R, int64_t K,
                                                             const float* __restrict__ sv, int64_t sv_ld, int64_t row_div,
                                                             int64_t sv_rows) {
  const int64_t total = R * K, stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / K, q = t - r * K;
    const int64_t ri = in_mod ? r % in_mod : r;
    const float f = sv ? sv[((r / row_div) % sv_rows) * sv_ld + q] : 1.f;
    out[r * ld_out + q] = in[ri * ld_in + q] * f;
  }
}

// M[(c * H + k) * Z + z] = Q_B0[h, k] W_1[c, z], z = al * H + h (the tables' order: [Ws | Wn])
__global__ __launch_bounds__(256) void cov_mk_kernel(const float* __restrict__ QB0, const float* __restrict__ W1, int64_t w1_ld,
                                                     int64_t H, int64_t C, int64_t Z, float* __restrict__ Mk) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= C * H * Z) return;
  const int64_t z = t % Z, ck = t / Z, k = ck % H, c = ck / H, hh = z % H;
  Mk[t] = QB0[hh * H + k] * W1[c * w1_ld + z];
}

// the last layer's columns of the class-pair matrix: Wc[(c * C + e) * ldw + col0 + i] = Q_B1[c, i] Q_B1[e, i]; QB1 = null
// (diagonal posterior): [c == e == i]
__global__ __launch_bounds__(256) void cov_qbpair_kernel(const float* __restrict__ QB1, int64_t C, float* __restrict__ Wc,
                                                         int64_t ldw, int64_t col0) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= C * C * C) return;
  const int64_t i = t % C, q = t / C, c = q / C, e = q - c * C;
  Wc[q * ldw + col0 + i] = QB1 ? QB1[c * C + i] * QB1[e * C + i] : ((c == e && e == i) ? 1.f : 0.f);
}

inline unsigned grid1(int64_t total) { return unsigned(std::max<int64_t>(1, cdiv(total, 256))); }

int launch_qt(const float* Q, int64_t n, int64_t ldq, bool aug, float* QT, hipStream_t s) {
  hipLaunchKernelGGL(cov_qt_kernel, dim3(grid1(ldq * ldq)), dim3(256), 0, s, Q, n, ldq, aug ? 1 : 0, QT);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_scale_rows(const float* in, int64_t ld_in, int64_t in_mod, float* out, int64_t ld_out, int64_t R, int64_t K,
                      const float* sv, int64_t sv_ld, int64_t row_div, int64_t sv_rows, hipStream_t s) {
  if (R <= 0 || K <= 0) return 0;
  hipLaunchKernelGGL(cov_scale_rows_kernel, dim3(unsigned(std::min<int64_t>(cdiv(R * K, 256), 65536))), dim3(256), 0, s, in, ld_in,
                     in_mod, out, ld_out, R, K, sv, sv_ld, row_div, sv_rows);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

NtProblem nt(const float* A, int64_t lda, int64_t a_bs, const float* B, int64_t ldb, int64_t b_bs, float* Out, int64_t ldo,
             int64_t o_es, int64_t o_bs, int64_t Ra, int64_t Rb, int64_t K, int64_t batch) {
  return NtProblem{A, lda, a_bs, B, ldb, b_bs, Out, ldo, o_es, o_bs, Ra, Rb, K, batch};
}

int64_t r4(int64_t n) { return cdiv(n, 4) * 4; }

struct CovOperands {
  int nb;
  const float* const* QA; const float* const* QB; const float* const* S;  // host arrays of nb device pointers
};

int cov_structured(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, const CovOperands& o, float* K,
                   int64_t ldk, hipStream_t s) {
  LGNN_CALL(forward_ensure_aux(h, s));
  GpModel g;
  LGNN_CALL(gp_model(h, g));
  const ClosedForm& cf = g.cf;
  const bool same = idx_a == idx_b && Ma == Mb, two = cf.L == 2;
  const int last = cf.L - 1;
  const bool kron0 = two && o.QA[0] != nullptr, kron1 = o.QA[last] != nullptr;
  const int64_t C = cf.C, Q = C * C, H = cf.H, Z = g.Z, ld = g.ld, ldp = g.ldp;
  const int64_t Zp = (two && !kron0) ? g.Zp : 0;  // table pairs the class contraction reads (Kronecker: the first layer is Cov0)
  const int64_t Zt = Zp + C, Kv = H * ld, Zs = std::max<int64_t>(Z, 1);
  Workspace& w = h->ws;
  StageTimer tm{h, s};

  // the call's small operands
  const int64_t o_mk = r4(Q * Zt), o_q0 = o_mk + (kron0 ? r4(C * H * Z) : 0), o_q1 = o_q0 + (kron0 ? ld * ld : 0),
                o_s0 = o_q1 + (kron1 ? ldp * ldp : 0), o_s1 = o_s0 + (two ? H * ld : 0), n_small = o_s1 + C * ldp;
  LGNN_CALL(w.cov_small.reserve(size_t(n_small) * 4));
  float* small = w.cov_small.as<float>();
  float *Wcat = small, *Mk = small + o_mk, *Q0T = small + o_q0, *Q1T = small + o_q1, *S0p = small + o_s0, *S1p = small + o_s1;
  if (Zp > 0) LGNN_CALL(launch_wpair(cf.W1, cf.w1_ld, H, C, cf.sage != 0, false, Wcat, Zt, s));
  hipLaunchKernelGGL(cov_qbpair_kernel, dim3(grid1(Q * C)), dim3(256), 0, s, kron1 ? o.QB[last] : nullptr, C, Wcat, Zt, Zp);
  LGNN_HIP_CHECK(hipGetLastError());
  if (kron0) {
    hipLaunchKernelGGL(cov_mk_kernel, dim3(grid1(C * H * Z)), dim3(256), 0, s, o.QB[0], cf.W1, cf.w1_ld, H, C, Z, Mk);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(launch_qt(o.QA[0], cf.in0, ld, true, Q0T, s));
  }
  if (kron1) LGNN_CALL(launch_qt(o.QA[last], cf.in_last, ldp, true, Q1T, s));
  if (two) {
    hipLaunchKernelGGL(cov_pad_kernel, dim3(grid1(H * ld)), dim3(256), 0, s, o.S[0], H, cf.in0 + 1, ld, S0p);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(cov_pad_kernel, dim3(grid1(C * ldp)), dim3(256), 0, s, o.S[last], C, cf.in_last + 1, ldp, S1p);
  LGNN_HIP_CHECK(hipGetLastError());

  // chunk length: everything a chunk pair holds under half the workspace limit (the other half: split-K partials)
  auto floats = [&](int64_t mc) {
    int64_t f = 2 * mc * Zs * ld + (2 + (kron1 ? 2 : 0) + C) * mc * ldp + mc * mc * (Zt + Q);
    if (kron0) f += mc * Z * ld + 2 * mc * C * Kv + mc * mc * Q;
    return f;
  };
  int64_t mc_max = std::min<int64_t>(std::max(Ma, Mb), 2048);  // (launch_gemm's grid bounds the pairs, as in gp_kernel)
  while (mc_max > 1 && floats(mc_max) * 4 > h->ws_limit / 2) mc_max = (mc_max + 1) / 2;
  // (V is not slabbed over k: one sample's buffers have to fit)
  LGNN_REQUIRE(floats(mc_max) * 4 <= h->ws_limit / 2, "lgnn_glm_covariance: the workspace limit is below one sample's buffers");
  const int64_t ca = std::min(mc_max, Ma), cb = std::min(mc_max, Mb), cm = std::max(ca, cb);
  LGNN_CALL(w.gp_tab_a.reserve(size_t(ca) * Zs * ld * 4));
  LGNN_CALL(w.gp_tab_b.reserve(size_t(cm) * Zs * ld * 4));
  LGNN_CALL(w.gp_phi_a.reserve(size_t(ca) * ldp * 4));
  LGNN_CALL(w.gp_phi_b.reserve(size_t(cb) * ldp * 4));
  if (kron1) {
    LGNN_CALL(w.cov_phit_a.reserve(size_t(ca) * ldp * 4));
    LGNN_CALL(w.cov_phit_b.reserve(size_t(cb) * ldp * 4));
  }
  LGNN_CALL(w.cov_phis.reserve(size_t(C) * cb * ldp * 4));
  LGNN_CALL(w.gp_g.reserve(size_t(ca) * cb * Zt * 4));
  LGNN_CALL(w.gp_kt.reserve(size_t(ca) * cb * Q * 4));
  if (kron0) {
    LGNN_CALL(w.cov_t2.reserve(size_t(cm) * Z * ld * 4));
    LGNN_CALL(w.cov_va.reserve(size_t(ca) * C * Kv * 4));
    LGNN_CALL(w.cov_vb.reserve(size_t(cm) * C * Kv * 4));
    LGNN_CALL(w.cov_add.reserve(size_t(ca) * cb * Q * 4));
  }
  float *Ta = w.gp_tab_a.as<float>(), *Tb = w.gp_tab_b.as<float>(), *Pa = w.gp_phi_a.as<float>(), *Pb = w.gp_phi_b.as<float>();
  float *Ra = kron1 ? w.cov_phit_a.as<float>() : Pa, *Rb = kron1 ? w.cov_phit_b.as<float>() : Pb;  // rotated [phi | s] rows
  float *PhiS = w.cov_phis.as<float>(), *G = w.gp_g.as<float>(), *Kt = w.gp_kt.as<float>();
  float *T2 = w.cov_t2.as<float>(), *Va = w.cov_va.as<float>(), *Vb = w.cov_vb.as<float>(), *Add = w.cov_add.as<float>();

  // rotated rows and V of a chunk whose tables T and rows P are built
  auto rotate = [&](int64_t mc, const float* T, const float* P, float* R, float* V) -> int {
    if (kron1) LGNN_CALL(launch_nt_gemm(h, nt(P, ldp, 0, Q1T, ldp, 0, R, ldp, 1, 0, mc, ldp, ldp, 1), s));
    if (kron0) {
      // T2[n][l'][z] = sum_l T[z][n][l] [Q_A0 0; 0 1][l, l']
      LGNN_CALL(launch_nt_gemm(h, nt(T, ld, mc * ld, Q0T, ld, 0, T2, ld * Z, Z, 1, mc, ld, ld, Z), s));
      // V[n][(c, k)][l] = sum_z M[(c, k), z] T2[n][l][z]
      LGNN_CALL(launch_nt_gemm(h, nt(Mk, Z, 0, T2, Z, ld * Z, V, ld, 1, C * Kv, C * H, ld, Z, mc), s));
    }
    return 0;
  };

  GemmEpilogue ep;
  ep.no_atomics = true;
  h->cov_chunk_pairs = 0;
  for (int64_t n0 = 0; n0 < Ma; n0 += ca) {
    const int64_t ma = std::min(ca, Ma - n0);
    bool a_built = false;
    for (int64_t m0 = same ? n0 : 0; m0 < Mb; m0 += cb) {  // same index list: upper chunk pairs only, mirrored below
      const int64_t mb = std::min(cb, Mb - m0), pairs = ma * mb;
      const bool diag = same && m0 == n0;
      ++h->cov_chunk_pairs;
      LGNN_CALL(tm.mark());  // tables
      if (!a_built) LGNN_CALL(build_tables(h, g, idx_a + n0, ma, Ta, Pa, s));
      if (!diag) LGNN_CALL(build_tables(h, g, idx_b + m0, mb, Tb, Pb, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());  // V: the rotations and the b side's scales
      if (!a_built) LGNN_CALL(rotate(ma, Ta, Pa, Ra, Va));
      a_built = true;
      if (!diag) LGNN_CALL(rotate(mb, Tb, Pb, Rb, Vb));
      if (Zp > 0) LGNN_CALL(launch_scale_rows(diag ? Ta : Tb, ld, 0, Tb, ld, Z * mb, ld, S0p, ld, mb, H, s));
      LGNN_CALL(launch_scale_rows(diag ? Ra : Rb, ldp, mb, PhiS, ldp, C * mb, ldp, S1p, ldp, mb, C, s));
      if (kron0) LGNN_CALL(launch_scale_rows(diag ? Va : Vb, Kv, 0, Vb, Kv, mb * C, Kv, S0p, 0, 1, 1, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());  // NT GEMM
      for (int64_t ab = 0; Zp > 0 && ab < (cf.sage ? 4 : 1); ++ab)
        LGNN_CALL(launch_nt_gemm(h, nt(Ta + (ab >> 1) * H * ma * ld, ld, ma * ld, Tb + (ab & 1) * H * mb * ld, ld, mb * ld,
                                       G + ab * H * pairs, mb, 1, pairs, ma, mb, cf.in0 + 1, H), s));
      LGNN_CALL(launch_nt_gemm(h, nt(Ra, ldp, 0, PhiS, ldp, mb * ldp, G + Zp * pairs, mb, 1, pairs, ma, mb,
                                     cf.in_last + 1, C), s));
      if (kron0) {  // (the diagonal chunk pair: the upper tiles only -- the mirror below writes the lower triangle)
        NtProblem p = nt(Va, Kv, 0, Vb, Kv, 0, Add, mb * C, 1, 0, ma * C, mb * C, Kv, 1);
        p.upper_only = diag ? 1 : 0;
        LGNN_CALL(launch_nt_gemm(h, p, s));
      }
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());  // class contraction
      LGNN_CALL(launch_gemm(Wcat, Zt, G, pairs, Kt, pairs, Q, Zt, pairs, ep, s));
      LGNN_CALL(tm.mark());
      LGNN_CALL(tm.mark());  // placement
      LGNN_CALL(launch_place_full(Kt, pairs, nullptr, 0, kron0 ? Add : nullptr, ma, mb, C, K + n0 * C * ldk + m0 * C, ldk, s));
      LGNN_CALL(tm.mark());
    }
  }
  if (same) LGNN_CALL(launch_mirror(K, Ma * C, ldk, 1, 0, s));
  return 0;
}

int cov_general(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, const CovOperands& o, float* K,
                int64_t ldk, hipStream_t s) {
  const bool same = idx_a == idx_b && Ma == Mb;
  const int L = h->L;
  const int64_t C = h->dims[L], P = h->n_params;
  struct Block { int64_t out, in, ow, ob, qa, qb; };  // widths, offsets in the parameter vector and in the small operands
  Block blk[2 * kMaxLayers];
  int64_t off = 0, small = r4(P), scr_row = 0;
  for (int l = 0; l < o.nb; ++l) {  // lgnn_jacobians' order: convs.{l}.weight | bias, then res.{l}.weight | bias
    Block& b = blk[l];
    b.out = l < L ? h->dims[l + 1] : h->dims[l - L + 1];
    b.in = l < L ? h->in_dim[l] : h->dims[l - L];
    b.ow = off; off += b.out * b.in;
    b.ob = off; off += b.out;
    b.qa = b.qb = 0;
    if (o.QA[l]) {
      b.qa = small; small += r4(b.in * b.in);
      b.qb = small; small += r4(b.out * b.out);
      scr_row = std::max(scr_row, b.out * b.in);
    }
  }
  LGNN_REQUIRE(off == P, "lgnn_glm_covariance: the blocks do not cover the model's parameters");
  Workspace& w = h->ws;
  LGNN_CALL(w.cov_small.reserve(size_t(small) * 4));
  float* sm = w.cov_small.as<float>();  // [sv [P] | per Kronecker block Q_A^T, Q_B^T]
  for (int l = 0; l < o.nb; ++l) {
    const Block& b = blk[l];
    hipLaunchKernelGGL(cov_flat_kernel, dim3(grid1(b.out * (b.in + 1))), dim3(256), 0, s, o.S[l], b.out, b.in, sm + b.ow, sm + b.ob);
    LGNN_HIP_CHECK(hipGetLastError());
    if (o.QA[l]) {
      LGNN_CALL(launch_qt(o.QA[l], b.in, b.in, false, sm + b.qa, s));
      LGNN_CALL(launch_qt(o.QB[l], b.out, b.out, false, sm + b.qb, s));
    }
  }
  // two chunks of Jacobian rows and the rotation's scratch under half the workspace limit (the other half is lgnn_jacobians')
  const int64_t per_sample = C * (2 * P + scr_row) * 4;
  LGNN_REQUIRE(per_sample <= h->ws_limit / 2, "lgnn_glm_covariance: the workspace limit is below one sample's Jacobian rows");
  int64_t mc_max = std::max<int64_t>(1, h->ws_limit / 2 / per_sample);
  mc_max = std::min<int64_t>(mc_max, std::max<int64_t>(1, 32767 / C));  // the rotations batch over the rows: grid.z
  const int64_t ca = std::min(mc_max, Ma), cb = std::min(mc_max, Mb), cm = std::max(ca, cb);
  LGNN_CALL(w.gp_jac_a.reserve(size_t(ca) * C * P * 4));
  LGNN_CALL(w.gp_jac_b.reserve(size_t(cm) * C * P * 4));
  if (scr_row > 0) LGNN_CALL(w.cov_scr.reserve(size_t(cm) * C * scr_row * 4));
  float *Ja = w.gp_jac_a.as<float>(), *Jb = w.gp_jac_b.as<float>(), *scr = w.cov_scr.as<float>();

  // J [R, P] -> its Kronecker blocks in the eigenbasis: (Q_B^T Jw Q_A | Jb Q_B) per row
  auto rotate = [&](float* J, int64_t R) -> int {
    for (int l = 0; l < o.nb; ++l) {
      if (!o.QA[l]) continue;
      const Block& b = blk[l];
      // scr_r[i'][oo] = sum_i Jw_r[oo, i] Q_A[i, i']
      LGNN_CALL(launch_nt_gemm(h, nt(J + b.ow, b.in, P, sm + b.qa, b.in, 0, scr, 1, b.out, b.out * b.in, b.out, b.in, b.in, R), s));
      // Jw_r[k, i'] = sum_oo Q_B[oo, k] scr_r[i'][oo]
      LGNN_CALL(launch_nt_gemm(h, nt(sm + b.qb, b.out, 0, scr, b.out, b.out * b.in, J + b.ow, b.in, 1, P, b.out, b.in, b.out, R), s));
      // bias: scr[r][k] = sum_oo Jb[r, oo] Q_B[oo, k], then back in place
      LGNN_CALL(launch_nt_gemm(h, nt(J + b.ob, P, 0, sm + b.qb, b.out, 0, scr, b.out, 1, 0, R, b.out, b.out, 1), s));
      LGNN_CALL(launch_scale_rows(scr, b.out, 0, J + b.ob, P, R, b.out, nullptr, 0, 1, 1, s));
    }
    return 0;
  };

  h->cov_chunk_pairs = 0;
  for (int64_t n0 = 0; n0 < Ma; n0 += ca) {
    const int64_t ma = std::min(ca, Ma - n0);
    LGNN_CALL(jacobians(h, idx_a + n0, ma, Ja, nullptr, s));
    LGNN_CALL(rotate(Ja, ma * C));
    for (int64_t m0 = same ? n0 : 0; m0 < Mb; m0 += cb) {
      const int64_t mb = std::min(cb, Mb - m0);
      const bool diag = same && m0 == n0;
      ++h->cov_chunk_pairs;
      if (!diag) {
        LGNN_CALL(jacobians(h, idx_b + m0, mb, Jb, nullptr, s));
        LGNN_CALL(rotate(Jb, mb * C));
      }
      LGNN_CALL(launch_scale_rows(diag ? Ja : Jb, P, 0, Jb, P, mb * C, P, sm, 0, 1, 1, s));
      NtProblem p = nt(Ja, P, 0, Jb, P, 0, K + n0 * C * ldk + m0 * C, ldk, 1, 0, ma * C, mb * C, P, 1);
      p.upper_only = diag ? 1 : 0;
      LGNN_CALL(launch_nt_gemm(h, p, s));
    }
  }
  if (same) LGNN_CALL(launch_mirror(K, Ma * C, ldk, 1, 0, s));
  return 0;
}

}  // namespace

int glm_covariance(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int n_blocks,
                   const float* const* QA, const float* const* QB, const float* const* S, int flags, float* K, int64_t ldk,
                   hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_REQUIRE((flags & ~LGNN_COV_FROM_JACOBIANS) == 0, "unknown flag");
  LGNN_REQUIRE(n_blocks == h->n_blocks(), "lgnn_glm_covariance: n_blocks is not the model's number of Linear layers");
  LGNN_REQUIRE(ldk >= Mb * h->dims[h->L], "row stride of K too small");
  for (int l = 0; l < n_blocks; ++l) {
    LGNN_REQUIRE(S[l] != nullptr, "lgnn_glm_covariance: a block without its inverse precisions");
    LGNN_REQUIRE((QA[l] == nullptr) == (QB[l] == nullptr), "lgnn_glm_covariance: a block with one of its two eigenbases");
  }
  const CovOperands o{n_blocks, QA, QB, S};
  if (closed_form_model(h) && !(flags & LGNN_COV_FROM_JACOBIANS)) return cov_structured(h, idx_a, Ma, idx_b, Mb, o, K, ldk, s);
  return cov_general(h, idx_a, Ma, idx_b, Mb, o, K, ldk, s);
}

}  // namespace lgnn

// K = J(idx_a) P^-1 J(idx_b)^T: functional_covariance of laplace/baselaplace.py:1223-1242, 1491-1494, 1638-1644, 1905-1910 and
// laplace/utils/matrix.py (inv_square_form)
extern "C" int lgnn_glm_covariance(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int n_blocks,
                                   const float* const* QA, const float* const* QB, const float* const* S, int flags, float* K,
                                   int64_t ldk, void* stream) {
  if (!h || !QA || !QB || !S || ((Ma > 0 && Mb > 0) && (!idx_a || !idx_b || !K))) { lgnn::set_error("null argument"); return 2; }
  if (Ma <= 0 || Mb <= 0) return 0;
  return lgnn::glm_covariance(h, idx_a, Ma, idx_b, Mb, n_blocks, QA, QB, S, flags, K, ldk, static_cast<hipStream_t>(stream));
}

extern "C" int64_t lgnn_glm_covariance_chunk_pairs(lgnn_ctx* h) { return h ? h->cov_chunk_pairs : -1; }
