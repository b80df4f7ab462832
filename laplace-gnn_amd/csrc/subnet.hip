// Subnetwork Laplace (Daxberger et al. 2021; laplace/subnetlaplace.py:175-199): the GGN and the Jacobians over a subset
// S of the Laplace parameter vector.
//
// Reference: GGNInterface with subnetwork_indices forms the whole J [M, C, P] by jacrev and slices its columns
// (laplace/curvature/curvature.py:127-128), then contracts the slice (:374-410).  Here the slice is built directly:
//   * 1- and 2-layer GCN / GraphSAGE without res / norm: the closed form of jac_closed_form_kernel (jacobian.hip) evaluated
//     for the selected columns only.  A first-layer column (h, i) is one pass over the deg(a) neighbours of the sample and its
//     C class rows are a scaling by W1[:, h]; a last-layer column is one feature of the sample.  M C S floats are written
//     instead of M C P.  For the GGN the Hessian square root of ggn_mix_rows_kernel (jacobian.hip) is applied while the column
//     is built: with p = softmax(f_a), the mixed rows of a first-layer column are sqrt(p_c) (W1[c, h] - sum_k p_k W1[k, h]) t
//     (GraphSAGE: the self and the neighbour half of W1 each), those of a last-layer column (c', d) are
//     sqrt(p_c) (delta_cc' - p_c') phi[d].  sum_k p_k W1[k, :] and sqrt(p) are staged in LDS once per sample.
//   * every other model: chunks of lgnn_jacobians' rows, a column gather that mixes on the way.
// Both write X [mc C, ld] (ld = S rounded up to 4 floats, padding zeroed) and hand it to the fp32 MFMA Gram kernel, which
// adds straight into the caller's H [S, S].
//
// Column order.  Element-granular gathers from the feature rows are uncoalesced unless neighbouring lanes read neighbouring
// floats, so the columns are processed in the order of their vector index -- which is (kind, unit, input column) order: W_0 row
// major, b_0, W_last row major, b_last -- and every value is written through the sorted column's position in the caller's
// list.  The outputs are in the caller's order; nothing is permuted afterwards.
#include "closedform.h"
#include "lgnn_internal.h"

#include <rocprim/rocprim.hpp>

namespace lgnn {

namespace {

// one selected column in processing order
struct SubCol {
  int32_t kind;  // 0: first-layer weight (unit h, col i)  1: first-layer bias (unit h)  2: last weight (unit c', col d)
                 // 3: last bias (unit c')  4: index outside [0, P): a zero column
  int32_t unit, col;
  int32_t dst;   // position in the caller's list
};
static_assert(sizeof(SubCol) == 16);

__global__ void subnet_iota_kernel(int32_t* __restrict__ v, int64_t S) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < S) v[j] = int32_t(j);
}

// the layout jac_closed_form_kernel writes: [W_0 (H x in0) | b_0 (H)] (2-layer models) then [W_last (C x in_last) | b_last (C)]
__global__ void subnet_plan_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ ord, int64_t S, int64_t P,
                                   int L, int64_t in0, int64_t H, int64_t C, int64_t in_last, SubCol* __restrict__ plan,
                                   int* __restrict__ bad) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= S) return;
  const int64_t q = keys[j];
  SubCol sc;
  sc.dst = ord[j];
  sc.kind = 4; sc.unit = 0; sc.col = 0;
  const int64_t off_last = L == 2 ? H * in0 + H : 0;
  if (q < 0 || q >= P) bad[4] = 1;
  else if (q < off_last) {
    if (q < H * in0) { sc.kind = 0; sc.unit = int32_t(q / in0); sc.col = int32_t(q - int64_t(sc.unit) * in0); }
    else { sc.kind = 1; sc.unit = int32_t(q - H * in0); }
  } else {
    const int64_t r = q - off_last;
    if (r < C * in_last) { sc.kind = 2; sc.unit = int32_t(r / in_last); sc.col = int32_t(r - int64_t(sc.unit) * in_last); }
    else { sc.kind = 3; sc.unit = int32_t(r - C * in_last); }
  }
  plan[j] = sc;
}

// X[(m C + c) ld + dst] for the planned columns of sample m; columns [S, ld) are zeroed.  probs == null: the Jacobian's own
// rows -- the entries jac_closed_form_kernel writes, from the same device functions (closedform.h), so the bits agree;
// otherwise the rows mixed with the Hessian square root.  Dynamic LDS: 2 C + w1_ld floats.
__global__ __launch_bounds__(256) void subnet_closed_form_kernel(const int64_t* __restrict__ idx, LGNN_CF_PARAMS,
                                                                 const SubCol* __restrict__ plan, int64_t S, int64_t ld,
                                                                 const float* __restrict__ probs, float* __restrict__ X,
                                                                 int* __restrict__ bad) {
  extern __shared__ float lds[];
  const ClosedForm cf = LGNN_CF_VIEW;
  const int64_t C = cf.C, H = cf.H;
  float* __restrict__ sp = lds;          // sqrt(p_c)
  float* __restrict__ pr = lds + C;      // p_c
  float* __restrict__ wbar = lds + 2 * C;  // sum_k p_k W1[k, :]  (GraphSAGE: both halves)
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  float* __restrict__ Xm = X + m * C * ld;
  const int64_t t0 = int64_t(blockIdx.y) * blockDim.x + threadIdx.x, tstep = int64_t(gridDim.y) * blockDim.x;
  if (a < 0 || a >= cf.N) {
    if (t0 == 0) bad[1] = 1;
    for (int64_t t = t0; t < C * ld; t += tstep) Xm[t] = 0.f;
    return;
  }
  const bool mix = probs != nullptr;
  if (mix) {
    const float* __restrict__ pm = probs + m * C;
    for (int64_t c = threadIdx.x; c < C; c += blockDim.x) { const float p = pm[c]; pr[c] = p; sp[c] = sqrtf(p); }
    if (cf.W1)
      for (int64_t q = threadIdx.x; q < cf.w1_ld; q += blockDim.x) {
        float t = 0.f;
        for (int64_t k = 0; k < C; ++k) t = fmaf(pm[k], cf.W1[k * cf.w1_ld + q], t);
        wbar[q] = t;
      }
    __syncthreads();
  }
  const int32_t ps = cf.rowptr[a], pe = cf.rowptr[a + 1];
  for (int64_t j = t0; j < ld; j += tstep) {
    SubCol sc;
    sc.kind = 4; sc.unit = 0; sc.col = 0; sc.dst = int32_t(j);  // padding: a zero column in place
    if (j < S) sc = plan[j];
    float* __restrict__ out = Xm + sc.dst;
    if (sc.kind <= 1) {
      const int64_t hh = sc.unit;
      const int64_t i = sc.kind == 0 ? int64_t(sc.col) : cf.in0;  // in0: the bias entry of unit hh
      const float tn = cf_neigh(cf, ps, pe, hh, i);
      float ts = 0.f;
      if (cf.sage) ts = cf_self(cf, a, hh, i);
      if (!mix) {
        for (int64_t c = 0; c < C; ++c) out[c * ld] = cf_class_row(cf, c, hh, ts, tn);
      } else {
        const float bs = wbar[hh], bn = cf.sage ? wbar[H + hh] : 0.f;
        for (int64_t c = 0; c < C; ++c) {
          const float v = cf.sage ? (cf.W1[c * cf.w1_ld + hh] - bs) * ts + (cf.W1[c * cf.w1_ld + H + hh] - bn) * tn
                                  : (cf.W1[c * cf.w1_ld + hh] - bs) * tn;
          out[c * ld] = sp[c] * v;
        }
      }
    } else if (sc.kind <= 3) {
      const float phi = sc.kind == 2 ? cf.PhiL.base[a * cf.PhiL.ld + sc.col] : (cf.PhiL.bias_col ? cf.PhiL.bias_col[a] : 1.f);
      const int64_t cq = sc.unit;
      if (!mix) {
        for (int64_t c = 0; c < C; ++c) out[c * ld] = c == cq ? phi : 0.f;
      } else {
        const float pq = pr[cq];
        for (int64_t c = 0; c < C; ++c) out[c * ld] = sp[c] * ((c == cq ? 1.f : 0.f) - pq) * phi;
      }
    } else {
      for (int64_t c = 0; c < C; ++c) out[c * ld] = 0.f;
    }
  }
}

// The other models: columns keys[0..S) of a chunk of Jacobian rows J [mc, C, P] -> X [mc C, ld] at their positions in the
// caller's list, mixed like ggn_mix_rows_kernel when probs != null; columns [S, ld) and out-of-range keys are zero columns.
__global__ __launch_bounds__(256) void subnet_gather_kernel(const float* __restrict__ J, int64_t P, int64_t C,
                                                            const int64_t* __restrict__ keys, const int32_t* __restrict__ ord,
                                                            int64_t S, int64_t ld, const float* __restrict__ probs,
                                                            float* __restrict__ X, int* __restrict__ bad) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t m = blockIdx.y;
  if (j >= ld) return;
  float* __restrict__ Xm = X + m * C * ld;
  int64_t q = -1, dst = j;
  if (j < S) { q = keys[j]; dst = ord[j]; if (q < 0 || q >= P) { bad[4] = 1; q = -1; } }
  if (q < 0) {
    for (int64_t c = 0; c < C; ++c) Xm[c * ld + dst] = 0.f;
    return;
  }
  const float* __restrict__ Jm = J + m * C * P + q;
  if (!probs) {
    for (int64_t c = 0; c < C; ++c) Xm[c * ld + dst] = Jm[c * P];
    return;
  }
  const float* __restrict__ pm = probs + m * C;
  float t = 0.f;
  for (int64_t k = 0; k < C; ++k) t += pm[k] * Jm[k * P];
  for (int64_t c = 0; c < C; ++c) Xm[c * ld + dst] = sqrtf(pm[c]) * (Jm[c * P] - t);
}

// ws.subnet_keys / ws.subnet_ord: the caller's indices in increasing order and their positions in the caller's list;
// closed-form models: ws.subnet_plan, the decoded columns
int subnet_prepare(lgnn_ctx* h, const int64_t* subnet, int64_t S, hipStream_t s) {
  Workspace& w = h->ws;
  LGNN_REQUIRE(S > 0 && S < (int64_t(1) << 31), "subnetwork size");
  LGNN_CALL(w.subnet_keys.reserve(size_t(S) * 8));
  LGNN_CALL(w.subnet_ord.reserve(size_t(S) * 4));
  LGNN_CALL(w.subnet_iota.reserve(size_t(S) * 4));
  hipLaunchKernelGGL(subnet_iota_kernel, dim3(unsigned(cdiv(S, 256))), dim3(256), 0, s, w.subnet_iota.as<int32_t>(), S);
  LGNN_HIP_CHECK(hipGetLastError());
  size_t bytes = 0;
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, subnet, w.subnet_keys.as<int64_t>(), w.subnet_iota.as<int32_t>(),
                                           w.subnet_ord.as<int32_t>(), size_t(S), 0, 64, s));
  LGNN_CALL(w.subnet_tmp.reserve(bytes));
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(w.subnet_tmp.p, bytes, subnet, w.subnet_keys.as<int64_t>(),
                                           w.subnet_iota.as<int32_t>(), w.subnet_ord.as<int32_t>(), size_t(S), 0, 64, s));
  if (!closed_form_model(h)) return 0;
  const int L = h->L;
  LGNN_REQUIRE(h->n_params < (int64_t(1) << 31), "subnetwork: parameter count");
  LGNN_CALL(w.subnet_plan.reserve(size_t(S) * sizeof(SubCol)));
  hipLaunchKernelGGL(subnet_plan_kernel, dim3(unsigned(cdiv(S, 256))), dim3(256), 0, s, w.subnet_keys.as<int64_t>(),
                     w.subnet_ord.as<int32_t>(), S, h->n_params, L, h->in_dim[0], L == 2 ? h->dims[1] : 0, h->dims[L],
                     h->in_dim[L - 1], w.subnet_plan.as<SubCol>(), w.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// the planned columns of samples idx[0..mc) into X [mc C, ld]; needs forward_ensure_aux and subnet_prepare
int launch_subnet_closed_form(lgnn_ctx* h, const int64_t* idx, int64_t mc, int64_t S, int64_t ld, const float* probs,
                              float* X, hipStream_t s) {
  ClosedForm cf;
  LGNN_CALL(closed_form_view(h, cf));
  LGNN_REQUIRE(mc < (int64_t(1) << 31), "too many samples");
  const size_t lds = size_t(2 * cf.C + cf.w1_ld) * 4;
  LGNN_REQUIRE(lds <= 48 * 1024, "subnetwork: classes + hidden width exceed the staging area");
  const unsigned per = unsigned(std::max<int64_t>(1, std::min<int64_t>(cdiv(ld, 256), cdiv(2048, mc))));
  hipLaunchKernelGGL(subnet_closed_form_kernel, dim3(unsigned(mc), per), dim3(256), lds, s, idx, LGNN_CF_ARGS(cf),
                     h->ws.subnet_plan.as<SubCol>(), S, ld, probs, X, h->ws.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_subnet_gather(lgnn_ctx* h, const float* J, int64_t mc, int64_t S, int64_t ld, const float* probs, float* X,
                         hipStream_t s) {
  LGNN_REQUIRE(mc < 65536, "subnetwork gather: chunk too large");
  hipLaunchKernelGGL(subnet_gather_kernel, dim3(unsigned(cdiv(ld, 256)), unsigned(mc)), dim3(256), 0, s, J, h->n_params,
                     h->dims[h->L], h->ws.subnet_keys.as<int64_t>(), h->ws.subnet_ord.as<int32_t>(), S, ld, probs, X,
                     h->ws.flags.as<int>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int jacobians_subset(lgnn_ctx* h, const int64_t* idx, int64_t M, const int64_t* subnet, int64_t S, float* J, float* f_out,
                     hipStream_t s) {
  LGNN_REQUIRE(h->L > 0, "no model bound");
  LGNN_CALL(subnet_prepare(h, subnet, S, s));
  const int64_t C = h->dims[h->L], P = h->n_params;
  if (closed_form_model(h)) {
    LGNN_CALL(forward_ensure_aux(h, s));
    if (f_out) LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), C, h->N, idx, M, C, f_out, h->ws.flags.as<int>() + 2, s));
    return launch_subnet_closed_form(h, idx, M, S, S, nullptr, J, s);
  }
  const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, 65535), h->ws_limit / std::max<int64_t>(C * P * 4, 1)));
  LGNN_CALL(h->ws.jac.reserve(size_t(mc_max) * C * P * 4));
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, h->ws.jac.as<float>(), f_out ? f_out + m0 * C : nullptr, s));
    LGNN_CALL(launch_subnet_gather(h, h->ws.jac.as<float>(), mc, S, S, nullptr, J + m0 * C * S, s));
  }
  return 0;
}

int subnet_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const int64_t* subnet, int64_t S,
                           float* H_out, float* loss_out, hipStream_t s) {
  LGNN_REQUIRE(h->L >= 1, "no model bound");
  LGNN_REQUIRE(S > 0 && S * S < (int64_t(1) << 40), "subnetwork GGN: S x S does not fit");
  LGNN_CALL(forward_ensure(h, s));
  const bool closed = closed_form_model(h);
  if (closed) LGNN_CALL(forward_ensure_aux(h, s));
  LGNN_CALL(subnet_prepare(h, subnet, S, s));
  const int64_t C = h->dims[h->L], P = h->n_params;
  const int64_t ld = cdiv(S, 4) * 4;  // 16-byte rows: launch_gram's vector path
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
  const int64_t per_sample = C * (closed ? ld : P + ld) * 4;
  int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / std::max<int64_t>(per_sample, 1)));
  if (!closed) mc_max = std::min<int64_t>(mc_max, 65535);
  LGNN_CALL(h->ws.subnet_x.reserve(size_t(mc_max) * C * ld * 4));
  if (!closed) LGNN_CALL(h->ws.jac.reserve(size_t(mc_max) * C * P * 4));
  float* X = h->ws.subnet_x.as<float>();
  const bool mix = h->lik != LGNN_LIK_REGRESSION;
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    const float* probs = mix ? h->ws.probs.as<float>() + m0 * C : nullptr;
    if (closed) LGNN_CALL(launch_subnet_closed_form(h, idx + m0, mc, S, ld, probs, X, s));
    else {
      LGNN_CALL(jacobians(h, idx + m0, mc, h->ws.jac.as<float>(), nullptr, s));
      LGNN_CALL(launch_subnet_gather(h, h->ws.jac.as<float>(), mc, S, ld, probs, X, s));
    }
    LGNN_CALL(launch_gram(X, ld, mc * C, S, H_out, s));
  }
  LGNN_CALL(launch_symmetrize_upper(H_out, S, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn

extern "C" int lgnn_jacobians_subset(lgnn_ctx* h, const int64_t* idx, int64_t M, const int64_t* subnet, int64_t S, float* J,
                                     float* f_out, void* stream) {
  if (!h || (M > 0 && (!idx || !J)) || (S > 0 && !subnet)) { lgnn::set_error("null argument"); return 2; }
  if (M <= 0 || S <= 0) return 0;
  return lgnn::jacobians_subset(h, idx, M, subnet, S, J, f_out, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_subnet_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const int64_t* subnet,
                                           int64_t S, float* H_out, float* loss_out, void* stream) {
  if (!h || !idx || !y || !subnet || !H_out || !loss_out || M <= 0 || S <= 0) {
    lgnn::set_error("empty batch, empty subnetwork or null pointers");
    return 2;
  }
  return lgnn::subnet_full_accumulate(h, idx, y, M, subnet, S, H_out, loss_out, static_cast<hipStream_t>(stream));
}
