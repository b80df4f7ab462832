// The closed-form Jacobian of 1- and 2-layer GCN / GraphSAGE models without res / norm, seen once.
//
// Reference: CurvatureInterface.jacobians (laplace/curvature/curvature.py:89-130) differentiates the whole model by
// torch.func.jacrev; for the models the reference can construct (<= 2 layers, gnn/models/base_gnn.py:109) every entry has a
// closed form.  With a = the sample's node, E[v] = [what the first Linear multiplies at node v | its bias
// column], d_v = act'(h_1[v]) and W_1 = [Ws | Wn] (GCN: W_1 = Wn):
//   last layer   d f_c / d W_last = e_c (x) phi_a,  d f_c / d b_last = s_a e_c
//   first layer  Tn[h, i] = sum_u P[a, u] d_u[h] E[u, i]      Ts[h, i] = d_a[h] E[a, i]   (GraphSAGE's self path)
//                d f_c / d W_0[h, i] = Ws[c, h] Ts[h, i] + Wn[c, h] Tn[h, i]              (i == in_0: the bias entry of unit h)
// Four kernels evaluate these entries -- the Jacobians (jacobian.hip), the per-sample gradients (fisher.hip), a subset of
// columns (subnet.hip) and the tables of the GP kernel (gpkernel.hip) -- and tests hold some of them to bit equality with each
// other, so the operands are resolved by ONE host function (closed_form_view, context.hip: it owns ForwardCache), reach every
// kernel through one argument list (LGNN_CF_PARAMS), and the three shared pieces of arithmetic are the device functions at the
// end of this file.
#pragma once
#include "lgnn_internal.h"

namespace lgnn {

// What a Linear multiplies, seen from an output node, plus its bias column: the rows the diagonal and last-layer kernels gather
struct FeatView {  // E[v, i]: i < width -> base[v*ld + i]; i == width -> bias column
  const float* base;
  int64_t ld;
  int64_t width;
  const float* bias_col;  // per-node scale (rowsum) or nullptr for the constant 1
  int64_t nrows;          // node ids outside [0, nrows) (flagged by the batch prologue) read as zero rows
};
// v known to be a node (a stored column of P, a checked sample id): no range check
__device__ __forceinline__ float feat_at(const FeatView& f, int64_t v, int64_t i) {
  return i < f.width ? f.base[v * f.ld + i] : (f.bias_col ? f.bias_col[v] : 1.f);
}
__device__ __forceinline__ float feat(const FeatView& f, int64_t v, int64_t i) {
  if (v < 0 || v >= f.nrows) return 0.f;
  if (i < f.width) return f.base[v * f.ld + i];
  return f.bias_col ? f.bias_col[v] : 1.f;
}
// GCN: [(P in_l) | rowsum(P)], GraphSAGE: [cat_l | 1] (needs forward_ensure_aux)
int feat_views(lgnn_ctx* h, int layer, FeatView& f);
// out [M, ldp] = [phi_n | s_n | 0 ...] of the batch rows idx[0..M) of a view (lastlayer_full.hip, ll_build_phi_kernel)
int launch_ll_build_phi(const int64_t* idx, int64_t M, const FeatView& Phi, int64_t ldp, float* out, hipStream_t s);

// L <= 2 and neither res nor norm: the model has the closed form above.  (Switches such as LGNN_JAC_PLANES or a call's
// _FROM_JACOBIANS flag are the caller's, written next to its call.)
bool closed_form_model(const lgnn_ctx* h);

struct ClosedForm {
  int L, sage;
  int64_t N, in0, H, C, in_last, P;  // H = 0 for one-layer models
  int64_t off_last;                  // where [W_last | b_last] starts in the parameter vector: after [W_0 | b_0]
  const int32_t* rowptr; const int32_t* col; const float* val;  // P
  FeatView E0, PhiL;                 // the first and the last Linear's features (the same view for one-layer models)
  const float* dact;                 // act'(h_1) [N, H]
  const float* W1; int64_t w1_ld;    // [C, w1_ld]: Wn (GCN), [Ws | Wn] (GraphSAGE); null / 0 for one-layer models
};
int closed_form_view(lgnn_ctx* h, ClosedForm& cf);  // closed_form_model(h); needs forward_ensure_aux

// Kernel side.  A workgroup handles one sample, so col[p], val[p] and the bias column at col[p] are wave-uniform and hipcc
// reads them through the scalar cache -- but only through pointers it knows not to alias the kernel's stores, and pointer
// members of a struct passed by value are not such pointers.  So a kernel takes the view's members as arguments of its own,
// every pointer const __restrict__, and assembles the view from them (registers only, nothing is copied); the host side
// spreads a ClosedForm over those arguments with LGNN_CF_ARGS.
#define LGNN_CF_PARAMS                                                                                                        \
  int64_t cf_N, const int32_t *__restrict__ cf_rowptr, const int32_t *__restrict__ cf_col, const float *__restrict__ cf_val,  \
      int cf_L, int cf_sage, int64_t cf_in0, int64_t cf_H, int64_t cf_C, const float *__restrict__ cf_e0, int64_t cf_e0_ld,   \
      const float *__restrict__ cf_e0_bias, const float *__restrict__ cf_dact, const float *__restrict__ cf_W1,               \
      int64_t cf_w1_ld, const float *__restrict__ cf_phil, int64_t cf_phil_ld, int64_t cf_in_last,                            \
      const float *__restrict__ cf_phil_bias, int64_t cf_P
#define LGNN_CF_ARGS(v)                                                                                                       \
  (v).N, (v).rowptr, (v).col, (v).val, (v).L, (v).sage, (v).in0, (v).H, (v).C, (v).E0.base, (v).E0.ld, (v).E0.bias_col,       \
      (v).dact, (v).W1, (v).w1_ld, (v).PhiL.base, (v).PhiL.ld, (v).in_last, (v).PhiL.bias_col, (v).P
#define LGNN_CF_VIEW                                                                                                          \
  ClosedForm {                                                                                                                \
    cf_L, cf_sage, cf_N, cf_in0, cf_H, cf_C, cf_in_last, cf_P, cf_L == 2 ? cf_H * cf_in0 + cf_H : 0, cf_rowptr, cf_col,       \
        cf_val, FeatView{cf_e0, cf_e0_ld, cf_in0, cf_e0_bias, cf_N}, FeatView{cf_phil, cf_phil_ld, cf_in_last, cf_phil_bias, cf_N}, \
        cf_dact, cf_W1, cf_w1_ld                                                                                              \
  }

// Tn[hh, i] of the sample whose row of P is [ps, pe), summed in the row's stored order
__device__ __forceinline__ float cf_neigh(const ClosedForm& cf, int32_t ps, int32_t pe, int64_t hh, int64_t i) {
  float tn = 0.f;
  for (int32_t p = ps; p < pe; ++p) {
    const int64_t u = cf.col[p];
    const float e = feat_at(cf.E0, u, i);
    tn = fmaf(cf.val[p] * cf.dact[u * cf.H + hh], e, tn);
  }
  return tn;
}
// Ts[hh, i] of node a (GraphSAGE: the bias column is the constant 1)
__device__ __forceinline__ float cf_self(const ClosedForm& cf, int64_t a, int64_t hh, int64_t i) {
  return cf.dact[a * cf.H + hh] * (i < cf.in0 ? cf.E0.base[a * cf.E0.ld + i] : 1.f);
}
// d f_c / d W_0[hh, i] from the two tiles' entries
__device__ __forceinline__ float cf_class_row(const ClosedForm& cf, int64_t c, int64_t hh, float ts, float tn) {
  return cf.sage ? cf.W1[c * cf.w1_ld + hh] * ts + cf.W1[c * cf.w1_ld + cf.H + hh] * tn : cf.W1[c * cf.w1_ld + hh] * tn;
}

}  // namespace lgnn
