// Matrix-free GLM predictive variance for 1- and 2-layer GCN and GraphSAGE models: diag(J P^-1 J^T) per evaluation node
// without ever materialising the Jacobians (one-layer models: glm_var_onelayer_kernel below).
//
// Reference: la(x) -> _glm_predictive_distribution (laplace/baselaplace.py:1123-1158): Js [M, C, P] from
// torch.func.jacrev of the dense model (laplace/curvature/curvature.py:89-130), f_var = Js P^-1 Js^T through
// KronDecomposed.inv_square_form (laplace/utils/matrix.py:396-451) resp. the diagonal einsum (baselaplace.py:1901-1903); the
// default link (probit, baselaplace.py:610-616) reads the diagonal of f_var only.  M * C * P floats cap that route at a few
// hundred evaluation nodes of an arxiv-sized model (P = 43 k: 7 MB per node).
//
// For the model family of the path the per-node Jacobian is closed form, with a = idx[n]:
//   last layer :  d f_c / d W_1 = e_c (x) phi_a,   phi_a = (P H_1)[a],    d f_c / d b_1 = s_a e_c,  s_a = rowsum(P)[a]
//   first layer:  d f_c / d W_0 = diag(w_c) T_a,   T_a = sum_u P[a,u] d_u (x) xhat_u,  d_u = act'(h_1[u]), xhat = P X
//                 d f_c / d b_0 = w_c * tb_a,      tb_a = sum_u P[a,u] rowsum(P)[u] d_u                 (w_c = W_1[c, :])
// Kronecker posterior (block l: f B_l (x) A_l + delta, eigenpairs (Q_B, lB), (Q_A, lA); the bias block shares Q_B):
//   W_0 + b_0:  M_c = sum_u P[a,u] r_{u,c} (x) ztilde_u  with  r_{u,c} = Q_B0^T (w_c * d_u)   (precomputed [nodes][C][H])
//               ztilde_u = [Q_A0^T xhat_u | rowsum(P)[u]]  (precomputed [N][F+1]);   var_c += sum_ij M_c[i,j]^2 S0[i,j],
//               S0[i,j] = 1 / (f lB0_i lA0_j + delta_w0), bias column j = F: 1 / (f lB0_i + delta_b0)
//   W_1 + b_1:  var_c += sum_i Q_B1[c,i]^2 sum_j phitilde_j^2 S1[i,j] + s_a^2 kappa_c
// Diagonal posterior: var_c = sum_h w_c[h]^2 sum_j T_a[h,j]^2 / prec_0[h,j] + sum_j phi_a[j]^2 / prec_1[c,j] + s_a^2 / prec_b1[c].
// GraphSAGE (gnn/models/layers.py:18-29): the first Linear sees cat_0[v] = [x_v | (P x)_v] (bias column 1) and the node itself
// joins its neighbours as one more entry:  d f_c / d W_0 = diag(ws_c * d_a) (x) cat_0[a] + sum_u P[a,u] diag(wn_c * d_u) (x) cat_0[u]
// (ws / wn = self / neighbour half of W_1's row c), the last layer's feature row is phi_a = cat_1[a], s_a = 1.  Same kernel:
// the self entry is staged behind the row's entries with weight 1 and its own rotated rows R_self[m, c, :].
// One workgroup per evaluation node: thread (row i, column group) keeps its slice of the H x (F+1) tile in registers.
#include "device_utils.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

constexpr int PJT = 64;   // feature columns of the tile per thread (the bias column is one more register)
constexpr int PUC = 48;   // neighbours staged per pass

__global__ void pred_mark_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, const int32_t* __restrict__ rowptr,
                                 const int32_t* __restrict__ col, uint8_t* __restrict__ need, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) { if (lane == 0) bad[1] = 1; return; }
  for (int32_t p = rowptr[n] + lane; p < rowptr[n + 1]; p += 64) need[col[p]] = 1;
}
__global__ void pred_slots_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ count, int32_t* __restrict__ slot) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k < *count) slot[list[k]] = int32_t(k);
}

// The one builder of the per-class row table: the signal of class c that arrives at the pre-norm row s_u,
// q_{u,c} = norm_u^T (d_u * w_c) (resnorm.hip's backward of one row, with w_c as the incoming gradient):
//   LayerNorm:  g = gamma * d_u * w_c,  q = rstd_u (g - mean(g) - xhat_u mean(g * xhat_u))     (means over the H channels)
//   BatchNorm (eval): q = gamma * rstd_channel * d_u * w_c;      no norm (plain models): q = d_u * w_c
// One wave per (node, class) row, H <= 256: four channels per lane in registers, two wave reductions for the LayerNorm.
// Row r = (k, c): node = list[k0 + k] (the needed nodes) or idx[k0 + k] (the evaluation nodes themselves, GraphSAGE's self
// entry; an id out of range gives a zero row).  A [(k, c), H].
__global__ __launch_bounds__(256) void pred_q_kernel(const int32_t* __restrict__ list, const int64_t* __restrict__ idx,
                                                     int64_t k0, int64_t kn, int64_t N, const float* __restrict__ dact,
                                                     int64_t H, const float* __restrict__ W1, int64_t ldw, int64_t C,
                                                     int norm, const float* __restrict__ gamma,
                                                     const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                     float* __restrict__ A) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = kn * C, stride = int64_t(gridDim.x) * 4;
  const float invH = 1.0f / float(H);
  for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < rows; r += stride) {
    const int64_t k = r / C, c = r - k * C;
    const int64_t node = list ? int64_t(list[k0 + k]) : idx[k0 + k];
    float* __restrict__ out = A + r * H;
    if (node < 0 || node >= N) {
      for (int64_t j = lane; j < H; j += 64) out[j] = 0.f;
      continue;
    }
    const float* __restrict__ dn = dact + node * H;
    const float* __restrict__ w = W1 + c * ldw;
    const float* __restrict__ xh = xhat + node * H;  // (read under a LayerNorm only)
    float g[4], x[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t j = lane + 64 * t;
      g[t] = 0.f; x[t] = 0.f;
      if (j < H) {
        g[t] = w[j] * dn[j];
        if (norm != LGNN_NORM_NONE) g[t] *= gamma[j];
        if (norm == LGNN_NORM_LAYER) { x[t] = xh[j]; s1 += g[t]; s2 += g[t] * x[t]; }
        else if (norm == LGNN_NORM_BATCH) g[t] *= rstd[j];
      }
    }
    if (norm == LGNN_NORM_LAYER) {
      const float m1 = wave_sum(s1) * invH, m2 = wave_sum(s2) * invH, rs = rstd[node];
#pragma unroll
      for (int t = 0; t < 4; ++t) g[t] = rs * (g[t] - m1 - x[t] * m2);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t j = lane + 64 * t;
      if (j < H) out[j] = g[t];
    }
  }
}

// Where a thread's first-layer row of a staged entry u comes from:
//   Table  : the per-class table R [slots, C, H] / Rs [M, C, H] = q_{u,c} (pred_q_kernel; KRON: rotated), the tile loops over
//            the classes.  Every Kronecker posterior, every model with res / norm, and lgnn_glm_variance_ext on any model.
//   InLoop : d_u read in the loop (diagonal posterior of plain models through lgnn_glm_variance(_mapped)): GCN keeps ONE class
//            independent tile T_a and mixes the classes in the tail, GraphSAGE multiplies by its two halves of W_1 per class.
enum class Rows { Table, InLoop };

// KRON = 1: R (rotated, per class) and the S tables; KRON = 0: diagonal posterior.
//   Zt  [N, ldz]   : ztilde (KRON) / xhat in place (diag), F1 - 1 = F columns used; the bias column is rowsum resp. 1
//   R   [slots, C, H] (Table) ; dact [N, H] (InLoop)
//   S0  [H, F1]    : weights of the squared tile entries (KRON: rotated basis; diag: 1 / prec of W_0 | b_0)
//   last layer: Pt [M, H] = phitilde (KRON) / phi (diag) of the batch rows; S1 [Ce, H] (KRON) / [C, H]; QB1sq [C, Ce] (KRON);
//   kappa [C].  C counts the OUTPUT rows -- the model's classes, or the rows of a linear map of the logits whose head E W_1
//   the caller passes as W1 (lgnn_glm_variance_mapped) -- and Ce = the model's classes (the eigen-directions of B_1)
//   SAGE = 1: one more staged entry per node (the node itself, weight 1; rows R_self[m] resp. the self half of W_1),
//   bias column 1 (rowsum == nullptr), last-layer width D1 = 2 H; W1 has row stride ldw, its neighbour half starts at wn_off
// RES_PASS: the pass of the res.0 block -- first layer only, Zt = X (KRON: X Q_Ar), bias column 1, S0 = Sr; its sum is ADDED
//   to what the conv pass (launched before it on the same stream) wrote to var_out: one workgroup per row, plain loads and
//   stores.  The conv pass (RES_PASS = false) ends with the last layer's tail.
template <int KRON, int SAGE, Rows ROWS, bool RES_PASS>
__global__ __launch_bounds__(512) void glm_var_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const float* __restrict__ val, const int32_t* __restrict__ slot,
                                                      const float* __restrict__ Zt, int64_t ldz, int64_t F1,
                                                      const float* __restrict__ R, const float* __restrict__ Rs,
                                                      const float* __restrict__ dact, const float* __restrict__ W1,
                                                      int64_t ldw, int64_t wn_off, int64_t H, int64_t C, int64_t Ce, int Hp,
                                                      const float* __restrict__ S0, const float* __restrict__ Pt, int64_t D1,
                                                      const float* __restrict__ S1, const float* __restrict__ QB1sq,
                                                      const float* __restrict__ kappa, const float* __restrict__ rowsum,
                                                      float* __restrict__ var_out) {
  static_assert(ROWS == Rows::Table || (!KRON && !RES_PASS), "in-loop rows: the diagonal posterior's conv pass only");
  constexpr bool TABLE = ROWS == Rows::Table;
  constexpr bool PER_CLASS = TABLE || SAGE;  // one tile per class; otherwise the GCN's class independent T_a
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  const int NG = 512 / Hp;          // column groups
  const int i = tid % Hp, g = tid / Hp;
  const bool row_ok = i < H;
  const int CW = NG * PJT;          // columns per chunk
  const int64_t F = F1 - 1;
  float* __restrict__ sy = sm;                       // [PUC][CW] staged p_au * ztilde_u (chunk columns)
  float* __restrict__ syb = sm + size_t(PUC) * CW;   // [PUC] staged p_au * rowsum(P)[u]: the bias column
  float* __restrict__ svar = syb + PUC;              // [C] per-class variance
  float* __restrict__ sg = svar + C;                 // [H] (diag: g[h]) / [Ce] scratch (kron: t_i)
  const int nsg = max(int(H), max(int(C), int(Ce)));
  int32_t* __restrict__ su = reinterpret_cast<int32_t*>(sg + nsg);  // [PUC] slot / node of the staged neighbours
  if (a < 0 || a >= N) {  // flagged by the marking kernel
    if (!RES_PASS)
      for (int c = tid; c < C; c += 512) var_out[m * C + c] = 0.f;
    return;
  }
  for (int c = tid; c < nsg; c += 512) { if (c < C) svar[c] = 0.f; sg[c] = 0.f; }
  const int32_t ps = rowptr[a], pe = rowptr[a + 1];
  const int deg = pe - ps + SAGE;  // GraphSAGE: the node itself is one more entry (the last)
  const int nub = (deg + PUC - 1) / PUC;
  __syncthreads();

  auto stage = [&](int ub, int64_t jc0) {  // neighbours [ub * PUC, ...) x columns [jc0, jc0 + CW)
    const int un = min(PUC, deg - ub * PUC);
    for (int t = tid; t < un * CW; t += 512) {
      const int u = t / CW, j = t - u * CW;
      const int32_t p = ps + ub * PUC + u;
      const bool self = SAGE && p >= pe;
      const int64_t node = self ? a : int64_t(col[p]);
      const float pv = self ? 1.f : val[p];
      const int64_t jj = jc0 + j;
      sy[t] = jj < F ? pv * Zt[node * ldz + jj] : 0.f;
      if (j == 0) {
        // staged id: table -> slot of the neighbour's rows, -1 for the self entry; otherwise the node id, the self
        // entry as -1 - node
        su[u] = TABLE ? (self ? -1 : slot[node]) : (self ? int32_t(-1 - node) : int32_t(node));
        syb[u] = pv * (rowsum ? rowsum[node] : 1.f);
      }
    }
    return un;
  };

  for (int64_t jc0 = 0; jc0 < F; jc0 += CW) {
    float Sreg[PJT];
#pragma unroll
    for (int j = 0; j < PJT; ++j) {
      const int64_t jj = jc0 + g * PJT + j;
      Sreg[j] = (row_ok && jj < F) ? S0[int64_t(i) * F1 + jj] : 0.f;
    }
    // the bias column rides along with the first chunk's column group 0
    const bool with_bias = jc0 == 0 && g == 0;
    const float Sb = (with_bias && row_ok) ? S0[int64_t(i) * F1 + F] : 0.f;
    int un = 0;
    if (nub == 1) { un = stage(0, jc0); __syncthreads(); }
    const int ncls = PER_CLASS ? int(C) : 1;
    for (int c = 0; c < ncls; ++c) {
      float Mt[PJT], Mb = 0.f;
#pragma unroll
      for (int j = 0; j < PJT; ++j) Mt[j] = 0.f;
      for (int ub = 0; ub < nub; ++ub) {
        if (nub > 1) { __syncthreads(); un = stage(ub, jc0); __syncthreads(); }
        for (int u0 = 0; u0 < un; u0 += 4) {
          float r[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            r[q] = 0.f;
            if (u0 + q < un && row_ok) {
              const int32_t id = su[u0 + q];
              if (TABLE) r[q] = id >= 0 ? R[(int64_t(id) * C + c) * H + i] : Rs[(m * C + c) * H + i];
              else if (SAGE) r[q] = id >= 0 ? dact[int64_t(id) * H + i] * W1[c * ldw + wn_off + i]
                                            : dact[int64_t(-1 - id) * H + i] * W1[c * ldw + i];
              else r[q] = dact[int64_t(id) * H + i];
            }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (u0 + q < un) {
              const float4* __restrict__ yr = reinterpret_cast<const float4*>(sy + (u0 + q) * CW + g * PJT);
#pragma unroll
              for (int j4 = 0; j4 < PJT / 4; ++j4) {
                const float4 y4 = yr[j4];
                Mt[4 * j4] = fmaf(r[q], y4.x, Mt[4 * j4]); Mt[4 * j4 + 1] = fmaf(r[q], y4.y, Mt[4 * j4 + 1]);
                Mt[4 * j4 + 2] = fmaf(r[q], y4.z, Mt[4 * j4 + 2]); Mt[4 * j4 + 3] = fmaf(r[q], y4.w, Mt[4 * j4 + 3]);
              }
              Mb = fmaf(r[q], syb[u0 + q], Mb);
            }
          }
        }
      }
      float part = Mb * Mb * Sb;
#pragma unroll
      for (int j = 0; j < PJT; ++j) part = fmaf(Mt[j] * Mt[j], Sreg[j], part);
      if (PER_CLASS) {
        part = wave_sum(part);
        if (lane == 0) atomicAdd(&svar[c], part);
      } else if (row_ok) {
        atomicAdd(&sg[i], part);  // g[h] = sum_j T[h, j]^2 / prec[h, j], summed over column groups and chunks
      }
    }
    __syncthreads();
  }
  if (RES_PASS) {  // the res.0 pass ends here (svar is complete: the column loop ends with a barrier)
    for (int c = tid; c < C; c += 512) var_out[m * C + c] += svar[c];
    return;
  }
  // ---- the class mixing of the diagonal posterior and the last layer
  const float sa = rowsum ? rowsum[a] : 1.f;
  const float* __restrict__ ph = Pt + m * D1;
  if (!KRON) {
    for (int c = tid; c < C; c += 512) {
      float v = PER_CLASS ? svar[c] : 0.f;
      if (!PER_CLASS)
        for (int64_t h = 0; h < H; ++h) { const float w = W1[c * ldw + h]; v = fmaf(w * w, sg[h], v); }
      for (int64_t j = 0; j < D1; ++j) v = fmaf(ph[j] * ph[j], S1[c * D1 + j], v);
      var_out[m * C + c] = v + sa * sa * kappa[c];
    }
  } else {
    // t_i = sum_j phitilde_j^2 S1[i, j]  (i < Ce), then var_c += sum_i QB1sq[c, i] t_i + s_a^2 kappa_c
    __syncthreads();
    for (int c = tid; c < Ce; c += 512) {
      float t = 0.f;
      for (int64_t j = 0; j < D1; ++j) t = fmaf(ph[j] * ph[j], S1[c * D1 + j], t);
      sg[c] = t;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 512) {
      float v = svar[c];
      for (int64_t k = 0; k < Ce; ++k) v = fmaf(QB1sq[c * Ce + k], sg[k], v);
      var_out[m * C + c] = v + sa * sa * kappa[c];
    }
  }
}

// One-layer models (out = P (X W^T + b) resp. [x | P x] W^T + b): J_n[c, (c', j)] = delta_cc' xt_n[j], bias entry rho_n, with
// xt_n = (P X)[n], rho_n = rowsum(P)[n] (GCN) or xt_n = cat_0[n], rho_n = 1 (GraphSAGE).  No tile, no neighbours:
//   KRON: var_c = sum_a QBsq[c, a] t_a + kappa_c rho^2,  t_a = sum_i S1[a, i] (Q_A^T xt)_i^2   (Pt holds the rotated rows)
//   diag: var_c = sum_i S1[c, i] xt_i^2 + kappa_c rho^2
// C counts the output rows (a linear map's rows under lgnn_glm_variance_mapped), Ce the model's classes.  One workgroup per
// evaluation node, one wave per row of S1.
template <int KRON>
__global__ __launch_bounds__(256) void glm_var_onelayer_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                               const float* __restrict__ Pt, int64_t D, int64_t C, int64_t Ce,
                                                               const float* __restrict__ S1, const float* __restrict__ QBsq,
                                                               const float* __restrict__ kappa,
                                                               const float* __restrict__ rowsum, float* __restrict__ var_out) {
  extern __shared__ float sm[];  // t [KRON ? Ce : C]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = blockIdx.x;
  const int64_t a = idx[m];
  if (a < 0 || a >= N) {  // flagged by the row gather
    for (int64_t c = tid; c < C; c += 256) var_out[m * C + c] = 0.f;
    return;
  }
  const float* __restrict__ ph = Pt + m * D;
  const int64_t rows = KRON ? Ce : C;
  for (int64_t r = wave; r < rows; r += 4) {
    float t = 0.f;
    for (int64_t i = lane; i < D; i += 64) t = fmaf(ph[i] * ph[i], S1[r * D + i], t);
    t = wave_sum(t);
    if (lane == 0) sm[r] = t;
  }
  __syncthreads();
  const float rho = rowsum ? rowsum[a] : 1.f;
  for (int64_t c = tid; c < C; c += 256) {
    float v = 0.f;
    if (KRON)
      for (int64_t k = 0; k < Ce; ++k) v = fmaf(QBsq[c * Ce + k], sm[k], v);
    else
      v = sm[c];
    var_out[m * C + c] = v + rho * rho * kappa[c];
  }
}

// glm_var_kernel's arguments on the host; the two passes differ in Zt / ldz / F1 / S0 / rowsum
struct GlmVarArgs {
  const int64_t* idx; int64_t M, N;
  Csr P;
  const int32_t* slot;
  const float* Zt; int64_t ldz, F1;
  const float* R; const float* Rs; const float* dact;
  const float* W1; int64_t ldw, wn_off, H, C, Ce; int Hp;
  const float* S0;
  const float* Pt; int64_t D1;
  const float* S1; const float* QB1sq; const float* kappa; const float* rowsum;
  float* var_out;
  size_t smem;
};

template <int KRON, int SAGE, Rows ROWS, bool RES_PASS>
int launch_glm_var_kernel(const GlmVarArgs& a, hipStream_t s) {
  LGNN_CALL((lds_opt_in<&glm_var_kernel<KRON, SAGE, ROWS, RES_PASS>>(150 * 1024)));
  hipLaunchKernelGGL((glm_var_kernel<KRON, SAGE, ROWS, RES_PASS>), dim3(unsigned(a.M)), dim3(512), a.smem, s, a.idx, a.M, a.N,
                     a.P.rowptr, a.P.col, a.P.val, a.slot, a.Zt, a.ldz, a.F1, a.R, a.Rs, a.dact, a.W1, a.ldw, a.wn_off, a.H, a.C,
                     a.Ce, a.Hp, a.S0, a.Pt, a.D1, a.S1, a.QB1sq, a.kappa, a.rowsum, a.var_out);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}
// the posterior x family dispatch of one pass (in-loop rows exist for the diagonal posterior only)
template <Rows ROWS, bool RES_PASS>
int launch_glm_var(bool kron, bool sage, const GlmVarArgs& a, hipStream_t s) {
  if constexpr (ROWS == Rows::Table)
    if (kron) return sage ? launch_glm_var_kernel<1, 1, ROWS, RES_PASS>(a, s) : launch_glm_var_kernel<1, 0, ROWS, RES_PASS>(a, s);
  return sage ? launch_glm_var_kernel<0, 1, ROWS, RES_PASS>(a, s) : launch_glm_var_kernel<0, 0, ROWS, RES_PASS>(a, s);
}

// The posterior's operands of a 2-layer model as the C entry points take them (include/laplace_gnn_hip.h):
//   kron: QA0 [F, F], QB0 [H, H], QA1 [D1, D1] rotate; diagonal posterior: the three are null.  S0 [H, F + 1], S1 [C, D1],
//   QB1sq [C, C] (kron only), kappa [C].
//   W1m [Cm, in_dim_1] (row major, or null): the head E W_1 of a linear map E [Cm, C] of the logits; f_var is then [M, Cm] =
//   diag(E J P^-1 J^T E^T) and S1 / QB1sq / kappa are the caller's mapped operands.
//   QAr [F_x, F_x], QBr [H, H] (kron), Sr [H, F_x + 1] for (W_r | b_r), F_x = dims[0]; null without res.
struct GlmOperands {
  const float* W1m; int64_t Cm;
  const float *QA0, *QB0, *S0, *QA1, *S1, *QB1sq, *kappa;
  const float *QAr, *QBr, *Sr;
};

// One-layer GCN / GraphSAGE: the only layer's operands arrive in the last layer's places (QA1 [F', F'], S1 [C, F'], QB1sq,
// kappa; F' = in_dim[0]), the first layer's (QA0, QB0, S0) are null.  Cm > 0: the rows of a linear map of the logits.
int glm_variance_onelayer(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t Cm, const float* QA1, const float* S1,
                          const float* QB1sq, const float* kappa, float* f_mu, float* f_var, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && S1 && kappa && f_var, "empty batch or null pointers");
  LGNN_REQUIRE(h->lik == LGNN_LIK_CLASSIFICATION, "matrix-free GLM predictive: classification");
  const bool kron = QA1 != nullptr;
  const bool sage = h->kind == LGNN_KIND_SAGE;
  LGNN_REQUIRE(!kron || QB1sq, "kron posterior needs all eigenvector matrices");
  LGNN_REQUIRE(Cm >= 0 && Cm <= 4096, "mapped GLM predictive: 1 <= rows of the map <= 4096");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t N = h->N, D = h->in_dim[0], Ce = h->dims[1], C = Cm > 0 ? Cm : Ce;
  int* bad = h->ws.flags.as<int>();
  if (f_mu) LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), Ce, N, idx, M, Ce, f_mu, bad + 2, s));
  const float* xt = sage ? h->fc.lin_in_p[0] : h->fc.prop_in[0].as<float>();
  const int64_t ldx = sage ? h->fc.lin_in_ld[0] : h->fc.prop_ld[0];
  LGNN_CALL(h->ws.planes_a.reserve(size_t(M) * D * 4 * 2));
  h->ws.planes_a_zero_ptr = nullptr;
  float* PhiB = h->ws.planes_a.as<float>();  // [M, D] the evaluation nodes' rows
  float* PhiT = PhiB + M * D;                // [M, D] rotated
  LGNN_CALL(launch_gather_rows(xt, ldx, N, idx, M, D, PhiB, bad + 2, s));
  const float* Pt = PhiB;
  if (kron) { LGNN_CALL(sgemm_rm(s, M, D, D, 1.f, PhiB, D, QA1, D, 0.f, PhiT, D)); Pt = PhiT; }
  const float* rowsum = sage ? nullptr : h->fc.rowsum.as<float>();
  const size_t smem = size_t(std::max(C, Ce)) * 4;
  LGNN_REQUIRE(smem <= 48 * 1024, "matrix-free GLM predictive: too many output rows");
  if (kron)
    hipLaunchKernelGGL(glm_var_onelayer_kernel<1>, dim3(unsigned(M)), dim3(256), smem, s, idx, M, N, Pt, D, C, Ce, S1, QB1sq, kappa,
                       rowsum, f_var);
  else
    hipLaunchKernelGGL(glm_var_onelayer_kernel<0>, dim3(unsigned(M)), dim3(256), smem, s, idx, M, N, Pt, D, C, Ce, S1, QB1sq, kappa,
                       rowsum, f_var);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// The one driver of 2-layer models.  First-layer Jacobian blocks with a = idx[n] (plain models: q_{u,c} = d_u * w_c):
//   d f_c / d W_0 = sum_u P[a,u] q_{u,c} (x) e_u,   d f_c / d b_0 = sum_u P[a,u] rho_u q_{u,c}     (e, rho: as above)
//   d f_c / d W_r = sum_u P[a,u] q_{u,c} (x) x_u,   d f_c / d b_r = sum_u P[a,u] q_{u,c}           (res.0 reads X itself)
// (GraphSAGE: the node itself joins with weight 1 and the self half of W_1's row.)  The variance is the header's expression
// per block, the res.0 block one more tile term of the same shape.
// `table` (set by the entry point, not derived from the model): the rows come from the per-class table [needed nodes][C][H]
// of pred_q_kernel -- every Kronecker posterior and every call of lgnn_glm_variance_ext; otherwise (diagonal posterior
// through the plain entries) the kernel reads d_u in its loop and nothing is marked, compacted or built.
// Two passes over ONE table and ONE Zt buffer: conv pass (+ last layer), then -- models with res -- the res.0 pass.
// Kronecker: Zt = E Q_A0 resp. X Q_Ar in planes_a, and the table is rebuilt for the second rotation (q rows are cheap, the
// table is the workspace; the unrotated rows go through planes_b in chunks).  Diagonal posterior: both passes read the same
// unrotated table, and Zt is E resp. X where the forward left them.
int glm_variance_2layer(lgnn_ctx* h, const int64_t* idx, int64_t M, const GlmOperands& o, bool table, float* f_mu, float* f_var,
                        hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && o.S0 && o.S1 && o.kappa && f_var, "empty batch or null pointers");
  const bool kron = o.QA0 != nullptr;
  const bool sage = h->kind == LGNN_KIND_SAGE;
  const bool res = h->has_res;
  LGNN_REQUIRE(!kron || (o.QB0 && o.QA1 && o.QB1sq), "kron posterior needs all eigenvector matrices");
  LGNN_REQUIRE(table || (!kron && !h->extras()), "in-loop rows: the diagonal posterior of a model without res / norm");
  LGNN_REQUIRE((o.Sr != nullptr) == res, "Sr comes with a res model, and only with one");
  LGNN_REQUIRE(res && kron ? (o.QAr && o.QBr) : (!o.QAr && !o.QBr), "QAr / QBr: kron posterior of a res model only");
  LGNN_CALL(forward_ensure_aux(h, s));
  // F: width of what the first Linear multiplies (GraphSAGE: the concatenation), D1: the same for the last Linear
  const int64_t N = h->N, F = h->in_dim[0], Fx = h->dims[0], H = h->dims[1], Ce = h->dims[2], D1 = h->in_dim[1];
  LGNN_REQUIRE(H <= 256, "matrix-free GLM predictive: hidden width <= 256");
  LGNN_REQUIRE(o.W1m == nullptr || (o.Cm > 0 && o.Cm <= 4096), "mapped GLM predictive: 1 <= rows of the map <= 4096");
  const int64_t C = o.W1m ? o.Cm : Ce;           // output rows
  const float* W1 = o.W1m ? o.W1m : h->W[1];     // their head [C, in_dim_1]
  const int64_t ldw = h->in_dim[1], wn_off = sage ? H : 0;  // W_1 [C, ldw]; its neighbour half
  const int Hp = H <= 64 ? 64 : (H <= 128 ? 128 : 256);
  const int NG = 512 / Hp, CW = NG * PJT;
  const size_t smem = (size_t(PUC) * CW + PUC + size_t(C) + size_t(std::max<int64_t>(H, std::max(C, Ce))) + PUC) * 4;
  LGNN_REQUIRE(smem <= 150 * 1024, "matrix-free GLM predictive: tile does not fit LDS");
  int* bad = h->ws.flags.as<int>();
  if (f_mu) LGNN_CALL(launch_gather_rows(h->fc.out.as<float>(), Ce, N, idx, M, Ce, f_mu, bad + 2, s));

  // e_u = (P X)[u] / cat_0[u] and x_u (GraphSAGE: the first half of cat_0[u]) where the forward left them; the bias column
  // (rowsum(P) / 1) is read where it is used
  const float* xhat = sage ? h->fc.lin_in_p[0] : h->fc.prop_in[0].as<float>();
  const int64_t ldx = sage ? h->fc.lin_in_ld[0] : h->fc.prop_ld[0];
  const int64_t ldz = cdiv(F, 4) * 4;  // row stride of the rotated inputs (F >= F_x)
  LGNN_CALL(h->ws.planes_a.reserve((kron ? size_t(N) * ldz * 4 : 0) + size_t(M) * D1 * 4 * 2));
  h->ws.planes_a_zero_ptr = nullptr;
  float* Ztw = h->ws.planes_a.as<float>();  // [N, ldz] (kron)
  float* PhiB = Ztw + (kron ? N * ldz : 0);  // [M, D1] phi_a = (P H_1)[a] resp. cat_1[a] of the batch rows
  float* PhiT = PhiB + M * D1;               // [M, D1] rotated
  if (sage) LGNN_CALL(launch_gather_rows(h->fc.lin_in_p[1], h->fc.lin_in_ld[1], N, idx, M, D1, PhiB, bad + 2, s));
  else LGNN_CALL(launch_gather_rows(h->fc.prop_in[1].as<float>(), h->fc.prop_ld[1], N, idx, M, D1, PhiB, bad + 2, s));
  const float* Pt = PhiB;
  if (kron) { LGNN_CALL(sgemm_rm(s, M, D1, D1, 1.f, PhiB, D1, o.QA1, D1, 0.f, PhiT, D1)); Pt = PhiT; }

  // slots of the nodes whose rows are needed: the columns of the batch rows of P
  int32_t nneed = 0;
  int32_t* slot = nullptr;
  float* Rw = nullptr;
  float* Rsw = nullptr;
  const int64_t rows_s = sage ? M : 0;
  int64_t chunk = 0;
  if (table) {
    LGNN_CALL(h->ws.active.reserve(size_t(N)));
    LGNN_HIP_CHECK(hipMemsetAsync(h->ws.active.p, 0, size_t(N), s));
    hipLaunchKernelGGL(pred_mark_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, h->P.rowptr, h->P.col,
                       h->ws.active.as<uint8_t>(), bad);
    LGNN_CALL(compact_active_rows(h, s));
    LGNN_HIP_CHECK(hipMemcpyAsync(&nneed, h->ws.act_count.p, 4, hipMemcpyDeviceToHost, s));
    LGNN_HIP_CHECK(hipStreamSynchronize(s));  // the size of the table has to reach the host
    LGNN_CALL(h->ws.misc.reserve(size_t(N) * 4));
    slot = h->ws.misc.as<int32_t>();
    hipLaunchKernelGGL(pred_slots_kernel, dim3(unsigned(cdiv(std::max<int64_t>(nneed, 1), 256))), dim3(256), 0, s,
                       h->ws.act_list.as<int32_t>(), h->ws.act_count.as<int32_t>(), slot);
    const int64_t rows_r = std::max<int64_t>(nneed, 1);
    LGNN_CALL(h->ws.top.reserve(size_t(rows_r + rows_s) * C * H * 4));
    Rw = h->ws.top.as<float>();
    Rsw = Rw + rows_r * C * H;
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(nneed, rows_s), (int64_t(1) << 28) / (C * H)));  // <= 1 GiB operand
    if (kron) LGNN_CALL(h->ws.planes_b.reserve(size_t(chunk) * C * H * 4));
  }
  const float* gamma = h->norm != LGNN_NORM_NONE ? h->norm_w[0] : nullptr;
  const float* nxh = h->norm != LGNN_NORM_NONE ? h->fc.xhat[0].as<float>() : nullptr;
  const float* nrs = h->norm != LGNN_NORM_NONE ? h->fc.rstd[0].as<float>() : nullptr;
  // table[slot, c, :] = q_{u,c} (neighbour half of W_1) and, GraphSAGE, table_self[m, c, :] = q_{a,c} (self half); kron:
  // rotated by QB through planes_b, in chunks of nodes
  auto build_table = [&](const float* QB) -> int {
    for (int pass = 0; pass < 2; ++pass) {
      const int64_t total = pass == 0 ? nneed : rows_s;
      float* dst = pass == 0 ? Rw : Rsw;
      for (int64_t k0 = 0; k0 < total; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, total - k0);
        float* qrows = QB ? h->ws.planes_b.as<float>() : dst + k0 * C * H;
        hipLaunchKernelGGL(pred_q_kernel, dim3(unsigned(std::min<int64_t>(cdiv(kn * C, 4), 65536))), dim3(256), 0, s,
                           pass == 0 ? h->ws.act_list.as<int32_t>() : static_cast<const int32_t*>(nullptr), idx, k0, kn, N,
                           h->fc.dact0.as<float>(), H, pass == 0 ? W1 + wn_off : W1, ldw, C, h->norm, gamma, nxh, nrs, qrows);
        if (QB) LGNN_CALL(sgemm_rm(s, kn * C, H, H, 1.f, qrows, H, QB, H, 0.f, dst + k0 * C * H, H));
      }
    }
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  };

  // ---- conv pass: convs.0 (W_0 | b_0) and the last layer
  GlmVarArgs a{idx, M, N, h->P, slot, xhat, ldx, F + 1, Rw, Rsw, h->fc.dact0.as<float>(), W1, ldw, wn_off, H, C, Ce, Hp, o.S0,
               Pt, D1, o.S1, o.QB1sq, o.kappa, sage ? nullptr : h->fc.rowsum.as<float>(), f_var, smem};
  if (table) LGNN_CALL(build_table(kron ? o.QB0 : nullptr));
  if (kron) { LGNN_CALL(sgemm_rm(s, N, F, F, 1.f, xhat, ldx, o.QA0, F, 0.f, Ztw, ldz)); a.Zt = Ztw; a.ldz = ldz; }
  if (table) LGNN_CALL((launch_glm_var<Rows::Table, false>(kron, sage, a, s)));
  else LGNN_CALL((launch_glm_var<Rows::InLoop, false>(kron, sage, a, s)));
  // ---- res pass: res.0 (W_r | b_r), added to the conv pass's result
  if (res) {
    if (kron) LGNN_CALL(build_table(o.QBr));
    a.Zt = h->fc.lin_in_p[0]; a.ldz = h->fc.lin_in_ld[0]; a.F1 = Fx + 1; a.S0 = o.Sr; a.rowsum = nullptr;
    if (kron) { LGNN_CALL(sgemm_rm(s, N, Fx, Fx, 1.f, a.Zt, a.ldz, o.QAr, Fx, 0.f, Ztw, ldz)); a.Zt = Ztw; a.ldz = ldz; }
    LGNN_CALL((launch_glm_var<Rows::Table, true>(kron, sage, a, s)));
  }
  return 0;
}

// lgnn_glm_variance(_mapped): 1-layer models, and plain 2-layer models with the rows their posterior always had
int glm_variance_plain(lgnn_ctx* h, const int64_t* idx, int64_t M, const GlmOperands& o, float* f_mu, float* f_var,
                       hipStream_t s) {
  if (h->L == 1) {  // (W1m: the head of the map only feeds the first layer's terms; a one-layer model has none)
    LGNN_REQUIRE(!o.QA0 && !o.QB0 && !o.S0, "matrix-free GLM predictive, 1-layer models: the first-layer operands are null");
    return glm_variance_onelayer(h, idx, M, o.W1m ? o.Cm : 0, o.QA1, o.S1, o.QB1sq, o.kappa, f_mu, f_var, s);
  }
  LGNN_REQUIRE(h->L == 2, "matrix-free GLM predictive: 1- and 2-layer models");
  LGNN_REQUIRE(!h->extras(), "matrix-free GLM predictive: models without res / norm (use the Jacobian route)");
  return glm_variance_2layer(h, idx, M, o, /*table=*/o.QA0 != nullptr, f_mu, f_var, s);
}

// lgnn_glm_variance_ext: 2-layer models with res / norm and, through the same table route, plain ones
int glm_variance_ext(lgnn_ctx* h, const int64_t* idx, int64_t M, const GlmOperands& o, float* f_mu, float* f_var,
                     hipStream_t s) {
  LGNN_REQUIRE(h->L == 2, "matrix-free GLM predictive: 2-layer models");
  LGNN_REQUIRE(h->act == LGNN_ACT_RELU, "matrix-free GLM predictive with res / norm: ReLU models");
  return glm_variance_2layer(h, idx, M, o, /*table=*/true, f_mu, f_var, s);
}

}  // namespace

}  // namespace lgnn

extern "C" int lgnn_glm_variance(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* QA0, const float* QB0, const float* S0,
                                 const float* QA1, const float* S1, const float* QB1sq, const float* kappa, float* f_mu,
                                 float* f_var_diag, void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  return lgnn::glm_variance_plain(h, idx, M, {nullptr, 0, QA0, QB0, S0, QA1, S1, QB1sq, kappa, nullptr, nullptr, nullptr}, f_mu,
                                  f_var_diag, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_glm_variance_mapped(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* W1m, int64_t Cm, const float* QA0,
                                        const float* QB0, const float* S0, const float* QA1, const float* S1, const float* QB1sq,
                                        const float* kappa, float* f_mu, float* var_mapped, void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  if (!W1m) { lgnn::set_error("lgnn_glm_variance_mapped: null head of the map"); return 2; }
  return lgnn::glm_variance_plain(h, idx, M, {W1m, Cm, QA0, QB0, S0, QA1, S1, QB1sq, kappa, nullptr, nullptr, nullptr}, f_mu,
                                  var_mapped, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_glm_variance_ext(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* W1m, int64_t Cm, const float* QA0,
                                     const float* QB0, const float* S0, const float* QA1, const float* S1, const float* QB1sq,
                                     const float* kappa, const float* QAr, const float* QBr, const float* Sr, float* f_mu,
                                     float* f_var, void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  if (!W1m && Cm != 0) { lgnn::set_error("lgnn_glm_variance_ext: rows of a map without its head"); return 2; }
  return lgnn::glm_variance_ext(h, idx, M, {W1m, Cm, QA0, QB0, S0, QA1, S1, QB1sq, kappa, QAr, QBr, Sr}, f_mu, f_var,
                                static_cast<hipStream_t>(stream));
}
