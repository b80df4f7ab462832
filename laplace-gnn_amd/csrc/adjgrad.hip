// Gradient of the negative log marginal likelihood of a KronLaplace fit w.r.t. the adjacency ("next" row 8(f)-4).
//
// Reference: gnn/marglik_training.py:197-216 calls ``neg_marglik.backward()`` and steps an optimiser on ``model.adj``:
// autograd walks back through log_marginal_likelihood (laplace/baselaplace.py:938-973), the eigendecomposed factors
// (laplace/utils/matrix.py:118-145, 371-394), the KFAC accumulation that the fork keeps attached to the graph
// (curvlinops/kfac.py:637-661 non-detached Hessian square root + create_graph=True, :789-790 / :836-837 clone instead
// of detach), three dense full-graph forwards, normalize_adj (gnn/models/utils.py:106-112) and the straight-through
// binarisation (gnn/models/utils.py:42-86, gnn/models/models.py:103-118).
//
// Here the same chain runs in reverse as explicit kernels on the stored sparsity pattern (2-layer GCN, ReLU):
//   host (python):   Gamma_B_l = d(neg marglik)/dB_l, Gamma_A_l = d/dA_l from the eigenpairs of the fitted factors
//   per batch:       seeds V, g1 = P^T scatter(V), u = mask * (g1 W1), g0 = P^T u               (kfac.hip's chain)
//                    g0bar = 2 g0 Gamma_B0            gradP[(a,b)] += <u[a], g0bar[b]>             SDDMM, 256 wide
//                    ubar  = mask * (P g0bar)         g1bar = ubar W1^T + 2 g1 Gamma_B1
//                    gradP[(a,b)] += <G[a], g1bar[b]> (a in batch)      Vbar = (P g1bar)[batch]  SDDMM + row gather
//                    fbar = dV/df . Vbar (the fork's attached square root) + softmax - onehot      outbar[batch] += fbar
//   once per fit:    gradP += <outbar[a], Z1[b]>;  H1bar = (P^T outbar) W1 + 2 (T/N) H1 Gamma_A1
//                    gradP += <(mask * H1bar)[a], Z0[b]>
//                    normalize_adj backward: P[a,b] = d_a A[b,a] d_b, d = rowsum(A)^-1/2; diagonal -> 0 (overwritten
//                    by fill_diagonal_(1) after the STE); symmetric models average (i,j) and (j,i)
// The dense GEMMs with the (small) Gamma / weight matrices are plain library calls (rocBLAS).
//
// This file: the kernels and launchers every model family shares, the once-per-fit finish, the dispatchers and the C entry
// points.  The families' own kernels and batch chains: adjgrad_gcn.hip (the chain above), adjgrad_sage.hip, adjgrad_ext.hip
// (res / norm, and the per-sample planes chain), adjgrad_diag.hip (diagonal posterior, closed form), adjgrad_onelayer.hip.
#include <rocblas/rocblas.h>

#include "adjgrad.h"
#include "device_utils.h"

namespace lgnn {

namespace {

// out[p] += sum_planes <L_c[a, :], R_c[b, :]> for every stored entry p = (a, b) of the CSR, rows a from an optional list.
// LPR lanes (a power of two >= width / 4, at most 64) share an entry; 64 / LPR entries are in flight per wave.
template <int LPR>
__global__ __launch_bounds__(256) void sddmm_planes_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           int64_t nrows, const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ nrows_dev,
                                                           const float* __restrict__ Lp, int64_t l_ld, int64_t l_stride,
                                                           const float* __restrict__ Rp, int64_t r_ld, int64_t r_stride,
                                                           int64_t width, int64_t nplanes, float* __restrict__ out) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, sl = lane % LPR;
  const int64_t total = rows ? int64_t(*nrows_dev) : nrows;
  for (int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); w < total; w += int64_t(gridDim.x) * 4) {
    const int64_t a = rows ? rows[w] : w;
    const int32_t s = rowptr[a], e = rowptr[a + 1];
    for (int32_t p0 = s; p0 < e; p0 += EPW) {
      const int32_t p = p0 + sub;
      const bool ok = p < e;
      const int64_t b = ok ? col[p] : 0;
      float acc = 0.f;
      // (small graphs with many planes -- the (sample, class) planes of the res / norm diagonal route: blockIdx.y splits the
      //  planes so that the launch fills the device; the parts meet in out[p] through float atomics)
      const int64_t cper = (nplanes + gridDim.y - 1) / gridDim.y;
      const int64_t cb = int64_t(blockIdx.y) * cper, ce = cb + cper < nplanes ? cb + cper : nplanes;
      for (int64_t c = cb; c < ce; ++c) {
        const float* __restrict__ lrow = Lp + c * l_stride + a * l_ld;
        const float* __restrict__ rrow = Rp + c * r_stride + b * r_ld;
        for (int64_t k = sl; k < width; k += LPR) acc += ok ? lrow[k] * rrow[k] : 0.f;
      }
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (ok && sl == 0) {
        if (gridDim.y > 1) atomicAdd(&out[p], acc);
        else out[p] += acc;  // one wave owns row a: a single writer per entry inside a launch
      }
    }
  }
}

// The same contraction on an arbitrary list of (a, b) pairs (candidate edges that are NOT stored: the reference's dense
// adj.grad has an entry for every pair, which is how its structure learning proposes new edges).
template <int LPR>
__global__ __launch_bounds__(256) void sddmm_coo_kernel(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb, int64_t K,
                                                        const float* __restrict__ Lp, int64_t l_ld, int64_t l_stride,
                                                        const float* __restrict__ Rp, int64_t r_ld, int64_t r_stride,
                                                        int64_t width, int64_t nplanes, const uint8_t* __restrict__ a_active,
                                                        float* __restrict__ out) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, sl = lane % LPR;
  const int64_t k = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * EPW + sub;
  const bool ok = k < K;
  const int64_t a = ok ? ca[k] : 0, b = ok ? cb[k] : 0;
  float acc = 0.f;
  if (ok && (a_active == nullptr || a_active[a])) {
    for (int64_t c = 0; c < nplanes; ++c) {
      const float* __restrict__ lrow = Lp + c * l_stride + a * l_ld;
      const float* __restrict__ rrow = Rp + c * r_stride + b * r_ld;
      for (int64_t q = sl; q < width; q += LPR) acc += lrow[q] * rrow[q];
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (ok && sl == 0) out[k] += acc;
}

// candidate pairs against the scattered seed planes: only pairs whose a is a batch node contribute
__global__ __launch_bounds__(256) void sddmm_coo_seed_kernel(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb,
                                                             int64_t K, int64_t N, int64_t C, const int32_t* __restrict__ pos,
                                                             const float* __restrict__ seeds, const float* __restrict__ g1bar,
                                                             int64_t c0, int64_t cc, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t k = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  const int64_t a = ca[k], b = cb[k];
  const int32_t m = pos[a];
  if (m == INT32_MAX) return;
  const float* __restrict__ sd = seeds + int64_t(m) * C * C + c0 * C;
  const int64_t nq = cc * C;
  float acc = 0.f;
  for (int64_t q = lane; q < nq; q += 64) {
    const int64_t c = q / C, kk = q - c * C;
    acc += sd[q] * g1bar[(c * N + b) * C + kk];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) out[k] += acc;
}

// candidate (a, b) of P = entry (i = b, j = a) of A:  gA = gP d_i d_j - 1/2 d_i^2 (rs[i] + cs[i]);  i == j -> 0
__global__ void cand_adj_grad_kernel(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb, int64_t K,
                                     const int32_t* __restrict__ a_rowptr, const float* __restrict__ gPc,
                                     const float* __restrict__ rs, const float* __restrict__ cs, float* __restrict__ out) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int64_t j = ca[k], i = cb[k];
  if (i == j) { out[k] = 0.f; return; }
  const float di = rsqrtf(float(a_rowptr[i + 1] - a_rowptr[i])), dj = rsqrtf(float(a_rowptr[j + 1] - a_rowptr[j]));
  out[k] = gPc[k] * di * dj - 0.5f * di * di * (rs[i] + cs[i]);
}

// gradP[(a, b)] += sum_{c in [c0, c0+cc)} sum_k seeds[m][c][k] * g1bar[c - c0][b][k]  for the first occurrence m of every
// batch node a = idx[m] (the scattered seed planes G_c are non-zero on those rows only and hold the accumulated seeds of
// duplicated node ids).  One wave per sample; lanes over (c, k).
__global__ __launch_bounds__(256) void sddmm_seed_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const int64_t* __restrict__ idx, int64_t M, int64_t N, int64_t C,
                                                         const int32_t* __restrict__ pos, const float* __restrict__ seeds,
                                                         const float* __restrict__ g1bar, int64_t c0, int64_t cc,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t a = idx[m];
  if (a < 0 || a >= N || pos[a] != m) return;  // duplicates: the first occurrence owns the accumulated seed row
  const float* __restrict__ sd = seeds + m * C * C + c0 * C;
  const int64_t nq = cc * C;
  for (int32_t p = rowptr[a]; p < rowptr[a + 1]; ++p) {
    const int64_t b = col[p];
    float acc = 0.f;
    for (int64_t q = lane; q < nq; q += 64) {
      const int64_t c = q / C, k = q - c * C;
      acc += sd[q] * g1bar[(c * N + b) * C + k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[p] += acc;
  }
}

// Vbar[m][c0 + c][k] = sum_b P[a, b] * g1bar[c][b][k], a = idx[m] (every sample, duplicates included)
__global__ __launch_bounds__(256) void seed_adjoint_gather_kernel(const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ col,
                                                                  const float* __restrict__ val,
                                                                  const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                                  int64_t C, const float* __restrict__ g1bar, int64_t c0,
                                                                  int64_t cc, float* __restrict__ vbar) {
  const int64_t nq = cc * C;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * nq) return;
  const int64_t m = t / nq, q = t - m * nq;
  const int64_t c = q / C, k = q - c * C;
  const int64_t a = idx[m];
  if (a < 0 || a >= N) return;
  float acc = 0.f;
  for (int32_t p = rowptr[a]; p < rowptr[a + 1]; ++p) acc += val[p] * g1bar[(c * N + col[p]) * C + k];
  vbar[m * C * C + (c0 + c) * C + k] = acc;
}

// fbar_m = d/df sum_{k,c} Vbar[k,c] V[k,c](f) + softmax(f) - onehot(y); outbar[idx[m]] += fbar_m.  One wave per sample.
// V[k,c] = alpha_c d_kc - beta_c u_k - gamma_c p_k (alpha = s (1 + t/2), beta = s, gamma = s t / 2, s = sqrt(p),
// t = f - mbar, u = p (1 + t)).  With dp_k/df_m = p_k (d_km - p_m), dmbar/df_m = u_m, ds_c/df_m = s_c (d_cm - p_m) / 2:
//   fbar_m = e1_m + e2_m - p_m sum(e1) - u_m sum(e2) - rho_m (u_m + p_m) + p_m <rho, u> + u_m <rho, p> - sigma_m p_m + p_m <sigma, p>
//   e1 = (Psi_cc alpha - r s - q gamma) / 2, e2 = s (Psi_cc - q) / 2, r_c = sum_k Psi_kc u_k, q_c = sum_k Psi_kc p_k,
//   rho_k = sum_c beta_c Psi_kc, sigma_k = sum_c gamma_c Psi_kc      (Psi = Vbar).
__global__ __launch_bounds__(256) void seed_adjoint_kernel(const float* __restrict__ logits, const float* __restrict__ probs,
                                                           const int64_t* __restrict__ idx, const int64_t* __restrict__ y,
                                                           int64_t M, int64_t N, int64_t C, const float* __restrict__ vbar,
                                                           int fork_exact, float loss_scale, float* __restrict__ outbar) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m = int64_t(blockIdx.x) * 4 + wave;
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) return;
  float* __restrict__ p_s = sm + size_t(wave) * 8 * C;  // p, u, s, alpha, gamma, rho, sigma, diag
  float* __restrict__ u_s = p_s + C;
  float* __restrict__ s_s = u_s + C;
  float* __restrict__ al_s = s_s + C;
  float* __restrict__ ga_s = al_s + C;
  float* __restrict__ rho_s = ga_s + C;
  float* __restrict__ sig_s = rho_s + C;
  float mb = 0.f;
  for (int64_t k = lane; k < C; k += 64) mb += probs[m * C + k] * logits[n * C + k];
  mb = wave_sum(mb);
  for (int64_t k = lane; k < C; k += 64) {
    const float p = probs[m * C + k], t = logits[n * C + k] - mb, s = sqrtf(p);
    p_s[k] = p; u_s[k] = p * (1.f + t); s_s[k] = s; al_s[k] = s * (1.f + 0.5f * t); ga_s[k] = 0.5f * s * t;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* __restrict__ vb = vbar + m * C * C;  // vb[c * C + k] = Psi[k, c]
  const int64_t yy = y[m];
  float se1 = 0.f, se2 = 0.f, sru = 0.f, srp = 0.f, ssp = 0.f;
  if (fork_exact) {
    // rho_k = sum_c beta_c Psi_kc, sigma_k = sum_c gamma_c Psi_kc  (lane = k)
    for (int64_t k = lane; k < C; k += 64) {
      float rho = 0.f, sig = 0.f;
      for (int64_t c = 0; c < C; ++c) {
        const float ps = vb[c * C + k];
        rho += s_s[c] * ps;
        sig += ga_s[c] * ps;
      }
      rho_s[k] = rho; sig_s[k] = sig;
      sru += rho * u_s[k]; srp += rho * p_s[k]; ssp += sig * p_s[k];
    }
    sru = wave_sum(sru); srp = wave_sum(srp); ssp = wave_sum(ssp);
  }
  // e1_c, e2_c (lane = c): r_c = sum_k Psi_kc u_k, q_c = sum_k Psi_kc p_k
  float e1_l[4], e2_l[4];  // C <= 256
  int nl = 0;
  for (int64_t c = lane; c < C; c += 64, ++nl) {
    float e1 = 0.f, e2 = 0.f;
    if (fork_exact) {
      float r = 0.f, q = 0.f;
      for (int64_t k = 0; k < C; ++k) {
        const float ps = vb[c * C + k];
        r += ps * u_s[k];
        q += ps * p_s[k];
      }
      const float dg = vb[c * C + c];
      e1 = 0.5f * (dg * al_s[c] - r * s_s[c] - q * ga_s[c]);
      e2 = 0.5f * s_s[c] * (dg - q);
    }
    e1_l[nl] = e1; e2_l[nl] = e2;
    se1 += e1; se2 += e2;
  }
  se1 = wave_sum(se1); se2 = wave_sum(se2);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  nl = 0;
  for (int64_t k = lane; k < C; k += 64, ++nl) {
    const float p = p_s[k], u = u_s[k];
    float fb = loss_scale * (p - (k == yy ? 1.f : 0.f));  // d (H_factor * CE) / d f
    if (fork_exact)
      fb += e1_l[nl] + e2_l[nl] - p * se1 - u * se2 - rho_s[k] * (u + p) + p * sru + u * srp - sig_s[k] * p + p * ssp;
    atomicAdd(&outbar[n * C + k], fb);
  }
}

__global__ void relu_mask_inplace_kernel(float* __restrict__ x, const float* __restrict__ h, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride) x[q] = h[q] > 0.f ? x[q] : 0.f;
}

// rs[a] = sum_b gP[a,b] P[a,b], cs[b] += the same (column sums): d J / d d_i = (rs[i] + cs[i]) / d_i
__global__ void gp_rowcol_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                 const float* __restrict__ val, const float* __restrict__ gP, int64_t N,
                                 float* __restrict__ rs, float* __restrict__ cs) {
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a >= N) return;
  float acc = 0.f;
  for (int32_t p = rowptr[a]; p < rowptr[a + 1]; ++p) {
    const float t = gP[p] * val[p];
    acc += t;
    atomicAdd(&cs[col[p]], t);
  }
  rs[a] = acc;
}

__device__ __forceinline__ int32_t find_col(const int32_t* __restrict__ col, int32_t s, int32_t e, int32_t want) {
  while (s < e) {  // sorted columns inside a row
    const int32_t mid = (s + e) >> 1;
    if (col[mid] < want) s = mid + 1;
    else e = mid;
  }
  return s;
}

// Entry p = (i, j) of the stored 0/1 adjacency A (row-major, lgnn_export_adj order):
//   gA[p] = gP[(j, i)] d_i d_j - 1/2 d_i^2 (rs[i] + cs[i]),   d = rowsum(A)^-1/2,   P = D A^T D;   diagonal -> 0
__global__ void adj_grad_kernel(const int32_t* __restrict__ a_rowptr, const int32_t* __restrict__ a_col,
                                const int32_t* __restrict__ p_rowptr, const int32_t* __restrict__ p_col,
                                const float* __restrict__ gP, const float* __restrict__ rs, const float* __restrict__ cs,
                                int64_t N, float* __restrict__ gA) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t s = a_rowptr[i], e = a_rowptr[i + 1];
  if (s == e) return;
  const float di = rsqrtf(float(e - s));
  const float rowterm = -0.5f * di * di * (rs[i] + cs[i]);
  for (int32_t p = s; p < e; ++p) {
    const int32_t j = a_col[p];
    if (j == i) { gA[p] = 0.f; continue; }
    const int32_t js = p_rowptr[j], je = p_rowptr[j + 1];
    const int32_t q = find_col(p_col, js, je, int32_t(i));  // P has the entry (j, i) exactly when A has (i, j)
    const float dj = rsqrtf(float(a_rowptr[j + 1] - a_rowptr[j]));
    gA[p] = gP[q] * di * dj + rowterm;
  }
}

// symmetric models propagate with (adj + adj^T) / 2: the parameter's gradient is the average of (i, j) and (j, i)
__global__ void adj_grad_symmetrize_kernel(const int32_t* __restrict__ a_rowptr, const int32_t* __restrict__ a_col,
                                           const float* __restrict__ gA, int64_t N, float* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int32_t p = a_rowptr[i]; p < a_rowptr[i + 1]; ++p) {
    const int32_t j = a_col[p];
    const int32_t q = find_col(a_col, a_rowptr[j], a_rowptr[j + 1], int32_t(i));
    out[p] = 0.5f * (gA[p] + gA[q]);
  }
}

// GCN top layer, all N rows (kfac_top.hip's unfused seed SpMM restated here with the planes of a class chunk only)
__global__ void seed_planes_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                   const float* __restrict__ val, int64_t N, int64_t C, const int32_t* __restrict__ pos,
                                   const float* __restrict__ seeds, float* __restrict__ g, uint8_t* __restrict__ active) {
  // g[c][n][k] = sum_{v in row n of P^T, v in batch} val * seeds[pos[v]][c][k]; one wave per node
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n >= N) return;
  const int64_t CC = C * C;
  bool any = false;
  for (int64_t q0 = 0; q0 < CC; q0 += 64) {
    const int64_t q = q0 + lane;
    float acc = 0.f;
    for (int32_t p = rowptr[n]; p < rowptr[n + 1]; ++p) {
      const int32_t mp = pos[col[p]];
      if (mp != INT32_MAX) {
        any = true;
        if (q < CC) acc += val[p] * seeds[int64_t(mp) * CC + q];
      }
    }
    if (q < CC) {
      const int64_t c = q / C, k = q - c * C;
      g[(c * N + n) * C + k] = acc;
    }
  }
  if (lane == 0) active[n] = any ? 1 : 0;
}

__global__ void add_inplace_kernel(float* __restrict__ x, const float* __restrict__ y, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride) x[q] += y[q];
}

// gradP[p] += c[a] for every entry p of row a (c has row stride ld);  candidates (a, b): grad_cand[k] += c[a]
__global__ __launch_bounds__(256) void row_const_kernel(const int32_t* __restrict__ rowptr, int64_t N, const float* __restrict__ c,
                                                        int64_t ld, float* __restrict__ gradP, const int32_t* __restrict__ ca,
                                                        int64_t K, float* __restrict__ grad_cand) {
  const int lane = threadIdx.x & 63;
  const int64_t a = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (a < N) {
    const float v = c[a * ld];
    for (int32_t p = rowptr[a] + lane; p < rowptr[a + 1]; p += 64) gradP[p] += v;
  }
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < K; k += stride) grad_cand[k] += c[int64_t(ca[k]) * ld];
}

}  // namespace

int launch_sddmm(const Csr& m, int64_t nrows, const int32_t* rows, const int32_t* nrows_dev, const float* L, int64_t l_ld,
                 int64_t l_stride, const float* R, int64_t r_ld, int64_t r_stride, int64_t width, int64_t nplanes,
                 float* out, hipStream_t s) {
  if (nrows <= 0 || width <= 0 || nplanes <= 0) return 0;
  const unsigned gx = unsigned(std::min<int64_t>(cdiv(nrows, 4), 8192));
  const unsigned gy = unsigned(std::max<int64_t>(1, std::min<int64_t>({nplanes, cdiv(2048, gx), int64_t(1024)})));
  const dim3 grid{gx, gy, 1};
#define LGNN_SDDMM(LPRV)                                                                                           \
  hipLaunchKernelGGL(sddmm_planes_kernel<LPRV>, grid, dim3(256), 0, s, m.rowptr, m.col, nrows, rows, nrows_dev, \
                     L, l_ld, l_stride, R, r_ld, r_stride, width, nplanes, out)
  if (width <= 8) LGNN_SDDMM(8);
  else if (width <= 16) LGNN_SDDMM(16);
  else if (width <= 32) LGNN_SDDMM(32);
  else LGNN_SDDMM(64);
#undef LGNN_SDDMM
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_sddmm_coo(const int32_t* ca, const int32_t* cb, int64_t K, const float* L, int64_t l_ld, int64_t l_stride,
                     const float* R, int64_t r_ld, int64_t r_stride, int64_t width, int64_t nplanes, const uint8_t* a_active,
                     float* out, hipStream_t s) {
  if (K <= 0 || width <= 0 || nplanes <= 0) return 0;
#define LGNN_SDDMM_COO(LPRV)                                                                                               \
  hipLaunchKernelGGL(sddmm_coo_kernel<LPRV>, dim3(unsigned(cdiv(K, 4 * (64 / LPRV)))), dim3(256), 0, s, ca, cb, K, L, l_ld, \
                     l_stride, R, r_ld, r_stride, width, nplanes, a_active, out)
  if (width <= 8) LGNN_SDDMM_COO(8);
  else if (width <= 16) LGNN_SDDMM_COO(16);
  else if (width <= 32) LGNN_SDDMM_COO(32);
  else LGNN_SDDMM_COO(64);
#undef LGNN_SDDMM_COO
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// C_rm[R, Nout] = alpha * A_rm[R, K] * B_rm[K, Nout] + beta * C_rm   (row major through the column-major library call)
int sgemm_rm(hipStream_t s, int64_t R, int64_t Nout, int64_t K, float alpha, const float* A, int64_t lda, const float* B,
             int64_t ldb, float beta, float* Cm, int64_t ldc) {
  rocblas_handle blas = static_cast<rocblas_handle>(blas_handle(s));
  LGNN_REQUIRE(blas != nullptr, "rocBLAS handle");
  LGNN_REQUIRE(R < (int64_t(1) << 31) && Nout < (int64_t(1) << 31) && K < (int64_t(1) << 31), "sgemm: dimension too large");
  const rocblas_status st = rocblas_sgemm(blas, rocblas_operation_none, rocblas_operation_none, rocblas_int(Nout),
                                          rocblas_int(R), rocblas_int(K), &alpha, B, rocblas_int(ldb), A, rocblas_int(lda),
                                          &beta, Cm, rocblas_int(ldc));
  if (st != rocblas_status_success) { set_error("rocblas_sgemm failed"); return 3; }
  return 0;
}

int check_model(const lgnn_ctx* h) {
  LGNN_REQUIRE(h->L == 2, "adjacency gradient: 1- and 2-layer models (SURVEY.md 8(f)-4)");
  LGNN_REQUIRE(!h->extras(), "adjacency gradient: models without res / norm");
  LGNN_REQUIRE(h->act == LGNN_ACT_RELU && h->lik == LGNN_LIK_CLASSIFICATION, "adjacency gradient: ReLU, classification");
  LGNN_REQUIRE(h->dims[2] <= 256, "adjacency gradient: at most 256 classes");
  LGNN_REQUIRE(h->kind == LGNN_KIND_GCN || (h->dims[1] % 4 == 0 && h->dims[1] <= 256),
               "adjacency gradient, GraphSAGE: hidden width a multiple of 4, at most 256");
  return 0;
}

int launch_gp_rowcol(lgnn_ctx* h, const float* gP, float* rs, float* cs, hipStream_t s) {
  hipLaunchKernelGGL(gp_rowcol_kernel, dim3(unsigned(cdiv(h->N, 256))), dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.val, gP,
                     h->N, rs, cs);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_seed_planes(lgnn_ctx* h, float* g, hipStream_t s) {
  hipLaunchKernelGGL(seed_planes_kernel, dim3(unsigned(cdiv(h->N, 4))), dim3(256), 0, s, h->PT.rowptr, h->PT.col, h->PT.val, h->N,
                     h->dims[h->L], h->ws.pos.as<int32_t>(), h->ws.seeds.as<float>(), g, h->ws.active.as<uint8_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_seed_sddmm(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* g1bar, int64_t c0, int64_t cc, float* grad_P,
                      const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s) {
  const int64_t N = h->N, C = h->dims[h->L];
  if (grad_P)
    hipLaunchKernelGGL(sddmm_seed_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, h->P.rowptr, h->P.col, idx, M, N, C,
                       h->ws.pos.as<int32_t>(), h->ws.seeds.as<float>(), g1bar, c0, cc, grad_P);
  if (K > 0)
    hipLaunchKernelGGL(sddmm_coo_seed_kernel, dim3(unsigned(cdiv(K, 4))), dim3(256), 0, s, cand_a, cand_b, K, N, C,
                       h->ws.pos.as<int32_t>(), h->ws.seeds.as<float>(), g1bar, c0, cc, grad_cand);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_seed_gather(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* g1bar, int64_t c0, int64_t cc, float* vbar,
                       hipStream_t s) {
  const int64_t C = h->dims[h->L];
  hipLaunchKernelGGL(seed_adjoint_gather_kernel, dim3(unsigned(cdiv(M * cc * C, 256))), dim3(256), 0, s, h->P.rowptr, h->P.col,
                     h->P.val, idx, M, h->N, C, g1bar, c0, cc, vbar);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_seed_adjoint(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* vbar, bool fork_exact,
                        float loss_scale, float* out_bar, hipStream_t s) {
  const int64_t C = h->dims[h->L];
  LGNN_REQUIRE(size_t(4) * 8 * C * 4 <= 64 * 1024, "too many classes for the seed adjoint kernel");
  hipLaunchKernelGGL(seed_adjoint_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), size_t(4) * 8 * C * 4, s,
                     h->fc.out.as<float>(), h->ws.probs.as<float>(), idx, static_cast<const int64_t*>(y), M, h->N, C, vbar,
                     fork_exact ? 1 : 0, loss_scale, out_bar);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_adj_grad_symmetrize(const Csr& a, const float* gA, int64_t N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(adj_grad_symmetrize_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, a.rowptr, a.col, gA, N, out);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_row_const(lgnn_ctx* h, const float* c, int64_t ld, float* grad_P, const int32_t* cand_a, int64_t K, float* grad_cand,
                     hipStream_t s) {
  hipLaunchKernelGGL(row_const_kernel, dim3(unsigned(cdiv(h->N, 4))), dim3(256), 0, s, h->P.rowptr, h->N, c, ld, grad_P, cand_a, K,
                     grad_cand);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// dense != null (plain 2-layer GCN, lgnn_kfac_adjgrad_batch_dense): every candidate-pair term is also added on the full grid,
// dense[a * N + b] += d/dP[a, b] (lora.hip's tile GEMMs); everything is then defined on all N rows as with candidates.
int kfac_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags, const float* gamma_B0,
                       const float* gamma_B1, const float* gamma_Br, float loss_scale, float* grad_P, float* out_bar,
                       const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s,
                       float* dense = nullptr) {
  LGNN_REQUIRE(K == 0 || (cand_a && cand_b && grad_cand), "candidate pairs without their buffers");
  if (h->L == 1)  // gamma_B holds one pointer
    return onelayer_kfac_adjgrad_batch(h, idx, y, M, flags, gamma_B0, loss_scale, grad_P, out_bar, cand_a, cand_b, K, grad_cand, s);
  LGNN_REQUIRE(M > 0 && idx && y && gamma_B0 && gamma_B1 && grad_P && out_bar, "empty batch or null pointers");
  if (h->extras())
    return kfac_adjgrad_batch_ext(h, idx, y, M, (flags & LGNN_FLAG_FORK_EXACT_SEED) != 0, gamma_B0, gamma_B1, gamma_Br,
                                  loss_scale, grad_P, out_bar, cand_a, cand_b, K, grad_cand, s);
  LGNN_CALL(check_model(h));
  LGNN_CALL(forward_ensure_aux(h, s));  // act'(h_1) is part of the auxiliary forward products
  LGNN_CALL(ensure_wt(h, s));
  const bool fork_exact = (flags & LGNN_FLAG_FORK_EXACT_SEED) != 0;
  if (h->kind == LGNN_KIND_SAGE)
    return sage_adjgrad_batch(h, idx, y, M, fork_exact, gamma_B0, gamma_B1, loss_scale, grad_P, out_bar, cand_a, cand_b, K,
                              grad_cand, s);
  return kfac_adjgrad_batch_gcn(h, idx, y, M, fork_exact, gamma_B0, gamma_B1, loss_scale, grad_P, out_bar, cand_a, cand_b, K,
                                grad_cand, s, dense);
}

// normalize_adj backward + the straight-through binarisation: d/dP on the stored entries (and the candidates) -> d/dA
int normalize_adj_backward(lgnn_ctx* h, const float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b,
                           int64_t K, const float* grad_cand, float* grad_cand_adj, hipStream_t s) {
  const int64_t N = h->N;
  LGNN_CALL(h->ws.misc.reserve(size_t(2) * N * 4 + size_t(h->nnz) * 4));
  float* rs = h->ws.misc.as<float>();
  float* cs = rs + N;
  float* tmp = cs + N;
  LGNN_HIP_CHECK(hipMemsetAsync(cs, 0, size_t(N) * 4, s));
  hipLaunchKernelGGL(gp_rowcol_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.val, grad_P,
                     N, rs, cs);
  float* first = h->sym ? tmp : grad_adj;
  hipLaunchKernelGGL(adj_grad_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->A.rowptr, h->A.col, h->P.rowptr,
                     h->P.col, grad_P, rs, cs, N, first);
  if (h->sym)
    hipLaunchKernelGGL(adj_grad_symmetrize_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->A.rowptr, h->A.col, tmp,
                       N, grad_adj);
  if (K > 0)  // candidates: un-symmetrised d/dA[i, j]; a symmetric model's caller passes both orientations and averages
    hipLaunchKernelGGL(cand_adj_grad_kernel, dim3(unsigned(cdiv(K, 256))), dim3(256), 0, s, cand_a, cand_b, K, h->A.rowptr,
                       grad_cand, rs, cs, grad_cand_adj);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int diag_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, float loss_scale,
                       float* grad_P, float* out_bar, float* h1_bar, float* e_bar, const int32_t* cand_a, const int32_t* cand_b,
                       int64_t K, float* grad_cand, hipStream_t s, float* dense = nullptr) {
  LGNN_REQUIRE(K == 0 || (cand_a && cand_b && grad_cand), "candidate pairs without their buffers");
  if (h->L == 1)  // (grad_P and the candidates take their terms in the finish; h1_bar is ignored)
    return onelayer_diag_adjgrad_batch(h, idx, y, M, gamma, loss_scale, out_bar, e_bar, s);
  if (h->kind == LGNN_KIND_SAGE)  // (e_bar [N, F + 1] carries the adjoint of P X in its first F columns)
    return persample_adjgrad_batch_sage(h, idx, y, M, gamma, nullptr, loss_scale, grad_P, out_bar, h1_bar, e_bar, cand_a, cand_b,
                                        K, grad_cand, s);
  if (h->extras())  // res / norm: no closed form, (sample, class) planes (e_bar stays untouched)
    return persample_adjgrad_batch_ext(h, idx, y, M, gamma, nullptr, loss_scale, grad_P, out_bar, h1_bar, cand_a, cand_b, K,
                                       grad_cand, s);
  return diag_adjgrad_batch_gcn(h, idx, y, M, gamma, loss_scale, grad_P, out_bar, h1_bar, e_bar, cand_a, cand_b, K, grad_cand, s,
                                dense);
}

// The full posterior's product kernel holds whole samples in a 128-row tile (fulladj.hip): refused here, up front, so that the
// refusal costs no Jacobian pass (check_model_ext alone admits up to 256 classes)
static int check_full_classes(const lgnn_ctx* h) {
  LGNN_REQUIRE(h->L >= 1 && h->dims[h->L] <= 127, "adjacency gradient, full posterior: at most 127 classes");
  return 0;
}

// Full posterior (FullLaplace): the (sample, class) chains of the diagonal posterior with the dense Gamma [P, P] as weighting.
// 2-layer GCN, plain or with res / norm: the planes chain (e_bar stays untouched); plain 2-layer GraphSAGE: the local chain.
int full_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* Gamma, float loss_scale,
                       float* grad_P, float* out_bar, float* h1_bar, float* e_bar, const int32_t* cand_a, const int32_t* cand_b,
                       int64_t K, float* grad_cand, hipStream_t s) {
  LGNN_REQUIRE(K == 0 || (cand_a && cand_b && grad_cand), "candidate pairs without their buffers");
  LGNN_REQUIRE(Gamma && e_bar, "empty batch or null pointers");
  LGNN_CALL(check_full_classes(h));  // before any launch or workspace reservation
  if (h->L == 1) return onelayer_full_adjgrad_batch(h, idx, y, M, Gamma, loss_scale, out_bar, e_bar, s);
  if (h->kind == LGNN_KIND_SAGE)
    return persample_adjgrad_batch_sage(h, idx, y, M, nullptr, Gamma, loss_scale, grad_P, out_bar, h1_bar, e_bar, cand_a, cand_b,
                                        K, grad_cand, s);
  return persample_adjgrad_batch_ext(h, idx, y, M, nullptr, Gamma, loss_scale, grad_P, out_bar, h1_bar, cand_a, cand_b, K,
                                     grad_cand, s);
}

// The product alone: K_out [M, C, C] = J_m Gamma J_m^T and R_out [M, C, P] = 2 Lambda_m J_m Gamma, in the chunks of the batch
// call (only the Jacobian rows of a chunk live in the workspace)
int full_directions(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* Gamma, float* K_out, float* R_out, hipStream_t s) {
  LGNN_REQUIRE(M > 0 && idx && Gamma && K_out && R_out, "empty batch or null pointers");
  LGNN_CALL(check_full_classes(h));
  const bool sage = h->kind == LGNN_KIND_SAGE;
  if (sage) {
    LGNN_REQUIRE(h->L == 2 && !h->extras(), "adjacency gradient, diagonal / full posterior, GraphSAGE: plain 2-layer models");
    LGNN_REQUIRE(h->act == LGNN_ACT_RELU && h->lik == LGNN_LIK_CLASSIFICATION, "adjacency gradient: ReLU, classification");
  } else if (h->L == 1) {
    LGNN_CALL(check_model_onelayer(h));
  } else {
    LGNN_CALL(check_model_ext(h));
  }
  LGNN_CALL(forward_ensure(h, s));
  const int64_t N = h->N, C = h->dims[h->L], H = h->dims[1], P = h->n_params;
  // (the chunks of the batch call: closed-form Jacobians need the J and R rows only)
  const int64_t per_sample = sage || h->L == 1 ? C * 2 * P * 4 : C * (2 * P + N * (3 * H + C) + 2 * N * std::max(H, C)) * 4;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / std::max<int64_t>(per_sample, 1)));
  LGNN_REQUIRE(chunk * C < (int64_t(1) << 31), "full posterior directions: chunk too large");
  LGNN_CALL(h->ws.jac.reserve(size_t(chunk) * C * P * 4));
  float* J = h->ws.jac.as<float>();
  for (int64_t m0 = 0; m0 < M; m0 += chunk) {
    const int64_t mc = std::min(chunk, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    LGNN_CALL(launch_full_directions(J, Gamma, idx + m0, h->fc.out.as<float>(), N, mc, C, P, R_out + m0 * C * P,
                                     K_out + m0 * C * C, s));
  }
  return 0;
}

// h1_bar [N, H] / e_bar [N, F + 1] (diagonal posterior, GCN: diag_adjgrad_batch): adjoints of H_1 and of [P X | rowsum(P)]
// that take the place of the Kronecker posterior's 2 a_scale H_1 Gamma_A1 (gamma_A1 is null then)
int adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* gamma_A0, const float* gamma_A1, float a1_scale,
                   float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand,
                   float* grad_cand_adj, hipStream_t s, const float* h1_bar, const float* e_bar, float* dense = nullptr) {
  LGNN_REQUIRE(K == 0 || (cand_a && cand_b && grad_cand && grad_cand_adj), "candidate pairs without their buffers");
  if (h->L == 1)  // (gamma_A and h1_bar are ignored: X^T X does not depend on the adjacency, there is no hidden layer)
    return onelayer_adjgrad_finish(h, out_bar, e_bar, grad_P, grad_adj, cand_a, cand_b, K, grad_cand, grad_cand_adj, s);
  if (h->extras()) LGNN_CALL(check_model_ext(h));
  else LGNN_CALL(check_model(h));
  LGNN_REQUIRE(out_bar && (gamma_A1 || (h1_bar && e_bar)) && grad_P && grad_adj, "null pointers");
  if (h->kind == LGNN_KIND_SAGE) {
    if (h1_bar && e_bar)  // diagonal posterior
      return sage_adjgrad_finish(h, out_bar, nullptr, nullptr, 0.f, grad_P, grad_adj, cand_a, cand_b, K, grad_cand, grad_cand_adj, s,
                                 h1_bar, e_bar, h->dims[0] + 1);
    LGNN_REQUIRE(gamma_A0 != nullptr, "GraphSAGE: the first layer's input covariance depends on the adjacency (gamma_A[0])");
    return sage_adjgrad_finish(h, out_bar, gamma_A0, gamma_A1, a1_scale, grad_P, grad_adj, cand_a, cand_b, K, grad_cand,
                               grad_cand_adj, s);
  }
  LGNN_CALL(forward_ensure(h, s));
  LGNN_CALL(ensure_wt(h, s));
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0];
  // Z1 = H1 W1^T + b1 and Z0 = X W0^T + b0 (the forward keeps neither: one scratch serves both)
  const int64_t zw = std::max(H, C);
  LGNN_CALL(h->ws.planes_a.reserve(size_t(N) * (zw + H + C) * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* Z = h->ws.planes_a.as<float>();  // Z1 [N, C], later Z0 [N, H]
  float* Hb = Z + N * zw;                   // H1bar [N, H]
  float* Zb = Hb + N * H;                   // Z1bar [N, C]
  GemmEpilogue eb1;
  eb1.bias = h->b[1];
  LGNN_CALL(launch_gemm(h->fc.hact_p[0], h->fc.hact_ld[0], h->Wt[1].as<float>(), C, Z, C, N, H, C, eb1, s));
  if (!dense) LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, out_bar, C, 0, Z, C, 0, C, 1, grad_P, s));
  LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, out_bar, C, 0, Z, C, 0, C, 1, nullptr, grad_cand, s));
  DenseNtArgs dn;  // (the full-grid forms of the terms: dense route only)
  dn.out = dense; dn.ldo = N; dn.ncols = N; dn.nrows = N;
  if (dense) {
    dn.L = out_bar; dn.l_ld = C; dn.R = Z; dn.r_ld = C; dn.width = C;
    LGNN_CALL(launch_dense_nt(dn, s));
  }
  // Z1bar = P^T outbar;  H1bar = Z1bar W1 + 2 a1_scale H1 Gamma_A1;  P0bar = mask * H1bar
  LGNN_CALL(launch_spmm(h->PT, N, out_bar, C, Zb, C, C, 0, s));
  LGNN_CALL(sgemm_rm(s, N, H, C, 1.f, Zb, C, h->W[1], H, 0.f, Hb, H));
  if (gamma_A1) LGNN_CALL(sgemm_rm(s, N, H, H, 2.f * a1_scale, h->fc.hact_p[0], h->fc.hact_ld[0], gamma_A1, H, 1.f, Hb, H));
  if (h1_bar) {
    hipLaunchKernelGGL(add_inplace_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * H, 256), 4096))), dim3(256), 0, s, Hb, h1_bar,
                       N * H);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  if (h->extras()) {  // s_bar = norm_bwd(mask * H1bar): the mask and the norm's row-local backward (resnorm.hip)
    LGNN_CALL(launch_resnorm_backward(h, 0, Hb, H, N, nullptr, true, s));
  } else {
    hipLaunchKernelGGL(relu_mask_inplace_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * H, 256), 4096))), dim3(256), 0, s,
                       Hb, h->fc.hact_p[0], N * H);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  GemmEpilogue eb0;
  eb0.bias = h->b[0];
  LGNN_CALL(launch_gemm(h->fc.lin_in_p[0], h->fc.lin_in_ld[0], h->Wt[0].as<float>(), H, Z, H, N, F, H, eb0, s));
  if (!dense) LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, Hb, H, 0, Z, H, 0, H, 1, grad_P, s));
  LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, Hb, H, 0, Z, H, 0, H, 1, nullptr, grad_cand, s));
  if (dense) {
    dn.L = Hb; dn.l_ld = H; dn.R = Z; dn.r_ld = H; dn.width = H;
    LGNN_CALL(launch_dense_nt(dn, s));
  }
  if (e_bar) {
    // P X = sum_u P[v, u] X[u]: gradP[(v, u)] += <e_bar[v, :F], X[u]>;  rowsum(P)[v] = sum_u P[v, u]: += e_bar[v, F]
    const int64_t F1 = F + 1;
    LGNN_CALL(forward_input_view(h, s));
    if (!dense) {
      LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, e_bar, F1, 0, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], 0, F, 1, grad_P, s));
      LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, e_bar, F1, 0, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], 0, F, 1, nullptr,
                                 grad_cand, s));
      LGNN_CALL(launch_row_const(h, e_bar + F, F1, grad_P, cand_a, K, grad_cand, s));
    }
    if (dense) {  // <e_bar[a, :F], X[b]> + e_bar[a, F] on every pair
      dn.L = e_bar; dn.l_ld = F1; dn.R = h->fc.lin_in_p[0]; dn.r_ld = h->fc.lin_in_ld[0]; dn.width = F;
      dn.rowc = e_bar + F; dn.rowc_ld = F1;
      LGNN_CALL(launch_dense_nt(dn, s));
    }
  }
  if (dense) return dense_adj_finish(h, dense, s);  // normalize_adj backward, symmetrisation, diagonal on the full grid
  return normalize_adj_backward(h, grad_P, grad_adj, cand_a, cand_b, K, grad_cand, grad_cand_adj, s);
}

}  // namespace lgnn

extern "C" int lgnn_kfac_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags,
                                       const float* const* gamma_B, float loss_scale, float* grad_P, float* out_bar,
                                       const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand, float* grad_cand,
                                       void* stream) {
  if (!h || !gamma_B) { lgnn::set_error("null argument"); return 2; }
  return lgnn::kfac_adjgrad_batch(h, idx, y, M, flags, gamma_B[0], h->L == 1 ? nullptr : gamma_B[1],
                                  h->has_res ? gamma_B[2] : nullptr, loss_scale, grad_P, out_bar, cand_a, cand_b, num_cand,
                                  grad_cand, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* const* gamma_A, float a_scale,
                                   float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b,
                                   int64_t num_cand, float* grad_cand, float* grad_cand_adj, void* stream) {
  if (!h || !gamma_A) { lgnn::set_error("null argument"); return 2; }
  return lgnn::adjgrad_finish(h, out_bar, gamma_A[0], h->L == 1 ? nullptr : gamma_A[1], a_scale, grad_P, grad_adj, cand_a, cand_b,
                              num_cand, grad_cand, grad_cand_adj, static_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int lgnn_diag_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                       float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                                       const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand, float* grad_cand,
                                       void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  return lgnn::diag_adjgrad_batch(h, idx, y, M, gamma, loss_scale, grad_P, out_bar, h1_bar, e_bar, cand_a, cand_b, num_cand,
                                  grad_cand, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_full_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* Gamma,
                                       float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                                       const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand, float* grad_cand,
                                       void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  return lgnn::full_adjgrad_batch(h, idx, y, M, Gamma, loss_scale, grad_P, out_bar, h1_bar, e_bar, cand_a, cand_b, num_cand,
                                  grad_cand, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_full_directions(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* Gamma, float* K_out, float* R_out,
                                    void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  return lgnn::full_directions(h, idx, M, Gamma, K_out, R_out, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_diag_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar,
                                        float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b,
                                        int64_t num_cand, float* grad_cand, float* grad_cand_adj, void* stream) {
  if (!h) { lgnn::set_error("null context"); return 2; }
  if ((!h1_bar && h->L != 1) || !e_bar) { lgnn::set_error("lgnn_diag_adjgrad_finish: null adjoint buffers"); return 2; }
  return lgnn::adjgrad_finish(h, out_bar, nullptr, nullptr, 0.f, grad_P, grad_adj, cand_a, cand_b, num_cand, grad_cand,
                              grad_cand_adj, static_cast<hipStream_t>(stream), h1_bar, e_bar);
}

// ---- the dense [N, N] route (plain 2-layer GCN; LoRASTEGCN, lora.hip) ---------------------------------------------------------
// The dense route reads nothing of the stored-entry accumulator: the kernels that only add into it are skipped, those whose
// other outputs are needed (the fused SDDMM + SpMM that also forms ubar; the diagonal posterior's entry kernel that also
// scatters h1_bar / e_bar) write into this zeroed scratch, which is never read.
static int dense_scope(lgnn_ctx* h, const char* what, hipStream_t s) {
  using namespace lgnn;
  if (h->kind != LGNN_KIND_GCN || h->L != 2 || h->extras()) {
    set_error(std::string(what) + ": the dense adjacency gradient covers plain 2-layer GCN models (no res / norm)");
    return 2;
  }
  if (h->N * h->N >= (int64_t(1) << 31)) {
    set_error(std::string(what) + ": N^2 exceeds int32 indexing of the dense gradient");
    return 2;
  }
  LGNN_CALL(h->ws.dense_stored.reserve(size_t(std::max<int64_t>(h->nnz, 1)) * 4));
  LGNN_HIP_CHECK(hipMemsetAsync(h->ws.dense_stored.p, 0, size_t(std::max<int64_t>(h->nnz, 1)) * 4, s));
  return 0;
}

extern "C" int lgnn_kfac_adjgrad_batch_dense(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags,
                                             const float* const* gamma_B, float loss_scale, float* out_bar,
                                             float* grad_adj_dense, void* stream) {
  if (!h || !gamma_B || !grad_adj_dense) { lgnn::set_error("null argument"); return 2; }
  LGNN_CALL(dense_scope(h, "lgnn_kfac_adjgrad_batch_dense", static_cast<hipStream_t>(stream)));
  return lgnn::kfac_adjgrad_batch(h, idx, y, M, flags, gamma_B[0], gamma_B[1], nullptr, loss_scale,
                                  h->ws.dense_stored.as<float>(), out_bar, nullptr, nullptr, 0, nullptr,
                                  static_cast<hipStream_t>(stream), grad_adj_dense);
}

extern "C" int lgnn_adjgrad_finish_dense(lgnn_ctx* h, const float* out_bar, const float* const* gamma_A, float a_scale,
                                         float* grad_adj_dense, void* stream) {
  if (!h || !gamma_A || !grad_adj_dense) { lgnn::set_error("null argument"); return 2; }
  LGNN_CALL(dense_scope(h, "lgnn_adjgrad_finish_dense", static_cast<hipStream_t>(stream)));
  float* scratch = h->ws.dense_stored.as<float>();
  return lgnn::adjgrad_finish(h, out_bar, gamma_A[0], gamma_A[1], a_scale, scratch, scratch, nullptr, nullptr, 0, nullptr,
                              nullptr, static_cast<hipStream_t>(stream), nullptr, nullptr, grad_adj_dense);
}

extern "C" int lgnn_diag_adjgrad_batch_dense(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                             float loss_scale, float* out_bar, float* h1_bar, float* e_bar,
                                             float* grad_adj_dense, void* stream) {
  if (!h || !grad_adj_dense) { lgnn::set_error("null argument"); return 2; }
  LGNN_CALL(dense_scope(h, "lgnn_diag_adjgrad_batch_dense", static_cast<hipStream_t>(stream)));
  return lgnn::diag_adjgrad_batch(h, idx, y, M, gamma, loss_scale, h->ws.dense_stored.as<float>(), out_bar, h1_bar, e_bar,
                                  nullptr, nullptr, 0, nullptr, static_cast<hipStream_t>(stream), grad_adj_dense);
}

extern "C" int lgnn_diag_adjgrad_finish_dense(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar,
                                              float* grad_adj_dense, void* stream) {
  if (!h || !grad_adj_dense) { lgnn::set_error("null argument"); return 2; }
  if (!h1_bar || !e_bar) { lgnn::set_error("lgnn_diag_adjgrad_finish_dense: null adjoint buffers"); return 2; }
  LGNN_CALL(dense_scope(h, "lgnn_diag_adjgrad_finish_dense", static_cast<hipStream_t>(stream)));
  float* scratch = h->ws.dense_stored.as<float>();
  return lgnn::adjgrad_finish(h, out_bar, nullptr, nullptr, 0.f, scratch, scratch, nullptr, nullptr, 0, nullptr, nullptr,
                              static_cast<hipStream_t>(stream), h1_bar, e_bar, grad_adj_dense);
}
