// Adjacency gradient of the marginal likelihood (adjgrad.hip), plain 2-layer GraphSAGE, every posterior.
// Kronecker (STEGraphSAGE, gnn/models/models.py:121-183; mean aggregation P = A / rowsum, gnn/models/layers.py:18-24): the
// top layer is not propagated, so everything per batch lives on the batch rows and their neighbours -- sample-major rows
// r = (m, c) instead of planes over all N nodes:
//   per batch:       DCAT = S W1 [M C, 2H] (S = the seed blocks)     dh[v] = DCAT_self[v] + sum_{u in batch} P[u,v] DCAT_neigh[u]
//                    g0 = mask * dh on the ACTIVE rows (batch + neighbours, compacted)         g0bar = 2 g0 Gamma_B0
//                    gradP[(a,b)] += <DCAT_neigh[a], mask_b * g0bar[b]>,  dcatbar[a] = [mask_a g0bar[a] | sum_b P[a,b] mask_b g0bar[b]]
//                    g1bar = dcatbar W1^T + 2 S Gamma_B1 = Vbar                                   (then as above)
//   once per fit:    T1 = outbar W1 + 2 (T/N) cat1 Gamma_A1;  gradP += <T1_neigh[a], H1[b]>;  Z0bar = mask * (T1_self + P^T T1_neigh)
//                    XNbar = Z0bar W0_neigh + 2 (T/N) (cat0 Gamma_A0)_neigh;  gradP += <XNbar[a], X[b]>
//                    mean_agg backward: gA[a,b] = (gradP[a,b] - sum_j gradP[a,j] P[a,j]) / max(rowsum_a, 1)
#include "adjgrad.h"
#include "device_utils.h"

#include <rocprim/rocprim.hpp>

namespace lgnn {

namespace {

// active[v] = 1 for the batch nodes and every column of their P rows (the rows where dh can be non-zero)
__global__ void sage_mark_active_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, const int32_t* __restrict__ rowptr,
                                        const int32_t* __restrict__ col, uint8_t* __restrict__ active) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t a = idx[m];
  if (a < 0 || a >= N) return;
  if (lane == 0) active[a] = 1;
  for (int32_t p = rowptr[a] + lane; p < rowptr[a + 1]; p += 64) active[col[p]] = 1;
}

__global__ void sage_index_active_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                         int32_t* __restrict__ widx) {
  const int64_t w = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (w < *count) widx[list[w]] = int32_t(w);
}

// G0[(w, c)] = act'(h_1[v]) * (DCAT[(pos[v], c), :H] + sum_{u in row v of P^T, u in batch} P^T[v,u] DCAT[(pos[u], c), H:]),
// v = list[w], classes c0 <= c < c0 + cc.  One wave per active node, PC classes at a time in registers; H % 4 == 0, <= 256.
template <int PC>
__global__ __launch_bounds__(256) void sage_dh_kernel(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_col,
                                                      const float* __restrict__ t_val, const int32_t* __restrict__ list,
                                                      const int32_t* __restrict__ count, const int32_t* __restrict__ pos,
                                                      const float* __restrict__ dcat, const float* __restrict__ dact,
                                                      int64_t C, int64_t H, int64_t c0, int64_t cc, float* __restrict__ G0) {
  const int lane = threadIdx.x & 63;
  const int k4 = lane * 4;
  const bool col_ok = k4 < H;
  const int64_t total = *count;
  for (int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); w < total; w += int64_t(gridDim.x) * 4) {
    const int64_t v = list[w];
    const int32_t mv = pos[v];
    const int32_t s = t_rowptr[v], e = t_rowptr[v + 1];
    float4 dm = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col_ok) dm = *reinterpret_cast<const float4*>(dact + v * H + k4);
    for (int64_t pc0 = 0; pc0 < cc; pc0 += PC) {
      float4 acc[PC];
#pragma unroll
      for (int c = 0; c < PC; ++c) {
        acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col_ok && pc0 + c < cc && mv != INT32_MAX)
          acc[c] = *reinterpret_cast<const float4*>(dcat + (int64_t(mv) * C + c0 + pc0 + c) * 2 * H + k4);
      }
      for (int32_t p = s; p < e; ++p) {
        const int32_t mu = pos[t_col[p]];
        if (mu == INT32_MAX) continue;  // wave-uniform
        const float a = t_val[p];
#pragma unroll
        for (int c = 0; c < PC; ++c) {
          if (col_ok && pc0 + c < cc) {
            const float4 x = *reinterpret_cast<const float4*>(dcat + (int64_t(mu) * C + c0 + pc0 + c) * 2 * H + H + k4);
            acc[c].x = fmaf(a, x.x, acc[c].x); acc[c].y = fmaf(a, x.y, acc[c].y);
            acc[c].z = fmaf(a, x.z, acc[c].z); acc[c].w = fmaf(a, x.w, acc[c].w);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < PC; ++c)
        if (col_ok && pc0 + c < cc)
          *reinterpret_cast<float4*>(G0 + (w * cc + pc0 + c) * H + k4) =
              make_float4(dm.x * acc[c].x, dm.y * acc[c].y, dm.z * acc[c].z, dm.w * acc[c].w);
    }
  }
}

// For the first occurrence m of every batch node a = idx[m] and the classes of the chunk, in one pass over row a of P:
//     out[(a, b)]        += sum_c <DCAT[(m, c), H:], x_c[b]>,     x_c[b] = act'(h_1[b]) * G0B[(widx[b], c)]
//     DCATB[(m, c), H:]   = sum_b P[a, b] x_c[b]                    DCATB[(m, c), :H] = x_c[a]
// (later occurrences of a node: zero rows -- their seed rows are zero and Vbar is read at the first occurrence.)
template <int PC>
__global__ __launch_bounds__(256) void sage_sddmm_spmm_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, const int64_t* __restrict__ idx,
                                                              int64_t M, int64_t N, const int32_t* __restrict__ pos,
                                                              const int32_t* __restrict__ widx, const float* __restrict__ dcat,
                                                              const float* __restrict__ G0B, const float* __restrict__ dact,
                                                              int64_t C, int64_t H, int64_t c0, int64_t cc,
                                                              float* __restrict__ dcatb, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int k4 = lane * 4;
  const bool col_ok = k4 < H;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); m < M; m += int64_t(gridDim.x) * 4) {
    const int64_t a = idx[m];
    const bool first = a >= 0 && a < N && pos[a] == m;
    if (!first) {
      for (int64_t c = 0; c < cc; ++c)
        if (col_ok) {
          float* __restrict__ r = dcatb + (m * C + c0 + c) * 2 * H;
          *reinterpret_cast<float4*>(r + k4) = zero4;
          *reinterpret_cast<float4*>(r + H + k4) = zero4;
        }
      continue;
    }
    const int32_t s = rowptr[a], e = rowptr[a + 1];
    const int64_t wa = widx[a];
    float4 da = zero4;
    if (col_ok) da = *reinterpret_cast<const float4*>(dact + a * H + k4);
    for (int64_t pc0 = 0; pc0 < cc; pc0 += PC) {
      float4 D[PC], acc[PC];
#pragma unroll
      for (int c = 0; c < PC; ++c) {
        acc[c] = zero4;
        D[c] = zero4;
        if (col_ok && pc0 + c < cc) D[c] = *reinterpret_cast<const float4*>(dcat + (m * C + c0 + pc0 + c) * 2 * H + H + k4);
      }
      for (int32_t p = s; p < e; ++p) {
        const int64_t b = col[p];
        const int64_t wb = widx[b];
        const float v = val[p];
        float4 db = zero4;
        if (col_ok) db = *reinterpret_cast<const float4*>(dact + b * H + k4);
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < PC; ++c) {
          if (col_ok && pc0 + c < cc) {
            float4 x = *reinterpret_cast<const float4*>(G0B + (wb * cc + pc0 + c) * H + k4);
            x.x *= db.x; x.y *= db.y; x.z *= db.z; x.w *= db.w;
            acc[c].x = fmaf(v, x.x, acc[c].x); acc[c].y = fmaf(v, x.y, acc[c].y);
            acc[c].z = fmaf(v, x.z, acc[c].z); acc[c].w = fmaf(v, x.w, acc[c].w);
            d += D[c].x * x.x + D[c].y * x.y + D[c].z * x.z + D[c].w * x.w;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
        if (lane == 0) out[p] += d;  // one wave owns row a (first occurrence): a single writer per entry inside a launch
      }
#pragma unroll
      for (int c = 0; c < PC; ++c)
        if (col_ok && pc0 + c < cc) {
          float* __restrict__ r = dcatb + (m * C + c0 + pc0 + c) * 2 * H;
          const float4 x = *reinterpret_cast<const float4*>(G0B + (wa * cc + pc0 + c) * H + k4);
          *reinterpret_cast<float4*>(r + k4) = make_float4(da.x * x.x, da.y * x.y, da.z * x.z, da.w * x.w);
          *reinterpret_cast<float4*>(r + H + k4) = acc[c];
        }
    }
  }
}

// candidate pairs (a, b): only a in the batch and b active contribute
__global__ __launch_bounds__(256) void sage_cand_kernel(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb, int64_t K,
                                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ widx,
                                                        const float* __restrict__ dcat, const float* __restrict__ G0B,
                                                        const float* __restrict__ dact, int64_t C, int64_t H, int64_t c0,
                                                        int64_t cc, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t k = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  const int64_t a = ca[k], b = cb[k];
  const int32_t m = pos[a];
  const int32_t wb = widx[b];
  if (m == INT32_MAX || wb < 0) return;
  float acc = 0.f;
  for (int64_t c = 0; c < cc; ++c) {
    const float* __restrict__ D = dcat + (int64_t(m) * C + c0 + c) * 2 * H + H;
    const float* __restrict__ x = G0B + (int64_t(wb) * cc + c) * H;
    for (int64_t q = lane; q < H; q += 64) acc += D[q] * dact[b * H + q] * x[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) out[k] += acc;
}

// Vbar[m][c][k] = g1bar[(first occurrence of idx[m], c)][k]   (every sample, duplicates included)
__global__ void sage_vbar_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int64_t CC,
                                 const int32_t* __restrict__ pos, const float* __restrict__ g1bar, float* __restrict__ vbar) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * CC) return;
  const int64_t m = t / CC, q = t - m * CC;
  const int64_t a = idx[m];
  if (a < 0 || a >= N) return;
  vbar[t] = g1bar[int64_t(pos[a]) * CC + q];
}

// mean_agg backward: rowdot[a] = sum_j gP[a,j] P[a,j];  gA[(a,b)] = (gP[(a,b)] - rowdot[a]) / rowsum_a  (stored rows: rowsum >= 1)
__global__ void sage_adj_grad_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ val,
                                     const float* __restrict__ gP, int64_t N, float* __restrict__ rowdot,
                                     float* __restrict__ gA) {
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int32_t s = rowptr[a], e = rowptr[a + 1];
  float acc = 0.f;
  for (int32_t p = s; p < e; ++p) acc += gP[p] * val[p];
  rowdot[a] = acc;
  for (int32_t p = s; p < e; ++p) gA[p] = (gP[p] - acc) * val[p];
}
// candidate (a, b) = entry (a, b) of A; an empty row's divisor is the constant 1 (layers.py:20) and carries no row term
__global__ void sage_cand_adj_grad_kernel(const int32_t* __restrict__ ca, int64_t K, const int32_t* __restrict__ rowptr,
                                          const float* __restrict__ gPc, const float* __restrict__ rowdot,
                                          float* __restrict__ out) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int64_t a = ca[k];
  const int32_t deg = rowptr[a + 1] - rowptr[a];
  out[k] = deg > 0 ? (gPc[k] - rowdot[a]) / float(deg) : gPc[k];
}

__global__ void relu_mask_ld_kernel(float* __restrict__ x, const float* __restrict__ dact, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride) x[q] *= dact[q];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Diagonal posterior, 2-layer GraphSAGE (STEGraphSAGE + DiagLaplace: the driver offers the pair, gnn/utils.py:55-59, 81):
//     s = [X | P X] W0^T + b0,  H1 = relu(s),  out = [H1 | P H1] W1^T + b1.
// Same identity as persample_adjgrad_batch_ext -- d sum_p gamma_p H_p = sum_n <K_n, d Lambda_n> + sum_{n,c} <R_n[c,:], d J_n[c,:]> --
// but everything of a (sample n, class c) pair is local to the rows {n} + N(n), so there are no planes: one workgroup per pair
// runs the tangent along R = (dW0, db0, dW1, db1) and its reverse on those rows,
//     h1dot[b] = act'(h1[b]) * ([X | P X][b] dW0^T + db0)                     (neighbours b of n)
//     gradP[(n, b)] += <h1dot[b], W1n[c]> + <H1[b], dW1n[c]>                   (W1 = [W1s | W1n]: self / neighbour halves)
//     h1_bar[b] += P[n, b] dW1n[c],  h1_bar[n] += dW1s[c]
//     px_bar[r] += (act'(h1[r]) * coef_r) dW0n,  coef_b = P[n, b] W1n[c],  coef_n = W1s[c]        (adjoint of P X, dW0 = [dW0s | dW0n])
// candidate pairs (n, b') get the same first line for their b': the caller's list is ordered by row once per call
// (sage_order_candidates), so a workgroup walks the slice [cand_ptr[n], cand_ptr[n + 1]) of the sorted positions cand_ord
// instead of scanning all K pairs; the results land at the pairs' places in the caller's list.
__global__ __launch_bounds__(256) void sage_diag_pair_kernel(const int64_t* __restrict__ idx, int64_t N, int64_t C, int64_t H,
                                                             int64_t F, int64_t P, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col, const float* __restrict__ val,
                                                             const float* __restrict__ cat0, const float* __restrict__ cat1,
                                                             const float* __restrict__ dact, const float* __restrict__ W1,
                                                             const float* __restrict__ R, const int32_t* __restrict__ cand_ptr,
                                                             const int32_t* __restrict__ cand_ord, const int32_t* __restrict__ cb,
                                                             float* __restrict__ grad_P, float* __restrict__ grad_cand,
                                                             float* __restrict__ h1_bar, float* __restrict__ px_bar,
                                                             int64_t px_ld) {
  extern __shared__ float sh[];  // w1s | w1n | dw1s | dw1n | cv | hd  [H each] | red [4]
  float* w1s = sh;
  float* w1n = w1s + H;
  float* dw1s = w1n + H;
  float* dw1n = dw1s + H;
  float* cv = dw1n + H;
  float* hd = cv + H;
  float* red = hd + H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  const int64_t m = q / C, c = q - m * C;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) return;
  const float* __restrict__ Rq = R + q * P;
  const float* __restrict__ dW0 = Rq;                  // [H][2F]
  const float* __restrict__ db0 = Rq + H * 2 * F;      // [H]
  const float* __restrict__ dW1c = db0 + H + c * 2 * H;  // row c of dW1 [C][2H]
  for (int64_t j = tid; j < H; j += 256) {
    w1s[j] = W1[c * 2 * H + j]; w1n[j] = W1[c * 2 * H + H + j];
    dw1s[j] = dW1c[j]; dw1n[j] = dW1c[H + j];
  }
  __syncthreads();
  // h1dot of row b -> hd[], then the pair's dot product (all threads get it)
  auto pair_dot = [&](int64_t b) -> float {
    for (int64_t j = wave; j < H; j += 4) {
      const float* __restrict__ wrow = dW0 + j * 2 * F;
      const float* __restrict__ xrow = cat0 + b * 2 * F;
      float acc = 0.f;
      for (int64_t i = lane; i < 2 * F; i += 64) acc += xrow[i] * wrow[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) hd[j] = dact[b * H + j] * (acc + db0[j]);
    }
    __syncthreads();
    float part = 0.f;
    for (int64_t j = tid; j < H; j += 256) part += hd[j] * w1n[j] + cat1[b * 2 * H + j] * dw1n[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    const float tot = red[0] + red[1] + red[2] + red[3];
    __syncthreads();  // hd / red are rewritten by the next row
    return tot;
  };
  // rows {n} + N(n): slot -1 = the node itself
  const int32_t s0 = rowptr[n], s1 = rowptr[n + 1];
  for (int32_t p = s0 - 1; p < s1; ++p) {
    const bool self = p < s0;
    const int64_t row = self ? n : int64_t(col[p]);
    const float pv = self ? 1.f : val[p];
    for (int64_t j = tid; j < H; j += 256) {
      cv[j] = dact[row * H + j] * pv * (self ? w1s[j] : w1n[j]);
      atomicAdd(&h1_bar[row * H + j], pv * (self ? dw1s[j] : dw1n[j]));
    }
    __syncthreads();
    for (int64_t f = tid; f < F; f += 256) {
      float acc = 0.f;
      for (int64_t j = 0; j < H; ++j) acc += cv[j] * dW0[j * 2 * F + F + f];
      atomicAdd(&px_bar[row * px_ld + f], acc);
    }
    if (!self) {
      const float d = pair_dot(row);  // (starts with a barrier-free phase on hd, ends with barriers)
      if (tid == 0) atomicAdd(&grad_P[p], d);
    } else {
      __syncthreads();
    }
  }
  // candidate pairs that start at n (a = n in the propagation matrix's coordinates): the row's slice of the sorted list
  const int32_t k1 = cand_ptr ? cand_ptr[n + 1] : 0;
  for (int32_t i = cand_ptr ? cand_ptr[n] : 0; i < k1; ++i) {
    const int32_t kk = cand_ord[i];
    const float d = pair_dot(cb[kk]);
    if (tid == 0) atomicAdd(&grad_cand[kk], d);
  }
}

// cand_ptr[n] = the first position of the sorted rows that is >= n, n = 0 .. N: row n's candidates are [cand_ptr[n], cand_ptr[n + 1])
__global__ void sage_cand_slices_kernel(const int32_t* __restrict__ rows, int64_t K, int64_t N, int32_t* __restrict__ cand_ptr) {
  const int64_t n = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n > N) return;
  int64_t lo = 0, hi = K;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (rows[mid] < n) lo = mid + 1; else hi = mid; }
  cand_ptr[n] = int32_t(lo);
}

__global__ void iota_i32_kernel(int32_t* __restrict__ v, int64_t n) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < n) v[j] = int32_t(j);
}

__global__ void add_strided_kernel(float* __restrict__ x, int64_t ldx, const float* __restrict__ y, int64_t ldy, int64_t rows,
                                   int64_t width) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < rows * width; t += stride) {
    const int64_t r = t / width, j = t - r * width;
    x[r * ldx + j] += y[r * ldy + j];
  }
}

}  // namespace

int sage_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool fork_exact, const float* gamma_B0,
                       const float* gamma_B1, float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a,
                       const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s) {
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], CC = C * C;
  LGNN_CALL(batch_prologue(h, idx, y, M, true, fork_exact, nullptr, s));
  const float* S = h->ws.seeds.as<float>();  // [M][C][C]: row (m, c) = column c of the seed block, zero for later occurrences
  LGNN_REQUIRE(M * C < (int64_t(1) << 31), "adjacency gradient: batch too large");
  // DCAT / DCATB [M C, 2H], g1bar [M C, C], Vbar [M][C][C]
  LGNN_CALL(h->ws.top.reserve(size_t(M) * C * 2 * H * 4 * 2 + size_t(M) * CC * 4 * 2));
  float* dcat = h->ws.top.as<float>();
  float* dcatb = dcat + M * C * 2 * H;
  float* g1b = dcatb + M * C * 2 * H;
  float* vbar = g1b + M * CC;
  LGNN_CALL(sgemm_rm(s, M * C, 2 * H, C, 1.f, S, C, h->W[1], 2 * H, 0.f, dcat, 2 * H));
  // active rows (batch + neighbours), their list and the inverse map
  LGNN_CALL(h->ws.active.reserve(size_t(N)));
  LGNN_HIP_CHECK(hipMemsetAsync(h->ws.active.p, 0, size_t(N), s));
  hipLaunchKernelGGL(sage_mark_active_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, h->P.rowptr, h->P.col,
                     h->ws.active.as<uint8_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(compact_active_rows(h, s));
  LGNN_CALL(h->ws.misc.reserve(size_t(N) * 4));
  int32_t* widx = h->ws.misc.as<int32_t>();
  LGNN_HIP_CHECK(hipMemsetAsync(widx, 0xFF, size_t(N) * 4, s));
  hipLaunchKernelGGL(sage_index_active_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->ws.act_list.as<int32_t>(),
                     h->ws.act_count.as<int32_t>(), widx);
  LGNN_HIP_CHECK(hipGetLastError());
  // the number of active rows stays on the device: buffers and grids are sized for the bound N, the kernels and the GEMM over
  // the active rows read the count themselves (no host round trip per batch)
  const int64_t na = N;
  {
    // class chunks: G0 and g0bar [na * cc, H] under the workspace cap
    const int64_t per_class = int64_t(na) * H * 4 * 2;
    const int64_t cc_max = std::max<int64_t>(1, std::min<int64_t>(C, h->ws_limit / std::max<int64_t>(per_class, 1)));
    LGNN_REQUIRE(int64_t(na) * cc_max < (int64_t(1) << 31), "adjacency gradient: too many active rows per chunk");
    LGNN_CALL(h->ws.planes_a.reserve(size_t(na) * cc_max * H * 4));
    LGNN_CALL(h->ws.planes_b.reserve(size_t(na) * cc_max * H * 4));
    h->ws.planes_a_zero_ptr = nullptr;
    float* G0 = h->ws.planes_a.as<float>();
    float* G0B = h->ws.planes_b.as<float>();
    const float* dact = h->fc.dact0.as<float>();
    for (int64_t c0 = 0; c0 < C; c0 += cc_max) {
      const int64_t cc = std::min(cc_max, C - c0);
      hipLaunchKernelGGL(sage_dh_kernel<8>, dim3(unsigned(std::min<int64_t>(cdiv(na, 4), 16384))), dim3(256), 0, s,
                         h->PT.rowptr, h->PT.col, h->PT.val, h->ws.act_list.as<int32_t>(), h->ws.act_count.as<int32_t>(),
                         h->ws.pos.as<int32_t>(), dcat, dact, C, H, c0, cc, G0);
      LGNN_HIP_CHECK(hipGetLastError());
      LGNN_CALL(launch_gemm_devrows(G0, H, gamma_B0, H, G0B, H, na * cc, h->ws.act_count.as<int32_t>(), cc, H, H, 2.f, s));
      if (K > 0)
        hipLaunchKernelGGL(sage_cand_kernel, dim3(unsigned(cdiv(K, 4))), dim3(256), 0, s, cand_a, cand_b, K,
                           h->ws.pos.as<int32_t>(), widx, dcat, G0B, dact, C, H, c0, cc, grad_cand);
      hipLaunchKernelGGL(sage_sddmm_spmm_kernel<8>, dim3(unsigned(std::min<int64_t>(cdiv(M, 4), 16384))), dim3(256), 0, s,
                         h->P.rowptr, h->P.col, h->P.val, idx, M, N, h->ws.pos.as<int32_t>(), widx, dcat, G0B, dact, C, H, c0,
                         cc, dcatb, grad_P);
      LGNN_HIP_CHECK(hipGetLastError());
    }
    // g1bar = dcatbar W1^T + 2 S Gamma_B1     [M C, C]
    LGNN_CALL(sgemm_rm(s, M * C, C, 2 * H, 1.f, dcatb, 2 * H, h->Wt[1].as<float>(), C, 0.f, g1b, C));
    LGNN_CALL(sgemm_rm(s, M * C, C, C, 2.f, S, C, gamma_B1, C, 1.f, g1b, C));
    hipLaunchKernelGGL(sage_vbar_kernel, dim3(unsigned(cdiv(M * CC, 256))), dim3(256), 0, s, idx, M, N, CC,
                       h->ws.pos.as<int32_t>(), g1b, vbar);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  LGNN_CALL(launch_seed_adjoint(h, idx, y, M, vbar, fork_exact, loss_scale, out_bar, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

// (diagonal posterior: gamma_A0 / gamma_A1 are null; h1_bar [N, H] = direct adjoint of H1, px_bar [N, px_ld] = of P X)
int sage_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* gamma_A0, const float* gamma_A1, float a_scale,
                        float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b, int64_t K,
                        float* grad_cand, float* grad_cand_adj, hipStream_t s, const float* h1_bar, const float* px_bar,
                        int64_t px_ld) {
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0];
  LGNN_CALL(forward_ensure_aux(h, s));
  LGNN_CALL(ensure_wt(h, s));
  const float* cat0 = h->fc.lin_in_p[0];  // [N, 2F]: X | P X
  const float* cat1 = h->fc.lin_in_p[1];  // [N, 2H]: H1 | P H1
  LGNN_REQUIRE(h->fc.lin_in_ld[0] == 2 * F && h->fc.lin_in_ld[1] == 2 * H, "internal: unexpected cat row stride");
  LGNN_CALL(h->ws.planes_a.reserve(size_t(N) * (2 * H + H + F) * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  float* T1 = h->ws.planes_a.as<float>();  // [N, 2H]
  float* Z0b = T1 + N * 2 * H;              // [N, H]
  float* XNb = Z0b + N * H;                 // [N, F]
  // T1 = outbar W1 + 2 a cat1 Gamma_A1: the self half feeds H1bar directly, the neighbour half is HNbar
  LGNN_CALL(sgemm_rm(s, N, 2 * H, C, 1.f, out_bar, C, h->W[1], 2 * H, 0.f, T1, 2 * H));
  if (gamma_A1) LGNN_CALL(sgemm_rm(s, N, 2 * H, 2 * H, 2.f * a_scale, cat1, 2 * H, gamma_A1, 2 * H, 1.f, T1, 2 * H));
  if (h1_bar) {  // joins the self half before the mask
    hipLaunchKernelGGL(add_strided_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * H, 256), 4096))), dim3(256), 0, s, T1, 2 * H,
                       h1_bar, H, N, H);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, T1 + H, 2 * H, 0, cat1, 2 * H, 0, H, 1, grad_P, s));
  LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, T1 + H, 2 * H, 0, cat1, 2 * H, 0, H, 1, nullptr, grad_cand, s));
  // Z0bar = mask * (T1_self + P^T T1_neigh)
  SpmmArgs sa{};
  sa.rowptr = h->PT.rowptr; sa.col = h->PT.col; sa.val = h->PT.val; sa.nrows = N;
  sa.in = T1 + H; sa.in_ld = 2 * H; sa.in_plane_stride = 0;
  sa.self = T1; sa.self_ld = 2 * H; sa.self_plane_stride = 0;
  sa.out = Z0b; sa.out_ld = H; sa.out_plane_stride = 0; sa.width = H; sa.out_act = -1;
  LGNN_CALL(launch_spmm_ex(sa, 1, s));
  hipLaunchKernelGGL(relu_mask_ld_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * H, 256), 4096))), dim3(256), 0, s, Z0b,
                     h->fc.dact0.as<float>(), N * H);
  LGNN_HIP_CHECK(hipGetLastError());
  // XNbar = Z0bar W0[:, F:] + 2 a (cat0 Gamma_A0)[:, F:]
  LGNN_CALL(sgemm_rm(s, N, F, H, 1.f, Z0b, H, h->W[0] + F, 2 * F, 0.f, XNb, F));
  if (gamma_A0) LGNN_CALL(sgemm_rm(s, N, F, 2 * F, 2.f * a_scale, cat0, 2 * F, gamma_A0 + F, 2 * F, 1.f, XNb, F));
  if (px_bar) {
    hipLaunchKernelGGL(add_strided_kernel, dim3(unsigned(std::min<int64_t>(cdiv(N * F, 256), 4096))), dim3(256), 0, s, XNb, F, px_bar,
                       px_ld, N, F);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  LGNN_CALL(launch_sddmm(h->P, N, nullptr, nullptr, XNb, F, 0, cat0, 2 * F, 0, F, 1, grad_P, s));
  LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, XNb, F, 0, cat0, 2 * F, 0, F, 1, nullptr, grad_cand, s));
  // mean_agg backward + the straight-through binarisation (P has the pattern and the row order of A)
  LGNN_CALL(h->ws.misc.reserve(size_t(N) * 4 + size_t(std::max<int64_t>(h->nnz, 1)) * 4));
  float* rowdot = h->ws.misc.as<float>();
  float* tmp = rowdot + N;
  float* first = h->sym ? tmp : grad_adj;
  hipLaunchKernelGGL(sage_adj_grad_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->P.rowptr, h->P.val, grad_P, N,
                     rowdot, first);
  LGNN_HIP_CHECK(hipGetLastError());
  if (h->sym) LGNN_CALL(launch_adj_grad_symmetrize(h->P, tmp, N, grad_adj, s));
  if (K > 0)
    hipLaunchKernelGGL(sage_cand_adj_grad_kernel, dim3(unsigned(cdiv(K, 256))), dim3(256), 0, s, cand_a, K, h->P.rowptr, grad_cand,
                       rowdot, grad_cand_adj);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// The candidates' rows in increasing order (stable radix sort; the caller's order is arbitrary, symmetric models pass both
// orientations concatenated): ws.cand_ord = the positions in the caller's list, ws.cand_ptr = every row's slice of them.  All 32
// bits of the signed ids are sorted, so a row outside [0, N) lands before slice 0 or behind slice N - 1 and is never visited,
// as it never matched a sample's node before.
static int sage_order_candidates(lgnn_ctx* h, const int32_t* cand_a, int64_t K, hipStream_t s) {
  Workspace& w = h->ws;
  const int64_t N = h->N;
  LGNN_REQUIRE(K < (int64_t(1) << 31), "adjacency gradient: too many candidates");
  LGNN_CALL(w.cand_rows.reserve(size_t(K) * 4));
  LGNN_CALL(w.cand_ord.reserve(size_t(K) * 4));
  LGNN_CALL(w.cand_iota.reserve(size_t(K) * 4));
  LGNN_CALL(w.cand_ptr.reserve(size_t(N + 1) * 4));
  hipLaunchKernelGGL(iota_i32_kernel, dim3(unsigned(cdiv(K, 256))), dim3(256), 0, s, w.cand_iota.as<int32_t>(), K);
  LGNN_HIP_CHECK(hipGetLastError());
  size_t bytes = 0;
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, cand_a, w.cand_rows.as<int32_t>(), w.cand_iota.as<int32_t>(),
                                           w.cand_ord.as<int32_t>(), size_t(K), 0, 32, s));
  LGNN_CALL(w.cand_tmp.reserve(bytes));
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(w.cand_tmp.p, bytes, cand_a, w.cand_rows.as<int32_t>(), w.cand_iota.as<int32_t>(),
                                           w.cand_ord.as<int32_t>(), size_t(K), 0, 32, s));
  hipLaunchKernelGGL(sage_cand_slices_kernel, dim3(unsigned(cdiv(N + 1, 256))), dim3(256), 0, s, w.cand_rows.as<int32_t>(), K, N,
                     w.cand_ptr.as<int32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// (gamma [P]: diagonal posterior; Gamma [P, P]: full posterior; exactly one of them, see chunk_directions)
int persample_adjgrad_batch_sage(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                 const float* Gamma, float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                                 const int32_t* cand_a, const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s) {
  LGNN_REQUIRE(h->L == 2 && !h->extras(), "adjacency gradient, diagonal / full posterior, GraphSAGE: plain 2-layer models");
  LGNN_REQUIRE(h->act == LGNN_ACT_RELU && h->lik == LGNN_LIK_CLASSIFICATION, "adjacency gradient: ReLU, classification");
  LGNN_REQUIRE(M > 0 && idx && y && (gamma != nullptr) != (Gamma != nullptr) && grad_P && out_bar && h1_bar && e_bar,
               "empty batch or null pointers");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0], P = h->n_params;
  LGNN_REQUIRE(P == H * 2 * F + H + C * 2 * H + C, "internal: parameter count");
  LGNN_REQUIRE(h->fc.lin_in_ld[0] == 2 * F && h->fc.lin_in_ld[1] == 2 * H, "internal: unexpected cat row stride");
  LGNN_REQUIRE(size_t(C * C + C) * 4 <= 64 * 1024 && size_t(6 * H + 4) * 4 <= 60 * 1024, "too many classes / hidden units");
  const int64_t per_sample = C * 2 * P * 4;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / std::max<int64_t>(per_sample, 1)));
  LGNN_CALL(h->ws.jac.reserve(size_t(chunk) * C * P * 4));
  LGNN_CALL(h->ws.adj_dir.reserve(size_t(chunk) * C * P * 4));
  LGNN_CALL(h->ws.probs.reserve(size_t(chunk) * (C + C * C) * 4));
  float* J = h->ws.jac.as<float>();
  float* R = h->ws.adj_dir.as<float>();
  float* probs = h->ws.probs.as<float>();
  float* Kn = probs + chunk * C;
  const int64_t* yy = static_cast<const int64_t*>(y);
  const int32_t* cand_ptr = nullptr;
  const int32_t* cand_ord = nullptr;
  if (K > 0) {
    LGNN_REQUIRE(cand_a && cand_b && grad_cand, "null candidate pointers");
    LGNN_CALL(sage_order_candidates(h, cand_a, K, s));
    cand_ptr = h->ws.cand_ptr.as<int32_t>();
    cand_ord = h->ws.cand_ord.as<int32_t>();
  }
  for (int64_t m0 = 0; m0 < M; m0 += chunk) {
    const int64_t mc = std::min(chunk, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    LGNN_CALL(chunk_directions(h, idx + m0, yy + m0, mc, J, gamma, Gamma, loss_scale, probs, Kn, R, out_bar, s));
    hipLaunchKernelGGL(sage_diag_pair_kernel, dim3(unsigned(mc * C)), dim3(256), size_t(6 * H + 4) * 4, s, idx + m0, N, C, H, F, P,
                       h->P.rowptr, h->P.col, h->P.val, h->fc.lin_in_p[0], h->fc.lin_in_p[1], h->fc.dact0.as<float>(), h->W[1], R,
                       cand_ptr, cand_ord, cand_b, grad_P, grad_cand, h1_bar, e_bar, F + 1);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace lgnn
