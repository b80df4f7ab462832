// First-layer gradient covariance B_0 of a 2-layer GCN WITHOUT class planes: the headline KFAC path.
//
// Reference: KFACLinearOperator._compute_loss_and_backward / _accumulate_gradient_covariance (curvlinops/kfac.py:607-661,
// 777-817) run one dense backward pass per class column c of the loss-Hessian square root through the model
// (gnn/models/base_gnn.py:141-156, gnn/models/layers.py:45-46) and add g^T g at the first Linear's output.
//
// The seed block is diagonal + rank 2 (kfac_top.hip, seed_spmm_gram_kernel):  V_m[k, c] = alpha_c d_kc - beta_c u_k - gamma_c p_k,
// hence  V_m[:, c]^T W_1 = alpha_c^m W_1[c, :] - beta_c^m b_m - gamma_c^m g_m  with the per-sample H-vectors b_m = u_m^T W_1,
// g_m = p_m^T W_1, and for a destination node n the C x H block of all its class rows is a sum over the batch's 2-hop paths
// j = (n <- v_j <- m_j), weight w_j = P^T[n, v_j] P^T[v_j, m_j]:
//     Y[n] = W_1 (.) (A_alpha Mk) + A_beta (B_k (.) Mk) + A_gamma (G_k (.) Mk)
//       A_*[c, j] = w_j * (alpha, -beta, -gamma)_c^{m_j}   (C x K),   Mk[j, :] = ReLU mask bits of v_j  (K x H, 0 / 1),
//       B_k[j, :] = b_{m_j},  G_k[j, :] = g_{m_j}                    (K x H, rows of a 20 MB per-batch table: L2 / MALL resident)
//     B_0 += Y[n]^T Y[n]
// (oracle: kfac_first_layer_B_by_paths, pinned to the reference's goldens).  ~13 paths per node at the arxiv shape, ~2.8 KB
// gathered per path where the plane route (backgemm.hip, fused256.hip) gathers 40 KB per edge; the price is three C x K x H
// products on the matrix pipes (+ ~1/3 of the Gram's MFMA work).
//
// Here, per mini-batch: path_tables_kernel (per-sample coefficient rows (alpha, -beta, -gamma), the rows (u, p), b_m, g_m),
// path_r_kernel (R = P^T[:, batch] as CSR over v: count, rocPRIM scan, fill), path_list_kernel (the 2-hop paths per destination
// node as CSR over n, likewise; one wave per node), their GraphSAGE twins, path_flag_kernel (the nodes with a path); per graph,
// the two_hop_* counts behind paths_pay and the overflow bound.  The two host drivers end in launch_paths_fused (paths_fused.hip)
// and, where a list can overflow its buffer, launch_paths_overflow (paths_overflow.hip); batchcache.hip may hold R and the lists.
#include "device_utils.h"
#include "paths.h"

namespace lgnn {

namespace {

// max_c sum_k |V[k, c]| of a sample's seed block V[k, c] = alpha_c d_kc - beta_c u_k - gamma_c p_k, as a bit pattern (a NaN is above
// everything): what PathScale's vmax is the largest of (paths.h).  Lane c holds (alpha, beta, gamma)_c (zeros past C), lane k
// holds u_k and p_k; every lane of the wave takes part.
__device__ __forceinline__ uint32_t seed_column_sum_max(float al, float be, float ga, float u, float p, int C, int lane) {
  float vs = 0.f;
  for (int k = 0; k < C; ++k) {
    const float uk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), k));
    const float pk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), k));
    vs += fabsf((lane == k ? al : 0.f) - be * uk - ga * pk);
  }
  uint32_t b = __float_as_uint(vs) & 0x7fffffffu;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b = max(b, uint32_t(__shfl_xor(int(b), o)));
  return b;
}

// One wave per batch sample (first occurrences only; a node listed t times carries t in its R weights).
// mode: 0 upstream seeds, 1 fork exact, 2 regression (V = sqrt(2) I).  The coefficient row holds the classes [cb, cb + 64) of the
// call in slot order (coef_slot); slots of classes >= ce are zero.
__global__ __launch_bounds__(256) void path_tables_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                                          const int64_t* __restrict__ idx, const int32_t* __restrict__ pos,
                                                          int64_t M, int64_t N, int C, int cb, int ce, int mode,
                                                          float* __restrict__ coef, float* __restrict__ up,
                                                          const float* __restrict__ W1, int H, float* __restrict__ bg,
                                                          uint32_t* __restrict__ vsum) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t n = idx[m];
  float* __restrict__ cm = coef + m * kCoefRow;
  float* __restrict__ um = up + m * C;
  float* __restrict__ pm = up + (M + m) * C;
  const bool own = n >= 0 && n < N && pos[n] == int32_t(m);
  float pk = 0.f, fk = 0.f;
  if (own && lane < C && mode != 2) { pk = probs[m * C + lane]; fk = logits[n * C + lane]; }
  const float mb = wave_sum(pk * fk);  // same summation order as seed_kernel / seed_spmm_gram_kernel
  const float sp = sqrtf(pk), t = fk - mb;
  float al = 0.f, be = 0.f, ga = 0.f, u = 0.f;
  if (own && lane < C) {
    if (mode == 2) al = 1.41421356237309515f;
    else if (mode == 1) { al = sp * (1.f + 0.5f * t); be = sp; ga = 0.5f * sp * t; u = pk * (1.f + t); }
    else { al = sp; be = sp; u = pk; }
  }
  // slot `lane` of each kind holds class cb + slot_class(lane): fetched from the lane that computed it.  Classes outside the
  // call's range [cb, ce) get zero coefficients: their rows of Y come out as exact zeros, the fused kernel stores them unasked
  const int c = cb + slot_class(lane);
  const bool have = c < ce;
  const int src = have ? c : 0;
  const float sal = __shfl(al, src), sbe = __shfl(be, src), sga = __shfl(ga, src);
  cm[lane] = have ? sal : 0.f;
  cm[kCoefStride + lane] = have ? -sbe : 0.f;
  cm[2 * kCoefStride + lane] = have ? -sga : 0.f;
  cm[3 * kCoefStride + lane] = 0.f;
  if (lane < C) { um[lane] = u; pm[lane] = own ? pk : 0.f; }
  {  // (one entry per row of the coefficient table)
    const uint32_t vb = seed_column_sum_max(al, be, ga, u, own ? pk : 0.f, C, lane);
    if (lane == 0) vsum[m] = vb;
  }
  // b_m = u_m^T W_1 and g_m = p_m^T W_1 (rows m and M + m of bg [2 M, H]; null: not wanted): u and p sit in the wave's lanes,
  // the C rows of W_1 (L2 resident) are read 16 bytes per lane -- four columns of both products per lane
  if (bg == nullptr) return;
  const bool colv = 4 * lane < H;  // (H <= 256: every column has a lane; the lanes past H read column 0 and store nothing)
  f32x4 b4 = {0.f, 0.f, 0.f, 0.f}, g4 = {0.f, 0.f, 0.f, 0.f};
  if (own) {  // (wave uniform: the v_readlane below run with every lane active)
    const float* __restrict__ w = W1 + (colv ? 4 * lane : 0);
    for (int c = 0; c < C; ++c) {
      const float uc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), c));
      const float pc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pk), c));
      const f32x4 wc = *reinterpret_cast<const f32x4*>(w + int64_t(c) * H);
      b4 += uc * wc;
      g4 += pc * wc;
    }
  }
  if (colv) {
    *reinterpret_cast<f32x4*>(bg + m * H + 4 * lane) = b4;
    *reinterpret_cast<f32x4*>(bg + (M + m) * H + 4 * lane) = g4;
  }
}

// R = P^T[:, batch]: for every distinct batch node u (its first position m) and every entry (v, val) of row u of P.
template <bool FILL>
__global__ __launch_bounds__(256) void path_r_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                     const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                     const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const float* __restrict__ val, int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ rptr, int32_t* __restrict__ r_m,
                                                     float* __restrict__ r_w) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t u = idx[m];
  if (u < 0 || u >= N || pos[u] != int32_t(m)) return;  // invalid ids are flagged by mark_batch_kernel
  const float tm = FILL ? float(mult[m]) : 0.f;
  const int32_t e = rowptr[u + 1];
  for (int32_t p = rowptr[u] + lane; p < e; p += 64) {
    const int32_t v = col[p];
    const int32_t k = atomicAdd(&cnt[v], 1);
    if constexpr (FILL) {
      const int32_t slot = rptr[v] + k;
      r_m[slot] = int32_t(m);
      r_w[slot] = val[p] * tm;
    }
  }
}

// *m = max(*m, bits).  Tens of thousands of waves meet on one word, and atomics on one address run one after the other (a
// full arxiv batch: 0.37 ms for 20 000 of them): the value only grows, so a wave that reads a value no smaller than its own
// has nothing to add, and almost none of them gets as far as the atomic.
__device__ __forceinline__ void atomic_max_bits(uint32_t* m, uint32_t bits) {
  if (bits > *reinterpret_cast<volatile uint32_t*>(m)) atomicMax(m, bits);
}
// *wsum = max(*wsum, the wave's sum of `wabs`) on the bit patterns (wabs >= 0 or NaN: PathScale in paths.h)
__device__ __forceinline__ void path_wsum_max(float wabs, int lane, uint32_t* __restrict__ wsum) {
  const uint32_t bits = __float_as_uint(wave_sum(wabs)) & 0x7fffffffu;
  if (lane == 0) atomic_max_bits(wsum, bits);
}

// The batch's 2-hop paths per destination node, materialised once per batch (count, rocPRIM scan, fill): the irregular
// three-level walk (row of P^T -> R pointers -> R entries) runs here with one wave per node and tens of thousands of waves
// in flight, so that ybuild_kernel's own chain is just  pointer -> entries -> table rows.
// One wave per node n:  cnt[n] = sum over the entries (v, pv) of row n of P^T of |R[v]|.
template <bool FILL>
__global__ __launch_bounds__(256) void path_list_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ val, int64_t N,
                                                        const int32_t* __restrict__ rptr, const int32_t* __restrict__ r_m,
                                                        const float* __restrict__ r_w, int32_t* __restrict__ pcnt,
                                                        const int32_t* __restrict__ pptr, int64_t cap,
                                                        int32_t* __restrict__ pm, int32_t* __restrict__ pv,
                                                        float* __restrict__ pw, uint32_t* __restrict__ wsum) {
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  if constexpr (FILL) {
    if (int64_t(pptr[N]) > cap) return;  // the list does not fit its buffer: ybuild enumerates on the fly (same results)
  }
  const int32_t s = rowptr[n], e = rowptr[n + 1];
  int32_t run = FILL ? pptr[n] : 0;
  float wabs = 0.f;  // FILL: the lane's share of sum_paths |w| of this node (PathScale's wsum)
  for (int32_t base = s; base < e; base += 64) {
    int32_t v = 0, r0 = 0, cnt = 0;
    float pval = 0.f;
    if (base + lane < e) {
      v = col[base + lane];
      pval = val[base + lane];
      r0 = rptr[v];
      cnt = rptr[v + 1] - r0;
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if constexpr (FILL) {
      const int32_t off = run + incl - cnt;
      for (int k = 0; k < cnt; ++k) {
        pm[off + k] = r_m[r0 + k];
        pv[off + k] = v;
        pw[off + k] = pval * r_w[r0 + k];
        wabs += fabsf(pval * r_w[r0 + k]);
      }
    }
    run += __shfl(incl, 63);
  }
  if (!FILL && lane == 0) pcnt[n] = run;
  if constexpr (FILL) path_wsum_max(wabs, lane, wsum);
}

// ---- GraphSAGE: the same fused kernel over ONE-hop paths ----------------------------------------------------------------
// cat_1 = [h_1 | P h_1], out = cat_1 W_1^T + b_1 (gnn/models/layers.py:26-29), so the first-layer gradient rows of node n are
//     G_c[n] = mask_n (.) ( S_c[n] W_1s + sum_m P[m, n] S_c[m] W_1n ),   S_c[m] = V_m[:, c]^T (the sample's seed column),
// W_1 = [W_1s | W_1n].  With V = diag(alpha) - u beta^T - p gamma^T this is the path sum of the GCN route with the mask at
// the DESTINATION (every path of n names n as its mask row), the neighbour half W_1n as the kernel's W_1 operand, and the
// self terms as pseudo paths:
//   sample index 2 m + 1 : neighbour path m -> n, weight P[m, n] mult_m, coefficients (alpha, -beta, -gamma)_m, rows u_m^T W_1n, p_m^T W_1n
//   sample index 2 m     : n's own beta / gamma terms: coefficients (0, -beta, -gamma)_m, rows u_m^T W_1s, p_m^T W_1s
//   sample index 2 M + c': n's own alpha term alpha_{m,c'} W_1s[c', :] as a "beta" product with a one-hot coefficient row
//                          (+1 at class c'), table row W_1s[c', :] and path weight mult_m alpha_{m,c'}
// (u^T [W_1s | W_1n] is one GEMM whose [M][2H] output IS the [2M][H] table in that order).  paths_fused_kernel runs unchanged.
__global__ __launch_bounds__(256) void sage_path_tables_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                                               const int64_t* __restrict__ idx, const int32_t* __restrict__ pos,
                                                               int64_t M, int64_t N, int C, int cb, int ce, int mode,
                                                               float* __restrict__ coef, float* __restrict__ up,
                                                               float* __restrict__ alpha, uint32_t* __restrict__ vsum) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M + C) return;
  const int c = cb + slot_class(lane);  // the class of slot `lane` (coef_slot order, see path_tables_kernel)
  const bool have = c < ce;             // (classes outside the call's range: zero coefficients)
  if (m >= M) {  // the one-hot rows
    float* __restrict__ cm = coef + (2 * M + (m - M)) * kCoefRow;
    cm[lane] = 0.f; cm[kCoefStride + lane] = (have && c == int(m - M)) ? 1.f : 0.f; cm[2 * kCoefStride + lane] = 0.f; cm[3 * kCoefStride + lane] = 0.f;
    if (lane == 0) vsum[2 * M + (m - M)] = 0u;
    return;
  }
  const int64_t n = idx[m];
  const bool own = n >= 0 && n < N && pos[n] == int32_t(m);
  float pk = 0.f, fk = 0.f;
  if (own && lane < C && mode != 2) { pk = probs[m * C + lane]; fk = logits[n * C + lane]; }
  const float mb = wave_sum(pk * fk);  // same summation order as seed_kernel
  const float sp = sqrtf(pk), t = fk - mb;
  float al = 0.f, be = 0.f, ga = 0.f, u = 0.f;
  if (own && lane < C) {
    if (mode == 2) al = 1.41421356237309515f;
    else if (mode == 1) { al = sp * (1.f + 0.5f * t); be = sp; ga = 0.5f * sp * t; u = pk * (1.f + t); }
    else { al = sp; be = sp; u = pk; }
  }
  const int src = have ? c : 0;
  float sal = __shfl(al, src), sbe = __shfl(be, src), sga = __shfl(ga, src);  // (unconditional: every lane takes part)
  if (!have) { sal = 0.f; sbe = 0.f; sga = 0.f; }
  float* __restrict__ cs = coef + (2 * m) * kCoefRow;      // the node's own beta / gamma terms
  float* __restrict__ cn = coef + (2 * m + 1) * kCoefRow;  // a neighbour path from sample m
  cs[lane] = 0.f; cs[kCoefStride + lane] = -sbe; cs[2 * kCoefStride + lane] = -sga; cs[3 * kCoefStride + lane] = 0.f;
  cn[lane] = sal; cn[kCoefStride + lane] = -sbe; cn[2 * kCoefStride + lane] = -sga; cn[3 * kCoefStride + lane] = 0.f;
  alpha[m * kCoefStride + lane] = al;  // class major: the weights of the one-hot alpha paths (sage_path_list_kernel)
  if (lane < C) { up[m * C + lane] = u; up[(M + m) * C + lane] = own ? pk : 0.f; }
  // (per row of the coefficient table; the sample's seed block stands at its neighbour row: its self term has the same block)
  const uint32_t vb = seed_column_sum_max(al, be, ga, u, own ? pk : 0.f, C, lane);
  if (lane == 0) { vsum[2 * m] = 0u; vsum[2 * m + 1] = vb; }
}

// One wave per node n: its paths (see above).  Row n of P^T lists the samples' nodes v with P[v, n] != 0.
template <bool FILL>
__global__ __launch_bounds__(256) void sage_path_list_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             const float* __restrict__ val, int64_t N, int64_t M, int C,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                             const float* __restrict__ alpha, int32_t* __restrict__ pcnt,
                                                             const int32_t* __restrict__ pptr, int32_t* __restrict__ pm,
                                                             int32_t* __restrict__ pv, float* __restrict__ pw,
                                                             uint32_t* __restrict__ wsum) {
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int32_t s = rowptr[n], e = rowptr[n + 1];
  int32_t run = FILL ? pptr[n] : 0;
  float wabs = 0.f;  // (as in path_list_kernel)
  for (int32_t base = s; base < e; base += 64) {
    int32_t mv = INT32_MAX;
    float w = 0.f;
    if (base + lane < e) { mv = pos[col[base + lane]]; w = val[base + lane]; }
    const bool in = mv != INT32_MAX;
    const uint64_t bal = __ballot(in);
    if constexpr (FILL) {
      if (in) {
        const int32_t o = run + __popcll(bal & ((uint64_t(1) << lane) - 1));
        pm[o] = 2 * mv + 1; pv[o] = int32_t(n); pw[o] = w * float(mult[mv]);
        wabs += fabsf(w * float(mult[mv]));
      }
    }
    run += __popcll(bal);
  }
  const int32_t ms = pos[n];
  if (ms != INT32_MAX) {  // n is a batch node: its own beta / gamma path and the C one-hot alpha paths
    if constexpr (FILL) {
      const float tm = float(mult[ms]);
      if (lane == 0) { pm[run] = 2 * ms; pv[run] = int32_t(n); pw[run] = tm; wabs += tm; }
      if (lane < C) {
        pm[run + 1 + lane] = int32_t(2 * M) + lane; pv[run + 1 + lane] = int32_t(n);
        pw[run + 1 + lane] = tm * alpha[int64_t(ms) * kCoefStride + lane];
        wabs += fabsf(tm * alpha[int64_t(ms) * kCoefStride + lane]);
      }
    }
    run += 1 + C;
  }
  if (!FILL && lane == 0) pcnt[n] = run;
  if constexpr (FILL) path_wsum_max(wabs, lane, wsum);
}

// ---- the scale of the fused kernel's fp16 Gram (PathScale in paths.h) -----------------------------------------------------
// One workgroup of 256 threads, thread j = column j: cn_j and 1 / cn_j from the largest |W_1[c, j]| over the C rows of W1a (the
// fused kernel's W_1 operand) and, GraphSAGE, of W1b (the self half, which reaches Y through the table rows of the one-hot
// paths); the normalised copy W1n = W1a diag(cn) and the largest normalised entry of both; the launch's maxima start at zero here.
__global__ __launch_bounds__(256) void path_colscale_kernel(const float* __restrict__ W1a, const float* __restrict__ W1b, int ld,
                                                            int C, int H, float* __restrict__ sc) {
  const int j = threadIdx.x;
  uint32_t* __restrict__ bits = reinterpret_cast<uint32_t*>(sc);
  if (j < 4) bits[j] = 0u;
  __syncthreads();
  // the column's entries in registers (C <= kCoefStride; unrolled, so that the loads are in flight together: one workgroup
  // walking the rows one dependent load at a time took 19 us, latency and nothing else)
  float va[kCoefStride], vb[kCoefStride];
#pragma unroll
  for (int c = 0; c < kCoefStride; ++c) {
    const bool in = j < H && c < C;
    va[c] = in ? W1a[int64_t(c) * ld + j] : 0.f;
    vb[c] = in && W1b ? W1b[int64_t(c) * ld + j] : 0.f;
  }
  uint32_t mx = 0u;
#pragma unroll
  for (int c = 0; c < kCoefStride; ++c)
    mx = max(mx, max(__float_as_uint(va[c]) & 0x7fffffffu, __float_as_uint(vb[c]) & 0x7fffffffu));
  // cn = 2^(127 - eb) for the biased exponent eb of the column's maximum, kept inside fp32's normal range together with its
  // inverse; a column of zeros (or of subnormals: its squares vanish in fp32) stays as it is
  const uint32_t eb = mx >> 23, k = eb == 0u ? 127u : min(max(eb, 1u), 253u);
  const float cn = __uint_as_float((254u - k) << 23);
  sc[kScaleCn + j] = cn;
  sc[kScaleCinv + j] = __uint_as_float(k << 23);
  uint32_t wm = 0u;
#pragma unroll
  for (int c = 0; c < kCoefStride; ++c) {
    const float v = va[c] * cn;
    if (j < H && c < C) sc[kScaleW1 + int64_t(c) * H + j] = v;
    wm = max(wm, max(__float_as_uint(v) & 0x7fffffffu, __float_as_uint(vb[c] * cn) & 0x7fffffffu));
  }
  if (wm) atomicMax(&bits[1], wm);
}
// A wave per row r of the coefficient table at a time (a sample; GraphSAGE: a sample index): its largest |alpha|, |beta|,
// |gamma| over the 64 class slots (16 lanes per kind, 16 bytes per lane), its rows b_r, g_r of the table times cn -- written to
// bgn, which the fused kernel reads in the table's place -- and their largest entries; the row's entry of `vsum`.  The waves
// stride over the rows and keep their maxima in registers; a workgroup ends in three atomics at most.  bg == nullptr (regression): no beta / gamma term.
// A table row's power of two for the piece products from the bit pattern of its largest |entry|: up = 2^k with up * max in
// [2^kPieceRowLog2, 2 * 2^kPieceRowLog2), k kept in [-126, 126] (both powers normal numbers); down = 2^-k, and zero for a row
// of zeros.
struct PieceRow { float up, down; };
__device__ __forceinline__ PieceRow piece_row(uint32_t max_bits) {
  const int k = min(max(127 + kPieceRowLog2 - int(max_bits >> 23), -126), 126);
  return {__uint_as_float(uint32_t(127 + k) << 23), max_bits ? __uint_as_float(uint32_t(127 - k) << 23) : 0.f};
}
// x as (x0 | x1 << 16), x0 = fp16(x), x1 = fp16(x - x0), both rounded to nearest (split_pair of paths_fused.hip)
__device__ __forceinline__ uint32_t piece_pack(float x) {
  const _Float16 x0 = _Float16(x);
  const _Float16 x1 = _Float16(x - float(x0));
  return uint32_t(__builtin_bit_cast(uint16_t, x0)) | uint32_t(__builtin_bit_cast(uint16_t, x1)) << 16;
}
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
__global__ __launch_bounds__(256) void path_bound_kernel(const float* __restrict__ coef, int64_t rows, const float* __restrict__ bg,
                                                         float* __restrict__ bgn, int H, const uint32_t* __restrict__ vsum,
                                                         float* __restrict__ sc, int pieces) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t amax = 0u, xmax = 0u, vmax = 0u;
  f32x4 cn = {0.f, 0.f, 0.f, 0.f};
  if (4 * lane < H) cn = *reinterpret_cast<const f32x4*>(sc + kScaleCn + 4 * lane);
  for (int64_t r = int64_t(blockIdx.x) * 4 + wave; r < rows; r += int64_t(gridDim.x) * 4) {
    const f32x4 cf = *reinterpret_cast<const f32x4*>(coef + r * kCoefRow + 4 * lane);
    uint32_t km = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) km = max(km, __float_as_uint(cf[q]) & 0x7fffffffu);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) km = max(km, uint32_t(__shfl_xor(int(km), o)));  // (within the kind's 16 lanes)
    amax = max(amax, uint32_t(__shfl(int(km), 0)));
    vmax = max(vmax, vsum[r]);
    if (bg == nullptr) continue;
    const float be = __uint_as_float(uint32_t(__shfl(int(km), 16))), ga = __uint_as_float(uint32_t(__shfl(int(km), 32)));
    uint32_t bm = 0u, gm = 0u;
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f}, g4 = b4;
    if (4 * lane < H) {
      b4 = *reinterpret_cast<const f32x4*>(bg + r * H + 4 * lane) * cn;
      g4 = *reinterpret_cast<const f32x4*>(bg + (rows + r) * H + 4 * lane) * cn;
      *reinterpret_cast<f32x4*>(bgn + r * H + 4 * lane) = b4;
      *reinterpret_cast<f32x4*>(bgn + (rows + r) * H + 4 * lane) = g4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bm = max(bm, __float_as_uint(b4[q]) & 0x7fffffffu);
        gm = max(gm, __float_as_uint(g4[q]) & 0x7fffffffu);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      bm = max(bm, uint32_t(__shfl_xor(int(bm), o)));
      gm = max(gm, uint32_t(__shfl_xor(int(gm), o)));
    }
    // (0 * inf is NaN: a non-finite operand stays visible whatever it meets)
    xmax = max(xmax, __float_as_uint(be * __uint_as_float(bm) + ga * __uint_as_float(gm)) & 0x7fffffffu);
    if (!pieces) continue;  // (LGNN_GRAM_F32: the call cannot run the piece instance)
    // The same rows for the fused kernel's piece products (PathScale, "the piece table"): row m times the power of two that
    // puts its largest entry in [2^6, 2^7), every entry as two fp16 pieces in one dword, and the sample's coefficient row
    // with -beta / -gamma times the inverse power.  A row of zeros takes zero coefficients (its products are zero).
    const PieceRow pb = piece_row(bm), pg = piece_row(gm);
    if (4 * lane < H) {
      b4 *= pb.up; g4 *= pg.up;
      uint32_t* __restrict__ pt = reinterpret_cast<uint32_t*>(bgn + piece_table_offset(rows, H));
      *reinterpret_cast<u32x4*>(pt + r * H + 4 * lane) = u32x4{piece_pack(b4[0]), piece_pack(b4[1]), piece_pack(b4[2]), piece_pack(b4[3])};
      *reinterpret_cast<u32x4*>(pt + (rows + r) * H + 4 * lane) = u32x4{piece_pack(g4[0]), piece_pack(g4[1]), piece_pack(g4[2]), piece_pack(g4[3])};
    }
    const int kind = lane >> 4;  // (alpha | -beta | -gamma | pad)
    *reinterpret_cast<f32x4*>(bgn + piece_coef_offset(rows, H) + r * kCoefRow + 4 * lane) = cf * (kind == 1 ? pb.down : kind == 2 ? pg.down : 1.f);
  }
  __shared__ uint32_t red[3][4];
  if (lane == 0) { red[0][wave] = amax; red[1][wave] = xmax; red[2][wave] = vmax; }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t* __restrict__ bits = reinterpret_cast<uint32_t*>(sc);
    const uint32_t* v = red[threadIdx.x];
    const int slot = threadIdx.x == 0 ? 0 : int(threadIdx.x) + 1;  // [0] amax, [2] bgmax, [3] vmax
    atomic_max_bits(&bits[slot], max(max(v[0], v[1]), max(v[2], v[3])));
  }
}

__global__ void path_flag_kernel(const int32_t* __restrict__ pptr, int64_t n0, int64_t n, uint8_t* __restrict__ flags) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k < n) flags[k] = pptr[n0 + k + 1] > pptr[n0 + k] ? 1 : 0;
}

// S2 = sum_v (entries of row v of P) * (entries of row v of P^T): the number of 2-hop paths n <- v <- m of the whole graph
__global__ void two_hop_count_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ rpt, int64_t N,
                                     unsigned long long* __restrict__ out) {
  unsigned long long acc = 0;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < N; v += stride)
    acc += (unsigned long long)(rp[v + 1] - rp[v]) * (unsigned long long)(rpt[v + 1] - rpt[v]);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// max over m of the paths n <- k <- m that START at m: sum over the entries k of row m of P of the entries of row k of P.
// M times this bounds a batch's path count from the host (duplicated batch nodes share their paths).  With P^T's row pointers
// as `rp2`: the samples m' that can share a node k with m -- M times that bounds twice the pairs of toppairs.hip.
__global__ void two_hop_max_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col,
                                   const int32_t* __restrict__ rp2, int64_t N, unsigned long long* __restrict__ out) {
  unsigned long long best = 0;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; m < N; m += stride) {
    unsigned long long acc = 0;
    for (int32_t p = rp[m]; p < rp[m + 1]; ++p) { const int32_t k = col[p]; acc += (unsigned long long)(rp2[k + 1] - rp2[k]); }
    best = acc > best ? acc : best;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(best, o); best = t > best ? t : best; }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(out, best);
}
}  // namespace

// The path route's cost grows with the batch's number of 2-hop paths (about 1 ns each at C = 40 on top of the per-node Gram),
// the plane route's with the graph's entries: on hub-heavy graphs (sum of squared degrees) the planes win -- arxiv sizes with
// power-law degrees: 183.7 ms per fit on paths against 107.2 ms on planes; uniform degrees: 84 against 95.  The expected
// paths per destination node, S2 / N * M / N, decides; S2 is counted once per graph (one stream synchronisation).
int two_hop_ensure(lgnn_ctx* h, hipStream_t s) {
  if (h->two_hop >= 0) return 0;
  h->two_hop = 0;
  if (h->nnz <= 0) return 0;
  DevBuf acc;
  LGNN_CALL(acc.reserve(64));
  unsigned long long host[3] = {0, 0, 0};
  LGNN_HIP_CHECK(hipMemsetAsync(acc.p, 0, 24, s));
  const dim3 grid{unsigned(std::min<int64_t>(cdiv(h->N, 256), 1024))};
  hipLaunchKernelGGL(two_hop_count_kernel, grid, dim3(256), 0, s, h->P.rowptr, h->PT.rowptr, h->N, acc.as<unsigned long long>());
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(two_hop_max_kernel, grid, dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.rowptr, h->N,
                     acc.as<unsigned long long>() + 1);
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(two_hop_max_kernel, grid, dim3(256), 0, s, h->P.rowptr, h->P.col, h->PT.rowptr, h->N,
                     acc.as<unsigned long long>() + 2);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_HIP_CHECK(hipMemcpyAsync(host, acc.p, 24, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));
  h->two_hop = double(host[0]);
  h->two_hop_max = double(host[1]);
  h->pair_hop_max = double(host[2]);
  return 0;
}
// ... at most this many: arxiv's 13.7 take the path route, the power-law graph's 24x the node count keep the class planes
constexpr double kPathsPerNodeLimit = 24.0;
bool paths_pay(const lgnn_ctx* h, int64_t M) {
  const double N = double(h->N);
  return h->two_hop >= 0 && h->two_hop / N * double(M) / N <= kPathsPerNodeLimit;
}

bool paths_supported(int kind, int L, const int64_t* dims, int act, int64_t nnz) {
  const int64_t C = dims[L], H = L >= 2 ? dims[L - 1] : 0;
  return (kind == LGNN_KIND_GCN || kind == LGNN_KIND_SAGE) && L == 2 && act == LGNN_ACT_RELU && nnz > 0 && C <= kCoefStride &&
         H > 128 && H <= 256 && H % 4 == 0;
}

// Entries of a batch's path list buffer (arxiv shape: 2.2 M paths per batch of 10 000 against 10 M).  LGNN_PATH_LIST_CAP, read
// per call: tests force the enumerating route
static int64_t path_list_cap(const lgnn_ctx* h) {
  int64_t cap = std::max<int64_t>(4 * h->nnz, int64_t(1) << 22);
  if (const char* e = getenv("LGNN_PATH_LIST_CAP")) cap = std::max<int64_t>(1, std::min<int64_t>(cap, atoll(e)));
  return cap;
}
// The top layer runs on top_pairs_kernel (toppairs.hip) when the host knows that the batch's pairs fit a list of the path
// list's capacity (the same kind of bound as can_overflow below: no device-side gate, no synchronisation); otherwise on
// top_tiles_kernel.  LGNN_PAIR_LIST_CAP, read per call: tests lower the capacity to keep that kernel covered
bool top_pairs_fit(const lgnn_ctx* h, int64_t M) {
  int64_t cap = path_list_cap(h);
  if (const char* e = getenv("LGNN_PAIR_LIST_CAP")) cap = std::max<int64_t>(1, std::min<int64_t>(cap, atoll(e)));
  const int64_t bound = top_pairs_bound(h, M);
  return bound > 0 && bound <= cap;
}

// The nodes of [nb, ne) that have a path, as a device-side list (GraphSAGE: 65 % of the nodes at the arxiv shape; a short last
// batch of a GCN: 70 %): the fused kernel's node loop, its barriers and its staging pipeline then only see those.
static int path_node_list(lgnn_ctx* h, PathLists& pl, int64_t nb, int64_t ne, hipStream_t s) {
  Workspace& ws = h->ws;
  const int64_t n = ne - nb;
  LGNN_CALL(ws.path_flags.reserve(size_t(h->N)));
  LGNN_CALL(ws.path_nodes.reserve(size_t(h->N) * 4));
  LGNN_CALL(ws.path_nnodes.reserve(64));
  hipLaunchKernelGGL(path_flag_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, pl.pptr, nb, n, ws.path_flags.as<uint8_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  pl.nodes = ws.path_nodes.as<int32_t>(); pl.nnodes = ws.path_nnodes.as<int32_t>();
  return compact_flags(ws.path_flags.as<uint8_t>(), n, ws.path_nodes.as<int32_t>(), ws.path_nnodes.as<int32_t>(), ws.select_tmp, s);
}
// The workspace's buffers of a path list of at most `cap` entries (`pl` points at them); pcnt[N] = 0, the scan's last input.
// (A list that overflows `cap` is not filled and keeps wsum = 0: the fused kernel returns at once on it anyway.)
static int path_list_reserve(lgnn_ctx* h, int64_t cap, PathLists& pl, hipStream_t s) {
  Workspace& ws = h->ws;
  LGNN_CALL(ws.path_pcnt.reserve(size_t(h->N + 1) * 4));
  LGNN_CALL(ws.path_pptr.reserve(size_t(h->N + 2) * 4));  // (N + 1 pointers and the list's wsum, see below)
  LGNN_CALL(ws.path_pm.reserve(size_t(cap) * 4));
  LGNN_CALL(ws.path_pv.reserve(size_t(cap) * 4));
  LGNN_CALL(ws.path_pw.reserve(size_t(cap) * 4));
  LGNN_HIP_CHECK(hipMemsetAsync(ws.path_pcnt.as<int32_t>() + h->N, 0, 4, s));
  // max_n sum_paths |w| of the list (PathScale in paths.h) is part of the list: the filling kernel leaves its bit pattern in
  // the word behind the N + 1 pointers, and a cache entry's copy of pptr takes it along
  LGNN_HIP_CHECK(hipMemsetAsync(ws.path_pptr.as<int32_t>() + h->N + 1, 0, 4, s));
  pl.pptr = ws.path_pptr.as<int32_t>(); pl.pm = ws.path_pm.as<int32_t>(); pl.pv = ws.path_pv.as<int32_t>();
  pl.pw = ws.path_pw.as<float>();
  return 0;
}
static int path_zeros_ensure(Workspace& ws, hipStream_t s) {  // 1 KiB of zeros, cleared once
  LGNN_CALL(ws.path_zeros.reserve(1024));
  if (!ws.path_zeros_set) LGNN_HIP_CHECK(hipMemsetAsync(ws.path_zeros.p, 0, 1024, s));
  ws.path_zeros_set = true;
  return 0;
}

// What a batch's launches share; the drivers add W1 / w1_ld, M / n_coef and no_bg, the launchers what changes per class chunk
static YArgs path_args(lgnn_ctx* h, const PathLists& pl, int64_t cb, int64_t cap, int64_t nb, int64_t ne) {
  YArgs y{};
  y.rowptr = h->PT.rowptr; y.col = h->PT.col; y.val = h->PT.val;
  y.rptr = pl.rptr; y.r_m = pl.r_m; y.r_w = pl.r_w;
  y.pptr = pl.pptr; y.pm = pl.pm; y.pv = pl.pv; y.pw = pl.pw; y.cap = cap;
  y.list = pl.nodes; y.n_list = pl.nnodes;
  y.coef = h->ws.path_coef.as<float>(); y.bg = h->ws.path_bg.as<float>(); y.zeros = h->ws.path_zeros.as<float>();
  y.mask = h->fc.mask_bits[0].as<uint32_t>(); y.mask_words = int(cdiv(h->dims[1], 32));
  y.N = h->N; y.n0 = nb; y.n1 = ne; y.H = int(h->dims[1]); y.cb = int(cb);
  return y;
}

// The fused kernel's launch arguments from the batch's: the PathScale block of this accumulate (paths.h) and the normalised
// copies of W_1 and the b / g table in ws.path_scale / ws.path_bgn, two small launches on the stream.  W1b: GraphSAGE's self half.
static int path_scale_args(lgnn_ctx* h, YArgs& y, const float* W1b, int ld, hipStream_t s) {
  Workspace& ws = h->ws;
  const int64_t C = h->dims[2], H = y.H, rows = y.n_coef;
  LGNN_CALL(ws.path_scale.reserve(size_t(kScaleW1 + C * H) * 4));
  if (!y.no_bg) LGNN_CALL(ws.path_bgn.reserve(size_t(piece_coef_offset(rows, H) + rows * kCoefRow) * 4));
  float* sc = ws.path_scale.as<float>();
  hipLaunchKernelGGL(path_colscale_kernel, dim3(1), dim3(256), 0, s, y.W1, W1b, ld, int(C), int(H), sc);
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(path_bound_kernel, dim3(unsigned(std::min<int64_t>(cdiv(rows, 4), 1024))), dim3(256), 0, s, y.coef, rows,
                     y.no_bg ? static_cast<const float*>(nullptr) : y.bg, ws.path_bgn.as<float>(), int(H),
                     ws.path_vsum.as<uint32_t>(), sc, fused_pieces_possible() ? 1 : 0);
  LGNN_HIP_CHECK(hipGetLastError());
  y.scale = sc; y.W1 = sc + kScaleW1; y.w1_ld = int(H);
  if (!y.no_bg) y.bg = ws.path_bgn.as<float>();
  return 0;
}

// B_0 scratch += sum over the class columns [cb, ce) of this batch (see the file header).  Needs batch_prologue's
// probabilities / multiplicities / positions and the cached forward (logits, mask bits).
int kfac_paths_first_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int seed_mode, int64_t cb, int64_t ce, float* scratch,
                           hipStream_t s, int64_t nb, int64_t ne, BatchEntry* entry, bool* built, const TopTilesReq* top) {
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1];
  if (ne < 0) ne = N;
  LGNN_REQUIRE(nb >= 0 && nb <= ne && ne <= N, "internal: node range");
  if (nb == ne) return 0;
  Workspace& ws = h->ws;
  LGNN_REQUIRE(paths_supported(h->kind, h->L, h->dims, h->act, h->nnz), "internal: path route on an unsupported model");
  // ---- per-sample tables and b_m / g_m
  LGNN_CALL(ws.path_coef.reserve(size_t(M) * kCoefRow * 4));
  LGNN_CALL(ws.path_up.reserve(size_t(2 * M) * C * 4));
  LGNN_CALL(ws.path_bg.reserve(size_t(2 * M) * H * 4));
  LGNN_CALL(ws.path_vsum.reserve(size_t(M) * 4));
  // the wave that owns a sample also forms its rows b_m, g_m of the [2 M, H] table (16-byte loads of W_1's rows: a weight tensor
  // that is not 16-byte aligned takes the small GEMM instead)
  const bool no_bg = seed_mode == 2;
  const bool bg_in_tables = !no_bg && (reinterpret_cast<uintptr_t>(h->W[1]) & 15) == 0;
  hipLaunchKernelGGL(path_tables_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, ws.probs.as<float>(),
                     h->fc.out.as<float>(), idx, ws.pos.as<int32_t>(), M, N, int(C), int(cb), int(ce), seed_mode,
                     ws.path_coef.as<float>(), ws.path_up.as<float>(), h->W[1], int(H),
                     bg_in_tables ? ws.path_bg.as<float>() : static_cast<float*>(nullptr), ws.path_vsum.as<uint32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  if (!no_bg && !bg_in_tables) {
    GemmEpilogue none;
    LGNN_CALL(launch_gemm(ws.path_up.as<float>(), C, h->W[1], H, ws.path_bg.as<float>(), H, 2 * M, C, H, none, s));
  }
  const int64_t cap = path_list_cap(h);
  // the overflow route below is gated on the device (the host cannot know a batch's path count without a synchronisation).
  // What the host does know is a bound: M times the largest number of paths that start at one node (counted once per graph
  // beside the graph's total).  If that fits the list, no batch can overflow: no planes, no launches behind the fused kernel
  // (arxiv shape: 10 000 x 726 paths against a cap of 10 M entries -- the 6.9 GB of planes are never reserved).
  const bool can_overflow = !(h->two_hop_max >= 0 && double(M) * h->two_hop_max <= double(cap));
  // the list of nodes with paths pays when a good share of the nodes has none: with p expected paths per node that share is
  // about exp(-p) (a full arxiv-shaped batch: p = 13.7, every node has paths -- the list would be pure overhead, measured
  // +0.17 ms per launch; its last batch of 941 samples: p = 1.3, 28 % of the nodes without)
  const double ppn = h->two_hop >= 0 ? h->two_hop / double(N) * double(M) / double(N) : 1e9;
  const bool use_list = ppn < 2.5;
  const bool whole = nb == 0 && ne == N;  // (a node share builds its own node list: the cached one covers all N nodes)
  // ---- R, the path list and the node list depend on the graph and the batch's ids only: a batch-structure cache entry
  // (batchcache.hip) holds them from the second accumulate of a batch on, and none of the kernels below is launched
  LGNN_CALL(path_zeros_ensure(ws, s));
  if (entry && entry->refused) entry = nullptr;
  if (entry && entry->has_paths && entry->cap != cap) batch_cache_drop_paths(h, entry);
  const bool cached = entry && entry->has_paths;
  PathLists pl{};
  if (cached) {
    pl = {entry->rptr, entry->r_m, entry->r_w, entry->pptr, entry->pm, entry->pv, entry->pw, nullptr, nullptr};
  } else {
    // ---- R = P^T[:, batch]
    LGNN_CALL(ws.path_cnt.reserve(size_t(N + 1) * 4));
    LGNN_CALL(ws.path_rptr.reserve(size_t(N + 1) * 4));
    LGNN_CALL(ws.path_rm.reserve(size_t(std::max<int64_t>(h->nnz, 1)) * 4));
    LGNN_CALL(ws.path_rw.reserve(size_t(std::max<int64_t>(h->nnz, 1)) * 4));
    LGNN_HIP_CHECK(hipMemsetAsync(ws.path_cnt.p, 0, size_t(N + 1) * 4, s));
    hipLaunchKernelGGL(path_r_kernel<false>, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, ws.pos.as<int32_t>(),
                       ws.mult.as<int32_t>(), h->P.rowptr, h->P.col, h->P.val, ws.path_cnt.as<int32_t>(),
                       static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), static_cast<float*>(nullptr));
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(exclusive_scan_i32(ws.path_cnt.as<int32_t>(), ws.path_rptr.as<int32_t>(), N + 1, ws.select_tmp, s));
    LGNN_HIP_CHECK(hipMemsetAsync(ws.path_cnt.p, 0, size_t(N + 1) * 4, s));
    hipLaunchKernelGGL(path_r_kernel<true>, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, ws.pos.as<int32_t>(),
                       ws.mult.as<int32_t>(), h->P.rowptr, h->P.col, h->P.val, ws.path_cnt.as<int32_t>(),
                       ws.path_rptr.as<int32_t>(), ws.path_rm.as<int32_t>(), ws.path_rw.as<float>());
    LGNN_HIP_CHECK(hipGetLastError());
    // ---- the paths of every destination node: count (one wave per node), scan, fill -- when they fit the buffer
    LGNN_CALL(path_list_reserve(h, cap, pl, s));
    const dim3 pgrid{unsigned(cdiv(N, 4))};
    hipLaunchKernelGGL(path_list_kernel<false>, pgrid, dim3(256), 0, s, h->PT.rowptr, h->PT.col, h->PT.val, N,
                       ws.path_rptr.as<int32_t>(), ws.path_rm.as<int32_t>(), ws.path_rw.as<float>(), ws.path_pcnt.as<int32_t>(),
                       static_cast<const int32_t*>(nullptr), cap, static_cast<int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                       static_cast<float*>(nullptr), static_cast<uint32_t*>(nullptr));
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(exclusive_scan_i32(ws.path_pcnt.as<int32_t>(), ws.path_pptr.as<int32_t>(), N + 1, ws.select_tmp, s));
    hipLaunchKernelGGL(path_list_kernel<true>, pgrid, dim3(256), 0, s, h->PT.rowptr, h->PT.col, h->PT.val, N,
                       ws.path_rptr.as<int32_t>(), ws.path_rm.as<int32_t>(), ws.path_rw.as<float>(), ws.path_pcnt.as<int32_t>(),
                       ws.path_pptr.as<int32_t>(), cap, ws.path_pm.as<int32_t>(), ws.path_pv.as<int32_t>(), ws.path_pw.as<float>(),
                       ws.path_pptr.as<uint32_t>() + N + 1);
    LGNN_HIP_CHECK(hipGetLastError());
    pl.rptr = ws.path_rptr.as<int32_t>(); pl.r_m = ws.path_rm.as<int32_t>(); pl.r_w = ws.path_rw.as<float>();
  }
  if (use_list) {
    if (cached && whole && entry->has_nodes) {
      pl.nodes = entry->nodes; pl.nnodes = entry->nnodes;
    } else {
      LGNN_CALL(path_node_list(h, pl, nb, ne, s));
    }
  }
  if (entry && !cached) {  // (this call goes on with the workspace's copy: the entry may be refused for its size)
    LGNN_CALL(batch_cache_store_paths(h, entry, cap, use_list && whole, s));
    if (built) *built = true;
  }
  // ---- the top layer from the tables and R: B_1 scratch += sum_n G_n^T G_n, from sample pairs (toppairs.hip; the term lists
  // are the entry's, or built from R into the workspace and copied into an entry that holds R) or per node (toptiles.hip)
  if (top && top->pairs) {
    TopPairs tp{};
    if (entry && entry->has_pairs) {
      tp = {entry->pair_s, entry->pair_m, entry->pair_m2, entry->pair_w, entry->pair_n};
    } else {
      LGNN_CALL(build_top_pairs(h, idx, M, PathR{pl.rptr, pl.r_m, pl.r_w}, tp, s));
      if (entry && entry->has_paths) LGNN_CALL(batch_cache_store_pairs(h, entry, s));  // (this call goes on with the workspace's)
    }
    LGNN_CALL(launch_top_pairs(h, tp, M, cb, ce, top->scratch, s));
  } else if (top) {
    LGNN_CALL(launch_top_tiles(h, PathR{pl.rptr, pl.r_m, pl.r_w}, M, cb, ce, top->act_list, top->act_count, top->scratch, s));
  }
  YArgs y = path_args(h, pl, cb, cap, nb, ne);
  y.W1 = h->W[1]; y.w1_ld = int(H); y.M = M; y.n_coef = M; y.no_bg = no_bg ? 1 : 0; y.piece_share_log2 = kPieceShareLog2Gcn;
  YArgs yf = y;  // (the overflow route keeps W_1 and the table as they are)
  LGNN_CALL(path_scale_args(h, yf, nullptr, int(H), s));
  LGNN_CALL(launch_paths_fused(h, yf, cb, ce, scratch, s));
  return can_overflow ? launch_paths_overflow(h, y, cb, ce, scratch, s) : 0;
}

// GraphSAGE: the same from the batch's one-hop paths (see sage_path_tables_kernel); needs what kfac_paths_first_layer needs.
int kfac_paths_first_layer_sage(lgnn_ctx* h, const int64_t* idx, int64_t M, int seed_mode, int64_t cb, int64_t ce, float* scratch,
                                hipStream_t s, int64_t nb, int64_t ne) {
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1];
  if (ne < 0) ne = N;
  LGNN_REQUIRE(nb >= 0 && nb <= ne && ne <= N, "internal: node range");
  if (nb == ne) return 0;
  Workspace& ws = h->ws;
  LGNN_REQUIRE(h->kind == LGNN_KIND_SAGE && paths_supported(h->kind, h->L, h->dims, h->act, h->nnz),
               "internal: path route on an unsupported model");
  const int64_t T = 2 * M + C;  // sample indices: 2 m (own beta / gamma), 2 m + 1 (neighbour path), 2 M + c' (one-hot alpha)
  LGNN_CALL(ws.path_coef.reserve(size_t(T) * kCoefRow * 4));
  LGNN_CALL(ws.path_up.reserve(size_t(2 * M) * C * 4));
  LGNN_CALL(ws.path_bg.reserve(size_t(2 * T) * H * 4));
  LGNN_CALL(ws.path_alpha.reserve(size_t(M) * kCoefStride * 4));
  LGNN_CALL(ws.path_vsum.reserve(size_t(T) * 4));
  hipLaunchKernelGGL(sage_path_tables_kernel, dim3(unsigned(cdiv(M + C, 4))), dim3(256), 0, s, ws.probs.as<float>(),
                     h->fc.out.as<float>(), idx, ws.pos.as<int32_t>(), M, N, int(C), int(cb), int(ce), seed_mode,
                     ws.path_coef.as<float>(), ws.path_up.as<float>(), ws.path_alpha.as<float>(), ws.path_vsum.as<uint32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  // b rows [0, T): u^T [W_1s | W_1n] as rows (2 m, 2 m + 1), then W_1s[c', :]; g rows [T, 2 T): p^T [W_1s | W_1n], then zeros
  float* bg = ws.path_bg.as<float>();
  GemmEpilogue none;
  LGNN_CALL(launch_gemm(ws.path_up.as<float>(), C, h->W[1], 2 * H, bg, 2 * H, M, C, 2 * H, none, s));
  LGNN_CALL(launch_gemm(ws.path_up.as<float>() + M * C, C, h->W[1], 2 * H, bg + T * H, 2 * H, M, C, 2 * H, none, s));
  LGNN_HIP_CHECK(hipMemcpy2DAsync(bg + 2 * M * H, size_t(H) * 4, h->W[1], size_t(2 * H) * 4, size_t(H) * 4, size_t(C),
                                  hipMemcpyDeviceToDevice, s));
  LGNN_HIP_CHECK(hipMemsetAsync(bg + (T + 2 * M) * H, 0, size_t(C) * H * 4, s));
  LGNN_CALL(path_zeros_ensure(ws, s));
  // ---- the paths of every node: count (one wave per node), scan, fill.  At most nnz + (C + 1) M of them: the list always fits
  const int64_t cap = std::max<int64_t>(h->nnz, 1) + (C + 1) * M + 64;
  LGNN_REQUIRE(cap < (int64_t(1) << 31), "too many paths for one launch");
  PathLists pl{};  // (no R: the paths are one hop)
  LGNN_CALL(path_list_reserve(h, cap, pl, s));
  const dim3 pgrid{unsigned(cdiv(N, 4))};
  hipLaunchKernelGGL(sage_path_list_kernel<false>, pgrid, dim3(256), 0, s, h->PT.rowptr, h->PT.col, h->PT.val, N, M, int(C),
                     ws.pos.as<int32_t>(), ws.mult.as<int32_t>(), ws.path_alpha.as<float>(), ws.path_pcnt.as<int32_t>(),
                     static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                     static_cast<float*>(nullptr), static_cast<uint32_t*>(nullptr));
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(exclusive_scan_i32(ws.path_pcnt.as<int32_t>(), ws.path_pptr.as<int32_t>(), N + 1, ws.select_tmp, s));
  hipLaunchKernelGGL(sage_path_list_kernel<true>, pgrid, dim3(256), 0, s, h->PT.rowptr, h->PT.col, h->PT.val, N, M, int(C),
                     ws.pos.as<int32_t>(), ws.mult.as<int32_t>(), ws.path_alpha.as<float>(), ws.path_pcnt.as<int32_t>(),
                     ws.path_pptr.as<int32_t>(), ws.path_pm.as<int32_t>(), ws.path_pv.as<int32_t>(), ws.path_pw.as<float>(),
                     ws.path_pptr.as<uint32_t>() + N + 1);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(path_node_list(h, pl, nb, ne, s));
  YArgs y = path_args(h, pl, cb, cap, nb, ne);
  y.W1 = h->W[1] + H; y.w1_ld = int(2 * H);  // the neighbour half: the alpha term of the neighbour paths
  y.M = T; y.n_coef = T; y.no_bg = 0;        // (the one-hot alpha paths go through the beta product: never skipped)
  y.piece_share_log2 = kPieceShareLog2Sage;
  LGNN_CALL(path_scale_args(h, y, h->W[1], int(2 * H), s));
  return launch_paths_fused(h, y, cb, ce, scratch, s);
}

}  // namespace lgnn
