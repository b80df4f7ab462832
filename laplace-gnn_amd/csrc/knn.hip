// Exact k nearest neighbours of the rows of X [N, F] by squared Euclidean distance, self excluded: the kNN initial graph of
// the reference's `--init_graph knng` configurations (get_knn_graph, gnn/utils.py:355-369; handed to the model at
// gnn/marglik_training.py:407-408) without ever forming N x N distances.
//
// The ORDER is defined by (d, index) ascending with d the fp32 difference form  d_ij = sum_f (x_if - x_jf)^2  (dist2 below: one
// fixed summation order for every kernel that ranks).  Four stages:
//
//  1. knn_norms_kernel     n_i = sum_f x_if^2 in fp32, and max_j n_j (atomicMax on the bits of a non-negative float: the
//                          result does not depend on arrival order).
//  2. knn_filter_kernel    a workgroup owns 64 query rows and sweeps 64-column tiles of its column split; the products x_i.x_j
//                          run on v_mfma_f32_32x32x2_f32 (K staged through LDS, the lane layout of dense_nt_kernel, lora.hip);
//                          the epilogue forms the Gram-form distance g_ij = n_i + n_j - 2 x_i.x_j in registers and keeps, per
//                          query row, the KC = 64 smallest g with their indices: accepted candidates (g below the row's
//                          running threshold) go to a 128-slot LDS buffer, a row whose buffer passed 64 entries is cut back to
//                          its 64 smallest by a rank select, which also lowers the threshold.  The smallest g that was ever
//                          turned away -- at the threshold or by a select -- is kept per row.  No distance reaches HBM: the
//                          kernel writes 64 indices and one float per (row, split).
//                          With several column splits a split hands on only its max(16, 2 k) best; the rest counts as
//                          turned away.
//  3. knn_rerank_kernel    per row: difference-form distances of its candidates (all splits) from X itself, rank select by
//                          (d, index), the k best written out, and the certificate below evaluated.
//  4. knn_fallback_kernel  rows without a certificate, compacted on the device (rocPRIM select, sorted): brute force over all N
//                          points in the difference form, one workgroup per row, the same (d, index) order.
//
// The result is therefore exact always; the filter only decides how fast.
//
// Certificate.  u = 2^-24.  The MFMA accumulates the F products of p = x_i.x_j in fp32; all the bound needs is that each
// product and each addition is rounded at most once to fp32, in whatever order the instruction combines its two k (an fma
// chain is one such order):  |fl(p) - p| <= gamma_F sum_f |x_if x_jf| <= F u (n_i + n_j) / 2 (1 + O(F u)), and 2 p carries twice
// that.  The
// norms are sums of F non-negative terms (one rounding per square, one per add, any order): |fl(n_i) - n_i| <= (F + 1) u n_i
// (1 + O(F u)).  The epilogue's two operations fl(fl(n_i + n_j) - 2 fl(p)) each round a value of magnitude at most
// 2 (n_i + n_j): 4 u (n_i + n_j) together.  Summed:
//     |g_ij - d^2_ij| <= (F + (F + 1) + 4) u (n_i + n_j) (1 + O(F u)) <= (2 F + 8) u (fl(n_i) + max_j fl(n_j)) =: E_i,
// the three spare units absorbing the second-order terms and the use of the computed norms in E_i (F u << 1).
// The fp32 difference form has a RELATIVE error: each term rounds the difference and the square, the chain F times:
// fl(d_ij) >= d^2_ij (1 - (F + 2) u).  A point j that the filter turned away has g_ij >= g_rej,i, so
//     fl(d_ij) >= (g_rej,i - E_i) (1 - (F + 2) u),
// and it ranks after the k-th kept candidate whenever  g_rej,i - E_i > fl(d_k,i) (1 + (F + 4) u)  ((F + 2) u expanded to first
// order; two more units for the second-order term and the rounding of this very comparison).  A row that passes needs nothing
// else; a row that turned nothing away (fewer than KC + 1 other points in every split) has g_rej = +inf and passes trivially.
#include "device_utils.h"
#include "mfma_tile.h"
#include "lgnn_internal.h"

#include <cfloat>
#include <climits>

namespace lgnn {

namespace {

constexpr int KT = 64;            // rows / columns of a filter tile
constexpr int KC = 64;            // candidates kept per (row, split)
constexpr int KBUF = 2 * KC;      // LDS slots per row: a tile adds at most KT to a row that holds at most KC
constexpr int KK = 16, KLD = KK + 1;  // K slab staged through LDS, padded row
// LDS of the filter: two staging slabs, the candidate buffers, per-row counters / thresholds / rejected minima: 74 KiB, two
// workgroups per CU
constexpr size_t kFilterLds = size_t(2 * KT * KLD + 2 * KT * KBUF + 5 * KT) * 4;
constexpr int kMaxSplits = 8;
constexpr int kMaxK = 32;
constexpr float kU = 5.9604644775390625e-8f;  // 2^-24

// the one fp32 difference form every ranking kernel uses: four interleaved fma chains, the tail on the first
template <bool VEC>
__device__ __forceinline__ float dist2(const float* __restrict__ xi, const float* __restrict__ xj, int64_t F) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int64_t f = 0;
  for (; f + 3 < F; f += 4) {
    float y0, y1, y2, y3;
    if (VEC) {
      const float4 y = *reinterpret_cast<const float4*>(xj + f);
      y0 = y.x; y1 = y.y; y2 = y.z; y3 = y.w;
    } else {
      y0 = xj[f]; y1 = xj[f + 1]; y2 = xj[f + 2]; y3 = xj[f + 3];
    }
    const float t0 = xi[f] - y0, t1 = xi[f + 1] - y1, t2 = xi[f + 2] - y2, t3 = xi[f + 3] - y3;
    a0 = fmaf(t0, t0, a0); a1 = fmaf(t1, t1, a1); a2 = fmaf(t2, t2, a2); a3 = fmaf(t3, t3, a3);
  }
  for (; f < F; ++f) {
    const float t = xi[f] - xj[f];
    a0 = fmaf(t, t, a0);
  }
  const float d = (a0 + a1) + (a2 + a3);
  return d == d ? d : INFINITY;  // a NaN distance ranks last
}

// (d, index) as one 64-bit key: d >= 0 (or +inf), so its bits order like the value
__device__ __forceinline__ uint64_t key_of(float d, int32_t j) {
  return (uint64_t(__float_as_uint(d)) << 32) | uint32_t(j);
}
constexpr uint64_t kKeyNone = ~uint64_t(0) >> 1;  // above every key of a real point (index < 2^31, d <= +inf)

// ---- 1. row norms and their maximum -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_norms_kernel(const float* __restrict__ X, int64_t N, int64_t F, int64_t ld,
                                                        float* __restrict__ nrm, unsigned* __restrict__ nmax_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* __restrict__ x = X + row * ld;
  float a = 0.f;
  for (int64_t f = lane; f < F; f += 64) a = fmaf(x[f], x[f], a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (lane == 0) {
    nrm[row] = a;
    if (a == a) atomicMax(nmax_bits, __float_as_uint(a));
  }
}

// ---- 2. the Gram-form filter --------------------------------------------------------------------------------------------
struct FilterArgs {
  const float* X; int64_t N, F, ld;
  const float* nrm;
  int32_t* cand;   // [N][splits][keep], -1 where a split had fewer points
  float* rej;      // [N][splits] smallest g turned away (+inf: none)
  int splits;
  int keep;        // candidates a split hands to the rerank (<= KC)
  int vec;         // rows are 16-byte aligned: float4 staging
};

__device__ __forceinline__ bool g_less(float g, int32_t j, float g2, int32_t j2) { return g < g2 || (g == g2 && j < j2); }

// one wave cuts the buffer of `row` back to its `keep` smallest (g, index); slot order afterwards = rank.  Every lane takes
// two slots into registers (absent ones as (+inf, INT32_MAX): no real candidate has g = +inf, it would not have passed the
// threshold) and counts the slots below its own from broadcast LDS reads.  (A variant that broadcast the slots with v_readlane
// instead was measured slower: the comparisons, not the LDS reads, are the cost.)
__device__ __noinline__ void filter_select(float* cg, int32_t* ci, int* cnt, float* thr, float* rejc, int row, int keep,
                                           int lane) {
  const int c = cnt[row];  // <= KBUF, the same for every lane
  float* g = cg + row * KBUF;
  int32_t* ix = ci + row * KBUF;
  const bool has0 = lane < c, has1 = lane + 64 < c;
  const float g0 = has0 ? g[lane] : INFINITY, g1 = has1 ? g[lane + 64] : INFINITY;
  const int32_t i0 = has0 ? ix[lane] : INT32_MAX, i1 = has1 ? ix[lane + 64] : INT32_MAX;
  int r0 = 0, r1 = 0;
#pragma unroll 4
  for (int e = 0; e < c; ++e) {
    const float ge = g[e];
    const int32_t ie = ix[e];
    r0 += g_less(ge, ie, g0, i0) ? 1 : 0;
    r1 += g_less(ge, ie, g1, i1) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();  // every lane has read the whole row before any lane overwrites a slot
  if (has0 && r0 < keep) { g[r0] = g0; ix[r0] = i0; }
  if (has1 && r1 < keep) { g[r1] = g1; ix[r1] = i1; }
  if (has0 && r0 == keep - 1) thr[row] = g0;
  if (has1 && r1 == keep - 1) thr[row] = g1;
  if (has0 && r0 == keep) rejc[row] = fminf(rejc[row], g0);  // the smallest of what this select drops
  if (has1 && r1 == keep) rejc[row] = fminf(rejc[row], g1);
  if (lane == 0) cnt[row] = c < keep ? c : keep;
}

__global__ __launch_bounds__(256) void knn_filter_kernel(FilterArgs a) {
  extern __shared__ float lds[];
  float* As = lds;
  float* Bs = As + KT * KLD;
  float* cg = Bs + KT * KLD;
  int32_t* ci = reinterpret_cast<int32_t*>(cg + KT * KBUF);
  int* cnt = reinterpret_cast<int*>(ci + KT * KBUF);
  float* thr = reinterpret_cast<float*>(cnt + KT);
  float* rejc = thr + KT;
  float* rejw = rejc + KT;  // [2][KT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t i0 = int64_t(blockIdx.x) * KT;
  const int64_t ntiles = (a.N + KT - 1) / KT;
  const int64_t ct0 = ntiles * blockIdx.y / a.splits, ct1 = ntiles * (blockIdx.y + 1) / a.splits;
  if (tid < KT) { cnt[tid] = 0; thr[tid] = INFINITY; rejc[tid] = INFINITY; }
  // staging: thread <-> (row tid / 4, 4 consecutive k)
  const int srow = tid >> 2, sk = (tid & 3) * 4;
  const bool a_ok = i0 + srow < a.N;
  const float* __restrict__ ap = a.X + (a_ok ? i0 + srow : 0) * a.ld;
  // this lane's 16 query rows (fixed for the whole sweep) and their norms
  float ni[16], rej[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t i = acc_row(i0 + wr * 32, lane, r);
    ni[r] = i < a.N ? a.nrm[i] : 0.f;
    rej[r] = INFINITY;
  }
  auto fetch = [&](const float* __restrict__ p, bool ok, int64_t k0, float (&v)[4]) {
    const int64_t k = k0 + sk;
    if (ok && a.vec && k + 3 < a.F) {
      const float4 q = *reinterpret_cast<const float4*>(p + k);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (ok && k + e < a.F) ? p[k + e] : 0.f;
    }
  };
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t j0 = ct * KT;
    const bool b_ok = j0 + srow < a.N;
    const float* __restrict__ bp = a.X + (b_ok ? j0 + srow : 0) * a.ld;
    f32x16 acc;
    acc_zero(acc);
    float va[4], vb[4];
    fetch(ap, a_ok, 0, va);
    fetch(bp, b_ok, 0, vb);
    for (int64_t k0 = 0; k0 < a.F; k0 += KK) {
      __syncthreads();  // the previous slab's reads (and the previous tile's select) are done
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[srow * KLD + sk + e] = va[e];
        Bs[srow * KLD + sk + e] = vb[e];
      }
      __syncthreads();
      if (k0 + KK < a.F) {  // the next slab's loads fly under this slab's MFMAs
        fetch(ap, a_ok, k0 + KK, va);
        fetch(bp, b_ok, k0 + KK, vb);
      }
      tile_nt_step<KK, KLD>(As, wr * 32, Bs, wc * 32, lane, acc);
    }
    // epilogue: g = n_i + n_j - 2 x_i.x_j against the row's threshold
    const int64_t j = j0 + wc * 32 + (lane & 31);
    if (j < a.N) {
      const float nj = a.nrm[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = acc_row(wr * 32, lane, r);
        const int64_t i = i0 + t;
        if (i >= a.N || i == j) continue;
        const float g = (ni[r] + nj) - 2.f * acc[r];
        if (g < thr[t]) {
          const int slot = atomicAdd(&cnt[t], 1);  // slot order is arrival order; the SET is not, and only the set is used
          cg[t * KBUF + slot] = g;
          ci[t * KBUF + slot] = int32_t(j);
        } else {
          rej[r] = fminf(rej[r], g);
        }
      }
    }
    __syncthreads();
#pragma nounroll
    for (int t = wave * 16; t < wave * 16 + 16; ++t)
      if (cnt[t] > KC) filter_select(cg, ci, cnt, thr, rejc, t, KC, lane);
    // (the next tile's slab loop synchronises before anything reads cnt / thr again; F >= 1)
  }
  // smallest rejected g per row: this lane's 16 rows over the 32 lanes that share them, then the two column waves
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = rej[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    // (the row map of mfma_tile.h written out: this kernel's code is held instruction for instruction)
    if ((lane & 31) == 0) rejw[wc * KT + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)] = v;
  }
  __syncthreads();
#pragma nounroll
  for (int t = wave * 16; t < wave * 16 + 16; ++t) {
    const int64_t i = i0 + t;
    if (i >= a.N) break;
    if (cnt[t] > a.keep) filter_select(cg, ci, cnt, thr, rejc, t, a.keep, lane);  // a split hands on its `keep` best only
    const int c = cnt[t];
    if (lane < a.keep) a.cand[(i * a.splits + blockIdx.y) * a.keep + lane] = lane < c ? ci[t * KBUF + lane] : -1;
    if (lane == 0) a.rej[i * a.splits + blockIdx.y] = fminf(rejc[t], fminf(rejw[t], rejw[KT + t]));
  }
}

// ---- 3. rerank in the difference form, certificate ----------------------------------------------------------------------
struct RerankArgs {
  const float* X; int64_t N, F, ld;
  const float* nrm; const unsigned* nmax_bits;
  const int32_t* cand; const float* rej;
  int splits, keep, k;
  int32_t* nbr; float* dist;
  uint8_t* flag;  // 1: the row has no certificate
};

template <bool VEC>
__global__ __launch_bounds__(64) void knn_rerank_kernel(RerankArgs a) {
  __shared__ uint64_t keys[kMaxSplits * KC];
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int C = a.splits * a.keep;
  const float* __restrict__ xi = a.X + i * a.ld;
  for (int e = lane; e < C; e += 64) {
    const int32_t j = a.cand[i * C + e];
    keys[e] = j < 0 ? kKeyNone : key_of(dist2<VEC>(xi, a.X + int64_t(j) * a.ld, a.F), j);
  }
  __syncthreads();
  for (int e = lane; e < C; e += 64) {
    const uint64_t me = keys[e];
    if (me == kKeyNone) continue;
    int rank = 0;
    for (int q = 0; q < C; ++q) rank += keys[q] < me ? 1 : 0;  // keys of real points are distinct (one index once)
    if (rank >= a.k) continue;
    const float d = __uint_as_float(unsigned(me >> 32));
    a.nbr[i * a.k + rank] = int32_t(uint32_t(me));
    a.dist[i * a.k + rank] = d;
    if (rank == a.k - 1) {
      float rj = INFINITY;
      for (int s = 0; s < a.splits; ++s) rj = fminf(rj, a.rej[i * a.splits + s]);
      const float E = float(2 * a.F + 8) * kU * (a.nrm[i] + __uint_as_float(*a.nmax_bits));
      const bool ok = rj - E > d * (1.f + float(a.F + 4) * kU);  // false for NaN on either side
      a.flag[i] = ok ? 0 : 1;
    }
  }
}

// ---- 4. brute force for the rows without a certificate -------------------------------------------------------------------
constexpr int FB = 128;  // threads; every thread keeps its own sorted k-list in LDS (slot p of thread t at [p * FB + t])

template <bool VEC>
__global__ __launch_bounds__(FB) void knn_fallback_kernel(const float* __restrict__ X, int64_t N, int64_t F, int64_t ld, int k,
                                                          const int32_t* __restrict__ rows, int32_t* __restrict__ nbr,
                                                          float* __restrict__ dist) {
  __shared__ uint64_t lst[kMaxK * FB];
  __shared__ uint64_t red[FB];
  const int tid = threadIdx.x;
  const int64_t i = rows[blockIdx.x];
  const float* __restrict__ xi = X + i * ld;
  int m = 0;
  for (int64_t j = tid; j < N; j += FB) {
    if (j == i) continue;
    const uint64_t key = key_of(dist2<VEC>(xi, X + j * ld, F), int32_t(j));
    if (m == k && key > lst[(k - 1) * FB + tid]) continue;
    int p = m < k ? m++ : k - 1;
    for (; p > 0 && lst[(p - 1) * FB + tid] > key; --p) lst[p * FB + tid] = lst[(p - 1) * FB + tid];
    lst[p * FB + tid] = key;
  }
  int head = 0;
  for (int r = 0; r < k; ++r) {  // k rounds of a workgroup-wide minimum over the list heads
    const uint64_t mine = head < m ? lst[head * FB + tid] : kKeyNone;
    red[tid] = mine;
    __syncthreads();
    for (int o = FB / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] = red[tid + o] < red[tid] ? red[tid + o] : red[tid];
      __syncthreads();
    }
    const uint64_t best = red[0];
    __syncthreads();
    if (mine == best && best != kKeyNone) {  // keys are distinct: one owner
      ++head;
      nbr[i * k + r] = int32_t(uint32_t(best));
      dist[i * k + r] = __uint_as_float(unsigned(best >> 32));
    }
  }
}

}  // namespace
}  // namespace lgnn

using namespace lgnn;

// see include/laplace_gnn_hip.h
extern "C" int lgnn_knn(const float* X, int64_t N, int64_t F, int64_t ld, int k, int32_t* nbr, float* dist,
                        int64_t* num_fallback, void* stream) {
  LGNN_REQUIRE(k >= 1 && k <= kMaxK, "knn: k must lie in [1, 32]");
  LGNN_REQUIRE(N >= 2 && N <= int64_t(INT32_MAX), "knn: N must lie in [2, 2^31)");
  LGNN_REQUIRE(int64_t(k) < N, "knn: k must be smaller than N (self is excluded)");
  LGNN_REQUIRE(F >= 1 && ld >= F, "knn: F >= 1 and row stride ld >= F");
  if (!X || !nbr || !dist || !num_fallback) { set_error("null argument"); return 2; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  *num_fallback = 0;
  const int64_t tiles = cdiv(N, KT);
  // few row tiles: split the column sweep so that some thousand workgroups exist (N = 2 708: 43 row tiles for 256 CUs)
  int64_t splits = cdiv(1024, tiles);
  if (splits > kMaxSplits) splits = kMaxSplits;
  if (splits > tiles) splits = tiles;
  // What a split hands to the rerank: all KC candidates when there is one split; with several, its max(16, 2 k) best -- the
  // rerank evaluates splits * keep difference-form distances per row with one lane per candidate row (Cora, F = 1 433: 8 x 64
  // candidates cost as much as the whole filter), and a split's next best g joins the rejected minimum, so the certificate
  // still covers everything that was not handed on.
  int keep = KC;
  if (splits > 1) keep = 2 * k > 16 ? (2 * k < KC ? 2 * k : KC) : 16;
  const bool vec = ld % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
  // workspace of the call, O(N * KC * splits): one block carved into 256-byte aligned pieces (and rocPRIM's temporary)
  DevBuf ws, tmp;
  size_t off = 0;
  auto piece = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
  const size_t o_nrm = piece(size_t(N) * 4), o_nmax = piece(4), o_cand = piece(size_t(N) * splits * keep * 4),
               o_rej = piece(size_t(N) * splits * 4), o_flag = piece(size_t(N)), o_list = piece(size_t(N) * 4),
               o_count = piece(4);
  LGNN_CALL(ws.reserve(off));
  char* base = ws.as<char>();
  float* nrm = reinterpret_cast<float*>(base + o_nrm);
  unsigned* nmax = reinterpret_cast<unsigned*>(base + o_nmax);
  int32_t* cand = reinterpret_cast<int32_t*>(base + o_cand);
  float* rej = reinterpret_cast<float*>(base + o_rej);
  uint8_t* flag = reinterpret_cast<uint8_t*>(base + o_flag);
  int32_t* list = reinterpret_cast<int32_t*>(base + o_list);
  int32_t* count = reinterpret_cast<int32_t*>(base + o_count);
  LGNN_HIP_CHECK(hipMemsetAsync(nmax, 0, 4, s));
  hipLaunchKernelGGL(knn_norms_kernel, dim3(unsigned(cdiv(N, 4))), dim3(256), 0, s, X, N, F, ld, nrm, nmax);
  LGNN_HIP_CHECK(hipGetLastError());
  FilterArgs fa{X, N, F, ld, nrm, cand, rej, int(splits), keep, vec ? 1 : 0};
  LGNN_CALL(lds_opt_in<&knn_filter_kernel>(int(kFilterLds)));
  hipLaunchKernelGGL(knn_filter_kernel, dim3(unsigned(tiles), unsigned(splits)), dim3(256), kFilterLds, s, fa);
  LGNN_HIP_CHECK(hipGetLastError());
  RerankArgs ra{X, N, F, ld, nrm, nmax, cand, rej, int(splits), keep, k, nbr, dist, flag};
  LGNN_HIP_CHECK(hipMemsetAsync(flag, 1, size_t(N), s));  // a row that ranked fewer than k real candidates stays flagged
  if (vec) hipLaunchKernelGGL(knn_rerank_kernel<true>, dim3(unsigned(N)), dim3(64), 0, s, ra);
  else hipLaunchKernelGGL(knn_rerank_kernel<false>, dim3(unsigned(N)), dim3(64), 0, s, ra);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(compact_flags(flag, N, list, count, tmp, s));
  int32_t nfb = 0;
  LGNN_HIP_CHECK(hipMemcpyAsync(&nfb, count, 4, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));  // the one synchronisation of the call: how many rows go to the brute force
  *num_fallback = nfb;
  if (nfb > 0) {
    if (vec) hipLaunchKernelGGL(knn_fallback_kernel<true>, dim3(unsigned(nfb)), dim3(FB), 0, s, X, N, F, ld, k, list,
                                nbr, dist);
    else hipLaunchKernelGGL(knn_fallback_kernel<false>, dim3(unsigned(nfb)), dim3(FB), 0, s, X, N, F, ld, k, list,
                            nbr, dist);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_HIP_CHECK(hipStreamSynchronize(s));  // the workspace is a local: it may not go while the kernel reads it
  }
  return 0;
}
