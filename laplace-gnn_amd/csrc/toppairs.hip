// GCN top layer of the two-hop path route from sample pairs: the sum of toptiles.hip without a per-node tile and without a Gram.
//
//     G_n[c, k] = sum_m w_nm V_m[k, c],   V_m[k, c] = a_c d_kc - b_c u_k - c_c p_k        (R[n, m] = w_nm, path_r_kernel)
//     B_1 += sum_n G_n^T G_n = sum_m s_m V_m V_m^T + sum_{m < m'} q_mm' (V_m V_m'^T + V_m' V_m^T)
//     s_m = sum_n w_nm^2,   q_mm' = sum_n w_nm w_nm'
//
// G_n is diagonal plus rank 2 d_n with d_n = 1 or 2 for nine active nodes in ten: top_tiles_kernel's dense 48 x 48 x 48 Gram per
// node (72 of its 90 MFMAs at C = 40) multiplies mostly structure.  Expanded, with primes on the second sample,
//     (V V'^T)[k, k'] = d_kk' a_k a'_k + u_k X_k' + p_k Y_k' - (a b')_k u'_k' - (a c')_k p'_k'
//     X = (b.b') u' + (b.c') p' - b a',   Y = (c.b') u' + (c.c') p' - c a'            (products of vectors: element-wise)
// which is four outer products -- the four K slots of ONE v_mfma_f32_16x16x4_f32 per output tile -- plus a diagonal.  A term is a
// sample (weight s_m / 2, m' = m) or a pair of samples that share a node (weight w_nm w_nm': one term per shared node, nothing
// is merged across nodes); the kernel accumulates T += weight V V'^T, and T + T^T reaches the scratch through
// top_pairs_reduce_kernel.  The coefficient rows (a | -b | -c) are zero outside the call's class range, so class ranges,
// regression (b = c = 0) and upstream seeds (c = 0) need nothing special, and duplicated ids live in the weights.
//
// The term lists depend on the graph and the batch's ids only: built once per batch from R (count per node, scan, fill -- as
// the path list is) and kept in the batch-structure cache entry beside R.
#include "device_utils.h"
#include "paths.h"

namespace lgnn {

namespace {

// One wave per batch sample: s_m = sum over the entries of its column of R of w^2 (fp64 sum; 0 for a repeated or invalid id).
__global__ __launch_bounds__(256) void pair_s_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                     const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                     const int32_t* __restrict__ rowptr, const float* __restrict__ val,
                                                     float* __restrict__ sq) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t u = idx[m];
  double acc = 0.0;
  if (u >= 0 && u < N && pos[u] == int32_t(m)) {
    const float tm = float(mult[m]);
    const int32_t e = rowptr[u + 1];
    for (int32_t p = rowptr[u] + lane; p < e; p += 64) {
      const float w = val[p] * tm;  // the weight as path_r_kernel stores it
      acc += double(w) * double(w);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) sq[m] = float(acc);
}

// cnt[n] = d (d - 1) / 2 for the d entries of row n of R; cnt[N] = 0 (the scan's last input)
__global__ void pair_count_kernel(const int32_t* __restrict__ rptr, int64_t N, int32_t* __restrict__ cnt) {
  const int64_t n = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n > N) return;
  int32_t c = 0;
  if (n < N) {
    const int32_t d = rptr[n + 1] - rptr[n];
    c = d * (d - 1) / 2;  // (d <= kTopSlice on this route: no overflow)
  }
  cnt[n] = c;
}

// One wave per node: the unordered pairs (a < b) of its R entries, pair (a, b) at  ptr[n] + a d - a (a + 1) / 2 + (b - a - 1).
__global__ __launch_bounds__(256) void pair_fill_kernel(const int32_t* __restrict__ rptr, const int32_t* __restrict__ r_m,
                                                        const float* __restrict__ r_w, int64_t N,
                                                        const int32_t* __restrict__ ptr, int64_t cap, int32_t* __restrict__ pm,
                                                        int32_t* __restrict__ pm2, float* __restrict__ pw) {
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  if (int64_t(ptr[N]) > cap) return;  // (cannot happen: the host's bound chose this route; a write past the buffer must not either)
  const int32_t s = rptr[n], d = rptr[n + 1] - s;
  if (d < 2) return;
  const int32_t base = ptr[n];
  for (int32_t a = 0; a + 1 < d; ++a) {
    const int32_t ma = r_m[s + a];
    const float wa = r_w[s + a];
    const int32_t row = base + a * d - a * (a + 1) / 2 - (a + 1);
    for (int32_t b = a + 1 + lane; b < d; b += 64) {
      pm[row + b] = ma;
      pm2[row + b] = r_m[s + b];
      pw[row + b] = wa * r_w[s + b];
    }
  }
}

template <int NBLK>
struct PairOps {       // what one term reads, as loaded (lane i = l & 15 of K slot q = l >> 4; kind(q) = -beta or -gamma)
  f32x4 am, km;        // alpha and kind(q) of sample m at the elements 16 t + i of the four tiles
  f32x4 a2, k2;        // the same of sample m'
  float ua[NBLK];      // u (q even) or p (q odd) of m at 16 t + i
  float u2[NBLK], p2[NBLK];  // u and p of m' at 16 t + i
  // the four dots, one per 16-lane row q: slots 4 i .. 4 i + 3 of kind(q >> 1) of m and of kind(q & 1) of m' (ys is k2 when the
  // call's classes start at 0: slot order is tile order then)
  f32x4 xs, ys;
  float w;             // the term's weight (0: no term)
};

// the sum of v over the 16 lanes of a row, in every lane of the row: quad butterflies, then the mirrored quad / half row (whose
// lanes all hold their group's sum by then) -- four DPP moves, no LDS
__device__ __forceinline__ float row_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad_perm [2, 3, 0, 1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));  // row_mirror
  return v;
}
__device__ __forceinline__ float row_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// the elements 16 t + i (t < NBLK) of one coefficient kind of a sample: one 16-byte load when the call's classes start at 0
template <int NBLK, bool CB0>
__device__ __forceinline__ f32x4 coef_tiles(const float* __restrict__ row, int i, int cb) {
  if constexpr (CB0) return *reinterpret_cast<const f32x4*>(row + 4 * i);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NBLK; ++t) {
    const int rel = 16 * t + i - cb;  // (< 64: the table's window covers every class from cb on)
    const float x = row[coef_slot(max(rel, 0))];
    v[t] = rel >= 0 ? x : 0.f;
  }
  return v;
}

// Persistent waves over the flat term list: terms [0, M) are the samples (weight s_m / 2), terms [M, M + *npairs) the pairs.
// CB0: the call's class range starts at class 0 (cb == 0).
template <int NBLK, bool CB0>
__global__ __launch_bounds__(NBLK == 4 ? 512 : 1024) void top_pairs_kernel(const float* __restrict__ sq, const int32_t* __restrict__ pm,
                                                         const int32_t* __restrict__ pm2, const float* __restrict__ pw,
                                                         const int32_t* __restrict__ npairs, const float* __restrict__ coef,
                                                         const float* __restrict__ up, int64_t M, int C, int cb,
                                                         float* __restrict__ part) {
  constexpr int NT = NBLK * (NBLK + 1) / 2, kTiles = NBLK * NBLK, kSlots = NBLK == 4 ? 2 : 4;
  __shared__ f32x4 red[kSlots * kTiles * 64];  // kSlots waves' register tiles, lane by lane
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int nwaves = blockDim.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const bool lo = q < 2, odd = (q & 1) != 0;
  const int kq = kCoefStride * (1 + (q & 1));
  const float* __restrict__ upq = up + (odd ? M * C : 0);
  const float* __restrict__ upp = up + M * C;

  f32x4 T[NBLK][NBLK];
#pragma unroll
  for (int t = 0; t < NBLK; ++t)
#pragma unroll
    for (int tk = 0; tk < NBLK; ++tk) T[t][tk] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the diagonal term of class 16 t + i sits in tile (t, t), column i, row i = 4 q + r: register i & 3 of the lanes q == i >> 2
  const int rsel = (i >> 2) == q ? (i & 3) : -1;

  const int64_t n = M + int64_t(*npairs);
  const int64_t gw = blockIdx.x * nwaves + wave, stride = int64_t(gridDim.x) * nwaves;

  auto load_term = [&](int64_t x, int32_t& m, int32_t& m2, float& w) {  // (wave uniform)
    m = 0; m2 = 0; w = 0.f;
    if (x < M) { m = m2 = int32_t(x); w = 0.5f * sq[x]; }
    else if (x < n) { m = pm[x - M]; m2 = pm2[x - M]; w = pw[x - M]; }
    m = __builtin_amdgcn_readfirstlane(m);
    m2 = __builtin_amdgcn_readfirstlane(m2);
    w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w)));
  };
  auto load_ops = [&](int32_t m, int32_t m2, float w, PairOps<NBLK>& o) {
    const float* __restrict__ c1 = coef + int64_t(m) * kCoefRow;
    const float* __restrict__ c2 = coef + int64_t(m2) * kCoefRow;
    o.w = w;
    o.am = coef_tiles<NBLK, CB0>(c1, i, cb);
    o.km = coef_tiles<NBLK, CB0>(c1 + kq, i, cb);
    o.a2 = coef_tiles<NBLK, CB0>(c2, i, cb);
    o.k2 = coef_tiles<NBLK, CB0>(c2 + kq, i, cb);
    o.xs = *reinterpret_cast<const f32x4*>(c1 + kCoefStride * (1 + (q >> 1)) + 4 * i);
    if constexpr (CB0) o.ys = o.k2;
    else o.ys = *reinterpret_cast<const f32x4*>(c2 + kq + 4 * i);
    const float* __restrict__ ua = upq + int64_t(m) * C;
    const float* __restrict__ u2 = up + int64_t(m2) * C;
    const float* __restrict__ p2 = upp + int64_t(m2) * C;
#pragma unroll
    for (int t = 0; t < NBLK; ++t) {  // columns past C: a clamped address, and zero
      const int k = min(16 * t + i, C - 1);
      const bool in = 16 * t + i < C;
      const float va = ua[k], vu = u2[k], vp = p2[k];
      o.ua[t] = in ? va : 0.f;
      o.u2[t] = in ? vu : 0.f;
      o.p2[t] = in ? vp : 0.f;
    }
  };

  int32_t m1, m1b;
  float w1;
  PairOps<NBLK> cur;
  load_term(gw, m1, m1b, w1);
  load_ops(m1, m1b, w1, cur);
  load_term(gw + stride, m1, m1b, w1);
  for (int64_t x = gw; x < n; x += stride) {
    // the term two steps ahead and the table rows one step ahead are asked for before this step's products
    int32_t m2, m2b;
    float w2;
    load_term(x + 2 * stride, m2, m2b, w2);
    PairOps<NBLK> nxt;
    load_ops(m1, m1b, w1, nxt);
    if (cur.w != 0.f) {  // (wave uniform; a repeated id's sample term has weight 0)
      // row q sums (b.b') (b.c') (c.b') (c.c') over the 64 slots: four per lane, then the row's 16 lanes
      const float pd = row_sum(cur.xs[0] * cur.ys[0] + cur.xs[1] * cur.ys[1] + cur.xs[2] * cur.ys[2] + cur.xs[3] * cur.ys[3]);
      const float d00 = row_value(pd, 0), d01 = row_value(pd, 16), d10 = row_value(pd, 32), d11 = row_value(pd, 48);
      const float da = odd ? d10 : d00, db = odd ? d11 : d01;
      // K slots: (u | X) (p | Y) (a (-b') | u') (a (-c') | p'); the table's signs: X = da u' + db p' + (-b) a'
      float A[NBLK], B[NBLK];
#pragma unroll
      for (int t = 0; t < NBLK; ++t) {
        A[t] = lo ? cur.ua[t] : cur.am[t] * cur.k2[t];
        const float xy = da * cur.u2[t] + db * cur.p2[t] + cur.km[t] * cur.a2[t];
        B[t] = cur.w * (lo ? xy : (odd ? cur.p2[t] : cur.u2[t]));
      }
      // the diagonal first, into the tile the products then add to: where V vanishes (one class: p = 1) the two cancel exactly
      int rs = rsel;
      asm volatile("" : "+v"(rs));  // (compared here, per term: not as lane masks held in scalar registers)
#pragma unroll
      for (int t = 0; t < NBLK; ++t) {
        const float dv = cur.w * cur.am[t] * cur.a2[t];
#pragma unroll
        for (int r = 0; r < 4; ++r) T[t][t][r] += rs == r ? dv : 0.f;
      }
#pragma unroll
      for (int t = 0; t < NBLK; ++t)
#pragma unroll
        for (int tk = 0; tk < NBLK; ++tk) T[t][tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t], B[tk], T[t][tk], 0, 0, 0);
    }
    cur = nxt;
    m1 = m2; m1b = m2b; w1 = w2;
  }

  // Workgroup reduction of the register tiles through LDS, without atomics (the 36 ds_add_f32 per wave of a float-atomic
  // reduction took 47 us of a full batch's 83: DESIGN 12.22, reduction variants b and c): the upper waves store their tiles lane by lane (16-byte stores), the
  // waves below add them, at most kSlots waves at a time, until wave 0 holds the sum -- in a fixed order.
  for (int live = nwaves; live > 1;) {
    const int k = min(kSlots, live >> 1);
    if (wave >= live - k && wave < live) {
      const int slot = wave - (live - k);
#pragma unroll
      for (int t = 0; t < NBLK; ++t)
#pragma unroll
        for (int tk = 0; tk < NBLK; ++tk) red[(slot * kTiles + t * NBLK + tk) * 64 + lane] = T[t][tk];
    }
    __syncthreads();
    if (wave >= live - 2 * k && wave < live - k) {
      const int slot = wave - (live - 2 * k);
#pragma unroll
      for (int t = 0; t < NBLK; ++t)
#pragma unroll
        for (int tk = 0; tk < NBLK; ++tk) T[t][tk] += red[(slot * kTiles + t * NBLK + tk) * 64 + lane];
    }
    __syncthreads();
    live -= k;
  }
  if (wave == 0) {
#pragma unroll
    for (int t = 0; t < NBLK; ++t)
#pragma unroll
      for (int tk = 0; tk < NBLK; ++tk) red[(t * NBLK + tk) * 64 + lane] = T[t][tk];
  }
  __syncthreads();
  // T + T^T of the upper tiles goes to the workgroup's row of `part` (plain stores; top_pairs_reduce_kernel adds the rows).
  // Element (row, col) of a tile is register row & 3 of lane (row >> 2) * 16 + col
  const float* __restrict__ rf = reinterpret_cast<const float*>(red);
  for (int x = threadIdx.x; x < NT * 256; x += blockDim.x) {
    const int t = x >> 8, ii = (x >> 4) & 15, jj = x & 15;
    int bi = 0, bj = 0, tt = t;  // t -> (bi <= bj)
    for (bi = 0; bi < NBLK; ++bi) {
      if (tt < NBLK - bi) { bj = bi + tt; break; }
      tt -= NBLK - bi;
    }
    part[int64_t(blockIdx.x) * (NT * 256) + x] = rf[((bi * NBLK + bj) * 64 + (ii >> 2) * 16 + jj) * 4 + (ii & 3)] +
                                                  rf[((bj * NBLK + bi) * 64 + (jj >> 2) * 16 + ii) * 4 + (jj & 3)];
  }
}

// scratch (upper triangle) += the sum of the workgroups' rows of `part`, in a fixed order: a workgroup takes 16 elements, its
// 16 slices of 16 threads each a share of the rows (independent loads), then the slices' sums are added through LDS
template <int NBLK>
__global__ __launch_bounds__(256) void top_pairs_reduce_kernel(const float* __restrict__ part, int nparts, int C,
                                                               float* __restrict__ scratch) {
  constexpr int NT = NBLK * (NBLK + 1) / 2;
  __shared__ float sums[256];
  const int e = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int x = blockIdx.x * 16 + e;  // (the grid covers NT * 256 elements exactly)
  float acc = 0.f;
  for (int b0 = slice; b0 < nparts; b0 += 64) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = b0 + 16 * j < nparts ? part[int64_t(b0 + 16 * j) * (NT * 256) + x] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += v[j];
  }
  sums[threadIdx.x] = acc;
  __syncthreads();
  if (slice != 0) return;
  const int t = x >> 8, ii = (x >> 4) & 15, jj = x & 15;
  int bi = 0, bj = 0, tt = t;  // t -> (bi <= bj)
  for (bi = 0; bi < NBLK; ++bi) {
    if (tt < NBLK - bi) { bj = bi + tt; break; }
    tt -= NBLK - bi;
  }
  const int row = bi * 16 + ii, colj = bj * 16 + jj;
  if (row > colj || colj >= C) return;
  float tot = 0.f;
#pragma unroll
  for (int sl = 0; sl < 16; ++sl) tot += sums[sl * 16 + e];
  scratch[int64_t(row) * C + colj] += tot;
}

template <int NBLK>
int top_pairs_launch(lgnn_ctx* h, const TopPairs& p, int64_t M, int64_t cb, float* scratch, hipStream_t s) {
  // one workgroup per CU, as top_tiles_kernel; then the sum over the workgroups
  constexpr int NT = NBLK * (NBLK + 1) / 2, kGrid = 256;
  LGNN_CALL(h->ws.pair_part.reserve(size_t(kGrid) * NT * 256 * 4));
  if (cb == 0)
    hipLaunchKernelGGL((top_pairs_kernel<NBLK, true>), dim3(kGrid), dim3(NBLK == 4 ? 512 : 1024), 0, s, p.sq, p.pm, p.pm2, p.pw,
                       p.npairs, h->ws.path_coef.as<float>(), h->ws.path_up.as<float>(), M, int(h->dims[h->L]), int(cb),
                       h->ws.pair_part.as<float>());
  else
    hipLaunchKernelGGL((top_pairs_kernel<NBLK, false>), dim3(kGrid), dim3(NBLK == 4 ? 512 : 1024), 0, s, p.sq, p.pm, p.pm2, p.pw,
                       p.npairs, h->ws.path_coef.as<float>(), h->ws.path_up.as<float>(), M, int(h->dims[h->L]), int(cb),
                       h->ws.pair_part.as<float>());
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(top_pairs_reduce_kernel<NBLK>, dim3(NT * 16), dim3(256), 0, s, h->ws.pair_part.as<float>(), kGrid,
                     int(h->dims[h->L]), scratch);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

// The most pairs a batch of M samples can have: every sample m meets, at each entry n of its row of P, at most the entries of
// row n of P^T (h->pair_hop_max is the largest such sum over all m); a pair is counted from both sides.
int64_t top_pairs_bound(const lgnn_ctx* h, int64_t M) {
  if (h->pair_hop_max < 0) return -1;
  const double b = double(M) * h->pair_hop_max * 0.5;
  return b < 2.0e9 ? int64_t(b) + 1 : -1;
}

// ws.pair_* from R (the workspace's or a cache entry's) and the batch prologue's positions / multiplicities
int build_top_pairs(lgnn_ctx* h, const int64_t* idx, int64_t M, const PathR& r, TopPairs& out, hipStream_t s) {
  Workspace& ws = h->ws;
  const int64_t N = h->N, cap = top_pairs_bound(h, M);
  LGNN_REQUIRE(cap > 0, "internal: the pair list needs a bound");
  LGNN_CALL(ws.pair_s.reserve(size_t(M) * 4));
  LGNN_CALL(ws.pair_cnt.reserve(size_t(N + 1) * 4));
  LGNN_CALL(ws.pair_ptr.reserve(size_t(N + 1) * 4));
  LGNN_CALL(ws.pair_m.reserve(size_t(cap) * 4));
  LGNN_CALL(ws.pair_m2.reserve(size_t(cap) * 4));
  LGNN_CALL(ws.pair_w.reserve(size_t(cap) * 4));
  hipLaunchKernelGGL(pair_s_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, ws.pos.as<int32_t>(),
                     ws.mult.as<int32_t>(), h->P.rowptr, h->P.val, ws.pair_s.as<float>());
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(pair_count_kernel, dim3(unsigned(cdiv(N + 1, 256))), dim3(256), 0, s, r.rptr, N, ws.pair_cnt.as<int32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(exclusive_scan_i32(ws.pair_cnt.as<int32_t>(), ws.pair_ptr.as<int32_t>(), N + 1, ws.select_tmp, s));
  hipLaunchKernelGGL(pair_fill_kernel, dim3(unsigned(cdiv(N, 4))), dim3(256), 0, s, r.rptr, r.r_m, r.r_w, N,
                     ws.pair_ptr.as<int32_t>(), cap, ws.pair_m.as<int32_t>(), ws.pair_m2.as<int32_t>(), ws.pair_w.as<float>());
  LGNN_HIP_CHECK(hipGetLastError());
  out = {ws.pair_s.as<float>(), ws.pair_m.as<int32_t>(), ws.pair_m2.as<int32_t>(), ws.pair_w.as<float>(),
         ws.pair_ptr.as<int32_t>() + N};
  return 0;
}

int launch_top_pairs(lgnn_ctx* h, const TopPairs& p, int64_t M, int64_t cb, int64_t ce, float* scratch, hipStream_t s) {
  const int64_t C = h->dims[h->L];
  LGNN_REQUIRE(C <= kCoefStride && cb >= 0 && cb < ce && ce <= C, "internal: top-layer pairs need C <= 64 and a class range");
  LGNN_REQUIRE(p.sq && p.pm && p.pm2 && p.pw && p.npairs && M > 0, "internal: top-layer pairs need the term lists");
  switch (int(cdiv(C, 16))) {
    case 1: return top_pairs_launch<1>(h, p, M, cb, scratch, s);
    case 2: return top_pairs_launch<2>(h, p, M, cb, scratch, s);
    case 3: return top_pairs_launch<3>(h, p, M, cb, scratch, s);
    default: return top_pairs_launch<4>(h, p, M, cb, scratch, s);
  }
}

}  // namespace lgnn
