// GCN top layer of the two-hop path route: B_1 scratch += sum over the active nodes n of G_n^T G_n, on the matrix pipes from
// what the path route has built anyway.
//
//     G_n[c, k] = sum_e w_e V_{m_e}[k, c]       over the entries e = (m_e, w_e) of row n of R = P^T[:, batch]
//               = d_ck sum_e w_e alpha_c^e + sum_e (w_e (-beta)_c^e) u_k^e + (w_e (-gamma)_c^e) p_k^e
//
// (the seed block is diagonal plus rank two: kfac_top.hip, seed_spmm_gram_kernel).  seed_spmm_gram_kernel rebuilds the coefficients
// of every (node, neighbour) pair from the probabilities and logits, finds the batch neighbours by walking the row of P^T with
// ballots and writes the tile row by row through LDS: ~300 vector instructions per pair on an issue-bound wave.  Here
//   * the coefficient rows (alpha | -beta | -gamma) and the rows (u, p) come from path_tables_kernel's tables (paths.hip),
//   * the pairs come from R (path_r_kernel; weights val * multiplicity), cached with the batch's path list,
//   * the rank-two sum is a v_mfma_f32_16x16x4_f32 product with the K slots (e0, beta) (e0, gamma) (e1, beta) (e1, gamma): two
//     entries per step.  A: lane (i = l & 15, q = l >> 4) holds w * coef[m][kind(q)][slots 4 i .. 4 i + 3] -- one 16-byte load
//     for the four class tiles (coef_slot order); B: lane (k, q) holds u or p of the entry at column 16 tk + k,
//   * the D layout of that product (column l & 15, rows 4 (l >> 4) + r) is a valid A and B operand layout of G_n^T G_n with the
//     classes visited in the order (tile t, register r, K slot q): the Gram runs on the register tiles, no LDS.
// One wave per active node, persistent; S (the upper 16 x 16 tiles of B_1) stays in registers across the wave's nodes and leaves
// through one workgroup reduction and one float atomic per element, as in seed_spmm_gram_kernel.
//
// The chain  list -> R pointers -> (m, w) -> table rows  is dependent loads: the R ranges of 64 of the wave's nodes are loaded at
// once (one per lane); the steps of those nodes form one sequence, whose (m, w) are loaded two steps ahead and whose table rows
// one step ahead of the products.
#include "device_utils.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

template <int NBLK>
struct TopOps {     // the operands of one step (two entries of R) as loaded
  f32x4 a;          // coef[m][-beta or -gamma][slots 4 i ..]
  f32x4 al;         // coef[m][alpha][slots 4 i' ..]
  float b[NBLK];    // u or p of the entry, one column per column tile
  float w;          // the entry's weight (0: no entry in this slot -- every operand above is zero then)
};

// (C > 48: 40 + 64 registers of S and G alone -- workgroups of 8 waves, two per SIMD, leave each wave 256 registers)
template <int NBLK>
__global__ __launch_bounds__(NBLK == 4 ? 512 : 1024) void top_tiles_kernel(const int32_t* __restrict__ rptr, const int32_t* __restrict__ r_m,
                                                         const float* __restrict__ r_w, const float* __restrict__ coef,
                                                         const float* __restrict__ up, int64_t M, int C, int cb, int ce,
                                                         const int32_t* __restrict__ act_list,
                                                         const int32_t* __restrict__ act_count, float* __restrict__ scratch) {
  constexpr int NT = NBLK * (NBLK + 1) / 2;
  __shared__ float red[NT * 256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int nwaves = blockDim.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int nct = (ce - cb + 15) >> 4;  // class tiles that hold a class of [cb, ce): the coefficient slots behind them are zero
  // the diagonal element of class c = cb + 16 t + i' sits in column c: the lane with (c & 15) == (l & 15), i.e. i' = (i - cb) & 15,
  // row i' = 4 q + r of class tile t, column tile c >> 4
  const int ip = (i - cb) & 15;
  const bool dlane = (ip >> 2) == q;
  const int rsel = dlane ? (ip & 3) : -1;  // the register of G[t][tk] that holds the lane's diagonal element (-1: none) ...
  const int dsh = (cb + ip) >> 4;          // ... in the column tile tk = t + dsh
  const bool want_al = (ip >> 2) == (q & 1) || (ip >> 2) == (q | 2);  // a diagonal lane or the lane it adds (l ^ 32)
  const int a_off = kCoefStride * (1 + (q & 1)) + 4 * i, al_off = 4 * ip;
  const float* __restrict__ upq = up + ((q & 1) ? M * C : 0);

  f32x4 S[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) S[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int total = *act_count;
  // node j of this wave is act_list[gw + j * stride]
  const int gw = blockIdx.x * nwaves + wave, stride = gridDim.x * nwaves;
  const int cnt = gw < total ? (total - gw + stride - 1) / stride : 0;
  for (int c0 = 0; c0 < cnt; c0 += 64) {
    const int cn = min(64, cnt - c0);
    int32_t s_l = 0, d_l = 0;  // lane j: first entry and number of entries of node j's row of R
    if (lane < cn) {
      const int32_t n = act_list[gw + int64_t(c0 + lane) * stride];
      s_l = rptr[n];
      d_l = rptr[n + 1] - s_l;
    }
    // step st of node j covers the entries 2 st, 2 st + 1; lanes q < 2 take the first, q >= 2 the second
    auto load_mw = [&](int j, int st, int32_t& m, float& w) {
      const int jj = min(j, 63);
      const int32_t sj = __builtin_amdgcn_readlane(s_l, jj), dj = __builtin_amdgcn_readlane(d_l, jj);
      const int e = 2 * st + (q >> 1);
      m = -1; w = 0.f;
      if (j < cn && e < dj) { m = r_m[sj + e]; w = r_w[sj + e]; }
    };
    auto load_ops = [&](int32_t m, float w, TopOps<NBLK>& o) {
      o.w = w;
      o.a = f32x4{0.f, 0.f, 0.f, 0.f};
      o.al = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int b = 0; b < NBLK; ++b) o.b[b] = 0.f;
      if (m >= 0) {
        const float* __restrict__ cm = coef + int64_t(m) * kCoefRow;
        o.a = *reinterpret_cast<const f32x4*>(cm + a_off);
        if (want_al) o.al = *reinterpret_cast<const f32x4*>(cm + al_off);
        const float* __restrict__ um = upq + int64_t(m) * C;
#pragma unroll
        for (int b = 0; b < NBLK; ++b) {  // columns past C: a clamped address, and zero
          const float v = um[min(16 * b + i, C - 1)];
          o.b[b] = 16 * b + i < C ? v : 0.f;
        }
      }
    };
    auto advance = [&](int& j, int& st) {  // the step after (j, st) in the sequence of all steps of the chunk's nodes
      const int32_t dj = __builtin_amdgcn_readlane(d_l, min(j, 63));
      if (j < cn && 2 * (st + 1) < dj) ++st;
      else { ++j; st = 0; }
    };
    int j0 = 0, st0 = 0, j1 = 0, st1 = 0;
    advance(j1, st1);
    int j2 = j1, st2 = st1;
    advance(j2, st2);
    TopOps<NBLK> cur;
    int32_t m1;
    float w1;
    load_mw(j0, st0, m1, w1);
    load_ops(m1, w1, cur);
    load_mw(j1, st1, m1, w1);

    f32x4 G[NBLK][NBLK];
    f32x4 asum = f32x4{0.f, 0.f, 0.f, 0.f};
    while (j0 < cn) {
      // ---- the build: G[t][tk] (+)= A_t B_tk.  (Class tiles past the range [cb, ce) have zero coefficients: exact zeros.)
      const f32x4 a = cur.a * cur.w;
      if (st0 == 0) {
        asum = cur.al * cur.w;
#pragma unroll
        for (int t = 0; t < NBLK; ++t)
#pragma unroll
          for (int tk = 0; tk < NBLK; ++tk)
            G[t][tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], cur.b[tk], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      } else {
        asum += cur.al * cur.w;
#pragma unroll
        for (int t = 0; t < NBLK; ++t)
#pragma unroll
          for (int tk = 0; tk < NBLK; ++tk)
            G[t][tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], cur.b[tk], G[t][tk], 0, 0, 0);
      }
      // the operands of the next step are asked for once this step's are consumed (they never hold registers side by side);
      // behind a node's last step the Gram below covers their latency
      int32_t m2;
      float w2;
      load_mw(j2, st2, m2, w2);  // two steps ahead
      load_ops(m1, w1, cur);     // one step ahead
      const int32_t d0 = __builtin_amdgcn_readlane(d_l, j0);
      if (2 * (st0 + 1) >= d0) {  // the node's last step: diagonal term, then the Gram of the finished tile
        // lanes q < 2 summed the even entries, lanes q >= 2 the odd ones
        f32x4 tot;
#pragma unroll
        for (int t = 0; t < 4; ++t) tot[t] = asum[t] + __shfl_xor(asum[t], 32);
        int rs = rsel, ds = dsh;
        asm volatile("" : "+v"(rs), "+v"(ds));  // (compared here, per node: not as 20 lane masks held in scalar registers)
        if (cb == 0) {
#pragma unroll
          for (int t = 0; t < NBLK; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) G[t][t][r] += rs == r ? tot[t] : 0.f;
        } else {
#pragma unroll
          for (int t = 0; t < NBLK; ++t)
#pragma unroll
            for (int tk = t; tk < NBLK; ++tk)
#pragma unroll
              for (int r = 0; r < 4; ++r) G[t][tk][r] += (rs == r && ds == tk - t) ? tot[t] : 0.f;
        }
        // S[tk][tk'] += sum over the classes (t, r, K slot q) of G[class][16 tk + .] G[class][16 tk' + .]
#pragma unroll
        for (int t = 0; t < NBLK; ++t)
          if (t < nct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int x = 0;
#pragma unroll
              for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
                for (int bj = bi; bj < NBLK; ++bj, ++x)
                  S[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(G[t][bi][r], G[t][bj][r], S[x], 0, 0, 0);
            }
          }
      }
      m1 = m2; w1 = w2;
      j0 = j1; st0 = st1;
      j1 = j2; st1 = st2;
      advance(j2, st2);
    }
  }

  // workgroup reduction of the register tiles through LDS, then one atomic per upper-triangular element
  for (int x = threadIdx.x; x < NT * 256; x += blockDim.x) red[x] = 0.f;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) atomicAdd(&red[t * 256 + (4 * q + r) * 16 + i], S[t][r]);
  __syncthreads();
  for (int x = threadIdx.x; x < NT * 256; x += blockDim.x) {
    const int t = x >> 8, ii = (x >> 4) & 15, jj = x & 15;
    int bi = 0, bj = 0, tt = t;  // t -> (bi <= bj)
    for (bi = 0; bi < NBLK; ++bi) {
      if (tt < NBLK - bi) { bj = bi + tt; break; }
      tt -= NBLK - bi;
    }
    const int row = bi * 16 + ii, colj = bj * 16 + jj;
    if (row <= colj && colj < C) atomicAdd(&scratch[int64_t(row) * C + colj], red[x]);
  }
}

template <int NBLK>
int top_tiles_launch(lgnn_ctx* h, const PathR& r, int64_t M, int64_t cb, int64_t ce, const int32_t* act_list,
                     const int32_t* act_count, float* scratch, hipStream_t s) {
  // one workgroup per CU: 16 waves, 4 per SIMD at the kernel's register count (C > 48: 8 waves)
  hipLaunchKernelGGL(top_tiles_kernel<NBLK>, dim3(256), dim3(NBLK == 4 ? 512 : 1024), 0, s, r.rptr, r.r_m, r.r_w, h->ws.path_coef.as<float>(),
                     h->ws.path_up.as<float>(), M, int(h->dims[h->L]), int(cb), int(ce), act_list, act_count, scratch);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_top_tiles(lgnn_ctx* h, const PathR& r, int64_t M, int64_t cb, int64_t ce, const int32_t* act_list,
                     const int32_t* act_count, float* scratch, hipStream_t s) {
  const int64_t C = h->dims[h->L];
  LGNN_REQUIRE(C <= kCoefStride && cb >= 0 && cb < ce && ce <= C, "internal: top-layer tiles need C <= 64 and a class range");
  LGNN_REQUIRE(r.rptr && r.r_m && r.r_w && act_list && act_count, "internal: top-layer tiles need R and the active rows");
  switch (int(cdiv(C, 16))) {
    case 1: return top_tiles_launch<1>(h, r, M, cb, ce, act_list, act_count, scratch, s);
    case 2: return top_tiles_launch<2>(h, r, M, cb, ce, act_list, act_count, scratch, s);
    case 3: return top_tiles_launch<3>(h, r, M, cb, ce, act_list, act_count, scratch, s);
    default: return top_tiles_launch<4>(h, r, M, cb, ce, act_list, act_count, scratch, s);
  }
}

}  // namespace lgnn
