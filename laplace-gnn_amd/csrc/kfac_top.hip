// The top layer of the KFAC accumulate: g_{L-1} = P^T scatter(V) (GCN) resp. scatter(V) (GraphSAGE) as class-major planes,
// the row lists of a batch (which rows of those planes, and of the level below, are not identically zero) and, on the GCN's
// fused route, the top-layer Gram from the same pass.  kfac.hip's steps and kfac_top_planes reach the kernels through the
// launchers at the end of the file (kfac.h).
#include "kfac.h"

namespace lgnn {

namespace {

// GCN top layer: g[c][n][k] = sum_{v in row n of P^T} val * [v in batch] * seeds[pos[v]][c][k].
// One wave per node; the (few) batch neighbours are found with a ballot, their seed rows are
// accumulated in an LDS row of C*C floats and written out class-major.
__global__ void seed_spmm_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                 const float* __restrict__ val, int64_t N, int64_t C,
                                 const int32_t* __restrict__ pos, const float* __restrict__ seeds,
                                 float* __restrict__ g, uint8_t* __restrict__ active, int64_t cb, int64_t ce) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = int64_t(blockIdx.x) * (blockDim.x >> 6) + wave;
  if (n >= N) return;
  const int64_t CC = C * C;
  const int64_t q0 = cb * C, nq = (ce - cb) * C;  // only the class planes [cb, ce) are built
  float* buf = sm + int64_t(wave) * nq;
  bool any = false;
  const int32_t s = rowptr[n], e = rowptr[n + 1];
  for (int32_t base = s; base < e; base += 64) {
    const int32_t p = base + lane;
    int32_t mp = INT32_MAX;
    float v = 0.f;
    if (p < e) { mp = pos[col[p]]; v = val[p]; }
    unsigned long long mask = __ballot(mp != INT32_MAX);
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int64_t mm = __shfl(mp, b);
      const float vv = __shfl(v, b);
      const float* __restrict__ src = seeds + mm * CC;
      if (!any) {
        for (int64_t q = lane; q < nq; q += 64) buf[q] = vv * src[q0 + q];
        any = true;
      } else {
        for (int64_t q = lane; q < nq; q += 64) buf[q] += vv * src[q0 + q];
      }
    }
  }
  // each lane re-reads only what it wrote itself (q = lane mod 64): no barrier needed
  for (int64_t q = lane; q < nq; q += 64) {
    const int64_t c = (q0 + q) / C, k = (q0 + q) - c * C;
    g[(c * N + n) * C + k] = any ? buf[q] : 0.f;
  }
  if (lane == 0) active[n] = any ? 1 : 0;
}

// active[v] = 1 for every node v that has a batch node among its P^T neighbours, i.e. every column of the P rows of
// the batch nodes: these are the only rows of the top-layer gradient that are not identically zero.  One wave per sample.
__global__ __launch_bounds__(256) void mark_active_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                          const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, uint8_t* __restrict__ active) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) return;  // flagged by mark_batch_kernel
  const int32_t e = rowptr[n + 1];
  for (int32_t p = rowptr[n] + lane; p < e; p += 64) active[col[p]] = 1;
}

// GraphSAGE: the rows of the top-layer gradient that are not identically zero are the batch nodes themselves
__global__ void mark_batch_flags_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, uint8_t* __restrict__ active) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n >= 0 && n < N) active[n] = 1;
}

using f32x4 = __attribute__((ext_vector_type(4))) float;

// GCN top layer over the ACTIVE nodes only, with the top-layer Gram fused in:
//     G_n[c][k] = sum_{v in row n of P^T, v in batch} val * V_v[k, c]                 (c in [cb, ce))
//     g[c][n][:] = G_n[c][:]                        (class-major planes for the backward GEMM; skipped when !g)
//     S        += G_n^T G_n = sum_c g_c[n]^T g_c[n]  (v_mfma_f32_16x16x4_f32 on the LDS copy of G_n)
// One wave per active node, persistent: the NBLK*(NBLK+1)/2 upper 16x16 tiles of S stay in registers, are reduced
// through LDS once per workgroup and leave with one float atomic per element.
//
// The seed block V_v of a batch sample is never materialised: it is diagonal plus rank two,
//     fork exact : V[k,c] = sqrt(p_c) [d_kc - p_k (1 + f_k - mbar) + 1/2 (d_kc - p_k)(f_c - mbar)]
//                         = alpha_c d_kc - beta_c u_k - gamma_c p_k
//     upstream   : V[k,c] = sqrt(p_c) (d_kc - p_k)                      (gamma = 0, u = p)
// so the wave loads the sample's C probabilities and logits (320 B instead of the 6.4 KB block), lane c keeps
// (alpha, beta, gamma)_c, lane k keeps (u, p)_k, and row c of G_n is built by lane c from v_readlane broadcasts,
// two columns per step.  The kernel is issue bound (a wave64 VALU instruction occupies its SIMD for 4 cycles), which
// is why the instruction count per node, not the bytes, is what the layout below minimises.
// Before: seed blocks written by seed_kernel (64 MB per arxiv-shaped batch), read back 1.5 times per active node,
// planes for all N rows to HBM, a separate Gram kernel over them: 0.14 + 0.54 + 0.62 ms per batch.
template <int NBLK>
__global__ __launch_bounds__(1024) void seed_spmm_gram_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t N, int C,
    const int32_t* __restrict__ pos, const float* __restrict__ probs, const float* __restrict__ logits,
    const int32_t* __restrict__ mult, int fork_exact, float* __restrict__ g, const int32_t* __restrict__ act_list,
    const int32_t* __restrict__ act_count, int cb, int ce, float* __restrict__ scratch, int ldb,
    // hub rows cut into slices (see top_tasks_* below).  mode 0: act_list holds node ids, a node's task is its whole row;
    // mode 1: act_list holds (node or -1 - node, begin, end) triples -- a negative node marks a SLICE of a hub row, whose
    // partial tile is added to hub_tiles[long_slot[node]] instead of being finished here; mode 2: act_list holds the ids of
    // the sliced hubs, their summed tiles are read back from hub_tiles and finished (planes + Gram)
    int mode, const int32_t* __restrict__ long_slot, float* __restrict__ hub_tiles, const uint8_t* __restrict__ active) {
  constexpr int NT = NBLK * (NBLK + 1) / 2;
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int nwaves = blockDim.x >> 6;
  const int nrows = ce - cb, rp = (nrows + 3) & ~3;
  // buf[r][k], r = c - cb < rp, k < ldb (>= C rounded up to 8; == 2 mod 4 so that the 16 lanes of an MFMA operand read and
  // the 8-byte row writes of 16 consecutive lanes fall into distinct banks).  Rows >= nrows stay zero; columns >= C are
  // masked when read.
  float* __restrict__ buf = sm + size_t(wave) * rp * ldb;
  for (int q = lane; q < rp * ldb; q += 64) buf[q] = 0.f;
  const bool rowok = lane >= cb && lane < ce;
  float* __restrict__ rowp = buf + (rowok ? lane - cb : 0) * ldb;
  bool colok[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b) colok[b] = b * 16 + (lane & 15) < C;
  // plane stores: 16 bytes per lane when C % 4 == 0, else 4
  const bool vec = (C & 3) == 0;
  const int cw = vec ? C >> 2 : C;                // stored units per row
  const int nunits = nrows * cw;
  const int step_r = 64 / cw, step_k = 64 % cw, r0 = lane / cw, k0 = lane % cw;

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int total = *act_count;
  // Node j of this wave is act_list[gw + j * S].  list -> rowptr -> col -> pos is a chain of dependent loads; it is
  // taken off the critical path: list and rowptr for 64 of the wave's nodes at once (one per lane), col/val two nodes
  // ahead, pos one node ahead.
  const int gw = blockIdx.x * nwaves + wave, S = gridDim.x * nwaves;
  const int cnt = gw < total ? (total - gw + S - 1) / S : 0;
  for (int c0 = 0; c0 < cnt; c0 += 64) {
    const int cn = min(64, cnt - c0);
    int32_t n_l = 0, s_l = 0, e_l = 0;
    if (lane < cn) {
      const int64_t t = gw + int64_t(c0 + lane) * S;
      if (mode == 1) {
        n_l = act_list[3 * t];
        s_l = act_list[3 * t + 1];
        e_l = act_list[3 * t + 2];
      } else {
        n_l = act_list[t];
        if (mode == 0) { s_l = rowptr[n_l]; e_l = rowptr[n_l + 1]; }  // mode 2: no entries, the tile comes from hub_tiles
      }
    }
    auto load_entries = [&](int j, int32_t& cj, float& vj) {
      const int jj = min(j, 63);
      const int32_t sj = __builtin_amdgcn_readlane(s_l, jj), ej = __builtin_amdgcn_readlane(e_l, jj);
      cj = -1; vj = 0.f;
      if (j < cn && sj + lane < ej) { cj = col[sj + lane]; vj = val[sj + lane]; }
    };
    int32_t cA, cB, cC, mpA, mpB;
    float vA, vB, vC;
    load_entries(0, cA, vA);
    mpA = cA >= 0 ? pos[cA] : INT32_MAX;
    load_entries(1, cB, vB);
    for (int j = 0; j < cn; ++j) {
      mpB = cB >= 0 ? pos[cB] : INT32_MAX;  // node j + 1
      load_entries(j + 2, cC, vC);           // node j + 2
      const int32_t n_enc = __builtin_amdgcn_readlane(n_l, j);
      const bool slice = n_enc < 0;  // a slice of a hub row: its partial tile goes to hub_tiles
      const int64_t n = slice ? -1 - int64_t(n_enc) : int64_t(n_enc);
      const int32_t s = __builtin_amdgcn_readlane(s_l, j), e = __builtin_amdgcn_readlane(e_l, j);
      bool any = false;
      if (mode == 2) {  // the summed tile of a sliced hub
        any = active[n] != 0;
        if (any) {
          const float* __restrict__ src = hub_tiles + int64_t(long_slot[n]) * nrows * C;
          for (int q = lane; q < nrows * C; q += 64) buf[(q / C) * ldb + (q % C)] = src[q];
        }
      }
      for (int32_t base = s; base < e; base += 64) {
        int32_t mp = mpA, cu = cA;
        float v = vA;
        if (base > s) {  // rows with more than 64 stored entries: the rest is not prefetched
          const int32_t p = base + lane;
          mp = INT32_MAX; v = 0.f; cu = 0;
          if (p < e) { cu = col[p]; mp = pos[cu]; v = val[p]; }
        }
        unsigned long long mask = __ballot(mp != INT32_MAX);
        while (mask) {
          const int b = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const int64_t mm = __shfl(mp, b);
          const int64_t u = __shfl(cu, b);
          float pk = 0.f, fk = 0.f;
          if (lane < C && fork_exact != 2) { pk = probs[mm * C + lane]; fk = logits[u * C + lane]; }
          // a node listed t times in the batch counts t times (the dense reference's x[x_indices] backward)
          const float vv = __shfl(v, b) * float(mult[mm]);
          const float mb = wave_sum(pk * fk);  // same summation order as seed_kernel
          const float sp = sqrtf(pk), t = fk - mb;
          // fork_exact: 0 upstream, 1 fork-exact classification seeds; 2 regression: V = sqrt(2) I (only the diagonal term)
          const float alpha = fork_exact == 2 ? 1.41421356237309515f : (fork_exact ? sp * (1.f + 0.5f * t) : sp);
          const float nbeta = -sp, ngamma = fork_exact == 1 ? -0.5f * sp * t : 0.f;
          int uvi = __float_as_int(vv * (fork_exact == 1 ? pk * (1.f + t) : pk));
          int pvi = __float_as_int(fork_exact == 1 ? vv * pk : 0.f);
          // Both are read with v_readlane (which ignores EXEC) inside the rowok region below, from lanes that are not
          // part of it: pin their computation here, for all lanes, so that it is not sunk into that region.
          asm volatile("" : "+v"(uvi), "+v"(pvi));
          // 4 column pairs per trip, no guards inside (ldb covers C rounded up to 8; lanes >= C hold zeros); the
          // readlanes are convergent, so only constant trip counts unroll
          if (rowok) {
            if (!any) {
              for (int k8 = 0; k8 < C; k8 += 8) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                  const int k = k8 + 2 * w;
                  const float u0 = __int_as_float(__builtin_amdgcn_readlane(uvi, k));
                  const float u1 = __int_as_float(__builtin_amdgcn_readlane(uvi, k + 1));
                  const float p0 = __int_as_float(__builtin_amdgcn_readlane(pvi, k));
                  const float p1 = __int_as_float(__builtin_amdgcn_readlane(pvi, k + 1));
                  *reinterpret_cast<float2*>(rowp + k) = make_float2(nbeta * u0 + ngamma * p0, nbeta * u1 + ngamma * p1);
                }
              }
            } else {
              for (int k8 = 0; k8 < C; k8 += 8) {
                float2 o[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) o[w] = *reinterpret_cast<float2*>(rowp + k8 + 2 * w);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                  const int k = k8 + 2 * w;
                  const float u0 = __int_as_float(__builtin_amdgcn_readlane(uvi, k));
                  const float u1 = __int_as_float(__builtin_amdgcn_readlane(uvi, k + 1));
                  const float p0 = __int_as_float(__builtin_amdgcn_readlane(pvi, k));
                  const float p1 = __int_as_float(__builtin_amdgcn_readlane(pvi, k + 1));
                  o[w].x += nbeta * u0 + ngamma * p0; o[w].y += nbeta * u1 + ngamma * p1;
                  *reinterpret_cast<float2*>(rowp + k) = o[w];
                }
              }
            }
          }
          if (rowok) rowp[lane] += vv * alpha;  // the diagonal term, column k = c
          any = true;
        }
      }
      mpA = mpB; cA = cB; vA = vB; cB = cC; vB = vC;
      if (!any) continue;  // a slice without batch neighbours, an inactive hub; cannot happen for a listed whole node
      // the other lanes' LDS writes are read below: same wave, LDS executes a wave's operations in order
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (slice) {
        float* __restrict__ dst = hub_tiles + int64_t(long_slot[n]) * nrows * C;
        for (int q = lane; q < nrows * C; q += 64) atomicAdd(&dst[q], buf[(q / C) * ldb + (q % C)]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next task overwrites the tile
        continue;
      }
      if (g) {
        int r = r0, k = k0;
        float* __restrict__ gn = g + (int64_t(cb) * N + n) * C;
        const int64_t plane = N * C;
        for (int qb = lane; qb < nunits; qb += 64 * 4) {
          float4 t4[4];
          int64_t off[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const bool ok = qb + 64 * w < nunits;
            if (vec) {
              const float* src = buf + r * ldb + 4 * k;
              const float2 lo = ok ? *reinterpret_cast<const float2*>(src) : make_float2(0.f, 0.f);
              const float2 hi = ok ? *reinterpret_cast<const float2*>(src + 2) : make_float2(0.f, 0.f);
              t4[w] = make_float4(lo.x, lo.y, hi.x, hi.y);
              off[w] = r * plane + 4 * k;
            } else {
              t4[w].x = ok ? buf[r * ldb + k] : 0.f;
              off[w] = r * plane + k;
            }
            r += step_r; k += step_k;
            if (k >= cw) { k -= cw; ++r; }
          }
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            if (qb + 64 * w < nunits) {
              if (vec) *reinterpret_cast<float4*>(gn + off[w]) = t4[w];
              else gn[off[w]] = t4[w].x;
            }
          }
        }
      }
      const float* __restrict__ xb = buf + (lane >> 4) * ldb + (lane & 15);
      for (int kk = 0; kk < rp; kk += 4) {
        float x[NBLK];
#pragma unroll
        for (int b = 0; b < NBLK; ++b) x[b] = colok[b] ? xb[kk * ldb + b * 16] : 0.f;
        int t = 0;
#pragma unroll
        for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
          for (int bj = bi; bj < NBLK; ++bj, ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[bi], x[bj], acc[t], 0, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // workgroup reduction of the register tiles through LDS, then one atomic per upper-triangular element
  __syncthreads();
  float* __restrict__ red = sm;  // NT * 256 floats (the launcher sizes the allocation for it)
  for (int q = threadIdx.x; q < NT * 256; q += blockDim.x) red[q] = 0.f;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) atomicAdd(&red[t * 256 + (4 * (lane >> 4) + r) * 16 + (lane & 15)], acc[t][r]);
  __syncthreads();
  for (int q = threadIdx.x; q < NT * 256; q += blockDim.x) {
    const int t = q >> 8, ii = (q >> 4) & 15, jj = q & 15;
    int bi = 0, bj = 0, tt = t;  // t -> (bi <= bj)
    for (bi = 0; bi < NBLK; ++bi) {
      if (tt < NBLK - bi) { bj = bi + tt; break; }
      tt -= NBLK - bi;
    }
    const int i = bi * 16 + ii, j = bj * 16 + jj;
    if (i <= j && j < C) atomicAdd(&scratch[int64_t(i) * C + j], red[q]);
  }
}

// Hub rows of the top layer.  A node's cost in seed_spmm_gram_kernel is its number of batch neighbours, walked by ONE wave
// (~2 us of issue-bound SIMD time per pair): on a power-law graph the largest hub (arxiv_powerlaw: 5 474 entries, ~330 in a
// batch) finishes alone long after the other waves (0.70 ms per batch against 0.29 ms on the uniform graph).  Rows with
// more than kTopSlice entries are therefore cut into slices that different waves take; a slice adds its partial tile to the
// hub's tile in global memory (float atomics) and a second, small launch finishes the summed tiles (planes + Gram).
// Per batch: one count / scan / fill pass over the active list builds the task triples.
__global__ void top_tasks_count_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                       const int32_t* __restrict__ rowptr, int64_t N, int32_t* __restrict__ cnt) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= N) return;
  int32_t c = 0;
  if (k < *count) {
    const int32_t n = list[k];
    const int32_t deg = rowptr[n + 1] - rowptr[n];
    c = deg > kTopSlice ? (deg + kTopSlice - 1) / kTopSlice : 1;
  }
  cnt[k] = c;
}
__global__ void top_tasks_fill_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cnt,
                                      const int32_t* __restrict__ offs, int32_t* __restrict__ tasks,
                                      int32_t* __restrict__ task_count) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int32_t total = *count;
  if (k >= total) return;
  const int32_t n = list[k], c = cnt[k], o = offs[k];
  const int32_t rs = rowptr[n], re = rowptr[n + 1];
  if (c == 1) {
    tasks[3 * o] = n; tasks[3 * o + 1] = rs; tasks[3 * o + 2] = re;
  } else {
    for (int32_t i = 0; i < c; ++i) {
      tasks[3 * (o + i)] = -1 - n;
      tasks[3 * (o + i) + 1] = rs + i * kTopSlice;
      tasks[3 * (o + i) + 2] = min(rs + (i + 1) * kTopSlice, re);
    }
  }
  if (k == total - 1) *task_count = o + c;
}

template <int NBLK>
int seed_spmm_gram_launch(lgnn_ctx* h, bool fork_exact, float* g, int64_t cb, int64_t ce, float* scratch, hipStream_t s,
                          const ActiveRows& rows) {
  const int C = int(h->dims[h->L]);
  constexpr int NT = NBLK * (NBLK + 1) / 2;
  const int rp = (int(ce - cb) + 3) & ~3;
  const int ldb = ((C + 7) & ~7) + 2;  // rows hold C rounded up to 8 columns; == 2 mod 4 keeps the LDS banks apart
  const size_t per_wave = size_t(rp) * ldb * 4;
  const int waves = int(std::max<size_t>(1, std::min<size_t>(16, (150 * 1024) / per_wave)));
  // + 64 floats: an MFMA operand read of the last row may run past it (those lanes are masked)
  const size_t smem = std::max(per_wave * waves + 256, size_t(NT) * 256 * 4);
  LGNN_REQUIRE(smem <= 158 * 1024, "too many classes for the seed SpMM kernel (use class ranges)");
  LGNN_CALL(lds_opt_in<&seed_spmm_gram_kernel<NBLK>>(158 * 1024));
  const int per_cu = int(std::max<size_t>(1, std::min<size_t>(2048 / (64 * waves), (158 * 1024) / smem)));
  const int fe = h->lik == LGNN_LIK_REGRESSION ? 2 : (fork_exact ? 1 : 0);
  LGNN_CALL(long_rows_ensure(h, s));
  if (h->n_top_multi <= 0) {
    hipLaunchKernelGGL(seed_spmm_gram_kernel<NBLK>, dim3(unsigned(256 * per_cu)), dim3(64 * waves), smem, s, h->PT.rowptr,
                       h->PT.col, h->PT.val, h->N, C, h->ws.pos.as<int32_t>(), h->ws.probs.as<float>(),
                       h->fc.out.as<float>(), h->ws.mult.as<int32_t>(), fe, g, rows.list,
                       rows.count, int(cb), int(ce), scratch, ldb, 0,
                       static_cast<const int32_t*>(nullptr), static_cast<float*>(nullptr), static_cast<const uint8_t*>(nullptr));
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  }
  // sliced hubs: task triples of this batch's active nodes, partial tiles, then the finishing launch over the sliced hubs
  const int64_t N = h->N, nrows = ce - cb;
  const int64_t cap = N + h->n_top_slices;
  LGNN_CALL(h->top_cnt.reserve(size_t(N) * 4));
  LGNN_CALL(h->top_offs.reserve(size_t(N) * 4));
  LGNN_CALL(h->top_tasks.reserve(size_t(cap) * 12));
  LGNN_CALL(h->top_task_count.reserve(64));
  LGNN_CALL(h->top_hub_tiles.reserve(size_t(h->n_long) * nrows * C * 4));
  LGNN_HIP_CHECK(hipMemsetAsync(h->top_task_count.p, 0, 4, s));
  LGNN_HIP_CHECK(hipMemsetAsync(h->top_hub_tiles.p, 0, size_t(h->n_long) * nrows * C * 4, s));
  hipLaunchKernelGGL(top_tasks_count_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, rows.list,
                     rows.count, h->PT.rowptr, N, h->top_cnt.as<int32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_CALL(exclusive_scan_i32(h->top_cnt.as<int32_t>(), h->top_offs.as<int32_t>(), N, h->ws.select_tmp, s));
  hipLaunchKernelGGL(top_tasks_fill_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, rows.list,
                     rows.count, h->PT.rowptr, h->top_cnt.as<int32_t>(), h->top_offs.as<int32_t>(),
                     h->top_tasks.as<int32_t>(), h->top_task_count.as<int32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(seed_spmm_gram_kernel<NBLK>, dim3(unsigned(256 * per_cu)), dim3(64 * waves), smem, s, h->PT.rowptr,
                     h->PT.col, h->PT.val, h->N, C, h->ws.pos.as<int32_t>(), h->ws.probs.as<float>(),
                     h->fc.out.as<float>(), h->ws.mult.as<int32_t>(), fe, g, h->top_tasks.as<int32_t>(),
                     h->top_task_count.as<int32_t>(), int(cb), int(ce), scratch, ldb, 1, h->long_slot.as<int32_t>(),
                     h->top_hub_tiles.as<float>(), rows.flags);
  LGNN_HIP_CHECK(hipGetLastError());
  // finishing launch: one wave per sliced hub (its count is a property of the graph: a constant in device memory)
  const unsigned fin_blocks = unsigned(std::min<int64_t>(cdiv(h->n_top_multi, waves), 256 * per_cu));
  hipLaunchKernelGGL(seed_spmm_gram_kernel<NBLK>, dim3(fin_blocks), dim3(64 * waves), smem, s, h->PT.rowptr, h->PT.col,
                     h->PT.val, h->N, C, h->ws.pos.as<int32_t>(), h->ws.probs.as<float>(), h->fc.out.as<float>(),
                     h->ws.mult.as<int32_t>(), fe, g, h->top_multi.as<int32_t>(), h->top_multi.as<int32_t>() + h->n_top_multi, int(cb), int(ce),
                     scratch, ldb, 2, h->long_slot.as<int32_t>(), h->top_hub_tiles.as<float>(),
                     rows.flags);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// GraphSAGE top layer: the last Linear's output is not propagated, so grad wrt its output is the
// scattered seed itself: G[c][idx[m]][k] = seeds[m][c][k] for first occurrences (planes pre-zeroed).
__global__ void scatter_seed_planes_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int64_t C,
                                           const int32_t* __restrict__ pos, const float* __restrict__ seeds,
                                           float* __restrict__ g, int64_t cb, int64_t ce) {
  const int64_t m = blockIdx.x;
  const int64_t n = idx[m];
  if (n < 0 || n >= N || pos[n] != m) return;
  const int64_t CC = C * C;
  for (int64_t q = cb * C + threadIdx.x; q < ce * C; q += blockDim.x) {
    const int64_t c = q / C, k = q - c * C;
    g[(c * N + n) * C + k] = seeds[m * CC + q];
  }
}

}  // namespace

int mark_rows(lgnn_ctx* h, const int64_t* idx, int64_t M, int which, DevBuf& flags, hipStream_t s) {
  const int64_t N = h->N;
  LGNN_CALL(flags.reserve(size_t(N)));
  LGNN_HIP_CHECK(hipMemsetAsync(flags.p, 0, size_t(N), s));
  if (which & kRowsNeighbours) {
    hipLaunchKernelGGL(mark_active_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, h->P.rowptr, h->P.col,
                       flags.as<uint8_t>());
    LGNN_HIP_CHECK(hipGetLastError());
  }
  if (which & kRowsBatch) {
    hipLaunchKernelGGL(mark_batch_flags_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, N, flags.as<uint8_t>());
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

int build_row_list(lgnn_ctx* h, const int64_t* idx, int64_t M, int which, DevBuf& flags, DevBuf& list, DevBuf& count,
                   hipStream_t s, ActiveRows* out) {
  LGNN_CALL(mark_rows(h, idx, M, which, flags, s));
  LGNN_CALL(compact_rows(h, flags.as<uint8_t>(), list, count, s));
  if (out) *out = ActiveRows{flags.as<uint8_t>(), list.as<int32_t>(), count.as<int32_t>()};
  return 0;
}

int launch_seed_spmm_gram(lgnn_ctx* h, bool fork_exact, float* g, int64_t cb, int64_t ce, float* scratch, const ActiveRows& rows,
                          hipStream_t s) {
  switch (int(cdiv(h->dims[h->L], 16))) {
    case 1: return seed_spmm_gram_launch<1>(h, fork_exact, g, cb, ce, scratch, s, rows);
    case 2: return seed_spmm_gram_launch<2>(h, fork_exact, g, cb, ce, scratch, s, rows);
    case 3: return seed_spmm_gram_launch<3>(h, fork_exact, g, cb, ce, scratch, s, rows);
    default: return seed_spmm_gram_launch<4>(h, fork_exact, g, cb, ce, scratch, s, rows);
  }
}

int launch_seed_spmm(lgnn_ctx* h, float* g, int64_t cb, int64_t ce, hipStream_t s) {
  const int64_t N = h->N, C = h->dims[h->L], nq = (ce - cb) * C;
  int waves = int(std::max<int64_t>(1, std::min<int64_t>(4, (48 * 1024) / (nq * 4))));
  LGNN_REQUIRE(nq * 4 <= 60 * 1024, "too many classes for the seed SpMM kernel (use class ranges)");
  hipLaunchKernelGGL(seed_spmm_kernel, dim3(unsigned(cdiv(N, waves))), dim3(64 * waves), size_t(waves) * nq * 4, s,
                     h->PT.rowptr, h->PT.col, h->PT.val, N, C, h->ws.pos.as<int32_t>(), h->ws.seeds.as<float>(),
                     g, h->ws.active.as<uint8_t>(), cb, ce);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_scatter_seed_planes(lgnn_ctx* h, const int64_t* idx, int64_t M, float* g, int64_t cb, int64_t ce, hipStream_t s) {
  hipLaunchKernelGGL(scatter_seed_planes_kernel, dim3(unsigned(M)), dim3(256), 0, s, idx, M, h->N, h->dims[h->L],
                     h->ws.pos.as<int32_t>(), h->ws.seeds.as<float>(), g, cb, ce);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// The GCN top layer of one batch for a caller outside the accumulate (adjgrad_gcn.hip): active rows (flags in ws.active, list in
// ws.act_list / ws.act_count) and the class-major planes g[c][n][:] of ALL C classes for those rows -- rows that are not
// active are NOT written.  Needs batch_prologue's probabilities / multiplicities; the Gram it also forms goes to a scratch.
int kfac_top_planes(lgnn_ctx* h, const int64_t* idx, int64_t M, bool fork_exact, float* g, hipStream_t s) {
  const int64_t C = h->dims[h->L];
  LGNN_REQUIRE(h->kind == LGNN_KIND_GCN, "internal: top-layer planes are a GCN step");
  ActiveRows rows{};
  LGNN_CALL(build_row_list(h, idx, M, kRowsNeighbours, h->ws.active, h->ws.act_list, h->ws.act_count, s, &rows));
  DevBuf& sc = h->ws.gram_scratch[h->L - 1];
  LGNN_CALL(sc.reserve(size_t(C) * C * 4));
  LGNN_HIP_CHECK(hipMemsetAsync(sc.p, 0, size_t(C) * C * 4, s));
  return launch_seed_spmm_gram(h, fork_exact, g, 0, C, sc.as<float>(), rows, s);
}

}  // namespace lgnn
