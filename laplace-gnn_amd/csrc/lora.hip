// All-pairs adjacency gradient and the LoRA structure-learning kernels (LoRASTEGCN, gnn/models/models.py:186-235).
//
// LoRASTEGCN parameterises the whole adjacency (gnn/models/models.py:226-232):
//     M = adj0 + scaling * (B @ A)        A = adj_lora_A [r, N], B = adj_lora_B [N, r], scaling = lora_alpha / r
//     M = (M + M^T) / 2                   (symmetric models)
//     A_hat = fill_diagonal_(BinarizeSTE(M, threshold), 1);   P = normalize_adj(A_hat)
// so any pair can cross the threshold, and what ``neg_marglik.backward()`` leaves in A and B (gnn/marglik_training.py:197-216)
// needs d(-marglik)/dA_hat on ALL N^2 pairs:  grad_A = scaling B^T G,  grad_B = scaling G A^T.
//
// Three pieces live here:
//  * the dense-grid terms of the adjacency gradient (adjgrad_gcn.hip's / adjgrad_diag.hip's chains with a dense [N, N] target instead of the stored
//    entries and a candidate list): every per-pair term <U[a], V[b]> summed over planes becomes a tile GEMM on the fp32
//    matrix cores (dense_nt_kernel, v_mfma_f32_32x32x2_f32; rows restricted to a device list where the term lives on a few
//    rows only -- the active rows of a batch, the batch rows of the seed term), the diagonal posterior's per-sample term
//    sum_j mask[b, j] <Tbar_n[j, :], Ee[b, :]> is a per-sample GEMM with the mask contraction in its epilogue
//    (dense_diag_pair_kernel), and normalize_adj backward + symmetrisation + zero diagonal run in place as one pass over
//    pairs of transposed tiles (dense_adj_finish_kernel);
//  * lgnn_lora_threshold: re-binarise adj0 + scaling B A against the engine's stored pattern, compacted flips on the device;
//  * lgnn_lora_grad: grad_A / grad_B from the dense G in one pass over row tiles of G.
#include "device_utils.h"
#include "mfma_tile.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// ---- C[orow(t), b] += sum_c sum_k L_c[lrow(t), k] R_c[b, k]  (+ rowc[orow]) ------------------------------------------------
// 64 x 64 output tile per workgroup, four waves of 32 x 32 (mfma_tile.h); K staged through LDS 16 wide (rows padded to 17
// floats).
// Every output row of a launch belongs to one list entry: one writer per element, no atomics.
constexpr int DT = 64, DKC = 16, DLD = DKC + 1;

__global__ __launch_bounds__(256) void dense_nt_kernel(DenseNtArgs g) {
  __shared__ float Ls[DT * DLD], Rs[DT * DLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t total = g.nrows_dev ? int64_t(*g.nrows_dev) : g.nrows;
  const int64_t t0 = int64_t(blockIdx.y) * DT, b0 = int64_t(blockIdx.x) * DT;
  if (t0 >= total) return;
  // staging: thread <-> (row tid / 4, 4 consecutive k)
  const int srow = tid >> 2, sk = (tid & 3) * 4;
  const int64_t st = t0 + srow;
  const bool l_ok = st < total;
  int64_t lrow = 0;
  if (l_ok) {
    const int64_t orow = g.orows ? int64_t(g.orows[st]) : st;
    lrow = g.lrows ? int64_t(g.lrows[st]) : orow;
  }
  const int64_t sb = b0 + srow;
  const bool r_ok = sb < g.ncols;
  f32x16 acc;
  acc_zero(acc);
  for (int64_t c = 0; c < g.nplanes; ++c) {
    const float* __restrict__ lp = g.L + c * g.l_stride + lrow * g.l_ld;
    const float* __restrict__ rp = g.R + c * g.r_stride + sb * g.r_ld;
    for (int64_t k0 = 0; k0 < g.width; k0 += DKC) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t k = k0 + sk + e;
        const bool kin = k < g.width;
        Ls[srow * DLD + sk + e] = (l_ok && kin) ? lp[k] : 0.f;
        Rs[srow * DLD + sk + e] = (r_ok && kin) ? rp[k] : 0.f;
      }
      __syncthreads();
      tile_nt_step<DKC, DLD>(Ls, wr * 32, Rs, wc * 32, lane, acc);
    }
  }
  const int64_t b = b0 + wc * 32 + (lane & 31);
  if (b >= g.ncols) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t t = acc_row(t0 + wr * 32, lane, r);
    if (t >= total) continue;
    const int64_t orow = g.orows ? int64_t(g.orows[t]) : t;
    float v = acc[r];
    if (g.rowc) v += g.rowc[orow * g.rowc_ld];
    g.out[orow * g.ldo + b] += v;
  }
}

// ---- diagonal posterior, one sample n = idx[m] (first occurrence, times its multiplicity) x 64 columns b:
//   out[n - row0, b] += mult * ( sum_j mask[b, j] sum_i Tbar[j, i] Ee[b, i] + <phibar[:H], H1[b]> + phibar[H] )
// out holds the rows [row0, row1) of the grid (the whole grid, or a row band of it: adjband.hip); samples outside are skipped.
// Tbar [H][FP] (zero padded beyond F + 1), Ee[b] = [P X | rowsum(P)][b].  64 x 64 tiles (rows j, columns b) on the fp32 MFMA,
// K = i staged through LDS; the mask contraction is the epilogue of each j tile and stays in registers (lane: one b).
__global__ __launch_bounds__(256) void dense_diag_pair_kernel(const int64_t* __restrict__ idx, int64_t m0, int64_t N,
                                                              const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                              const float* __restrict__ mask, int64_t H,
                                                              const float* __restrict__ PX, int64_t ldx,
                                                              const float* __restrict__ rowsum, int64_t F,
                                                              const float* __restrict__ H1p, int64_t ldh,
                                                              const float* __restrict__ T, const float* __restrict__ phibar,
                                                              int64_t row0, int64_t row1, float* __restrict__ out) {
  __shared__ float Ts[DT * DLD], Es[DT * DLD];
  __shared__ float red[2][DT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t m = m0 + blockIdx.y;
  const int64_t n = idx[m];
  if (n < row0 || n >= row1 || pos[n] != int32_t(m)) return;  // (uniform) duplicates: the first occurrence carries the multiplicity
  const int64_t F1 = F + 1, FP = (F1 + 3) & ~int64_t(3);
  const float* __restrict__ Tm = T + int64_t(blockIdx.y) * H * FP;
  const float* __restrict__ pbm = phibar + int64_t(blockIdx.y) * (H + 1);
  const int64_t b0 = int64_t(blockIdx.x) * DT;
  const int srow = tid >> 2, sk = (tid & 3) * 4;
  const int64_t sb = b0 + srow;
  const bool b_ok = sb < N;
  const int64_t bl = b0 + wc * 32 + (lane & 31);  // this lane's column
  float part = 0.f;
  for (int64_t j0 = 0; j0 < H; j0 += DT) {
    const int64_t sj = j0 + srow;
    const bool j_ok = sj < H;
    f32x16 acc;
    acc_zero(acc);
    for (int64_t i0 = 0; i0 < F1; i0 += DKC) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + sk + e;
        Ts[srow * DLD + sk + e] = (j_ok && i < F1) ? Tm[sj * FP + i] : 0.f;
        Es[srow * DLD + sk + e] = !b_ok ? 0.f : (i < F ? PX[sb * ldx + i] : (i == F ? rowsum[sb] : 0.f));
      }
      __syncthreads();
      tile_nt_step<DKC, DLD>(Ts, wr * 32, Es, wc * 32, lane, acc);
    }
    if (bl < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = acc_row(j0 + wr * 32, lane, r);
        if (j < H) part = fmaf(acc[r], mask[bl * H + j], part);
      }
    }
  }
  part += __shfl_xor(part, 32);
  if (lane < 32) red[wr][wc * 32 + lane] = part;
  __syncthreads();
  if (tid < DT) {
    const int64_t b = b0 + tid;
    if (b < N) {
      float dot = 0.f;
      for (int64_t j = 0; j < H; ++j) dot = fmaf(pbm[j], H1p[b * ldh + j], dot);
      const float v = red[0][tid] + red[1][tid] + dot + pbm[H];
      out[(n - row0) * N + b] += float(mult[m]) * v;
    }
  }
}

// ---- normalize_adj backward on the dense grid, in place: G[a, b] = d/dP[a, b] -> d/dA[i, j] ----------------------------------
//   gA[i, j] = G[j, i] d_i d_j + rt_i,   rt_i = -1/2 d_i^2 (rs_i + cs_i),   d = rowsum(A_hat)^-1/2  (P = D A_hat^T D)
//   symmetric models: (gA[i, j] + gA[j, i]) / 2;  diagonal 0 (overwritten by fill_diagonal_(1)).
// One workgroup per pair of transposed 32 x 32 tiles (I <= J): both are read into LDS before either is written.
__global__ __launch_bounds__(256) void dense_adj_finish_kernel(float* __restrict__ G, int64_t N, const int32_t* __restrict__ a_rowptr,
                                                               const float* __restrict__ rs, const float* __restrict__ cs, int sym) {
  __shared__ float Ga[32][33], Gb[32][33];
  const int64_t I = blockIdx.y, J = blockIdx.x;
  if (I > J) return;
  const int tid = threadIdx.x;
  for (int e = tid; e < 1024; e += 256) {
    const int r = e >> 5, c = e & 31;
    const int64_t i = I * 32 + r, j = J * 32 + c;
    Ga[r][c] = (i < N && j < N) ? G[i * N + j] : 0.f;
    const int64_t i2 = J * 32 + r, j2 = I * 32 + c;
    Gb[r][c] = (i2 < N && j2 < N) ? G[i2 * N + j2] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const int r = e >> 5, c = e & 31;
    // tile (I, J): i = I*32 + r, j = J*32 + c;  G[j, i] = Gb[c][r], G[i, j] = Ga[r][c]
    {
      const int64_t i = I * 32 + r, j = J * 32 + c;
      if (i < N && j < N) {
        float v = 0.f;
        if (i != j) {
          const float di = rsqrtf(float(a_rowptr[i + 1] - a_rowptr[i])), dj = rsqrtf(float(a_rowptr[j + 1] - a_rowptr[j]));
          const float dd = di * dj;  // (one product for both orientations: a symmetric model's result is bit symmetric)
          const float rti = -0.5f * di * di * (rs[i] + cs[i]);
          const float gij = fmaf(Gb[c][r], dd, rti);  // (explicit fmas: the same rounding in both orientations)
          if (sym) {
            const float rtj = -0.5f * dj * dj * (rs[j] + cs[j]);
            v = 0.5f * (gij + fmaf(Ga[r][c], dd, rtj));
          } else {
            v = gij;
          }
        }
        G[i * N + j] = v;
      }
    }
    if (I != J) {  // tile (J, I): i = J*32 + r, j = I*32 + c;  G[j, i] = Ga[c][r], G[i, j] = Gb[r][c]
      const int64_t i = J * 32 + r, j = I * 32 + c;
      if (i < N && j < N) {
        const float di = rsqrtf(float(a_rowptr[i + 1] - a_rowptr[i])), dj = rsqrtf(float(a_rowptr[j + 1] - a_rowptr[j]));
        const float dd = di * dj;
        const float rti = -0.5f * di * di * (rs[i] + cs[i]);
        const float gij = fmaf(Ga[c][r], dd, rti);
        float v = gij;
        if (sym) {
          const float rtj = -0.5f * dj * dj * (rs[j] + cs[j]);
          v = 0.5f * (gij + fmaf(Gb[r][c], dd, rtj));
        }
        G[i * N + j] = v;
      }
    }
  }
}

// stored entries of P gathered from the dense G: gP[p] = G[a, col[p]]
__global__ void gather_stored_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                     const float* __restrict__ G, float* __restrict__ gP) {
  const int lane = threadIdx.x & 63;
  const int64_t a = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (a >= N) return;
  for (int32_t p = rowptr[a] + lane; p < rowptr[a + 1]; p += 64) gP[p] = G[a * N + col[p]];
}

// ---- LoRA ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool csr_has(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t i,
                                        int32_t j) {
  int32_t s = rowptr[i], e = rowptr[i + 1];
  while (s < e) {  // sorted columns inside a row
    const int32_t mid = (s + e) >> 1;
    if (col[mid] < j) s = mid + 1;
    else e = mid;
  }
  return s < rowptr[i + 1] && col[s] == j;
}

// m_ij = adj0_ij + (sum_k B[i, k] A[k, j]) * scaling  (the reference's order: B @ A, times scaling, plus adj)
__device__ __forceinline__ float lora_value(const int32_t* __restrict__ b_rowptr, const int32_t* __restrict__ b_col,
                                            const float* __restrict__ A, const float* __restrict__ B, int64_t r, int64_t N,
                                            float scaling, int64_t i, int64_t j) {
  float t = 0.f;
  for (int64_t k = 0; k < r; ++k) t = fmaf(B[i * r + k], A[k * N + j], t);
  const float base = csr_has(b_rowptr, b_col, i, int32_t(j)) ? 1.f : 0.f;
  return base + t * scaling;
}

// One thread per off-diagonal pair (i, j): want = value > threshold, have = the engine stores (i, j).  Flips are compacted per
// wave: a 64-bit ballot, one atomic on the counter, each flipping lane writes at base + its rank among the set bits below it.
// Entries past `cap` are counted but not written (the host grows the buffers and runs again).
__global__ __launch_bounds__(256) void lora_threshold_kernel(const int32_t* __restrict__ b_rowptr, const int32_t* __restrict__ b_col,
                                                             const int32_t* __restrict__ s_rowptr, const int32_t* __restrict__ s_col,
                                                             const float* __restrict__ A, const float* __restrict__ B, int64_t r,
                                                             int64_t N, float scaling, float threshold, int sym,
                                                             unsigned long long* __restrict__ counter, int64_t cap,
                                                             int64_t* __restrict__ fr, int64_t* __restrict__ fc,
                                                             uint8_t* __restrict__ fs) {
  const int lane = threadIdx.x & 63;
  const int64_t i = blockIdx.y;
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool flip = false, want = false;
  if (j < N && j != i) {
    float v = lora_value(b_rowptr, b_col, A, B, r, N, scaling, i, j);
    if (sym) v = 0.5f * (v + lora_value(b_rowptr, b_col, A, B, r, N, scaling, j, i));
    want = v > threshold;
    flip = want != csr_has(s_rowptr, s_col, i, int32_t(j));
  }
  const unsigned long long bal = __ballot(flip);
  if (bal == 0ull) return;
  unsigned long long base = 0ull;
  if (lane == __ffsll(static_cast<long long>(bal)) - 1) base = atomicAdd(counter, static_cast<unsigned long long>(__popcll(bal)));
  base = __shfl(base, __ffsll(static_cast<long long>(bal)) - 1);
  if (flip) {
    const unsigned long long below = lane ? (bal & ((~0ull) >> (64 - lane))) : 0ull;
    const int64_t o = int64_t(base) + __popcll(below);
    if (o < cap) { fr[o] = i; fc[o] = j; fs[o] = want ? 1 : 0; }
  }
}

// One pass over row tiles of G (64 rows per workgroup, 64 x 64 sub-tiles of G staged in LDS, left to right):
//   gB[i, k]         = scaling * sum_j G[i, j] A[k, j]      (complete inside the workgroup: it owns the rows)
//   part[t][k, j]    = sum_{i in tile t} B[i, k] G[i, j]    (the partial of grad_A; lora_grad_reduce sums t in order)
// Thread <-> (column / row tid & 63 of the sub-tile, k = (tid >> 6) + 4 q): 16 accumulators of each kind, LDS reads either
// conflict free (stride 65) or broadcast.
constexpr int LRT = 64, LCT = 64, LMAXR = 64;
__global__ __launch_bounds__(256) void lora_grad_kernel(const float* __restrict__ G, const float* __restrict__ A,
                                                        const float* __restrict__ B, int64_t r, int64_t N, float scaling,
                                                        float* __restrict__ gB, float* __restrict__ part) {
  __shared__ float Gs[LRT][LCT + 1];
  __shared__ float Bs[LRT][LMAXR + 1];
  __shared__ float As[LMAXR][LCT + 1];
  const int tid = threadIdx.x, l64 = tid & 63, kq = tid >> 6;
  const int64_t i0 = int64_t(blockIdx.x) * LRT;
  for (int e = tid; e < LRT * LMAXR; e += 256) {
    const int il = e / LMAXR, k = e % LMAXR;
    Bs[il][k] = (k < r && i0 + il < N) ? B[(i0 + il) * r + k] : 0.f;
  }
  float accB[LMAXR / 4];
#pragma unroll
  for (int q = 0; q < LMAXR / 4; ++q) accB[q] = 0.f;
  for (int64_t c0 = 0; c0 < N; c0 += LCT) {
    __syncthreads();
    for (int e = tid; e < LMAXR * LCT; e += 256) {
      const int k = e / LCT, jl = e % LCT;
      As[k][jl] = (k < r && c0 + jl < N) ? A[int64_t(k) * N + c0 + jl] : 0.f;
    }
    for (int e = tid; e < LRT * LCT; e += 256) {
      const int il = e / LCT, jl = e % LCT;
      const int64_t i = i0 + il, j = c0 + jl;
      Gs[il][jl] = (i < N && j < N) ? G[i * N + j] : 0.f;
    }
    __syncthreads();
    float accA[LMAXR / 4];
#pragma unroll
    for (int q = 0; q < LMAXR / 4; ++q) accA[q] = 0.f;
    for (int il = 0; il < LRT; ++il) {  // grad_A partial: column l64
      const float g = Gs[il][l64];
#pragma unroll
      for (int q = 0; q < LMAXR / 4; ++q) accA[q] = fmaf(Bs[il][kq + 4 * q], g, accA[q]);
    }
    for (int jl = 0; jl < LCT; ++jl) {  // grad_B: row l64
      const float g = Gs[l64][jl];
#pragma unroll
      for (int q = 0; q < LMAXR / 4; ++q) accB[q] = fmaf(g, As[kq + 4 * q][jl], accB[q]);
    }
    if (c0 + l64 < N) {
#pragma unroll
      for (int q = 0; q < LMAXR / 4; ++q) {
        const int k = kq + 4 * q;
        if (k < r) part[(int64_t(blockIdx.x) * r + k) * N + c0 + l64] = accA[q];
      }
    }
  }
  const int64_t i = i0 + l64;
  if (i < N)
#pragma unroll
    for (int q = 0; q < LMAXR / 4; ++q) {
      const int k = kq + 4 * q;
      if (k < r) gB[i * r + k] = scaling * accB[q];
    }
}

__global__ void lora_grad_reduce_kernel(const float* __restrict__ part, int64_t tiles, int64_t rN, float scaling,
                                        float* __restrict__ gA) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < rN; e += stride) {
    float s = 0.f;
    for (int64_t t = 0; t < tiles; ++t) s += part[t * rN + e];  // fixed order: deterministic
    gA[e] = scaling * s;
  }
}

}  // namespace

int launch_dense_nt(const DenseNtArgs& g, hipStream_t s) {
  if (g.nrows <= 0 || g.ncols <= 0 || g.width <= 0 || g.nplanes <= 0) return 0;
  LGNN_REQUIRE(g.out && g.L && g.R, "dense grid term: null pointers");
  LGNN_REQUIRE(cdiv(g.nrows, DT) < 65536, "dense grid term: too many rows");
  const dim3 grid{unsigned(cdiv(g.ncols, DT)), unsigned(cdiv(g.nrows, DT)), 1};
  hipLaunchKernelGGL(dense_nt_kernel, grid, dim3(256), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_dense_diag_pair(const int64_t* idx, int64_t m0, int64_t mc, int64_t N, const int32_t* pos, const int32_t* mult,
                           const float* mask, int64_t H, const float* PX, int64_t ldx, const float* rowsum, int64_t F,
                           const float* H1p, int64_t ldh, const float* T, const float* phibar, int64_t row0, int64_t row1,
                           float* out, hipStream_t s) {
  if (mc <= 0) return 0;
  LGNN_REQUIRE(mc < 65536, "dense grid term: too many samples in a chunk");
  LGNN_REQUIRE(row0 >= 0 && row0 <= row1 && row1 <= N, "dense grid term: rows outside the grid");
  hipLaunchKernelGGL(dense_diag_pair_kernel, dim3(unsigned(cdiv(N, DT)), unsigned(mc)), dim3(256), 0, s, idx, m0, N, pos, mult,
                     mask, H, PX, ldx, rowsum, F, H1p, ldh, T, phibar, row0, row1, out);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int dense_adj_finish(lgnn_ctx* h, float* G, hipStream_t s) {
  const int64_t N = h->N;
  LGNN_CALL(h->ws.misc.reserve(size_t(2) * N * 4 + size_t(std::max<int64_t>(h->nnz, 1)) * 4));
  float* rs = h->ws.misc.as<float>();
  float* cs = rs + N;
  float* gP = cs + N;
  hipLaunchKernelGGL(gather_stored_kernel, dim3(unsigned(cdiv(N * 64, 256))), dim3(256), 0, s, h->P.rowptr, h->P.col, N, G, gP);
  LGNN_HIP_CHECK(hipGetLastError());
  LGNN_HIP_CHECK(hipMemsetAsync(cs, 0, size_t(N) * 4, s));
  LGNN_CALL(launch_gp_rowcol(h, gP, rs, cs, s));
  const unsigned nt = unsigned(cdiv(N, 32));
  hipLaunchKernelGGL(dense_adj_finish_kernel, dim3(nt, nt), dim3(256), 0, s, G, N, h->A.rowptr, rs, cs, h->sym ? 1 : 0);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn

using namespace lgnn;

extern "C" int lgnn_lora_threshold(lgnn_ctx* h, const int32_t* base_rowptr, const int32_t* base_col, const float* lora_A,
                                   const float* lora_B, int64_t r, float scaling, float threshold, int symmetric,
                                   int64_t* num_flips, void* stream) {
  if (!h || !num_flips) { set_error("null argument"); return 2; }
  LGNN_REQUIRE(base_rowptr && base_col && lora_A && lora_B, "lgnn_lora_threshold: null pointers");
  LGNN_REQUIRE(r >= 1, "lgnn_lora_threshold: rank must be >= 1");
  const int64_t N = h->N;
  LGNN_REQUIRE(N >= 1 && N < 65536, "lgnn_lora_threshold: graph too large (one grid row per node)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DevBuf& cnt = h->ws.lora_count;
  LGNN_CALL(cnt.reserve(64));
  auto run = [&](int64_t cap) -> int {
    LGNN_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8, s));
    const dim3 grid{unsigned(cdiv(N, 256)), unsigned(N), 1};
    hipLaunchKernelGGL(lora_threshold_kernel, grid, dim3(256), 0, s, base_rowptr, base_col, h->A.rowptr, h->A.col, lora_A, lora_B,
                       r, N, scaling, threshold, symmetric ? 1 : 0, cnt.as<unsigned long long>(), cap,
                       h->ws.lora_rows.as<int64_t>(), h->ws.lora_cols.as<int64_t>(), h->ws.lora_state.as<uint8_t>());
    LGNN_HIP_CHECK(hipGetLastError());
    return 0;
  };
  int64_t cap = std::max<int64_t>(int64_t(h->ws.lora_state.bytes), 2 * h->nnz + 4096);
  auto grow = [&](int64_t c) -> int {
    LGNN_CALL(h->ws.lora_rows.reserve(size_t(c) * 8));
    LGNN_CALL(h->ws.lora_cols.reserve(size_t(c) * 8));
    LGNN_CALL(h->ws.lora_state.reserve(size_t(c)));
    return 0;
  };
  LGNN_CALL(grow(cap));
  LGNN_CALL(run(cap));
  unsigned long long n = 0;
  LGNN_HIP_CHECK(hipMemcpyAsync(&n, cnt.p, 8, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));
  if (int64_t(n) > cap) {  // more flips than the buffers hold: grow to the exact count and run again
    cap = int64_t(n);
    LGNN_CALL(grow(cap));
    LGNN_CALL(run(cap));
  }
  *num_flips = int64_t(n);
  if (n == 0) return 0;
  return graph_update(h, h->ws.lora_rows.as<int64_t>(), h->ws.lora_cols.as<int64_t>(), h->ws.lora_state.as<uint8_t>(),
                      int64_t(n), s);
}

extern "C" int lgnn_lora_grad(lgnn_ctx* h, const float* grad_adj_dense, const float* lora_A, const float* lora_B, int64_t r,
                              float scaling, float* grad_A, float* grad_B, void* stream) {
  if (!h) { set_error("null context"); return 2; }
  LGNN_REQUIRE(grad_adj_dense && lora_A && lora_B && grad_A && grad_B, "lgnn_lora_grad: null pointers");
  LGNN_REQUIRE(r >= 1 && r <= LMAXR, "lgnn_lora_grad: rank must be in [1, 64]");
  const int64_t N = h->N;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t tiles = cdiv(N, LRT);
  LGNN_REQUIRE(tiles * r * N * 4 <= h->ws_limit, "lgnn_lora_grad: the grad_A partials (r N^2 / 16 bytes) exceed the workspace limit");
  LGNN_CALL(h->ws.lora_part.reserve(size_t(tiles) * r * N * 4));
  hipLaunchKernelGGL(lora_grad_kernel, dim3(unsigned(tiles)), dim3(256), 0, s, grad_adj_dense, lora_A, lora_B, r, N, scaling,
                     grad_B, h->ws.lora_part.as<float>());
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3(unsigned(std::min<int64_t>(cdiv(r * N, 256), 4096))), dim3(256), 0, s,
                     h->ws.lora_part.as<float>(), tiles, r * N, scaling, grad_A);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}
