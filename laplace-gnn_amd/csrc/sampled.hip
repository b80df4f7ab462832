// lgnn_sampled_forward: the logits of S parameter samples at a batch of evaluation nodes in one pass.
//
// What it replaces: the sampling predictive's loop (laplace/baselaplace.py:1160-1199, reached from mc_eval,
// gnn/marglik_training.py:341-353): per sample, vector_to_parameters + one forward over all N nodes.  Here the weights of
// the bound model are never written.  With U = P X, rho = rowsum(P) and in0 = [U | rho] (GCN) or [X | U | 1] (GraphSAGE) --
// the last column is what the bias is multiplied with --
//   GCN        h_s[r] = act(in0[r] [W0_s | b0_s]^T)         z_s[r] = h_s[r] W1_s^T                  (C floats)
//              f_s[m] = sum_b P[idx_m, b] (z_s[b] + b1_s)
//   GraphSAGE  h_s[r] as above                              z_s[r] = [W1a_s h_s[r] | W1b_s h_s[r]]  (2 C floats, W1 = [W1a | W1b])
//              f_s[m] = z_s[idx_m][:C] + sum_b P[idx_m, b] z_s[b][C:] + b1_s
//   1 layer    f_s[m] = in0[idx_m] [W_s | b_s]^T
// Three steps per call, no host round trip:
//   (a) the needed rows R (the columns of P's rows idx; GraphSAGE: and idx) as flags -> sorted list (compact_flags) -> positions;
//   (b) first_layer_kernel: a 64-row tile of R x one sample per workgroup pass.  The first product runs on
//       v_mfma_f32_32x32x2_f32 (lane layout and tile step: mfma_tile.h; K staged through LDS 64 wide, the next stage in
//       registers while the current one is multiplied; the B operand read from theta as stored: K contiguous, scalar loads --
//       rows of theta are not 16-byte aligned in general); the hidden width is walked in tiles of 64; bias (times the row's
//       bias column) and activation in registers, the tile goes to LDS and meets W1_s's 64 columns on the same MFMA while it
//       is there.  Only z reaches memory; h_s never does;
//   (c) sampled_gather_kernel: the CSR gather over the rows idx with the bias (one wave per (sample, node), a fixed order),
//       then the optional softmax.
// No float atomics: every output element has one writer and one summation order, which does not depend on the chunk the
// sample runs in.  The samples go in chunks sized so that z stays under the workspace limit.
#include "device_utils.h"
#include "mfma_tile.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// in0[r, col] = rowsum(P)[r] (GCN) or 1 (GraphSAGE): the column the bias is multiplied with
__global__ void sampled_bias_column_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ val, int64_t N,
                                           int gcn, float* __restrict__ in0, int64_t ldk, int64_t col) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= N) return;
  float acc = 1.f;
  if (gcn) {
    acc = 0.f;
    for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) acc += val[p];
  }
  in0[r * ldk + col] = acc;
}

// (a) flags of the rows the evaluation nodes read: one wave per batch row
__global__ __launch_bounds__(256) void sampled_mark_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                           const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, int self,
                                                           uint8_t* __restrict__ need, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t m = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n < 0 || n >= N) {
    if (lane == 0) *bad = 1;
    return;
  }
  if (self && lane == 0) need[n] = 1;
  for (int32_t p = rowptr[n] + lane; p < rowptr[n + 1]; p += 64) need[col[p]] = 1;
}

__global__ void sampled_positions_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ count, int64_t cap,
                                         int32_t* __restrict__ rpos) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r < cap && r < int64_t(*count)) rpos[rows[r]] = int32_t(r);
}

// 1 layer: R is the batch itself (a repeated id is a row of its own), -1 where the id is invalid
__global__ void sampled_batch_rows_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int32_t* __restrict__ rows,
                                          int32_t* __restrict__ count, int* __restrict__ bad) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m == 0) *count = int32_t(M);
  if (m >= M) return;
  const int64_t n = idx[m];
  const bool ok = n >= 0 && n < N;
  if (!ok) *bad = 1;
  rows[m] = ok ? int32_t(n) : -1;
}

struct HiddenArgs {
  static constexpr bool linearised = false;
  static constexpr bool hessian = false;
  const float* in0; int64_t ldk;
  const int32_t* rows; const int32_t* count;
  const float* theta; int64_t P;   // the chunk's first sample, floats between samples
  int64_t Fp, H;                   // columns of the first Linear's weight, its rows (1 layer: the classes)
  int64_t off1, ld1, C, Cz;        // W1_s at theta_s + off1 with row stride ld1; z has Cz = C (GCN) or 2 C (GraphSAGE) columns
  float* z; int64_t rcap;          // z[(s * rcap + r) * Cz + c]   (1 layer: the output, [(s * rcap + m) * H + c])
  int act;
};

// (b).  grid: (workers over the row tiles, samples of the chunk, windows of SZW columns of z).  Two argument structs, one
// text: HiddenArgs writes act(.) into the hidden tile and multiplies it with the sample's own W1_s; FwdArgs (the GGN's
// forward product, ggnmat.hip) writes D . (.) instead, multiplies it with the bound W1, and then runs h dW1^T over the same
// accumulators.  HessArgs (the exact Hessian's residual product, hessmat.hip) keeps the first product in its accumulators, runs
// G dW1 for the same 64 x 64 tile on a second one, and writes E and T from registers: no hidden tile, no z.
// (The HessArgs instance asks for two waves per SIMD, the forward instances' occupancy: left alone it takes 251 + 16 registers.)
template <class Args, bool ONE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Args::hessian ? 2 : 1))) void first_layer_kernel(Args g) {
  constexpr bool LIN = Args::linearised;
  constexpr bool HESS = Args::hessian;
  static_assert(!(HESS && ONE), "one-layer models have no second derivative");
  // As / Bs (the first product's K stage) and Ws (W1's tile) are never live at the same time: one region
  __shared__ float stage[SZW * SLDH];
  __shared__ float Hs[SBM * SLDH];
  __shared__ float bcol[SBM];
  __shared__ int rid[(LIN || HESS) && !ONE ? SBM : 1];  // LIN / HESS: the tile rows' node ids, for D and h
  float* As = stage;
  float* Bs = stage + SBM * SLDT;
  float* Ws = stage;
  static_assert(SZW * SLDH >= (SBM + SBH) * SLDT, "the K stage fits the region of the W1 tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31;
  const int64_t cnt = int64_t(*g.count);
  const float* __restrict__ th = g.theta + int64_t(blockIdx.y) * g.P;
  const int64_t zw0 = int64_t(blockIdx.z) * SZW;
  const int zrows = ONE ? 0 : int(g.Cz - zw0 < SZW ? g.Cz - zw0 : SZW);  // columns of z this workgroup owns
  const int srow = tid >> 2, sk = (tid & 3) * 16;  // A staging: thread <-> (row, 16 consecutive k)
  const int bj = tid >> 6, bk = tid & 63;          // B staging: thread <-> (rows bj + 4 e, one k)
  for (int64_t tile = blockIdx.x; tile * SBM < cnt; tile += gridDim.x) {
    const int64_t t0 = tile * SBM;
    int64_t arow = -1;
    if (t0 + srow < cnt) arow = g.rows[t0 + srow];
    const float* __restrict__ ap = g.in0 + (arow < 0 ? 0 : arow) * g.ldk;
    __syncthreads();  // the previous tile's last reads of bcol / rid / the LDS tiles
    // what the bias is multiplied with: rowsum(P) (GCN) or 1 (GraphSAGE); 0 for padding rows and invalid ids (a zero row)
    if ((tid & 3) == 0) {
      bcol[srow] = arow < 0 ? 0.f : ap[g.Fp];
      if constexpr ((LIN || HESS) && !ONE) rid[srow] = int(arow);
    }
    f32x16 zacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) acc_zero(zacc[i]);
    for (int64_t j0 = 0; j0 < g.H; j0 += SBH) {
      f32x16 acc;
      acc_zero(acc);
      // the next K stage travels in registers while the matrix cores work on the current one
      float4 pa[4];
      float pb[16];
      auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t k = k0 + sk + 4 * e;
          pa[e] = make_float4(0.f, 0.f, 0.f, 0.f);
          // (ldk % 4 == 0; the columns from Fp on meet zeros of the B stage)
          if (arow >= 0 && k < g.ldk) pa[e] = *reinterpret_cast<const float4*>(ap + k);
        }
        const int64_t k = k0 + bk;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t j = j0 + bj + 4 * e;
          pb[e] = (j < g.H && k < g.Fp) ? th[j * g.Fp + k] : 0.f;
        }
      };
      fetch(0);
      for (int64_t k0 = 0; k0 < g.Fp; k0 += SBK) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float* d = As + srow * SLDT + sk + 4 * e;
          d[0] = pa[e].x; d[1] = pa[e].y; d[2] = pa[e].z; d[3] = pa[e].w;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) Bs[(bj + 4 * e) * SLDT + bk] = pb[e];
        __syncthreads();
        if (k0 + SBK < g.Fp) fetch(k0 + SBK);
        tile_nt_step<SBK, SLDT>(As, wr * 32, Bs, wc * 32, lane, acc);
      }
      // bias in registers: this lane's column of the tile, the rows' bias columns from LDS
      const int64_t jb = j0 + wc * 32 + l31;
      const float bias = jb < g.H ? th[g.H * g.Fp + jb] : 0.f;
      if constexpr (HESS) {
        // gd = G[t0 .. t0 + 64) dW1z[:, j0 .. j0 + 64): the class columns in chunks of 64 through the K stage's two tiles
        f32x16 gd;
        acc_zero(gd);
        for (int64_t cz0 = 0; cz0 < g.Cz; cz0 += SBK) {
          __syncthreads();  // every wave has read the stage before
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t c = cz0 + sk + e;
            As[srow * SLDT + sk + e] = (arow >= 0 && c < g.Cz) ? g.G[(t0 + srow) * g.Cz + c] : 0.f;
          }
#pragma unroll 1
          for (int cz = wave; cz < SBK; cz += 4) {  // Bs[h][cz] = dW1z[cz0 + cz][j0 + h], lanes along h
            const int64_t c = cz0 + cz, hh = j0 + lane;
            const int64_t half = c >= g.C ? 1 : 0;  // (Cz <= 2 C: no division)
            float v = 0.f;
            if (c < g.Cz && hh < g.H) v = th[g.off1 + (c - half * g.C) * g.ld1 + half * g.H + hh];
            Bs[lane * SLDT + cz] = v;
          }
          __syncthreads();
          tile_nt_step<SBK, SLDT>(As, wr * 32, Bs, wc * 32, lane, gd);
        }
        const bool curved = g.act != LGNN_ACT_RELU;  // (uniform: the ReLU run reads neither h nor G W1)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(wr * 32, lane, r);
          const int64_t t = t0 + row;
          const int rr = rid[row];
          if (t >= cnt || rr < 0 || jb >= g.H) continue;
          const float ds = fmaf(bcol[row], bias, acc[r]);
          const float d = g.dact[int64_t(rr) * g.H + jb];
          float tv = gd[r] * d;
          if (curved) tv = fmaf(g.GW1[t * g.H + jb] * (-2.f * g.h1[int64_t(rr) * g.h1_ld + jb] * d), ds, tv);
          const int64_t o = (int64_t(blockIdx.y) * g.rcap + t) * g.H + jb;
          g.E[o] = d * ds;
          g.T[o] = tv;
        }
      } else if constexpr (ONE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(wr * 32, lane, r);
          const int64_t t = t0 + row;
          if (t < cnt && jb < g.H) g.z[(int64_t(blockIdx.y) * g.rcap + t) * g.H + jb] = fmaf(bcol[row], bias, acc[r]);
        }
      } else {
        const int64_t j = j0 + lane;
        // Ws = 64 hidden columns (from j0) of the z window's rows of W1 = w + off; zacc += Hs Ws^T
        auto times_w1 = [&](const float* __restrict__ w, int64_t off) {
          for (int cz = wave; cz < ((zrows + 31) & ~31); cz += 4) {
            const int64_t c = zw0 + cz;
            float v = 0.f;
            if (c < g.Cz && j < g.H) v = w[off + (c % g.C) * g.ld1 + (c / g.C) * g.H + j];
            Ws[cz * SLDH + lane] = v;
          }
          __syncthreads();
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int zb = wc + 2 * i;
            if (zb * 32 < zrows) tile_nt_step<SBH, SLDH>(Hs, wr * 32, Ws, zb * 32, lane, zacc[i]);  // (uniform in the wave)
          }
        };
        __syncthreads();  // every wave has read the last K stage: the region takes W1's tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(wr * 32, lane, r);
          const float s = fmaf(bcol[row], bias, acc[r]);
          if constexpr (LIN) {
            const int rr = rid[row];
            const float d = (rr >= 0 && jb < g.H) ? g.dact[int64_t(rr) * g.H + jb] : 0.f;
            Hs[row * SLDH + wc * 32 + l31] = d * s;
          } else {
            Hs[row * SLDH + wc * 32 + l31] = act_apply(s, g.act);
          }
        }
        if constexpr (LIN) {
          times_w1(g.W1, 0);
          __syncthreads();  // the tiles take h and the direction's dW1
          const int rr = rid[srow];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t jj = j0 + sk + e;
            Hs[srow * SLDH + sk + e] = (rr >= 0 && jj < g.H) ? g.h1[int64_t(rr) * g.h1_ld + jj] : 0.f;
          }
        }
        times_w1(th, g.off1);
        // (the next tile of the hidden width starts with a barrier before it writes the regions again)
      }
    }
    if constexpr (!ONE && !HESS) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int64_t c = zw0 + (wc + 2 * i) * 32 + l31;
        if ((wc + 2 * i) * 32 >= zrows || c >= g.Cz) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t t = acc_row(t0 + wr * 32, lane, r);
          if (t < cnt) g.z[(int64_t(blockIdx.y) * g.rcap + t) * g.Cz + c] = zacc[i][r];
        }
      }
    }
  }
}

template <class Args>
int launch_first_layer_t(const Args& a, bool two, int64_t ndir, hipStream_t s) {
  const dim3 grid(unsigned(std::min<int64_t>(cdiv(a.rcap, SBM), 512)), unsigned(ndir), two ? unsigned(cdiv(a.Cz, SZW)) : 1u);
  if (two) hipLaunchKernelGGL((first_layer_kernel<Args, false>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((first_layer_kernel<Args, true>), grid, dim3(256), 0, s, a);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// (c) one wave per (sample, batch row): 64 / cw groups of lanes share the row's entries (entry p to group p % groups), the
// groups' partial sums meet in a fixed butterfly order
__global__ __launch_bounds__(256) void sampled_gather_kernel(GatherArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (w >= g.ns * g.M) return;
  const int64_t sl = w / g.M, m = w - sl * g.M;
  const int64_t n = g.idx[m];
  float* __restrict__ o = g.out + w * g.C;
  if (n < 0 || n >= g.N) {  // (flagged by step (a))
    for (int64_t c = lane; c < g.C; c += 64) o[c] = 0.f;
    return;
  }
  const float* __restrict__ zs = g.z + sl * g.rcap * g.Cz;
  const float* __restrict__ th = g.theta + sl * g.P;
  const int ng = 64 / g.cw, grp = lane / g.cw, cl = lane % g.cw;
  const int32_t ps = g.rowptr[n], pe = g.rowptr[n + 1];
  const int64_t coff = g.sage ? g.C : 0;
  for (int64_t c0 = 0; c0 < g.C; c0 += g.cw) {
    const int64_t c = c0 + cl;
    const bool ok = c < g.C;
    const float bias = ok ? th[g.offb + c] : 0.f;
    const float zb = g.sage ? 0.f : bias;  // GCN: the bias is added before the propagation, P (h W1^T + b1)
    float acc = 0.f;
    if (ok)
      for (int32_t p = ps + grp; p < pe; p += ng)
        acc = fmaf(g.val[p], zs[int64_t(g.rpos[g.col[p]]) * g.Cz + coff + c] + zb, acc);
    for (int d = g.cw; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
    if (ok && grp == 0) {
      if (g.sage) acc += zs[int64_t(g.rpos[n]) * g.Cz + c] + bias;
      o[c] = acc;
    }
  }
}

// softmax of the rows of out [rows, C] in place, one wave per row; rows of invalid ids stay zero
__global__ __launch_bounds__(256) void sampled_softmax_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N,
                                                              int64_t rows, int64_t C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;
  const int64_t n = idx[w % M];
  if (n < 0 || n >= N) return;
  float* __restrict__ o = out + w * C;
  float mx = -INFINITY;
  for (int64_t c = lane; c < C; c += 64) mx = fmaxf(mx, o[c]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float sum = 0.f;
  for (int64_t c = lane; c < C; c += 64) sum += expf(o[c] - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int64_t c = lane; c < C; c += 64) o[c] = expf(o[c] - mx) * inv;
}

}  // namespace

// in0: what the first Linear multiplies, seen from an output row, with the bias' column.  The graph and X only.
int sampled_ensure_input(lgnn_ctx* h, hipStream_t s) {
  SampledState& sf = h->sf;
  if (sf.in_valid) return 0;
  const int64_t N = h->N, F = h->dims[0], Fp = h->in_dim[0];
  const bool gcn = h->kind == LGNN_KIND_GCN;
  sf.ldk = cdiv(Fp + 1, 4) * 4;
  LGNN_CALL(sf.in0.reserve(size_t(N) * sf.ldk * 4));
  float* in0 = sf.in0.as<float>();
  LGNN_HIP_CHECK(hipMemsetAsync(in0, 0, size_t(N) * sf.ldk * 4, s));
  if (!gcn)
    LGNN_HIP_CHECK(hipMemcpy2DAsync(in0, size_t(sf.ldk) * 4, h->X, size_t(F) * 4, size_t(F) * 4, size_t(N),
                                    hipMemcpyDeviceToDevice, s));
  LGNN_CALL(launch_spmm(h->P, N, h->X, F, in0 + (gcn ? 0 : F), sf.ldk, F, 0, s));
  hipLaunchKernelGGL(sampled_bias_column_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, h->P.rowptr, h->P.val, N,
                     gcn ? 1 : 0, in0, sf.ldk, Fp);
  LGNN_HIP_CHECK(hipGetLastError());
  sf.in_valid = true;
  return 0;
}

// (a) R = the rows the evaluation nodes read, deduplicated and sorted (sf.rows, sf.count on the device), and where each of
// them stands in R (sf.rpos); 1 layer: R is the batch itself
int sampled_needed_rows(lgnn_ctx* h, const int64_t* idx, int64_t M, hipStream_t s) {
  SampledState& sf = h->sf;
  const int64_t N = h->N;
  const bool two = h->L == 2, sage = h->kind == LGNN_KIND_SAGE;
  int* bad = h->ws.flags.as<int>() + 2;  // "node index outside [0, num_nodes)" (lgnn_check_async_errors)
  LGNN_CALL(sf.rows.reserve(size_t(std::max(N, M)) * 4));
  LGNN_CALL(sf.count.reserve(4));
  int32_t* rows = sf.rows.as<int32_t>();
  int32_t* count = sf.count.as<int32_t>();
  if (two) {
    LGNN_CALL(sf.need.reserve(size_t(N)));
    LGNN_CALL(sf.rpos.reserve(size_t(N) * 4));
    LGNN_HIP_CHECK(hipMemsetAsync(sf.need.p, 0, size_t(N), s));
    hipLaunchKernelGGL(sampled_mark_kernel, dim3(unsigned(cdiv(M, 4))), dim3(256), 0, s, idx, M, N, h->P.rowptr, h->P.col,
                       sage ? 1 : 0, sf.need.as<uint8_t>(), bad);
    LGNN_HIP_CHECK(hipGetLastError());
    LGNN_CALL(compact_flags(sf.need.as<uint8_t>(), N, rows, count, sf.select_tmp, s));
    hipLaunchKernelGGL(sampled_positions_kernel, dim3(unsigned(cdiv(N, 256))), dim3(256), 0, s, rows, count, N,
                       sf.rpos.as<int32_t>());
    LGNN_HIP_CHECK(hipGetLastError());
  } else {
    hipLaunchKernelGGL(sampled_batch_rows_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, N, rows, count, bad);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

int launch_first_layer(const FwdArgs& a, bool two, int64_t ndir, hipStream_t s) { return launch_first_layer_t(a, two, ndir, s); }

int launch_first_layer(const HessArgs& a, int64_t ndir, hipStream_t s) {
  const dim3 grid(unsigned(std::min<int64_t>(cdiv(a.rcap, SBM), 512)), unsigned(ndir), 1u);
  hipLaunchKernelGGL((first_layer_kernel<HessArgs, false>), grid, dim3(256), 0, s, a);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_sampled_gather(const GatherArgs& g, hipStream_t s) {
  LGNN_REQUIRE(cdiv(g.ns * g.M, 4) < (int64_t(1) << 31), "too many (sample, node) pairs per chunk");
  hipLaunchKernelGGL(sampled_gather_kernel, dim3(unsigned(cdiv(g.ns * g.M, 4))), dim3(256), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int sampled_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* theta, int64_t S, uint32_t flags, float* out,
                    hipStream_t s) {
  LGNN_REQUIRE(h->L > 0 && h->X, "no model bound (call lgnn_bind_model first)");
  LGNN_REQUIRE(!h->extras(), "lgnn_sampled_forward: a model bound with res / norm is not covered (its samples take the "
                             "per-sample forward)");
  LGNN_REQUIRE(h->L <= 2, "lgnn_sampled_forward: a model with more than two layers is not covered (its samples take the "
                          "per-sample forward)");
  LGNN_REQUIRE(M >= 0 && S >= 0 && M < (int64_t(1) << 31), "batch size out of range");
  if (M == 0 || S == 0) return 0;
  SampledState& sf = h->sf;
  const int64_t N = h->N, Fp = h->in_dim[0];
  const bool two = h->L == 2, sage = h->kind == LGNN_KIND_SAGE;
  const int64_t H = h->dims[1], C = h->dims[h->L];
  const int64_t Cz = sage ? 2 * C : C, ld1 = sage ? 2 * H : H;
  const int64_t off1 = H * Fp + H, offb = two ? off1 + C * ld1 : C * Fp;
  const int64_t P = h->n_params;
  LGNN_REQUIRE(P == offb + C, "parameter count of the bound model");
  LGNN_CALL(sampled_ensure_input(h, s));
  LGNN_CALL(sampled_needed_rows(h, idx, M, s));
  int32_t* rows = sf.rows.as<int32_t>();
  int32_t* count = sf.count.as<int32_t>();
  const int64_t rcap = two ? N : M;  // host-known bound of |R|
  // chunks of samples: z [chunk, N, Cz] stays under the workspace limit (1 layer: no z, the product is the output)
  int64_t chunk = std::min<int64_t>(S, 32768);
  if (two) {
    const int64_t per_sample = N * Cz * 4;
    chunk = std::max<int64_t>(1, std::min(chunk, h->ws_limit / per_sample));
    LGNN_CALL(sf.z.reserve(size_t(chunk) * per_sample));
  }
  const int64_t gather_waves = chunk * M;
  LGNN_REQUIRE(cdiv(gather_waves, 4) < (int64_t(1) << 31), "too many (sample, node) pairs per chunk");
  int cw = 1;
  while (cw < 64 && cw < C) cw <<= 1;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t ns = std::min(chunk, S - s0);
    float* out_c = out + s0 * M * C;
    HiddenArgs a{};
    a.in0 = sf.in0.as<float>(); a.ldk = sf.ldk;
    a.rows = rows; a.count = count;
    a.theta = theta + s0 * P; a.P = P;
    a.Fp = Fp; a.H = H;
    a.off1 = off1; a.ld1 = ld1; a.C = C; a.Cz = Cz;
    a.z = two ? sf.z.as<float>() : out_c; a.rcap = rcap;
    a.act = h->act;
    if (h->timing) LGNN_CALL(record_event(h, s));
    LGNN_CALL(launch_first_layer_t(a, two, ns, s));
    if (h->timing) LGNN_CALL(record_event(h, s));
    if (two) {
      GatherArgs g{};
      g.idx = idx; g.M = M; g.N = N;
      g.rowptr = h->P.rowptr; g.col = h->P.col; g.val = h->P.val;
      g.rpos = sf.rpos.as<int32_t>();
      g.z = sf.z.as<float>(); g.rcap = rcap; g.Cz = Cz; g.C = C;
      g.sage = sage ? 1 : 0; g.cw = cw;
      g.theta = theta + s0 * P; g.P = P; g.offb = offb;
      g.ns = ns; g.out = out_c;
      LGNN_CALL(launch_sampled_gather(g, s));
    }
    if (flags & LGNN_SAMPLED_SOFTMAX) {
      hipLaunchKernelGGL(sampled_softmax_kernel, dim3(unsigned(cdiv(ns * M, 4))), dim3(256), 0, s, idx, M, N, ns * M, C, out_c);
      LGNN_HIP_CHECK(hipGetLastError());
    }
  }
  return 0;
}

}  // namespace lgnn

using namespace lgnn;

extern "C" int lgnn_sampled_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* theta, int64_t S, uint32_t flags,
                                    float* out, void* stream) {
  if (!h || (M > 0 && S > 0 && (!idx || !theta || !out))) { set_error("null argument"); return 2; }
  return sampled_forward(h, idx, M, theta, S, flags, out, static_cast<hipStream_t>(stream));
}
