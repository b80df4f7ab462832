// Adjacency gradient of the marginal likelihood (adjgrad.hip), plain 2-layer GCN under the diagonal posterior: the closed form.
#include "adjgrad.h"
#include "device_utils.h"

namespace lgnn {

namespace {

// Diagonal posterior (DiagLaplace on an STE-GCN: the shipped gnn/configs/original/stegcn_config.yaml:7).  With
// gamma_p = f / (2 (H_p f + delta_p)) held fixed (f = the likelihood's H_factor), d(-marglik) = f dCE + sum_p gamma_p dH_p, and the diagonal GGN of a
// 2-layer GCN is closed form per batch sample n (laplace/curvature/curvature.py:412-432 with the fork's
// attached Jacobians, :89-130), Ee = [P X | rowsum(P)], H1e = [H_1 | 1], g0e [H, F+1] / g1e [C, H+1] = gamma by (W | b) rows:
//     T_n[j, :] = sum_v P[n, v] mask[v, j] Ee[v, :]      H_{W0|b0}[j, :] += q_n[j] T_n[j, :]^2
//     phi_n     = (P H1e)[n]                             H_{W1|b1}[c, :] += p_c (1 - p_c) phi_n^2
//     q_n[j]    = sum_c p_c W1[c, j]^2 - (sum_c p_c W1[c, j])^2,   p_n = softmax(f_n)
// Reverse, per sample (oracle: diag_marglik_adj_grad, pinned to the reference's model.adj.grad):
//     r[j] = sum_i g0e[j, i] T[j, i]^2      a[c] = sum_j g1e[c, j] phi[j]^2
//     pbar[c] = (1 - 2 p_c) a[c] + sum_j r[j] (W1[c, j]^2 - 2 W1[c, j] m[j]),  m = p W1;   fbar = p * pbar - p (p . pbar) + CE'
//     phibar = 2 phi * (sum_c p_c (1 - p_c) g1e[c, :])        Tbar[j, :] = 2 q[j] g0e[j, :] T[j, :]
//     gradP[(n, v)] += sum_j mask[v, j] <Tbar[j, :], Ee[v, :]> + <phibar, H1e[v]>          (dadj_entry_kernel; candidates: dadj_cand_kernel)
//     h1_bar[v] += P[n, v] phibar[:H]        e_bar[v, :] += P[n, v] sum_j mask[v, j] Tbar[j, :]
// (h1_bar, e_bar and out_bar are propagated once per fit by adjgrad_finish.)  T of a chunk of samples lives in the workspace
// ([chunk][H][F + 1 rounded up to 4] floats: 0.5 GB for a Cora-shaped batch); one workgroup per sample throughout.

__device__ __forceinline__ float block_sum_256(float v, float* red) {  // red: 4 floats of LDS; every thread gets the sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // (red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// The per-sample arrays of the tile kernel in LDS: r, q, mv [H], phi [H + 1], p, a, pb [C], red [4].
struct DadjSample {
  float *r, *q, *mv, *phi, *p, *a, *pb, *red;
  __device__ DadjSample(float* s, int64_t H, int64_t C) {
    r = s; q = r + H; mv = q + H; phi = mv + H; p = phi + H + 1; a = p + C; pb = a + C; red = pb + C;
  }
};

// T[m][j][:] = sum_v P[n, v] mask[v, j] Ee[v, :], n = idx[m0 + m] -- and everything else of the sample, in one pass over the
// tile: p, q (which needs the softmax and W_1 only) first; the row's entries staged VCH at a time, thread <-> 4 x 4 sub-tiles
// in registers (two 16-byte LDS reads per 16 FMAs and staged entry); with the LAST group of entries a sub-tile leaves as
// Tbar = 2 q g0e T and adds its share of r[j] = sum_i g0e T^2 (LDS atomics); then the last layer and the logits' adjoint.
// DET (the fixed-order pass behind DiagLaplace.propose_edges, lgnn_diag_adjgrad_band_sparse): no float atomic decides a bit --
// the last group leaves T unscaled, r[j] is one wave's fixed-order sum over the finished row, a second sweep scales T to Tbar;
// the logits' adjoint goes to fbar [chunk][C] for the serial entry kernel instead of out_bar.
template <bool DET>
__global__ __launch_bounds__(256) void dadj_tile_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ y,
                                                        int64_t m0, int64_t N, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const float* __restrict__ val,
                                                        const float* __restrict__ mask, int64_t H, const float* __restrict__ PX,
                                                        int64_t ldx, const float* __restrict__ rowsum, int64_t F, int VCH,
                                                        const float* __restrict__ probs, int64_t C, const float* __restrict__ W1,
                                                        const float* __restrict__ PH, int64_t ldp,
                                                        const float* __restrict__ gamma, float loss_scale, float* __restrict__ T,
                                                        float* __restrict__ phibar, float* __restrict__ out_bar,
                                                        float* __restrict__ fbar) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int64_t F1 = F + 1, FP = (F1 + 3) & ~int64_t(3), HP = (H + 3) & ~int64_t(3), H1 = H + 1;
  float* __restrict__ mk = sm;                     // [VCH][HP]  w_u * mask rows, zero padded
  float* __restrict__ ev = mk + int64_t(VCH) * HP; // [VCH][FP]  rows of Ee, zero padded
  const DadjSample S(ev + int64_t(VCH) * FP, H, C);
  const float* __restrict__ g0 = gamma;
  const float* __restrict__ gb0 = g0 + H * F;
  const float* __restrict__ g1 = gb0 + H;
  const float* __restrict__ gb1 = g1 + C * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = m0 + blockIdx.x;
  const int64_t n = idx[m];
  float* __restrict__ Tm = T + int64_t(blockIdx.x) * H * FP;
  float* __restrict__ pbm = phibar + int64_t(blockIdx.x) * H1;
  if (n < 0 || n >= N) {  // flagged by the prologue: contributes nothing
    for (int64_t e = tid; e < H * FP; e += 256) Tm[e] = 0.f;
    for (int64_t j = tid; j < H1; j += 256) pbm[j] = 0.f;
    if (DET)
      for (int64_t c = tid; c < C; c += 256) fbar[int64_t(blockIdx.x) * C + c] = 0.f;
    return;
  }
  for (int64_t c = tid; c < C; c += 256) S.p[c] = probs[m * C + c];
  for (int64_t j = tid; j < H1; j += 256) S.phi[j] = j < H ? PH[n * ldp + j] : rowsum[n];
  __syncthreads();
  for (int64_t j = tid; j < H; j += 256) {
    float s1 = 0.f, s2 = 0.f;
    for (int64_t c = 0; c < C; ++c) {
      const float w = W1[c * H + j];
      s1 = fmaf(S.p[c], w, s1);
      s2 = fmaf(S.p[c] * w, w, s2);
    }
    S.mv[j] = s1;
    S.q[j] = s2 - s1 * s1;
    S.r[j] = 0.f;
  }
  const int32_t ps = rowptr[n], pe = rowptr[n + 1];
  if (ps == pe)
    for (int64_t e = tid; e < H * FP; e += 256) Tm[e] = 0.f;
  const int nI = int(FP / 4), nSub = int(HP / 4) * nI;
  for (int32_t p0 = ps; p0 < pe; p0 += VCH) {
    const int un = min(VCH, pe - p0);
    const bool last = p0 + VCH >= pe;
    __syncthreads();
    for (int64_t t = tid; t < int64_t(un) * (HP + FP); t += 256) {
      const int u = int(t / (HP + FP));
      const int64_t k = t - int64_t(u) * (HP + FP);
      const int64_t v = col[p0 + u];
      if (k < HP) mk[int64_t(u) * HP + k] = k < H ? val[p0 + u] * mask[v * H + k] : 0.f;
      else {
        const int64_t i = k - HP;
        ev[int64_t(u) * FP + i] = i < F ? PX[v * ldx + i] : (i == F ? rowsum[v] : 0.f);
      }
    }
    __syncthreads();
    for (int st = tid; st < nSub; st += 256) {
      const int jb = st / nI, ib = st - jb * nI;
      float acc[4][4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t j = 4 * jb + rr;
        const float4 t4 = (p0 == ps || j >= H) ? make_float4(0.f, 0.f, 0.f, 0.f)
                                               : *reinterpret_cast<const float4*>(Tm + j * FP + 4 * ib);
        acc[rr][0] = t4.x; acc[rr][1] = t4.y; acc[rr][2] = t4.z; acc[rr][3] = t4.w;
      }
      for (int u = 0; u < un; ++u) {
        const float4 m4 = *reinterpret_cast<const float4*>(mk + int64_t(u) * HP + 4 * jb);
        const float4 e4 = *reinterpret_cast<const float4*>(ev + int64_t(u) * FP + 4 * ib);
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ee[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) acc[rr][cc] = fmaf(mm[rr], ee[cc], acc[rr][cc]);
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t j = 4 * jb + rr;
        if (j >= H) continue;
        if (last && !DET) {  // T -> Tbar on the way out, r[j] from the unscaled entries
          const float qj = 2.f * S.q[j];
          float rs = 0.f;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const int64_t i = 4 * ib + cc;
            const float g = i < F ? g0[j * F + i] : (i == F ? gb0[j] : 0.f);
            const float t = acc[rr][cc];
            rs = fmaf(g * t, t, rs);
            acc[rr][cc] = qj * g * t;
          }
          atomicAdd(&S.r[j], rs);
        }
        *reinterpret_cast<float4*>(Tm + j * FP + 4 * ib) = make_float4(acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]);
      }
    }
  }
  if (DET) {
    __syncthreads();  // T is complete (this workgroup's own writes)
    if (ps != pe)
      for (int64_t j = wave; j < H; j += 4) {
        float rs = 0.f;
        for (int64_t i = lane; i < F1; i += 64) {
          const float t = Tm[j * FP + i];
          rs = fmaf((i < F ? g0[j * F + i] : gb0[j]) * t, t, rs);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rs += __shfl_xor(rs, o);
        if (lane == 0) S.r[j] = rs;
      }
    __syncthreads();
    if (ps != pe)
      for (int64_t e = tid; e < H * FP; e += 256) {
        const int64_t j = e / FP, i = e - j * FP;
        const float g = i < F ? g0[j * F + i] : (i == F ? gb0[j] : 0.f);
        Tm[e] = 2.f * S.q[j] * g * Tm[e];
      }
  }
  __syncthreads();  // r is complete
  for (int64_t c = wave; c < C; c += 4) {
    float acc = 0.f;
    for (int64_t j = lane; j < H1; j += 64) acc = fmaf((j < H ? g1[c * H + j] : gb1[c]) * S.phi[j], S.phi[j], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) S.a[c] = acc;
  }
  __syncthreads();
  for (int64_t c = wave; c < C; c += 4) {
    float acc = 0.f;
    for (int64_t j = lane; j < H; j += 64) {
      const float w = W1[c * H + j];
      acc = fmaf(S.r[j], w * w - 2.f * w * S.mv[j], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) S.pb[c] = (1.f - 2.f * S.p[c]) * S.a[c] + acc;
  }
  __syncthreads();
  float part = 0.f;
  for (int64_t c = tid; c < C; c += 256) part = fmaf(S.p[c], S.pb[c], part);
  const float dot = block_sum_256(part, S.red);
  const int64_t yc = y[m];
  if (DET)
    for (int64_t c = tid; c < C; c += 256)
      fbar[int64_t(blockIdx.x) * C + c] = S.p[c] * (S.pb[c] - dot) + loss_scale * (S.p[c] - (c == yc ? 1.f : 0.f));
  else if (out_bar)  // (null: a row band's second visit of the sample, adjband.hip -- the sparse pass has accumulated it)
    for (int64_t c = tid; c < C; c += 256)
      atomicAdd(&out_bar[n * C + c], S.p[c] * (S.pb[c] - dot) + loss_scale * (S.p[c] - (c == yc ? 1.f : 0.f)));
  for (int64_t j = tid; j < H1; j += 256) {
    float lg = 0.f;
    for (int64_t c = 0; c < C; ++c) lg = fmaf(S.p[c] * (1.f - S.p[c]), j < H ? g1[c * H + j] : gb1[c], lg);
    pbm[j] = 2.f * S.phi[j] * lg;
  }
}

// value of one (sample, column node v) pair: sum_j mask[v, j] <Tbar[j, :], Ee[v, :]> + <phibar, H1e[v]> (candidate pairs; the
// stored entries take dadj_entry_kernel).  mk: [H] floats of LDS.  Every thread returns the value.
__device__ __forceinline__ float dadj_pair(const float* __restrict__ Tm, const float* __restrict__ pbm, int64_t v, int64_t H,
                                           int64_t F, const float* __restrict__ mask, const float* __restrict__ PX, int64_t ldx,
                                           const float* __restrict__ rowsum, const float* __restrict__ H1p, int64_t ldh,
                                           float* __restrict__ mk, float* __restrict__ red) {
  const int tid = threadIdx.x;
  const int64_t F1 = F + 1, FP = (F1 + 3) & ~int64_t(3);
  __syncthreads();
  for (int64_t j = tid; j < H; j += 256) mk[j] = mask[v * H + j];
  __syncthreads();
  float part = 0.f;
  for (int64_t i = tid; i < F1; i += 256) {
    float ca = 0.f;
    for (int64_t j = 0; j < H; ++j)
      if (mk[j] != 0.f) ca = fmaf(mk[j], Tm[j * FP + i], ca);
    part = fmaf(ca, i < F ? PX[v * ldx + i] : rowsum[v], part);
  }
  for (int64_t j = tid; j < H; j += 256) part = fmaf(pbm[j], H1p[v * ldh + j], part);
  if (tid == 0) part += pbm[H];
  return block_sum_256(part, red);
}

// The entries of a sample's row, EV at a time: ca[u][i] = sum_j mask[v_u, j] Tbar[j, i] is an (EV x H) . (H x F1) product per
// group.  Thread <-> (ib, jq): four columns of the tile (one 16-byte load per row) and every NJ-th row; the EV mask values of a
// row are two 16-byte LDS broadcasts; 32 FMAs per row visited.  The row slices meet in LDS (cas [EV][ICH], float atomics when
// NJ > 1), ICH columns at a time; the sums are then contracted with Ee[v_u, :] (gradP) and scattered (e_bar).
constexpr int EV = 8;
constexpr int ICH = 1024;  // columns of the tile per pass (cas: 32 KiB)
// DET: ONE workgroup takes the chunk's samples one after the other (launched with a grid of 1), the row slices are not split
// (NJ = 1: no LDS atomics), and out_bar takes the tile kernel's fbar here -- every address is added to in sample order.
template <bool DET>
__global__ __launch_bounds__(256) void dadj_entry_kernel(const int64_t* __restrict__ idx, int64_t m0, int64_t N,
                                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, const float* __restrict__ mask, int64_t H,
                                                         const float* __restrict__ PX, int64_t ldx,
                                                         const float* __restrict__ rowsum, int64_t F,
                                                         const float* __restrict__ H1p, int64_t ldh, const float* __restrict__ T,
                                                         const float* __restrict__ phibar, float* __restrict__ gradP,
                                                         float* __restrict__ h1_bar, float* __restrict__ e_bar, int64_t mc,
                                                         int64_t C, const float* __restrict__ fbar,
                                                         float* __restrict__ out_bar) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int64_t F1 = F + 1, FP = (F1 + 3) & ~int64_t(3);
  const int icw = int(min<int64_t>(ICH, FP));   // columns per pass
  float* __restrict__ mk = sm;                   // [H][EV]
  float* __restrict__ cas = mk + H * EV;         // [EV][icw]
  float* __restrict__ red = cas + EV * icw;      // [4][EV]
  float* __restrict__ wv = red + 4 * EV;         // [EV]
  int32_t* __restrict__ vid = reinterpret_cast<int32_t*>(wv + EV);  // [EV]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t blk = DET ? 0 : int64_t(blockIdx.x); blk < (DET ? mc : int64_t(blockIdx.x) + 1); ++blk) {
  const int64_t n = idx[m0 + blk];
  if (n < 0 || n >= N) continue;  // (uniform over the workgroup)
  if (DET) {
    __syncthreads();  // the previous sample's adds are done before this one's
    for (int64_t c = tid; c < C; c += 256) out_bar[n * C + c] += fbar[blk * C + c];
  }
  const float* __restrict__ Tm = T + blk * H * FP;
  const float* __restrict__ pbm = phibar + blk * (H + 1);
  const int32_t ps = rowptr[n], pe = rowptr[n + 1];
  for (int32_t p0 = ps; p0 < pe; p0 += EV) {
    const int un = min(EV, pe - p0);
    __syncthreads();
    if (tid < EV) {
      vid[tid] = tid < un ? col[p0 + tid] : 0;
      wv[tid] = tid < un ? val[p0 + tid] : 0.f;
    }
    __syncthreads();
    for (int64_t t = tid; t < H * EV; t += 256) {
      const int u = int(t % EV);
      mk[t] = u < un ? mask[int64_t(vid[u]) * H + t / EV] : 0.f;
    }
    float part[EV];
#pragma unroll
    for (int u = 0; u < EV; ++u) part[u] = 0.f;
    for (int64_t c0 = 0; c0 < FP; c0 += icw) {
      const int cw = int(min<int64_t>(icw, FP - c0));  // a multiple of 4
      const int nI = cw / 4;
      const int NJ = (DET || nI >= 256) ? 1 : int(min<int64_t>(256 / nI, H));  // row slices
      __syncthreads();  // mk staged / the previous pass's cas consumed
      if (NJ > 1)
        for (int t = tid; t < EV * cw; t += 256) cas[(t / cw) * icw + (t % cw)] = 0.f;
      __syncthreads();
      for (int st = tid; st < nI * NJ; st += 256) {
        const int jq = st / nI, ib = st - jq * nI;
        float ca[EV][4];
#pragma unroll
        for (int u = 0; u < EV; ++u)
#pragma unroll
          for (int c = 0; c < 4; ++c) ca[u][c] = 0.f;
        for (int64_t j = jq; j < H; j += NJ) {
          const float4 t4 = *reinterpret_cast<const float4*>(Tm + j * FP + c0 + 4 * ib);
          const float4 m0v = *reinterpret_cast<const float4*>(mk + j * EV);
          const float4 m1v = *reinterpret_cast<const float4*>(mk + j * EV + 4);
          const float mm[EV] = {m0v.x, m0v.y, m0v.z, m0v.w, m1v.x, m1v.y, m1v.z, m1v.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
          for (int u = 0; u < EV; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) ca[u][c] = fmaf(mm[u], tt[c], ca[u][c]);
        }
#pragma unroll
        for (int u = 0; u < EV; ++u)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (NJ > 1) atomicAdd(&cas[u * icw + 4 * ib + c], ca[u][c]);
            else cas[u * icw + 4 * ib + c] = ca[u][c];
          }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < EV; ++u)
        if (u < un) {
          const int64_t v = vid[u];
          for (int i = tid; i < cw; i += 256) {
            const int64_t gi = c0 + i;
            if (gi >= F1) break;
            const float c = cas[u * icw + i];
            part[u] = fmaf(c, gi < F ? PX[v * ldx + gi] : rowsum[v], part[u]);
            if (c != 0.f) atomicAdd(&e_bar[v * F1 + gi], wv[u] * c);
          }
        }
    }
    for (int64_t j = tid; j < H; j += 256) {
      const float pj = pbm[j];
#pragma unroll
      for (int u = 0; u < EV; ++u)
        if (u < un) {
          const int64_t v = vid[u];
          part[u] = fmaf(pj, H1p[v * ldh + j], part[u]);
          atomicAdd(&h1_bar[v * H + j], wv[u] * pj);
        }
    }
#pragma unroll
    for (int u = 0; u < EV; ++u) {
      float x = part[u];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
      if (lane == 0) red[wave * EV + u] = x;
    }
    __syncthreads();
    if (tid < un)  // (a repeated node id: several samples share the entry, hence the atomic)
      atomicAdd(&gradP[p0 + tid], red[tid] + red[EV + tid] + red[2 * EV + tid] + red[3 * EV + tid] + pbm[H]);
  }
  }
}

// candidate pairs (a, b): a contributes through the samples that are a -- the first one's tile, times its multiplicity
__global__ __launch_bounds__(256) void dadj_cand_kernel(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb, int64_t K,
                                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ mult,
                                                        int64_t m0, int64_t mc, const float* __restrict__ mask, int64_t H,
                                                        const float* __restrict__ PX, int64_t ldx,
                                                        const float* __restrict__ rowsum, int64_t F,
                                                        const float* __restrict__ H1p, int64_t ldh, const float* __restrict__ T,
                                                        const float* __restrict__ phibar, float* __restrict__ grad_cand) {
  extern __shared__ float sm[];
  float* __restrict__ mk = sm;
  float* __restrict__ red = mk + H;
  for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
    const int32_t m = pos[ca[k]];
    if (m == INT32_MAX || m < m0 || m >= m0 + mc) continue;  // (uniform over the workgroup)
    const float* __restrict__ Tm = T + int64_t(m - m0) * H * ((F + 4) & ~int64_t(3));
    const float* __restrict__ pbm = phibar + int64_t(m - m0) * (H + 1);
    const float tot = dadj_pair(Tm, pbm, cb[k], H, F, mask, PX, ldx, rowsum, H1p, ldh, mk, red);
    if (threadIdx.x == 0) grad_cand[k] += float(mult[m]) * tot;
  }
}

}  // namespace

// dense != null (lgnn_diag_adjgrad_batch_dense): the entries' terms are also added on the full grid (lora.hip).
// band1 > band0 (lgnn_diag_adjgrad_band_batch, adjband.hip): dense holds the rows [band0, band1) of that grid and nothing else
// is accumulated -- the tiles of the samples are formed again, the entry and candidate kernels are skipped, the four
// accumulators are null.  det (lgnn_diag_adjgrad_band_sparse): the fixed-order kernels -- the same sums, the same bits on every run;
// the entry kernel then runs the chunk's samples one after the other in one workgroup.
int diag_adjgrad_batch_gcn(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma, float loss_scale,
                           float* grad_P, float* out_bar, float* h1_bar, float* e_bar, const int32_t* cand_a,
                           const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s, float* dense, int64_t band0,
                           int64_t band1, bool det) {
  LGNN_CALL(check_model(h));
  LGNN_REQUIRE(h->kind == LGNN_KIND_GCN, "adjacency gradient, diagonal posterior: GCN models");
  const bool band = band1 > band0;
  LGNN_REQUIRE(!det || (!band && !dense && K == 0), "fixed-order pass: stored entries only");
  LGNN_REQUIRE(M > 0 && idx && y && gamma, "empty batch or null pointers");
  if (band) LGNN_REQUIRE(dense && !grad_P && !out_bar && !h1_bar && !e_bar && K == 0, "row band: the band buffer only");
  else LGNN_REQUIRE(grad_P && out_bar && h1_bar && e_bar, "empty batch or null pointers");
  LGNN_CALL(forward_ensure_aux(h, s));
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], F = h->dims[0], F1 = F + 1;
  LGNN_REQUIRE(h->in_dim[1] == H, "internal: GCN head stride");
  LGNN_CALL(batch_prologue(h, idx, y, M, false, false, nullptr, s));
  // T of a chunk of samples under the workspace cap
  const int64_t FP = (F1 + 3) & ~int64_t(3), HP = (H + 3) & ~int64_t(3);  // tile rows / staged rows padded to 16 bytes
  const int64_t per_sample = H * FP * 4;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(M, h->ws_limit / per_sample));
  // tile kernel: staged entries (as many as fit, at most 8) + the per-sample arrays, within the 64 KiB of a default launch
  const size_t smem_s = size_t(3 * H + (H + 1) + 3 * C + 4) * 4;
  LGNN_REQUIRE(smem_s + size_t(HP + FP) * 4 <= 62 * 1024, "adjacency gradient, diagonal posterior: hidden + input width too large");
  const int vch = int(std::min<int64_t>(8, (62 * 1024 - int64_t(smem_s)) / ((HP + FP) * 4)));
  const size_t smem_t = size_t(vch) * (HP + FP) * 4;
  const size_t smem_e = size_t(H * 8 + 8 * std::min<int64_t>(1024, FP) + 4 * 8 + 8 + 8) * 4;  // (dadj_entry_kernel: EV = 8 mask rows + the column sums of a pass; the candidates' kernel needs H + 4)
  LGNN_REQUIRE(smem_e <= 60 * 1024, "adjacency gradient, diagonal posterior: hidden width too large");
  const float* mask = h->fc.dact0.as<float>();
  const float* PX = h->fc.prop_in[0].as<float>();
  const int64_t ldx = h->fc.prop_ld[0];
  const float* rowsum = h->fc.rowsum.as<float>();
  LGNN_CALL(h->ws.jac.reserve(size_t(chunk) * per_sample));
  LGNN_CALL(h->ws.misc.reserve(size_t(chunk) * (H + 1 + C) * 4));
  float* T = h->ws.jac.as<float>();
  float* phibar = h->ws.misc.as<float>();
  float* fbar = phibar + chunk * (H + 1);  // [chunk][C]: the logits' adjoints of a chunk (fixed-order pass)
  for (int64_t m0 = 0; m0 < M; m0 += chunk) {
    const int64_t mc = std::min(chunk, M - m0);
#define LGNN_DADJ_TILE(DETV)                                                                                                    \
    hipLaunchKernelGGL(dadj_tile_kernel<DETV>, dim3(unsigned(mc)), dim3(256), smem_t + smem_s, s, idx,                            \
                       static_cast<const int64_t*>(y), m0, N, h->P.rowptr, h->P.col, h->P.val, mask, H, PX, ldx, rowsum, F, vch,  \
                       h->ws.probs.as<float>(), C, h->W[1], h->fc.prop_in[1].as<float>(), h->fc.prop_ld[1], gamma, loss_scale, T, \
                       phibar, out_bar, fbar)
#define LGNN_DADJ_ENTRY(DETV, GRID)                                                                                             \
    hipLaunchKernelGGL(dadj_entry_kernel<DETV>, dim3(GRID), dim3(256), smem_e, s, idx, m0, N, h->P.rowptr, h->P.col, h->P.val,  \
                       mask, H, PX, ldx, rowsum, F, h->fc.hact_p[0], h->fc.hact_ld[0], T, phibar, grad_P, h1_bar, e_bar, mc, C, \
                       fbar, out_bar)
    if (det) {
      LGNN_DADJ_TILE(true);
      LGNN_DADJ_ENTRY(true, 1u);
    } else {
      LGNN_DADJ_TILE(false);
      if (!band) LGNN_DADJ_ENTRY(false, unsigned(mc));
    }
#undef LGNN_DADJ_TILE
#undef LGNN_DADJ_ENTRY
    if (K > 0)
      hipLaunchKernelGGL(dadj_cand_kernel, dim3(unsigned(std::min<int64_t>(K, 65535))), dim3(256), size_t(H + 4) * 4, s, cand_a, cand_b, K,
                         h->ws.pos.as<int32_t>(), h->ws.mult.as<int32_t>(), m0, mc, mask, H, PX, ldx, rowsum, F,
                         h->fc.hact_p[0], h->fc.hact_ld[0], T, phibar, grad_cand);
    LGNN_HIP_CHECK(hipGetLastError());
    if (dense)
      LGNN_CALL(launch_dense_diag_pair(idx, m0, mc, N, h->ws.pos.as<int32_t>(), h->ws.mult.as<int32_t>(), mask, H, PX, ldx, rowsum,
                                       F, h->fc.hact_p[0], h->fc.hact_ld[0], T, phibar, band ? band0 : 0, band ? band1 : N,
                                       dense, s));
  }
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn
