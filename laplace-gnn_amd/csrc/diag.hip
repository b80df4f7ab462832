// Diagonal GGN of one mini-batch, without materialising Jacobians.
//
// Reference: GGNInterface.diag (laplace/curvature/curvature.py:412-432) builds Js[M, C, P] with
// torch.func.jacrev (:89-130; 3.4 GB for the Cora-shaped config) and contracts
// einsum('bcp,bck,bkp->p', Js, Lambda, Js), Lambda_n = diag(p_n) - p_n p_n^T (:365-372).
// For the model family of the path the per-sample Jacobian is closed form:
//
//   last layer (any L):  J_n wrt W_{L-1} = I_C (x) phi_n, wrt b = s_n I_C
//        diag(W)[k,i] = sum_n Lambda_n[k,k] phi_n[i]^2 ,  diag(b)[k] = sum_n Lambda_n[k,k] s_n^2
//        GCN : phi_n = (P h)[n], s_n = rowsum(P)[n]      GraphSAGE: phi_n = cat[n], s_n = 1
//   first layer of a 2-layer model: with E[v] = [in-features the first Linear multiplies | bias column]
//        GCN : E[v] = [(P X)[v] | rowsum(P)[v]],   GraphSAGE: E[v] = [cat_0[v] | 1]
//        T[n,j,i] = sum_v P[n,v] act'(h_1[v,j]) E[v,i]     S[n,j,i] = act'(h_1[n,j]) E[n,i]  (GraphSAGE self path)
//        diag(W_0)[j,i] = sum_n qbb[n,j] T^2 + 2 qab[n,j] S T + qaa[n,j] S^2
//        q**[n,j] = w*_j^T Lambda_n w*_j with w_j the j-th column of the self / neighbour half of W_1.
// The reference cannot construct models with more than 2 layers (live breakpoint at
// gnn/models/base_gnn.py:109), so L <= 2 covers everything it can run; deeper models and models with res / norm contract
// chunks of explicit Jacobians (diag_from_jacobians).
//
// The file holds the kernels, one launcher per kernel and the driver diag_accumulate.  The empirical / Monte-Carlo Fisher's
// diagonal (fisher.hip) is the same sum with other weights: it calls the launchers diag.h declares.
#include "closedform.h"
#include "device_utils.h"
#include "diag.h"
#include "lgnn_internal.h"

namespace lgnn {

namespace {

// q[m, j] = w_j^T Lambda_m u_j = sum_k p_k w_kj u_kj - (sum_k p_k w_kj)(sum_k p_k u_kj)
// out[0] = (neigh,neigh), out[1] = (self,neigh), out[2] = (self,self); W1 is [C, ldw]
__global__ void q_kernel(const float* __restrict__ probs, int64_t M, int64_t C, const float* __restrict__ W1,
                         int64_t ldw, int64_t d, int64_t off_self, int64_t off_neigh, int has_self,
                         float* __restrict__ q) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * d) return;
  const int64_t m = t / d, j = t - m * d;
  float snn = 0.f, sn = 0.f, sss = 0.f, ss = 0.f, ssn = 0.f;
  if (!probs) {  // regression: Lambda = I (laplace/curvature/curvature.py:429-430), q = sum_k w_kj u_kj
    for (int64_t k = 0; k < C; ++k) {
      const float wn = W1[k * ldw + off_neigh + j];
      snn += wn * wn;
      if (has_self) {
        const float ws = W1[k * ldw + off_self + j];
        sss += ws * ws;
        ssn += ws * wn;
      }
    }
    q[t] = snn;
    if (has_self) { q[M * d + t] = ssn; q[2 * M * d + t] = sss; }
    return;
  }
  // centred form: q = sum_k p_k (w_k - wbar)(u_k - ubar), wbar = sum_k p_k w_k -- no cancellation between two large sums
  // (and exactly zero for a single class, where softmax is 1 and Lambda vanishes)
  for (int64_t k = 0; k < C; ++k) {
    const float p = probs[m * C + k];
    sn += p * W1[k * ldw + off_neigh + j];
    if (has_self) ss += p * W1[k * ldw + off_self + j];
  }
  for (int64_t k = 0; k < C; ++k) {
    const float p = probs[m * C + k];
    const float dn = W1[k * ldw + off_neigh + j] - sn;
    snn += p * dn * dn;
    if (has_self) {
      const float dsf = W1[k * ldw + off_self + j] - ss;
      sss += p * dsf * dsf;
      ssn += p * dsf * dn;
    }
  }
  q[t] = snn;
  if (has_self) {
    q[M * d + t] = ssn;
    q[2 * M * d + t] = sss;
  }
}

// Classification batches of the closed-form diagonal: what batch_prologue + q_kernel did in five launches (mark, clear,
// seed, q, unmark) as one.  One wave per sample: p = softmax(logits[idx[m]]) -> probs, loss += logsumexp - f[y]
// (CrossEntropyLoss(reduction='sum')), the q rows of q_kernel from the probabilities in LDS, and the sticky flags the
// prologue raises (word 1: node id out of range, word 0 = 2: label out of range).  The diagonal needs neither the batch
// positions nor the multiplicities of duplicated ids (every occurrence is its own sample), so nothing is marked.
__global__ __launch_bounds__(256) void diag_prologue_kernel(const float* __restrict__ logits, int64_t C,
                                                            const int64_t* __restrict__ idx, const int64_t* __restrict__ y,
                                                            int64_t M, int64_t N, const float* __restrict__ W1, int64_t ldw,
                                                            int64_t d, int64_t off_self, int64_t off_neigh, int has_self,
                                                            float* __restrict__ probs, float* __restrict__ q,
                                                            float* __restrict__ loss, int* __restrict__ bad) {
  extern __shared__ float sm[];
  __shared__ float loss_part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* p_s = sm + size_t(wave) * C;
  float loss_acc = 0.f;
  for (int64_t m = int64_t(blockIdx.x) * 4 + wave; m < M; m += int64_t(gridDim.x) * 4) {
    const int64_t n = idx[m];
    if (n < 0 || n >= N) {  // no entries in the first-layer kernel, zero weight in the last-layer kernel
      if (lane == 0) bad[1] = 1;
      for (int64_t k = lane; k < C; k += 64) probs[m * C + k] = 0.f;
      for (int64_t j = lane; j < (has_self ? 3 : 1) * d; j += 64) q[(j / d) * M * d + m * d + (j % d)] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int64_t k = lane; k < C; k += 64) { const float v = logits[n * C + k]; p_s[k] = v; mx = fmaxf(mx, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float fy = 0.f;
    if (lane == 0) {
      const int64_t yy = y[m];
      if (yy < 0 || yy >= C) *bad = 2;
      else fy = logits[n * C + yy];
    }
    float se = 0.f;
    for (int64_t k = lane; k < C; k += 64) { const float e = expf(p_s[k] - mx); p_s[k] = e; se += e; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const float inv = 1.0f / se;
    for (int64_t k = lane; k < C; k += 64) { const float p = p_s[k] * inv; p_s[k] = p; probs[m * C + k] = p; }
    if (lane == 0) loss_acc += logf(se) + mx - fy;
    // p_s is read across lanes below: same wave, LDS executes a wave's operations in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int64_t j = lane; j < d; j += 64) {  // q_kernel's centred form, same summation order
      float sn = 0.f, ss = 0.f, snn = 0.f, sss = 0.f, ssn = 0.f;
      for (int64_t k = 0; k < C; ++k) {
        sn += p_s[k] * W1[k * ldw + off_neigh + j];
        if (has_self) ss += p_s[k] * W1[k * ldw + off_self + j];
      }
      for (int64_t k = 0; k < C; ++k) {
        const float p = p_s[k];
        const float dn = W1[k * ldw + off_neigh + j] - sn;
        snn += p * dn * dn;
        if (has_self) {
          const float dsf = W1[k * ldw + off_self + j] - ss;
          sss += p * dsf * dsf;
          ssn += p * dsf * dn;
        }
      }
      q[m * d + j] = snn;
      if (has_self) { q[M * d + m * d + j] = ssn; q[2 * M * d + m * d + j] = sss; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the next sample overwrites p_s
  }
  if (lane == 0) loss_part[wave] = loss_acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (loss_part[0] + loss_part[1]) + (loss_part[2] + loss_part[3]));
}

constexpr int JPT = 16;  // hidden units per thread
constexpr int DCH = 32;  // (sample, neighbour) entries staged per chunk

// grid (i-chunks of 64, j-chunks of 64, sample slabs); block 256 = 64 i-lanes x 4 j-groups of JPT.
//   T[n, j, i] = sum_v P[n, v] act'(h_1[v, j]) E[v, i]     diag(W_0)[j, i] += q[n, j] T^2  (+ the GraphSAGE self terms)
// At the shapes this runs at (Cora: 16 MB in total) the kernel is bound by load LATENCY, not bytes or flops: a thread
// that walks its samples' neighbours one after the other waits for one dependent load chain per neighbour (0.25 ms for
// 1 299 samples).  So the slab's (sample, neighbour) entries are laid out as ONE list -- every sample followed by a
// virtual entry for the node itself that closes the sample (and carries the self row GraphSAGE needs) -- and consumed in
// chunks of DCH: wave 0 resolves the chunk's entries (sample, column, value), all four waves then fetch the entries'
// feature and derivative row slices into LDS with every load of the chunk in flight at once, and the FMAs run from LDS.
template <int HAS_SELF>
__global__ __launch_bounds__(256) void diag_first_layer_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
    const int64_t* __restrict__ idx, int64_t M, int64_t slab, FeatView E, const float* __restrict__ dact,
    int64_t H, const float* __restrict__ q, float* __restrict__ diag_w, float* __restrict__ diag_b) {
  __shared__ float sE[DCH][64], sD[DCH][64], sQ[HAS_SELF ? 3 : 1][DCH][64];
  __shared__ float sa[DCH];
  __shared__ int32_t sv[DCH], sm[DCH];  // column (node) of the entry; sample index if the entry closes its sample, else -1
  __shared__ int32_t soff[65], snode[64];
  const int tid = threadIdx.x, lane = tid & 63, jg = tid >> 6;
  const int64_t i = int64_t(blockIdx.x) * 64 + lane;
  const int64_t j0 = int64_t(blockIdx.y) * 64;
  const int64_t ncols = E.width + 1;
  const bool i_ok = i < ncols;
  const int64_t m_begin = int64_t(blockIdx.z) * slab, m_end = min(M, m_begin + slab);
  const int ns = int(m_end - m_begin);  // <= 64
  // entry offsets of the slab's samples: len(row) + 1 each (invalid node ids: 0, flagged by the batch prologue)
  if (tid < 64) {
    int32_t len = 0, node = -1;
    if (tid < ns) {
      const int64_t n = idx[m_begin + tid];
      if (n >= 0 && n < E.nrows) { node = int32_t(n); len = rowptr[n + 1] - rowptr[n] + 1; }
    }
    snode[tid] = node;
    int32_t incl = len;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    soff[tid + 1] = incl;
    if (tid == 0) soff[0] = 0;
  }
  __syncthreads();
  const int32_t etot = soff[64];
  float acc[JPT], T[JPT];
#pragma unroll
  for (int jj = 0; jj < JPT; ++jj) { acc[jj] = 0.f; T[jj] = 0.f; }

  for (int32_t c0 = 0; c0 < etot; c0 += DCH) {
    const int cn = min(DCH, int(etot - c0));
    // (1) wave 0: resolve the chunk's entries
    if (tid < DCH) {
      int32_t v = 0, mk = -1;
      float a = 0.f;
      if (tid < cn) {
        const int32_t g = c0 + tid;
        int lo = 0, hi = ns;  // sample k with soff[k] <= g < soff[k + 1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= g) lo = mid; else hi = mid; }
        const int32_t node = snode[lo], r = g - soff[lo], len = soff[lo + 1] - soff[lo] - 1;
        if (r < len) { const int32_t p = rowptr[node] + r; v = col[p]; a = val[p]; }
        else { v = node; mk = lo; }  // the virtual entry: closes sample lo, weight 0
      }
      sv[tid] = v; sa[tid] = a; sm[tid] = mk;
    }
    __syncthreads();
    // (2) all waves: the entries' row slices, every load of the chunk in flight at once
    for (int e = jg; e < cn; e += 4) {
      const int64_t v = sv[e];
      sE[e][lane] = i_ok ? feat(E, v, i) : 0.f;
      sD[e][lane] = (j0 + lane < H) ? dact[v * H + j0 + lane] : 0.f;
      const int mk = sm[e];
      if (mk >= 0) {
        const int64_t m = m_begin + mk;
        const bool ok = j0 + lane < H;
        sQ[0][e][lane] = ok ? q[m * H + j0 + lane] : 0.f;
        if (HAS_SELF) {
          sQ[1][e][lane] = ok ? q[M * H + m * H + j0 + lane] : 0.f;
          sQ[2][e][lane] = ok ? q[2 * M * H + m * H + j0 + lane] : 0.f;
        }
      }
    }
    __syncthreads();
    // (3) FMAs from LDS; a closing entry folds the finished T into the accumulator
    for (int e = 0; e < cn; ++e) {
      const float ev = sE[e][lane];
      const float4* __restrict__ dr = reinterpret_cast<const float4*>(&sD[e][jg * JPT]);
      const int mk = sm[e];
      if (mk < 0) {
        const float ea = ev * sa[e];
#pragma unroll
        for (int q4 = 0; q4 < JPT / 4; ++q4) {
          const float4 d4 = dr[q4];
          T[4 * q4] = fmaf(d4.x, ea, T[4 * q4]); T[4 * q4 + 1] = fmaf(d4.y, ea, T[4 * q4 + 1]);
          T[4 * q4 + 2] = fmaf(d4.z, ea, T[4 * q4 + 2]); T[4 * q4 + 3] = fmaf(d4.w, ea, T[4 * q4 + 3]);
        }
      } else {
#pragma unroll
        for (int jj = 0; jj < JPT; ++jj) {
          const float qbb = sQ[0][e][jg * JPT + jj];
          if (HAS_SELF) {
            const float sf = sD[e][jg * JPT + jj] * ev;
            acc[jj] += qbb * T[jj] * T[jj] + 2.f * sQ[1][e][jg * JPT + jj] * sf * T[jj] + sQ[2][e][jg * JPT + jj] * sf * sf;
          } else {
            acc[jj] += qbb * T[jj] * T[jj];
          }
          T[jj] = 0.f;
        }
      }
    }
    __syncthreads();
  }
  if (!i_ok) return;
#pragma unroll
  for (int jj = 0; jj < JPT; ++jj) {
    const int64_t j = j0 + jg * JPT + jj;
    if (j < H) {
      if (i < E.width) atomicAdd(&diag_w[j * E.width + i], acc[jj]);
      else atomicAdd(&diag_b[j], acc[jj]);
    }
  }
}

// ---- staging of the matrix-core kernels below: entries resolved up front, rows by LDS-DMA --------------------------------
// diag_first_layer_kernel above stages a chunk of entries, waits for it, computes, and starts over: per chunk one exposed
// round trip for the entries (row pointer -> column / value) and one for their rows.  The kernels below
// (a) resolve ALL entries of a slab up front, in parallel, into LDS (one chain per workgroup, not one per chunk);
// (b) copy the entries' rows global -> LDS by the DMA path (global_load_lds, no data registers) into a ring of NBUF slots,
//     NBUF - 1 chunks ahead of the products, behind counted s_waitcnt vmcnt -- every wave issues the same number of copies
//     per chunk (padding entries copy zeros) so that the count is a compile-time constant -- and one raw barrier per chunk.
__device__ __forceinline__ void lds_dma4(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, reinterpret_cast<__attribute__((address_space(3))) void*>(
                                            reinterpret_cast<uintptr_t>(lds_dst)), 4, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// all but the youngest `ahead` chunks' copies (NI instructions each) have landed; ahead <= MAXA (wave uniform)
template <int NI, int MAXA> __device__ __forceinline__ void wait_chunks(int ahead) {
  if constexpr (MAXA == 0) {
    wait_vmcnt<0>();
  } else {
    if (ahead >= MAXA) wait_vmcnt<MAXA * NI>();
    else wait_chunks<NI, MAXA - 1>(ahead);
  }
}

constexpr int kDiagMaxEntries = 512;  // entries resolved per pass (a slab of 64 Cora samples has ~380)

// ---- GCN: the per-sample outer products on the matrix cores ---------------------------------------------------------------
// T_n = sum_v P[n, v] act'(h_1[v]) (x) E[v] is a [64 hidden x 64 input] product with K = the sample's row length: with
// v_mfma_f32_32x32x2_f32 a pair of entries is one K step, lane l supplying A[j = l & 31][k = l >> 5] = act'(h_1[v_k, j]) and
// B[k][i = l & 31] = P[n, v_k] E[v_k, i] -- BOTH operands are one dword per lane straight from the staged rows; no operand
// is wave uniform, so no broadcast traffic (LDS b128 reads that all lanes address alike, scalar cache, v_readlane) exists.
// The earlier VALU kernel's counters at the Cora shape (profiles/r03_cora_sq_counters_valu.txt): 30 M VALU instructions
// for 5.6 M packed FMAs -- 11 M of them v_readlane -- 54 % VALU busy for 0.12 ms; here the VALU only folds a finished sample,
// acc += q[j] T[j, i]^2 on the accumulator layout, 64 packed instructions per sample.  Measured at the Cora shape
// (1 299 samples, 42 slabs x 6 column blocks = 252 workgroups): 0.067 ms against 0.131 ms for the round-2 kernel; by
// switching phases off (DESIGN.md has the table): prologue 8 us, entry resolution + operand reads 21 us, row copies 7 us,
// MFMAs 14 us, folds 8 us, the 64 float atomics per lane of the flush 15 us -- a latency chain of one wave per SIMD, not
// a throughput bound: shorter slabs overlap more workgroups per CU but multiply the atomics (5.6 us per million).
//   * a wave owns a 64 x 64 tile of (hidden, input) pairs: T and the running sum are 4 + 4 accumulator tiles (128 VGPRs);
//     the 4 waves of a workgroup share the slab's entry stream and the act' rows and take 4 adjacent column blocks;
//   * E = [P X | rowsum(P) | 0] is ONE padded matrix (the bias column sits in the first pad column: context.hip
//     build_px), so a row's 256-column block is one 16-byte-per-lane LDS-DMA copy;
//   * samples are padded to an even number of entries (weight 0) so that a K step never straddles two samples;
//   * entries resolved up front, rows through the NBUF-slot DMA ring with counted vmcnt waits (see above).
__device__ float g_diag_zero16[4] = {0.f, 0.f, 0.f, 0.f};
using f32x16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;

__device__ __forceinline__ void lds_dma16(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds(src, reinterpret_cast<__attribute__((address_space(3))) void*>(
                                            reinterpret_cast<uintptr_t>(lds_dst)), 16, 0, 0);
}

template <int DCH, int NBUF>
__global__ __launch_bounds__(256) void diag_first_layer_mfma_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
    const int64_t* __restrict__ idx, int64_t M, int64_t slab, const float* __restrict__ E, int64_t ldE, int64_t F, int64_t N,
    const float* __restrict__ dact, int64_t H, const float* __restrict__ q, float* __restrict__ diag_w,
    float* __restrict__ diag_b) {
  constexpr int ROW = 256 + 64;        // floats per staged entry: 256 columns of E, 64 hidden units of act'
  constexpr int BUF = DCH * ROW;       // floats per ring slot
  constexpr int NI = DCH / 2;          // DMA instructions per wave and chunk (DCH / 4 entries x 2 rows)
  constexpr int NP = DCH / 2;          // K steps (pairs of entries) per chunk
  constexpr int MAXE = kDiagMaxEntries;
  static_assert(NBUF >= 2 && (NBUF - 2) * NI <= 63 && DCH % 4 == 0 && MAXE % DCH == 0, "ring: vmcnt is a 6-bit counter");
  // ONE LDS object (hipcc drains vmcnt before reads of a second one):
  // ring | q rows of the slab [64][64] | entries {column, weight, pair record} | slab tables
  __shared__ float smem[NBUF * BUF + 64 * 64 + 3 * MAXE + 65 + 3 * 64 + 63];
  float* __restrict__ ring = smem;
  float* __restrict__ sq = smem + NBUF * BUF;
  int32_t* __restrict__ sv = reinterpret_cast<int32_t*>(sq + 64 * 64);
  float* __restrict__ sa = sq + 64 * 64 + MAXE;
  // record of the K step that starts at an even entry: sample | 256 (first step of its sample) | 512 (last); -1 past the end
  int32_t* __restrict__ sflag = reinterpret_cast<int32_t*>(sa + MAXE);
  int32_t* __restrict__ soff = sflag + MAXE;  // padded (even) entry offsets of the samples
  int32_t* __restrict__ snode = soff + 65;
  int32_t* __restrict__ sbase = snode + 64;
  int32_t* __restrict__ slen = sbase + 64;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t cblk = int64_t(blockIdx.x) * 256;   // the workgroup's 256 columns of E; wave w: cblk + 64 w .. + 63
  const int64_t j0 = int64_t(blockIdx.y) * 64;
  const int64_t m_begin = int64_t(blockIdx.z) * slab, m_end = min(M, m_begin + slab);
  const int ns = int(m_end - m_begin);  // <= 64
  if (tid < 64) {
    int32_t len = 0, node = -1, base = 0;
    if (tid < ns) {
      const int64_t n = idx[m_begin + tid];
      if (n >= 0 && n < N) { node = int32_t(n); base = rowptr[n]; len = rowptr[n + 1] - base; }
    }
    snode[tid] = node;
    sbase[tid] = base;
    slen[tid] = len;
    int32_t incl = (len + 1) & ~1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    soff[tid + 1] = incl;
    if (tid == 0) soff[0] = 0;
  }
  for (int f = tid; f < 64 * 64; f += 256) {  // q rows of the slab's samples (zero past the slab / past H)
    const int sidx = f >> 6, j = f & 63;
    sq[f] = (sidx < ns && j0 + j < H) ? q[(m_begin + sidx) * H + j0 + j] : 0.f;
  }
  __syncthreads();
  const int32_t etot = soff[64];
  f32x16 T[2][2], acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { T[a][b][r] = 0.f; acc[a][b][r] = 0.f; }
  // DMA sources of this lane: 4 columns of E (16 bytes), one hidden unit of act'
  const bool e_ok = cblk + 4 * lane < ldE, j_ok = j0 + lane < H;
  const float* __restrict__ esrc = E + cblk + 4 * lane;
  const float* __restrict__ dsrc = dact + j0 + lane;

  for (int32_t sb0 = 0; sb0 < etot; sb0 += MAXE) {
    const int ne = min(MAXE, int(etot - sb0));  // even
    const int nch = (ne + DCH - 1) / DCH;
    for (int e = tid; e < nch * DCH; e += 256) {  // every entry of this pass: sample by bisection, then column / value
      const int32_t g = sb0 + e;
      int32_t v = 0, fl = -1;
      float a = 0.f;
      if (e < ne) {
        int lo = 0, hi = ns;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= g) lo = mid; else hi = mid; }
        const int32_t r = g - soff[lo], len = slen[lo];
        v = snode[lo];  // (the padding entry of an odd row: weight 0)
        if (r < len) { const int32_t p = sbase[lo] + r; v = col[p]; a = val[p]; }
        fl = lo | (r == 0 ? 256 : 0) | (r + 2 >= len ? 512 : 0);
      }
      sv[e] = v; sa[e] = a; sflag[e] = fl;
    }
    __syncthreads();
    auto issue = [&](int c) {  // chunk c -> ring slot c % NBUF; wave w copies the rows of entries w, w + 4, ...
      float* __restrict__ slot = ring + (c % NBUF) * BUF;
#pragma unroll
      for (int k = 0; k < DCH / 4; ++k) {
        const int el = wave + 4 * k, e = c * DCH + el;
        const bool ok = e < ne;
        const int64_t v = sv[e];
        lds_dma16((ok && e_ok) ? esrc + v * ldE : g_diag_zero16, slot + el * ROW);
        lds_dma4((ok && j_ok) ? dsrc + v * H : g_diag_zero16, slot + el * ROW + 256);
      }
    };
    for (int c = 0; c < NBUF - 1 && c < nch; ++c) issue(c);
    for (int c = 0; c < nch; ++c) {
      wait_chunks<NI, NBUF - 2>(min(NBUF - 2, nch - 1 - c));  // chunks after c whose copies are in flight
      asm volatile("s_barrier" ::: "memory");  // chunk c has landed for all waves; chunk c - 1 is consumed
      if (c + NBUF - 1 < nch) issue(c + NBUF - 1);
      // the chunk's K steps: all operands on their way before the first product (one LDS round trip per chunk, not per step)
      const float* __restrict__ slot = ring + (c % NBUF) * BUF + lhi * ROW;  // this lane's K index: entry 2 p + lhi
      float A0[NP], A1[NP], B0[NP], B1[NP];
      int fl[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const float* __restrict__ row = slot + 2 * p * ROW;
        const float w = sa[c * DCH + 2 * p + lhi];
        A0[p] = row[256 + l31]; A1[p] = row[256 + 32 + l31];
        B0[p] = w * row[wave * 64 + l31]; B1[p] = w * row[wave * 64 + 32 + l31];
        fl[p] = __builtin_amdgcn_readfirstlane(sflag[c * DCH + 2 * p]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (fl[p] < 0) break;  // past the last entry
        if (fl[p] & 256) {     // a sample's first step starts from zero
          const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          T[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[p], B0[p], z, 0, 0, 0);
          T[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[p], B1[p], z, 0, 0, 0);
          T[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[p], B0[p], z, 0, 0, 0);
          T[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[p], B1[p], z, 0, 0, 0);
        } else {
          T[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[p], B0[p], T[0][0], 0, 0, 0);
          T[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[p], B1[p], T[0][1], 0, 0, 0);
          T[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[p], B0[p], T[1][0], 0, 0, 0);
          T[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[p], B1[p], T[1][1], 0, 0, 0);
        }
        if (fl[p] & 512) {  // the sample is complete: acc += q[j] T[j, i]^2
          // accumulator register r: j = 32 jt + 8 (r >> 2) + 4 lhi + (r & 3)
          const float* __restrict__ qs = sq + (fl[p] & 255) * 64 + 4 * lhi;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float qv = qs[32 * jt + 8 * (r >> 2) + (r & 3)];
#pragma unroll
              for (int it = 0; it < 2; ++it) acc[jt][it][r] = fmaf(qv * T[jt][it][r], T[jt][it][r], acc[jt][it][r]);
            }
        }
      }
    }
    __syncthreads();  // the next pass overwrites the entry table and the ring
  }
  // flush: accumulator register r of tile (jt, it) is (hidden j0 + 32 jt + 8 (r >> 2) + 4 lhi + (r & 3), column + 32 it + l31)
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int64_t i = cblk + wave * 64 + it * 32 + l31;
      if (i > F) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = j0 + 32 * jt + 8 * (r >> 2) + 4 * lhi + (r & 3);
        if (j < H) atomicAdd(i < F ? &diag_w[j * F + i] : &diag_b[j], acc[jt][it][r]);
      }
    }
}

// ---- GCN, wide inputs (Cora: F = 1 433): the same per-sample outer products, output tiles owned ------------------------------
// Round 3's kernel above cut the samples into 42 slabs and every workgroup flushed its [64 x 256] partial tile with float
// atomics: 35.9 MB through the fabric for a 0.37 MB result (97 x), E re-fetched by whichever XCD a workgroup landed on, and a
// per-workgroup latency chain (32 samples) that left the matrix pipes 12 % busy.  Here
//   * a workgroup (4 waves, one per SIMD) owns 192 columns x 64 hidden units for a LONG slab of samples (Cora: 8 column blocks x
//     32 slabs of 41 samples); wave (jh, ch) holds a 32 x 96 tile of T and of the running sum (3 + 3 accumulator tiles: one
//     A operand read feeds three MFMAs);
//   * blockIdx.x = column block + ncb * slab: with 8 column blocks the workgroups of a column block share an XCD (blocks are
//     dealt round-robin: speed only), so an XCD's L2 holds exactly its 192-column slice of E (2 MB) -- E crosses the fabric once;
//   * ONE 16-byte-per-lane LDS-DMA copy stages an entry: lanes 0 .. 47 its 192 columns of E, lanes 48 .. 63 the 64 act' values;
//   * sqrt(q) rides on the A operand (q = w^T Lambda w >= 0), so folding a finished sample is one FMA per accumulator register,
//     acc += T'^2 -- the fp32 MFMAs and the VALU share the SIMD's ALUs, every saved vector instruction is matrix time;
//   * the slab's partial tile goes to a workspace with PLAIN stores, every element written exactly once;
//     diag_tile_reduce_kernel adds the slabs up in a fixed order: no atomics, deterministic, 16 x 0.37 MB written.
constexpr int kTileCols = 192;
constexpr int kTileDch = 12;    // entries per ring chunk (two copies per wave)
constexpr int kTileNbuf = 4;
constexpr int kTileSlabMax = 96;
constexpr int kTileMaxE = 768;  // entries resolved per pass

__global__ __launch_bounds__(256) void diag_first_layer_tile_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
    const int64_t* __restrict__ idx, int64_t M, int64_t slab, int ncb, const float* __restrict__ E, int64_t ldE, int64_t F,
    int64_t N, const float* __restrict__ dact, int64_t H, const float* __restrict__ q, float* __restrict__ part,
    int64_t part_ld) {
  constexpr int DCH = kTileDch, NBUF = kTileNbuf, ROW = 256, BUF = DCH * ROW, NI = DCH / 4, NP = DCH / 2, MAXE = kTileMaxE;
  constexpr int SM = kTileSlabMax;
  static_assert((NBUF - 2) * NI <= 63 && DCH % 4 == 0 && MAXE % DCH == 0, "ring");
  // ONE LDS object: ring | sqrt(q) rows of the slab [SM][64] | entries {column, weight, pair record} | slab tables
  __shared__ __attribute__((aligned(16))) float smem[NBUF * BUF + SM * 64 + 3 * MAXE + (SM + 1) + 3 * SM];
  float* __restrict__ ring = smem;
  float* __restrict__ sq = smem + NBUF * BUF;
  int32_t* __restrict__ sv = reinterpret_cast<int32_t*>(sq + SM * 64);
  float* __restrict__ sa = sq + SM * 64 + MAXE;
  // record of the K step that starts at an even entry: sample | 256 (first step of its sample) | 512 (last); -1 past the end
  int32_t* __restrict__ sflag = reinterpret_cast<int32_t*>(sa + MAXE);
  int32_t* __restrict__ soff = sflag + MAXE;  // padded (even) entry offsets of the samples
  int32_t* __restrict__ snode = soff + SM + 1;
  int32_t* __restrict__ sbase = snode + SM;
  int32_t* __restrict__ slen = sbase + SM;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jh = wave >> 1, ch = wave & 1;  // hidden half, column half (96 columns = three 32-column MFMA tiles)
  const int cb = int(blockIdx.x) % ncb, slab_i = int(blockIdx.x) / ncb;
  const int64_t cblk = int64_t(cb) * kTileCols;
  const int64_t j0 = int64_t(blockIdx.y) * 64;
  const int64_t m_begin = int64_t(slab_i) * slab, m_end = min(M, m_begin + slab);
  const int ns = int(m_end - m_begin);  // <= SM
  if (tid < 64) {  // exclusive prefix sums of the padded row lengths, two samples per lane (SM <= 128)
    int32_t len2[2], incl = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int sidx = 2 * tid + u;
      int32_t len = 0, node = -1, base = 0;
      if (sidx < ns) {
        const int64_t n = idx[m_begin + sidx];
        if (n >= 0 && n < N) { node = int32_t(n); base = rowptr[n]; len = rowptr[n + 1] - base; }
      }
      if (sidx < SM) { snode[sidx] = node; sbase[sidx] = base; slen[sidx] = len; }
      len2[u] = (len + 1) & ~1;
      incl += len2[u];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (2 * tid + 1 <= SM) soff[2 * tid + 1] = incl - len2[1];
    if (2 * tid + 2 <= SM) soff[2 * tid + 2] = incl;
    if (tid == 0) soff[0] = 0;
  }
  for (int f = tid; f < SM * 64; f += 256) {  // sqrt(q) rows of the slab's samples (zero past the slab / past H)
    const int sidx = f >> 6, j = f & 63;
    sq[f] = (sidx < ns && j0 + j < H) ? sqrtf(fmaxf(q[(m_begin + sidx) * H + j0 + j], 0.f)) : 0.f;
  }
  __syncthreads();
  const int32_t etot = soff[min(ns, SM)];
  f32x16 T[3], acc[3];
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) { T[b][r] = 0.f; acc[b][r] = 0.f; }
  // DMA source of this lane: lanes 0 .. 47 four columns of E, lanes 48 .. 63 four hidden units of act'
  const bool is_e = lane < 48;
  const int64_t ecol = cblk + 4 * lane, dcol = j0 + 4 * (lane - 48);
  const bool src_ok = is_e ? ecol < ldE : dcol < H;
  const float* __restrict__ src0 = is_e ? E + ecol : dact + dcol;
  const int64_t src_ld = is_e ? ldE : H;

  for (int32_t sb0 = 0; sb0 < etot; sb0 += MAXE) {
    const int ne = min(MAXE, int(etot - sb0));  // even
    const int nch = (ne + DCH - 1) / DCH;
    for (int e = tid; e < nch * DCH; e += 256) {  // every entry of this pass: sample by bisection, then column / value
      const int32_t g = sb0 + e;
      int32_t v = 0, fl = -1;
      float a = 0.f;
      if (e < ne) {
        int lo = 0, hi = ns;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= g) lo = mid; else hi = mid; }
        const int32_t r = g - soff[lo], len = slen[lo];
        v = max(snode[lo], 0);  // (the padding entry of an odd row: weight 0)
        if (r < len) { const int32_t p = sbase[lo] + r; v = col[p]; a = val[p]; }
        fl = lo | (r == 0 ? 256 : 0) | (r + 2 >= len ? 512 : 0);
      }
      sv[e] = v; sa[e] = a; sflag[e] = fl;
    }
    __syncthreads();
    auto issue = [&](int c) {  // chunk c -> ring slot c % NBUF; wave w copies the rows of entries w, w + 4, w + 8
      float* __restrict__ slot = ring + (c % NBUF) * BUF;
#pragma unroll
      for (int k = 0; k < DCH / 4; ++k) {
        const int el = wave + 4 * k, e = c * DCH + el;
        const int64_t v = sv[e];
        lds_dma16((e < ne && src_ok) ? src0 + v * src_ld : g_diag_zero16, slot + el * ROW);
      }
    };
    for (int c = 0; c < NBUF - 1 && c < nch; ++c) issue(c);
    for (int c = 0; c < nch; ++c) {
      wait_chunks<NI, NBUF - 2>(min(NBUF - 2, nch - 1 - c));  // chunks after c whose copies are in flight
      asm volatile("s_barrier" ::: "memory");  // chunk c has landed for all waves; chunk c - 1 is consumed
      if (c + NBUF - 1 < nch) issue(c + NBUF - 1);
      const float* __restrict__ slot = ring + (c % NBUF) * BUF + lhi * ROW;  // this lane's K index: entry 2 p + lhi
      float A[NP], B0[NP], B1[NP], B2[NP];
      int fl[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const float* __restrict__ row = slot + 2 * p * ROW;
        fl[p] = __builtin_amdgcn_readfirstlane(sflag[c * DCH + 2 * p]);
        const float sqv = sq[(max(fl[p], 0) & 255) * 64 + 32 * jh + l31];
        A[p] = sa[c * DCH + 2 * p + lhi] * sqv * row[kTileCols + 32 * jh + l31];
        B0[p] = row[ch * 96 + l31]; B1[p] = row[ch * 96 + 32 + l31]; B2[p] = row[ch * 96 + 64 + l31];
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        // (steps past the last entry carry weight 0: they add nothing and need no branch)
        T[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[p], B0[p], T[0], 0, 0, 0);
        T[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[p], B1[p], T[1], 0, 0, 0);
        T[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[p], B2[p], T[2], 0, 0, 0);
        if (fl[p] >= 0 && (fl[p] & 512)) {  // the sample is complete: acc += (sqrt(q_j) T[j, i])^2, T = 0 for the next one
          // A REAL branch (the empty statement keeps hipcc from if-converting it): left to itself it folds on EVERY K step
          // behind 32 v_cndmask and picks the first step's zero accumulator with 32 more -- ~100 vector instructions per
          // K step on the ALUs the fp32 MFMAs run on, which is what round 3's kernel spent its 67 us on.
          asm volatile("" ::: "memory");
#pragma unroll
          for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[b][r] = fmaf(T[b][r], T[b][r], acc[b][r]); T[b][r] = 0.f; }
        }
      }
    }
    __syncthreads();  // the next pass overwrites the entry table and the ring
  }
  // the slab's partial tile: accumulator register r of tile b is (hidden j0 + 32 jh + 8 (r >> 2) + 4 lhi + (r & 3), column + 32 b + l31)
  float* __restrict__ pt = part + int64_t(slab_i) * H * part_ld;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int64_t i = cblk + ch * 96 + b * 32 + l31;
    if (i > F) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t j = j0 + 32 * jh + 8 * (r >> 2) + 4 * lhi + (r & 3);
      if (j < H) pt[j * part_ld + i] = acc[b][r];
    }
  }
}
// diag(W_0)[j, i] += sum_slabs part[slab][j][i] (i < F), diag(b_0)[j] += ... (i == F): a fixed summation order.  Thread t of
// linear block `blk` owns four consecutive columns of one hidden unit (part_ld % 4 == 0: 16-byte reads).  Runs as extra
// z-slices of the last-layer launch (TileReduce below): no launch of its own, and it overlaps that latency-bound kernel.
struct TileReduce {
  const float* part; int64_t part_ld; int nslab; int64_t H, F; float* diag_w; float* diag_b;
  int z0;  // first z-slice of the launch that reduces (z0 < 0: nothing to reduce)
};
__device__ __forceinline__ void diag_tile_reduce(const TileReduce& a, int64_t blk) {
  const int64_t q4 = (a.F + 4) / 4;  // groups of four columns covering 0 .. F
  const int64_t t = blk * 256 + threadIdx.x;
  if (t >= a.H * q4) return;
  const int64_t j = t / q4, i = 4 * (t - j * q4);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < a.nslab; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(a.part + (int64_t(s) * a.H + j) * a.part_ld + i);
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  const float e[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (i + u < a.F) a.diag_w[j * a.F + i + u] += e[u];
    else if (i + u == a.F) a.diag_b[j] += e[u];
  }
}

// grid (i-chunks of 256, C, slabs): diag(W)[k,i] += sum_n wgt[n,k] phi[n,i]^2 ; bias with s_n.
// wgt = p_k (1 - p_k) from the probabilities (GGN), or the caller's [M, C] array (empirical Fisher: scale * r_k^2)
__global__ void diag_last_layer_kernel(const float* __restrict__ probs, const int64_t* __restrict__ idx, int64_t M,
                                       int64_t C, int64_t slab, FeatView Phi, float* __restrict__ diag_w,
                                       float* __restrict__ diag_b, const float* __restrict__ wgt, TileReduce red) {
  if (red.z0 >= 0 && int(blockIdx.z) >= red.z0) {  // the first layer's partial tiles (diag_first_layer_tile_kernel)
    diag_tile_reduce(red, blockIdx.x + int64_t(gridDim.x) * (blockIdx.y + int64_t(gridDim.y) * (blockIdx.z - red.z0)));
    return;
  }
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (i > Phi.width) return;
  const int64_t m_begin = int64_t(blockIdx.z) * slab, m_end = min(M, m_begin + slab);
  float acc = 0.f;
  // four samples per step: their ids first, then the (dependent) feature loads together -- one latency chain per four samples
  for (int64_t m = m_begin; m < m_end; m += 4) {
    int64_t n[4];
    float wt[4], ph[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) n[u] = m + u < m_end ? idx[m + u] : -1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t mm = min(m + u, m_end - 1);
      const float p = wgt ? wgt[mm * C + k] : probs[mm * C + k];
      wt[u] = wgt ? p : p * (1.f - p);
      ph[u] = feat(Phi, n[u], i);  // id -1 (past the slab) or out of range: 0
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += wt[u] * ph[u] * ph[u];
  }
  if (i < Phi.width) atomicAdd(&diag_w[k * Phi.width + i], acc);
  else atomicAdd(&diag_b[k], acc);
}

// Generic depth: diag[p] += sum_m sum_{c,k} J[m,c,p] Lambda_m[c,k] J[m,k,p] from a chunk of explicit Jacobians
// J [mc, C, P] (jacobian.hip); Lambda_m = diag(p_m) - p_m p_m^T (laplace/curvature/curvature.py:365-372, 428), so
// per sample: sum_c p_c t_c^2 - (sum_c p_c t_c)^2 with t_c = J[m,c,p].  regression (H_lik = None, :429-430): sum_c t_c^2.
__global__ __launch_bounds__(256) void diag_from_jac_kernel(const float* __restrict__ J, const float* __restrict__ probs,
                                                            int64_t mc, int64_t C, int64_t P, int regression,
                                                            float* __restrict__ diag) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t m_begin = int64_t(blockIdx.y) * 8, m_end = min(mc, m_begin + 8);
  float acc = 0.f;
  for (int64_t m = m_begin; m < m_end; ++m) {
    const float* __restrict__ Jm = J + m * C * P + p;
    float s2 = 0.f, s1 = 0.f;
    for (int64_t c = 0; c < C; ++c) {
      const float t = Jm[c * P];
      const float pc = regression ? 1.f : probs[m * C + c];
      s2 += pc * t * t;
      s1 += pc * t;
    }
    acc += regression ? s2 : s2 - s1 * s1;
  }
  atomicAdd(&diag[p], acc);
}

int diag_from_jacobians(lgnn_ctx* h, const int64_t* idx, int64_t M, float* diag_out, hipStream_t s) {
  const int64_t C = h->dims[h->L], P = h->n_params;
  // chunk of samples whose Jacobians [mc, C, P] take at most a quarter of the workspace cap (the planes of
  // jacobian.hip are chunked against the cap by themselves)
  const int64_t mc_max = std::max<int64_t>(1, std::min<int64_t>(M, (h->ws_limit / 4) / std::max<int64_t>(C * P * 4, 1)));
  LGNN_CALL(h->ws.jac.reserve(size_t(mc_max) * C * P * 4));
  float* J = h->ws.jac.as<float>();
  for (int64_t m0 = 0; m0 < M; m0 += mc_max) {
    const int64_t mc = std::min(mc_max, M - m0);
    LGNN_CALL(jacobians(h, idx + m0, mc, J, nullptr, s));
    hipLaunchKernelGGL(diag_from_jac_kernel, dim3(unsigned(cdiv(P, 256)), unsigned(cdiv(mc, 8))), dim3(256), 0, s, J,
                       h->ws.probs.as<float>() + m0 * C, mc, C, P, h->lik == LGNN_LIK_REGRESSION ? 1 : 0, diag_out);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

const TileReduce kNoReduce{nullptr, 0, 0, 0, 0, nullptr, nullptr, -1};

// LGNN_DIAG_SLAB: samples per workgroup slab, clamped to [1, cap]; unset: the launch's own choice
int64_t slab_or_env(int64_t chosen, int64_t cap) {
  if (const char* e = getenv("LGNN_DIAG_SLAB")) return std::max<int64_t>(1, std::min<int64_t>(cap, atoll(e)));
  return chosen;
}
// LGNN_DIAG_STAGED forces the register-staged first-layer kernel for GCN too (tests compare the two)
bool staged_forced() { return getenv("LGNN_DIAG_STAGED") != nullptr; }

// GCN, narrow inputs: diag_first_layer_mfma_kernel, partial tiles flushed with float atomics
int launch_first_layer_mfma(lgnn_ctx* h, const FeatView& E, const int64_t* idx, int64_t M, const float* q, float* diag_out,
                            hipStream_t s) {
  const int64_t H = h->dims[1], in0 = h->in_dim[0];
  const unsigned gx = unsigned(cdiv(E.width + 1, 256)), gy = unsigned(cdiv(H, 64));
  const int64_t sl = slab_or_env(std::max<int64_t>(4, std::min<int64_t>(64, cdiv(M * gx * gy, 512))), 64);
  hipLaunchKernelGGL((diag_first_layer_mfma_kernel<8, 3>), dim3(gx, gy, unsigned(cdiv(M, sl))), dim3(256), 0, s,
                     h->P.rowptr, h->P.col, h->P.val, idx, M, sl, E.base, E.ld, E.width, h->N,
                     h->fc.dact0.as<float>(), H, q, diag_out, diag_out + H * in0);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// GCN, wide inputs (ncb >= 4 column blocks): owned output tiles, long slabs, plain-store partials in ws.jac; `red` names them
// for the fixed-order reduction that rides on the last-layer launch (no atomics)
int launch_first_layer_tile(lgnn_ctx* h, const FeatView& E, int64_t ncb, const int64_t* idx, int64_t M, const float* q,
                            float* diag_out, hipStream_t s, TileReduce& red) {
  const int64_t H = h->dims[1], in0 = h->in_dim[0];
  const int64_t gyt = cdiv(H, 64);
  int64_t nsl = std::max<int64_t>(1, std::min<int64_t>(cdiv(256, ncb * gyt), cdiv(M, 16)));  // ~ one workgroup per CU
  const int64_t sl = slab_or_env(std::min<int64_t>(kTileSlabMax, cdiv(M, nsl)), kTileSlabMax);
  nsl = cdiv(M, sl);
  const int64_t part_ld = ncb * kTileCols;
  LGNN_CALL(h->ws.jac.reserve(size_t(nsl) * H * part_ld * 4));
  float* part = h->ws.jac.as<float>();
  hipLaunchKernelGGL(diag_first_layer_tile_kernel, dim3(unsigned(ncb * nsl), unsigned(gyt)), dim3(256), 0, s,
                     h->P.rowptr, h->P.col, h->P.val, idx, M, sl, int(ncb), E.base, E.ld, E.width, h->N,
                     h->fc.dact0.as<float>(), H, q, part, part_ld);
  LGNN_HIP_CHECK(hipGetLastError());
  red = TileReduce{part, part_ld, int(nsl), H, E.width, diag_out, diag_out + H * in0, 0};
  return 0;
}

// diag_last_layer_kernel; a pending tile reduction (red.z0 >= 0) becomes extra z-slices of the launch
int launch_last_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, const float* wgt, float* out, TileReduce red,
                      hipStream_t s) {
  const int64_t C = h->dims[h->L];
  FeatView Phi;
  feat_views(h, h->L - 1, Phi);
  dim3 grid{unsigned(cdiv(Phi.width + 1, 256)), unsigned(C), unsigned(cdiv(M, slab))};
  if (red.z0 >= 0) {
    red.z0 = int(grid.z);
    const int64_t blocks = cdiv(red.H * ((red.F + 4) / 4), 256);
    grid.z += unsigned(cdiv(blocks, int64_t(grid.x) * grid.y));
  }
  hipLaunchKernelGGL(diag_last_layer_kernel, grid, dim3(256), 0, s, h->ws.probs.as<float>(), idx, M, C, slab, Phi, out,
                     out + C * Phi.width, wgt, red);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// The first layer of a 2-layer model: the matrix-core kernels for GCN, the register-staged kernel for GraphSAGE (its self path
// needs three q rows and the node's own rows per closing entry) and under LGNN_DIAG_STAGED.  off: where the last layer's
// block starts in diag_out; red: the tile kernel's partials, still to be added up.
int first_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, bool staged, const float* q, float* diag_out,
                hipStream_t s, TileReduce& red, int64_t& off) {
  red = kNoReduce;
  off = 0;
  if (h->L != 2) return 0;
  if (h->timing) LGNN_CALL(record_event(h, s));  // dominant kernel of the diagonal path (bench.py roofline)
  if (staged) {
    LGNN_CALL(launch_diag_first_layer_staged(h, idx, M, slab, q, diag_out, s));
  } else {
    // GCN: E = [P X | rowsum(P) | 0] is one padded matrix (context.hip build_px)
    FeatView E;
    feat_views(h, 0, E);
    LGNN_REQUIRE(E.ld >= E.width + 1 && E.ld % 4 == 0, "internal: P X without its bias column");
    const int64_t ncb = cdiv(E.width + 1, kTileCols);
    if (ncb >= 4 && h->dims[1] % 4 == 0) LGNN_CALL(launch_first_layer_tile(h, E, ncb, idx, M, q, diag_out, s, red));
    else LGNN_CALL(launch_first_layer_mfma(h, E, idx, M, q, diag_out, s));
  }
  if (h->timing) { LGNN_CALL(record_event(h, s)); h->ev_planes += M; }
  off = h->dims[1] * h->in_dim[0] + h->dims[1];
  return 0;
}

}  // namespace

// Samples per workgroup slab of the staged first-layer and the last-layer kernel.  A thread walks its slab's samples and
// their neighbours one after the other (dependent loads: a latency chain), so small problems want short slabs -- Cora shape:
// 0.42 -> 0.2 ms with 16 instead of 64 -- while every slab costs one atomic per output element: aim for `target` workgroups.
// (measured at the Cora shape: 1 024 - 2 048 workgroups are the optimum -- fewer lengthen the per-workgroup chain,
//  more multiply the float atomics of the flush: 0.13 ms at 2 048, 0.26 ms at 8 192)
int64_t diag_slab(const lgnn_ctx* h, int64_t M, int64_t target) {
  int64_t tiles = 1;
  if (h->L == 2) tiles = cdiv(h->in_dim[0] + 1, 64) * cdiv(h->dims[1], 64);
  return std::max<int64_t>(8, std::min<int64_t>(64, cdiv(M * tiles, target)));
}

int launch_diag_first_layer_staged(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, const float* q, float* diag_out,
                                   hipStream_t s) {
  const int64_t H = h->dims[1], in0 = h->in_dim[0];
  FeatView E;
  feat_views(h, 0, E);
  const dim3 grid{unsigned(cdiv(E.width + 1, 64)), unsigned(cdiv(H, 64)), unsigned(cdiv(M, slab))};
  if (h->kind == LGNN_KIND_SAGE)
    hipLaunchKernelGGL(diag_first_layer_kernel<1>, grid, dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.val, idx, M, slab, E,
                       h->fc.dact0.as<float>(), H, q, diag_out, diag_out + H * in0);
  else
    hipLaunchKernelGGL(diag_first_layer_kernel<0>, grid, dim3(256), 0, s, h->P.rowptr, h->P.col, h->P.val, idx, M, slab, E,
                       h->fc.dact0.as<float>(), H, q, diag_out, diag_out + H * in0);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_diag_last_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, const float* wgt, float* out,
                           hipStream_t s) {
  return launch_last_layer(h, idx, M, slab, wgt, out, kNoReduce, s);
}

int diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags, float* diag_out,
                    float* loss_out, hipStream_t s) {
  (void)flags;
  LGNN_REQUIRE(M > 0 && idx && y && diag_out && loss_out, "empty batch or null pointers");
  LGNN_REQUIRE(h->L >= 1, "no model bound");
  const int L = h->L;
  const int64_t C = h->dims[L];
  const bool regression = h->lik == LGNN_LIK_REGRESSION;
  if (!closed_form_model(h) || getenv("LGNN_JAC_PLANES") != nullptr) {
    // deeper models (the reference builds them once the breakpoint at gnn/models/base_gnn.py:109 is removed): per-sample
    // Jacobians in chunks + the contraction with Lambda; no closed form
    LGNN_CALL(forward_ensure(h, s));
    LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
    LGNN_CALL(diag_from_jacobians(h, idx, M, diag_out, s));
    LGNN_CALL(batch_epilogue(h, idx, M, s));
    return 0;
  }
  LGNN_CALL(forward_ensure_aux(h, s));
  // classification: probabilities, loss, q and the id / label checks in ONE launch (diag_prologue_kernel); regression
  // (Lambda = I, no probabilities) keeps the shared prologue
  const bool light = !regression;
  if (!light) LGNN_CALL(batch_prologue(h, idx, y, M, false, false, loss_out, s));
  const bool staged = staged_forced() || h->kind == LGNN_KIND_SAGE;
  // the matrix-core kernels size their own slabs; behind them the last-layer kernel takes longer slabs, fewer atomics
  // (~768 workgroups, three per CU)
  const int64_t slab = slab_or_env(diag_slab(h, M, staged ? 2048 : 768), 64);

  const int64_t H = L == 2 ? h->dims[1] : 0;
  const int has_self = h->kind == LGNN_KIND_SAGE ? 1 : 0;
  LGNN_CALL(h->ws.misc.reserve(size_t(3) * M * H * 4 + size_t(M) * C * 4));
  float* q = h->ws.misc.as<float>();
  if (light) {
    LGNN_CALL(h->ws.probs.reserve(size_t(M) * C * 4));
    LGNN_REQUIRE(4 * C * 4 <= 60 * 1024, "too many classes for the prologue kernel");
    hipLaunchKernelGGL(diag_prologue_kernel, dim3(unsigned(std::min<int64_t>(cdiv(M, 4), 4096))), dim3(256),
                       size_t(4 * C) * 4, s, h->fc.out.as<float>(), C, idx, static_cast<const int64_t*>(y), M, h->N,
                       L == 2 ? h->W[1] : nullptr, L == 2 ? h->in_dim[1] : 0, H, int64_t(0), has_self ? H : int64_t(0),
                       has_self, h->ws.probs.as<float>(), q, loss_out, h->ws.flags.as<int>());
    LGNN_HIP_CHECK(hipGetLastError());
  } else if (L == 2) {
    // regression: Lambda = I, i.e. q = sum_k w_kj^2 and unit weights in the last layer (the interface's factor is the caller's)
    hipLaunchKernelGGL(q_kernel, dim3(unsigned(cdiv(M * H, 256))), dim3(256), 0, s, static_cast<const float*>(nullptr), M, C,
                       h->W[1], h->in_dim[1], H, int64_t(0), has_self ? H : int64_t(0), has_self, q);
  }
  TileReduce red;
  int64_t off;
  LGNN_CALL(first_layer(h, idx, M, slab, staged, q, diag_out, s, red, off));
  const float* wgt = nullptr;
  if (regression) {
    float* ones = q + 3 * M * H;
    LGNN_CALL(launch_fill_i32(reinterpret_cast<int32_t*>(ones), M * C, 0x3f800000, s));  // 1.0f
    wgt = ones;
  }
  LGNN_CALL(launch_last_layer(h, idx, M, slab, wgt, diag_out + off, red, s));
  if (!light) LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn
