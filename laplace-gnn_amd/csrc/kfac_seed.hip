// The start and the end of every batch -- KFAC, diagonal, last layer, adjacency gradient, predictive: mark the batch nodes
// (pos[n] = first place of node n in the batch), softmax / loss / multiplicities and, where a route reads them from memory,
// the C x C seed blocks V of the loss-Hessian square root (kfac.hip's header has the chain they start); unmark at the end.
#include "kfac.h"

namespace lgnn {

namespace {

// guard (optional): the ids a batch-structure cache entry was built from.  A difference means the batch's memory was changed
// behind the caller's version counter: sticky flag word 3 (the cached lists would give a wrong factor without any sign)
__global__ void mark_batch_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int32_t* __restrict__ pos,
                                  int* __restrict__ bad, const int64_t* __restrict__ guard) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t n = idx[m];
  if (guard && guard[m] != n) bad[3] = 1;
  if (n < 0 || n >= N) { bad[1] = 1; return; }  // sticky flag word 1: node id out of range
  atomicMin(&pos[n], int32_t(m));  // duplicates: the first occurrence owns the accumulated seed row
}
__global__ void unmark_batch_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int32_t* __restrict__ pos) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t n = idx[m];
  if (n >= 0 && n < N) pos[n] = INT32_MAX;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// One wave per sample.  f = logits[idx[m]], p = softmax(f), mbar = sum_k p_k f_k.
//   fork exact : V[k,c] = sqrt(p_c) [d_kc - p_k (1 + f_k - mbar) + 1/2 (d_kc - p_k)(f_c - mbar)]
//   upstream   : V[k,c] = sqrt(p_c) (d_kc - p_k)                       (kfac_utils.py:122-126)
// written as seeds[first][c][k] (+=: duplicated node ids accumulate like x[x_indices]' backward).
// loss += logsumexp(f) - f[y]   (CrossEntropyLoss(reduction='sum'))
// seed modes: 0 upstream, 1 fork exact, 2 regression (sqrt(2) I), and the single-column "gradient" seeds of the empirical
// / Monte-Carlo Fisher (curvlinops/kfac.py:663-674: ONE backward pass of the loss itself): 3 classification
// V[k, 0] = rs (p_k - [k == y_seed]), 4 regression V[k, 0] = rs (f_k - y_seed_k); columns c > 0 stay zero.
__global__ __launch_bounds__(256) void seed_kernel(const float* __restrict__ logits, int64_t C,
                                                   const int64_t* __restrict__ idx, const void* __restrict__ y_,
                                                   int64_t M, int64_t N, const int32_t* __restrict__ pos, int fork_exact,
                                                   float* __restrict__ seeds, float* __restrict__ probs,
                                                   float* __restrict__ loss, int* __restrict__ bad,
                                                   int32_t* __restrict__ mult, const void* __restrict__ yseed_,
                                                   float resid_scale) {
  extern __shared__ float sm[];
  __shared__ float loss_part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* f_s = sm + size_t(wave) * 2 * C;
  float* p_s = f_s + C;
  float loss_acc = 0.f;  // lane 0: this wave's share of the batch loss (one atomic per workgroup, not per sample)
  for (int64_t m = int64_t(blockIdx.x) * 4 + wave; m < M; m += int64_t(gridDim.x) * 4) {
    const int64_t n = idx[m];
    if (n < 0 || n >= N) continue;  // flagged by mark_batch_kernel
    float mx = -INFINITY;
    for (int64_t k = lane; k < C; k += 64) {
      const float v = logits[n * C + k];
      f_s[k] = v;
      mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    float se = 0.f;
    for (int64_t k = lane; k < C; k += 64) {
      const float e = expf(f_s[k] - mx);
      p_s[k] = e;
      se += e;
    }
    se = wave_sum(se);
    const float inv = 1.0f / se;
    float mb = 0.f;
    for (int64_t k = lane; k < C; k += 64) {
      const float p = p_s[k] * inv;
      p_s[k] = p;
      if (probs) probs[m * C + k] = p;
      mb += p * f_s[k];
    }
    mb = wave_sum(mb);
    // f_s / p_s are read across lanes below: same wave, LDS executes a wave's operations in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (fork_exact == 2 || fork_exact == 4) {
      // regression: sum_k (f_k - y_k)^2 with float targets [M, C] (MSELoss(reduction='sum'); the factor 0.5 of the
      // interface is applied by the caller)
      if (loss) {
        const float* __restrict__ yr = static_cast<const float*>(y_) + m * C;
        float sq = 0.f;
        for (int64_t k = lane; k < C; k += 64) { const float dlt = f_s[k] - yr[k]; sq += dlt * dlt; }
        sq = wave_sum(sq);
        if (lane == 0) loss_acc += sq;
      }
    } else if (lane == 0 && loss) {
      const int64_t yy = static_cast<const int64_t*>(y_)[m];
      if (yy < 0 || yy >= C) *bad = 2;
      else loss_acc += logf(se) + mx - f_s[yy];
    }
    if (lane == 0 && mult) atomicAdd(&mult[pos[n]], 1);  // how often the node occurs in the batch, kept at its first place
    if (seeds && fork_exact >= 3) {
      float* __restrict__ dst = seeds + int64_t(pos[n]) * C * C;  // row c = 0 of the block
      if (fork_exact == 3) {
        const int64_t ys = static_cast<const int64_t*>(yseed_)[m];
        if (ys < 0 || ys >= C) { if (lane == 0) *bad = 2; }
        else for (int64_t k = lane; k < C; k += 64) atomicAdd(&dst[k], resid_scale * (p_s[k] - (k == ys ? 1.f : 0.f)));
      } else {
        const float* __restrict__ yr = static_cast<const float*>(yseed_) + m * C;
        for (int64_t k = lane; k < C; k += 64) atomicAdd(&dst[k], resid_scale * (f_s[k] - yr[k]));
      }
    } else if (seeds) {
      const int64_t first = pos[n];
      float* __restrict__ dst = seeds + first * C * C;
      const int64_t CC = C * C;
      for (int64_t q = lane; q < CC; q += 64) {
        const int64_t c = q / C, k = q - c * C;
        const float pc = p_s[c], pk = p_s[k];
        const float d = (k == c) ? 1.f : 0.f;
        float v;
        if (fork_exact == 2) v = d * 1.41421356237309515f;  // regression: Hessian square root sqrt(2) I (kfac_utils.py:116-120)
        else if (fork_exact) v = sqrtf(pc) * (d - pk * (1.f + f_s[k] - mb) + 0.5f * (d - pk) * (f_s[c] - mb));
        else v = sqrtf(pc) * (d - pk);
        atomicAdd(&dst[q], v);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the next sample overwrites f_s / p_s
  }
  if (loss) {
    if (lane == 0) loss_part[wave] = loss_acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (loss_part[0] + loss_part[1]) + (loss_part[2] + loss_part[3]));
  }
}

}  // namespace

// shared by kfac / diag / last layer: mark the batch, compute seeds/probs/loss.
int batch_prologue(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool want_seeds, bool fork_exact,
                   float* loss_out, hipStream_t s, const void* y_seed, float resid_scale, const int64_t* guard_ids) {
  const int64_t N = h->N, C = h->dims[h->L];
  // y_seed != null: single-column gradient seeds of the empirical / MC Fisher (labels resp. fp32 targets to seed with)
  const int seed_mode = y_seed ? (h->lik == LGNN_LIK_REGRESSION ? 4 : 3)
                               : (h->lik == LGNN_LIK_REGRESSION ? 2 : (fork_exact ? 1 : 0));
  LGNN_REQUIRE(2 * C * 4 <= 64 * 1024, "too many classes for the seed kernel");
  int* bad = h->ws.flags.as<int>();  // allocated and zeroed by lgnn_create; sticky until lgnn_check_async_errors
  hipLaunchKernelGGL(mark_batch_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, N,
                     h->ws.pos.as<int32_t>(), bad, guard_ids);
  LGNN_CALL(h->ws.probs.reserve(size_t(M) * C * 4));
  LGNN_CALL(h->ws.mult.reserve(size_t(M) * 4));
  LGNN_HIP_CHECK(hipMemsetAsync(h->ws.mult.p, 0, size_t(M) * 4, s));
  float* seeds = nullptr;
  if (want_seeds) {
    LGNN_CALL(h->ws.seeds.reserve(size_t(M) * C * C * 4));
    LGNN_HIP_CHECK(hipMemsetAsync(h->ws.seeds.p, 0, size_t(M) * C * C * 4, s));
    seeds = h->ws.seeds.as<float>();
  }
  LGNN_REQUIRE(8 * C * 4 <= 60 * 1024, "too many classes for the seed kernel");
  hipLaunchKernelGGL(seed_kernel, dim3(unsigned(std::min<int64_t>(cdiv(M, 4), 2048))), dim3(256), size_t(8 * C) * 4, s,
                     h->fc.out.as<float>(), C, idx,
                     y, M, N, h->ws.pos.as<int32_t>(), seed_mode, seeds,
                     h->ws.probs.as<float>(), loss_out, bad, h->ws.mult.as<int32_t>(), y_seed, resid_scale);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

int batch_epilogue(lgnn_ctx* h, const int64_t* idx, int64_t M, hipStream_t s) {
  hipLaunchKernelGGL(unmark_batch_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, h->N,
                     h->ws.pos.as<int32_t>());
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lgnn
