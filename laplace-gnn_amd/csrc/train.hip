// Training-mode forward with dropout and the backward to every trainable parameter (lgnn_train_forward / lgnn_train_backward).
//
// The reference trains its weights with autograd on the dense N x N model (gnn/marglik_training.py:165-186:
// f = model(train_indices); loss.backward(); optimizer.step()).  Here one forward call writes a tape into buffers of its own
// (TrainState: the inputs of every nn.Linear, the LayerNorm's normalised rows and 1 / sigma; the keep-masks are the caller's),
// and one backward call walks the layers top down:
//
//   hidden layer l < L-1:  s = res_l(x) + conv_l(P, x);  y = LayerNorm(s);  a = act(y);  x' = a * mask * scale
//   GCN        conv(P, x) = P (x W^T + 1 b^T):   T = P^T d;  dW = T^T x;  db = colsum(T);  dx = T W        (+ d Wr for res)
//   GraphSAGE  conv(P, x) = [x | P x] W^T + b:   dW = d^T cat;  db = colsum(d);  dcat = d W;  dx = dcat_1 + P^T dcat_2
//
// Kernels of this file: train_epilogue_kernel (bias of the cached P X route, res, LayerNorm, activation, dropout; writes
// the tape), train_back_epilogue_kernel (mask * scale * act' and the LayerNorm backward, per-workgroup partials of d gamma /
// d beta), wgrad_splitk_kernel (dW = D^T In with the reduction over the NODES split into slabs, fp32 MFMA, the bias column
// folded in as a column of ones) with wgrad_reduce_kernel (slabs summed in a fixed order: no float atomics, two runs agree
// bit for bit), and the gather's backward over the batch ids sorted by node (repeated ids add in batch order).
// The first GCN layer runs through the cached [P X | rowsum(P)] (build_px): no SpMM at the hidden width in the forward, and
// [dW_0 | db_0] = d^T [P X | rowsum(P)] in the backward.  All N rows take part in every level.
#include "lgnn_internal.h"

#include <rocprim/rocprim.hpp>

#include "device_utils.h"

namespace lgnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- forward epilogue ------------------------------------------------------------------------------------------------
struct TrainEpArgs {
  float* S; int64_t ld;        // [N, W] in place: pre-norm sum in, layer output out
  int64_t N, W;
  const float* rowsum; const float* bias;  // optional: S[n, j] += rowsum[n] * bias[j] (the propagated bias of the P X route)
  const float* add; int64_t add_ld;        // optional: S += add (res_0 on the P X route)
  int norm; float eps; const float* gamma; const float* beta;
  float* xhat; float* rstd;    // LayerNorm tape
  int act;                     // -1: none (last layer)
  const uint8_t* mask; float scale;  // keep-mask [N, W] or null
};

// one wave per row
__global__ __launch_bounds__(256) void train_epilogue_kernel(TrainEpArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= g.N) return;
  float* row = g.S + n * g.ld;
  const bool pre = g.rowsum != nullptr || g.add != nullptr;
  const float rs = g.rowsum ? g.rowsum[n] : 0.f;
  float sum = 0.f;
  for (int64_t c = lane; c < g.W; c += 64) {
    float v = row[c];
    if (g.rowsum) v += rs * g.bias[c];
    if (g.add) v += g.add[n * g.add_ld + c];
    if (pre) row[c] = v;
    sum += v;
  }
  float mean = 0.f, rstd = 1.f;
  if (g.norm == LGNN_NORM_LAYER) {
    mean = wave_sum(sum) / float(g.W);
    float var = 0.f;
    for (int64_t c = lane; c < g.W; c += 64) { const float d = row[c] - mean; var += d * d; }
    rstd = rsqrtf(wave_sum(var) / float(g.W) + g.eps);
    if (lane == 0) g.rstd[n] = rstd;
  } else if (g.act < 0 && !g.mask) {
    return;
  }
  for (int64_t c = lane; c < g.W; c += 64) {
    float v = row[c];
    if (g.norm == LGNN_NORM_LAYER) {
      const float xh = (v - mean) * rstd;
      g.xhat[n * g.W + c] = xh;
      v = xh * g.gamma[c] + g.beta[c];
    }
    if (g.act >= 0) v = act_apply(v, g.act);
    if (g.mask) v = g.mask[n * g.W + c] ? v * g.scale : 0.f;
    row[c] = v;
  }
}

static int launch_train_epilogue(const TrainEpArgs& g, hipStream_t s) {
  if (g.N <= 0) return 0;
  hipLaunchKernelGGL(train_epilogue_kernel, dim3(unsigned(cdiv(g.N, 4))), dim3(256), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- backward epilogue -----------------------------------------------------------------------------------------------
struct TrainBackEpArgs {
  float* G; int64_t ld;          // [N, W] in place: d / d(layer output) in, d / d(pre-norm sum) out
  int64_t N, W;
  const float* hout; int64_t h_ld;  // the layer's output (after dropout)
  int act; const uint8_t* mask; float scale, inv_scale;  // 1 / (1 - p) and 1 - p
  int norm; const float* gamma; const float* xhat; const float* rstd;
  float* part;                   // LayerNorm: [blocks][2][W] partial d gamma, d beta
};

constexpr int kNormBlocks = 512;

__global__ __launch_bounds__(256) void train_back_epilogue_kernel(TrainBackEpArgs g) {
  extern __shared__ float acc[];  // LayerNorm: [4 waves][2][W]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ln = g.norm == LGNN_NORM_LAYER;
  float* mine = acc + size_t(wave) * 2 * g.W;
  if (ln) {
    for (int64_t c = lane; c < g.W; c += 64) { mine[c] = 0.f; mine[g.W + c] = 0.f; }
  }
  // every lane owns the columns c = lane (mod 64) of its wave's accumulators: plain loads and stores, a fixed order
  for (int64_t n = int64_t(blockIdx.x) * 4 + wave; n < g.N; n += int64_t(gridDim.x) * 4) {
    float* row = g.G + n * g.ld;
    float s1 = 0.f, s2 = 0.f;
    for (int64_t c = lane; c < g.W; c += 64) {
      const float hv = g.hout[n * g.h_ld + c];
      const bool keep = g.mask ? g.mask[n * g.W + c] != 0 : true;
      const float a = g.mask ? hv * g.inv_scale : hv;  // the activation's output before dropout
      float da = keep ? row[c] * g.scale * act_deriv_from_out(a, g.act) : 0.f;
      if (ln) {
        const float xh = g.xhat[n * g.W + c];
        mine[c] += da * xh;
        mine[g.W + c] += da;
        da *= g.gamma[c];
        s1 += da;
        s2 += da * xh;
      }
      row[c] = da;
    }
    if (ln) {
      const float m1 = wave_sum(s1) / float(g.W), m2 = wave_sum(s2) / float(g.W), r = g.rstd[n];
      for (int64_t c = lane; c < g.W; c += 64) row[c] = r * (row[c] - m1 - g.xhat[n * g.W + c] * m2);
    }
  }
  if (!ln) return;
  __syncthreads();
  for (int64_t c = threadIdx.x; c < 2 * g.W; c += 256)
    g.part[size_t(blockIdx.x) * 2 * g.W + c] = ((acc[c] + acc[2 * g.W + c]) + acc[4 * g.W + c]) + acc[6 * g.W + c];
}

__global__ void norm_part_reduce_kernel(const float* __restrict__ part, int blocks, int64_t W, float* __restrict__ dgamma,
                                        float* __restrict__ dbeta) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= 2 * W) return;
  float v = 0.f;
  for (int b = 0; b < blocks; ++b) v += part[size_t(b) * 2 * W + c];
  if (c < W) dgamma[c] = v;
  else dbeta[c - W] = v;
}

// ---- weight gradient: out[w, k] = sum_n D[n, w] In[n, k]  (+ column k = K: sum_n D[n, w]) -------------------------------------
struct WgradArgs {
  const float* D; int64_t ld_d; int64_t W;   // backward signal [N, W]
  const float* In; int64_t ld_in; int64_t K; // the Linear's input [N, K]
  int ones;                                  // 1: a virtual column K of ones (plain bias); 0: In has K columns, no more
  int64_t N, rows_per_slab;
  float* part; int64_t ld_p;                 // [slabs][W][ld_p], ld_p = K + ones
};

// One wave per (32 rows of the result) x (128 columns) x slab of nodes; a workgroup's four waves take four row tiles of the
// same columns (they read the same In rows).  v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5] = D[n + k][w0 + i]
// and B[k][j = l & 31] = In[n + k][k0 + j]: both are 128-byte row segments, straight from memory.
__global__ __launch_bounds__(256) void wgrad_splitk_kernel(WgradArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t w0 = (int64_t(blockIdx.y) * 4 + wave) * 32;
  if (w0 >= g.W) return;
  const int64_t k0 = int64_t(blockIdx.x) * 128;
  const int64_t n0 = int64_t(blockIdx.z) * g.rows_per_slab;
  const int64_t n1 = n0 + g.rows_per_slab < g.N ? n0 + g.rows_per_slab : g.N;
  const int64_t wc = w0 + l31;
  const bool w_ok = wc < g.W;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
  bool k_ok[4], k_one[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t kc = k0 + j * 32 + l31;
    k_ok[j] = kc < g.K;
    k_one[j] = g.ones && kc == g.K;
  }
  const float* dp = g.D + wc;
  const float* ip = g.In + k0 + l31;
  // four steps of two nodes per trip (loads of a trip issue together); rows past the slab read as zeros
  for (int64_t nb = n0; nb < n1; nb += 8) {
    float a[4], b[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t n = nb + 2 * u + lhi;
      const bool r_ok = n < n1;
      a[u] = (r_ok && w_ok) ? dp[n * g.ld_d] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) b[u][j] = (r_ok && k_ok[j]) ? ip[n * g.ld_in + j * 32] : ((r_ok && k_one[j]) ? 1.f : 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u][j], acc[j], 0, 0, 0);
  }
  float* out = g.part + size_t(blockIdx.z) * g.W * g.ld_p;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t kc = k0 + j * 32 + l31;
    if (kc >= g.ld_p) continue;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t wr = w0 + (q & 3) + 8 * (q >> 2) + 4 * lhi;
      if (wr < g.W) out[wr * g.ld_p + kc] = acc[j][q];
    }
  }
}

struct WgradOut {
  float* W0; float* b0; int64_t rows0;  // rows [0, rows0) of the result: weight [rows0, K] and bias
  float* W1; float* b1;                 // rows [rows0, W): a second Linear stacked below (GCN: res.{l}); may be null
  float* Wc; float* bc; int64_t kc;     // the first kc columns of rows [0, rows0) once more (GraphSAGE: res.{l}); may be null
};

__global__ void wgrad_reduce_kernel(const float* __restrict__ part, int slabs, int64_t W, int64_t K, int64_t ld_p, WgradOut o) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= W * ld_p) return;
  const int64_t w = t / ld_p, k = t % ld_p;
  float v = 0.f;
  for (int z = 0; z < slabs; ++z) v += part[size_t(z) * W * ld_p + t];  // fixed slab order
  if (w < o.rows0) {
    if (k < K) {
      o.W0[w * K + k] = v;
      if (o.Wc && k < o.kc) o.Wc[w * o.kc + k] = v;
    } else {
      o.b0[w] = v;
      if (o.bc) o.bc[w] = v;
    }
  } else if (o.W1) {
    if (k < K) o.W1[(w - o.rows0) * K + k] = v;
    else o.b1[w - o.rows0] = v;
  }
}

// In has K columns and, with ones = 0, one more that plays the bias column (the cached [P X | rowsum(P)])
static int launch_wgrad(lgnn_ctx* h, const float* D, int64_t ld_d, int64_t W, const float* In, int64_t ld_in, int64_t K,
                        bool ones, const WgradOut& o, hipStream_t s) {
  const int64_t N = h->N, ld_p = K + 1;
  WgradArgs g{};
  g.D = D; g.ld_d = ld_d; g.W = W; g.In = In; g.ld_in = ld_in; g.ones = ones ? 1 : 0; g.N = N; g.ld_p = ld_p;
  g.K = ones ? K : K + 1;  // real columns read from In
  const int64_t kblocks = cdiv(ld_p, 128), wblocks = cdiv(cdiv(W, 32), 4);
  // enough workgroups for every CU several times over, partials bounded by 32 MiB
  int64_t slabs = std::min<int64_t>(cdiv(N, 32), cdiv(1024, kblocks * wblocks));
  slabs = std::max<int64_t>(1, std::min<int64_t>(slabs, (int64_t(32) << 20) / (W * ld_p * 4)));
  g.rows_per_slab = cdiv(cdiv(N, slabs), 2) * 2;
  slabs = cdiv(N, g.rows_per_slab);
  LGNN_REQUIRE(slabs < 65536 && wblocks < 65536, "weight gradient: grid too large");
  LGNN_CALL(h->tr.part.reserve(size_t(slabs) * W * ld_p * 4));
  g.part = h->tr.part.as<float>();
  hipLaunchKernelGGL(wgrad_splitk_kernel, dim3(unsigned(kblocks), unsigned(wblocks), unsigned(slabs)), dim3(256), 0, s, g);
  LGNN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(unsigned(cdiv(W * ld_p, 256))), dim3(256), 0, s, h->tr.part.as<float>(),
                     int(slabs), W, K, ld_p, o);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- the gather's backward --------------------------------------------------------------------------------------------
__global__ void train_keys_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, int32_t* __restrict__ keys,
                                  int32_t* __restrict__ ord, int* __restrict__ bad_flag) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t v = idx[m];
  const bool ok = v >= 0 && v < N;
  if (!ok) *bad_flag = 1;  // sticky, reported by lgnn_check_async_errors; such a sample receives no gradient
  keys[m] = ok ? int32_t(v) : int32_t(N);
  ord[m] = int32_t(m);
}

// G[node, c] = sum of grad_out[m, c] over the batch positions m of that node, in ascending m (the sort is stable).
// The first position of a run adds the whole run in one thread per column: a serial loop as long as the node's multiplicity
// (loaders list a node a few times at most)
__global__ void train_scatter_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ ord, int64_t M, int64_t N,
                                     int64_t C, const float* __restrict__ grad_out, float* __restrict__ G, int64_t ld) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= M * C) return;
  const int64_t p = t / C, c = t % C;
  const int32_t key = keys[p];
  if (key >= N || (p > 0 && keys[p - 1] == key)) return;
  float v = 0.f;
  for (int64_t q = p; q < M && keys[q] == key; ++q) v += grad_out[int64_t(ord[q]) * C + c];
  G[int64_t(key) * ld + c] = v;
}

static int sort_batch(lgnn_ctx* h, const int64_t* idx, int64_t M, hipStream_t s) {
  TrainState& t = h->tr;
  LGNN_REQUIRE(M < (int64_t(1) << 31) && h->N < (int64_t(1) << 31) - 1, "batch too large");
  LGNN_CALL(t.keys.reserve(size_t(M) * 4)); LGNN_CALL(t.keys_sorted.reserve(size_t(M) * 4));
  LGNN_CALL(t.ord.reserve(size_t(M) * 4)); LGNN_CALL(t.ord_sorted.reserve(size_t(M) * 4));
  hipLaunchKernelGGL(train_keys_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, h->N, t.keys.as<int32_t>(),
                     t.ord.as<int32_t>(), h->ws.flags.as<int>() + 2);
  LGNN_HIP_CHECK(hipGetLastError());
  unsigned bits = 1;
  while ((int64_t(1) << bits) <= h->N) ++bits;
  size_t bytes = 0;
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, t.keys.as<int32_t>(), t.keys_sorted.as<int32_t>(), t.ord.as<int32_t>(),
                                           t.ord_sorted.as<int32_t>(), size_t(M), 0, bits, s));
  LGNN_CALL(t.sort_tmp.reserve(bytes));
  LGNN_HIP_CHECK(rocprim::radix_sort_pairs(t.sort_tmp.p, bytes, t.keys.as<int32_t>(), t.keys_sorted.as<int32_t>(),
                                           t.ord.as<int32_t>(), t.ord_sorted.as<int32_t>(), size_t(M), 0, bits, s));
  return 0;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
static int64_t max_width(const lgnn_ctx* h) {
  int64_t w = 0;
  for (int l = 1; l <= h->L; ++l) w = std::max(w, h->dims[l]);
  return w;
}

static int hidden_epilogue(lgnn_ctx* h, int l, float* S, int64_t ld, const float* rowsum, const float* bias, const float* add,
                           hipStream_t s) {
  TrainState& t = h->tr;
  const int64_t N = h->N, W = h->dims[l + 1];
  const bool hidden = l < h->L - 1;
  TrainEpArgs e{};
  e.S = S; e.ld = ld; e.N = N; e.W = W; e.rowsum = rowsum; e.bias = bias; e.add = add; e.add_ld = W;
  e.act = -1; e.scale = 1.f;
  if (hidden) {
    e.act = h->act;
    e.mask = t.masks[l]; e.scale = e.mask ? t.scale : 1.f;
    if (h->norm == LGNN_NORM_LAYER) {
      LGNN_CALL(t.xhat[l].reserve(size_t(N) * W * 4));
      LGNN_CALL(t.rstd[l].reserve(size_t(N) * 4));
      e.norm = LGNN_NORM_LAYER; e.eps = h->norm_eps; e.gamma = h->norm_w[l]; e.beta = h->norm_b[l];
      e.xhat = t.xhat[l].as<float>(); e.rstd = t.rstd[l].as<float>();
    }
  } else if (!rowsum && !add) {
    return 0;
  }
  return launch_train_epilogue(e, s);
}

static int train_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const uint8_t* const* masks, float scale, float* out,
                         hipStream_t s) {
  LGNN_REQUIRE(h->L > 0 && h->X, "no model bound (call lgnn_bind_model first)");
  LGNN_REQUIRE(h->norm != LGNN_NORM_BATCH, "training-mode BatchNorm1d (batch statistics, running-stat update) is not supported");
  LGNN_REQUIRE(scale > 0.f, "drop_scale must be positive (1 / (1 - p))");
  TrainState& t = h->tr;
  ForwardCache& fc = h->fc;
  const int64_t N = h->N;
  const int L = h->L;
  const int64_t C = h->dims[L], maxw = max_width(h);
  t.tape_valid = false;
  t.M = M;
  t.scale = masks ? scale : 1.f;
  for (int l = 0; l < kMaxLayers; ++l) t.masks[l] = (masks && l < L - 1) ? masks[l] : nullptr;
  LGNN_CALL(ensure_wt(h, s));
  LGNN_CALL(long_rows_fwd_ensure(h, s));
  const int32_t* lr = h->n_long_fwd > 0 ? (h->P.rowptr == h->PT.rowptr ? h->long_rows.as<int32_t>() : h->long_rows_fwd.as<int32_t>())
                                         : nullptr;
  const int64_t nlr = h->n_long_fwd > 0 ? h->n_long_fwd : 0;
  LGNN_CALL(t.out.reserve(size_t(N) * C * 4));
  SpmmArgs a{};
  a.rowptr = h->P.rowptr; a.col = h->P.col; a.val = h->P.val; a.nrows = N; a.out_act = -1;
  a.long_rows = lr; a.n_long = nlr;

  if (h->kind == LGNN_KIND_GCN) {
    // what depends on the graph and X only: [P X | rowsum(P)] and the padded X (kept across weight updates)
    LGNN_CALL(forward_input_view(h, s));
    if (!(fc.x_valid && fc.px_valid)) LGNN_CALL(build_px(h, s));
    fc.x_valid = true;
    fc.px_valid = true;
    LGNN_CALL(t.z.reserve(size_t(N) * maxw * 4));
    if (h->has_res) LGNN_CALL(t.res.reserve(size_t(N) * maxw * 4));
    for (int l = 0; l < L; ++l) {
      const int64_t din = h->dims[l], dout = h->dims[l + 1];
      const bool hidden = l < L - 1, res = hidden && h->has_res;
      if (hidden) LGNN_CALL(t.in[l + 1].reserve(size_t(N) * dout * 4));
      float* S = hidden ? t.in[l + 1].as<float>() : t.out.as<float>();
      const float* in = l == 0 ? fc.lin_in_p[0] : t.in[l].as<float>();
      const int64_t in_ld = l == 0 ? fc.lin_in_ld[0] : din;
      if (res) {
        GemmEpilogue er;
        er.no_atomics = true;
        er.bias = h->br[l];
        LGNN_CALL(launch_gemm(in, in_ld, h->Wrt[l].as<float>(), dout, t.res.as<float>(), dout, N, din, dout, er, s));
      }
      if (l == 0) {
        // P (X W^T + 1 b^T) = (P X) W^T + rowsum(P) b^T
        GemmEpilogue ep;
        ep.no_atomics = true;
        LGNN_CALL(launch_gemm(fc.prop_in[0].as<float>(), fc.prop_ld[0], h->Wt[0].as<float>(), dout, S, dout, N, din, dout, ep, s));
        LGNN_CALL(hidden_epilogue(h, l, S, dout, fc.rowsum.as<float>(), h->b[0], res ? t.res.as<float>() : nullptr, s));
      } else {
        GemmEpilogue ep;
        ep.no_atomics = true;
        ep.bias = h->b[l];
        LGNN_CALL(launch_gemm(in, in_ld, h->Wt[l].as<float>(), dout, t.z.as<float>(), dout, N, din, dout, ep, s));
        SpmmArgs p = a;
        p.in = t.z.as<float>(); p.in_ld = dout; p.out = S; p.out_ld = dout; p.width = dout;
        if (res) { p.self = t.res.as<float>(); p.self_ld = dout; }
        LGNN_CALL(launch_spmm_ex(p, 1, s));
        LGNN_CALL(hidden_epilogue(h, l, S, dout, nullptr, nullptr, nullptr, s));
      }
    }
  } else {
    for (int l = 0; l < L; ++l) LGNN_CALL(t.in[l].reserve(size_t(N) * 2 * h->dims[l] * 4));
    for (int l = 0; l < L; ++l) {
      const int64_t d = h->dims[l], dout = h->dims[l + 1];
      const bool hidden = l < L - 1;
      float* cat = t.in[l].as<float>();
      if (l > 0 || !t.input_valid) {
        if (l == 0)
          LGNN_HIP_CHECK(hipMemcpy2DAsync(cat, size_t(2 * d) * 4, h->X, size_t(d) * 4, size_t(d) * 4, size_t(N),
                                          hipMemcpyDeviceToDevice, s));
        SpmmArgs p = a;
        p.in = cat; p.in_ld = 2 * d; p.out = cat + d; p.out_ld = 2 * d; p.width = d;
        LGNN_CALL(launch_spmm_ex(p, 1, s));
        if (l == 0) t.input_valid = true;
      }
      GemmEpilogue ep;
      ep.no_atomics = true;
      ep.bias = (hidden && h->has_res) ? h->bcomb[l].as<float>() : h->b[l];  // Wt[l] holds (W_l + [Wr_l | 0])^T then
      if (hidden) {
        float* nxt = t.in[l + 1].as<float>();
        LGNN_CALL(launch_gemm(cat, 2 * d, h->Wt[l].as<float>(), dout, nxt, 2 * dout, N, 2 * d, dout, ep, s));
        LGNN_CALL(hidden_epilogue(h, l, nxt, 2 * dout, nullptr, nullptr, nullptr, s));
      } else {
        LGNN_CALL(launch_gemm(cat, 2 * d, h->Wt[l].as<float>(), dout, t.out.as<float>(), dout, N, 2 * d, dout, ep, s));
      }
    }
  }
  if (M > 0) {
    LGNN_CALL(sort_batch(h, idx, M, s));
    LGNN_CALL(launch_gather_rows(t.out.as<float>(), C, N, idx, M, C, out, h->ws.flags.as<int>() + 2, s));
  }
  t.tape_valid = true;
  return 0;
}

// ---- backward ---------------------------------------------------------------------------------------------------------
struct TrainGrads {
  float* const* W; float* const* b; float* const* Wr; float* const* br; float* const* nw; float* const* nb;
};

// d / d(output of hidden layer j) [N, W] at (G, ld), in place -> d / d(pre-norm sum of layer j); d gamma, d beta
static int back_epilogue(lgnn_ctx* h, int j, float* G, int64_t ld, const TrainGrads& gr, hipStream_t s) {
  TrainState& t = h->tr;
  const int64_t N = h->N, W = h->dims[j + 1];
  TrainBackEpArgs e{};
  e.G = G; e.ld = ld; e.N = N; e.W = W;
  e.hout = t.in[j + 1].as<float>();
  e.h_ld = h->kind == LGNN_KIND_SAGE ? 2 * W : W;
  e.act = h->act; e.mask = t.masks[j]; e.scale = e.mask ? t.scale : 1.f;
  e.inv_scale = 1.f / e.scale;
  size_t smem = 0;
  const int blocks = int(std::min<int64_t>(cdiv(N, 4), kNormBlocks));
  if (h->norm == LGNN_NORM_LAYER) {
    LGNN_REQUIRE(W <= 2048, "training backward: LayerNorm wider than 2048");
    e.norm = LGNN_NORM_LAYER; e.gamma = h->norm_w[j]; e.xhat = t.xhat[j].as<float>(); e.rstd = t.rstd[j].as<float>();
    LGNN_CALL(t.norm_part.reserve(size_t(blocks) * 2 * W * 4));
    e.part = t.norm_part.as<float>();
    smem = size_t(4) * 2 * W * 4;
  }
  hipLaunchKernelGGL(train_back_epilogue_kernel, dim3(unsigned(blocks)), dim3(256), smem, s, e);
  LGNN_HIP_CHECK(hipGetLastError());
  if (h->norm == LGNN_NORM_LAYER) {
    hipLaunchKernelGGL(norm_part_reduce_kernel, dim3(unsigned(cdiv(2 * W, 256))), dim3(256), 0, s, t.norm_part.as<float>(), blocks,
                       W, gr.nw[j], gr.nb[j]);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

static int train_backward(lgnn_ctx* h, const float* grad_out, const TrainGrads& gr, hipStream_t s) {
  TrainState& t = h->tr;
  LGNN_REQUIRE(h->L > 0 && h->X, "no model bound (call lgnn_bind_model first)");
  LGNN_REQUIRE(t.tape_valid, "lgnn_train_backward without a matching lgnn_train_forward: none ran, its tape was consumed by an "
                             "earlier backward, or the parameters / the graph changed since");
  t.tape_valid = false;
  const int64_t N = h->N, M = t.M;
  const int L = h->L;
  const int64_t C = h->dims[L], maxw = max_width(h);
  LGNN_REQUIRE(gr.W && gr.b, "null gradient pointer array");
  for (int l = 0; l < L; ++l) LGNN_REQUIRE(gr.W[l] && gr.b[l], "null weight / bias gradient pointer");
  if (h->has_res) {
    LGNN_REQUIRE(gr.Wr && gr.br, "the model has res Linears: grad_res_W / grad_res_b are needed");
    for (int l = 0; l < L - 1; ++l) LGNN_REQUIRE(gr.Wr[l] && gr.br[l], "null res gradient pointer");
  }
  if (h->norm == LGNN_NORM_LAYER) {
    LGNN_REQUIRE(gr.nw && gr.nb, "the model has LayerNorms: grad_norm_w / grad_norm_b are needed");
    for (int l = 0; l < L - 1; ++l) LGNN_REQUIRE(gr.nw[l] && gr.nb[l], "null norm gradient pointer");
  }
  LGNN_CALL(t.ga.reserve(size_t(N) * 2 * maxw * 4));
  LGNN_CALL(t.gb.reserve(size_t(N) * 2 * maxw * 4));
  LGNN_CALL(long_rows_ensure(h, s));
  SpmmArgs pt{};
  pt.rowptr = h->PT.rowptr; pt.col = h->PT.col; pt.val = h->PT.val; pt.nrows = N; pt.out_act = -1;
  pt.long_rows = h->n_long > 0 ? h->long_rows.as<int32_t>() : nullptr;
  pt.n_long = h->n_long > 0 ? h->n_long : 0;
  const bool gcn = h->kind == LGNN_KIND_GCN;
  float* cur = t.ga.as<float>();
  float* nxt = t.gb.as<float>();

  // the gather's backward: d / d(all-node logits).  GCN keeps a level's signal d in the right half of [T | d] (row stride
  // 2 dout) so that T = P^T d and d stack into one operand for the layers with a res Linear
  const int64_t ld_top = gcn ? 2 * C : C;
  float* Gtop = gcn ? cur + C : cur;
  LGNN_HIP_CHECK(hipMemsetAsync(cur, 0, size_t(N) * ld_top * 4, s));
  if (M > 0) {
    LGNN_REQUIRE(grad_out, "null grad_out");
    hipLaunchKernelGGL(train_scatter_kernel, dim3(unsigned(cdiv(M * C, 256))), dim3(256), 0, s, t.keys_sorted.as<int32_t>(),
                       t.ord_sorted.as<int32_t>(), M, N, C, grad_out, Gtop, ld_top);
    LGNN_HIP_CHECK(hipGetLastError());
  }

  for (int l = L - 1; l >= 0; --l) {
    const int64_t din = h->dims[l], dout = h->dims[l + 1];
    const bool res = h->has_res && l < L - 1;
    if (gcn) {
      float* d = cur + dout;  // [N, dout], row stride 2 dout
      if (l == 0) {
        // [dW_0 | db_0] = d^T [P X | rowsum(P)];  [dWr_0 | dbr_0] = d^T [X | 1]
        WgradOut o{};
        o.W0 = gr.W[0]; o.b0 = gr.b[0]; o.rows0 = dout;
        LGNN_CALL(launch_wgrad(h, d, 2 * dout, dout, h->fc.prop_in[0].as<float>(), h->fc.prop_ld[0], din, false, o, s));
        if (res) {
          WgradOut r{};
          r.W0 = gr.Wr[0]; r.b0 = gr.br[0]; r.rows0 = dout;
          LGNN_CALL(launch_wgrad(h, d, 2 * dout, dout, h->fc.lin_in_p[0], h->fc.lin_in_ld[0], din, true, r, s));
        }
        break;
      }
      SpmmArgs p = pt;
      p.in = d; p.in_ld = 2 * dout; p.out = cur; p.out_ld = 2 * dout; p.width = dout;
      LGNN_CALL(launch_spmm_ex(p, 1, s));  // T = P^T d
      const int64_t w = res ? 2 * dout : dout;
      WgradOut o{};
      o.W0 = gr.W[l]; o.b0 = gr.b[l]; o.rows0 = dout;
      if (res) { o.W1 = gr.Wr[l]; o.b1 = gr.br[l]; }
      LGNN_CALL(launch_wgrad(h, cur, 2 * dout, w, t.in[l].as<float>(), din, din, true, o, s));
      // d / d h_l = T W_l (+ d Wr_l) into the right half of the next level's pair
      const float* B = h->W[l];
      if (res) {
        LGNN_CALL(t.wstack.reserve(size_t(2) * dout * din * 4));
        LGNN_HIP_CHECK(hipMemcpyAsync(t.wstack.p, h->W[l], size_t(dout) * din * 4, hipMemcpyDeviceToDevice, s));
        LGNN_HIP_CHECK(hipMemcpyAsync(t.wstack.as<float>() + dout * din, h->Wr[l], size_t(dout) * din * 4,
                                      hipMemcpyDeviceToDevice, s));
        B = t.wstack.as<float>();
      }
      GemmEpilogue ep;
      ep.no_atomics = true;
      LGNN_CALL(launch_gemm(cur, 2 * dout, B, din, nxt + din, 2 * din, N, w, din, ep, s));
      LGNN_CALL(back_epilogue(h, l - 1, nxt + din, 2 * din, gr, s));
      std::swap(cur, nxt);
    } else {
      // GraphSAGE: d [N, dout] contiguous in cur
      WgradOut o{};
      o.W0 = gr.W[l]; o.b0 = gr.b[l]; o.rows0 = dout;
      if (res) { o.Wc = gr.Wr[l]; o.bc = gr.br[l]; o.kc = din; }
      LGNN_CALL(launch_wgrad(h, cur, dout, dout, t.in[l].as<float>(), 2 * din, 2 * din, true, o, s));
      if (l == 0) break;
      GemmEpilogue ep;
      ep.no_atomics = true;
      LGNN_CALL(launch_gemm(cur, dout, h->Wback(l), 2 * din, nxt, 2 * din, N, dout, 2 * din, ep, s));  // dcat = d W
      SpmmArgs p = pt;
      p.in = nxt + din; p.in_ld = 2 * din; p.self = nxt; p.self_ld = 2 * din; p.out = cur; p.out_ld = din; p.width = din;
      LGNN_CALL(launch_spmm_ex(p, 1, s));  // d / d h_l = dcat_1 + P^T dcat_2
      LGNN_CALL(back_epilogue(h, l - 1, cur, din, gr, s));
    }
  }
  return 0;
}

}  // namespace lgnn

using namespace lgnn;

extern "C" int lgnn_train_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const uint8_t* const* drop_masks, float drop_scale,
                                  float* out, void* stream) {
  if (!h || (M > 0 && (!idx || !out))) { set_error("null argument"); return 2; }
  return train_forward(h, idx, M, drop_masks, drop_scale, out, static_cast<hipStream_t>(stream));
}

extern "C" int lgnn_train_backward(lgnn_ctx* h, const float* grad_out, float* const* grad_W, float* const* grad_b,
                                   float* const* grad_res_W, float* const* grad_res_b, float* const* grad_norm_w,
                                   float* const* grad_norm_b, void* stream) {
  if (!h) { set_error("null context"); return 2; }
  const TrainGrads gr{grad_W, grad_b, grad_res_W, grad_res_b, grad_norm_w, grad_norm_b};
  return train_backward(h, grad_out, gr, static_cast<hipStream_t>(stream));
}
