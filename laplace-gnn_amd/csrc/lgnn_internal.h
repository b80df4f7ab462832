// Internal declarations shared by the HIP translation units of liblaplace_gnn_hip.so.
// gfx950 (MI355X / CDNA4) only: wave64, fp32-input MFMA, 160 KiB LDS per CU.
#pragma once
#include <atomic>
#include <cstring>  // rocprim's texture iterator needs host memset declared first
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/laplace_gnn_hip.h"

namespace lgnn {

void set_error(const std::string& msg);

#define LGNN_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      lgnn::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                 \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

#define LGNN_REQUIRE(cond, msg)                                                           \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      lgnn::set_error(std::string(msg) + " (" #cond ")");                                 \
      return 2;                                                                           \
    }                                                                                     \
  } while (0)

#define LGNN_CALL(expr)                                                                   \
  do {                                                                                    \
    int _rc = (expr);                                                                     \
    if (_rc != 0) return _rc;                                                             \
  } while (0)

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// More than 64 KiB of dynamic LDS needs an explicit opt-in, and the attribute belongs to the current device's copy of the
// kernel: set it the first time `Kernel` is launched on a device (`bytes`: the kernel's fixed upper bound), remembered in one
// bit per device.  Two threads that race set it twice, which is harmless; a device id beyond the mask sets it on every call.
template <auto Kernel>
int lds_opt_in(int bytes) {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  LGNN_HIP_CHECK(hipGetDevice(&dev));
  const uint64_t bit = dev < 64 ? uint64_t(1) << dev : 0;
  if (done.load(std::memory_order_acquire) & bit) return 0;
  LGNN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.fetch_or(bit, std::memory_order_release);
  return 0;
}

// Grow-only device buffer (no allocation in steady state).  It owns its memory: the destructor frees it, so a member of a
// context struct needs no entry in a release list, and a function's temporary may be left through LGNN_CALL / LGNN_HIP_CHECK /
// LGNN_REQUIRE.  Move only.  hipFree waits for the device, so an error return never frees under a running kernel; success
// paths synchronise their stream before a temporary goes out of scope.  What a struct owns is listed once, by the each_buf
// visitor under its members (lgnn_device_bytes sums over it).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool host = false;  // reserve_host: pinned host memory the device reads and writes in place (same address on both sides)
  DevBuf() = default;
  ~DevBuf();
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept;
  DevBuf& operator=(DevBuf&& o) noexcept;
  int reserve(size_t want);
  int reserve_host(size_t want);
  void release();
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible_v<DevBuf>);

// CSR with int32 indices (N, nnz < 2^31), fp32 values aligned with `col`
struct Csr {
  int32_t* rowptr = nullptr;  // [n+1]
  int32_t* col = nullptr;     // [nnz]
  float* val = nullptr;       // [nnz]
};

constexpr int kMaxLayers = 8;

struct ForwardCache {
  bool valid = false;
  bool aux_valid = false;            // rowsum / propagated inputs for diag + last layer
  bool wt_valid = false;             // lgnn_ctx::Wt (transposed weights) match the bound weights' current version
  // What depends on the graph and X only -- not on the weights -- survives lgnn_invalidate and is rebuilt at bind time:
  bool x_valid = false;              // Xpad, gram_raw[0] (GCN: X^T X)
  bool px_valid = false;             // rowsum, prop_in[0] (GCN: P X)
  DevBuf Xpad;                       // GCN, F % 4 != 0: X copied to rows of F rounded up to 4 floats (zero padded) so that
                                     // the first GEMM, SpMM and Gram run their 16-byte paths (Cora: F = 1 433)
  int64_t prop_ld[kMaxLayers] = {};  // row stride of prop_in[l]
  bool gram_valid[kMaxLayers] = {};  // raw input Grams (upper triangle) per layer
  DevBuf lin_in[kMaxLayers];         // GraphSAGE: cat_l = [h_l | P h_l]  [N, 2 d_l]
  DevBuf act_out[kMaxLayers];        // GCN: h_{l+1} = act(P Z_l), l < L-1 : [N, out_l]
  const float* lin_in_p[kMaxLayers] = {};  // what nn.Linear l sees: [N, in_l] with row stride lin_in_ld
  int64_t lin_in_ld[kMaxLayers] = {};
  const float* hact_p[kMaxLayers] = {};    // activation output h_{l+1} (input of layer l+1), row stride hact_ld
  int64_t hact_ld[kMaxLayers] = {};
  DevBuf out;                        // logits for all nodes [N, C]
  DevBuf tmp;                        // [N, max width] scratch of the forward
  DevBuf gram_raw[kMaxLayers];       // [in_l, in_l] raw in^T in (upper sub-tiles valid)
  DevBuf prop_in[kMaxLayers];        // P @ lin_in[l]  [N, in_l]   (diag / last layer; GCN)
  DevBuf rowsum;                     // rowsum(P) [N]
  DevBuf dact0;                      // act'(h_1) [N, dims[1]] (closed-form diagonal GGN of 2-layer models)
  DevBuf mask_bits[kMaxLayers];      // ReLU: bit j of word w of node n = (h_{l+1}[n][32w+j] > 0)
  // models with res / norm (gnn/models/base_gnn.py:141-149): the norm's backward needs the normalised rows and 1/sigma
  DevBuf xhat[kMaxLayers];           // [N, dims[l+1]] normalised pre-activation of hidden layer l
  DevBuf rstd[kMaxLayers];           // LayerNorm: [N] 1/sqrt(var + eps) per row; BatchNorm (eval): [dims[l+1]] per channel
  DevBuf res_out;                    // [N, max width] res_l(h_l) of the layer being computed (GCN)
  DevBuf pre_norm;                   // [N, max width] s_l = res_l(h_l) + conv_l(h_l) before the norm
  template <class F> void each_buf(F&& f) const {
    for (int l = 0; l < kMaxLayers; ++l) {
      f(lin_in[l]); f(act_out[l]); f(gram_raw[l]); f(prop_in[l]); f(mask_bits[l]); f(xhat[l]); f(rstd[l]);
    }
    f(Xpad); f(out); f(tmp); f(rowsum); f(dact0); f(res_out); f(pre_norm);
  }
};

struct Workspace {
  DevBuf pos;       // int32 [N]   batch position of a node, INT_MAX if not in batch
  DevBuf seeds;     // fp32 [M, C, C] (c-major rows inside a sample: [m][c][k])
  DevBuf probs;     // fp32 [M, C] softmax
  DevBuf mult;      // int32 [M]: occurrences of the node whose first batch position this is (0 elsewhere)
  DevBuf planes_a;  // backward planes, ping
  // GraphSAGE compact top level: planes_a is kept all zero outside the rows of the current batch (which are cleared
  // again after use); these remember for which buffer / extent that holds
  const void* planes_a_zero_ptr = nullptr;
  size_t planes_a_zero_bytes = 0;
  DevBuf planes_b;  // backward planes, pong
  DevBuf gram_scratch[kMaxLayers];  // [out_l, out_l] per-call partial B (upper sub-tiles)
  DevBuf misc;
  DevBuf jac;      // fp32 [chunk, C, P]: Jacobians of a chunk of samples (generic-depth diagonal GGN)
  DevBuf top;    // top-layer gradient planes [C][N][C]
  DevBuf active;   // uint8 [N]: node has a non-zero top-layer gradient row
  DevBuf val_act;  // fp32 [nnz]: P^T values with inactive source columns zeroed
  DevBuf act_list; // int32 [N]: sorted ids of the active nodes; act_count: their number (device int32)
  DevBuf act_count;
  DevBuf select_tmp;
  DevBuf flags;  // 64 B of asynchronous error flags
  DevBuf out_flags, out_list, out_count;  // GraphSAGE KFAC: rows of the first backward plane set that can be non-zero
  DevBuf val_act2;  // P^T's values with the columns outside that row set zeroed (second backward level of deeper models)
  // two-hop path route of the first layer's B (paths.hip): per-sample coefficient rows [M][3][64], the rows (u | p) [2 M][C]
  // and their products with W_1 [2 M][H]; R = P^T[:, batch] as CSR over v (counts / cursors, row pointers, sample, weight)
  DevBuf path_coef, path_up, path_bg, path_cnt, path_rptr, path_rm, path_rw, path_zeros;
  DevBuf path_alpha;  // GraphSAGE: the samples' alpha coefficients, class major [M][64] (weights of the one-hot paths)
  DevBuf path_pcnt, path_pptr, path_pm, path_pv, path_pw;  // the batch's paths per destination node (CSR over n)
  DevBuf path_flags, path_nodes, path_nnodes;              // nodes of the launch's range that have a path: flags, list, count
  DevBuf path_scale, path_bgn;  // the fp16 Gram's PathScale block (paths.h) and the column-normalised copy of path_bg
  DevBuf path_vsum;             // ... and, per row of the coefficient table, max_c sum_k |V[k, c]| of the row's seed block (bits)
  // the top layer's term lists (toppairs.hip): s_m [M]; per-node pair counts and their scan [N + 1]; the pairs (m, m', w w')
  DevBuf pair_s, pair_cnt, pair_ptr, pair_m, pair_m2, pair_w;
  DevBuf pair_part;  // top_pairs_kernel's partial sums, one row of upper tiles per workgroup
  // (the list's capacity is max(4 nnz, 4 M entries); a batch whose list is longer takes the enumerating route on the device)
  bool path_zeros_set = false;
  DevBuf gram_scratch_res[kMaxLayers];  // res / norm models: per-call partial B of res.{l} (GCN; GraphSAGE shares the conv's)
  DevBuf planes_c;  // GCN with res, >= 3 layers: u_l Wr_l of the level being computed; adjacency gradient (diag, res / norm): tangent planes
  DevBuf adj_z0;    // adjacency gradient of res / norm models: Z0 = X W0^T + b0 [N, H]
  DevBuf adj_dir;   // the same, diagonal posterior: parameter directions R [chunk, C, P]
  // LoRA (lora.hip): compacted flips of lgnn_lora_threshold (rows, cols int64, state uint8), their counter, and the
  // per-row-tile partials of grad_A in lgnn_lora_grad
  DevBuf lora_rows, lora_cols, lora_state, lora_count, lora_part;
  DevBuf dense_stored;  // fp32 [nnz]: scratch accumulator of the stored-entry terms on the dense route
  DevBuf dense_rows;    // int32 [2 M + 1]: output / operand rows of the seed term on the dense route
  // subnetwork Laplace (subnet.hip): the caller's indices sorted (int64 [S]) with their positions in the caller's list
  // (int32 [S]; subnet_iota: the unsorted positions), the sort's scratch, the decoded columns of the closed-form route
  // and the chunk X [mc C, ld] the Gram kernel reads
  DevBuf subnet_keys, subnet_ord, subnet_iota, subnet_tmp, subnet_plan, subnet_x;
  // functional Laplace (gpkernel.hip): tables [z][mc][ld] and [phi | s] rows of the two chunks, G [z'][ma mb], the class
  // contraction's output Kt [(c, e)][ma mb], Phi Phi^T [ma][mb], W_pair [(c, e)][z'], split-K partials, and the two chunks of
  // Jacobian rows of the general route
  DevBuf gp_tab_a, gp_tab_b, gp_phi_a, gp_phi_b, gp_g, gp_kt, gp_s, gp_wpair, gp_part, gp_jac_a, gp_jac_b;
  // joint GLM predictive (glmcov.hip; it shares the gp_* buffers above): the rotated [phi | s] rows of the two chunks, the
  // b side's C scaled copies, the rotated tables [n][l][z], V [(n, c)][k][l] of the two chunks, the first layer's term
  // [(n, c)][(m, e)], the call's small operands (class pairs, M, Q^T, padded S) and the general route's rotation scratch
  DevBuf cov_phit_a, cov_phit_b, cov_phis, cov_t2, cov_va, cov_vb, cov_add, cov_small, cov_scr;
  // GGN-times-block products (ggnmat.hip): a chunk of Jacobian rows [mc C, P], U = J V^T [mc C, k], W^T [k, mc C] and the
  // chunk's product [k, P]
  DevBuf ggn_jac, ggn_u, ggn_wt, ggn_tmp;
  // ... and of its structured route: q and qbar [kc][|R|][Cz] (u and w [kc][M][C] share ggn_u / ggn_wt), the slab partials
  // [slabs][kc][P]
  DevBuf ggn_q, ggn_qbar, ggn_part;
  // exact Hessian's residual product (hessmat.hip; it shares ggn_wt for the residual rows and ggn_part): G [|R|][Cz], G W1
  // [|R|][H], and E, T [kc][|R|][H]
  DevBuf hess_g, hess_gw1, hess_e, hess_t;
  // per-sample GraphSAGE adjacency gradient (adjgrad_sage.hip): the candidates' rows sorted (int32 [K]) with their positions
  // in the caller's list (int32 [K]; cand_iota: the unsorted positions), the sort's scratch, and the slice of every row
  // (int32 [N + 1])
  DevBuf cand_rows, cand_ord, cand_iota, cand_tmp, cand_ptr;
  template <class F> void each_buf(F&& f) const {
    for (int l = 0; l < kMaxLayers; ++l) { f(gram_scratch[l]); f(gram_scratch_res[l]); }
    f(pos); f(seeds); f(probs); f(mult); f(planes_a); f(planes_b); f(misc); f(jac); f(top); f(active); f(val_act);
    f(act_list); f(act_count); f(select_tmp); f(flags); f(out_flags); f(out_list); f(out_count); f(val_act2);
    f(path_coef); f(path_up); f(path_bg); f(path_cnt); f(path_rptr); f(path_rm); f(path_rw); f(path_zeros); f(path_alpha);
    f(path_pcnt); f(path_pptr); f(path_pm); f(path_pv); f(path_pw); f(path_flags); f(path_nodes); f(path_nnodes);
    f(path_scale); f(path_bgn); f(path_vsum);
    f(pair_s); f(pair_cnt); f(pair_ptr); f(pair_m); f(pair_m2); f(pair_w); f(pair_part);
    f(planes_c); f(adj_z0); f(adj_dir); f(lora_rows); f(lora_cols); f(lora_state); f(lora_count); f(lora_part);
    f(dense_stored); f(dense_rows);
    f(subnet_keys); f(subnet_ord); f(subnet_iota); f(subnet_tmp); f(subnet_plan); f(subnet_x);
    f(gp_tab_a); f(gp_tab_b); f(gp_phi_a); f(gp_phi_b); f(gp_g); f(gp_kt); f(gp_s); f(gp_wpair); f(gp_part); f(gp_jac_a);
    f(gp_jac_b); f(cov_phit_a); f(cov_phit_b); f(cov_phis); f(cov_t2); f(cov_va); f(cov_vb); f(cov_add); f(cov_small);
    f(cov_scr); f(ggn_jac); f(ggn_u); f(ggn_wt); f(ggn_tmp); f(ggn_q); f(ggn_qbar); f(ggn_part);
    f(hess_g); f(hess_gw1); f(hess_e); f(hess_t);
    f(cand_rows); f(cand_ord); f(cand_iota); f(cand_tmp); f(cand_ptr);
  }
};

// ---- batch-structure cache (batchcache.hip) ---------------------------------------------------------------------------
// What a KFAC accumulate derives from the graph and a batch's node ids alone -- not from the weights: the active-row list
// of the GCN top layer and the two-hop path list of the path route.  The caller names a batch by a 64-bit tag
// (lgnn_kfac_batch_tag); a tag seen a second time gets an entry, every later accumulate of that batch launches none of the
// kernels that build these lists.  Entries own their memory (exact sizes, allocated once: Workspace buffers move when
// they grow) and are dropped when the graph changes, never by lgnn_invalidate.
template <class T>
struct DevArray {  // typed array of an entry: filled once at its exact size (batchcache.hip), null until then
  DevBuf buf;
  operator T*() const { return buf.as<T>(); }
};
struct BatchEntry {
  uint64_t tag = 0;
  int64_t M = 0;
  uint64_t last_use = 0;
  size_t bytes = 0, path_bytes = 0;  // device bytes of the whole entry / of its path part
  bool refused = false;         // over the budget (or out of memory): the tag stays known, nothing is kept or built again
  DevArray<int64_t> ids;       // [M] the node ids the entry was built from (compared on every hit by mark_batch_kernel)
  // active rows: flags [N], sorted list [act_n], count (device int32)
  bool has_act = false;
  DevArray<uint8_t> active;
  DevArray<int32_t> act_list;
  DevArray<int32_t> act_count;
  // two-hop paths per destination node (CSR over all N nodes); pm / pv / pw stay null when the list overflowed `cap`
  bool has_paths = false;
  int64_t cap = 0;              // the list capacity the build ran with (LGNN_PATH_LIST_CAP): another capacity is a rebuild
  DevArray<int32_t> pptr;       // [N + 1]
  DevArray<int32_t> pm;
  DevArray<int32_t> pv;
  DevArray<float> pw;
  // nodes of [0, N) with a path (short batches only): list, count (device int32)
  bool has_nodes = false;
  DevArray<int32_t> nodes;
  DevArray<int32_t> nnodes;
  // R = P^T[:, batch] (part of the path structure: the overflow route and the top-layer tiles, toptiles.hip, read it)
  DevArray<int32_t> rptr;       // [N + 1]
  DevArray<int32_t> r_m;
  DevArray<float> r_w;
  // the top layer's term lists (toppairs.hip), built from R the first time a call of this batch runs top_pairs_kernel: s_m [M],
  // the pairs of samples that share a node (m, m', w w') and their number (device int32); counted in path_bytes
  bool has_pairs = false;
  bool pairs_refused = false;   // the lists did not fit the budget: the rest of the entry stays, they are built per call
  DevArray<float> pair_s;
  DevArray<int32_t> pair_m;
  DevArray<int32_t> pair_m2;
  DevArray<float> pair_w;
  DevArray<int32_t> pair_n;
};
struct BatchCache {
  std::vector<BatchEntry*> entries;
  std::vector<uint64_t> seen;   // tags met once and not cached yet (bounded; the oldest goes first)
  uint64_t pending_tag = 0;     // lgnn_kfac_batch_tag: consumed and cleared by the next accumulate
  uint64_t clock = 0;
  size_t bytes = 0;
  int64_t hits = 0, misses = 0, builds = 0;
};

// ---- training-mode forward / backward (train.hip) ---------------------------------------------------------------------
// The tape of one lgnn_train_forward call and the scratch of its backward.  Nothing here is read by the eval-mode calls:
// dropped activations never reach ForwardCache.  Every buffer is counted by lgnn_device_bytes (each_buf).
struct TrainState {
  bool tape_valid = false;   // a forward ran, neither parameters nor graph changed since, no backward consumed it yet
  bool input_valid = false;  // GraphSAGE: in[0] = [X | P X] matches the graph and X
  int64_t M = 0;
  float scale = 1.f;                         // 1 / (1 - p)
  const uint8_t* masks[kMaxLayers] = {};     // borrowed keep-masks [N, dims[l+1]] per hidden layer (null: keep everything)
  DevBuf in[kMaxLayers];     // what nn.Linear l reads: GCN l >= 1: h_l [N, dims[l]]; GraphSAGE: cat_l = [h_l | P h_l] [N, 2 dims[l]]
  DevBuf xhat[kMaxLayers];   // LayerNorm: normalised rows [N, dims[l+1]]
  DevBuf rstd[kMaxLayers];   // LayerNorm: 1 / sigma per row [N]
  DevBuf out;                // all-node logits [N, C]
  DevBuf z, res;             // [N, max width]: Z_l = h_l W_l^T + b_l and res_l(h_l) of the layer being computed (GCN)
  DevBuf ga, gb;             // backward signals, ping / pong [N, 2 max width]
  DevBuf keys, keys_sorted, ord, ord_sorted, sort_tmp;  // batch ids sorted by node (stable): the gather's backward adds in m order
  DevBuf part;               // split-K partials of the weight gradient [slabs][rows][cols + 1]
  DevBuf wstack;             // GCN with res: [W_l ; Wr_l] [2 dims[l+1], dims[l]]
  DevBuf norm_part;          // per-workgroup partials of d gamma / d beta [blocks][2][width]
  template <class F> void each_buf(F&& f) const {
    for (int l = 0; l < kMaxLayers; ++l) { f(in[l]); f(xhat[l]); f(rstd[l]); }
    f(out); f(z); f(res); f(ga); f(gb); f(keys); f(keys_sorted); f(ord); f(ord_sorted); f(sort_tmp);
    f(part); f(wstack); f(norm_part);
  }
};

// ---- sampled forward (sampled.hip) --------------------------------------------------------------------------------------
// Buffers of lgnn_sampled_forward alone.  The entry never reserves a Workspace or ForwardCache buffer: a captured fit holds
// raw pointers into those.  in0 depends on the graph and X only (in_valid is dropped where ForwardCache::px_valid is).
struct SampledState {
  bool in_valid = false;
  int64_t ldk = 0;     // row stride of in0: in_0 + 1 rounded up to 4 floats
  DevBuf in0;          // [N, ldk]: GCN [P X | rowsum(P) | 0 ..], GraphSAGE [X | P X | 1 | 0 ..] (the last used column meets the bias)
  DevBuf need;         // uint8 [N]: the row is needed by the call's evaluation nodes
  DevBuf rows;         // int32 [max(N, M)]: the needed rows R, sorted (1 layer: the batch's ids, -1 where invalid)
  DevBuf count;        // int32: |R| (device)
  DevBuf rpos;         // int32 [N]: position of a needed row in R
  DevBuf z;            // fp32 [S_chunk, N, C or 2 C]: the second Linear's products of a chunk of samples
  DevBuf select_tmp;   // rocPRIM select scratch
  template <class F> void each_buf(F&& f) const {
    f(in0); f(need); f(rows); f(count); f(rpos); f(z); f(select_tmp);
  }
};

}  // namespace lgnn

struct lgnn_ctx {
  int64_t N = 0;
  int64_t nnz = 0;
  int kind = 0;
  bool sym = false;
  bool self_loops = false;  // LGNN_KIND_SELF_LOOPS: GraphSAGE keeps and edits the diagonal (STEGraphSAGE, gnn/models/models.py:135, 160-180)
  // stored 0/1 adjacency A (rows) and its transpose; AT aliases A when symmetric
  lgnn::Csr A, AT;
  lgnn::DevBuf A_rowptr, A_col, AT_rowptr, AT_col, val_fwd, val_bwd, deg_scale;
  // propagation matrix P (forward) and P^T (backward) views into the buffers above
  lgnn::Csr P, PT;
  // model
  int L = 0;
  int64_t dims[lgnn::kMaxLayers + 1] = {};
  int64_t in_dim[lgnn::kMaxLayers] = {};  // columns of weight l (2*dims[l] for GraphSAGE)
  const float* W[lgnn::kMaxLayers] = {};
  const float* b[lgnn::kMaxLayers] = {};
  const float* X = nullptr;
  int act = 0, lik = 0;
  int64_t n_params = 0;
  lgnn::DevBuf Wt[lgnn::kMaxLayers];  // W_l^T [in_l, out_l] (forward GEMM operand)
  // optional pieces of BaseGNN.forward (gnn/models/base_gnn.py:86-113, 141-149), bound by lgnn_bind_extras:
  // x = res_l(x) + conv_l(adj, x); x = norms[l](x); x = act(x) for every hidden layer l < L-1
  bool has_res = false;
  int norm = 0;            // LGNN_NORM_*
  float norm_eps = 1e-5f;
  const float* Wr[lgnn::kMaxLayers] = {};  // res.{l}.weight [dims[l+1], dims[l]]
  const float* br[lgnn::kMaxLayers] = {};
  const float* norm_w[lgnn::kMaxLayers] = {};
  const float* norm_b[lgnn::kMaxLayers] = {};
  const float* norm_mean[lgnn::kMaxLayers] = {};  // BatchNorm1d running statistics (eval mode)
  const float* norm_var[lgnn::kMaxLayers] = {};
  lgnn::DevBuf Wrt[lgnn::kMaxLayers];    // GCN: Wr_l^T [dims[l], dims[l+1]] (forward GEMM operand)
  // GraphSAGE with res: convs.{l}.lin and res.{l} read the same rows, so the forward and the backward use ONE combined
  // weight  Wcomb_l = W_l + [Wr_l | 0]  [dims[l+1], 2 dims[l]] (row major; its transpose goes to Wt[l]) and bias b_l + br_l
  lgnn::DevBuf Wcomb[lgnn::kMaxLayers], bcomb[lgnn::kMaxLayers];
  bool extras() const { return has_res || norm != 0; }
  int n_blocks() const { return has_res ? 2 * L - 1 : L; }  // KFAC blocks: convs.{0..L-1}.lin, then res.{0..L-2}
  const float* Wback(int l) const {  // what the backward through layer l multiplies with
    return (has_res && kind == LGNN_KIND_SAGE && l < L - 1) ? Wcomb[l].as<float>() : W[l];
  }
  lgnn::ForwardCache fc;
  lgnn::Workspace ws;
  int64_t ws_limit = int64_t(32) << 30;  // backward planes (ping + pong) per class chunk: 288 GB of HBM, keep chunks large
  // rows of P^T with more than kLongRow stored entries (hubs), built once on first use (longrows.hip)
  int64_t cov_chunk_pairs = 0;     // chunk pairs the last lgnn_glm_covariance computed
  bool last_route_paths = false;   // the last KFAC accumulate took the two-hop path route
  int last_top_kernel = 0;         // ... and its top layer ran on 0: seed_spmm_gram_kernel, 1: top_tiles_kernel, 2: top_pairs_kernel
  double two_hop_max = -1.0;       // largest number of 2-hop paths starting at one node (same count pass)
  double pair_hop_max = -1.0;      // largest number of samples one sample can share a node with: P row, then P^T rows (same pass)
  double two_hop = -1.0;           // number of 2-hop paths n <- v <- m of the graph (-1: not counted yet; paths.hip)
  int64_t n_long = -1;             // -1: not looked at yet
  int64_t n_long_tasks = 0;
  lgnn::DevBuf long_rows, long_slot, long_tasks, hub;
  // top-layer kernel (kfac_top.hip): hubs with more than kTopSlice entries are cut into slices; their node ids, count, and the
  // number of slices over all of them (host copies); per-batch task list and partial tiles
  lgnn::DevBuf top_multi, top_tasks, top_task_count, top_cnt, top_offs, top_hub_tiles;
  int64_t n_top_multi = 0, n_top_slices = 0;
  // the same list for the forward matrix P (the forward SpMMs)
  int64_t n_long_fwd = -1;
  lgnn::DevBuf long_rows_fwd;
  // timing of the dominant kernel
  bool timing = false;
  std::vector<hipEvent_t> ev;   // pairs (start, stop), grown on demand
  size_t ev_used = 0;           // events recorded since the last reset
  int64_t ev_planes = 0;
  lgnn::BatchCache bcache;
  lgnn::TrainState tr;
  lgnn::SampledState sf;
  // every DevBuf the context owns (the batch cache reports its own bytes: lgnn_batch_cache_stats)
  template <class F> void each_buf(F&& f) const {
    for (int l = 0; l < lgnn::kMaxLayers; ++l) { f(Wt[l]); f(Wrt[l]); f(Wcomb[l]); f(bcomb[l]); }
    f(A_rowptr); f(A_col); f(AT_rowptr); f(AT_col); f(val_fwd); f(val_bwd); f(deg_scale);
    f(long_rows); f(long_slot); f(long_tasks); f(hub); f(long_rows_fwd);
    f(top_multi); f(top_tasks); f(top_task_count); f(top_cnt); f(top_offs); f(top_hub_tiles);
    fc.each_buf(f); ws.each_buf(f); tr.each_buf(f); sf.each_buf(f);
  }
  ~lgnn_ctx();  // the timing events and the batch cache; the buffers free themselves
};

namespace lgnn {

struct SpmmArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  int64_t nrows;
  const float* in;
  int64_t in_ld;
  int64_t in_plane_stride;
  float* out;
  int64_t out_ld;
  int64_t out_plane_stride;
  int64_t width;
  const float* self;  // optional [plane][r][self_ld]
  int64_t self_ld;
  int64_t self_plane_stride;
  const float* hact;  // optional: multiply by act'(hact[r]) (shared by all planes)
  int64_t hact_ld;
  int act;
  int out_act;  // -1 none, else apply activation to the result
  // rows with more than kLongRow stored entries (hubs), optional: the row kernel skips them and a side kernel with a
  // whole workgroup per row writes them (vector path only)
  const int32_t* long_rows; int64_t n_long;
  // entries whose value is exactly zero are not gathered (per-batch copies of P^T's values with the columns of all-zero
  // source rows zeroed: at the products shape 99.6 % of the first backward SpMM's entries)
  bool skip_zero;
};

struct FusedArgs {
  const int32_t* rowptr; const int32_t* col; const float* val;
  int64_t nrows;     // rows per plane (N)
  int64_t nplanes;
  const float* in; int64_t in_ld; int64_t in_plane_stride;
  float* store; int64_t store_ld; int64_t store_plane_stride;  // optional
  const float* self; int64_t self_ld; int64_t self_plane_stride;  // optional
  const float* hact; int64_t hact_ld; int act;                    // optional
  // GraphSAGE fast path of the 256-wide kernel (both set): rows whose flag is 0 have an all-zero self row (not read);
  // ReLU derivative from bit masks [nrows][mask_words] instead of the float activations
  const uint8_t* self_rows; const uint32_t* mask_bits; int mask_words;
  int64_t width;     // D <= DT
  float* scratch;    // [D, D]
  int unused_;       // (keeps the fields below at their kernel-argument offsets: shifted by 8 bytes, hipcc merges the hub
                     //  instances' scalar argument loads differently and spills SGPRs in spmm_gram256_kernel)
  // 256-wide kernel: rows with more than 64 stored entries arrive finished from long_rows_spmm (longrows.hip):
  // long_slot[row] = slot in hub (-1: ordinary row), hub [plane][n_long][width]
  const int32_t* long_slot; const float* hub; int64_t hub_plane_stride; int64_t n_long;
  // 256-wide kernel, GraphSAGE fast path: only the rows listed here can be non-zero (the batch nodes and their neighbours:
  // 58 % of the rows at the arxiv shape) -- a block is 32 LISTED rows, the others are never visited.  count on the device.
  const int32_t* row_list; const int32_t* row_count;
};

struct BackGemmArgs {
  const float* G;   // planes [P][N][K]
  const float* W;   // [K][ldw] row major, Nout columns used
  int64_t ldw;
  float* U;         // planes [P][N + 1][Nout]: row N of a plane is a spare row (takes the stores of padding rows)
  int64_t u_plane_stride;  // floats between planes of U, >= (N + 1) * Nout
  int64_t N, K, Nout;
  int64_t planes;
  const int32_t* rows;      // optional sorted list of active nodes (null: all N)
  const int32_t* na_dev;    // device count of `rows`
  const uint32_t* mask_bits; int64_t mask_words;  // ReLU mask bits of h (or null)
  const float* hact; int64_t hact_ld; int act;    // float activations otherwise
};
bool backgemm_supported(int64_t K, int64_t Nout, bool with_mask);
int launch_backgemm(const BackGemmArgs& g, hipStream_t s);
int launch_relu_mask_bits(const float* h, int64_t ld, int64_t N, int64_t H, uint32_t* bits, hipStream_t s);
// out[0:count) = sorted indices i with flags[i] != 0; *count_dev = count   (graph.hip, rocPRIM select)
int compact_flags(const uint8_t* flags, int64_t n, int32_t* out, int32_t* count_dev, DevBuf& tmp, hipStream_t s);
// the reserve-plus-select half of a row list: list / count = the sorted ids of the rows flagged in flags [N] (graph.hip) ...
int compact_rows(lgnn_ctx* h, const uint8_t* flags, DevBuf& list, DevBuf& count, hipStream_t s);
// ... for the workspace's own triple: ws.act_list / ws.act_count = the compacted list of the rows flagged in ws.active
int compact_active_rows(lgnn_ctx* h, hipStream_t s);
int kfac_top_planes(lgnn_ctx* h, const int64_t* idx, int64_t M, bool fork_exact, float* g, hipStream_t s);  // kfac_top.hip
int exclusive_scan_i32(int32_t* in, int32_t* out, int64_t n, DevBuf& tmp, hipStream_t s);  // graph.hip, rocPRIM

// ---- graph.hip -----------------------------------------------------------------------
int graph_build(lgnn_ctx* h, const int64_t* edge_index, int64_t E, hipStream_t s);
int graph_values(lgnn_ctx* h, bool same, hipStream_t s);
int graph_update(lgnn_ctx* h, const int64_t* fi, const int64_t* fj, const uint8_t* st, int64_t K, hipStream_t s);

// ---- dense [N, N] adjacency gradient (lora.hip) -----------------------------------------------------------------------------
// out[orow(t) * ldo + b] += sum_c sum_k L[c * l_stride + lrow(t) * l_ld + k] * R[c * r_stride + b * r_ld + k]  (+ rowc[orow * rowc_ld])
// for list entries t < nrows (or *nrows_dev), b < ncols; orow(t) = orows ? orows[t] : t, lrow(t) = lrows ? lrows[t] : orow(t).
// Output rows must be distinct within a launch.
struct DenseNtArgs {
  float* out = nullptr;
  int64_t ldo = 0, ncols = 0, nrows = 0;
  const int32_t* nrows_dev = nullptr;
  const int32_t* orows = nullptr;
  const int32_t* lrows = nullptr;
  const float* L = nullptr;
  int64_t l_ld = 0, l_stride = 0;
  const float* R = nullptr;
  int64_t r_ld = 0, r_stride = 0;
  int64_t width = 0, nplanes = 1;
  const float* rowc = nullptr;
  int64_t rowc_ld = 0;
};
int launch_dense_nt(const DenseNtArgs& g, hipStream_t s);
int launch_dense_diag_pair(const int64_t* idx, int64_t m0, int64_t mc, int64_t N, const int32_t* pos, const int32_t* mult,
                           const float* mask, int64_t H, const float* PX, int64_t ldx, const float* rowsum, int64_t F,
                           const float* H1p, int64_t ldh, const float* T, const float* phibar, int64_t row0, int64_t row1,
                           float* out, hipStream_t s);  // out: the rows [row0, row1) of the grid
int launch_gp_rowcol(lgnn_ctx* h, const float* gP, float* rs, float* cs, hipStream_t s);  // adjgrad.hip
int dense_adj_finish(lgnn_ctx* h, float* G, hipStream_t s);

// ---- kernels (launchers) -------------------------------------------------------------
// out[r, 0:width) = sum_j val[j] * in[col[j], 0:width)   for r in [0, nrows)
// epilogue: 0 none, 1 relu, 2 tanh
int launch_spmm(const Csr& m, int64_t nrows, const float* in, int64_t in_ld, float* out, int64_t out_ld,
                int64_t width, int epilogue, hipStream_t s, const int32_t* long_rows = nullptr, int64_t n_long = 0);
// rowsum of the CSR values
int launch_csr_rowsum(const Csr& m, int64_t nrows, float* out, hipStream_t s);

// C[R, Nout] = A[R, K] @ B[K, Nout] (+ bias[Nout]) (* dact(Hact[r / rows_per_node]))
struct GemmEpilogue {
  const float* bias = nullptr;
  const float* hact = nullptr;  // activation output of the layer below, [N, Nout] (ld = hact_ld)
  int64_t hact_ld = 0;
  int act = 0;                  // LGNN_ACT_*
  int64_t hact_row_mod = 0;     // hact row = r % hact_row_mod (planes are [c][n][w]); 0 -> r
  int out_act = -1;             // apply activation to the result itself (-1 none)
  const uint8_t* row_active = nullptr;  // optional [hact rows]: rows flagged 0 are neither computed on nor written
  bool no_atomics = false;              // never split K over workgroups that combine with float atomics: the result is the
                                        // same bits on every run (training path; fewer workgroups at few-tile, long-K shapes)
};
int launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t R,
                int64_t K, int64_t Nout, const GemmEpilogue& ep, hipStream_t s);
// C[0 : R) = alpha A[0 : R) B with R = *r_dev * r_mul (<= rows_bound) read on the device
int launch_gemm_devrows(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t rows_bound,
                        const int32_t* r_dev, int64_t r_mul, int64_t K, int64_t Nout, float alpha, hipStream_t s);
// the same on the listed nodes of every plane ([plane][plane_rows][.] in A and C), list length read on the device
int launch_gemm_listed(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t planes,
                       int64_t plane_rows, const int32_t* list, const int32_t* na_dev, int64_t K, int64_t Nout,
                       const GemmEpilogue& ep, hipStream_t s);

// scratch[D, D] (upper sub-tiles) += X[0:R, col0:col0+D)^T X[...]; X row-major with ld
int launch_gram(const float* X, int64_t ld, int64_t R, int64_t D, float* scratch, hipStream_t s);
// out[i,j] += scale * (X^T X)[i,j] on the upper sub-tiles, without atomics when the rows are not split
int launch_gram_scaled(const float* X, int64_t ld, int64_t R, int64_t D, float* out, float scale, hipStream_t s);
// nz weighted Grams over the same rows: out[z] += scale * zscale[z] * X^T diag(row_scale[z]^2) X (upper sub-tiles)
int launch_gram_batched(const float* X, int64_t ld, int64_t R, int64_t D, float* out, int64_t out_zstride, int64_t nz,
                        const float* row_scale, const float* zscale, float scale, hipStream_t s);
// lower triangle <- upper triangle
int launch_symmetrize_upper(float* H, int64_t D, hipStream_t s);
// out[i,j] += scale * scratch[min(i,j), max(i,j)]
int launch_sym_accumulate(const float* scratch, int64_t D, float scale, float* out, hipStream_t s, int64_t scratch_ld = 0);
// fused: rows r=(plane, n): y = sum_j val*in_plane[col[j]]; scratch += y^T y; optional store of y
int launch_spmm_ex(const SpmmArgs& a, int64_t nplanes, hipStream_t s);
int launch_spmm_gram_ex(const FusedArgs& a, hipStream_t s);
int launch_spmm_gram256(const FusedArgs& a, hipStream_t s);  // fused256.hip
// `rows`: rows per plane incl. a spare row where one exists; planes wider than 128 columns go through 32-bit buffer
// offsets (fused256.hip), so rows * in_ld * 4 must stay below 4 GiB there -- otherwise the unfused path takes over
bool fused_supported(int64_t width, int64_t in_ld, int64_t in_plane_stride, const void* in, int64_t rows);
int launch_spmm_gram(const Csr& m, int64_t nrows, int64_t nplanes, const float* in, float* store_or_null,
                     int64_t width, float* scratch, hipStream_t s);

int launch_transpose(const float* in, int64_t rows, int64_t cols, float* out, hipStream_t s);
int launch_act_deriv(const float* h, int64_t ld, int64_t N, int64_t H, int act, float* out, hipStream_t s);
int launch_fill_i32(int32_t* p, int64_t n, int32_t v, hipStream_t s);
int launch_gather_rows(const float* in, int64_t ld, int64_t nrows_in, const int64_t* idx, int64_t M, int64_t width,
                       float* out, int* bad_flag, hipStream_t s);

// ---- resnorm.hip: row-local pieces of models with res / norm (gnn/models/base_gnn.py:141-149) ------------------
// h[n] = act(gamma * xhat[n] + beta), xhat = (s[n] - mean) * rstd; LayerNorm: per-row statistics (saved in rstd [N]);
// eval-mode BatchNorm1d: running statistics (rstd [width], written here too)
int launch_norm_forward(lgnn_ctx* h, int layer, const float* spre, int64_t s_ld, float* out, int64_t out_ld, hipStream_t s);
// U [rows, width] (rows = planes * N, node = row % N), in place:
//   t = U (+ add);  if mask: t *= act'(h_{layer+1}[node]);  U = norm_backward_layer(t)
int launch_resnorm_backward(lgnn_ctx* h, int layer, float* U, int64_t ld, int64_t rows, const float* add, bool mask,
                            hipStream_t s);
int build_sage_res_weights(lgnn_ctx* h, int layer, hipStream_t s);  // Wcomb / bcomb of a GraphSAGE layer with res
// ---- longrows.hip -----------------------------------------------------------------------
constexpr int kLongRow = 64;
constexpr int kTopSlice = 128;  // stored entries of a hub row per top-layer task  // rows of P^T with more stored entries leave the fused kernel's per-wave gather
int long_rows_ensure(lgnn_ctx* h, hipStream_t s);  // builds h->long_* once (synchronises the stream that one time)
int long_rows_fwd_ensure(lgnn_ctx* h, hipStream_t s);  // the list of long rows of P (forward SpMMs)
// hub[plane][slot][0:width) = sum_j val[j] * in[plane][col[j]][0:width) for the long rows of P^T
int launch_long_rows_spmm(lgnn_ctx* h, const float* val, const float* in, int64_t in_ld, int64_t in_plane_stride,
                          int64_t nplanes, int64_t width, hipStream_t s);
// ---- kfac.hip (its kernels and launchers: kfac_seed.hip, kfac_top.hip; what those three share: kfac.h) ----------
struct KfacPlan {
  bool seeds_on_the_fly;       // GCN top layer rebuilds the seed blocks from probabilities + logits
  bool sage_compact;           // GraphSAGE top level over the batch nodes only (compacted backward GEMM + fused MODE 1)
  bool need_pong;              // the second plane buffer is written by some step
  bool paths;                  // 2-layer GCN, ReLU, 128 < H <= 256, C <= 64: B_0 from the batch's 2-hop paths (paths.hip, paths_fused.hip),
                               // no class planes, no backward GEMM, no gather of planes
  bool fuse[kMaxLayers];       // step l (l = L-1 .. 1): fused SpMM^T -> Gram kernel (else SpMM + Gram through HBM)
  bool backgemm[kMaxLayers];   // step l: compacted producer / consumer backward GEMM (else the generic GEMM)
  int64_t maxw, cc_max;        // widest GEMM output of the lower layers; class planes per chunk under the workspace cap
};
KfacPlan plan_kfac(int kind, int L, int64_t N, int64_t nnz, const int64_t* dims, int act, bool no_fuse, int64_t ws_limit,
                   bool no_paths = false);
// empirical / Monte-Carlo Fisher variant of the KFAC accumulate (curvlinops/kfac.py:663-674)
struct KfacFisherOpts {
  const void* y_seed;   // labels int64 [M] (classification) / fp32 targets [M, C] (regression) the gradient seed uses
  float resid_scale;    // seed = resid_scale * d loss_n / d f_n  (p - onehot resp. f - y)
  float b_scale;        // B_out += b_scale * g^T g               (1 / mc_samples)
  bool add_loss_and_A;  // this call also adds the loss of the true labels `y` and the A increment
};
struct KfacShare { int64_t begin, end, count; };  // parts [begin, end) of `count` equal parts of a batch (lgnn_kfac_accumulate_share)
int kfac_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train, uint32_t flags,
                    int64_t class_begin, int64_t class_end, float* const* A_out, float* const* B_out, float* loss_out,
                    hipStream_t s, const KfacFisherOpts* fisher = nullptr, const KfacShare* share = nullptr);
// kfac_seed.hip: the start and the end of every batch
int batch_prologue(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool want_seeds, bool fork_exact,
                   float* loss_out, hipStream_t s, const void* y_seed = nullptr, float resid_scale = 1.0f,
                   const int64_t* guard_ids = nullptr);  // guard_ids: the ids a cache entry was built from (compared on the device)
int batch_epilogue(lgnn_ctx* h, const int64_t* idx, int64_t M, hipStream_t s);
// timing hook (lgnn_enable_kernel_timing): one HIP event on the launch stream; callers bracket the dominant kernel
int record_event(lgnn_ctx* h, hipStream_t s);
// ---- batchcache.hip -----------------------------------------------------------------------
size_t batch_cache_budget();                 // LGNN_BATCH_CACHE_MB in bytes, read per call (0: off)
void batch_cache_clear(lgnn_ctx* h);         // the graph changed / the context goes: every entry and every remembered tag
int batch_cache_lookup(lgnn_ctx* h, uint64_t tag, const int64_t* idx, int64_t M, BatchEntry** out, hipStream_t s);
int batch_cache_store_active(lgnn_ctx* h, BatchEntry* e, hipStream_t s);   // from ws.active / act_list / act_count
int batch_cache_store_paths(lgnn_ctx* h, BatchEntry* e, int64_t cap, bool have_nodes, hipStream_t s);  // path list, R, node list
int batch_cache_store_pairs(lgnn_ctx* h, BatchEntry* e, hipStream_t s);   // from ws.pair_* (an entry that has its path part)
void batch_cache_drop_paths(lgnn_ctx* h, BatchEntry* e);
// ---- gram_stream.hip ----------------------------------------------------------------------
// scratch [width, width] (upper 32 x 32 sub-tiles) += Y^T Y for rows of `width` floats (row stride ld), 128 < width <= 256:
// all eight waves of a persistent workgroup per CU on the matrix pipes, row blocks by LDS-DMA
int launch_gram256_stream(const float* Y, int64_t ld, int64_t rows, int64_t width, float* scratch, hipStream_t s,
                          const int32_t* gate = nullptr, int64_t gate_cap = 0);
// ---- paths.hip (its kernels: paths_fused.hip, paths_overflow.hip; what those three share: paths.h) ----------
bool paths_supported(int kind, int L, const int64_t* dims, int act, int64_t nnz);
int two_hop_ensure(lgnn_ctx* h, hipStream_t s);   // h->two_hop = 2-hop paths of the graph, counted once (one synchronisation)
bool paths_pay(const lgnn_ctx* h, int64_t M);     // expected paths per destination node of a batch of M small enough
constexpr int kCoefStride = 64;  // classes per coefficient kind (zero padded): the class window [cb, cb + 64) of a call
constexpr int kCoefRow = 256;    // floats per sample in the coefficient table: (alpha | -beta | -gamma | pad) = 1 KiB, one LDS-DMA piece
struct PathR { const int32_t* rptr; const int32_t* r_m; const float* r_w; };  // R = P^T[:, batch] as CSR over the nodes
// The GCN top layer of the path route on the matrix pipes (toptiles.hip): scratch [C, C] += B_1 of the classes [cb, ce) from R
// and the tables path_tables_kernel has written for the same (cb, ce) (ws.path_coef, ws.path_up).
int launch_top_tiles(lgnn_ctx* h, const PathR& r, int64_t M, int64_t cb, int64_t ce, const int32_t* act_list,
                     const int32_t* act_count, float* scratch, hipStream_t s);
// The same sum from sample pairs (toppairs.hip): s_m [M], the pairs (m, m', w w') of samples that share a node, their number
struct TopPairs { const float* sq; const int32_t* pm; const int32_t* pm2; const float* pw; const int32_t* npairs; };
int64_t top_pairs_bound(const lgnn_ctx* h, int64_t M);  // a host-known bound of a batch's pairs (-1: none)
bool top_pairs_fit(const lgnn_ctx* h, int64_t M);       // ... fits the pair list (LGNN_PAIR_LIST_CAP, read per call)
int build_top_pairs(lgnn_ctx* h, const int64_t* idx, int64_t M, const PathR& r, TopPairs& out, hipStream_t s);  // into ws.pair_*
int launch_top_pairs(lgnn_ctx* h, const TopPairs& p, int64_t M, int64_t cb, int64_t ce, float* scratch, hipStream_t s);
// the batch's active rows, B_1 scratch; pairs: top_pairs_kernel instead of top_tiles_kernel
struct TopTilesReq { const int32_t* act_list; const int32_t* act_count; float* scratch; bool pairs; };
// scratch [H, H] += B_0 of this batch's class columns [cb, ce) (seed_mode: 0 upstream, 1 fork exact, 2 regression)
// (top: also run the top layer from the tables and R built here -- launch_top_tiles / launch_top_pairs -- once both are in place)
// (nb, ne: the destination nodes whose Y_n^T Y_n this call adds -- B_0 is a sum over nodes: the multi-GPU cut of these routes)
// (entry: the batch's cache entry or null; its path part is used if present and built into it otherwise; *built is set then)
int kfac_paths_first_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int seed_mode, int64_t cb, int64_t ce, float* scratch,
                           hipStream_t s, int64_t nb = 0, int64_t ne = -1, BatchEntry* entry = nullptr, bool* built = nullptr,
                           const TopTilesReq* top = nullptr);
int kfac_paths_first_layer_sage(lgnn_ctx* h, const int64_t* idx, int64_t M, int seed_mode, int64_t cb, int64_t ce,
                                float* scratch, hipStream_t s, int64_t nb = 0, int64_t ne = -1);  // GraphSAGE: one-hop paths through the same fused kernel
// ---- forward.hip ------------------------------------------------------------------------
int forward_ensure(lgnn_ctx* h, hipStream_t s);
int forward_ensure_grams(lgnn_ctx* h, hipStream_t s);
int forward_ensure_aux(lgnn_ctx* h, hipStream_t s);
int forward_input_view(lgnn_ctx* h, hipStream_t s);  // GCN: lin_in_p[0] / lin_in_ld[0] (X or its padded copy)
int build_px(lgnn_ctx* h, hipStream_t s);            // rowsum(P) and (GCN) [P X | rowsum(P) | 0]: graph and X only
int ensure_wt(lgnn_ctx* h, hipStream_t s);           // transposed weights (forward GEMM, adjacency gradient)
// gcn2_forward.hip: small plain 2-layer GCN, forward + auxiliary products through the cached P X
bool gcn2_small_forward_supported(const lgnn_ctx* h);
int gcn2_forward_through_px(lgnn_ctx* h, hipStream_t s);
// ---- diag.hip (its kernels' launchers, which fisher.hip calls too: diag.h) --------------------------------------------------
int diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags, float* diag_out,
                    float* loss_out, hipStream_t s);
// ---- lastlayer_full.hip (launch_ll_build_phi takes a FeatView: declared in closedform.h) ----------------------------------
int lastlayer_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* H_out,
                              float* loss_out, hipStream_t s);
int lastlayer_pairs_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* S, float* Sb,
                               float* loss_out, hipStream_t s);
int lastlayer_features(lgnn_ctx* h, const int64_t* idx, int64_t M, float* out, float* f_out, hipStream_t s);
int lastlayer_pairs_place(lgnn_ctx* h, const float* S, const float* Sb, float* H_out, hipStream_t s);
// ---- fisher.hip ---------------------------------------------------------------------------
int ef_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y_seed, const void* y_loss, int64_t M, float resid_scale,
                  float scale, float* diag_out, float* full_out, float* grads_out, float* loss_out, hipStream_t s);
// ---- lastlayer_kron.hip -----------------------------------------------------------------
int lastlayer_kron_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train, uint32_t flags,
                              float* A_out, float* B_out, float* Bb_out, float* loss_out, hipStream_t s);
int lastlayer_diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* diag_out, float* loss_out,
                              hipStream_t s);
// ---- jacobian.hip -----------------------------------------------------------------------
int jacobians(lgnn_ctx* h, const int64_t* idx, int64_t M, float* J, float* f_out, hipStream_t s);
// all-weights full GGN from chunks of those rows: H_out [P, P] += sum_n J_n^T Lambda_n J_n
int full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* H_out, float* loss_out, hipStream_t s);
// ---- subnet.hip -------------------------------------------------------------------------
// columns subnet[0..S) (device, caller's order) of the Jacobians: J [M, C, S]
int jacobians_subset(lgnn_ctx* h, const int64_t* idx, int64_t M, const int64_t* subnet, int64_t S, float* J, float* f_out,
                     hipStream_t s);
int subnet_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const int64_t* subnet, int64_t S,
                           float* H_out, float* loss_out, hipStream_t s);
// ---- gpkernel.hip -----------------------------------------------------------------------
// K = J(idx_a) J(idx_b)^T in the layout `flags` names (LGNN_GP_*); out [M, C] = J(idx) v
int gp_kernel(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags, float* K, int64_t ldk,
              hipStream_t s);
int gp_jvp(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* v, float* out, hipStream_t s);
// ---- glmcov.hip -------------------------------------------------------------------------
// K = J(idx_a) P^-1 J(idx_b)^T for a block-diagonal Kronecker / diagonal posterior (lgnn_glm_covariance)
int glm_covariance(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int n_blocks,
                   const float* const* QA, const float* const* QB, const float* const* S, int flags, float* K, int64_t ldk,
                   hipStream_t s);
// Out_z[i * ldo + j * o_es] = sum_k A_z[i, k] B_z[j, k] for z < batch (A_z = A + z a_bs: [Ra, K] with row stride lda, B_z
// likewise, Out_z = Out + z o_bs) on the fp32 matrix cores; no float atomics (split-K partials in ws.gp_part, added in order)
struct NtProblem {
  const float* A; int64_t lda, a_bs;
  const float* B; int64_t ldb, b_bs;
  float* Out; int64_t ldo, o_es, o_bs;
  int64_t Ra, Rb, K, batch;
  int upper_only = 0;  // Out_z is square and symmetric and the caller mirrors it: tiles strictly below the diagonal are skipped
};
int launch_nt_gemm(lgnn_ctx* h, const NtProblem& p, hipStream_t s);
// ---- ggnmat.hip -------------------------------------------------------------------------
// out [M, C, k] = J V^T;  G [k, P] += sum_n J_n^T Lambda_n J_n V^T and *loss_out += loss, for V [k, P]
int jvp_block(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V, int64_t k, float* out, hipStream_t s);
int ggn_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k, int flags, float* G,
               float* loss_out, hipStream_t s);
// ---- hessmat.hip ------------------------------------------------------------------------
// G [k, P] += R V^T, R = sum_n sum_c r_nc grad^2 f_nc: what the exact Hessian of the loss adds to the GGN (closed-form models)
int hessian_resid_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V, int64_t k, float* G,
                         hipStream_t s);
// ---- sampled.hip ------------------------------------------------------------------------
// out [S, M, C] = the logits (flags & LGNN_SAMPLED_SOFTMAX: their softmax) of S parameter vectors theta [S, n_params] at idx
int sampled_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* theta, int64_t S, uint32_t flags, float* out,
                    hipStream_t s);
// its pieces, shared with ggnmat.hip: in0 (SampledState::in0 / ldk), the needed-row list of a batch (SampledState::rows /
// count / rpos) and the CSR gather of step (c)
int sampled_ensure_input(lgnn_ctx* h, hipStream_t s);
int sampled_needed_rows(lgnn_ctx* h, const int64_t* idx, int64_t M, hipStream_t s);
struct GatherArgs {
  const int64_t* idx; int64_t M, N;
  const int32_t* rowptr; const int32_t* col; const float* val;
  const int32_t* rpos;
  const float* z; int64_t rcap, Cz, C;
  int sage, cw;                     // cw: lanes per entry group, the smallest power of two >= min(C, 64)
  const float* theta; int64_t P, offb;
  int64_t ns;                       // samples of the chunk
  float* out;                       // the chunk's [ns, M, C]
};
int launch_sampled_gather(const GatherArgs& g, hipStream_t s);
// The first-layer tile kernel of step (b): 64-row tiles of the needed rows, the first product's K stage and the hidden tile 64
// wide (rows padded to 65 floats), windows of SZW columns of z per workgroup.  ggnmat.hip's transposed products stage the same
// 64 x 64 tiles.
constexpr int SBM = 64, SBH = 64, SBK = 64, SLDT = SBK + 1, SLDH = SBH + 1, SZW = 128;
// Its linearised instance (ggnmat.hip): theta is a block of directions (dW0, db0, dW1, db1), and
//   z_i[r] = (D[r] . (in0[r] [dW0 | db0]^T)) W1^T + h[r] dW1^T
struct FwdArgs {
  static constexpr bool linearised = true;
  static constexpr bool hessian = false;
  const float* in0; int64_t ldk;
  const int32_t* rows; const int32_t* count;
  const float* theta; int64_t P;    // the chunk's first direction, floats between directions
  int64_t Fp, H;                    // columns of the first Linear's weight, its rows (1 layer: the classes)
  const float* dact; const float* h1; int64_t h1_ld;  // D = act'(s) [N, H], h [N, H] with row stride h1_ld
  const float* W1; int64_t ld1, off1, C, Cz;          // the bound W1 (row stride ld1); dW1 of a direction at theta_i + off1
  float* z; int64_t rcap;           // z[(i * rcap + t) * Cz + c]   (1 layer: u[(i * rcap + m) * H + c])
};
int launch_first_layer(const FwdArgs& a, bool two, int64_t ndir, hipStream_t s);
// Its second-derivative instance (hessmat.hip, 2-layer models): theta is a block of directions, dS = in0 [dW0 | db0]^T, and
//   E_i[t] = D . dS     T_i[t] = (G[t] dW1) . D + GW1[t] . D2 . dS     (D2 = act''(s): 0 for ReLU, -2 h D for tanh)
// for the listed rows t; G dW1 runs on the same MFMA step while dS waits in its accumulators.  Nothing but E and T is written.
struct HessArgs {
  static constexpr bool linearised = false;
  static constexpr bool hessian = true;
  const float* in0; int64_t ldk;
  const int32_t* rows; const int32_t* count;
  const float* theta; int64_t P;
  int64_t Fp, H;
  const float* dact; const float* h1; int64_t h1_ld; int act;
  const float* G; const float* GW1;                   // G [rcap, Cz], GW1 [rcap, H], rows listed like `rows`
  int64_t ld1, off1, C, Cz;                           // dW1 of a direction at theta_i + off1, row stride ld1
  float* E; float* T; int64_t rcap;                   // [(i * rcap + t) * H + j]
};
int launch_first_layer(const HessArgs& a, int64_t ndir, hipStream_t s);
// ---- fulladj.hip ------------------------------------------------------------------------
// full posterior: Kn [mc][C][C] = (J_m Gamma) J_m^T (zeroed here, float atomics) and R [mc * C, P] = 2 Lambda_m (J_m Gamma) of a
// chunk's Jacobian rows J [mc * C, P]; Lambda_m from the softmax of logits [N, C] at idx[m]; C <= 127
int launch_full_directions(const float* J, const float* Gamma, const int64_t* idx, const float* logits, int64_t N,
                           int64_t mc, int64_t C, int64_t P, float* R, float* Kn, hipStream_t s);
// ---- eigh.hip ---------------------------------------------------------------------------
void* blas_handle(hipStream_t s);  // the process-wide rocblas_handle, bound to `s`
// ---- adjgrad.hip ------------------------------------------------------------------------
// C_rm[R, Nout] = alpha * A_rm[R, K] * B_rm[K, Nout] + beta * C_rm (rocBLAS on blas_handle(s))
int sgemm_rm(hipStream_t s, int64_t R, int64_t Nout, int64_t K, float alpha, const float* A, int64_t lda, const float* B,
             int64_t ldb, float beta, float* Cm, int64_t ldc);

}  // namespace lgnn
