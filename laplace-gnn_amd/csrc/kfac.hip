// KFAC factors of one mini-batch for L-layer GCN / GraphSAGE models.
//
// Reference: CurvlinopsInterface.kron (laplace/curvature/curvlinops.py:77-108) ->
// KFACLinearOperator._compute_kfac (curvlinops/kfac.py:540-581): forward pre-hooks accumulate the
// input covariance of every nn.Linear (kfac.py:819-875), then one backward pass per class column c
// of the loss-Hessian square root (kfac.py:653-661) accumulates g^T g at every Linear output
// (kfac.py:777-817).  The reference runs C dense N x N backward passes through autograd; here the
// model family is closed form, so the C right-hand sides travel together as class-major planes
// T[c][n][w] through explicit kernels:
//     seeds  V[m][c][k]                 (softmax + fork-exact v_c, one wave per sample)
//     top    g_{L-1} = P^T scatter(V)   (seed SpMM: only neighbours that are batch nodes contribute)
//     down   up = act'(h) * (g_l W_l)   (fp32 MFMA GEMM, epilogue mask)
//            g_{l-1} = P^T up           (fused SpMM^T -> LDS tile -> MFMA Gram; g never hits HBM
//                                        unless a lower layer needs it)
//
// This file: the plan, the steps of one accumulate over one state struct and the driver.  The batch prologue / epilogue and
// the seed kernels are in kfac_seed.hip, the top layer's kernels and the row-list launchers in kfac_top.hip (kfac.h).
#include "kfac.h"

namespace lgnn {

namespace {

// values of P^T with the columns of all-zero source rows removed: the fused SpMM issues no load for them
__global__ void mask_values_kernel(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz,
                                   const uint8_t* __restrict__ active, const int32_t* __restrict__ pos,
                                   float* __restrict__ out) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < nnz; p += stride) {
    const int32_t j = col[p];
    const bool on = active ? active[j] != 0 : pos[j] != INT32_MAX;
    out[p] = on ? val[p] : 0.f;
  }
}

int launch_mask_values(lgnn_ctx* h, const uint8_t* active, float* out, hipStream_t s) {
  hipLaunchKernelGGL(mask_values_kernel, dim3(unsigned(std::min<int64_t>(cdiv(h->nnz, 256), 4096))), dim3(256), 0, s,
                     h->PT.col, h->PT.val, h->nnz, active, h->ws.pos.as<int32_t>(), out);
  LGNN_HIP_CHECK(hipGetLastError());
  return 0;
}

// zero the listed rows of every plane again (16 bytes per thread): U[p][rows[i]][0 .. width)
__global__ void clear_rows_kernel(float* __restrict__ U, int64_t plane_stride, int64_t width, int64_t planes,
                                  const int32_t* __restrict__ rows, const int32_t* __restrict__ count) {
  const int64_t w4 = width / 4, per_plane = int64_t(*count) * w4, total = per_plane * planes;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t p = q / per_plane, r = q - p * per_plane;
    const int64_t i = r / w4, c4 = r - i * w4;
    *reinterpret_cast<float4*>(U + p * plane_stride + int64_t(rows[i]) * width + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// 256-wide fused kernel: rows of P^T with more than kLongRow stored entries are computed by whole workgroups first
// (longrows.hip) and handed over as finished rows; the list is built on the first call (one stream synchronisation).
int attach_long_rows(lgnn_ctx* h, FusedArgs& a, hipStream_t s) {
  if (a.width <= 128) return 0;  // the narrower kernels keep their own row loop
  LGNN_CALL(long_rows_ensure(h, s));
  if (h->n_long <= 0) return 0;
  LGNN_CALL(launch_long_rows_spmm(h, a.val, a.in, a.in_ld, a.in_plane_stride, a.nplanes, a.width, s));
  a.long_slot = h->long_slot.as<int32_t>();
  a.hub = h->hub.as<float>();
  a.hub_plane_stride = h->n_long * a.width;
  a.n_long = h->n_long;
  return 0;
}

// One accumulate's state.  kfac_resolve fills it in; after that only the step that owns a field writes it.
struct KfacBatch {
  // the call's arguments
  lgnn_ctx* h; const int64_t* idx; const void* y; int64_t M, n_train; uint32_t flags;
  float* const* A_out; float* const* B_out; float* loss_out; hipStream_t s;
  const KfacFisherOpts* fisher; const KfacShare* share;
  // kfac_resolve
  uint64_t batch_tag;         // names the batch of THIS call only
  KfacPlan plan;
  int64_t cb, ce;             // the class planes this call builds
  int64_t nb, ne;             // path routes: the destination nodes whose Y_n^T Y_n this call adds
  bool first;                 // this call holds the share with class 0 (or part 0)
  bool once;                  // ... and adds what exists once per batch: the loss and the A increment
  bool no_fuse, fork_exact;
  bool share_nodes;           // share mode on a path route: the cut is over nodes [nb, ne), all classes
  bool no_classes;            // share mode with more parts than classes: only what exists once per batch is left
  bool seeds_on_the_fly;      // GCN top layer rebuilds the seed blocks; every other route reads them from ws.seeds
  bool paths_route;           // B_0 from the batch's paths (paths.hip): no class planes below the top layer
  bool be_route;              // the route builds the lists a batch-structure cache entry holds
  BatchEntry* be;             // this batch's entry or null
  bool be_built;              // (top layer, path route) the call filled part of the entry
  // top layer
  ActiveRows rows;            // GCN: the rows of g_{L-1} that are not identically zero -- the workspace's, or the cache entry's on
                              // a hit; the list may come late (kfac_lower_prepare).  GraphSAGE's compact route: the batch nodes
  float* gtop;                // planes [C][N][C]
  bool top_tiles, top_pairs;  // GCN path route: B_{L-1} from top_tiles_kernel / top_pairs_kernel, launched by the path route
  // kfac_lower_prepare
  const float* val_top;       // P^T's values with the columns of all-zero rows of g_{L-1} zeroed (or P^T's own)
  const uint8_t* row_active;  // GCN: the flags the first backward GEMM's epilogue reads (null: every row is computed)
  // the backward levels
  bool second_level_built;    // GraphSAGE: out_flags / out_list / val_act2 exist for this batch
};

// Argument checks, routes, plan, the share's cut and the cache lookup -- everything that is decided before the first launch.
int kfac_resolve(KfacBatch& b, int64_t cb, int64_t ce) {
  lgnn_ctx* h = b.h;
  b.batch_tag = h->bcache.pending_tag;
  h->bcache.pending_tag = 0;
  const int64_t* idx = b.idx;
  const void* y = b.y;
  const int64_t M = b.M, n_train = b.n_train;
  const uint32_t flags = b.flags;
  float* const* A_out = b.A_out;
  float* const* B_out = b.B_out;
  float* loss_out = b.loss_out;
  const KfacFisherOpts* fisher = b.fisher;
  const KfacShare* share = b.share;
  hipStream_t s = b.s;
  LGNN_REQUIRE(M > 0 && idx && (y || (fisher && !fisher->add_loss_and_A)), "empty batch or null batch pointers");
  LGNN_REQUIRE(h->L > 0, "no model bound");
  // Share mode (lgnn_kfac_accumulate_share): parts [begin, end) of `count` equal parts of the batch's work; HOW a batch is
  // cut is decided below, once the route is known -- destination-node ranges on the path routes (B_0 = sum_n Y_n^T Y_n:
  // nothing is computed twice), class ranges everywhere else.  Until then the range is "everything".
  LGNN_REQUIRE(!share || (share->count > 0 && share->begin >= 0 && share->begin < share->end && share->end <= share->count && !fisher),
               "share must satisfy 0 <= begin < end <= count");
  if (share) { cb = 0; ce = h->dims[h->L]; }
  LGNN_REQUIRE(cb >= 0 && cb < ce && ce <= h->dims[h->L], "class range must satisfy 0 <= begin < end <= C");
  // B_l = sum over class columns c of g_c^T g_c: a class range is an exact additive share of the batch.
  // The share that contains class 0 also carries what exists once per batch: the loss and the A increment
  // (and, for GraphSAGE, the whole top-layer Gram, which is only M*C rows).
  b.first = share ? share->begin == 0 : cb == 0;
  // empirical / MC Fisher: one plane (the gradient seed sits in column 0 of the block), B scaled by 1 / mc_samples, the
  // loss of the TRUE labels and the A increment only with the call that is told to add them
  b.once = fisher ? fisher->add_loss_and_A : b.first;
  LGNN_REQUIRE(!fisher || (cb == 0 && ce == 1 && fisher->y_seed), "internal: Fisher seeds use plane 0 only");
  LGNN_REQUIRE(n_train > 0, "n_train must be positive");
  LGNN_REQUIRE(A_out && B_out && loss_out, "null output pointers");
  // the input Grams feed the A increment, which only the share with class 0 adds (ranks of a multi-GPU job that
  // hold no such share never compute them)
  if (b.once) LGNN_CALL(forward_ensure_grams(h, s));
  else LGNN_CALL(forward_ensure(h, s));
  const int64_t N = h->N;
  const int L = h->L;
  const int64_t C = h->dims[L];
  // models with res / norm (gnn/models/base_gnn.py:141-149) take the unfused route: GEMM, row-local norm backward,
  // SpMM^T and Gram as separate kernels (resnorm.hip)
  b.no_fuse = (flags & LGNN_FLAG_NO_FUSE) != 0 || h->extras();
  LGNN_REQUIRE(M < INT32_MAX, "batch too large");

  b.fork_exact = (flags & LGNN_FLAG_FORK_EXACT_SEED) != 0;
  // the two-hop path route (paths.hip) where the shape allows it and the batch's expected number of paths makes it pay
  bool no_paths = (flags & LGNN_FLAG_NO_PATHS) != 0 || fisher != nullptr || b.no_fuse ||
                  !paths_supported(h->kind, L, h->dims, h->act, h->nnz);
  if (!no_paths && h->kind == LGNN_KIND_GCN) {  // (GraphSAGE's paths are one hop: at most nnz + (C + 1) M of them, always cheaper)
    LGNN_CALL(two_hop_ensure(h, s));
    no_paths = !paths_pay(h, M) && (flags & LGNN_FLAG_FORCE_PATHS) == 0;
  }
  b.plan = plan_kfac(h->kind, L, N, h->nnz, h->dims, h->act, b.no_fuse, h->ws_limit, no_paths);
  // share mode: the cut.  Path routes: nodes [nb, ne), all classes (the top layer's small Gram goes with part 0); otherwise
  // classes [C begin / count, C end / count) -- possibly none, then only what exists once per batch is left to do.
  b.nb = 0;
  b.ne = N;
  b.share_nodes = share && b.plan.paths;
  if (b.share_nodes) {
    b.nb = N * share->begin / share->count;
    b.ne = N * share->end / share->count;
  } else if (share) {
    cb = C * share->begin / share->count;
    ce = C * share->end / share->count;
  }
  b.cb = cb;
  b.ce = ce;
  b.no_classes = cb >= ce;  // (share mode with more parts than classes)
  // GCN, fused path: the top-layer kernel rebuilds each sample's C x C seed block from its probabilities and logits,
  // so the blocks are never written (64 MB per arxiv-shaped batch); every other path reads them from ws.seeds
  b.seeds_on_the_fly = b.plan.seeds_on_the_fly && !fisher;  // the on-the-fly rebuild knows the GGN blocks only
  b.paths_route = b.plan.paths && !fisher && (h->kind == LGNN_KIND_GCN ? b.seeds_on_the_fly : true);
  // batch-structure cache (batchcache.hip): the caller named this batch (lgnn_kfac_batch_tag) and the route builds the lists
  // an entry holds -- the GCN top layer's active rows, the path route's two-hop paths
  b.be_route = h->kind == LGNN_KIND_GCN && b.seeds_on_the_fly;
  if (b.be_route) LGNN_CALL(batch_cache_lookup(h, b.batch_tag, idx, M, &b.be, s));
  return 0;
}

// A_l += in_l^T in_l / n_train (kfac.py:870 divides by M, curvlinops.py:46-53 multiplies by M/N), and the B scratches' reset
int kfac_input_factors(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int L = h->L;
  for (int l = 0; b.once && l < L; ++l)
    LGNN_CALL(launch_sym_accumulate(h->fc.gram_raw[l].as<float>(), h->in_dim[l], 1.0f / float(b.n_train), b.A_out[l], s));
  // res.{l} sees h_l itself: its input covariance is the conv's (GCN) resp. the leading block of cat_l's (GraphSAGE)
  for (int l = 0; b.once && h->has_res && l < L - 1; ++l)
    LGNN_CALL(launch_sym_accumulate(h->fc.gram_raw[l].as<float>(), h->dims[l], 1.0f / float(b.n_train), b.A_out[L + l], s,
                                    h->in_dim[l]));
  for (int l = 0; l < L; ++l) {
    const int64_t D = h->dims[l + 1];
    LGNN_CALL(h->ws.gram_scratch[l].reserve(size_t(D) * D * 4));
    LGNN_HIP_CHECK(hipMemsetAsync(h->ws.gram_scratch[l].p, 0, size_t(D) * D * 4, s));
    if (h->has_res && h->kind == LGNN_KIND_GCN && l < L - 1) {
      LGNN_CALL(h->ws.gram_scratch_res[l].reserve(size_t(D) * D * 4));
      LGNN_HIP_CHECK(hipMemsetAsync(h->ws.gram_scratch_res[l].p, 0, size_t(D) * D * 4, s));
    }
  }
  return 0;
}

// GCN top layer: the active rows, then B_{L-1} and (unless nobody reads them) the planes g_{L-1} of the classes [cb, ce)
int kfac_top_gcn(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int64_t N = h->N, C = h->dims[h->L];
  const int L = h->L;
  LGNN_CALL(h->ws.top.reserve(size_t(N) * C * C * 4 + 16));  // + 16: the backward GEMM reads rows shifted by one float
  b.gtop = h->ws.top.as<float>();
  LGNN_CALL(h->ws.active.reserve(size_t(N)));
  float* sc = h->ws.gram_scratch[L - 1].as<float>();
  if (!b.seeds_on_the_fly) {  // seeds from memory, all N rows; the kernel leaves the row flags, the list comes late
    LGNN_CALL(launch_seed_spmm(h, b.gtop, b.cb, b.ce, s));
    b.rows.flags = h->ws.active.as<uint8_t>();
    return launch_gram(b.gtop + b.cb * N * C, C, (b.ce - b.cb) * N, C, sc, s);
  }
  // active rows first (columns of the batch nodes' P rows), then one pass over those rows only
  if (b.be && b.be->has_act) {
    b.rows = ActiveRows{b.be->active, b.be->act_list, b.be->act_count};
  } else {
    LGNN_CALL(build_row_list(h, b.idx, b.M, kRowsNeighbours, h->ws.active, h->ws.act_list, h->ws.act_count, s, &b.rows));
    if (b.be) {  // (this call goes on with the workspace's copy: the entry may be refused for its size)
      LGNN_CALL(batch_cache_store_active(h, b.be, s));
      b.be_built = true;
    }
  }
  // a single-layer model needs the Gram only -- and so does the two-hop path route (paths.hip), which never reads planes
  float* gplanes = (L > 1 && !b.paths_route) ? b.gtop : nullptr;
  const bool top_here = !b.share_nodes || b.first;  // node shares: B_{L-1} (all classes, 0.24 ms) goes with part 0
  if (L > 1 && !b.plan.fuse[L - 1] && !b.paths_route)
    // the unfused lower path reads every row of the planes: the rows this kernel skips must be zero
    LGNN_HIP_CHECK(hipMemsetAsync(b.gtop + b.cb * N * C, 0, size_t(N) * (b.ce - b.cb) * C * 4, s));
  // path route, no planes wanted, no sliced hubs: the top layer runs on the matrix pipes from the path route's tables and
  // R (toptiles.hip), launched by kfac_paths_first_layer once both are in place
  if (top_here && b.paths_route && !gplanes && C <= kCoefStride && b.nb < b.ne) {
    LGNN_CALL(long_rows_ensure(h, s));
    b.top_tiles = h->n_top_multi <= 0;
    b.top_pairs = b.top_tiles && top_pairs_fit(h, b.M);
  }
  if (top_here && !b.top_tiles) LGNN_CALL(launch_seed_spmm_gram(h, b.fork_exact, gplanes, b.cb, b.ce, sc, b.rows, s));
  return 0;
}

// GraphSAGE top layer: the last Linear's output is not propagated -- B_{L-1} is the Gram of the seed rows, the planes are
// the scattered seeds
int kfac_top_sage(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int64_t N = h->N, C = h->dims[h->L];
  const bool planes = h->L > 1 && !b.paths_route;  // (the path route reads the samples' probabilities, not seed planes)
  if (planes) {
    LGNN_CALL(h->ws.top.reserve(size_t(N) * C * C * 4 + 16));  // + 16: the backward GEMM reads rows shifted by one float
    b.gtop = h->ws.top.as<float>();
  }
  LGNN_CALL(h->ws.active.reserve(size_t(N)));
  // rows (m, c) of the accumulated seeds; rows of non-first duplicates are zero
  if (b.first) LGNN_CALL(launch_gram(h->ws.seeds.as<float>(), C, b.M * C, C, h->ws.gram_scratch[h->L - 1].as<float>(), s));
  if (planes) {
    // the compact top level reads the planes at the batch nodes only; every other path reads all rows
    if (!b.plan.sage_compact) LGNN_HIP_CHECK(hipMemsetAsync(b.gtop + b.cb * N * C, 0, size_t(N) * (b.ce - b.cb) * C * 4, s));
    LGNN_CALL(launch_scatter_seed_planes(h, b.idx, b.M, b.gtop, b.cb, b.ce, s));
  }
  return 0;
}

// 2-layer models: B_0 from the batch's 2-hop (GraphSAGE: one-hop) paths -- no class planes (paths.hip, paths_fused.hip)
int kfac_path_route(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  const int mode = h->lik == LGNN_LIK_REGRESSION ? 2 : (b.fork_exact ? 1 : 0);
  float* scratch = h->ws.gram_scratch[0].as<float>();
  if (h->kind != LGNN_KIND_GCN)
    return kfac_paths_first_layer_sage(h, b.idx, b.M, mode, b.cb, b.ce, scratch, b.s, b.nb, b.ne);
  const TopTilesReq top{b.rows.list, b.rows.count, h->ws.gram_scratch[h->L - 1].as<float>(), b.top_pairs};
  return kfac_paths_first_layer(h, b.idx, b.M, mode, b.cb, b.ce, scratch, b.s, b.nb, b.ne, b.be, &b.be_built,
                                b.top_tiles ? &top : nullptr);
}

// Before the backward levels: P^T's values for the first of them, the row lists it reads, the plane buffers.
// Source rows of the first backward plane set are non-zero only where the top-layer gradient is:
// GCN: nodes with a batch node among their P^T neighbours (flags from the top layer);
// GraphSAGE: the batch nodes themselves.  Zeroed values make the fused SpMM skip those gathers.
int kfac_lower_prepare(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int64_t N = h->N;
  const int L = h->L;
  const bool gcn = h->kind == LGNN_KIND_GCN;
  b.val_top = h->PT.val;
  b.row_active = nullptr;
  if (!b.no_fuse && h->nnz > 0) {
    LGNN_CALL(h->ws.val_act.reserve(size_t(h->nnz) * 4));
    LGNN_CALL(launch_mask_values(h, gcn ? b.rows.flags : (const uint8_t*)nullptr, h->ws.val_act.as<float>(), s));
    b.val_top = h->ws.val_act.as<float>();
    // GraphSAGE, fused path: the top-level GEMM g W_l runs over the (distinct) batch nodes only -- 6 % of the rows at
    // the arxiv shape -- through the compacted-row backward GEMM; the other rows of its output stay zero
    if (b.plan.sage_compact)
      LGNN_CALL(build_row_list(h, b.idx, b.M, kRowsBatch, h->ws.active, h->ws.act_list, h->ws.act_count, s, &b.rows));
    if (gcn) {
      b.row_active = b.rows.flags;
      if (!b.rows.list) {  // seeds from memory: the flags are seed_spmm_kernel's (ws.active)
        LGNN_CALL(compact_active_rows(h, s));
        b.rows.list = h->ws.act_list.as<int32_t>();
        b.rows.count = h->ws.act_count.as<int32_t>();
      }
    }
  }
  // The pong buffer holds g_{l-1} when a lower layer needs it (L > 2) and the SpMM output of the unfused path;
  // the fused two-layer path never touches it (plan_kfac decides, from the same per-layer flags the levels use).
  const int64_t maxw = b.plan.maxw, cc_max = b.plan.cc_max;
  for (int l = 1; l < L; ++l)
    LGNN_REQUIRE(h->fc.hact_ld[l - 1] == (h->kind == LGNN_KIND_GCN ? h->dims[l] : 2 * h->dims[l]),
                 "internal: activation row stride differs from the plan's");
  LGNN_CALL(h->ws.planes_a.reserve(size_t(cc_max) * (N + 1) * maxw * 4));  // + 1: the backward GEMM's spare row per plane
  if (b.plan.need_pong) LGNN_CALL(h->ws.planes_b.reserve(size_t(cc_max) * N * maxw * 4));
  // GCN with res below the top level: dh_l = g_l W_l + u_l Wr_l needs a third buffer
  if (h->has_res && gcn && L > 2) LGNN_CALL(h->ws.planes_c.reserve(size_t(cc_max) * N * maxw * 4));
  return 0;
}

// The tail of every backward level: g_{l-1} = P^T (rows of a.in) (+ self rows, activation mask) and scratch += its Gram --
// one fused launch (timed: bracketed by events, the dominant launch only), or SpMM into pong, GraphSAGE's norm backward
// (norm_level >= 0) and the Gram through HBM
int propagate_and_gram(KfacBatch& b, FusedArgs& a, bool fuse, bool timed, float* pong, int norm_level) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  if (fuse) {
    LGNN_CALL(attach_long_rows(h, a, s));
    if (timed) LGNN_CALL(record_event(h, s));
    LGNN_CALL(launch_spmm_gram_ex(a, s));
    if (timed) { LGNN_CALL(record_event(h, s)); h->ev_planes += a.nplanes; }
    return 0;
  }
  LGNN_REQUIRE(pong != nullptr, "internal: unfused path without its output planes");
  const int64_t N = a.nrows, d = a.width;
  SpmmArgs sa{};
  sa.rowptr = a.rowptr; sa.col = a.col; sa.val = a.val; sa.nrows = N;
  sa.skip_zero = a.val != h->PT.val;  // the per-batch values: zero at the columns of all-zero source rows
  sa.in = a.in; sa.in_ld = a.in_ld; sa.in_plane_stride = a.in_plane_stride;
  sa.self = a.self; sa.self_ld = a.self_ld; sa.self_plane_stride = a.self_plane_stride;
  sa.hact = a.hact; sa.hact_ld = a.hact_ld; sa.act = a.act;
  sa.out = pong; sa.out_ld = d; sa.out_plane_stride = N * d; sa.width = d; sa.out_act = -1;
  LGNN_CALL(launch_spmm_ex(sa, a.nplanes, s));
  if (norm_level >= 0) LGNN_CALL(launch_resnorm_backward(h, norm_level, pong, d, a.nplanes * N, nullptr, false, s));
  return launch_gram(pong, d, a.nplanes * N, d, a.scratch, s);
}

// GCN, level l of the class chunk's cc planes g [cc][N][dims[l+1]]:  up = act'(h_l) * (g W_l)  (gnn/models/layers.py:45-46
// backward through lin and the activation) into ping, then g_{l-1} = P^T up (into pong when a lower level reads it)
int kfac_level_gcn(KfacBatch& b, int l, int64_t cc, const float* g, float* ping, float* pong) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int64_t N = h->N;
  const int64_t dout = h->dims[l + 1];  // width of g
  const int64_t d = h->dims[l];         // width of g_{l-1}
  const bool store = (l - 1) > 0, dominant = (l - 1) == 0;
  GemmEpilogue ep;
  ep.hact = h->fc.hact_p[l - 1]; ep.hact_ld = h->fc.hact_ld[l - 1]; ep.act = h->act; ep.hact_row_mod = N;
  const bool top_level = l == h->L - 1;
  const bool fuse_here = b.plan.fuse[l];
  if (top_level && fuse_here) ep.row_active = b.row_active;  // inactive rows are never read below
  int64_t ping_stride = N * d;
  // res / norm (unfused route only): below the top level the layer above has a res Linear whose gradient u_l (still
  // in `ping` from the previous step) joins in, dh_l = g_l W_l + u_l Wr_l; then the activation mask and the norm's
  // row-local backward turn dh_l into u_{l-1}, the gradient at s_{l-1} -- what res.{l-1} sees and what P^T propagates
  const bool res_term = h->has_res && !top_level;
  if (res_term) {
    GemmEpilogue none;
    LGNN_CALL(launch_gemm(ping, dout, h->Wr[l], d, h->ws.planes_c.as<float>(), d, cc * N, dout, d, none, s));
    ep = none;  // the mask moves behind the sum
  }
  // (32-bit row offsets inside a plane: beyond 2 GiB per plane the generic GEMM takes over)
  if (b.plan.backgemm[l]) {
    LGNN_REQUIRE(b.row_active != nullptr, "internal: compacted backward GEMM without its row list");
    ping_stride = (N + 1) * d;  // row N of every plane takes the stores of rows past the end of the list
    BackGemmArgs bg{};
    bg.u_plane_stride = ping_stride;
    bg.G = g; bg.W = h->W[l]; bg.ldw = d; bg.U = ping; bg.N = N; bg.K = dout; bg.Nout = d; bg.planes = cc;
    bg.rows = b.rows.list; bg.na_dev = b.rows.count;
    if (h->act == LGNN_ACT_RELU) { bg.mask_bits = h->fc.mask_bits[l - 1].as<uint32_t>(); bg.mask_words = cdiv(d, 32); }
    else { bg.hact = ep.hact; bg.hact_ld = ep.hact_ld; bg.act = h->act; }
    LGNN_CALL(launch_backgemm(bg, s));
  } else {
    LGNN_CALL(launch_gemm(g, dout, h->W[l], d, ping, d, cc * N, dout, d, ep, s));
  }
  if (res_term || h->norm != LGNN_NORM_NONE)
    LGNN_CALL(launch_resnorm_backward(h, l - 1, ping, d, cc * N, res_term ? h->ws.planes_c.as<float>() : nullptr, res_term, s));
  if (h->has_res)  // B of res.{l-1}: the Gram of u_{l-1} before the propagation (curvlinops/kfac.py:777-817)
    LGNN_CALL(launch_gram(ping, d, cc * N, d, h->ws.gram_scratch_res[l - 1].as<float>(), s));
  FusedArgs a{};
  a.rowptr = h->PT.rowptr; a.col = h->PT.col; a.val = (top_level && fuse_here) ? b.val_top : h->PT.val;
  a.nrows = N; a.nplanes = cc;
  a.in = ping; a.in_ld = d; a.in_plane_stride = ping_stride;
  LGNN_REQUIRE(!store || pong != nullptr, "internal: stored planes without a buffer");
  a.store = store ? pong : nullptr; a.store_ld = d; a.store_plane_stride = N * d;
  a.width = d; a.scratch = h->ws.gram_scratch[l - 1].as<float>();
  return propagate_and_gram(b, a, fuse_here, h->timing && dominant, pong, -1);
}

// GraphSAGE, second backward level of a deeper model: g (the level above's output) is non-zero only where that level could
// write, i.e. on the batch nodes and their neighbours (products shape: 20 % of the rows).  Once per batch: the flags and the
// list of those rows and P^T's values with the other columns zeroed (their rows are not gathered); the list's length stays
// on the device.  Called at the first chunk that reaches the level, after that chunk's top level has been enqueued.
int ensure_second_level(KfacBatch& b) {
  if (b.second_level_built) return 0;
  lgnn_ctx* h = b.h;
  LGNN_CALL(h->ws.val_act2.reserve(size_t(h->nnz) * 4));
  LGNN_CALL(mark_rows(h, b.idx, b.M, kRowsBoth, h->ws.out_flags, b.s));
  LGNN_CALL(launch_mask_values(h, h->ws.out_flags.as<uint8_t>(), h->ws.val_act2.as<float>(), b.s));
  LGNN_CALL(compact_rows(h, h->ws.out_flags.as<uint8_t>(), h->ws.out_list, h->ws.out_count, b.s));
  b.second_level_built = true;
  return 0;
}

// GraphSAGE, level l:  dcat = g W_l  [cc*N, 2d] into ping;  g_{l-1} = act'(h_l) * (dcat[:, :d] + P^T dcat[:, d:])
int kfac_level_sage(KfacBatch& b, int l, int64_t cc, const float* g, float* ping, float* pong) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int64_t N = h->N;
  const int L = h->L;
  const int64_t dout = h->dims[l + 1];  // width of g
  const int64_t d = h->dims[l];         // width of g_{l-1}
  const bool store = (l - 1) > 0, dominant = (l - 1) == 0;
  const bool compact = b.plan.sage_compact && l == L - 1;
  const bool second = l == L - 2 && !b.no_fuse && h->nnz > 0;
  int64_t ping_stride = N * 2 * d;
  if (compact) {
    // rows of dcat other than the batch nodes' are zero: the buffer is zeroed once (per allocation / extent)
    // and the rows written here are cleared again after the fused kernel has consumed them
    ping_stride = (N + 1) * 2 * d;
    const size_t extent = size_t(cc) * ping_stride * 4;
    if (h->ws.planes_a_zero_ptr != h->ws.planes_a.p || h->ws.planes_a_zero_bytes < extent) {
      LGNN_HIP_CHECK(hipMemsetAsync(h->ws.planes_a.p, 0, extent, s));
      h->ws.planes_a_zero_ptr = h->ws.planes_a.p;
      h->ws.planes_a_zero_bytes = extent;
    }
    BackGemmArgs bg{};
    bg.G = g; bg.W = h->W[l]; bg.ldw = 2 * d; bg.U = ping; bg.N = N; bg.K = dout; bg.Nout = 2 * d; bg.planes = cc;
    bg.u_plane_stride = ping_stride;
    bg.rows = b.rows.list; bg.na_dev = b.rows.count;
    LGNN_CALL(launch_backgemm(bg, s));
  } else {
    GemmEpilogue ep;
    if (second) {
      LGNN_CALL(ensure_second_level(b));
      // g W_l on the listed rows only, straight from and into the planes (the kernel gathers the A rows and scatters
      // the C rows through the list and reads the list's length on the device: no host round trip); the other rows
      // of dcat are zero
      LGNN_HIP_CHECK(hipMemsetAsync(ping, 0, size_t(cc) * N * 2 * d * 4, s));
      LGNN_CALL(launch_gemm_listed(g, dout, h->Wback(l), 2 * d, ping, 2 * d, cc, N, h->ws.out_list.as<int32_t>(),
                                   h->ws.out_count.as<int32_t>(), dout, 2 * d, ep, s));
    } else {
      // (with res: W_l + [Wr_l | 0] -- the Linear's output gradient is also res.{l}'s, base_gnn.py:141-144)
      LGNN_CALL(launch_gemm(g, dout, h->Wback(l), 2 * d, ping, 2 * d, cc * N, dout, 2 * d, ep, s));
    }
    h->ws.planes_a_zero_ptr = nullptr;  // every row written
  }
  FusedArgs a{};
  a.rowptr = h->PT.rowptr; a.col = h->PT.col; a.val = (l == L - 1) ? b.val_top : h->PT.val;
  if (second) a.val = h->ws.val_act2.as<float>();
  a.nrows = N; a.nplanes = cc;
  a.in = ping + d; a.in_ld = 2 * d; a.in_plane_stride = ping_stride;
  a.self = ping; a.self_ld = 2 * d; a.self_plane_stride = ping_stride;
  a.hact = h->fc.hact_p[l - 1]; a.hact_ld = h->fc.hact_ld[l - 1]; a.act = h->act;
  if (compact && h->act == LGNN_ACT_RELU && d > 128) {
    // 256-wide kernel, nothing conditional in its row loop: self rows exist for the batch nodes only (flags),
    // the ReLU derivative comes from the bit masks of the forward
    a.self_rows = b.rows.flags;
    a.mask_bits = h->fc.mask_bits[l - 1].as<uint32_t>();
    a.mask_words = int(cdiv(d, 32));
    if (!store && b.plan.fuse[l]) {
      // g_{l-1} = act' * (dcat_self + P^T dcat_neigh) can be non-zero on the batch nodes and their neighbours only
      // (the columns of the batch nodes' P rows): the fused kernel visits just those rows
      LGNN_CALL(build_row_list(h, b.idx, b.M, kRowsBoth, h->ws.out_flags, h->ws.out_list, h->ws.out_count, s));
      a.row_list = h->ws.out_list.as<int32_t>();
      a.row_count = h->ws.out_count.as<int32_t>();
    }
  }
  LGNN_REQUIRE(!store || pong != nullptr, "internal: stored planes without a buffer");
  a.store = store ? pong : nullptr; a.store_ld = d; a.store_plane_stride = N * d;
  a.width = d; a.scratch = h->ws.gram_scratch[l - 1].as<float>();
  LGNN_REQUIRE(b.plan.fuse[l] || !compact, "internal: compact GraphSAGE top level without the fused kernel");
  LGNN_CALL(propagate_and_gram(b, a, b.plan.fuse[l], h->timing && dominant, pong, h->norm != LGNN_NORM_NONE ? l - 1 : -1));
  if (compact) {
    hipLaunchKernelGGL(clear_rows_kernel, dim3(2048), dim3(256), 0, s, ping, ping_stride, 2 * d, cc, b.rows.list, b.rows.count);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// B_l += b_scale * (this batch's Gram), the epilogue, the cache counters
int kfac_finish(KfacBatch& b) {
  lgnn_ctx* h = b.h;
  hipStream_t s = b.s;
  const int L = h->L;
  const float b_scale = b.fisher ? b.fisher->b_scale : 1.0f;
  for (int l = 0; l < L; ++l)
    LGNN_CALL(launch_sym_accumulate(h->ws.gram_scratch[l].as<float>(), h->dims[l + 1], b_scale, b.B_out[l], s));
  // res.{l}: GCN -- the Gram of u_l taken before the propagation; GraphSAGE -- the Linear's output is not propagated, so
  // convs.{l}.lin and res.{l} see the same gradient and share B
  for (int l = 0; h->has_res && l < L - 1; ++l)
    LGNN_CALL(launch_sym_accumulate((h->kind == LGNN_KIND_GCN ? h->ws.gram_scratch_res[l] : h->ws.gram_scratch[l]).as<float>(),
                                    h->dims[l + 1], b_scale, b.B_out[L + l], s));
  LGNN_CALL(batch_epilogue(h, b.idx, b.M, s));
  // lgnn_batch_cache_stats: a hit launched none of the list-building kernels, a build filled (part of) an entry, a miss ran
  // the uncached code under a tag
  if (b.be_route && b.batch_tag != 0 && batch_cache_budget() != 0) {
    if (!b.be) ++h->bcache.misses;
    else if (b.be_built) ++h->bcache.builds;
    else ++h->bcache.hits;
  }
  return 0;
}

}  // namespace

int record_event(lgnn_ctx* h, hipStream_t s) {
  if (h->ev_used >= h->ev.size()) {
    hipEvent_t e;
    LGNN_HIP_CHECK(hipEventCreate(&e));
    h->ev.push_back(e);
  }
  LGNN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used++], s));
  return 0;
}

// Every path decision of kfac_accumulate as a pure function of the shapes (base pointers come from hipMalloc and
// are 256-byte aligned, so alignment follows from the widths).  One helper serves the launch loop, the workspace
// sizing (need_pong, cc_max) and lgnn_kfac_plan, so that the prediction cannot drift from what the loop does.
KfacPlan plan_kfac(int kind, int L, int64_t N, int64_t nnz, const int64_t* dims, int act, bool no_fuse,
                   int64_t ws_limit, bool no_paths) {
  KfacPlan p{};
  const int64_t C = dims[L];
  const bool gcn = kind == LGNN_KIND_GCN;
  p.seeds_on_the_fly = gcn && !no_fuse && C <= 64;
  const int64_t d_top = L > 1 ? dims[L - 1] : 0;
  auto hact_ld = [&](int l) { return gcn ? dims[l + 1] : 2 * dims[l + 1]; };  // row stride of h_{l+1} (context.hip)
  p.sage_compact = !gcn && L > 1 && !no_fuse && nnz > 0 && backgemm_supported(C, 2 * d_top, false) &&
                   (N + 1) * 2 * d_top * 4 < (int64_t(1) << 31) &&
                   fused_supported(d_top, 2 * d_top, (N + 1) * 2 * d_top, nullptr, N + 1) && hact_ld(L - 2) % 4 == 0;
  const bool row_active = gcn && !no_fuse && nnz > 0;  // flags of the non-zero top-layer gradient rows exist
  p.need_pong = L > 2 || no_fuse;
  p.paths = !no_fuse && !no_paths && (gcn ? p.seeds_on_the_fly : true) && paths_supported(kind, L, dims, act, nnz);
  if (p.paths) p.sage_compact = false;  // (GraphSAGE: one-hop paths instead of the compact top level + fused LIST kernel)
  for (int l = L - 1; l >= 1; --l) {
    const int64_t d = dims[l], dout = dims[l + 1];
    const bool top = l == L - 1;
    if (gcn) {
      p.fuse[l] = !no_fuse && fused_supported(d, d, N * d, nullptr, N + 1);
      p.backgemm[l] = top && p.fuse[l] && row_active && backgemm_supported(dout, d, act == LGNN_ACT_RELU) &&
                      (N + 1) * d * 4 < (int64_t(1) << 31);
    } else {
      const bool compact = p.sage_compact && top;
      const int64_t stride = (compact ? N + 1 : N) * 2 * d;
      p.fuse[l] = !no_fuse && fused_supported(d, 2 * d, stride, nullptr, N + 1) && hact_ld(l - 1) % 4 == 0;
      p.backgemm[l] = compact;
    }
    if (!p.fuse[l]) p.need_pong = true;  // the unfused path writes its SpMM output there
    p.maxw = std::max(p.maxw, gcn ? d : 2 * d);  // GEMM output width of layer l
  }
  if (p.paths) {  // Y [N][classes][H] is the only plane-sized buffer; no fused kernel, no backward GEMM, no second buffer
    p.need_pong = false;
    for (int l = 0; l < L; ++l) p.fuse[l] = p.backgemm[l] = false;
  }
  const int64_t per_class = p.paths ? N * p.maxw * 4 : (N + 1) * p.maxw * 4 * (p.need_pong ? 2 : 1);
  p.cc_max = std::max<int64_t>(1, std::min<int64_t>(C, ws_limit / std::max<int64_t>(per_class, 1)));
  return p;
}

int kfac_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train, uint32_t flags,
                    int64_t cb, int64_t ce, float* const* A_out, float* const* B_out, float* loss_out, hipStream_t s,
                    const KfacFisherOpts* fisher, const KfacShare* share) {
  KfacBatch b{};
  b.h = h; b.idx = idx; b.y = y; b.M = M; b.n_train = n_train; b.flags = flags;
  b.A_out = A_out; b.B_out = B_out; b.loss_out = loss_out; b.s = s; b.fisher = fisher; b.share = share;
  LGNN_CALL(kfac_resolve(b, cb, ce));
  const bool gcn = h->kind == LGNN_KIND_GCN;
  const int L = h->L;
  LGNN_CALL(batch_prologue(h, idx, y, M, !b.seeds_on_the_fly, b.fork_exact, b.once ? loss_out : nullptr, s,
                           fisher ? fisher->y_seed : nullptr, fisher ? fisher->resid_scale : 1.0f, b.be ? b.be->ids : nullptr));
  LGNN_CALL(kfac_input_factors(b));
  // a part without a class column: what exists once per batch has been added above.  (GraphSAGE goes on: its whole
  // top-layer Gram belongs to part 0, and every loop over the classes [cb, ce) below is empty)
  if (b.no_classes && gcn) return batch_epilogue(h, idx, M, s);

  LGNN_CALL(gcn ? kfac_top_gcn(b) : kfac_top_sage(b));
  h->last_route_paths = b.paths_route;
  h->last_top_kernel = b.top_pairs ? 2 : (b.top_tiles ? 1 : 0);
  if (b.paths_route) LGNN_CALL(kfac_path_route(b));

  // the lower layers, chunked over classes
  if (L > 1 && !b.paths_route) {
    LGNN_CALL(kfac_lower_prepare(b));
    const int64_t N = h->N, C = h->dims[L], cc_max = b.plan.cc_max;
    for (int64_t c0 = b.cb; c0 < b.ce; c0 += cc_max) {
      const int64_t cc = std::min(cc_max, b.ce - c0);
      const float* g = b.gtop + c0 * N * C;  // planes [cc][N][dims[l+1]] of layer l
      float* ping = h->ws.planes_a.as<float>();
      float* pong = b.plan.need_pong ? h->ws.planes_b.as<float>() : nullptr;
      for (int l = L - 1; l >= 1; --l) {
        LGNN_CALL(gcn ? kfac_level_gcn(b, l, cc, g, ping, pong) : kfac_level_sage(b, l, cc, g, ping, pong));
        // stream order makes the two buffers reusable: the next GEMM reads g (= pong) and overwrites
        // ping, which the SpMM above has finished reading; the next SpMM then overwrites pong
        g = pong;
      }
    }
  }
  return kfac_finish(b);
}

}  // namespace lgnn

// Host-only: which kernels a KFAC accumulate of this shape would run (no context, no device work) -- lets the path
// decisions be tested per branch without allocating the planes (products-shaped GraphSAGE: 5 GB per plane).
extern "C" int lgnn_kfac_plan(int kind, int num_layers, const int64_t* dims, int64_t num_nodes, int64_t nnz, int activation,
                              uint32_t flags, int64_t workspace_limit, int64_t* out) {
  using namespace lgnn;
  if (!dims || !out) { set_error("null argument"); return 2; }
  LGNN_REQUIRE(num_layers >= 1 && num_layers <= kMaxLayers, "num_layers out of range");
  LGNN_REQUIRE(kind == LGNN_KIND_GCN || kind == LGNN_KIND_SAGE, "unknown graph kind");
  LGNN_REQUIRE(workspace_limit > 0 && num_nodes > 0, "workspace limit and node count must be positive");
  const KfacPlan p = plan_kfac(kind, num_layers, num_nodes, nnz, dims, activation, (flags & LGNN_FLAG_NO_FUSE) != 0,
                               workspace_limit, (flags & LGNN_FLAG_NO_PATHS) != 0);
  out[0] = p.seeds_on_the_fly; out[1] = p.sage_compact; out[2] = p.need_pong; out[3] = p.cc_max;
  for (int l = 0; l < num_layers; ++l)
    out[4 + l] = (p.fuse[l] ? 1 : 0) | (p.backgemm[l] ? 2 : 0) | ((p.paths && l == num_layers - 1) ? 4 : 0);
  return 0;
}

// Empirical / Monte-Carlo Fisher KFAC: one backward pass per call, seeded with resid_scale * d loss(f, y_seed) / d f.
extern "C" int lgnn_kfac_accumulate_fisher(lgnn_ctx* h, const int64_t* idx, const void* y_seed, const void* y_loss,
                                           int64_t M, int64_t n_train, uint32_t flags, float resid_scale, float b_scale,
                                           float* const* A_out, float* const* B_out, float* loss_out, void* stream) {
  using namespace lgnn;
  if (!h) { set_error("null context"); return 2; }
  LGNN_REQUIRE(y_seed != nullptr, "the Fisher accumulate needs the labels / targets to seed with");
  KfacFisherOpts o{y_seed, resid_scale, b_scale, y_loss != nullptr};
  return kfac_accumulate(h, idx, y_loss, M, n_train, flags, 0, 1, A_out, B_out, loss_out, static_cast<hipStream_t>(stream), &o);
}
