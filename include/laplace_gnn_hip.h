/*
 * laplace_gnn_hip.h -- C ABI of the MI355X (gfx950) curvature-accumulation engine.
 *
 * This is the drop-in boundary for ONE path of anitasyang/Laplace-GNN: what
 * `laplace.curvature.CurvlinopsGGN.kron / .diag / .full` do for a GCN / GraphSAGE model
 * inside `Laplace(...).fit()`.  The reference is pure Python (no native code), so nothing
 * in it binds a C library today; each entry point below names the reference interface it
 * replaces (file:line under the reference tree).  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP, one GPU per process) unless marked "host";
 *     tensors are row-major, fp32 / int64 exactly as PyTorch hands them over;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued asynchronously on it.  The calls that DO synchronise `stream` -- a
 *     count has to reach the host before the next launch or allocation can be sized -- are,
 *     completely:
 *       lgnn_create, lgnn_adj_to_edge_index     the deduplicated nnz / the off-diagonal count;
 *       lgnn_check_async_errors                 by design (reports the sticky error flags);
 *       the FIRST KFAC / adjacency-gradient call on a graph, once per graph: the list of rows with
 *         more than 64 stored entries (hubs) and the graph's number of 2-hop paths;
 *       lgnn_glm_variance(_mapped), lgnn_glm_variance_ext, once per call: the size of the per-class row table;
 *       lgnn_update_adjacency: the new number of stored entries.
 *     Everything else -- KFAC of GCN / GraphSAGE models of any depth, diagonal and last-layer GGN, forward,
 *     Jacobians -- enqueue only; workspaces grow on first use of a shape and are reused after;
 *   - every function returns 0 on success, non-zero on error; the message is available
 *     from lgnn_last_error() (thread-local).  No C++ exception crosses the boundary;
 *   - borrowed pointers (weights, features, indices, outputs) are owned by the caller
 *     and must stay valid until the stream work that uses them has finished;
 *   - accumulate-style calls ADD into caller-owned fp32 buffers, so one all-reduce of
 *     those buffers is all a data-parallel caller needs.
 */
#ifndef LAPLACE_GNN_HIP_H
#define LAPLACE_GNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGNN_ABI_VERSION 1

#if defined(__GNUC__)
#define LGNN_API __attribute__((visibility("default")))
#else
#define LGNN_API
#endif

/* graph kinds: which propagation matrix the convolutions use */
#define LGNN_KIND_GCN 0  /* D^-1/2 A^T D^-1/2, self loops added  (gnn/models/models.py:23-31, utils.py:106-112) */
#define LGNN_KIND_SAGE 1 /* A / max(rowsum,1), self loops removed (gnn/models/models.py:47, layers.py:18-24)    */
/* bit of `kind` in lgnn_create, GraphSAGE only: the diagonal is part of the graph.  STEGraphSAGE zeroes it once in its
 * constructor (gnn/models/models.py:135) and its forward_adj never overwrites it again (models.py:160-180, against :114 of
 * STEGCN), so adj[i, i] is a learnable entry: pairs (i, i) of the edge list are kept, lgnn_update_adjacency edits them, and a
 * stored (i, i) is an ordinary entry of A and A^T (row sum deg + 1, layers.py:18-24).  A GCN context refuses the bit. */
#define LGNN_KIND_SELF_LOOPS 0x100

/* activations between layers (gnn/models/base_gnn.py:85, default "relu") */
#define LGNN_ACT_RELU 0
#define LGNN_ACT_TANH 1

/* normalisation between a hidden layer's convolution and its activation (gnn/models/base_gnn.py:86-95, 148) */
#define LGNN_NORM_NONE 0  /* nn.Identity                                        */
#define LGNN_NORM_LAYER 1 /* nn.LayerNorm(hidden): per-row statistics           */
#define LGNN_NORM_BATCH 2 /* nn.BatchNorm1d(hidden) in eval mode: running stats */

/* likelihoods (laplace/curvature/curvature.py:63-72) */
#define LGNN_LIK_CLASSIFICATION 0 /* CrossEntropyLoss(sum), factor 1   */
#define LGNN_LIK_REGRESSION 1     /* MSELoss(sum), factor 0.5          */

/* flags of lgnn_kfac_accumulate */
#define LGNN_FLAG_FORK_EXACT_SEED 1u /* back-propagate d/df sum_i f_i S_ic(f) (curvlinops/kfac.py:637-661 as
                                        modified by the fork) instead of upstream's detached S[:,c]          */
#define LGNN_FLAG_NO_FUSE 2u         /* debugging: run SpMM^T and the Gram contraction as separate kernels    */
#define LGNN_FLAG_NO_PATHS 4u        /* 2-layer GCN: keep the class-plane route (backward GEMM + fused SpMM^T -> Gram) instead
                                        of the two-hop path route (csrc/paths*.hip); same results up to fp32 reassociation */
#define LGNN_FLAG_FORCE_PATHS 8u     /* take the path route wherever the model's shape allows it, also on hub-heavy graphs where
                                        the library would choose the planes (its default weighs the batch's expected number of
                                        2-hop paths per node); the first eligible call counts the graph's 2-hop paths once and
                                        synchronises the stream that one time                                            */

typedef struct lgnn_ctx lgnn_ctx; /* opaque: graph + bound model + forward cache + workspace */

/* ---- library ------------------------------------------------------------------------ */
LGNN_API int lgnn_abi_version(void);
LGNN_API const char* lgnn_last_error(void);

/* ---- graph ingest: the integer path (bit exact) ---------------------------------------
 * Replaces gnn/utils.py:325-330 (edge_index -> dense adj, duplicates summed),
 * gnn/marglik_training.py:405 (clamp to 1), gnn/models/models.py:23 / :47 (self loops on /
 * off), gnn/models/base_gnn.py:68-72 (optional symmetrise) and gnn/models/utils.py:106-112 /
 * gnn/models/layers.py:18-24 (normalisation, done once here instead of on every forward).
 * edge_index: int64 [2,E] (row 0 = source/row, row 1 = target/col of the dense adj).
 * Synchronises `stream` once (the deduplicated nnz has to reach the host).                */
LGNN_API int lgnn_create(lgnn_ctx** out, int64_t num_nodes, const int64_t* edge_index, int64_t num_edges,
                int kind, int symmetric, void* stream);
LGNN_API void lgnn_destroy(lgnn_ctx* h);

/* nnz of the stored 0/1 adjacency (incl. self loops for GCN and for LGNN_KIND_SELF_LOOPS).  host value. */
LGNN_API int64_t lgnn_nnz(const lgnn_ctx* h);
LGNN_API int64_t lgnn_num_nodes(const lgnn_ctx* h);
/* Rows of the backward propagation matrix with more than 64 stored entries (hubs): the 256-wide fused kernel receives
 * them finished from a side kernel instead of gathering them in one wave.  -1 until the first KFAC call built the list. */
LGNN_API int64_t lgnn_num_long_rows(const lgnn_ctx* h);
/* 1 if the last lgnn_kfac_accumulate* call on this context took the two-hop path route (csrc/paths*.hip), 0 if it built class
 * planes: which of the two implementations of curvlinops/kfac.py:653-661, 777-817 ran (measurement labels; host value). */
LGNN_API int lgnn_kfac_last_route(const lgnn_ctx* h);
/* 1 if the top layer of that call ran on a matrix-pipe kernel of the path route (csrc/toptiles.hip or csrc/toppairs.hip: GCN,
 * no sliced hub rows), 0 if seed_spmm_gram_kernel ran (host value). */
LGNN_API int lgnn_kfac_last_top(const lgnn_ctx* h);
/* Which kernel that was: 0 seed_spmm_gram_kernel, 1 top_tiles_kernel (per-node tiles and Grams), 2 top_pairs_kernel (one MFMA
 * K step per sample and per pair of samples that share a node; taken when a host-known bound of the pairs fits the list). */
LGNN_API int lgnn_kfac_last_top_kernel(const lgnn_ctx* h);
/* Which MFMAs the last launch of the path route's fused kernel (csrc/paths_fused.hip) ran on: 0 fp32 throughout (LGNN_GRAM_F32=1,
 * or a launch without a usable scale), 1 the Gram on fp16 pieces and the beta / gamma path products on fp32, 2 those products
 * on fp16 pieces too (where the launch's scalars pass the rule of PathScale); -1 if the last call did not take that route or
 * its path list overflowed its buffer, so that the fused kernel did not run.  `scalars` (5 floats, may be null) receives the launch's bound terms amax, w1max, bgmax, vmax, wsum (PathScale in
 * csrc/paths.h).  Waits for the device: a query for tests and measurements, not for use inside a fit. */
LGNN_API int lgnn_last_paths_product_role(lgnn_ctx* h, float* scalars);
/* 1 if the stored adjacency equals its transpose (then forward and backward share one CSR) */
LGNN_API int lgnn_is_symmetric(const lgnn_ctx* h);

/* Export the stored adjacency in the order `model.adj.nonzero()` yields (row-major):
 * rows,cols int64 [nnz].  (tests: bit-exactness against the reference.)                    */
LGNN_API int lgnn_export_adj(const lgnn_ctx* h, int64_t* rows, int64_t* cols, void* stream);
/* gnn/utils.py:333-336 adj_to_edge_index: diagonal dropped, row-major, int64 [2,E'].
 * Call with edge_index_out = NULL to get E' in *num_out (host); then again with a buffer. */
LGNN_API int lgnn_adj_to_edge_index(const lgnn_ctx* h, int64_t* edge_index_out, int64_t* num_out, void* stream);
/* Apply a structure-learning step to the stored 0/1 adjacency in place: `num_flips` pairs (rows[k], cols[k]) (device, int64)
 * and the state each shall have afterwards (device uint8: 1 = stored, 0 = absent).  What the reference does by writing its
 * dense `adj` parameter (`adj_optimizer.step()`, gnn/marglik_training.py:211-221) and re-thresholding it on the next forward
 * (`BinarizeSTE` + `fill_diagonal_(1)` + `normalize_adj`, gnn/models/models.py:103-116, gnn/models/utils.py:42-112): here the
 * caller (laplace_gnn_amd.models.STEGCN) thresholds its continuous values and hands over the entries that changed side.
 * Diagonal pairs are ignored (a GCN's self loops are overwritten ones, GraphSAGE's zeros) unless the context was created with
 * LGNN_KIND_SELF_LOOPS: then (i, i) is inserted and removed like any other pair (on a symmetric graph it is its own mirror).  A
 * pair listed twice or an id out of range is an error.  No re-ingest: the flips are sorted and merged into both CSRs, degrees and the values of the propagation
 * matrices are recomputed, everything cached from the graph (forward pass, P X, long-row lists) is dropped; what depends on
 * the features only survives.  Synchronises the stream (the new entry count has to reach the host).                       */
LGNN_API int lgnn_update_adjacency(lgnn_ctx* h, const int64_t* rows, const int64_t* cols, const uint8_t* state,
                                   int64_t num_flips, void* stream);
/* Export the propagation matrix the convs multiply with (A_hat or A_bar) as COO in row-major
 * order: rows,cols int64 [nnz], vals fp32 [nnz].                                            */
LGNN_API int lgnn_export_propagation(const lgnn_ctx* h, int64_t* rows, int64_t* cols, float* vals, void* stream);

/* ---- model binding ----------------------------------------------------------------------
 * Replaces the module state gnn/models/base_gnn.py:62-76 + the parameter filter
 * laplace/curvature/curvature.py:74-79: L layers `convs.{l}.lin` with weight [dims[l+1], in_l]
 * and bias [dims[l+1]]; in_l = dims[l] (GCN) or 2*dims[l] (GraphSAGE, cat[x, mean_agg]).
 * X: [N, dims[0]].  Pointers are borrowed.  Binding (re)sizes the workspace and invalidates the
 * forward cache; call lgnn_invalidate() after changing weights in place.                     */
LGNN_API int lgnn_bind_model(lgnn_ctx* h, int num_layers, const int64_t* dims /* host [L+1] */,
                    const float* const* weights /* host array of L device ptrs */,
                    const float* const* biases /* host array of L device ptrs */, const float* X,
                    int activation, int likelihood);
/* Optional pieces of BaseGNN.forward (gnn/models/base_gnn.py:86-113 construction, :141-149 forward; shipped configs
 * gnn/configs/original/gcn_config.yaml:36-58 use norm: layer + res: True).  Call after lgnn_bind_model (which resets them):
 *   res_weights / res_biases : host arrays of L-1 device pointers, `res.{l}.weight` [dims[l+1], dims[l]] / `res.{l}.bias`
 *                              (NULL: res=False); x = res_l(x) + conv_l(adj, x) for every hidden layer;
 *   norm_kind                : LGNN_NORM_*; norm_weight / norm_bias [dims[l+1]] per hidden layer (`norms.{l}.weight|bias`),
 *                              norm_mean / norm_var = BatchNorm1d running statistics (eval mode; NULL otherwise).
 * The `res.{l}` Linears are Laplace parameters AFTER all `convs.*` (named_parameters order; laplace/curvature/
 * curvature.py:74-79 filters `norms.*` out): every per-parameter output grows accordingly -- A_out / B_out of the KFAC calls
 * take 2 L - 1 pointers (convs.0 .. convs.{L-1}, res.0 .. res.{L-2}; curvlinops/kfac.py:877-916 gives every nn.Linear its
 * block), diag / Jacobians / full GGN append the res parameters.  With extras bound the KFAC accumulate runs its unfused
 * route (GEMM, row-local norm backward, SpMM^T, Gram as separate kernels) and the diagonal GGN / Jacobians the generic plane
 * route; the adjacency gradient and the matrix-free GLM variance refuse such models.                                 */
LGNN_API int lgnn_bind_extras(lgnn_ctx* h, const float* const* res_weights, const float* const* res_biases, int norm_kind,
                     const float* const* norm_weight, const float* const* norm_bias, const float* const* norm_mean,
                     const float* const* norm_var, float norm_eps);
LGNN_API int lgnn_invalidate(lgnn_ctx* h);
/* bytes currently held by the context (graph + caches + workspace).  host value.  What the first fit sizes and later fits of
 * the same shape leave alone; the entries of the batch-structure cache are NOT in this figure -- the second fit over a
 * loader allocates them, bounded by LGNN_BATCH_CACHE_MB, and lgnn_batch_cache_stats reports their bytes. */
LGNN_API int64_t lgnn_device_bytes(const lgnn_ctx* h);
/* cap for the backward workspace (chunks over classes are sized to fit); default 32 GiB */
LGNN_API int lgnn_set_workspace_limit(lgnn_ctx* h, int64_t bytes);

/* ---- forward: model(x_indices) -> [M, C]  (gnn/models/base_gnn.py:136-161, eval mode) ----- */
LGNN_API int lgnn_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, float* out /* [M, C] */, void* stream);
/* all-node logits [N, C] (what forward() indexes into) */
LGNN_API int lgnn_forward_all(lgnn_ctx* h, float* out /* [N, C] */, void* stream);

/* ---- sampled forward: the logits of S parameter samples at a batch, in one pass ---------------------------------------
 * Replaces the loop of the sampling predictive (laplace/baselaplace.py:1160-1199 _nn_predictive_samples, reached from mc_eval,
 * gnn/marglik_training.py:341-353: per sample vector_to_parameters + model(indices), a forward over all N nodes).
 *   theta : [S, n_params] row major, each row in the Laplace parameter order: W_0 [dims[1], in_0] row major, b_0, W_1, b_1
 *           (a 1-layer model: W, b).  Rows need no alignment.
 *   out   : [S, M, C]; out[s, m, :] = the logits the model would give at node idx[m] if sample s were written into it; with
 *           LGNN_SAMPLED_SOFTMAX their softmax.  Every batch row is one output row (a repeated id is computed twice).
 * The bound weights, the cached forward and every other cache are neither read nor changed; what the call keeps (P X with the
 * bias column, the needed-row list, the second Linear's products of a chunk of samples) lives in buffers of its own, counted
 * by lgnn_device_bytes.  The samples go in chunks sized so that those products stay under lgnn_set_workspace_limit.  No
 * float atomics: two calls on the same inputs agree bit for bit, and a sample's numbers do not depend on its chunk.
 * Enqueues only.  Ids outside [0, num_nodes) raise the sticky flag lgnn_check_async_errors reports and give zero rows.
 * Plain GCN / GraphSAGE with 1 or 2 layers, relu or tanh, any widths; a model bound with res / norm or with more than two
 * layers is refused with a message naming the case.                                                                      */
#define LGNN_SAMPLED_SOFTMAX 1u
LGNN_API int lgnn_sampled_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* theta /* [S, P] row major */,
                                  int64_t S, uint32_t flags /* LGNN_SAMPLED_SOFTMAX */, float* out /* [S, M, C] */,
                                  void* stream);

/* ---- training-mode forward and its backward to the parameters --------------------------------------------------------
 * Replaces what autograd does for the weight update of the driver's loop (gnn/marglik_training.py:165-186: model.train();
 * f = model(train_indices); loss = criterion(f, train_labels); loss.backward(); optimizer.step()) on BaseGNN.forward in
 * training mode (gnn/models/base_gnn.py:136-161 with the convs of gnn/models/layers.py:18-46): per hidden layer
 * s = res_l(x) + conv_l(P, x), norms[l] (Identity or LayerNorm), act, inverted dropout on all N rows; the last conv; rows idx.
 *   lgnn_train_forward : out [M, C] = logits of the batch.  drop_masks: host array of L-1 device pointers to uint8 keep-masks
 *                        [N, dims[l+1]] (1 = kept, the caller draws them; borrowed until the backward has run), or NULL / a NULL
 *                        entry for no dropout; kept activations are multiplied by drop_scale = 1 / (1 - p).  The call writes a
 *                        tape into buffers of its own: the cached eval-mode forward (lgnn_forward) is neither read nor changed.
 *   lgnn_train_backward: grad_out [M, C] = d loss / d out.  Every gradient is OVERWRITTEN (autograd accumulates): grad_W[l]
 *                        [dims[l+1], in_l] / grad_b[l] of convs.{l}.lin, grad_res_W[l] [dims[l+1], dims[l]] / grad_res_b[l] of
 *                        res.{l}, grad_norm_w[l] / grad_norm_b[l] [dims[l+1]] of norms.{l} (host arrays of device pointers; NULL
 *                        where the model has none).  A node listed several times in idx receives the sum of its rows (in batch
 *                        order: one thread per class column walks a node's positions, so a node listed thousands of times is
 *                        a serial loop of that length); the GCN bias is propagated, db_l = sum_n rowsum(P)[n] d_l[n, :].
 *                        No product of either call combines partial sums with float atomics: the weight gradients are split-K
 *                        products over the nodes whose partials are summed in a fixed order, every other dense product runs
 *                        unsplit, the SpMMs and reductions have a fixed order -- two calls on the same inputs agree bit for bit.
 *                        The call consumes the tape: without a forward since the last backward, the last lgnn_invalidate /
 *                        lgnn_bind_model or the last lgnn_update_adjacency it fails with a message.
 * fp32; relu / tanh; GCN and GraphSAGE of any bound depth; BatchNorm1d in training mode is refused.  Device memory grows with
 * N * width (the tape and two signal buffers), never with M * P.                                                          */
LGNN_API int lgnn_train_forward(lgnn_ctx* h, const int64_t* idx, int64_t M, const uint8_t* const* drop_masks /* host */,
                                float drop_scale, float* out /* [M, C] */, void* stream);
LGNN_API int lgnn_train_backward(lgnn_ctx* h, const float* grad_out /* [M, C] */, float* const* grad_W, float* const* grad_b,
                                 float* const* grad_res_W, float* const* grad_res_b, float* const* grad_norm_w,
                                 float* const* grad_norm_b, void* stream);

/* ---- KFAC factors of one mini-batch --------------------------------------------------------
 * Replaces CurvlinopsInterface.kron (laplace/curvature/curvlinops.py:77-108) =
 * KFACLinearOperator._compute_kfac (curvlinops/kfac.py:540-581, 607-661, 777-875) +
 * _rescale_kron_factors (curvlinops.py:46-53) + the loss (curvlinops.py:106).
 *   A_out[l]  [in_l, in_l]  += in_l^T in_l / n_train      (all N rows the Linear sees)
 *   B_out[l]  [out_l,out_l] += sum_c g_{l,c}^T g_{l,c}     (one backward per class column c)
 *   *loss_out               += factor * loss(model(idx), y)
 * idx int64 [M]; y int64 [M] (classification) -- regression passes fp32 targets [M, C] as y.
 * The batch is the unit: B has cross-sample terms inside a batch, so callers
 * must keep the reference loader's batch boundaries.                                          */
LGNN_API int lgnn_kfac_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train,
                         uint32_t flags, float* const* A_out /* host array of L device ptrs */,
                         float* const* B_out /* host array of L device ptrs */, float* loss_out,
                         void* stream);

/* The same for the class columns [class_begin, class_end) only.  B_l is a sum over the C class columns of
 * the Hessian square root (one reference backward pass each, curvlinops/kfac.py:653-661), so class ranges
 * are exact additive shares of a batch: a data-parallel caller can balance (batch, class-range) units over
 * ranks without ever splitting a batch's samples.  The share that contains class 0 also adds the loss and
 * the A increment (once per batch).                                                                  */
LGNN_API int lgnn_kfac_accumulate_classes(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train,
                                 uint32_t flags, int64_t class_begin, int64_t class_end,
                                 float* const* A_out, float* const* B_out, float* loss_out, void* stream);

/* Parts [part_begin, part_end) of `part_count` equal parts of the batch's work -- the unit a data-parallel caller deals
 * to its ranks (laplace_gnn_amd.KronLaplace: part_count = C, contiguous balanced runs of (batch, part) units).  HOW a
 * batch is cut is the library's choice, the same on every rank for the same (graph, model, batch size, flags):
 *   - path routes (2-layer GCN / GraphSAGE, lgnn_kfac_last_route == 1): B_0 = sum over destination nodes n of Y_n^T Y_n,
 *     so a part is the node range [N part_begin / part_count, N part_end / part_count) with ALL classes -- nothing is
 *     computed twice (a class range would repeat the path products, which do not depend on the class count);
 *     the small top-layer factor goes with part 0;
 *   - everywhere else: the class range [C part_begin / part_count, C part_end / part_count) of
 *     lgnn_kfac_accumulate_classes (possibly empty).
 * The parts of a batch add up to lgnn_kfac_accumulate exactly (sums of disjoint terms); part 0 also adds the loss and
 * the A increment.  Replaces the same reference loop as lgnn_kfac_accumulate (curvlinops/kfac.py:653-661, 777-817).      */
LGNN_API int lgnn_kfac_accumulate_share(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train,
                               uint32_t flags, int64_t part_begin, int64_t part_end, int64_t part_count,
                               float* const* A_out, float* const* B_out, float* loss_out, void* stream);

/* ---- empirical / Monte-Carlo Fisher -----------------------------------------------------------------------------
 * KFAC with FisherType.EMPIRICAL / FisherType.MC (curvlinops/kfac.py:663-674; reached through CurvlinopsEF and
 * CurvlinopsGGN(stochastic=True), laplace/curvature/curvlinops.py:143-179): ONE backward pass per call, seeded with
 * resid_scale * d loss(f_n, y_seed_n) / d f_n  (softmax - onehot, resp. f - y_seed for the regression likelihood);
 * B_out[l] += b_scale * g^T g  (b_scale = 1 / mc_samples).  y_loss != NULL: the call also adds factor-free
 * loss(model(idx), y_loss) and the A increment (once per batch); y_loss == NULL: further MC samples of a batch.
 * MC labels are drawn by the caller (curvlinops/kfac.py:698-745 draw_label) and passed as y_seed.             */
LGNN_API int lgnn_kfac_accumulate_fisher(lgnn_ctx* h, const int64_t* idx, const void* y_seed, const void* y_loss, int64_t M,
                                int64_t n_train, uint32_t flags, float resid_scale, float b_scale, float* const* A_out,
                                float* const* B_out, float* loss_out, void* stream);
/* Per-sample loss gradients G[m, :] = J_m^T r_m (CurvatureInterface.gradients, laplace/curvature/curvature.py:169-210)
 * and what EFInterface (:435-504) and GGNInterface with stochastic=True (:343-364, 401-432) build from them:
 *   grads_out [M, P]  = G (may be NULL)     diag_out [P] += scale * sum_m G[m, p]^2 (may be NULL)
 *   full_out [P, P]  += scale * G^T G (may be NULL)         *loss_out += loss(model(idx), y_loss) when y_loss != NULL
 * r_m = resid_scale * (softmax(f_m) - onehot(y_seed_m)), regression: resid_scale * (f_m - y_seed_m).          */
LGNN_API int lgnn_ef_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y_seed, const void* y_loss, int64_t M,
                       float resid_scale, float scale, float* diag_out, float* full_out, float* grads_out,
                       float* loss_out, void* stream);

/* Host-only query (no context, no device work): which kernels lgnn_kfac_accumulate would run for a model of this
 * shape -- the per-layer choice between the fused SpMM^T -> Gram kernel and the SpMM + Gram pair through HBM, the
 * compacted backward GEMM, and the workspace layout (curvlinops/kfac.py:653-661 has one autograd backward per class
 * instead; nothing to choose there).  out: int64 [4 + num_layers] = {seeds_on_the_fly, sage_compact, need_pong,
 * classes_per_chunk, step_0 .. step_{L-1}} with step_l = 1 (fused) | 2 (compacted backward GEMM) | 4 (step L-1 only: the
 * first layer's B comes from the batch's two-hop paths, no class planes); step_0 is unused. */
LGNN_API int lgnn_kfac_plan(int kind, int num_layers, const int64_t* dims /* host [L+1] */, int64_t num_nodes, int64_t nnz,
                   int activation, uint32_t flags, int64_t workspace_limit, int64_t* out /* host */);

/* ---- diagonal GGN of one mini-batch ----------------------------------------------------------
 * Replaces GGNInterface.diag (laplace/curvature/curvature.py:412-432 with jacobians :89-130 and
 * _get_functional_hessian :365-372):  diag_out[P] += einsum('bcp,bck,bkp->p', J, Lambda, J),
 * parameter order = named_parameters() (W0 row-major, b0, W1, b1, ...).  1- and 2-layer models: closed form, no
 * Jacobians; deeper models and the regression likelihood (y = fp32 targets [M, C], H_lik = None: sum J^T J): chunks
 * of per-sample Jacobians contracted on the device.                                              */
LGNN_API int lgnn_diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags,
                         float* diag_out /* [P] */, float* loss_out, void* stream);

/* ---- full GGN over all weights of one mini-batch ---------------------------------------------------------------
 * Replaces CurvlinopsInterface.full (laplace/curvature/curvlinops.py:110-140: GGNLinearOperator @ I, one GGN-vector
 * product per column, curvlinops/ggn.py:44-75) = GGNInterface.full (laplace/curvature/curvature.py:374-410):
 * H_out[P, P] += sum_n J_n^T Lambda_n J_n (regression: sum_n J_n^T J_n, no factor), parameters in named_parameters
 * order; *loss_out += loss(model(idx), y) without the interface factor.  Chunks of per-sample Jacobians are mixed in
 * place with the Hessian square root and contracted by the fp32 MFMA Gram kernel; for models whose P x P fits.     */
LGNN_API int lgnn_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* H_out, float* loss_out,
                         void* stream);

/* ---- last-layer full GGN of one mini-batch ------------------------------------------------------
 * Replaces GGNInterface.full with last_layer_jacobians (laplace/curvature/curvature.py:132-167,
 * 374-410): J_n = [I_C (x) phi_n^T | s_n I_C], H_out[P_ll, P_ll] += sum_n J_n^T Lambda_n J_n,
 * P_ll = C*(D+1), weight index c*D+d then C bias entries.                                         */
LGNN_API int lgnn_lastlayer_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M,
                                   float* H_out, float* loss_out, void* stream);

/* What CurvatureInterface.last_layer_jacobians (laplace/curvature/curvature.py:132-167) builds its Jacobians from:
 * phi_out [M, D + 1] = [input row of the final nn.Linear seen from the batch node | bias scale s_n] (GraphSAGE:
 * [h_n | (A_bar h)_n | 1]; GCN: [(A_hat h)_n | rowsum(A_hat)_n]), f_out [M, C] = logits (or NULL);
 * J_n = [I_C (x) phi_n^T | s_n I_C].                                                                              */
LGNN_API int lgnn_lastlayer_features(lgnn_ctx* h, const int64_t* idx, int64_t M, float* phi_out, float* f_out, void* stream);

/* The same matrix accumulated in its natural layout: H = sum_n Lambda_n (x) phi~_n phi~_n^T, so block (c, c') of H is the
 * weighted Gram Phi~^T diag(Lambda[:, c, c']) Phi~ -- symmetric in (c, c') and inside the block.  S_pairs
 * [C (C + 1) / 2][D][D] (pairs c <= c' row major; the upper 32 x 32 sub-tiles of each block are valid) and Sb_pairs
 * [C (C + 1) / 2][D + 1] (bias column of each block) are caller-owned and ADDED to: a fit accumulates every batch
 * there (a data-parallel caller all-reduces them: half the bytes of H) and calls lgnn_lastlayer_pairs_place ONCE,
 * which adds the blocks into H_out [P_ll, P_ll] and mirrors the upper triangle.                                  */
LGNN_API int lgnn_lastlayer_pairs_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* S_pairs,
                                    float* Sb_pairs, float* loss_out, void* stream);
LGNN_API int lgnn_lastlayer_pairs_place(lgnn_ctx* h, const float* S_pairs, const float* Sb_pairs, float* H_out, void* stream);

/* ---- last-layer Kronecker and diagonal GGN of one mini-batch --------------------------------------
 * What KronLLLaplace / DiagLLLaplace (laplace/lllaplace.py:381-475, 477-...) ask of their backend on the final nn.Linear
 * alone: CurvlinopsInterface.kron (laplace/curvature/curvlinops.py:77-108) resp. GGNInterface.diag with
 * last_layer_jacobians (laplace/curvature/curvature.py:132-167, 412-432).  With f_n = W phi_n + s_n b per batch row
 * (phi_n, s_n as lgnn_lastlayer_features) and the KFAC seeds V_n [C, C] of lgnn_kfac_accumulate (flags:
 * LGNN_FLAG_FORK_EXACT_SEED or upstream's, for which V_n V_n^T = Lambda_n = diag(p_n) - p_n p_n^T):
 *   A_out  [D, D] += Phi^T Phi / n_train            Bb_out [C, C] += sum_n s_n^2 V_n V_n^T  (bias block; = B for GraphSAGE)
 *   B_out  [C, C] += sum_n V_n V_n^T                *loss_out     += sum_n CE(f_n, y_n)
 *   diag_out [C D + C] += diag(sum_n J_n^T Lambda_n J_n): [c D + d] += Lambda_n[c, c] phi_n[d]^2, [C D + c] += Lambda_n[c, c] s_n^2
 * All outputs are caller-owned fp32 device buffers that are ADDED to; the calls are asynchronous on `stream`.  Every batch
 * row is one sample (a repeated node id counts twice).  Classification only; models of any depth.  Nothing of size M C C
 * is written to memory: softmax and seeds live in registers / LDS, the sums are reduced per workgroup.                */
LGNN_API int lgnn_lastlayer_kron_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, int64_t n_train,
                                   uint32_t flags, float* A_out, float* B_out, float* Bb_out, float* loss_out, void* stream);
LGNN_API int lgnn_lastlayer_diag_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, float* diag_out,
                                   float* loss_out, void* stream);

/* Invalid batch contents (node ids outside [0, N), labels outside [0, C)) are detected on the device: such
 * samples contribute nothing and a sticky flag is raised.  This call synchronises `stream`, reports the flag
 * (non-zero return + message) and clears it; call it once per fit, not per batch.                          */
LGNN_API int lgnn_check_async_errors(lgnn_ctx* h, void* stream);
/* The same report WITHOUT synchronising: the flags are sticky words in pinned host memory, so this sees the errors of every kernel
 * that has finished; errors of work still in flight are reported by the next peek or check.  For callers that queue fit after fit
 * (a replayed hipGraph of a whole fit, DiagLaplace.fit_graph) and must not stall the stream once per fit; the reference's own
 * index errors on a CUDA / HIP device are asynchronous device-side asserts as well.                                          */
LGNN_API int lgnn_peek_async_errors(lgnn_ctx* h);

/* ---- batch-structure cache -----------------------------------------------------------------------
 * Part of what lgnn_kfac_accumulate* prepares per batch depends on the graph and the batch's node ids only, not on the
 * weights: the GCN top layer's active-row list and the path route's two-hop path list.  A caller that runs the same batches
 * fit after fit (gnn/marglik_training.py:125-127 builds its loader once, shuffle=False) names each batch with a non-zero tag
 * right before the accumulate call; the tag is consumed and cleared by that call.  The first accumulate under a tag runs
 * unchanged and only remembers the tag; the second builds an entry (one stream synchronisation: two counts size it); from
 * then on none of the list-building kernels is launched for that batch, for whole-batch, class-range and share calls alike.
 * The caller guarantees that one tag always names the same ids of the same length; as a guard every entry keeps a copy of
 * its ids, compared on the device on every use (lgnn_check_async_errors reports a difference).  Entries are dropped when
 * the graph changes (lgnn_update_adjacency), not by lgnn_invalidate.  LGNN_BATCH_CACHE_MB (read per call, default 2048;
 * 0 = off) bounds the device memory: least recently used entries go first, a batch larger than the budget is not cached.
 * Tag 0 / no call: nothing is cached.  Host-only calls.                                                              */
LGNN_API int lgnn_kfac_batch_tag(lgnn_ctx* h, uint64_t tag);
/* Forget a tag's entry (tag 0: every entry and every remembered tag). */
LGNN_API int lgnn_batch_cache_drop(lgnn_ctx* h, uint64_t tag);
/* out[5] = entries, device bytes, hits, misses, builds (accumulate calls under a tag on a route that uses the cache) */
LGNN_API int lgnn_batch_cache_stats(const lgnn_ctx* h, int64_t* out);

/* ---- timing hook (bench.py roofline) -----------------------------------------------------------
 * While enabled, every launch of the dominant kernel of the path in use -- KFAC: the fused SpMM^T -> Gram kernel of
 * the lowest layer; diagonal GGN: the first-layer kernel; last-layer full GGN: the batched weighted Gram -- is
 * bracketed by HIP events recorded on `stream` itself (torch.cuda.Event only sees torch's current stream).
 * lgnn_kernel_timing_read synchronises on the recorded events and returns the number of launches, their summed
 * duration in ms and the summed number of units they processed (KFAC: class planes; diagonal: samples; last layer:
 * class pairs); enabling resets the counters.                                                     */
LGNN_API int lgnn_enable_kernel_timing(lgnn_ctx* h, int enable);
LGNN_API int lgnn_kernel_timing_read(lgnn_ctx* h, int64_t* launches, double* total_ms, int64_t* planes);
/* The same events, launch by launch (host array of `capacity` doubles, milliseconds, in launch order; *launches = how many
 * were recorded): bench.py separates the full batches' launches from the short last batch's.  Synchronises on the events. */
LGNN_API int lgnn_kernel_timing_launches(lgnn_ctx* h, double* ms_out, int64_t capacity, int64_t* launches);

/* ---- per-sample Jacobians for the GLM predictive ("next" row) ------------------------------------
 * Replaces CurvatureInterface.jacobians (laplace/curvature/curvature.py:89-130, torch.func.jacrev of the dense
 * model): J [M, C, P] fp32 with J[m][c][:] = d f[idx[m], c] / d theta, parameters in named_parameters order
 * (per layer: weight [out, in] row major, then bias); f_out [M, C] = logits[idx] or NULL.  M*C*P floats, as the
 * reference; the samples are processed in chunks that fit the workspace cap.                              */
LGNN_API int lgnn_jacobians(lgnn_ctx* h, const int64_t* idx, int64_t M, float* J, float* f_out, void* stream);

/* ---- subnetwork Laplace: Jacobians and full GGN over a subset of the parameters ---------------------------------
 * What FullSubnetLaplace (laplace/subnetlaplace.py:175-199) asks of its backend: GGNInterface with subnetwork_indices
 * slices the columns of the whole Jacobian (laplace/curvature/curvature.py:127-128) and contracts the slice
 * (laplace/curvature/curvature.py:374-410).  `subnet` int64 [S] (device): DISTINCT indices in [0, P) into the parameter
 * vector of lgnn_jacobians (named_parameters order, weight row major, then bias), in any order; every output is in the
 * caller's order.
 *   lgnn_jacobians_subset:        J [M, C, S] = columns subnet[0..S) of lgnn_jacobians' J; f_out [M, C] = logits[idx] or NULL
 *   lgnn_subnet_full_accumulate:  H_out [S, S] += sum_n J_S,n^T Lambda_n J_S,n  (regression: sum_n J_S,n^T J_S,n, no factor);
 *                                 *loss_out += loss(model(idx), y) without the interface factor, as lgnn_full_accumulate
 * 1- and 2-layer GCN / GraphSAGE without res / norm: only the selected columns are built, from the closed form, with the
 * Hessian square root applied on the way (M C S floats written, 2 M C S^2 flops contracted); every other model: chunks of
 * lgnn_jacobians' rows and a column gather.  Chunks follow the workspace limit.  Invalid batch ids: zero rows and the sticky
 * flag, as lgnn_jacobians; an index outside [0, P): a zero column and the sticky flag (lgnn_check_async_errors).          */
LGNN_API int lgnn_jacobians_subset(lgnn_ctx* h, const int64_t* idx, int64_t M, const int64_t* subnet, int64_t S, float* J,
                          float* f_out, void* stream);
LGNN_API int lgnn_subnet_full_accumulate(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const int64_t* subnet,
                                int64_t S, float* H_out, float* loss_out, void* stream);

/* ---- functional (GP) Laplace: the kernel J J^T without the Jacobians ------------------------------------------------
 * What FunctionalLaplace (laplace/baselaplace.py:1922-2960) contracts from two batches' Jacobians (_kernel_batch :2684-2715,
 * _kernel_star :2717-2747, _kernel_batch_star :2749-2776, _mean_scatter_term_batch :2787-2812), with J as lgnn_jacobians
 * defines it.  idx_a [Ma], idx_b [Mb] int64 on the device; C = number of outputs.
 *   lgnn_gp_kernel writes (never accumulates) K = J(idx_a) J(idx_b)^T:
 *     flags == 0                  K[(n C + c) ldk + (m C + e)]: the [Ma C, Mb C] block, ldk >= Mb C
 *     LGNN_GP_INDEPENDENT         C planes K[c][n][m] = <J[n, c, :], J[m, c, :]>, row stride ldk >= Mb, plane stride Ma ldk
 *     LGNN_GP_MATCHED             Ma == Mb: K[n][c][e] = <J_a[n, c, :], J_b[n, e, :]> (dense [Ma, C, C]; ldk unused);
 *                                 with LGNN_GP_INDEPENDENT K[n][c] (dense [Ma, C])
 *     LGNN_GP_FROM_JACOBIANS      take the general route on any model (cross-check, timing baseline)
 *   lgnn_gp_jvp: out [M, C] = sum_p J[m, c, p] v[p] for v [P] on the device.
 * 1- and 2-layer GCN / GraphSAGE without res / norm: from per-sample tables of the first layer and the last layer's feature
 * rows, a batched NT GEMM on the fp32 matrix cores and a class contraction -- no Jacobian is written.  Every other model:
 * chunks of lgnn_jacobians' rows through the same NT GEMM.  Chunks follow the workspace limit.  No float atomics: two calls
 * on the same input return the same bits; with idx_a == idx_b (the same pointer) the result is exactly symmetric.  Invalid
 * ids: zero rows / columns and the sticky flag, as lgnn_jacobians (lgnn_check_async_errors).  With kernel timing enabled
 * the structured route records four event pairs per chunk pair: tables, NT GEMM, class contraction, placement.          */
#define LGNN_GP_INDEPENDENT 1
#define LGNN_GP_MATCHED 2
#define LGNN_GP_FROM_JACOBIANS 4
LGNN_API int lgnn_gp_kernel(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb, int flags,
                            float* K, int64_t ldk, void* stream);
LGNN_API int lgnn_gp_jvp(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* v, float* out, void* stream);

/* ---- joint GLM predictive: the cross-node covariance J P^-1 J^T ------------------------------------------------------
 * What _glm_predictive_distribution(joint=True) (laplace/baselaplace.py:1123-1158; the joint predictive :1223-1242) gets from
 * functional_covariance -- KronLaplace :1638-1644 through laplace/utils/matrix.py (inv_square_form), DiagLaplace :1905-1910,
 * FullLaplace :1491-1494 -- for a posterior that is block diagonal over the model's Linear layers, with J as lgnn_jacobians
 * defines it.  idx_a [Ma], idx_b [Mb] int64 on the device; C = number of outputs.
 *   K[(n C + c) ldk + (m C + e)] = sum_p sum_q J_a[n, c, p] (P^-1)[p, q] J_b[m, e, q]; written, never accumulated; ldk >= Mb C.
 * QA, QB, S are HOST arrays of n_blocks device pointers, blocks in lgnn_jacobians' order (convs.* first, then res.*); n_blocks
 * must be the model's number of Linear layers.  Per block l (weight [out_l, in_l], bias [out_l]):
 *   S[l]  [out_l, in_l + 1]  inverse precisions, the last column is the bias (the S0 convention of lgnn_glm_variance);
 *   Kronecker posterior: QA[l] [in_l, in_l], QB[l] [out_l, out_l], eigenvectors in columns, S[l][i, j] = 1 / (f lB_i lA_j +
 *     delta_W), S[l][i, in_l] = 1 / (f lB_i + delta_b) in QB[l]'s basis: the block of P^-1 is (Q_B (x) Q_A) diag(S) (Q_B (x) Q_A)^T;
 *   diagonal posterior: QA[l] = QB[l] = NULL and S[l] = 1 / precision of (W_l | b_l).
 * 1- and 2-layer GCN / GraphSAGE without res / norm (relu or tanh): from the tables and feature rows of lgnn_gp_kernel, no
 * Jacobian row is written (csrc/glmcov.hip has the stages and the flop count); every other model, and any model under
 * LGNN_COV_FROM_JACOBIANS: chunks of lgnn_jacobians' rows, rotated block by block, one side scaled.  Chunks follow the
 * workspace limit (a limit below one sample's buffers is an error); lgnn_glm_covariance_chunk_pairs: how many chunk pairs the last call computed.  No float atomics: two calls
 * on the same input return the same bits; with idx_a == idx_b (the same pointer) only the upper chunk pairs are computed and K
 * is exactly symmetric.  Invalid ids: zero rows / columns and the sticky flag (lgnn_check_async_errors).  Enqueues only.  With
 * kernel timing enabled the structured route records five event pairs per chunk pair: tables, V (rotations and scales), NT
 * GEMM, class contraction, placement.                                                                                      */
#define LGNN_COV_FROM_JACOBIANS 1
LGNN_API int lgnn_glm_covariance(lgnn_ctx* h, const int64_t* idx_a, int64_t Ma, const int64_t* idx_b, int64_t Mb,
                                 int n_blocks, const float* const* QA, const float* const* QB, const float* const* S,
                                 int flags, float* K, int64_t ldk, void* stream);
LGNN_API int64_t lgnn_glm_covariance_chunk_pairs(lgnn_ctx* h);

/* ---- low-rank Laplace: products of the Jacobian and of the GGN with a block of parameter directions ----------------
 * What LowRankLaplace (laplace/baselaplace.py:1679-1835) asks of its backend is eig_lowrank (laplace/curvature/
 * asdfghjkl.py:212-236: power iteration on Hessian-vector products, one vector at a time).  Here the curvature is the GGN of
 * lgnn_full_accumulate and a product takes a block V [k, P] of directions on the device; a direction is a contiguous row of
 * P floats (the layout of theta in lgnn_sampled_forward), parameters in lgnn_jacobians' order.
 *   lgnn_jvp_block:  out [M, C, k]: out[m, c, i] = <J[m, c, :], V[i, :]>  (written, never accumulated)
 *   lgnn_ggn_matmat: G [k, P]: G[i, :] += sum_n J_n^T Lambda_n J_n V[i, :], Lambda_n = diag(p_n) - p_n p_n^T (regression:
 *                    the identity, no interface factor, as lgnn_subnet_full_accumulate);
 *                    *loss_out += loss(model(idx), y) without the interface factor, as lgnn_full_accumulate
 *     LGNN_GGN_FROM_JACOBIANS     take the general route on any model (cross-check, timing baseline)
 * 1- and 2-layer GCN / GraphSAGE (relu or tanh) without res / norm: no Jacobian and no [rows, H k] intermediate reaches memory.
 * With in0 = [P X | rowsum P] (GCN) or [X | P X | 1] (GraphSAGE), R the rows the batch reads and D = act'(s), per direction
 * (dW0, db0, dW1, db1): q[r] = (D[r] . (in0[r] [dW0 | db0]^T)) W1^T + h[r] dW1^T on v_mfma_f32_32x32x2_f32 with D and W1 applied
 * while the tile is on chip (lgnn_sampled_forward's product, linearised); u[n] = sum_b P[n, b] (q[b] + db1); w[n] = Lambda_n u[n];
 * qbar[b] = sum_n P[n, b] w[n] as a gather over P^T's rows; g_b1 = sum_n rho_n w[n]; g_W1 = sum_r qbar[r]^T h[r]; sbar[r] = D[r] .
 * (qbar[r] W1) built in the prologue of the MFMA product [g_W0 | g_b0] = sum_r sbar[r]^T in0[r].  R is split into slabs whose
 * partial [k, P] outputs a second pass adds in slab order.  The directions go in chunks that keep q, u, w, qbar and the partials
 * under the workspace limit.  Every other model, and any model under LGNN_GGN_FROM_JACOBIANS: chunks of lgnn_jacobians' rows,
 * U = J_c V^T on the fp32 matrix cores, Lambda applied to U, G += (Lambda U)^T J_c.  The P x P matrix is never formed.  No float
 * atomics in the products: every element of out / G has one writer and a fixed summation order, two calls on the same input
 * return the same bits.  Invalid ids: zero rows and the sticky flag, as lgnn_jacobians (lgnn_check_async_errors).  With kernel
 * timing enabled lgnn_ggn_matmat records four event pairs per chunk (structured: forward + gather, curvature, qbar + bias, outer
 * products + finish; general: J V^T, Lambda, (Lambda U)^T J, the addition into G), lgnn_jvp_block one.
 *   lgnn_block_gram:  out [ka, kb] = A B^T for blocks of directions A [ka, P], B [kb, P] (written, never accumulated): the
 *                    Gram and Rayleigh-Ritz matrices of the block eigensolver on the same fp32 MFMA NT GEMM as lgnn_gp_kernel
 *                    (split-K partials added in slab order; A == B gives an exactly symmetric result).                     */
#define LGNN_GGN_FROM_JACOBIANS 1
LGNN_API int lgnn_block_gram(lgnn_ctx* h, const float* A, int64_t ka, const float* B, int64_t kb, int64_t P, float* out,
                             void* stream);
LGNN_API int lgnn_jvp_block(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* V /* [k, P] */, int64_t k,
                            float* out /* [M, C, k] */, void* stream);
LGNN_API int lgnn_ggn_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V /* [k, P] */, int64_t k,
                             int flags, float* G /* [k, P] */, float* loss_out, void* stream);

/* ---- exact Hessian of the loss: what it adds to the GGN, as a block product --------------------------------------------
 * CurvlinopsHessian (laplace/curvature/curvlinops.py:182-187) multiplies with the Hessian of the summed loss by double backward
 * (curvlinops/hessian.py).  That matrix is H = sum_n J_n^T Lambda_n J_n + R with R = sum_n sum_c r_nc grad^2 f_nc, r_n =
 * softmax(f_n) - onehot(y_n) (regression: r_n = f_n - y_n; GGN + R is then the interface's factor 0.5 times the Hessian of
 * MSELoss(sum)).  lgnn_ggn_matmat is the first term; this entry is the second:
 *   lgnn_hessian_resid_matmat: G [k, P]: G[i, :] += R V[i, :]   (directions and parameters laid out as in lgnn_ggn_matmat)
 * Plain 1- and 2-layer GCN / GraphSAGE (relu or tanh, no res / norm, both likelihoods) only: every other model is refused with
 * "exact Hessian: closed-form models only" -- its second derivatives are not in chunks of Jacobian rows.  One layer: R = 0, G is
 * left untouched.  Two layers, in lgnn_ggn_matmat's notation with D2 = act''(s) (0 for ReLU, -2 tanh(s) D for tanh), S [N, C]
 * the residual rows added at the batch's nodes (a repeated id adds) and G = P^T S (GraphSAGE: Gs = S, Gn = P^T S against W1 =
 * [W1a | W1b]), per direction (dW0, db0, dW1, db1):
 *   dS = in0 [dW0 | db0]^T,  E = D . dS,  T = (G dW1) . D + (G W1) . D2 . dS,
 *   (RV)_W1 = G^T E,  [(RV)_W0 | (RV)_b0] = T^T in0,  (RV)_b1 = 0
 * on the batch's needed rows: G as a gather over P^T's rows, G W1 once per call, dS and G dW1 on v_mfma_f32_32x32x2_f32 with
 * the elementwise step in registers, the two outer products in slabs added in slab order.  Only the residual rows, G, G W1, E, T
 * ([rows, H] per direction), the slab partials and G reach memory; the directions go in chunks under the workspace limit.  No
 * float atomics: two calls on the same input return the same bits.  An invalid id or label contributes zero and raises the
 * sticky flag (lgnn_check_async_errors).  Enqueues only.  With kernel timing enabled: one event pair per chunk.              */
LGNN_API int lgnn_hessian_resid_matmat(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* V /* [k, P] */,
                                       int64_t k, float* G /* [k, P] */, void* stream);

/* ---- gradient of the negative log marginal likelihood w.r.t. the adjacency ("next" row 8(f)-4) --------------
 * Replaces what autograd does for ``neg_marglik.backward()`` into ``model.adj`` (gnn/marglik_training.py:197-216):
 * back through KronDecomposed.logdet / log_marginal_likelihood (laplace/utils/matrix.py:371-394,
 * laplace/baselaplace.py:938-973), the KFAC accumulation the fork keeps attached to the graph (curvlinops/kfac.py:
 * 637-661 non-detached square root + create_graph, :789-790, :836-837), the forward passes, normalize_adj
 * (gnn/models/utils.py:106-112) and the straight-through binarisation (gnn/models/utils.py:42-86).  2-layer GCN,
 * ReLU, classification.  The caller supplies gamma_B[l] = d(neg marglik)/dB_l, gamma_A[l] = d/dA_l (from the
 * eigenpairs of the fitted factors; fp32 [out_l, out_l] / [in_l, in_l], symmetric).
 *   per batch :  grad_P [nnz] += the terms of this batch on the stored entries of the propagation matrix (order of
 *                lgnn_export_propagation);  out_bar [N, C] += d/d(all-node logits) of loss_scale * CE and of the seeds
 *   once      :  adds the forward-pass terms (a_scale = batches / N_train: A_1 = a_scale * H1^T H1) to grad_P, then
 *                grad_adj [nnz] = gradient w.r.t. the stored entries of the 0/1 adjacency, order of lgnn_export_adj
 *                (diagonal 0: fill_diagonal_(1) overwrites it; symmetric models: average of (i,j) and (j,i)).
 * Candidate edges (num_cand may be 0): the reference's dense adj.grad also has an entry for every NON-edge -- that is how
 * its structure learning proposes edges.  cand_a / cand_b int32 [num_cand] list pairs in the propagation matrix's
 * coordinates (entry (i, j) of the adjacency <-> a = j, b = i); grad_cand [num_cand] accumulates like grad_P and
 * lgnn_adjgrad_finish writes grad_cand_adj [num_cand] = d / d adj[i, j] (no symmetrisation: a symmetric model's caller
 * lists both orientations and averages).
 * Models bound with res / norm (lgnn_bind_extras; gnn/models/base_gnn.py:141-149 -- the STE-GCN configurations of Cornell /
 * Texas / Wisconsin / Circle, gnn/configs/original/stegcn_config.yaml:54-105, 129-145): GCN only.  gamma_B then has one more
 * entry per hidden layer after the conv entries (the res.{l} blocks, named_parameters order; res=True only); the chain gains
 * the norm's row-local backward, the res block's B and the adjoint of the pre-norm rows through the LayerNorm statistics.
 * All N rows, unfused kernels: these configurations are graphs of a few hundred to a few thousand nodes.
 * One-layer GCN models (the Banana block of gnn/configs/original/stegcn_config.yaml:108-127 and gcn_config.yaml: num_layers 1;
 * out = P (X W^T + 1 b^T), gnn/models/base_gnn.py:136-161 with a single conv): gamma_B / gamma_A are host arrays of ONE
 * pointer.  A_0 = X^T X a_scale does not depend on the adjacency (the Linear sees all N rows of X), so gamma_A is not read;
 * B_0 is the top layer of the chain above: gbar = 2 g Gamma_B, the seed SDDMM on the batch rows' entries, the seed adjoint
 * into out_bar; the finish adds <out_bar[a], Z[b]>, Z = X W^T + 1 b^T.  Any activation (there is none to apply).  One-layer
 * GraphSAGE, deeper models and the dense variants below for one layer are refused.                                        */
LGNN_API int lgnn_kfac_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags,
                            const float* const* gamma_B /* host array of L device ptrs */, float loss_scale,
                            float* grad_P, float* out_bar, const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand,
                            float* grad_cand, void* stream);
LGNN_API int lgnn_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* const* gamma_A /* host array of L device ptrs */,
                        float a_scale, float* grad_P, float* grad_adj, const int32_t* cand_a, const int32_t* cand_b,
                        int64_t num_cand, float* grad_cand, float* grad_cand_adj, void* stream);

/* The same gradient under a DIAGONAL posterior -- what the shipped STE-GCN configuration differentiates
 * (gnn/configs/original/stegcn_config.yaml:7 hessian_structure: diag; gnn/marglik_training.py:197-216 with DiagLaplace,
 * laplace/baselaplace.py:1848-1857; the fork's GGNInterface.jacobians keeps the graph, laplace/curvature/curvature.py:89-130,
 * so diag() (:412-432) is differentiable in the adjacency).  2-layer GCN, ReLU, classification.
 *   gamma [n_params] (parameter order W_0, b_0, W_1, b_1) = d(-marglik)/dH_p = f / (2 (f H_p + delta_p)), f = H_factor;
 *   per batch :  grad_P [nnz] += the terms on the stored entries of the batch nodes' rows;  out_bar [N, C] += d/d(logits) of
 *                loss_scale * CE and of the softmax inside the GGN;  h1_bar [N, H] += d/dH_1 and e_bar [N, F + 1] +=
 *                d/d[P X | rowsum(P)] of the closed-form diagonal;  candidates as above;
 *   once      :  lgnn_diag_adjgrad_finish propagates out_bar, h1_bar and e_bar through the forward pass into grad_P and writes
 *                grad_adj [nnz] / grad_cand_adj exactly like lgnn_adjgrad_finish.  It serves the diagonal and the full posterior
 *                (lgnn_full_adjgrad_batch below fills the same accumulators).
 * Workspace: [chunk][H][F + 1 rounded up to 4] floats for the first-layer tiles of a chunk of samples (0.5 GB for a Cora-shaped
 * batch), under the workspace limit (lgnn_set_workspace_limit); no synchronisation, nothing allocated after the first call.
 * Models bound with res / norm (GCN; the shipped WebKB / Circle configurations are exactly diag + res + LayerNorm): no closed
 * form of the diagonal GGN exists; gamma covers the res.{l} parameters too (after W_1, b_1), e_bar is left untouched, and per
 * (sample, class) the kernel chain runs one tangent forward pass along R = 2 Lambda J diag(gamma) and its reverse pass
 * (d sum_p gamma_p H_p = <K, d Lambda> + <R, d J>, K = J diag(gamma) J^T).  Workspace per sample of a chunk: 2 C P floats
 * (Jacobian rows and directions) + C N (3 H + C) floats of planes -- sized for graphs of a few hundred to a few thousand nodes.
 * Plain 2-layer GraphSAGE models (STEGraphSAGE + DiagLaplace; the driver offers the pair, gnn/utils.py:55-59, 81): the same identity,
 * evaluated locally -- everything of a (sample, class) pair lives on the rows {n} + N(n), one workgroup per pair, no planes; e_bar
 * [N, F + 1] carries the adjoint of P X in its first F columns, h1_bar the direct adjoint of H_1; workspace 2 C P floats per sample.
 * One-layer GCN models (stegcn_config.yaml:108-127, Banana: diag, num_layers 1): gamma [C F + C] in the order W [C, F] row
 * major, b [C]; h1_bar is ignored and may be NULL (both calls).  With psi_n = [P X | rowsum(P)][n] the diagonal GGN is
 * H_{(c, j)} = sum_n p_c (1 - p_c) psi_n[j]^2 (laplace/curvature/curvature.py:412-432 on J_n[c, (c', j)] = delta_cc' psi_n[j]),
 * so a batch only adds to out_bar and e_bar, one wave per sample: kappa_c = sum_j Gamma_c[j] psi_j^2, pbar_c = (1 - 2 p_c)
 * kappa_c, out_bar[n] += p * (pbar - <p, pbar>) + loss_scale (p - onehot(y)), e_bar[n] += 2 psi * sum_c p_c (1 - p_c) Gamma_c;
 * grad_P and the candidates take <out_bar[a], Z[b]> + <e_bar[a, :F], X[b]> + e_bar[a, F] in the finish.  No workspace beyond
 * the batch prologue's.                                                                                                    */
LGNN_API int lgnn_diag_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                            float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                            const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand, float* grad_cand, void* stream);
LGNN_API int lgnn_diag_adjgrad_finish(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar, float* grad_P,
                             float* grad_adj, const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand,
                             float* grad_cand, float* grad_cand_adj, void* stream);

/* The same gradient under the FULL posterior -- the third choice of the structure-learning loop's --hessian_structure
 * (gnn/utils.py:57-59; gnn/marglik_training.py:197-216 with FullLaplace, laplace/baselaplace.py:1377-1505; the full GGN it
 * differentiates: laplace/curvature/curvature.py:374-410 over the fork's attached Jacobians, :89-130).  The identity of the
 * diagonal posterior's (sample, class) chains does not need a diagonal weighting: with
 *   Gamma [P, P] fp32, symmetric = d(1/2 logdet(f H + Delta))/dH = (f / 2) (f H + Delta)^-1, f = H_factor,
 *   K_n = J_n Gamma J_n^T [C, C],  R_n = 2 Lambda_n J_n Gamma [C, P]   (one fp32-MFMA pass over J Gamma, csrc/fulladj.hip;
 *   K_n's partial sums over the column blocks meet in float atomics),
 * d<Gamma, H> = sum_n <K_n, d Lambda_n> + sum_{n,c} <R_n[c, :], d J_n[c, :]>, and the tangent / reverse chains are the diagonal
 * posterior's.  lgnn_full_adjgrad_batch has the buffer contract of lgnn_diag_adjgrad_batch: it accumulates into grad_P, out_bar
 * (incl. loss_scale * CE's adjoint), h1_bar, e_bar and grad_cand, runs chunks of samples under the workspace limit, takes
 * repeated node ids, does not synchronise, and is finished by lgnn_diag_adjgrad_finish.  2-layer GCN, plain or with res / norm
 * (the planes chain; e_bar stays untouched; workspace per sample of a chunk 2 C P floats + C N (3 H + C) floats of planes), and
 * plain 2-layer GraphSAGE (the local chain; 2 C P floats per sample); ReLU, classification, C <= 127.  Gamma is read as
 * stored; parameter order W_0, b_0, W_1, b_1[, Wr_0, br_0].
 * lgnn_full_directions is the product alone: K_out [M, C, C] and R_out [M, C, P] of the samples idx (Lambda_n from the softmax
 * of the model's logits), e.g. K_n = J_n Sigma J_n^T for Gamma = Sigma; same chunks, only the Jacobian rows in the workspace.
 * One-layer GCN models: Gamma in the order W [C, F] row major, b [C]; h1_bar is ignored and may be NULL.  K_n and R_n come from
 * the closed-form Jacobian rows and the same product kernel (2 C P floats per sample of a chunk); no tangent pass, no planes:
 * d J_n[c, :] = delta_cc' d psi_n, hence e_bar[n, j] += sum_c R_n[c, pos(c, j)], pos(c, j) = c F + j / C F + c for j = F.
 * Both entry points take one-layer GCN models.                                                                             */
LGNN_API int lgnn_full_adjgrad_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* Gamma,
                            float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar,
                            const int32_t* cand_a, const int32_t* cand_b, int64_t num_cand, float* grad_cand, void* stream);
LGNN_API int lgnn_full_directions(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* Gamma, float* K_out, float* R_out,
                         void* stream);

/* ---- the adjacency gradient on ALL N x N pairs (LoRASTEGCN, gnn/models/models.py:186-235) --------------------------------
 * LoRA parameterises the whole adjacency, adj0 + scaling * (adj_lora_B @ adj_lora_A) (models.py:226-232), so the gradient
 * that neg_marglik.backward() leaves in A and B (gnn/marglik_training.py:197-216) needs d(-marglik)/d adj on every pair.
 * The same chains as lgnn_kfac_adjgrad_batch / lgnn_adjgrad_finish and lgnn_diag_adjgrad_batch / _finish, but the caller's
 * grad_adj_dense [N, N] (fp32, row major, zeroed before the first batch) takes the place of grad_P, candidates and grad_adj:
 * every per-pair term becomes a tile GEMM on the full grid (fp32 MFMA, lora.hip), the _finish call turns it in place into
 * grad_adj_dense[i, j] = d(-marglik)/d adj[i, j]: normalize_adj backward (gnn/models/utils.py:106-112), the STE as identity
 * (gnn/models/utils.py:42-86), a symmetric model's (i, j) / (j, i) average, the diagonal 0 (fill_diagonal_(1)).  Between the
 * calls the buffer holds d/dP on the grid.  Plain 2-layer GCN (no res / norm), N^2 < 2^31.  Workspace: the same as the
 * sparse chains; the Kronecker batch runs all N rows (as with candidates).                                                  */
LGNN_API int lgnn_kfac_adjgrad_batch_dense(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, uint32_t flags,
                                  const float* const* gamma_B /* host array of 2 device ptrs */, float loss_scale,
                                  float* out_bar, float* grad_adj_dense, void* stream);
LGNN_API int lgnn_adjgrad_finish_dense(lgnn_ctx* h, const float* out_bar, const float* const* gamma_A, float a_scale,
                              float* grad_adj_dense, void* stream);
LGNN_API int lgnn_diag_adjgrad_batch_dense(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                  float loss_scale, float* out_bar, float* h1_bar, float* e_bar, float* grad_adj_dense,
                                  void* stream);
LGNN_API int lgnn_diag_adjgrad_finish_dense(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar,
                                   float* grad_adj_dense, void* stream);

/* ---- the all-pairs gradient in ROW BANDS (DiagLaplace.propose_edges) -------------------------------------------------------
 * The reference's structure learning moves every entry of a dense adj along adj.grad (gnn/marglik_training.py:197-224): a
 * non-edge becomes an edge when its entry of d(-marglik)/d adj is negative enough.  The _dense calls above hold that gradient
 * as N x N floats; these calls hold [a1 - a0, N] of it at a time.  Under the diagonal posterior the GGN is a sum over
 * samples (laplace/curvature/curvature.py:412-432), the per-sample all-pairs term of a sample writes only the row of its own
 * node, and the remaining terms of row a are <out_bar[a], Z1[b]> + <Hb[a], Z0[b]> + <e_bar[a, :F], X[b]> + e_bar[a, F] over
 * whole-graph adjoints -- so a band of rows needs the samples whose node lies in it and the band's rows of three tile GEMMs.
 * Plain directed 2-layer GCN (no res / norm, symmetric = 0), ReLU, classification.
 *   lgnn_diag_adjgrad_band_sparse, per batch: lgnn_diag_adjgrad_batch without candidates -- the same accumulators, the same
 *     sums -- with every sum in a fixed order, so that two runs leave the same bits: no float atomic in LDS, and one
 *     workgroup adds the chunk's samples to grad_P, out_bar, h1_bar and e_bar one after the other (slower per batch than the
 *     parallel scatter; the bands dominate the pass).
 *   lgnn_diag_adjgrad_band_prepare, once: Z1 [N, C] = H_1 W_1^T + b_1, Z0 [N, H] = X W_0^T + b_0, Hb [N, H] = act'(h_1) *
 *     (P^T out_bar W_1 + h1_bar); grad_P [nnz] is completed in place as lgnn_diag_adjgrad_finish completes it (the three
 *     bilinear terms on the stored entries); rs / cs [N] = the row / column sums of grad_P * P behind normalize_adj
 *     backward's rt_i (gnn/models/utils.py:106-112), summed in a fixed order; all outputs caller owned.
 *   lgnn_diag_adjgrad_band_batch, per band and sub-batch: band [a1 - a0, N] (zeroed by the caller; 64-bit row offsets) += the
 *     per-sample all-pairs term of lgnn_diag_adjgrad_batch_dense for samples whose node lies in [a0, a1); nothing else is
 *     accumulated.  Repeated node ids and chunks under the workspace limit as there; a node outside the band contributes
 *     nothing, an id outside the graph raises the sticky flag (lgnn_check_async_errors).
 *   lgnn_diag_adjgrad_band_finish, per band: adds the three bilinear terms for the rows [a0, a1) (fp32 MFMA tiles) and turns the
 *     band in place into band[j - a0, i] = d(-marglik)/d adj[i, j] = G[j, i] d_i d_j + rt_i (the STE as identity,
 *     gnn/models/utils.py:42-86); the diagonal and the stored entries of the adjacency leave as +inf, so that a smallest-k
 *     selection over the band sees the non-edges only.  One writer per element, no float atomics on the band.
 * None of the four synchronises.                                                                                           */
LGNN_API int lgnn_diag_adjgrad_band_sparse(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                  float loss_scale, float* grad_P, float* out_bar, float* h1_bar, float* e_bar, void* stream);
LGNN_API int lgnn_diag_adjgrad_band_prepare(lgnn_ctx* h, const float* out_bar, const float* h1_bar, const float* e_bar,
                                   float* grad_P, float* Hb, float* Z0, float* Z1, float* rs, float* cs, void* stream);
LGNN_API int lgnn_diag_adjgrad_band_batch(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, const float* gamma,
                                 int64_t a0, int64_t a1, float* band /* [a1 - a0, N] */, void* stream);
LGNN_API int lgnn_diag_adjgrad_band_finish(lgnn_ctx* h, const float* out_bar, const float* Hb, const float* Z0, const float* Z1,
                                  const float* e_bar, const float* rs, const float* cs, int64_t a0, int64_t a1,
                                  float* band /* [a1 - a0, N] */, void* stream);

/* ---- LoRA structure learning (LoRASTEGCN) -----------------------------------------------------------------------------
 * lgnn_lora_threshold: re-binarise the LoRA adjacency (gnn/models/models.py:226-230) against the stored pattern and edit it
 * in place (lgnn_update_adjacency).  For every off-diagonal pair: t = (B @ A)[i, j] * scaling, m = adj0[i, j] + t, symmetric
 * models (m_ij + m_ji) / 2; stored afterwards iff m > threshold.  base_rowptr / base_col: int32 CSR of adj0's 0/1 pattern
 * (sorted columns); lora_A [r, N], lora_B [N, r] fp32.  The flips are compacted on the device; only their number reaches the
 * host (*num_flips; synchronises the stream).  The diagonal is never edited (the GCN's self loops).
 * lgnn_lora_grad: grad_A [r, N] = scaling B^T G and grad_B [N, r] = scaling G A^T (overwritten) from the dense gradient G of
 * lgnn_*_finish_dense; one pass over row tiles of G, grad_A's partials summed in a fixed order.  1 <= r <= 64.           */
LGNN_API int lgnn_lora_threshold(lgnn_ctx* h, const int32_t* base_rowptr, const int32_t* base_col, const float* lora_A,
                                 const float* lora_B, int64_t r, float scaling, float threshold, int symmetric,
                                 int64_t* num_flips, void* stream);
LGNN_API int lgnn_lora_grad(lgnn_ctx* h, const float* grad_adj_dense, const float* lora_A, const float* lora_B, int64_t r,
                            float scaling, float* grad_A, float* grad_B, void* stream);

/* ---- matrix-free GLM predictive ("next" row 8(f)-3 at scale) -------------------------------------------------------
 * Replaces the Jacobian route of the default la(x) (laplace/baselaplace.py:1123-1158 + laplace/utils/matrix.py:396-451 resp.
 * baselaplace.py:1901-1903) for 1- and 2-layer GCN and GraphSAGE models: f_mu [M, C] = logits and f_var_diag [M, C] = diag(J P^-1 J^T) per
 * evaluation node from the closed-form Jacobian, nothing of size M * C * P is formed.  The probit link (the default,
 * baselaplace.py:610-616) needs exactly this diagonal.
 *   Kronecker posterior: QA0 [F, F], QB0 [H, H], QA1 [H, H] = eigenvectors (columns) of A_0, B_0, A_1;
 *     S0 [H, F + 1]: 1 / (f lB0_i lA0_j + delta_W0), column F: 1 / (f lB0_i + delta_b0);  S1 [C, H]: 1 / (f lB1_i lA1_j + delta_W1);
 *     QB1sq [C, C] = Q_B1[c, i]^2;  kappa [C] = sum_i Q_B1[c, i]^2 / (f lB1_i + delta_b1)      (bias blocks share Q_B)
 *   diagonal posterior: QA0 = QB0 = QA1 = QB1sq = NULL; S0 [H, F + 1] = 1 / precision of (W_0 | b_0), S1 [C, H] of W_1,
 *     kappa [C] of b_1.
 *   GraphSAGE: F and the H of QA1 / S1's second dimension read as the widths of what the two Linear layers multiply
 *     (2 F and 2 H: cat = [h | P h], gnn/models/layers.py:26-29).
 *   One-layer models (GCN and GraphSAGE; gnn/configs/original/gcn_config.yaml, Banana: num_layers 1): QA0 = QB0 = S0 = NULL and
 *     QA1 [F', F'], S1 [C, F'], QB1sq, kappa describe the ONLY layer, F' = the width its Linear multiplies (F, GraphSAGE 2 F).
 *     J_n[c, (c', j)] = delta_cc' xt_n[j] with xt_n = (P X)[n], bias entry rho_n = rowsum(P)[n] (GraphSAGE: xt_n = [x_n | (P X)_n],
 *     rho_n = 1):  Kronecker  var_n[c] = sum_a Q_B[c, a]^2 sum_i S1[a, i] (Q_A^T xt_n)_i^2 + kappa[c] rho_n^2,
 *     diagonal  var_n[c] = sum_i S1[c, i] xt_n[i]^2 + kappa[c] rho_n^2.  The mapped variant reads W1m's rows as Cm only.
 *   Activation: this entry and the mapped one read act' as a float per hidden unit and accept relu and tanh alike (checked
 *     against the Jacobian route under tanh, tests/test_gpu_tanh.py); lgnn_glm_variance_ext and every adjacency-gradient
 *     entry (lgnn_*_adjgrad_*, lgnn_full_directions) refuse a 2-layer tanh model with a message naming ReLU.                */
LGNN_API int lgnn_glm_variance(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* QA0, const float* QB0, const float* S0,
                      const float* QA1, const float* S1, const float* QB1sq, const float* kappa, float* f_mu,
                      float* f_var_diag, void* stream);
/* The same for a linear map of the logits: var_mapped [M, Cm] = diag(E J P^-1 J^T E^T) for E [Cm, C], handed over as the
 * mapped head W1m = E W_1 [Cm, in_dim_1] (row major; GraphSAGE: both halves).  With E = [I ; 1^T / C ; I + 1 1^T / C]
 * (Cm = 2 C + 1) polarisation gives the row sums and the total of the C x C predictive covariance next to its diagonal --
 * all that the Laplace bridge with its zero-mean correction reads (link_approx "bridge" / "bridge_norm",
 * laplace/baselaplace.py:637-661: f_var.sum(-1), f_var.sum((1, 2)), diagonal) -- so those links no longer need Jacobians.
 * Operands as above except: Kronecker posterior S1 [C, .] as above, QB1sq [Cm, C] = (E Q_B1)[r, i]^2,
 * kappa [Cm] = sum_i (E Q_B1)[r, i]^2 / (f lB1_i + delta_b1);  diagonal posterior S1 [Cm, .] = (E * E) S1,
 * kappa [Cm] = (E * E) kappa (elementwise squares of E: the posterior is independent across parameters).
 * f_mu [M, C] stays the model's logits (may be NULL).  Cm <= 4096.                                                  */
LGNN_API int lgnn_glm_variance_mapped(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* W1m, int64_t Cm,
                             const float* QA0, const float* QB0, const float* S0, const float* QA1, const float* S1,
                             const float* QB1sq, const float* kappa, float* f_mu, float* var_mapped, void* stream);

/* The same predictive for 2-layer GCN / GraphSAGE models built with res=True and / or norm="layer"|"batch" -- the reference's
 * shipped GCN configurations for Cornell / Texas / Wisconsin (gnn/configs/original/gcn_config.yaml:36-58), evaluated by the
 * driver with exactly this call (gnn/marglik_training.py:332-353) -- and, through the same route, for plain ones.  Replaces
 * the same reference lines as lgnn_glm_variance (laplace/baselaplace.py:1123-1158 + laplace/utils/matrix.py:396-451 resp.
 * baselaplace.py:1901-1903), whose autograd walks res[0] and norms[0] (gnn/models/base_gnn.py:136-161) once per class and
 * evaluation node: here the norm's transposed Jacobian is applied in closed form to d_u * w_c, one wave per (node, class) row.
 * The res.0 block (nn.Linear on X, gnn/models/base_gnn.py:100-113) adds one more first-layer term of the same shape.
 *   W1m [Cm, in_dim_1] / Cm: as lgnn_glm_variance_mapped, or NULL / 0 for the model's own classes (S1 / QB1sq / kappa are the
 *     mapped operands under a map);
 *   QA0 .. kappa: as lgnn_glm_variance;
 *   res.0, Kronecker posterior: QAr [F, F], QBr [H, H] = eigenvectors (columns) of A_r = X^T X's factor and B_r;
 *     Sr [H, F + 1]: 1 / (f lBr_i lAr_j + delta_Wr), column F: 1 / (f lBr_i + delta_br)  (F = the feature width for both
 *     families: res.0 reads X itself);  diagonal posterior: QAr = QBr = NULL, Sr = 1 / precision of (W_r | b_r);
 *     all three NULL for a model without res.
 * ReLU, hidden width <= 256.  The norm's own parameters are not Laplace parameters (laplace/curvature/curvature.py:74-79).
 * An id out of range: sticky flag (lgnn_check_async_errors), variance row 0.                                           */
LGNN_API int lgnn_glm_variance_ext(lgnn_ctx* h, const int64_t* idx, int64_t M, const float* W1m, int64_t Cm,
                          const float* QA0, const float* QB0, const float* S0, const float* QA1, const float* S1,
                          const float* QB1sq, const float* kappa, const float* QAr, const float* QBr, const float* Sr,
                          float* f_mu, float* f_var, void* stream);

/* ---- decomposition of the fitted factors ("next" row: KronLaplace.fit -> Kron.decompose) ----------
 * Replaces the per-factor torch.linalg.eigh calls of laplace/utils/matrix.py:118-145 (symeig,
 * laplace/utils/utils.py:193-226) by one call for all factors: n <= 256 -- a one-workgroup Householder tridiagonalisation
 * per factor (all factors side by side), a one-workgroup divide and conquer on the tridiagonal matrices (lgnn_tridiag_eig
 * below), a back-transformation kernel; 256 < n <= 512 (n % 4 == 0) -- the same with rocSOLVER's divide and conquer (one
 * chain per factor on side streams joined back into `stream`); larger n -- ONE strided-batched rocSOLVER syevd.
 * A: device fp32 [batch][n][n], symmetric, overwritten with the eigenvectors: ROW j of matrix b is the unit eigenvector of
 * eigenvalue W[b][j]; W: device fp32 [batch][n], ascending; info: device int32 [batch] (0 = converged).  Asynchronous on
 * (n <= 256: 1 = a NaN or Inf in the factor).  Asynchronous on `stream`; no graph handle involved.    */
LGNN_API int lgnn_symeig_batched(float* A, int64_t n, int64_t batch, float* W, int32_t* info, void* stream);

/* The divide and conquer step of the n <= 256 route on its own (csrc/eigh.hip, tridiag_dc_kernel): eigenpairs of `batch`
 * symmetric tridiagonal matrices, diagonal d [batch][n] and off-diagonal e [batch][n] (the last entry of each row unused),
 * device fp32, in place: d <- eigenvalues ascending, ROW j of Z [batch][n][n] <- unit eigenvector j; info[b] = 1 where d or e
 * holds a NaN or Inf (d and Z of that matrix are left alone), else 0.  1 <= n <= 256.  Asynchronous on `stream`.     */
LGNN_API int lgnn_tridiag_eig(float* d, float* e, int64_t n, int64_t batch, float* Z, int32_t* info, void* stream);

/* ---- kNN initial graph (the reference's `--init_graph knng` configurations) ----------------------
 * Replaces torch_geometric.nn.knn_graph(X, k, loop=False, cosine=False) inside get_knn_graph (gnn/utils.py:355-369, handed
 * to the model at gnn/marglik_training.py:407-408): the exact k nearest neighbours of every row of X by squared Euclidean
 * distance, self excluded, without forming N x N distances (csrc/knn.hip: a Gram-form filter on the fp32 matrix cores keeps
 * 64 candidates per row, they are re-ranked in the difference form, a per-row certificate decides whether that was enough,
 * the rows without one are recomputed by brute force -- the result is exact either way).
 *   X: device fp32 [N, F], row stride ld >= F floats (64-bit row offsets);  1 <= k <= 32, k < N < 2^31, F >= 1;
 *   nbr: device int32 [N, k], dist: device fp32 [N, k], ascending per row.
 * Order: by (d, index) with d the fp32 difference form sum_f (x_f - y_f)^2 (one fixed summation order); equal d: the
 * smaller index first.  Two calls on the same input agree bit for bit.  X is expected to be finite.
 *   num_fallback: HOST int64, the number of rows that took the brute-force route.
 * The call synchronises `stream` once (to read that count; a second time, after the brute force, if the count is not zero).
 * No graph handle involved; the workspace (O(N * 64 * splits)) lives for the call.  Anything else: an error through
 * lgnn_last_error.                                                                                                      */
LGNN_API int lgnn_knn(const float* X, int64_t N, int64_t F, int64_t ld, int k, int32_t* nbr, float* dist,
                      int64_t* num_fallback, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LAPLACE_GNN_HIP_H */
