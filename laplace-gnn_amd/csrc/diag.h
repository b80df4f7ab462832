// What diag.hip shares with fisher.hip: the empirical / Monte-Carlo Fisher's diagonal is the closed-form diagonal GGN with
// other weights (q rows from the residuals, last-layer weights r^2), so it runs diag.hip's register-staged first-layer kernel
// and its last-layer kernel.  A kernel lives in exactly one file; another file reaches it through a launcher declared here.
// (The matrix-core first-layer kernels and the tile reduction are diag_accumulate's alone and stay inside diag.hip.)
#pragma once
#include "lgnn_internal.h"

namespace lgnn {

// samples per workgroup slab of the two kernels below at about `target` workgroups, in [8, 64]
int64_t diag_slab(const lgnn_ctx* h, int64_t M, int64_t target);
// 2-layer models: diag_out[W_0 | b_0] += sum_n q-weighted squares of the first layer's closed-form rows; q [1 or 3][M][H]
// (diag_first_layer_kernel<GraphSAGE ? 1 : 0>)
int launch_diag_first_layer_staged(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, const float* q, float* diag_out,
                                   hipStream_t s);
// out[W_last | b_last] += sum_n wgt[n, k] phi~_n^2 (diag_last_layer_kernel); wgt [M, C], null: p_k (1 - p_k) from ws.probs
int launch_diag_last_layer(lgnn_ctx* h, const int64_t* idx, int64_t M, int64_t slab, const float* wgt, float* out,
                           hipStream_t s);

}  // namespace lgnn
