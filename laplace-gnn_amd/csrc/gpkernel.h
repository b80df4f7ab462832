// The pieces of the structured J J^T route (gpkernel.hip) that the joint GLM predictive (glmcov.hip) runs too: the first
// layer's tables and the [phi | s] rows of a chunk of samples, the class pairs of W_1, the placement into the caller's
// [(n, c), (m, e)] layout and the mirror of the upper triangle.  launch_nt_gemm and NtProblem: lgnn_internal.h.
#pragma once
#include "closedform.h"
#include "lgnn_internal.h"

namespace lgnn {

// the structured route's view of the bound model: the closed form's operands and the table geometry
struct GpModel {
  ClosedForm cf;
  int64_t Z, Zp;      // tables per sample, table pairs (0 for one-layer models)
  int64_t ld, ldp;    // row strides of the tables and of the [phi | s] rows
};
int gp_model(lgnn_ctx* h, GpModel& g);  // needs forward_ensure_aux

// tables T [z][mc][ld] (gp_table_kernel) and rows Phi [mc][ldp] = [phi_n | s_n | 0 ..] of the samples idx[0..mc); ids outside
// [0, N): zero rows and the sticky flag
int build_tables(lgnn_ctx* h, const GpModel& g, const int64_t* idx, int64_t mc, float* T, float* Phi, hipStream_t s);

// Wp[q * ldw + (ab * H + h)] = W^al[c, h] W^be[e, h];  q = c * C + e, or q = c = e with diag_only (gp_wpair_kernel)
int launch_wpair(const float* W1, int64_t w1_ld, int64_t H, int64_t C, bool sage, bool diag_only, float* Wp, int64_t ldw,
                 hipStream_t s);

// K[(n C + c) ldk + (m C + e)] = Kt[(c C + e) pairs + n mb + m] + [c == e] S[c s_cs + n mb + m] + Add[(n C + c) mb C + m C + e]
// for n < ma, m < mb; Kt, S and Add may each be null (0)
int launch_place_full(const float* Kt, int64_t pairs, const float* S, int64_t s_cs, const float* Add, int64_t ma, int64_t mb,
                      int64_t C, float* K, int64_t ldk, hipStream_t s);

// lower triangle <- upper triangle of `planes` D x D matrices with row stride ld
int launch_mirror(float* K, int64_t D, int64_t ld, int64_t planes, int64_t plane, hipStream_t s);

struct StageTimer {  // lgnn_enable_kernel_timing: one event pair per stage of every chunk pair, in stage order
  lgnn_ctx* h; hipStream_t s;
  int mark() { return h->timing ? record_event(h, s) : 0; }
};

}  // namespace lgnn
