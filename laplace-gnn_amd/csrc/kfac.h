// What the translation units of the KFAC accumulate share -- kfac_seed.hip (batch marks, seeds, prologue / epilogue),
// kfac_top.hip (the top layer's kernels and launchers), kfac.hip (plan, steps, driver, C entry points).  What other files use
// (batch_prologue, batch_epilogue, kfac_top_planes, plan_kfac, kfac_accumulate, record_event) is declared in lgnn_internal.h.
// A kernel lives in exactly one file; another file reaches it through a launcher declared here.
#pragma once
#include "device_utils.h"
#include "lgnn_internal.h"

namespace lgnn {

// A batch's rows as flags [N], their sorted list and its length on the device: the workspace's buffers or a cache entry's
struct ActiveRows { const uint8_t* flags; const int32_t* list; const int32_t* count; };

// ---- kfac_top.hip ---------------------------------------------------------------------------------------------------------------
// Which rows a row list holds: the columns of the batch nodes' P rows (the rows of the GCN top-layer gradient that are not
// identically zero), the batch nodes themselves (GraphSAGE's), or both (what one more propagation can reach)
enum : int { kRowsNeighbours = 1, kRowsBatch = 2, kRowsBoth = 3 };
// flags [N] = 1 on those rows, 0 elsewhere: reserve, memset, the mark kernel(s)
int mark_rows(lgnn_ctx* h, const int64_t* idx, int64_t M, int which, DevBuf& flags, hipStream_t s);
// The row-list builder: mark_rows, then compact_rows (list / count = the sorted ids of those rows and how many); the triple is
// returned in *out.  (A caller with a launch of its own between the two halves calls them one by one.)
int build_row_list(lgnn_ctx* h, const int64_t* idx, int64_t M, int which, DevBuf& flags, DevBuf& list, DevBuf& count,
                   hipStream_t s, ActiveRows* out = nullptr);
// GCN top layer over the listed rows with the Gram fused in (seed_spmm_gram_kernel, sliced hubs included):
// scratch [C, C] += B_{L-1} of the classes [cb, ce); g (optional): the class-major planes of those rows
int launch_seed_spmm_gram(lgnn_ctx* h, bool fork_exact, float* g, int64_t cb, int64_t ce, float* scratch, const ActiveRows& rows,
                          hipStream_t s);
// GCN top layer from the seed blocks in ws.seeds, all N rows: planes [cb, ce) of g and the row flags ws.active
int launch_seed_spmm(lgnn_ctx* h, float* g, int64_t cb, int64_t ce, hipStream_t s);
// GraphSAGE top layer: planes [cb, ce) of g at the batch nodes = their seed blocks (the other rows are not written)
int launch_scatter_seed_planes(lgnn_ctx* h, const int64_t* idx, int64_t M, float* g, int64_t cb, int64_t ce, hipStream_t s);

}  // namespace lgnn
