// What the structured GGN product (ggnmat.hip) shares with the exact Hessian's residual product (hessmat.hip): the shapes of a
// closed-form model, the batch's opening, and launchers of the transposed gather and of the slab-wise outer product.  The
// kernels stay in ggnmat.hip; their header comment there describes them.
#pragma once
#include "lgnn_internal.h"

namespace lgnn {

struct TnArgs {
  const float* A; int64_t a_ld, a_ds;   // A[i * a_ds + t * a_ld + a]: qbar [kc][rcap][Cz] or w [kc][M][C]
  int64_t acols;                         // its columns
  int mode;                              // 0: At = A's tile;  1: At[t][h] = D[row_t][h] sum_cz A[t][cz] W1z[cz][h]
  const float* W1; int64_t ld1, C, H;    // mode 1
  const float* dact;
  const float* B; int64_t b_ld, bcols;   // B[row * b_ld + b]: in0 or h
  const float* in0; int64_t ldk, Fp;     // the bias column in0[row * ldk + Fp] (bias_off >= 0)
  const int32_t* rows; const int32_t* count;
  int64_t adim;                          // output rows: H (mode 1) or acols
  int64_t ooff, old, amod, ashift;       // output element (a, b) at ooff + (a % amod) * old + (a / amod) * ashift + b
  int64_t bias_off;                      // -1: none; else element a of sum_t At[t][a] bcol[t] at bias_off + a
  float* part; int64_t P, kc;            // part[(slab * kc + i) * P + ...]
  int btiles;
  // hessmat.hip: B belongs to the direction and is listed like A, B[i * b_ds + t * b_ld + b] (0, 0: B[row_t * b_ld + b])
  int64_t b_ds; int b_listed;
};

// the shapes and operands the structured drivers read (sampled.hip's parameter layout)
struct StructModel {
  bool two, sage;
  int64_t N, Fp, H, C, Cz, ld1, off1, offb, P, rcap;
};

constexpr int kMaxSlabs = 16;

// forward_ensure_aux, the model's shapes, in0 and the batch's needed rows (SampledState::rows / count / rpos)
int struct_prepare(lgnn_ctx* h, const int64_t* idx, int64_t M, StructModel& m, hipStream_t s);
// slabs of R's row tiles for a chunk of kc directions and `tiles` output tiles: about 1024 workgroups (the shapes alone)
int struct_slabs(const StructModel& m, int64_t kc, int64_t tiles);
// qbar [kc][rcap][Cz] = the gather of w [kc][M][C] over P^T's rows (ggn_qbar_kernel, the batch prologue's pos / mult)
int launch_ggn_qbar(lgnn_ctx* h, const StructModel& m, const float* w, int64_t M, int64_t kc, float* qbar, hipStream_t s);
// ggn_tn_kernel over (nslab, t.kc, output tiles); ggn_finish_kernel: G [kc * P] += the slabs' partials in slab order
int launch_ggn_tn(const TnArgs& t, int nslab, int64_t atiles, hipStream_t s);
int launch_ggn_finish(const float* part, int nslab, int64_t per, float* G, hipStream_t s);

}  // namespace lgnn
