// What the translation units of the path route share -- paths.hip (tables, lists, host drivers), paths_fused.hip (the headline
// kernel), paths_overflow.hip (a batch whose path list does not fit its buffer): the launch arguments and the two launchers.
#pragma once
#include "lgnn_internal.h"

namespace lgnn {

constexpr int kYRows = 48;  // classes per launch of paths_fused_kernel: three 16-class MFMA tiles
// Where class c of a call's class range [cb, cb + 64) sits inside the 64 slots of one coefficient kind: the four 16-class MFMA
// tiles of a slot i side by side, so that a product-wave lane fetches its A operands of all tiles with one 16-byte load.
__device__ __forceinline__ int coef_slot(int rel) { return ((rel & 15) << 2) | (rel >> 4); }
__device__ __forceinline__ int slot_class(int slot) { return ((slot & 3) << 4) | (slot >> 2); }
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct YArgs {
  const int32_t* rowptr; const int32_t* col; const float* val;  // P^T
  const int32_t* rptr; const int32_t* r_m; const float* r_w;    // R = P^T[:, batch]
  const int32_t* pptr; const int32_t* pm; const int32_t* pv; const float* pw;  // the paths per node (when they fit `cap`)
  int64_t cap;
  const float* coef;        // [M][256]: (alpha | -beta | -gamma | 0) x 64 classes
  const float* zeros;       // >= 1 KiB of zeros
  const float* bg;          // [2 M][H]: rows b_m, then rows g_m
  const uint32_t* mask;     // [N][mask_words] ReLU bits of h_1
  int mask_words;
  const float* W1;          // [C][w1_ld]: the H columns Y is multiplied with (GraphSAGE: the neighbour half of W_1)
  int w1_ld;
  float* Y;                 // [N][R][H]
  int64_t N, M;             // all nodes (pptr has N + 1 entries); rows of a table half
  int64_t n0, n1;           // the destination nodes this launch visits: [n0, n1)
  const int32_t* list;      // optional: the nodes of that range that have a path (relative to n0), ...
  const int32_t* n_list;    // ... and how many (device side: no host round trip); null: every node of the range
  int H, c0, R;
  int cb;                   // first class of the coefficient table's slots (the call's class range starts there)
  int64_t n_coef;           // rows of the coefficient table
  int unused_;              // (keeps the fields below at their kernel-argument offsets: hipcc merges the argument loads
                            //  by offset, and shifted by 4 bytes paths_fused_kernel spills more SGPRs)
  int no_bg;                // regression / nothing but the diagonal term: the beta / gamma products vanish
  int gram_f32;             // LGNN_GRAM_F32: paths_fused_kernel's Gram on fp32 MFMAs instead of the fp16 pieces
  const float* scale;       // paths_fused_kernel: the launch's PathScale block (below); W1 and bg are its normalised copies then
};
// (the kernels take YArgs by value and hipcc merges the argument loads by offset, see unused_: the layout is part of the kernels)
static_assert(sizeof(YArgs) == 248 && __builtin_offsetof(YArgs, no_bg) == 228, "YArgs: paths_fused_kernel's argument offsets");

// What the fp16 Gram of paths_fused_kernel needs to know about the size of the tile values (floats; paths.hip fills it per
// accumulate, on the stream).  Every term of Y[n][c, j] is linear in column j of W_1 (paths.hip's header), so column j is
// NORMALISED by the power of two cn_j = 2^-floor(log2 max_c |W_1[c, j]|): the fused kernel reads W1n = W_1 diag(cn) and
// bgn = bg diag(cn), builds Y diag(cn) with not one instruction more, and multiplies its Gram by 1 / (cn_i cn_j) at the flush.
// All of it is exact (powers of two).  What is left is ONE bound per launch, from TWO triangle inequalities over a node's
// paths (a mask bit is 0 or 1), one over a path's three terms, one over the rows k of the sample's seed block
// V[k, c] = alpha_c d_kc - beta_c u_k - gamma_c p_k, of which a path's vector is V[:, c]^T W_1:
//     |Y[n][c, j]| cn_j <= wsum * min(tri, vmax * w1max),     tri = amax * w1max + bgmax,
//   wsum  = max_n sum_paths |w|                  (where the path list is built: the float behind pptr[N], see path_list_reserve)
//   amax  = max_m max_c |alpha_c^m|,   w1max = max |W_1 diag(cn)| (< 2; GraphSAGE: both halves of W_1),
//   bgmax = max_m (max_c |beta_c^m| max_j |bgn_b[m, j]| + max_c |gamma_c^m| max_j |bgn_g[m, j]|),
//   vmax  = max_m max_c sum_k |V_m[k, c]|        (the tables kernels, per sample).
// The second sees what the first cannot: where the softmax is sure of its class the three terms cancel (V is zero for a
// one-hot p) and a tile value is rounding noise far below `tri`.  The fused kernel's fp32 sums carry that noise whatever the
// exact value is, so the bound it scales by is  wsum * (min(tri, vmax * w1max) + 2^-12 tri):  2^-12 covers 4 096 terms of
// 2^-24 relative error each, all of one sign.  The maxima are taken on the bit patterns of |x| (unsigned order = numeric
// order, and a NaN is above everything): a non-finite operand gives a non-finite bound, and such a launch runs the fp32 role.
constexpr int kScaleCn = 4, kScaleCinv = kScaleCn + 256, kScaleW1 = kScaleCinv + 256;  // offsets: cn [256], 1 / cn [256], W1n [C][H]
// ([0] amax, [1] w1max, [2] bgmax, [3] vmax as bit patterns)

// R, the path list and the node list of a batch as the launches below read them: the workspace's or a cache entry's
struct PathLists {
  const int32_t* rptr; const int32_t* r_m; const float* r_w;
  const int32_t* pptr; const int32_t* pm; const int32_t* pv; const float* pw;
  const int32_t* nodes; const int32_t* nnodes;
};

// scratch += B_0 of the classes [cb, ce) over the nodes [y.n0, y.n1), kYRows classes per launch (sets y.c0, y.R, y.gram_f32);
// on the device a launch returns at once if the path list overflowed y.cap (paths_fused.hip) ...
int launch_paths_fused(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s);
// ... and this one unless it did: the same sum through class planes in ws.planes_a and the streaming Gram (paths_overflow.hip)
int launch_paths_overflow(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s);

}  // namespace lgnn
