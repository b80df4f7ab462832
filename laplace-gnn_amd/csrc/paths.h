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
  int piece_share_log2;     // K of the piece products' rule (PathScale; path_role_kernel alone reads it).  (The field also keeps
                            //  those below at their kernel-argument offsets: hipcc merges the argument loads by offset, and
                            //  shifted by 4 bytes paths_fused_kernel spills more SGPRs)
  int no_bg;                // regression / nothing but the diagonal term: the beta / gamma products vanish
  int gram_f32;             // LGNN_GRAM_F32: paths_fused_kernel's Gram on fp32 MFMAs instead of the fp16 pieces
  const float* scale;       // paths_fused_kernel: the launch's PathScale block (below); W1 and bg are its normalised copies then
};
// (the kernels take YArgs by value and hipcc merges the argument loads by offset, see piece_share_log2: the layout is part of the kernels)
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
constexpr int kScaleCn = 8, kScaleCinv = kScaleCn + 256, kScaleW1 = kScaleCinv + 256;  // offsets: cn [256], 1 / cn [256], W1n [C][H]
// ([0] amax, [1] w1max, [2] bgmax, [3] vmax as bit patterns; [4] wsum and [5] the role the launch ran, kRole*, written by
// path_role_kernel for lgnn_last_paths_product_role: nothing on the device reads those two)
constexpr int kScaleWsum = 4, kScaleRole = 5;
// everything on fp32 MFMAs; the Gram on fp16 pieces and the beta / gamma products on fp32; those products on fp16 pieces too
constexpr int kRoleF32 = 0, kRoleGramF16 = 1, kRoleProductsF16 = 2;
// The beta / gamma products run on fp16 pieces where  min(tri, vmax * w1max) >= 2^-K tri  (below); K per model family, since
// GraphSAGE's `tri` carries the self half of W_1 as table rows and its ratio lies lower at the same cancellation.
constexpr int kPieceShareLog2Gcn = 1, kPieceShareLog2Sage = 3;
// -1 in the role word: the call's path list overflowed its buffer and the fused kernel did not run
constexpr int kRoleNone = -1;
// THE PIECE PRODUCTS.  A path's beta term is a_c (mask (.) b_m)[j], a_c = w s (-beta_c^m) (s: the launch's power of two, on the
// path weight), the gamma term likewise.  fp16 has 5 exponent bits, so both sides are normalised, exactly: table row m by the
// power of two 2^k_m that puts max_j |bgn[m, j]| in [2^6, 2^7) (kPieceRowLog2), the sample's beta coefficients by 2^-k_m (the
// g row and the gamma coefficients by a power of their own) -- the product is what it was.  Then
//     |a'| = |w| s |beta_c^m| 2^-k_m <= s wsum |beta_c^m| max_j |bgn[m, j]| / 2^6 <= s wsum tri / 2^6,
// and s * bound < 2^15 with bound >= wsum min(tri, vmax w1max) >= wsum 2^-K tri under the rule: |a'| < 2^(9 + K), 2^12 at the
// most, a sixteenth of fp16's range (it is the product of the two maxima that is bounded, not bgmax alone).  A row of zeros
// takes zero coefficients, so no large a' ever meets it.  Each operand is two fp16 pieces rounded to nearest (x0 = fp16(x),
// x1 = fp16(x - x0): 22 bits while x1 is a normal number, i.e. for |x| >= 2^-3, and 2^-25 absolutely below), all four piece
// products are kept, each is exact in fp32: a term carries about 2^-21 relative error where the fp32 MFMA carries 2^-24,
// hence the wider rounding share of the bound for this role (2^-9 tri: 4 096 terms of 2^-21).  WHY 2^6 AND NOT 2^13 for the
// rows: a' is small against its bound (the bound takes every maximum at once); with rows at 2^13 the largest a' of the test
// shapes is 0.02 .. 0.05, its second piece a subnormal, and B_0 came out five times further from fp64 than on fp32 MFMAs
// (measured, GraphSAGE 6e-7 against 1e-7); at 2^6 the largest a' is 2 .. 60 and the distance to fp64 is the fp32 role's.
// THE RULE.  The pieces run only where cancellation between a path's terms is moderate, min(tri, vmax w1max) >= 2^-K tri:
// where the seed block vanishes a tile value is rounding noise of terms of size `tri`, and 2^-21 of them is eight times the
// noise of the fp32 products.  K is what a sweep gives per family (tests/test_gpu_path_products_f16.py: W_1, b_1 x 2^k, k = 0
// .. 20, both splits restated in numpy; the largest ratio at which the restated B_0 leaves a quarter of the suite's two
// bounds is 0.28 for the GCN, so 2^-1, and 0.10 for GraphSAGE, so 2^-3).
constexpr int kPieceRowLog2 = 6;
// What path_bound_kernel leaves in ws.path_bgn for a table of `rows` samples (float offsets): the normalised fp32 table
// [2 rows][H], the PIECE table [2 rows][H] of packed dwords, the coefficient rows [rows][kCoefRow] that go with the pieces.
__host__ __device__ __forceinline__ int64_t piece_table_offset(int64_t rows, int64_t H) { return 2 * rows * H; }
__host__ __device__ __forceinline__ int64_t piece_coef_offset(int64_t rows, int64_t H) { return 4 * rows * H; }

// R, the path list and the node list of a batch as the launches below read them: the workspace's or a cache entry's
struct PathLists {
  const int32_t* rptr; const int32_t* r_m; const float* r_w;
  const int32_t* pptr; const int32_t* pm; const int32_t* pv; const float* pw;
  const int32_t* nodes; const int32_t* nnodes;
};

// scratch += B_0 of the classes [cb, ce) over the nodes [y.n0, y.n1), kYRows classes per launch (sets y.c0, y.R, y.gram_f32);
// on the device a launch returns at once if the path list overflowed y.cap (paths_fused.hip) ...
int launch_paths_fused(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s);
// whether a call of launch_paths_fused may run the piece instance at all (not under LGNN_GRAM_F32; read per call)
bool fused_pieces_possible();
// ... and this one unless it did: the same sum through class planes in ws.planes_a and the streaming Gram (paths_overflow.hip)
int launch_paths_overflow(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s);

}  // namespace lgnn
