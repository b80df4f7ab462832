// paths_fused_kernel and its launcher: B_0 of a 2-layer GCN / GraphSAGE from a batch's path list (paths.hip builds the list and
// states the algebra).
// The route (round 4): everything of a node on one CU, ONE persistent 512-thread workgroup per CU whose eight waves
// have two ROLES.  The hardware deals a workgroup's waves round-robin to the CU's four SIMDs, so hardware waves g and g + 4
// share a SIMD -- and its one matrix pipe:
//   waves 0 .. 3, the PRODUCT waves (one per SIMD): wave cg owns the columns [64 cg, 64 cg + 64) of Y[n] for all <= 48
//       classes of the launch.  Per step of FOUR paths: three 16-byte loads of the paths' coefficient rows (A operands: lane
//       (i, k) = class slot i of path k, the four class tiles of a slot side by side in the table row), two 16-byte loads of
//       the table rows b_m, g_m (B operands: lane (i, k) = columns 64 cg + 4 i .. + 3 of path k -- the four 16-column MFMA
//       tiles of the wave interleave the columns, so one load feeds all four), one mask word; for the beta / gamma products
//       12 v_mfma_f32_16x16x32_f16 per step (3 class tiles x 4 column tiles, both terms and all four products of two fp16
//       pieces per operand along K: 192 cycles, see PCurH) in the instance most launches run, 24 v_mfma_f32_16x16x4_f32
//       (768 cycles) in the other (a launch whose terms cancel too far for pieces, the regression likelihood, LGNN_GRAM_F32:
//       path_role_kernel); and, per PAIR of steps, 12
//       v_mfma_f32_16x16x32_bf16 for the alpha product of both (192 cycles, exact: the mask is 0 / 1 and the weighted
//       coefficient goes in as three bf16 pieces along K, see PAlpha).  No LDS staging, no window, no restaging of hubs: the
//       operands of step s + 1 are in flight while the MFMAs of step s issue, across node boundaries (a node's triples
//       (m, v, w) arrive with ONE coalesced load a node ahead and are handed to the lanes with ds_bpermute).
//       Y[n] = W_1 (.) T1 + Y2 (W_1's rows straight from L2) comes out SCALED -- its columns by the powers of two that W_1 and
//       the b / g table carry (PathScale in paths.h), all of it by the launch's s, which rides on the path weights (GramScale)
//       -- and is split into two fp16 pieces HERE, once per value; the pieces go to one of TWO LDS tiles (FusedShared; 18
//       16-byte stores per node: h1 goes out twice) -- under LGNN_GRAM_F32, or without a usable scale, the fp32 values.
//   waves 4 .. 7, the GRAM waves: S += Y[n - 1]^T Y[n - 1] from the other tile into register-resident upper-triangular
//       accumulators (the 36 sub-tiles of gram256.h, 9 per wave, as 34 tiles of 16 x 16: 136 accumulator registers), nothing
//       else: their loop is LDS reads and MFMAs -- v_mfma_f32_16x16x32_f16 on the pieces, 16 cycles each and two per 16 tile
//       rows, so that a product wave's MFMA waits 16 cycles for this wave's turn on the pipe, not 32 (gram_f16_role).
// ONE hand-off per node (LDS counters).  The product wave of a SIMD needs the matrix pipe for about a third of a node's cycles
// and sleeps on memory part of the rest; the Gram wave is a dense MFMA stream that takes every slot the product wave leaves: the
// two phases that round 3 ran back to back in every wave (7.7 ms per arxiv batch, matrix pipes 57 % busy) now overlap.
#include "gram256.h"
#include "paths.h"

namespace lgnn {
namespace {

constexpr int kYStride = 272;  // floats per row of the fp32 tile: 256 + 16, so that the four rows of a Gram operand read (lanes
                               // 16 k .. 16 k + 15 read row k0 + k) fall on disjoint banks
// The tile as fp16 PIECES (the default Gram role): a scaled tile value y is h0 + h1, h0 = fp16(y), h1 = fp16(y - h0) (see
// gram_f16_role).  A dword holds the same piece of two tile rows (row r in the low half, r + 1 in the high
// half); the tile rows come in GROUPS of four, g = row / 4, i.e. (chunk of 16 rows, lane group of the Gram's MFMA operand), and a
// group is three PLANES (h1, h0, h1 again) of 256 columns x 2 dwords (rows 4 g, 4 g + 1 | rows 4 g + 2, 4 g + 3): 2 KiB each.
// A Gram lane reads the 8 bytes of its column from each plane (ds_read_b64; 16 lanes: 128 contiguous bytes) and so holds
// (h1, h0, h1), both operand forms of gram_f16_role, with three plain reads; a product lane writes the 32 bytes of its four columns to each plane (two ds_write_b128).  The 8 lanes one ds_write_b128 cycle serves are 32 bytes
// apart, which would put them on 16 of the 32 banks twice: the two 16-byte halves of a lane's 32 bytes swap places in the lanes
// piece_swap() names, and the 8 lanes cover the 32 banks once.  A lane group's reads stay a permutation of 128 contiguous bytes
// (two lane groups share an LDS cycle and the same banks there: see gram_f16_role).
// WHY h1 IS STORED TWICE (144 KiB as with three bf16 planes, where two planes would take 96): the second copy costs the
// product wave six LDS stores per node and no vector instruction; the other ways to the second operand form all cost the
// Gram wave.  Tried with two planes: reading plane h1 twice -- hipcc merges the two reads and copies registers (two v_mov
// per block and chunk: vector-ALU time, which on this chip is matrix-pipe time); the second read made volatile -- hipcc
// then gathers every read of a chunk at the loop's end and waits for them in the open (measured: a fit 3 ms SLOWER than
// on bf16 pieces); a six-register vector per block -- 1 138 registers spilled.  The spare 16 KiB of the CU's LDS have no
// use here (one workgroup per CU either way; the fp32 tiles of the fallback take 102 KiB).
constexpr int kPlaneDwords = 512;             // one plane: 256 columns x 2 dwords
constexpr int kGroupDwords = 3 * kPlaneDwords;
constexpr int kYGroups = kYRows / 4;
// whether the four-column group q (columns 4 q .. 4 q + 3) stores its column pairs in swapped order
__device__ __forceinline__ int piece_swap(int q) { return (q ^ (q >> 2)) & 1; }
// dword offset inside a plane of column c's two dwords
__device__ __forceinline__ int piece_col(int c) { return 8 * (c >> 2) + 4 * (((c >> 1) & 1) ^ piece_swap(c >> 2)) + 2 * (c & 1); }

struct alignas(16) FusedShared {
  union {  // the node tiles (double buffered), in the form the launch's Gram role reads
    uint32_t pc[2][kYGroups][3][kPlaneDwords];  // fp16 pieces: 2 x 72 KiB
    float y[2][kYRows][kYStride];               // fp32 (LGNN_GRAM_F32, or a launch without a usable scale): 2 x 51 KiB
  };
  // hand-off counters (one writer each): ready[p] = nodes whose tile columns product wave p has published, done[g] = nodes
  // Gram wave g has contracted
  int ready[4], done[4];
};
static_assert(sizeof(FusedShared) <= 160 * 1024, "the CU's LDS");

// min over the four counters of a hand-off array (one 16-byte LDS read; wave uniform)
__device__ __forceinline__ int lds_min4(const int* c) {
  int4 v;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(uint32_t(reinterpret_cast<uintptr_t>(c))) : "memory");
  return __builtin_amdgcn_readfirstlane(min(min(v.x, v.y), min(v.z, v.w)));
}
// publish a counter: one ds_write_b32 on the 32-bit LDS address (a store through the generic pointer is a system-scope
// flat_store into the LDS aperture followed by vmcnt(0): a memory round trip per node on the product wave's chain).  A wave's
// LDS operations execute in order, so the counter lands after the wave's earlier tile stores / tile reads; the lgkmcnt(0)
// behind it keeps hipcc's own lgkmcnt(N) counts right (it does not see this operation).
__device__ __forceinline__ void lds_publish(int* c, int value, int lane) {
  if (lane == 0)
    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" :: "v"(uint32_t(reinterpret_cast<uintptr_t>(c))), "v"(value) : "memory");
}

// Path ranges [p0, p1) of this workgroup's nodes (node i = entry blockIdx.x + i * gridDim.x of the list of nodes with paths,
// or of the whole range), 32 nodes at a time in ONE register (the product role has none to spare): lanes l and 32 + l hold
// the range of node base + l, a node's range is two v_readlane with a wave-uniform index.  Every 32 nodes the wave loads the
// next window through buffer descriptors (the list entry first, then pptr[n] / pptr[n + 1]: one buffer_load_dword) and waits
// for it right there with vmcnt(0): one memory round trip per 32 nodes.  (A scalar load per node -- the index is strided, so
// every node is a new line -- put a scalar-cache miss on the wave's chain once per node: the values rotate into loop-carried
// registers, so hipcc waits lgkmcnt(0) where the load is issued.)  Inline assembly as below: the product role counts its
// vector loads by hand, and this block leaves none outstanding.  A lane past `cnt` reads outside the descriptor: zeros, the
// empty range.  Nodes are asked for in ascending order.
// Kept for what it does to the ISA (no scalar load, no lgkmcnt(0) behind one in the node loop), NOT for speed: measured
// alone, neither this window nor the LDS-store publish above moves the launch time beyond the run-to-run spread (DESIGN
// 12.15), and the kernel spills 12 / 24 more SGPRs to VGPR lanes with them.
using i32x4 = int __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_rsrc(const void* p, uint64_t bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  return i32x4{int(uint32_t(u)), int(uint32_t(u >> 32) & 0xffffu), int(uint32_t(bytes > 0xffffffffull ? 0xffffffffull : bytes)),
               0x00020000};
}
template <bool LIST>
struct NodeRanges {
  i32x4 prs, lrs;    // pptr (N + 1 entries), the node list (nn entries)
  uint32_t r;        // lane l < 32: pptr[n] of node base + l, lane 32 + l: its pptr[n + 1]
  int64_t base, cnt;
  uint32_t n0;
  __device__ __forceinline__ void init(const int32_t* __restrict__ pptr, const int32_t* __restrict__ list, int64_t n0_, int64_t N,
                                       int64_t nn, int64_t cnt_) {
    prs = make_rsrc(pptr, uint64_t(N + 1) * 4);
    lrs = make_rsrc(LIST ? list : pptr, uint64_t(LIST ? nn : 0) * 4);
    n0 = uint32_t(n0_); cnt = cnt_;
    fill(0);
  }
  __device__ __forceinline__ void fill(int64_t b) {
    base = b;
    // (an opaque copy of the thread number: as a loop invariant the lane's index would live -- in the product role: in
    // scratch memory -- from one window to the next, 32 nodes on, for the sake of one v_and)
    uint32_t tx = threadIdx.x;
    asm volatile("" : "+v"(tx));
    const uint32_t ii = uint32_t(b) + (tx & 31u);
    const bool in = int64_t(ii) < cnt;
    const uint32_t k = blockIdx.x + ii * gridDim.x;
    uint32_t node = k;
    if constexpr (LIST)
      asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, 0 offen\n\ts_waitcnt vmcnt(0)" : "=&v"(node) : "v"(in ? k * 4u : 0xfffffff0u), "s"(lrs) : "memory");
    const uint32_t off = in ? (n0 + node) * 4u + ((tx >> 3) & 4u) : 0xfffffff0u;
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, 0 offen\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(off), "s"(prs) : "memory");
  }
  __device__ __forceinline__ void get(int64_t i, int32_t& p0, int32_t& p1) {
    if (i - base >= 32) fill(i);
    const int l = int(i - base);
    p0 = __builtin_amdgcn_readlane(int(r), l); p1 = __builtin_amdgcn_readlane(int(r), l + 32);
  }
};

// ---- loads of the product waves: inline assembly with hand-placed wait counts.  hipcc's own counts are exact only along one
// path; at the loop headers of this kernel it merges the paths pessimistically (measured: the wait for a step's operands also
// waited for half of the NEXT step's, i.e. one step of prefetch distance instead of two), and any load it tracks itself would
// make it wait for vmcnt(0) -- it does not see the assembly loads queued behind.  So every vector load of the role's loop is
// issued here and waited for with a counted s_waitcnt whose "+v" operands tie the loaded registers to the wait (uses cannot
// move above it).  vmcnt counts in order: waiting until at most n operations are outstanding retires everything older than
// the n youngest.
// BUFFER loads (descriptor in SGPRs + one 32-bit byte offset per lane): on this chip the fp32 MFMAs run on the SIMD's vector
// ALUs, so every VALU instruction of either wave of a SIMD is matrix-pipe time lost, not work hidden behind the MFMAs
// (measured: the product wave's MFMA time and the time of its other instructions add up, with or without the Gram wave) --
// 64-bit address arithmetic per load was a quarter of this wave's instructions.  An offset past the table's end reads zeros.
// PAD: five wait states in front of the load, inside the same statement.  A descriptor that hipcc has spilled to a VGPR lane
// comes back with v_readlane right in front of the statement that uses it, and a vector-memory instruction that reads an SGPR
// fewer than five wait states after a vector-ALU instruction wrote it reads the OLD value; hipcc pads its own loads and
// does not look into an assembly statement.  (Measured: with the coefficient table's descriptor reloaded one instruction in
// front of a step's first load, the no-list instance's B_0 was 0.57 off the oracle at C = 7.)  The FIRST load of every group
// below is padded -- the reloads of a group's descriptors stand in front of it -- not each one: 5 cycles per step, not 30.
template <int OFF, bool PAD = false>
__device__ __forceinline__ void bload4(f32x4& d, uint32_t voff, const i32x4& rsrc) {
  if constexpr (PAD)
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(d) : "v"(voff), "s"(rsrc), "n"(OFF) : "memory");
  else
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(d) : "v"(voff), "s"(rsrc), "n"(OFF) : "memory");
}
template <bool PAD = false>
__device__ __forceinline__ void bload1(uint32_t& d, uint32_t voff, const i32x4& rsrc) {
  if constexpr (PAD) asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, 0 offen" : "=v"(d) : "v"(voff), "s"(rsrc) : "memory");
  else asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(d) : "v"(voff), "s"(rsrc) : "memory");
}
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4v = __attribute__((ext_vector_type(4))) uint32_t;
using u32x2v = __attribute__((ext_vector_type(2))) uint32_t;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
// The two fp16 pieces of two scaled tile values (ya in the low halves, yb in the high halves), each rounded to nearest:
// h0 = fp16(y), h1 = fp16(y - h0) (see gram_f16_role; the difference is exact).  3 vector instructions.
__device__ __forceinline__ void split_pair(float ya, float yb, uint32_t& h0, uint32_t& h1) {
  // (the conversion in assembly as well: left to itself hipcc fuses it into the FMA that made y (v_fma_mix), computes every
  // value twice and keeps W_1's rows, T1 and Y2 alive beside the results -- 95 registers spilled; the pieces are those of the
  // ROUNDED fp32 value, the one the fp32 tile holds)
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h0) : "v"(ya), "v"(yb));
  // y - h0 with the fp16 piece as an operand of a mixed-precision FMA: widens the piece, subtracts -- exactly -- and rounds
  // to fp16 (the mode's round to nearest, subnormals kept) in ONE instruction per value.  hipcc does not find the form itself
  // (it converts, subtracts and packs: three more instructions per pair, on the wave that paces the kernel).
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(h1) : "v"(h0), "v"(ya));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(h1) : "v"(h0), "v"(yb));
}

struct PTables {  // descriptors of what the role reads
  i32x4 coef, b, g, mask, pm, pv, pw;
};

// The paths of a chunk (up to 64): lane l holds path p0 + l as the BYTE OFFSETS of its sample's rows in the coefficient table
// (oc) and the b / g tables (ob), of its middle node's mask words (om), and its weight.  Unconditional loads from a clamped
// index; lanes past the range get offsets 0 and weight 0 in meta_finish: every load formed from them is valid, every product
// with them is zero.
struct PMeta { uint32_t oc, ob, om, w; };  // (w: the bits of a float)
__device__ __forceinline__ void meta_issue(const PTables& tb, int32_t p0, int32_t p1, int lane, PMeta& t) {
  const uint32_t q = uint32_t(max(min(p0 + lane, p1 - 1), 0)) * 4u;
  bload1<true>(t.oc, q, tb.pm);  // (sample m, node v: turned into offsets in meta_finish)
  bload1(t.om, q, tb.pv);
  bload1(t.w, q, tb.pw);
}
// `scale`: the launch's power of two s (GramScale): the weight goes on as w s, so every tile value comes out as s y -- exactly,
// and at one multiply per chunk and lane.
template <int YOUNGER>  // vector-memory operations issued after the triples' loads that may still be in flight
__device__ __forceinline__ void meta_finish(int32_t p0, int32_t p1, int lane, uint32_t row_bytes, uint32_t mask_bytes, float scale,
                                            PMeta& t) {
  asm volatile("s_waitcnt vmcnt(%3)" : "+v"(t.oc), "+v"(t.om), "+v"(t.w) : "n"(YOUNGER) : "memory");
  const bool in = p0 + lane < p1;
  const uint32_t m = in ? t.oc : 0u, v = in ? t.om : 0u;
  t.oc = m * uint32_t(kCoefRow * 4); t.ob = m * row_bytes; t.om = v * mask_bytes;
  t.w = in ? __float_as_uint(__uint_as_float(t.w) * scale) : 0u;
}

struct PLane {        // what a product-wave lane is: class slot / column slot i, path k of a step
  int kq;
  uint32_t oc, ob, om;  // the lane's byte offsets inside a coefficient row (16 i), a table row (4 (64 cg + 4 i)) and a node's
                        // mask words; past H: the row's start resp. an offset outside the mask (reads zero: no bit set)
  int mshift;           // bit of the lane's first column inside its mask word
};

struct POps {        // the loaded operands of one step (22 registers)
  f32x4 ca[3];      // coefficient rows (alpha | -beta | -gamma), class slots (i, t = 0 .. 3)
  f32x4 b4, g4;     // rows b_m, g_m at the lane's four columns
  uint32_t mw;       // mask word of the path's middle node
  float w;           // path weight (0 past the chunk's last path)
};

// Issue the loads of step s (paths 4 s .. 4 s + 3 of the chunk `mt`): kStepLoads<NOBG> instructions, nothing conditional.
template <bool NOBG> constexpr int kStepLoads = NOBG ? 2 : 6;
template <bool NOBG>
__device__ __forceinline__ void p_load(const PTables& tb, const PMeta& mt, int s, const PLane& pl, POps& o) {
  const int src = 4 * s + pl.kq;  // the lane that holds this lane's path (s < 16)
  const uint32_t oc = uint32_t(__shfl(int(mt.oc), src)) + pl.oc;
  const uint32_t om = uint32_t(__shfl(int(mt.om), src)) + pl.om;
  o.w = __uint_as_float(uint32_t(__shfl(int(mt.w), src)));
  bload4<0, true>(o.ca[0], oc, tb.coef);
  if constexpr (!NOBG) {
    const uint32_t ob = uint32_t(__shfl(int(mt.ob), src)) + pl.ob;
    bload4<kCoefStride * 4>(o.ca[1], oc, tb.coef);
    bload4<2 * kCoefStride * 4>(o.ca[2], oc, tb.coef);
    bload4<0>(o.b4, ob, tb.b);
    bload4<0>(o.g4, ob, tb.g);
  }
  bload1(o.mw, om, tb.mask);
}
// the step's loads have landed once at most YOUNGER younger vector-memory operations are outstanding
template <bool NOBG, int YOUNGER>
__device__ __forceinline__ void p_wait(POps& o) {
  if constexpr (NOBG)
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(o.ca[0]), "+v"(o.mw) : "n"(YOUNGER) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%6)" : "+v"(o.ca[0]), "+v"(o.ca[1]), "+v"(o.ca[2]), "+v"(o.b4), "+v"(o.g4), "+v"(o.mw)
                 : "n"(YOUNGER) : "memory");
}

// A step's beta / gamma MFMA operands: lane (i, k): A[row i][k] = weighted coefficient of class 16 t + i, B[k][col i] = masked
// table value of the lane's column ct.
struct PCur { float a1[3], a2[3], bb[4], gg[4]; };
// The same operands for v_mfma_f32_16x16x32_f16 (the launches path_role() gives the fp16 products, see PathScale in paths.h):
// both sides as two fp16 pieces, x = x0 + x1 with x0 = fp16(x), x1 = fp16(x - x0) as in split_pair, and ALL FOUR piece
// products along K.  The instruction's lane (i, q) owns the K slots 8 q .. 8 q + 7, and lane group q is path q of the step, so
// a lane's eight slots are its own path's
//   A operand of class tile t:    a0 a0 | a1 a1 | c0 c0 | c1 c1    (a = w s (-beta') of class 16 t + i, c = w s (-gamma'))
//   B operand of column tile ct:  b0 b1 | b0 b1 | g0 g1 | g0 g1    (the masked dwords of the PIECE table, each one twice)
// and ONE MFMA per (class tile, column tile) is the step's four paths, both terms: 12 of 16 cycles where the fp32 form takes
// 24 of 32.  The table's rows come normalised by a power of two per row and the coefficients by its inverse (path_bound_kernel,
// PathScale): the primes.  The B side's pieces are made once per table row there; a lane's b4 / g4 are the same two 16-byte
// loads, of packed dwords (b0 | b1 << 16).  ONE operand set (28 registers, what the two fp32 sets take together).
struct PCurH { u32x4v a[3], b[4]; };
// a as (a0 | a0 << 16) and (a1 | a1 << 16): 3 vector instructions (in assembly for split_pair's reasons)
__device__ __forceinline__ void split_twice(float a, uint32_t& h0, uint32_t& h1) {
  asm("v_cvt_pk_f16_f32 %0, %1, %1" : "=v"(h0) : "v"(a));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(h1) : "v"(h0), "v"(a));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "+v"(h1) : "v"(h0), "v"(a));
}
// a step's beta / gamma operands from its landed loads (`bits`: the lane's mask bits from bit 0 on): 6 + 8 vector instructions
// in the fp32 form, 24 + 16 as pieces
template <bool HI>
__device__ __forceinline__ void p_bg(const POps& o, int bits, PCur& c) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int tt = HI ? 3 : t;
    c.a1[t] = (HI && t > 0) ? 0.f : o.w * o.ca[1][tt];
    c.a2[t] = (HI && t > 0) ? 0.f : o.w * o.ca[2][tt];
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int on = __builtin_amdgcn_sbfe(bits, ct, 1);
    c.bb[ct] = __uint_as_float(uint32_t(on) & __float_as_uint(o.b4[ct]));
    c.gg[ct] = __uint_as_float(uint32_t(on) & __float_as_uint(o.g4[ct]));
  }
}
template <bool HI>
__device__ __forceinline__ void p_bg(const POps& o, int bits, PCurH& c) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (HI && t > 0) { c.a[t] = u32x4v{0u, 0u, 0u, 0u}; continue; }
    const int tt = HI ? 3 : t;
    uint32_t h[4];
    split_twice(o.w * o.ca[1][tt], h[0], h[1]);
    split_twice(o.w * o.ca[2][tt], h[2], h[3]);
    c.a[t] = u32x4v{h[0], h[1], h[2], h[3]};
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const uint32_t on = uint32_t(__builtin_amdgcn_sbfe(bits, ct, 1));
    const uint32_t b = on & __float_as_uint(o.b4[ct]), g = on & __float_as_uint(o.g4[ct]);
    c.b[ct] = u32x4v{b, b, g, g};
  }
}
// The alpha product T1 += (w alpha) Mk of a PAIR of steps as v_mfma_f32_16x16x32_bf16, exactly.  Mk is 0 or 1 and a bf16 as it
// is; a = w alpha is cut into three bf16 pieces by TRUNCATION,
//   r1 = a - (a & 0xffff0000), r2 = r1 - (r1 & 0xffff0000), pieces = the high halves of a, r1, r2:
// a's high half keeps 8 significant bits, so r1 has at most 16 and r2 at most 8: both differences are exact, r2's low half
// is zero, and the three pieces sum to a.  (Only a piece below fp32's normal range, |r2| < 1.2e-38, is not safe: the bf16 MFMA
// may flush it, an error below 1e-38 per term.)  Every piece meets 0 or 1, so the products are exact and no cross term exists.
// The instruction's lane (i, q) holds A[row i][k = 8 q + j] and B[k = 8 q + j][col i], j = 0 .. 7, in four registers: lane
// group q is path q of the pair's step A and path q of its step B, and its eight K slots are its own registers,
//   A operand of class tile t:   a a1 | a2 b | b1 b2 | 0 0     (pieces of step A's path, of step B's path, two empty slots)
//   B operand of column tile ct: mA mA | mA mB | mB mB | 0 0   (bf16 1.0 where the step's path has the column's mask bit)
// with D laid out as the fp32 16x16x4's (col i, rows 4 q + r).  Step A's transform writes its slots (and zero into the high
// half of the shared register), step B's adds its own.  In a `half` pair step B's slots are written all the same, from B's
// landed operands: its paths lie past the chunk's last one and have weight zero (meta_finish), so its slots of the A operand
// are zero whatever its mask bits are.
struct PAlpha { u32x4v a[3], m[4]; };
constexpr uint32_t kHiHalves = 0x07060302u;  // v_perm_b32(x, y): y's high half below x's high half
// One step's MFMA operands.  SB: the pair's second step.  HI (a second launch of a call with more than 48 classes): the
// launch's only class tile is the fourth of the slot.  `bg`: also the beta / gamma operands (not in a `half` pair's second
// step).  About 48 vector instructions (each costs the SIMD's matrix pipe its issue cycles, see above): 7 per class tile for
// the alpha pieces (multiply, two ANDs, two subtractions, two to pack), 13 for the mask -- bit ct of the mask word as 0 / -1
// with one v_bfe_i32, ANDed with the bf16 ones of its slots --, 6 + 8 for beta / gamma.
template <bool NOBG, bool HI, bool SB, class CUR>
__device__ __forceinline__ void p_xform(const POps& o, const PLane& pl, CUR& c, PAlpha& al, bool bg) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int tt = HI ? 3 : t;
    if (HI && t > 0) {
      if constexpr (!SB) al.a[t][0] = 0u;
      al.a[t][1] = 0u; al.a[t][2] = 0u;
      continue;
    }
    // (the empty statement keeps hipcc from contracting the multiply into the subtraction: the pieces are those of the
    // ROUNDED product, and r1 has 16 significant bits only as the difference of two fp32 numbers)
    float av = o.w * o.ca[0][tt];
    asm("" : "+v"(av));
    const uint32_t h0 = __float_as_uint(av) & 0xffff0000u;
    const float r1 = av - __uint_as_float(h0);
    const float r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    if constexpr (!SB) {
      al.a[t][0] = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(av), kHiHalves);
      al.a[t][1] = __float_as_uint(r2) >> 16;
    } else {
      al.a[t][1] |= h0;
      al.a[t][2] = __builtin_amdgcn_perm(__float_as_uint(r2), __float_as_uint(r1), kHiHalves);
    }
  }
  const int bits = int(o.mw >> pl.mshift);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int on = __builtin_amdgcn_sbfe(bits, ct, 1);  // 0 or -1
    if constexpr (!SB) {
      al.m[ct][0] = uint32_t(on) & 0x3f803f80u;
      al.m[ct][1] = uint32_t(on) & 0x00003f80u;
    } else {
      al.m[ct][1] |= uint32_t(on) & 0x3f800000u;
      al.m[ct][2] = uint32_t(on) & 0x3f803f80u;
    }
  }
  if constexpr (!NOBG) {
    if (bg) p_bg<HI>(o, bits, c);  // (wave uniform)
  }
}
// an empty statement that reads every register of `c`: keeps the set alive (and out of the other set's registers) up to here
template <bool NOBG>
__device__ __forceinline__ void p_keep(const PCur& c) {
  if constexpr (!NOBG) {
    asm volatile("" :: "v"(c.a1[0]), "v"(c.a1[1]), "v"(c.a1[2]), "v"(c.a2[0]), "v"(c.a2[1]), "v"(c.a2[2]));
    asm volatile("" :: "v"(c.bb[0]), "v"(c.bb[1]), "v"(c.bb[2]), "v"(c.bb[3]), "v"(c.gg[0]), "v"(c.gg[1]), "v"(c.gg[2]), "v"(c.gg[3]));
  }
}
template <bool NOBG> __device__ __forceinline__ void p_keep(const PCurH&) {}  // (one set: nothing to keep apart)
__device__ __forceinline__ f32x4 mfma_bf16(u32x4v a, u32x4v b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the 24 beta / gamma MFMAs of one step (v_mfma_f32_16x16x4_f32);  D: col = i, row = 4 k + r
__device__ __forceinline__ void p_mfma(const PCur& c, f32x4 (&y2)[3][4]) {
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a1[t], c.bb[ct], y2[t][ct], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a2[t], c.gg[ct], y2[t][ct], 0, 0, 0);
}
// A node's FIRST pair: its alpha product and its first step's beta product take the inline constant 0 as C and so START the
// node's accumulators (the gamma product accumulates into the beta one): nothing clears the 96 accumulator registers between
// nodes.
__device__ __forceinline__ void p_mfma_first(const PCur& c, f32x4 (&y2)[3][4]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a1[t], c.bb[ct], zero, 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a2[t], c.gg[ct], y2[t][ct], 0, 0, 0);
}
// the same on pieces: 12 v_mfma_f32_16x16x32_f16 per step, beta and gamma in one
__device__ __forceinline__ f32x4 mfma_f16(u32x4v a, u32x4v b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ void p_mfma(const PCurH& c, f32x4 (&y2)[3][4]) {
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = mfma_f16(c.a[t], c.b[ct], y2[t][ct]);
}
__device__ __forceinline__ void p_mfma_first(const PCurH& c, f32x4 (&y2)[3][4]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) y2[t][ct] = mfma_f16(c.a[t], c.b[ct], zero);
}
// the 12 alpha MFMAs of a pair (v_mfma_f32_16x16x32_bf16)
template <bool FIRST>
__device__ __forceinline__ void p_mfma_alpha(const PAlpha& al, f32x4 (&t1)[3][4]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) t1[t][ct] = mfma_bf16(al.a[t], al.m[ct], FIRST ? zero : t1[t][ct]);
}

// The product wave's work as a stream of CHUNKS: at most 64 paths of one node (one register of triples); a node is one chunk
// (a hub: several), a node without paths one empty chunk.  Wave-uniform scalar state; the range of the node after the one
// being cut is read a node ahead (NodeRanges).
template <bool LIST>
struct ChunkGen {
  int64_t gi;            // node being cut into chunks (index into this workgroup's nodes; nodes >= cnt are empty)
  int32_t gp, gend;      // its remaining paths
  int32_t pa0, pa1;      // the path range of node gi + 1
  NodeRanges<LIST> nr;
  __device__ __forceinline__ void init(const int32_t* __restrict__ pptr, const int32_t* __restrict__ list, int64_t n0, int64_t N,
                                       int64_t nn, int64_t cnt) {
    nr.init(pptr, list, n0, N, nn, cnt);
    gi = 0;
    nr.get(0, gp, gend);
    nr.get(1, pa0, pa1);
  }
  // the next chunk [q0, q1) and whether it is its node's last
  __device__ __forceinline__ void next(int64_t cnt, int32_t& q0, int32_t& q1, bool& last) {
    q0 = gp; q1 = min(gp + 64, gend);
    last = q1 >= gend;
    if (last) {
      ++gi;
      gp = pa0; gend = pa1;
      nr.get(gi + 1, pa0, pa1);
    } else {
      gp = q1;
    }
  }
};

// The product wave of SIMD cg.  Steps come in PAIRS (8 paths): buffer A holds the loaded operands of the pair's first step, B
// of its second; each is refilled for the NEXT pair -- this chunk's, or the next chunk's first (usually the next node's) --
// right after its values were turned into MFMA operands, so two steps' loads (12 instructions) are in flight behind the
// MFMAs being issued.  A pair's order: wait A, transform A (its beta / gamma operands and its slots of the alpha operands),
// refill A, A's 24 beta / gamma MFMAs, wait B, transform B, refill B, the pair's 12 alpha MFMAs, B's 24 beta / gamma MFMAs
// (regression likelihood, NOBG: the 12 alpha MFMAs are the pair's only ones).  The loads are unconditional and in one fixed order, the hand-counted waits rely on it; A / B are written
// nowhere else inside the loop.  Hence the chunk stream: hubs and empty nodes take the same path as everything else; a step past
// the chunk's last path multiplies zero weights (meta_finish), an empty chunk is one such step.
// A pair is ONE body with two wave-uniform flags, and the flags only choose among MFMAs and the operand transform: every load,
// wait, p_keep pin and refill is outside the branches, in the same order and number whatever the flags are, so every counted
// vmcnt holds whichever pairs follow each other.
//   first  the first pair of a node: its alpha MFMAs and its first step's beta MFMAs take C = 0 (p_mfma_alpha<true>,
//          p_mfma_first), which is what clears the accumulators -- nothing else does;
//   half   the last pair of a chunk whose second step has no path (4 (2 j + 1) >= paths of the chunk): p_wait(B) and B's refill
//          stay, B's beta / gamma operands and MFMAs are left out; its slots of the alpha operands are written as ever (zero
//          weights: see PAlpha) -- a branch around them makes hipcc keep the seven operand tuples twice and copy them.
// (Four complete straight-line bodies, one per flag combination, is what was tried first: hipcc then gives the accumulators
// and the in-flight operand registers new values per body, moves them between registers at the joins and spills 130 - 500
// registers; with the branches around the MFMAs alone the accumulators stay where they are.)
// An earlier branch around the second step's MFMAs "gave wrong tiles now and then".  Its code is gone, so the cause cannot be
// read off it; the two suspects are the MFMA -> VALU wait states between a branch's last MFMA and the tile write's first
// accumulator read (in a `half` pair that MFMA is a 16x16x32 bf16 one now: no more passes than the fp32 one), and a load inside
// the branch that broke the counts.  In the ISA of the straight-line loop twelve buffer
// loads, the poll of `done` (an LDS read and its wait) and a vmcnt(0) lie between the two, far more than the 12 wait states of
// the 8-pass 16x16x4 -- but nothing there is a guarantee, and hipcc places no s_nop of its own.  Both are excluded by
// construction now: no branch holds a load, and `s_nop 11` (12 wait states) sits in front of the tile write's first
// accumulator read on every path.
template <bool NOBG, bool HI, class CUR>
__device__ __forceinline__ void pair_body(const PTables& tb, const PMeta& mx, int sx, const PLane& pl, POps& A, POps& B, CUR& cA,
                                          CUR& cB, PAlpha& al, f32x4 (&t1)[3][4], f32x4 (&y2)[3][4], bool first, bool half) {
  constexpr int NL = kStepLoads<NOBG>;
  // A's loads: the NL youngest outstanding may be B's (the first pair of a chunk: B's and the three path loads -- there
  // the count also waits for B's first half, issued a whole pair earlier)
  p_wait<NOBG, NL>(A);
  p_xform<NOBG, HI, false>(A, pl, cA, al, true);
  p_keep<NOBG>(cB);  // (cB's MFMAs may still be queued: cA must not be prepared into their operand registers)
  p_load<NOBG>(tb, mx, sx, pl, A);
  if constexpr (!NOBG) {
    if (first) p_mfma_first(cA, y2);
    else p_mfma(cA, y2);
  }
  p_wait<NOBG, NL>(B);  // (younger: A's refill)
  p_xform<NOBG, HI, true>(B, pl, cB, al, !half);
  p_keep<NOBG>(cA);  // (likewise)
  p_load<NOBG>(tb, mx, sx + 1, pl, B);
  if (first) p_mfma_alpha<true>(al, t1);
  else p_mfma_alpha<false>(al, t1);
  if constexpr (!NOBG)
    if (!half) p_mfma(cB, y2);
}
// CUR: the form of the beta / gamma operands, PCur (fp32 MFMAs) or PCurH (fp16 pieces: the tables are then the piece table and
// the coefficient rows that go with it, which path_bound_kernel leaves behind the normalised fp32 table)
template <bool LIST, bool NOBG, bool HI, class CUR>
__device__ __forceinline__ void product_role(const YArgs& a, const int32_t* __restrict__ pptr, const int32_t* __restrict__ list,
                                             FusedShared& sh, int64_t nn, int64_t cnt, int cg, float scale, bool f32_tile) {
  const int lane = threadIdx.x & 63;
  const int H = a.H;
  const bool path_wave = 64 * cg < H;  // (H <= 192: the last product wave has no columns)
  if (!path_wave) return;  // (its ready counter was set to "everything" at the kernel's top)
  PLane pl;
  const int li = lane & 15;
  pl.kq = lane >> 4;
  const int col = 64 * cg + 4 * li;
  const bool col_ok = col < H;  // (H % 4 == 0: the lane's four columns are in or out together)
  pl.oc = 16u * uint32_t(li);
  pl.ob = col_ok ? 4u * uint32_t(col) : 0u;
  pl.om = col_ok ? 4u * uint32_t(col >> 5) : 0x7ffffff0u;  // (past H: outside the mask, the load returns zero bits)
  pl.mshift = col & 31;
  const uint32_t row_bytes = uint32_t(H) * 4u, mask_bytes = uint32_t(a.mask_words) * 4u;
  PTables tb;
  constexpr bool PH = __is_same(CUR, PCurH);
  static_assert(!(PH && NOBG), "the piece products are the beta / gamma products");
  const float* __restrict__ tab = PH ? a.bg + piece_table_offset(a.M, H) : a.bg;
  tb.coef = make_rsrc(PH ? a.bg + piece_coef_offset(a.M, H) : a.coef, uint64_t(a.n_coef) * kCoefRow * 4);
  tb.b = make_rsrc(tab, uint64_t(a.M) * row_bytes);
  tb.g = make_rsrc(tab + a.M * int64_t(H), uint64_t(a.M) * row_bytes);
  tb.mask = make_rsrc(a.mask, uint64_t(a.N) * mask_bytes);
  tb.pm = make_rsrc(a.pm, uint64_t(a.cap) * 4);
  tb.pv = make_rsrc(a.pv, uint64_t(a.cap) * 4);
  tb.pw = make_rsrc(a.pw, uint64_t(a.cap) * 4);
  // W_1's rows of the launch, read at the tile write (48 KB that every workgroup reads: L2 resident)
  const uint32_t w1_row_bytes = uint32_t(a.w1_ld) * 4u;
  const i32x4 w1rs = make_rsrc(a.W1 + int64_t(a.c0) * a.w1_ld, uint64_t(a.R - 1) * w1_row_bytes + row_bytes);
  constexpr int NL = kStepLoads<NOBG>;
  ChunkGen<LIST> gen;
  gen.init(pptr, list, a.n0, a.N, nn, cnt);
  int32_t q0c, q1c, q0n, q1n;
  bool lastc, lastn;
  gen.next(cnt, q0c, q1c, lastc);
  gen.next(cnt, q0n, q1n, lastn);
  PMeta mc, mn;
  meta_issue(tb, q0c, q1c, lane, mc);
  meta_issue(tb, q0n, q1n, lane, mn);
  meta_finish<0>(q0c, q1c, lane, row_bytes, mask_bytes, scale, mc);
  meta_finish<0>(q0n, q1n, lane, row_bytes, mask_bytes, scale, mn);
  POps A, B;
  p_load<NOBG>(tb, mc, 0, pl, A);
  p_load<NOBG>(tb, mc, 1, pl, B);
  // the node's accumulators: started by the first step of the node's first pair (pair_body, `first`), never cleared.  (The
  // zeros here are y2's value under NOBG, where no MFMA writes it.)
  f32x4 t1[3][4], y2[3][4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) { t1[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f}; y2[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // Two sets of prepared MFMA operands, alternating (p_keep pins them to registers of their own): the next step is prepared
  // while the MFMAs of the previous one may still be reading theirs.  The pieces have ONE set (cB is cA, p_keep is empty):
  // the transform of a pair's second step then follows the first step's MFMAs by ordinary register dependency -- the
  // MFMAs are builtins, hipcc orders the rewrite of their operands behind them.
  CUR cA = {}, cB_ = {};
  CUR& cB = PH ? cA : cB_;  // (the pieces: one set)
  // the pair's alpha operands; the fourth register of each (the two empty K slots) stays zero
  PAlpha al;
#pragma unroll
  for (int t = 0; t < 3; ++t) al.a[t] = u32x4v{0u, 0u, 0u, 0u};
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) al.m[ct] = u32x4v{0u, 0u, 0u, 0u};
  bool node_has = false;  // the node being built has a path so far
  bool firstc = true;     // the chunk being run is its node's first
  for (int64_t i = 0; i < cnt;) {  // node i's tile is built while the Gram waves contract node i - 1's (or i - 2's)
    // the chunk after the next: its range now, its paths a whole chunk before they are used.  In flight from here
    // (oldest first): A, B (issued by the previous chunk's last pair), these three loads
    int32_t q0f, q1f;
    bool lastf;
    gen.next(cnt, q0f, q1f, lastf);
    PMeta mf2;
    meta_issue(tb, q0f, q1f, lane, mf2);
    const int kch = q1c - q0c, np = max((kch + 7) >> 3, 1);
    node_has = node_has || kch > 0;
    // NOT peeled (unroll(disable) also keeps hipcc from peeling the first pair off for the sake of `first`): the peeled pair
    // and the loop's body kept A's coefficient registers in different places, and the copy between them sat on the loop's exit
    // -- in front of the wait, where the refill was still in flight: stale operands now and then.  Nothing but the counted
    // waits orders a use behind these loads, so the kernel's ISA must not copy an operand register between a load and its wait.
#pragma clang loop unroll(disable)
    for (int j = 0; j < np; ++j) {
      // the pair after this one: this chunk's, else the next chunk's first
      const bool more = j + 1 < np;
      PMeta mx;
      mx.oc = more ? mc.oc : mn.oc; mx.ob = more ? mc.ob : mn.ob; mx.om = more ? mc.om : mn.om; mx.w = more ? mc.w : mn.w;
      const int sx = more ? 2 * (j + 1) : 0;
      const bool first = firstc && j == 0, half = !more && 4 * (2 * j + 1) >= kch;  // (wave uniform)
      pair_body<NOBG, HI, CUR>(tb, mx, sx, pl, A, B, cA, cB, al, t1, y2, first, half);
    }
    if (lastc) {
      // W_1's 48 x 4 values of the lane: twelve 16-byte loads, the YOUNGEST vector-memory operations of the wave from here to
      // the vmcnt(0) below (older, in order: the three path loads of the loop's top, the refills of A and B).  A row past the
      // launch's classes lies outside the descriptor and reads zeros; so does every row of a lane past H (w1_off).
      // The lane's place in the tile is worked out HERE, per node, from an opaque copy of the lane number: as loop invariants
      // the twelve load offsets and the store offsets would hold some twenty registers through the pair loop, which has
      // none to spare (the alpha operands took them), for the sake of as many vector instructions per node.
      int wl = lane;
      asm volatile("" : "+v"(wl));
      const int wkq = wl >> 4, wcol = 64 * cg + 4 * (wl & 15);
      const bool wcol_ok = wcol < H;
      const uint32_t w1_off = wcol_ok ? uint32_t(4 * wkq) * w1_row_bytes + 4u * uint32_t(wcol) : 0x7ff00000u;
      // the lane's two 16-byte stores inside a piece plane (dword offsets: columns col, col + 1 and col + 2, col + 3)
      const int pc_lo = 8 * (wcol >> 2) + 4 * piece_swap(wcol >> 2), pc_hi = pc_lo ^ 4;
      f32x4 w1[3][4];
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (t == 0 && r == 0) bload4<0, true>(w1[t][r], w1_off, w1rs);
          else bload4<0>(w1[t][r], w1_off + uint32_t(16 * t + r) * w1_row_bytes, w1rs);
        }
      // tile i & 1 was last read by the Gram of node i - 2: every Gram wave must have counted i - 1 nodes
      if (i >= 2)
        while (lds_min4(sh.done) < int(i) - 1) __builtin_amdgcn_s_sleep(2);
      // (s_nop 11 behind the wait: the MFMA -> VALU wait states of the pair loop's last MFMAs, whichever body issued them;
      // see the header)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(w1[t][0]), "+v"(w1[t][1]), "+v"(w1[t][2]), "+v"(w1[t][3]) :: "memory");
      asm volatile("s_nop 11" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);  // (no accumulator read moves above the pad)
      if (node_has && wcol_ok) {
        // Y[n] = W_1 (.) T1 + Y2.  Rows past the launch's classes come out as the zeros they already are (their coefficients
        // and their rows of W_1 are zero): one branch around unconditional 16-byte stores.
        if (f32_tile) {  // the fp32 tile: twelve stores
          float (*ytile)[kYStride] = sh.y[i & 1];
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4 o;
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) o[ct] = w1[t][r][ct] * t1[t][ct][r] + y2[t][ct][r];
              *reinterpret_cast<f32x4*>(&ytile[16 * t + 4 * wkq + r][wcol]) = o;
            }
        } else {
          // the pieces: the lane's rows 16 t + 4 kq + 0 .. 3 are group 4 t + kq, its columns two 16-byte stores per plane
          uint32_t* __restrict__ grp = &sh.pc[i & 1][wkq][0][0];
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            u32x4v pz[2][2];  // [piece h0, h1][column pair]: (rows 0 1 | rows 2 3) of the pair's two columns
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
              for (int rp = 0; rp < 2; ++rp) {
                const float ya = w1[t][2 * rp][ct] * t1[t][ct][2 * rp] + y2[t][ct][2 * rp];
                const float yb = w1[t][2 * rp + 1][ct] * t1[t][ct][2 * rp + 1] + y2[t][ct][2 * rp + 1];
                uint32_t q0, q1;
                split_pair(ya, yb, q0, q1);
                pz[0][ct >> 1][2 * (ct & 1) + rp] = q0;
                pz[1][ct >> 1][2 * (ct & 1) + rp] = q1;
              }
            uint32_t* __restrict__ g = grp + 4 * t * kGroupDwords;
            // planes in the order (h1, h0, h1)
            *reinterpret_cast<u32x4v*>(g + pc_lo) = pz[1][0];
            *reinterpret_cast<u32x4v*>(g + pc_hi) = pz[1][1];
            *reinterpret_cast<u32x4v*>(g + kPlaneDwords + pc_lo) = pz[0][0];
            *reinterpret_cast<u32x4v*>(g + kPlaneDwords + pc_hi) = pz[0][1];
            *reinterpret_cast<u32x4v*>(g + 2 * kPlaneDwords + pc_lo) = pz[1][0];
            *reinterpret_cast<u32x4v*>(g + 2 * kPlaneDwords + pc_hi) = pz[1][1];
          }
        }
      }
      ++i;
      lds_publish(&sh.ready[cg], int(i), lane);
      // The accumulators' values end here: the next pair is a node's first and starts them.  hipcc cannot know that (the
      // flag is data), and would keep all 96 registers live through the tile write above -- where the 48 values of W_1 and
      // the pieces need them: an empty statement that defines them anew, no instruction.
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        asm volatile("" : "=v"(t1[t][0]), "=v"(t1[t][1]), "=v"(t1[t][2]), "=v"(t1[t][3]));
        if constexpr (!NOBG) asm volatile("" : "=v"(y2[t][0]), "=v"(y2[t][1]), "=v"(y2[t][2]), "=v"(y2[t][3]));
      }
      node_has = false;
    }
    // rotate the chunk stream (the paths issued at the top are older than the 2 NL loads of the last pair's refills)
    meta_finish<2 * NL>(q0f, q1f, lane, row_bytes, mask_bytes, scale, mf2);
    firstc = lastc;
    q0c = q0n; q1c = q1n; lastc = lastn; mc = mn;
    q0n = q0f; q1n = q1f; lastn = lastf; mn = mf2;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the refills past the last chunk
}

// The Gram wave W: its 9 upper 32 x 32 sub-tiles of gram256.h, each as 2 x 2 tiles of v_mfma_f32_16x16x4_f32 (the lower tile
// of a diagonal sub-tile is never read by the symmetrising pass and is skipped: 34 MFMAs per four tile rows).  The SAME
// instruction shape as the product wave's on purpose: the two waves of a SIMD take turns on its matrix pipe instruction by
// instruction, so with 64-cycle 32x32x2 instructions here every one of the product wave's 32-cycle instructions waited 64
// cycles and that wave -- a third of the pipe's time for a third of the work plus its serial sections -- was the critical path
// (measured: its node time = time alone + 155 x 64 cycles; Gram waves idle 30 %).
// Operand of a k step (4 tile rows) for the 16 columns 32 b + 16 h: lane l holds Y[k0 + (l >> 4)][32 b + 16 h + (l & 15)] -- as
// A operand (row l & 15, k = l >> 4) and as B operand (k = l >> 4, column l & 15) alike.
template <int W>  // (the flush both Gram roles share, below)
__device__ __forceinline__ void gram_flush(const YArgs& a, const f32x4 (&acc)[9][2][2], float inv2, float* __restrict__ scratch);
template <int W>
__device__ __forceinline__ void gram16_load(const float* __restrict__ p, float (&x)[8][2]) {
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    x[b][0] = tiles256_uses<W>(b) ? p[b * 32] : 0.f;
    x[b][1] = tiles256_uses<W>(b) ? p[b * 32 + 16] : 0.f;
  }
}
template <int W>
__device__ __forceinline__ void gram16_mfma(const float (&x)[8][2], f32x4 (&acc)[9][2][2]) {
#pragma unroll
  for (int s = 0; s < 9; ++s)
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
      for (int hj = 0; hj < 2; ++hj) {
        if (Tiles256<W>::si[s] == Tiles256<W>::sj[s] && hi > hj) continue;  // (below the diagonal)
        acc[s][hi][hj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[Tiles256<W>::si[s]][hi], x[Tiles256<W>::sj[s]][hj],
                                                              acc[s][hi][hj], 0, 0, 0);
      }
}
template <int W, bool LIST>
__device__ __forceinline__ void gram_role(const YArgs& a, const int32_t* __restrict__ pptr, const int32_t* __restrict__ list,
                                          FusedShared& sh, int64_t nn, int64_t cnt, float* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  f32x4 acc[9][2][2];
#pragma unroll
  for (int s = 0; s < 9; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[s][q >> 1][q & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (a.R + 3) >> 2;  // tile rows four at a time (rows past R are zero)
  NodeRanges<LIST> nr;
  nr.init(pptr, list, a.n0, a.N, nn, cnt);
  int32_t p0, p1;
  nr.get(0, p0, p1);
  for (int64_t i = 0; i < cnt; ++i) {
    int32_t q0, q1;
    nr.get(i + 1, q0, q1);
    // node i's tile: every product wave must have published i + 1 nodes
    while (lds_min4(sh.ready) < int(i) + 1) __builtin_amdgcn_s_sleep(2);
    if (p1 > p0) {
      const float* __restrict__ base = &sh.y[i & 1][0][0] + (lane >> 4) * kYStride + (lane & 15);
      float xa[8][2], xb[8][2];
      gram16_load<W>(base, xa);
      for (int kk = 0; kk < nk; kk += 2) {
        if (kk + 1 < nk) gram16_load<W>(base + (kk + 1) * 4 * kYStride, xb);
        __builtin_amdgcn_sched_barrier(0);
        gram16_mfma<W>(xa, acc);
        __builtin_amdgcn_sched_barrier(0);
        if (kk + 1 < nk) {
          if (kk + 2 < nk) gram16_load<W>(base + (kk + 2) * 4 * kYStride, xa);
          __builtin_amdgcn_sched_barrier(0);
          gram16_mfma<W>(xb, acc);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    lds_publish(&sh.done[W], int(i) + 1, lane);  // (the tile's reads have returned: the MFMAs above consumed them)
    p0 = q0; p1 = q1;
  }
  gram_flush<W>(a, acc, 1.f, scratch);  // (accumulator layout of 16x16x4: column l & 15, rows 4 (l >> 4) + r)
}

// The same Gram on v_mfma_f32_16x16x32_f16 (the default; LGNN_GRAM_F32=1, or a launch without a usable scale, runs gram_role
// above).  Every SCALED fp32 tile value y' = s cn_j y (GramScale: |y'| <= 2^15) is split into two fp16 pieces, each rounded
// to nearest:  h0 = fp16(y'), h1 = fp16(y' - h0)  (the difference is exact; each piece carries 11 significand bits, so h0 + h1
// is y' to 2^-22 |y'| while h1 is a normal fp16, |y'| >= 2^-3 or so, and to 2^-25 absolutely -- half an fp16 subnormal step --
// below: 2^-40 of the launch's range).  A product y z is ALL FOUR piece products, h0 k0 + h1 k1 + h0 k1 + h1 k0 = (h0 + h1)(k0 +
// k1): nothing is dropped.  The product waves form the pieces (split_pair) and store them in the layout of FusedShared: this
// role only reads them.  Why two scales: fp16 has 5 exponent bits, the pieces of a value 2^-12 below the range are short and
// those 2^-25 below it are gone.  The columns of a tile differ by what W_1's columns differ by (tests run 2^30), so they are
// normalised one by one, for free (PathScale in paths.h); what is left is the spread over nodes and classes inside a column,
// where a value far below the column's largest does not matter to the column's sums of squares.
// WHY THIS SHAPE: the two waves of a SIMD take turns on its matrix pipe instruction by instruction (gram_role's header), so
// every MFMA of the product wave waits one instruction of this wave: 16 cycles with the 16x16x32 form, 32 with 32x32x16
// (a full arxiv batch 3.75 -> 3.62 ms for that alone).
// Tiles: gram_role's, acc[9][2][2] of 16 x 16 (34 per wave, 136 accumulator registers; lane l holds D[4 (l >> 4) + r][l & 15]).
// Operands: a lane is (column l & 15 of a 16-column block, K group q = l >> 4); for the 16-row chunk cc lane group q reads the
// row group 4 cc + q: per 16-column block the 8 bytes of its column from the planes h1, h0 and h1 again, six registers
// (h1a h1b h0a h0b h1a h1b; a = rows 0 1 of the group, b = rows 2 3), in two operand forms that overlap:
//     T = (h1a h1b h0a h0b),  U = (h0a h0b h1a h1b).
// Per chunk and tile two MFMAs with K = 32 = 4 row groups x (2 pieces x 4 rows):
//     T[i] x T[j] = h1 k1 + h0 k0,   T[i] x U[j] = h1 k0 + h0 k1.
// (U x U + U x T is the same sum; with THIS pair -- T the only A operand, U a B operand alone -- hipcc keeps the six registers
// of a block where the reads put them, 8 v_mov per chunk; with U as the A operand it builds operands through scratch memory.)
// Which K slot a (lane group, register half) is does not matter and is nowhere written down: the instruction's A and B layouts
// mirror each other (lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15]), and A and B of one
// lane are filled by the same reads, so slot k of A and slot k of B are the same (tile row, piece) whatever k is.
// AN ODD NUMBER OF 8-ROW CHUNKS (R = 40: five) needs nothing of its own any more: the tile's rows past R are zero pieces (the
// product waves store all 48 rows, zeros past the launch's classes), so the last 16-row chunk runs as it stands, its two
// MFMAs per tile being what the bf16 role's special case took.  (One MFMA -- lane groups 2, 3 on the same rows -- would need T
// x T in lane groups 0, 1 and T x U in 2, 3: B operands from different registers, a select per operand.)
// R = 40 is 3 x 2 = 6 MFMAs of 16 cycles per tile: 34 x 6 x 16 = 3 264 matrix cycles per node against 4 352 on three bf16 pieces.
// ONE operand set (96 registers beside 136 accumulators: a second set, or half of one, does not fit): a wave's sub-tiles run
// in the order GramOrder names, chosen so that its column blocks are used up one after the other; the reads of the NEXT chunk's
// block go out right behind the last MFMA that reads the block, a sub-tile and a half or more before their first use.  Behind
// a node's last chunk those reads fetch the same chunk again (values nobody uses): the body stays straight-line.
// Inside a sub-tile the order is all T x T, all T x U: an accumulator comes round every third or fourth MFMA.
// Bank conflicts: the 16 lanes of a lane group read 128 contiguous bytes of a plane (permuted by piece_col), but groups and
// planes are multiples of 256 bytes apart, so the two lane groups that share an LDS cycle (ds_read_b64 serves lanes 0 - 31,
// then 32 - 63) meet on the same 32 banks: every read is 2-way, 4 LDS cycles instead of 2 -- 36 reads per chunk beside
// 68 MFMAs of 16 cycles.  (Only a layout with the rows of a group pair side by side could avoid it.)
// A NaN or an infinity never gets here: it makes the launch's bound non-finite, and the launch runs the fp32 role.
struct PieceBlk { u32x4v t; u32x2v h1; };  // a 16-column block's pieces of the lane's 4 rows of a chunk, (rows 0 1 | rows 2 3)
                                            // each: t = (h1, h0) is the form T as it stands, U is its upper half beside h1

// the order a wave runs its sub-tiles in (indices into Tiles256<W>).  Wave 0: (0,0) (0,2) (0,3) (0,4) (0,5) (0,1) (1,1) (1,2)
// (1,3); waves 1, 2: the two with the far row block, the 2 x 2 between the pairs, the own pair's; wave 3: (6,6) (1,6) (2,6)
// (3,6) (6,7) (1,7) (2,7) (3,7) (7,7)
template <int W> struct GramOrder;
template <> struct GramOrder<0> { static constexpr int o[9] = {0, 3, 4, 7, 8, 1, 2, 5, 6}; };
template <> struct GramOrder<1> { static constexpr int o[9] = {7, 8, 3, 4, 5, 6, 0, 1, 2}; };
template <> struct GramOrder<2> { static constexpr int o[9] = {7, 8, 3, 4, 5, 6, 0, 1, 2}; };
template <> struct GramOrder<3> { static constexpr int o[9] = {0, 7, 3, 5, 1, 8, 4, 6, 2}; };
// position in that order of the last sub-tile that reads the 32-column block b (-1: the wave does not use it)
template <int W> __device__ __forceinline__ constexpr int gram_last_use(int b) {
  int last = -1;
  for (int p = 0; p < 9; ++p)
    if (Tiles256<W>::si[GramOrder<W>::o[p]] == b || Tiles256<W>::sj[GramOrder<W>::o[p]] == b) last = p;
  return last;
}
template <int W> __device__ __forceinline__ constexpr int gram_first_use(int b) {  // (likewise the first)
  for (int p = 0; p < 9; ++p)
    if (Tiles256<W>::si[GramOrder<W>::o[p]] == b || Tiles256<W>::sj[GramOrder<W>::o[p]] == b) return p;
  return -1;
}

// the lane's pieces of its column in both 16-column halves of the 32-column block b: three ds_read_b64 each.  `off`: dword
// offset in the tile of the chunk's row group of the lane group + piece_col of the lane's column li in an even 16-column block;
// in the odd block beside it the swap of piece_col is the other one, piece_col(16 + li) = 32 + (piece_col(li) ^ 4), and
// everything else in `off` is a multiple of 8
__device__ __forceinline__ void piece_load(const uint32_t* __restrict__ tile, int off, int b, PieceBlk (&x)[8][2]) {
  const uint32_t* __restrict__ pe = tile + off;
  const uint32_t* __restrict__ po = tile + (off ^ 4) + 32;
  const u32x2v e1 = *reinterpret_cast<const u32x2v*>(pe + b * 64), e0 = *reinterpret_cast<const u32x2v*>(pe + kPlaneDwords + b * 64);
  const u32x2v o1 = *reinterpret_cast<const u32x2v*>(po + b * 64), o0 = *reinterpret_cast<const u32x2v*>(po + kPlaneDwords + b * 64);
  x[b][0].t = u32x4v{e1[0], e1[1], e0[0], e0[1]};
  x[b][0].h1 = *reinterpret_cast<const u32x2v*>(pe + 2 * kPlaneDwords + b * 64);
  x[b][1].t = u32x4v{o1[0], o1[1], o0[0], o0[1]};
  x[b][1].h1 = *reinterpret_cast<const u32x2v*>(po + 2 * kPlaneDwords + b * 64);
}
__device__ __forceinline__ u32x4v piece_u(const PieceBlk& p) { return u32x4v{p.t[2], p.t[3], p.h1[0], p.h1[1]}; }
__device__ __forceinline__ u32x4v piece_t(const PieceBlk& p) { return p.t; }
// A 16-row chunk: 34 x 2 MFMAs, and the next chunk's reads (at `off` of the tile) as the blocks are used up.
template <int W>
__device__ __forceinline__ void piece_chunk16(PieceBlk (&x)[8][2], f32x4 (&acc)[9][2][2], const uint32_t* tile, int off) {
#pragma unroll
  for (int p = 0; p < 9; ++p) {
    const int s = GramOrder<W>::o[p], si = Tiles256<W>::si[s], sj = Tiles256<W>::sj[s];
    // An empty statement that redefines a block's registers where the chunk first uses them: hipcc otherwise forms U (a copy
    // of h0 beside h1) right behind the reads and waits for them there, with the latency in the open.
#pragma unroll
    for (int b = 0; b < 8; ++b)
      if (gram_first_use<W>(b) == p)
#pragma unroll
        for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(x[b][h].t), "+v"(x[b][h].h1));
    const u32x4v ta[2] = {piece_t(x[si][0]), piece_t(x[si][1])};
    const u32x4v ub[2] = {piece_u(x[sj][0]), piece_u(x[sj][1])}, tb[2] = {piece_t(x[sj][0]), piece_t(x[sj][1])};
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj) {
          if (si == sj && hi > hj) continue;  // (below the diagonal)
          acc[s][hi][hj] = mfma_f16(ta[hi], f == 1 ? ub[hj] : tb[hj], acc[s][hi][hj]);
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < 8; ++b)
      if (gram_last_use<W>(b) == p) piece_load(tile, off, b, x);
  }
}
// S += (what a Gram wave holds) * inv2 / (cn_i cn_j): undoes the launch's scale (GramScale; 1 for the fp32 role) and the
// column normalisation of PathScale.  Of a diagonal sub-tile only the part on and above the diagonal (the symmetrising pass
// rewrites the rest).  (The lane's place is worked out anew, from nothing that lives through the node loop.)
template <int W>
__device__ __forceinline__ void gram_flush(const YArgs& a, const f32x4 (&acc)[9][2][2], float inv2, float* __restrict__ scratch) {
  const int64_t D = a.H;
  const float* __restrict__ cinv = a.scale + kScaleCinv;
  const int fl = int(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
  const int li = fl & 15, lq = (fl >> 4) & 3;
#pragma unroll
  for (int s = 0; s < 9; ++s)
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
      for (int hj = 0; hj < 2; ++hj) {
        if (Tiles256<W>::si[s] == Tiles256<W>::sj[s] && hi > hj) continue;
        const int64_t jj = Tiles256<W>::sj[s] * 32 + 16 * hj + li;
        const float cj = inv2 * cinv[jj];  // (jj < 256: inside the block whatever H is)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t ii = Tiles256<W>::si[s] * 32 + 16 * hi + 4 * lq + r;
          if (ii < D && jj < D && (Tiles256<W>::si[s] != Tiles256<W>::sj[s] || ii <= jj))
            atomicAdd(&scratch[ii * D + jj], acc[s][hi][hj][r] * cj * cinv[ii]);
        }
      }
}
template <int W, bool LIST>
__device__ __forceinline__ void gram_f16_role(const YArgs& a, const int32_t* __restrict__ pptr, const int32_t* __restrict__ list,
                                              FusedShared& sh, int64_t nn, int64_t cnt, float inv2, float* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  f32x4 acc[9][2][2];
#pragma unroll
  for (int s = 0; s < 9; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[s][q >> 1][q & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n16 = (a.R + 15) >> 4;  // chunks of 16 tile rows (rows past R are zero pieces; 16 n16 <= kYRows)
  // dword offset inside a tile (piece_load) of the lane's reads of chunk 0: lane group q reads the row group q of a chunk
  const int start = (lane >> 4) * kGroupDwords + piece_col(lane & 15);
  NodeRanges<LIST> nr;
  nr.init(pptr, list, a.n0, a.N, nn, cnt);
  int32_t p0, p1;
  nr.get(0, p0, p1);
  for (int64_t i = 0; i < cnt; ++i) {
    int32_t q0, q1;
    nr.get(i + 1, q0, q1);
    // node i's tile: every product wave must have published i + 1 nodes
    while (lds_min4(sh.ready) < int(i) + 1) __builtin_amdgcn_s_sleep(2);
    if (p1 > p0) {
      const uint32_t* tile = &sh.pc[i & 1][0][0][0];
      int off = start;
      PieceBlk x[8][2];
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (tiles256_uses<W>(b)) piece_load(tile, off, b, x);
      __builtin_amdgcn_sched_barrier(0);
      for (int cc = 0; cc < n16; ++cc) {  // (wave-uniform trip count)
        off += cc + 1 < n16 ? 4 * kGroupDwords : 0;
        piece_chunk16<W>(x, acc, tile, off);
      }
    }
    lds_publish(&sh.done[W], int(i) + 1, lane);  // (the tile's reads have returned: LDS operations execute in order)
    p0 = q0; p1 = q1;
  }
  gram_flush<W>(a, acc, inv2, scratch);
}

// The launch's scale (wave uniform, the same in every wave of every workgroup): s = 2^e with s * bound in [2^14, 2^15) for the
// bound of PathScale (paths.h), so that every scaled tile value is an fp16 well below 65504 whatever the last bit of the
// fp32 sums does; inv2 = s^-2 for the flush.  The fp16 role runs for 2^-49 <= bound < 2^78 (biased exponents 78 .. 204), where
// s (2^-63 .. 2^63) and s^-2 are normal fp32 numbers, the scaled weights w s and alpha pieces stay far inside fp32's range,
// and a workgroup's sums of s^2 y^2 <= 2^30 cannot overflow; a zero, tiny, huge or non-finite bound (and LGNN_GRAM_F32) gives
// s = 1 and the fp32 tile and role -- at 2^78 the Gram's entries pass fp32's range themselves.
// PH: the scale of the instance that runs the beta / gamma products on fp16 pieces (the share of `tri` that stands for the sums'
// rounding is 2^-9 there, 2^-12 with fp32 products: a piece product carries 2^-21 where the fp32 MFMA carries 2^-24).
struct GramScale { float s, inv2; bool f32; };
template <bool PH>
__device__ __forceinline__ GramScale gram_scale(const YArgs& a, const int32_t* __restrict__ pptr) {
  const float wsum = __int_as_float(pptr[a.N + 1]);  // (the word behind the list's pointers: path_list_reserve)
  // (PathScale: the smaller of the two triangle inequalities and a share of the first for the sums' rounding; `tri` stands
  // in the sum as it is, so a NaN or an infinity in it stays visible whatever fminf does)
  const float tri = a.scale[0] * a.scale[1] + a.scale[2];
  const float bound = wsum * (fminf(tri, a.scale[3] * a.scale[1]) + (PH ? 0x1p-9f : 0x1p-12f) * tri);
  const uint32_t eb = __builtin_amdgcn_readfirstlane(int((__float_as_uint(bound) >> 23) & 0x1ffu));  // (a sign bit: a NaN's)
  GramScale g;
  g.f32 = a.gram_f32 != 0 || eb < 78u || eb > 204u;
  g.s = g.f32 ? 1.f : __uint_as_float((268u - eb) << 23);
  g.inv2 = g.f32 ? 1.f : __uint_as_float((2u * eb - 155u) << 23);
  return g;
}

// The role of a call's launches (kRole*, paths.h), written in front of them into the word of the scale block that both
// instances of the kernel below read, and that lgnn_last_paths_product_role reports beside the launch's wsum: the products run
// on pieces where PathScale's rule allows it (a comparison with a NaN is false) and the piece instance's scale is usable.
// One thread.  -1 where the path list overflowed its buffer (both instances return at once then).  The rule is evaluated here
// once per call, not in every wave of both instances: each instance's scale then has its role as a constant.
__global__ void path_role_kernel(YArgs a, const int32_t* __restrict__ pptr, float* __restrict__ sc) {
  const float tri = a.scale[0] * a.scale[1] + a.scale[2];
  const bool rule = a.gram_f32 == 0 && a.no_bg == 0 && fminf(tri, a.scale[3] * a.scale[1]) >= ldexpf(tri, -a.piece_share_log2);
  int role = gram_scale<false>(a, pptr).f32 ? kRoleF32 : kRoleGramF16;
  if (rule && !gram_scale<true>(a, pptr).f32) role = kRoleProductsF16;
  if (int64_t(pptr[a.N]) > a.cap) role = kRoleNone;
  sc[kScaleWsum] = __int_as_float(pptr[a.N + 1]);
  reinterpret_cast<int32_t*>(sc)[kScaleRole] = role;
}

// LIST: the node loop runs over a device-side list of the nodes that have a path.  PH: the instance whose product waves run
// the beta / gamma products on fp16 pieces.  A call launches BOTH instances and the one that path_role_kernel's word does not
// name returns at once -- two kernels, not two roles in one, so that each instance's registers are allocated for one form of
// the product role (both forms in one kernel: 256 VGPRs and two of them spilled, 128 / 114 SGPR spills) and the fp32 instance
// stays the code it was.  (One kernel with the rule as a run-time flag was not tried again after the loads got their pads.)
template <bool LIST, bool PH>
__global__ __launch_bounds__(512, 2) void paths_fused_kernel(YArgs a, const int32_t* __restrict__ pptr,
                                                             const int32_t* __restrict__ list, float* __restrict__ scratch) {
  __shared__ FusedShared sh;  // ONE LDS object
  if (int64_t(pptr[a.N]) > a.cap) return;  // the path list overflowed its buffer: the enumerating route takes over
  if ((reinterpret_cast<const int32_t*>(a.scale)[kScaleRole] == kRoleProductsF16) != PH) return;  // (the same in every workgroup)
  // the tiles are zero where nobody writes: columns >= H (zero bits are zero pieces); the fp32 form is the larger one
  static_assert(sizeof(sh.pc) >= sizeof(sh.y) && sizeof(sh.pc) % 16 == 0, "the tiles' union");
  for (int q = threadIdx.x; q < int(sizeof(sh.pc) / 16); q += 512) reinterpret_cast<u32x4v*>(&sh.pc[0][0][0][0])[q] = u32x4v{0u, 0u, 0u, 0u};
  if (threadIdx.x < 4) {
    sh.ready[threadIdx.x] = 64 * int(threadIdx.x) < a.H ? 0 : INT32_MAX;  // (H <= 192: the last product wave has no columns)
    sh.done[threadIdx.x] = 0;
  }
  __syncthreads();
  const int hw = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t stride = gridDim.x;
  const int64_t nn = LIST ? int64_t(__builtin_amdgcn_readfirstlane(*a.n_list)) : a.n1 - a.n0;
  const int64_t cnt = nn > int64_t(blockIdx.x) ? (nn - blockIdx.x + stride - 1) / stride : 0;
  // (hardware waves g and g + 4 share a SIMD: one product wave and one Gram wave on each, see the kernel's header)
  const GramScale gs = gram_scale<PH>(a, pptr);
  switch (hw) {
    // (the Gram role on fp16 pieces unless the launch has no usable scale or LGNN_GRAM_F32 asks for the fp32 one; wave-uniform,
    // and the same choice as the product waves' tile form: both read gs.f32)
    case 4: if (!PH && gs.f32) gram_role<0, LIST>(a, pptr, list, sh, nn, cnt, scratch); else gram_f16_role<0, LIST>(a, pptr, list, sh, nn, cnt, gs.inv2, scratch); break;
    case 5: if (!PH && gs.f32) gram_role<1, LIST>(a, pptr, list, sh, nn, cnt, scratch); else gram_f16_role<1, LIST>(a, pptr, list, sh, nn, cnt, gs.inv2, scratch); break;
    case 6: if (!PH && gs.f32) gram_role<2, LIST>(a, pptr, list, sh, nn, cnt, scratch); else gram_f16_role<2, LIST>(a, pptr, list, sh, nn, cnt, gs.inv2, scratch); break;
    case 7: if (!PH && gs.f32) gram_role<3, LIST>(a, pptr, list, sh, nn, cnt, scratch); else gram_f16_role<3, LIST>(a, pptr, list, sh, nn, cnt, gs.inv2, scratch); break;
    default:
      if constexpr (PH) {  // (never under no_bg, never with the fp32 tile)
        if (a.c0 != a.cb) product_role<LIST, false, true, PCurH>(a, pptr, list, sh, nn, cnt, hw, gs.s, false);
        else product_role<LIST, false, false, PCurH>(a, pptr, list, sh, nn, cnt, hw, gs.s, false);
      } else if (a.c0 != a.cb) {  // classes cb + 48 ..: the fourth tile of the coefficient slots
        if (a.no_bg) product_role<LIST, true, true, PCur>(a, pptr, list, sh, nn, cnt, hw, gs.s, gs.f32);
        else product_role<LIST, false, true, PCur>(a, pptr, list, sh, nn, cnt, hw, gs.s, gs.f32);
      } else {
        if (a.no_bg) product_role<LIST, true, false, PCur>(a, pptr, list, sh, nn, cnt, hw, gs.s, gs.f32);
        else product_role<LIST, false, false, PCur>(a, pptr, list, sh, nn, cnt, hw, gs.s, gs.f32);
      }
      break;
  }
}

// persistent workgroups of paths_fused_kernel: one per CU (144 KB of LDS each).  Leaving CUs to the side stream's eigensolver
// did not help (252 / 248 / 240 workgroups: 50.6 / 51.5 / 52.4 ms per GraphSAGE fit)
constexpr int64_t kFusedWorkgroups = 256;

}  // namespace

bool fused_pieces_possible() {
  const char* e = getenv("LGNN_GRAM_F32");  // =1: the Gram role on fp32 MFMAs (the A/B arm and fallback); read per call
  return !(e && atoi(e) != 0);
}

int launch_paths_fused(lgnn_ctx* h, YArgs y, int64_t cb, int64_t ce, float* scratch, hipStream_t s) {
  LGNN_REQUIRE(y.N < (int64_t(1) << 31), "too many nodes for one launch");
  const dim3 grid{unsigned(std::min<int64_t>(y.n1 - y.n0, kFusedWorkgroups))};
  LGNN_REQUIRE(y.scale != nullptr, "internal: the fused kernel needs its scale block");
  y.Y = nullptr; y.gram_f32 = fused_pieces_possible() ? 0 : 1;
  hipLaunchKernelGGL(path_role_kernel, dim3(1), dim3(1), 0, s, y, y.pptr, const_cast<float*>(y.scale));
  LGNN_HIP_CHECK(hipGetLastError());
  for (int64_t c0 = cb; c0 < ce; c0 += kYRows) {
    y.c0 = int(c0); y.R = int(std::min<int64_t>(kYRows, ce - c0));
    if (h->timing) LGNN_CALL(record_event(h, s));  // dominant kernel of the KFAC path (bench.py roofline)
    if (y.list) hipLaunchKernelGGL((paths_fused_kernel<true, false>), grid, dim3(512), 0, s, y, y.pptr, y.list, scratch);
    else hipLaunchKernelGGL((paths_fused_kernel<false, false>), grid, dim3(512), 0, s, y, y.pptr, y.list, scratch);
    LGNN_HIP_CHECK(hipGetLastError());
    if (!y.no_bg && !y.gram_f32) {  // (the piece instance can only be named without either)
      if (y.list) hipLaunchKernelGGL((paths_fused_kernel<true, true>), grid, dim3(512), 0, s, y, y.pptr, y.list, scratch);
      else hipLaunchKernelGGL((paths_fused_kernel<false, true>), grid, dim3(512), 0, s, y, y.pptr, y.list, scratch);
      LGNN_HIP_CHECK(hipGetLastError());
    }
    if (h->timing) { LGNN_CALL(record_event(h, s)); h->ev_planes += y.R; }
  }
  return 0;
}

}  // namespace lgnn
