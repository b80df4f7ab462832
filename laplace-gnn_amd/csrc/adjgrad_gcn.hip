// Adjacency gradient, Kronecker posterior, plain 2-layer GCN: the per-batch chain of adjgrad.hip's header (seeds, u, g0, g0bar,
// ubar, g1bar, Vbar) and the kernels only it launches.  kfac_adjgrad_batch (adjgrad.hip) dispatches here.
#include <rocblas/rocblas.h>

#include "adjgrad.h"
#include "device_utils.h"

namespace lgnn {

namespace {

// The two consumers of g0bar's rows in ONE pass over the entries of the active rows a of P (they gather the same rows):
//     out[(a, b)] += sum_c <u_c[a], R_c[b]>                      (the SDDMM of the step g0 = P^T u)
//     U_c[a]       = dact[a] * sum_b P[a, b] R_c[b]               (ubar: the SpMM of the step behind it; overwrites u)
// Every gathered row of R is used for both: halves the gather traffic of the two steps and skips the 42 % of rows whose u
// is zero.  Plane major: grid (row groups, planes), one wave per (row, plane).  A wave that gathers k planes at once has a
// working set of k * 173 MB at the arxiv shape, far beyond the 256 MiB Infinity Cache, so its gathers go to HBM (3.3 TB/s
// measured); here all CUs work on ONE plane at a time (blocks are dispatched x first), which stays cache resident while its
// rows are gathered ~15 times each.  Eight entries per step; their eight dot products go through one shuffle tree (three
// halving exchanges leave lane l with entry l % 8, three more finish it); the planes' contributions to out[p] meet through
// float atomics.
__global__ __launch_bounds__(256) void sddmm_spmm_pm_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const float* __restrict__ val, const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ nrows_dev, float* __restrict__ U,
                                                            int64_t u_plane_stride, const float* __restrict__ R, int64_t N,
                                                            int64_t width, const float* __restrict__ dact,
                                                            float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int c0 = lane * 4;
  const bool col_ok = c0 < width;
  const int64_t total = rows ? int64_t(*nrows_dev) : N;
  const int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (w >= total) return;
  const int64_t a = rows ? int64_t(rows[w]) : w;
  const int64_t plane = blockIdx.y;
  float* __restrict__ Up = U + plane * u_plane_stride;
  const float* __restrict__ Rp = R + plane * N * width;
  const int32_t s = rowptr[a], e = rowptr[a + 1];
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f), dm = u, acc = u;
  if (col_ok) {
    u = *reinterpret_cast<const float4*>(Up + a * width + c0);
    dm = *reinterpret_cast<const float4*>(dact + a * width + c0);
  }
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0, b2 = (lane & 4) != 0;
  for (int32_t base = s; base < e; base += 64) {
    const int32_t p = base + lane;
    const int32_t cj = p < e ? col[p] : int32_t(a);  // padding entries re-read the row's own slice (cached), weight 0
    const float cv = p < e ? val[p] : 0.f;
    const int n = min(64, int(e - base));
    for (int u0 = 0; u0 < n; u0 += 8) {
      float4 x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t b = __builtin_amdgcn_readlane(cj, min(u0 + k, 63));
        x[k] = col_ok ? *reinterpret_cast<const float4*>(Rp + b * width + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float d[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), min(u0 + k, 63)));
        acc.x = fmaf(v, x[k].x, acc.x); acc.y = fmaf(v, x[k].y, acc.y);
        acc.z = fmaf(v, x[k].z, acc.z); acc.w = fmaf(v, x[k].w, acc.w);
        d[k] = u.x * x[k].x + u.y * x[k].y + u.z * x[k].z + u.w * x[k].w;
      }
      float e4[4], f2[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) e4[i] = (b0 ? d[2 * i + 1] : d[2 * i]) + __shfl_xor(b0 ? d[2 * i] : d[2 * i + 1], 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) f2[i] = (b1 ? e4[2 * i + 1] : e4[2 * i]) + __shfl_xor(b1 ? e4[2 * i] : e4[2 * i + 1], 2);
      float g = (b2 ? f2[1] : f2[0]) + __shfl_xor(b2 ? f2[0] : f2[1], 4);
      g += __shfl_xor(g, 8);
      g += __shfl_xor(g, 16);
      g += __shfl_xor(g, 32);
      // lane l < 8 holds the dot product of entry u0 + (l & 7) = u0 + 4 b2 + 2 b1 + b0
      if (lane < 8 && u0 + lane < n) atomicAdd(&out[base + u0 + lane], g);
    }
  }
  if (col_ok)
    *reinterpret_cast<float4*>(Up + a * width + c0) = make_float4(dm.x * acc.x, dm.y * acc.y, dm.z * acc.z, dm.w * acc.w);
}

// y[plane][r] = sum_p val[p] in[plane][col[p]] for rows of up to 256 columns, one wave per row, ENTRIES WITH A ZERO VALUE
// ARE NOT GATHERED (the per-batch copy of P^T's values has zeros at the columns of all-zero source rows: 42 % of the entries
// at the arxiv shape).  The plane is a buffer resource and the row a part of the vector offset: a dead slot's offset is out
// of range, the load returns zeros without touching memory, so the loop has no branch; 8 rows in flight per wave.
using srd_t = __amdgpu_buffer_rsrc_t;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
__global__ __launch_bounds__(256) void spmm256_skip_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, int64_t N, const float* __restrict__ in,
                                                           int64_t in_plane_stride, int64_t width, float* __restrict__ out) {
  constexpr int UNR = 8;
  constexpr uint32_t kDead = 0xfffff000u;
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int64_t plane = blockIdx.y;
  const uint32_t plane_bytes = uint32_t(N * width * 4);
  const srd_t srd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in + plane * in_plane_stride), 0, plane_bytes, 0x00020000);
  const uint32_t lane_off = lane * 4 < width ? uint32_t(lane) * 16u : kDead;
  const uint32_t row_bytes = uint32_t(width) * 4u;
  const int32_t s = rowptr[row], e = rowptr[row + 1];
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int32_t base = s; base < e; base += 64) {
    const int32_t p = base + lane;
    float cv = 0.f;
    uint32_t cj = kDead;
    if (p < e) {
      cv = val[p];
      if (cv != 0.f) cj = uint32_t(col[p]) * row_bytes;
    }
    const int n = min(64, int(e - base));
    for (int u0 = 0; u0 < n; u0 += UNR) {
      float4 x[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t so = uint32_t(__builtin_amdgcn_readlane(int(cj), min(u0 + u, 63)));
        // (a dead slot or a dead lane: kDead + anything below 4 KiB stays out of range of a < 4 GiB - 8 KiB plane)
        const uint32_t voff = so == kDead || lane_off == kDead ? kDead : so + lane_off;
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(srd, int(voff), 0, 0);
        x[u] = make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), min(u0 + u, 63)));
        y.x = fmaf(v, x[u].x, y.x); y.y = fmaf(v, x[u].y, y.y); y.z = fmaf(v, x[u].z, y.z); y.w = fmaf(v, x[u].w, y.w);
      }
    }
  }
  if (lane * 4 < width) *reinterpret_cast<float4*>(out + (plane * N + row) * width + lane * 4) = y;
}

// rows that are not active: ubar = 0 there (u was zero and stays zero: nothing to do; the planes were written in full by
// the GEMM, whose inactive rows are zeros already)

__global__ void mask_values_by_flag_kernel(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz,
                                           const uint8_t* __restrict__ active, float* __restrict__ out) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < nnz; p += stride) out[p] = active[col[p]] ? val[p] : 0.f;
}

// first occurrences of the batch's nodes: orows[t] = idx[m], lrows[t] = m for every m with pos[idx[m]] == m (the seed term's
// rows on the dense route; any order -- the rows are distinct)
__global__ void first_rows_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t N, const int32_t* __restrict__ pos,
                                  int32_t* __restrict__ orows, int32_t* __restrict__ lrows, int32_t* __restrict__ count) {
  const int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int64_t a = idx[m];
  if (a < 0 || a >= N || pos[a] != int32_t(m)) return;
  const int32_t t = atomicAdd(count, 1);
  orows[t] = int32_t(a);
  lrows[t] = int32_t(m);
}

}  // namespace

// (the caller has checked the model and ensured the auxiliary forward products and W^T)
int kfac_adjgrad_batch_gcn(lgnn_ctx* h, const int64_t* idx, const void* y, int64_t M, bool fork_exact, const float* gamma_B0,
                           const float* gamma_B1, float loss_scale, float* grad_P, float* out_bar, const int32_t* cand_a,
                           const int32_t* cand_b, int64_t K, float* grad_cand, hipStream_t s, float* dense) {
  const int64_t N = h->N, C = h->dims[2], H = h->dims[1], CC = C * C;
  LGNN_CALL(batch_prologue(h, idx, y, M, true, fork_exact, nullptr, s));

  // top layer: g1 planes [C][N][C] + flags / list of the rows that are not identically zero.  Without candidate pairs only
  // ACTIVE rows are ever read below (the zero-skipping SpMM, the active-row SDDMM + SpMM, the batch rows' gathers), so the
  // fit's own top-layer kernel writes just those rows (0.3 ms instead of 3.5 ms over all N rows) and the backward GEMM runs
  // over the compacted list (0.9 ms instead of 4.4 ms): rows that are not active hold whatever the buffers held and are
  // never looked at.  Candidate pairs can name any row: then everything is defined on all N rows as before.
  const bool compact = K == 0 && dense == nullptr && H == 256 && h->fc.mask_bits[0].p != nullptr && backgemm_supported(C, H, true) &&
                       (N + 1) * H * 4 < (int64_t(1) << 31);
  const int64_t u_stride = compact ? (N + 1) * H : N * H;  // the compacted backward GEMM wants a spare row per plane
  LGNN_CALL(h->ws.top.reserve(size_t(N) * CC * 4 + 16));
  LGNN_CALL(h->ws.active.reserve(size_t(N)));
  float* g1 = h->ws.top.as<float>();
  if (compact) {
    LGNN_CALL(kfac_top_planes(h, idx, M, fork_exact, g1, s));
  } else {
    LGNN_CALL(launch_seed_planes(h, g1, s));
    LGNN_CALL(compact_active_rows(h, s));
  }
  LGNN_CALL(h->ws.jac.reserve(size_t(M) * CC * 4));  // Vbar [M][C][C]
  float* vbar = h->ws.jac.as<float>();
  int32_t* first_rows = nullptr;
  if (dense) {  // the seed term's rows: the first occurrence of every batch node
    LGNN_CALL(h->ws.dense_rows.reserve(size_t(2 * M + 1) * 4));
    first_rows = h->ws.dense_rows.as<int32_t>();
    LGNN_HIP_CHECK(hipMemsetAsync(first_rows + 2 * M, 0, 4, s));
    hipLaunchKernelGGL(first_rows_kernel, dim3(unsigned(cdiv(M, 256))), dim3(256), 0, s, idx, M, N, h->ws.pos.as<int32_t>(),
                       first_rows, first_rows + M, first_rows + 2 * M);
    LGNN_HIP_CHECK(hipGetLastError());
  }
  // values of P^T with the columns of inactive (all-zero) source rows removed
  LGNN_CALL(h->ws.val_act.reserve(size_t(std::max<int64_t>(h->nnz, 1)) * 4));
  float* val_act = h->ws.val_act.as<float>();
  hipLaunchKernelGGL(mask_values_by_flag_kernel, dim3(unsigned(std::min<int64_t>(cdiv(std::max<int64_t>(h->nnz, 1), 256), 4096))),
                     dim3(256), 0, s, h->PT.col, h->PT.val, h->nnz, h->ws.active.as<uint8_t>(), val_act);
  LGNN_HIP_CHECK(hipGetLastError());

  // class chunks: three [cc][N][H] plane buffers (u / ubar, g0, g0bar) + g1bar [cc][N][C] under the workspace cap
  const int64_t per_class = N * (3 * H + C) * 4;
  const int64_t cc_max = std::max<int64_t>(1, std::min<int64_t>(C, h->ws_limit / std::max<int64_t>(per_class, 1)));
  LGNN_CALL(h->ws.planes_a.reserve(size_t(cc_max) * (u_stride + N * H) * 4));
  LGNN_CALL(h->ws.planes_b.reserve(size_t(cc_max) * N * (H + C) * 4));
  h->ws.planes_a_zero_ptr = nullptr;
  for (int64_t c0 = 0; c0 < C; c0 += cc_max) {
    const int64_t cc = std::min(cc_max, C - c0);
    float* U = h->ws.planes_a.as<float>();
    float* G0 = U + cc_max * u_stride;
    float* G0B = h->ws.planes_b.as<float>();
    float* G1B = G0B + cc_max * N * H;
    const float* g1c = g1 + c0 * N * C;
    // u = mask * (g1 W1)     [cc * N, H]
    if (compact) {
      // the compacted backward GEMM of the fit: active rows only (row N of every plane takes its padding stores)
      BackGemmArgs bg{};
      bg.G = g1c; bg.W = h->W[1]; bg.ldw = H; bg.U = U; bg.u_plane_stride = u_stride; bg.N = N; bg.K = C; bg.Nout = H;
      bg.planes = cc;
      bg.rows = h->ws.act_list.as<int32_t>(); bg.na_dev = h->ws.act_count.as<int32_t>();
      bg.mask_bits = h->fc.mask_bits[0].as<uint32_t>(); bg.mask_words = cdiv(H, 32);
      LGNN_CALL(launch_backgemm(bg, s));
    } else {
      GemmEpilogue ep;
      ep.hact = h->fc.hact_p[0]; ep.hact_ld = h->fc.hact_ld[0]; ep.act = h->act; ep.hact_row_mod = N;
      LGNN_CALL(launch_gemm(g1c, C, h->W[1], H, U, H, cc * N, C, H, ep, s));
    }
    // g0 = P^T u  (source rows with u = 0 are not gathered: their values are zeroed)
    SpmmArgs sa{};
    sa.rowptr = h->PT.rowptr; sa.col = h->PT.col; sa.val = val_act; sa.nrows = N;
    sa.in = U; sa.in_ld = H; sa.in_plane_stride = u_stride; sa.out = G0; sa.out_ld = H; sa.out_plane_stride = N * H;
    sa.width = H; sa.out_act = -1;
    if (H % 4 == 0 && H <= 256 && N * H * 4 < (int64_t(1) << 32) - (int64_t(1) << 14)) {
      hipLaunchKernelGGL(spmm256_skip_kernel, dim3(unsigned(cdiv(N, 4)), unsigned(cc)), dim3(256), 0, s, h->PT.rowptr, h->PT.col,
                         val_act, N, U, u_stride, H, G0);
      LGNN_HIP_CHECK(hipGetLastError());
    } else {
      LGNN_CALL(launch_spmm_ex(sa, cc, s));
    }
    // g0bar = 2 g0 Gamma_B0
    LGNN_CALL(sgemm_rm(s, cc * N, H, H, 2.f, G0, H, gamma_B0, H, 0.f, G0B, H));
    // gradP[(a,b)] += sum_c <u_c[a], g0bar_c[b]> and ubar = mask * (P g0bar) (overwrites u), both over the active rows only
    // (u, hence ubar's consumers, vanish elsewhere); candidates first: they read u before it is overwritten
    LGNN_CALL(launch_sddmm_coo(cand_a, cand_b, K, U, H, N * H, G0B, H, N * H, H, cc, h->ws.active.as<uint8_t>(), grad_cand, s));
    if (dense) {  // sum_c <u_c[a], g0bar_c[b]> over the active rows a (u vanishes elsewhere), all b
      DenseNtArgs dn;
      dn.out = dense; dn.ldo = N; dn.ncols = N; dn.nrows = N; dn.nrows_dev = h->ws.act_count.as<int32_t>();
      dn.orows = h->ws.act_list.as<int32_t>();
      dn.L = U; dn.l_ld = H; dn.l_stride = u_stride; dn.R = G0B; dn.r_ld = H; dn.r_stride = N * H; dn.width = H; dn.nplanes = cc;
      LGNN_CALL(launch_dense_nt(dn, s));
    }
    if (H % 4 == 0 && H <= 256) {
      // (candidate pairs reach g1bar at arbitrary rows, so ubar is then needed everywhere, not on the active rows only)
      const int32_t* rows = (K > 0 || dense) ? nullptr : h->ws.act_list.as<int32_t>();
      hipLaunchKernelGGL(sddmm_spmm_pm_kernel, dim3(unsigned(cdiv(N, 4)), unsigned(cc)), dim3(256), 0, s, h->P.rowptr, h->P.col,
                         h->P.val, rows, h->ws.act_count.as<int32_t>(), U, u_stride, G0B, N, H, h->fc.dact0.as<float>(), grad_P);
      LGNN_HIP_CHECK(hipGetLastError());
    } else {
      LGNN_CALL(launch_sddmm(h->P, N, h->ws.act_list.as<int32_t>(), h->ws.act_count.as<int32_t>(), U, H, N * H, G0B, H, N * H,
                             H, cc, grad_P, s));
      SpmmArgs sb{};
      sb.rowptr = h->P.rowptr; sb.col = h->P.col; sb.val = h->P.val; sb.nrows = N;
      sb.in = G0B; sb.in_ld = H; sb.in_plane_stride = N * H; sb.out = U; sb.out_ld = H; sb.out_plane_stride = N * H;
      sb.width = H; sb.out_act = -1;
      sb.hact = h->fc.hact_p[0]; sb.hact_ld = h->fc.hact_ld[0]; sb.act = h->act;
      LGNN_CALL(launch_spmm_ex(sb, cc, s));
    }
    // g1bar = ubar W1^T + 2 g1 Gamma_B1     [cc * N, C]
    if (compact) {  // planes of U are (N + 1) rows apart: one batched call, plane by plane
      rocblas_handle blas = static_cast<rocblas_handle>(blas_handle(s));
      LGNN_REQUIRE(blas != nullptr, "rocBLAS handle");
      const float one = 1.f, zero = 0.f;
      const rocblas_status st = rocblas_sgemm_strided_batched(
          blas, rocblas_operation_none, rocblas_operation_none, rocblas_int(C), rocblas_int(N), rocblas_int(H), &one,
          h->Wt[1].as<float>(), rocblas_int(C), 0, U, rocblas_int(H), rocblas_stride(u_stride), &zero, G1B, rocblas_int(C),
          rocblas_stride(N * C), rocblas_int(cc));
      if (st != rocblas_status_success) { set_error("rocblas_sgemm_strided_batched failed"); return 3; }
    } else {
      LGNN_CALL(sgemm_rm(s, cc * N, C, H, 1.f, U, H, h->Wt[1].as<float>(), C, 0.f, G1B, C));
    }
    LGNN_CALL(sgemm_rm(s, cc * N, C, C, 2.f, g1c, C, gamma_B1, C, 1.f, G1B, C));
    // gradP[(a,b)] += sum_c <G_c[a], g1bar_c[b]> for the batch rows a;  Vbar = (P g1bar)[batch rows]
    // (the dense route takes the stored entries' term on the full grid below)
    LGNN_CALL(launch_seed_sddmm(h, idx, M, G1B, c0, cc, dense ? nullptr : grad_P, cand_a, cand_b, K, grad_cand, s));
    if (dense) {  // sum_c <G_c[a], g1bar_c[b]>: the seed rows of the batch nodes a, all b
      DenseNtArgs dn;
      dn.out = dense; dn.ldo = N; dn.ncols = N; dn.nrows = M; dn.nrows_dev = first_rows + 2 * M;
      dn.orows = first_rows; dn.lrows = first_rows + M;
      dn.L = h->ws.seeds.as<float>() + c0 * C; dn.l_ld = CC; dn.l_stride = C;
      dn.R = G1B; dn.r_ld = C; dn.r_stride = N * C; dn.width = C; dn.nplanes = cc;
      LGNN_CALL(launch_dense_nt(dn, s));
    }
    LGNN_CALL(launch_seed_gather(h, idx, M, G1B, c0, cc, vbar, s));
  }
  LGNN_CALL(launch_seed_adjoint(h, idx, y, M, vbar, fork_exact, loss_scale, out_bar, s));
  LGNN_CALL(batch_epilogue(h, idx, M, s));
  return 0;
}

}  // namespace lgnn
