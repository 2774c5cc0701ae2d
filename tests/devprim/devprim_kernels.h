// tests/devprim/devprim_kernels.h — TEST INFRASTRUCTURE: thin __global__ wrappers over the shared device primitives of qm_dev_common.h, one
// primitive call per thread / wave / workgroup and a store of what it returned.  No arithmetic of their own: whatever a test sees is the primitive's.
// Compiled twice: by hipcc for gfx950 with the product's flags (tests/devprim/devprim.hip -> tests/_build/libqm_devprim.so) and for the host through
// tests/emu/hip_emu.h (tests/emu_prim).  Never linked into libqmhip.so.
#pragma once
#include "../../qm_control_amd/csrc/kernels/qm_dev_common.h"

extern __shared__ double qm_smem[];

// ---- (a) scalar maps: element i of every input array -> element i of every output array; arrays are [k][n] ----
enum { DP_RCP, DP_RSQ, DP_FRCP, DP_LOG, DP_SINCOS, DP_RECIP, DP_RSQRT, DP_RSQRT_N2, DP_GIVENS, DP_HOUSE, DP_BARRIER_VAL, DP_BARRIER_D12,
       DP_ROT_ZYX_FAST, DP_ROT_ZYX_LIB, DP_EULER_E_FAST, DP_ROT_AXIS_FAST, DP_N_SCALAR };
struct DpScalarArgs { int op, n; const double* in; double* out; };
__global__ void dp_scalar_kernel(DpScalarArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, n = a.n; if (i >= n) return;
  const double* x = a.in + i; double* y = a.out + i;
  switch (a.op) {
    case DP_RCP: y[0] = __builtin_amdgcn_rcp(x[0]); break;
    case DP_RSQ: y[0] = __builtin_amdgcn_rsq(x[0]); break;
    case DP_FRCP: y[0] = qm_frcp(x[0]); break;
    case DP_LOG: y[0] = qm_log(x[0]); break;
    case DP_SINCOS: { double s, c; qm_sincos(x[0], s, c); y[0] = s; y[n] = c; break; }
    case DP_RECIP: y[0] = qm_recip(x[0]); break;
    case DP_RSQRT: y[0] = qm_rsqrt(x[0]); break;
    case DP_RSQRT_N2: y[0] = qm_rsqrt_n2(x[0]); break;
    case DP_GIVENS: { double c, s; qm_givens(x[0], x[n], c, s); y[0] = c; y[n] = s; break; }
    case DP_HOUSE: { double al, vk, b2; const bool ok = qm_house_scalars(x[0], x[n], al, vk, b2); y[0] = al; y[n] = vk; y[2 * n] = b2; y[3 * n] = ok ? 1.0 : 0.0; break; }
    case DP_BARRIER_VAL: y[0] = barrier_val(x[0], x[n], x[2 * n]); break;
    case DP_BARRIER_D12: { double d1, d2; barrier_d12(x[0], x[n], x[2 * n], d1, d2); y[0] = d1; y[n] = d2; break; }
    case DP_ROT_ZYX_FAST: { double R[9]; rot_zyx<true>(x[0], x[n], x[2 * n], R); for (int k = 0; k < 9; ++k) y[k * n] = R[k]; break; }
    case DP_ROT_ZYX_LIB: { double R[9]; rot_zyx<false>(x[0], x[n], x[2 * n], R); for (int k = 0; k < 9; ++k) y[k * n] = R[k]; break; }
    case DP_EULER_E_FAST: { double E[9]; euler_E<true>(x[0], x[n], E); for (int k = 0; k < 9; ++k) y[k * n] = E[k]; break; }
    case DP_ROT_AXIS_FAST: { const double ax[3] = {x[0], x[n], x[2 * n]}; double R[9]; rot_axis_angle<true>(ax, x[3 * n], R); for (int k = 0; k < 9; ++k) y[k * n] = R[k]; break; }
    default: break;
  }
}

// ---- (b) wave reductions, broadcasts and the single DPP steps; every lane's result is stored.  Called under a FULL exec mask, as the kernels do:
// the launch covers whole 256-thread blocks and no lane leaves before the call ----
enum { DP_WAVE_SUM, DP_WAVE_MAX, DP_BCAST, DP_DPP0_111, DP_DPP0_112, DP_DPP0_114, DP_DPP0_118, DP_DPP_142_A, DP_DPP_143_C,
       DP_DPP_111_F, DP_DPP_112_F, DP_DPP_114_F, DP_DPP_118_F, DP_N_WAVE };
struct DpWaveArgs { int op, src; const double* old; const double* in; double* out; };
__global__ void dp_wave_kernel(DpWaveArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x; const double v = a.in[i], o = a.old[i]; double r = 0.0;
  switch (a.op) {      // (wave-uniform)
    case DP_WAVE_SUM: r = qm_wave_sum(v); break;
    case DP_WAVE_MAX: r = qm_wave_max(v); break;
    case DP_BCAST: r = qm_bcast(v, a.src); break;
    case DP_DPP0_111: r = qm_dpp0<0x111>(v); break;
    case DP_DPP0_112: r = qm_dpp0<0x112>(v); break;
    case DP_DPP0_114: r = qm_dpp0<0x114>(v); break;
    case DP_DPP0_118: r = qm_dpp0<0x118>(v); break;
    case DP_DPP_142_A: r = qm_dpp<0x142, 0xa>(o, v); break;
    case DP_DPP_143_C: r = qm_dpp<0x143, 0xc>(o, v); break;
    case DP_DPP_111_F: r = qm_dpp<0x111, 0xf>(o, v); break;
    case DP_DPP_112_F: r = qm_dpp<0x112, 0xf>(o, v); break;
    case DP_DPP_114_F: r = qm_dpp<0x114, 0xf>(o, v); break;
    case DP_DPP_118_F: r = qm_dpp<0x118, 0xf>(o, v); break;
    default: break;
  }
  a.out[i] = r;
}

// ---- (c) qm_rows_gather / qm_rows_scatter: one wave per block, block b takes the rows from row0 = 64 b ----
struct DpRowsArgs { size_t nrows, stride; const double* src; double* lanes; const double* vals; double* dst; const unsigned long long* mask; };
template <int W> __global__ void dp_rows_kernel(DpRowsArgs a) {
  const int l = threadIdx.x; const size_t row0 = (size_t)64 * blockIdx.x; const double* src = a.src; double v[W];
  qm_rows_gather<W>(qm_smem, row0, a.nrows, l, v, [src](size_t r, int c) { return src[r * W + c]; });
  for (int q = 0; q < W; ++q) a.lanes[(row0 + l) * W + q] = v[q];
  for (int q = 0; q < W; ++q) v[q] = a.vals[(row0 + l) * W + q];
  qm_rows_scatter<W>(qm_smem, a.dst, a.stride, row0, a.mask[blockIdx.x], l, v);
}

// ---- (d) wg_gemm: the two operand tiles arrive as whole 32 x QM_LD images (sentinels included), every output goes through the epilogue ----
struct DpGemmArgs { const double* A; const double* B; int mt, nt, ks0, ks1; double* C; int* calls; };
template <bool TA, bool TB> __global__ void dp_wg_gemm_kernel(DpGemmArgs a) {
  double* At = qm_smem; double* Bt = qm_smem + QM_TILE;
  for (int i = threadIdx.x; i < QM_TILE; i += blockDim.x) { At[i] = a.A[i]; Bt[i] = a.B[i]; }
  __syncthreads();
  double* C = a.C; int* calls = a.calls;
  wg_gemm<TA, TB>(At, Bt, a.mt, a.nt, a.ks0, a.ks1, [C, calls](int row, int col, double v) { C[row * 32 + col] = v; atomicAdd(calls + row * 32 + col, 1); });
}

// ---- (e) register fragments (one wave) ----
// load (bounded or whole-tile) -> the registers as they are -> store
struct DpFragArgs { const double* src; int ld, rows, cols, tile; double* regs; double* dst; int ldd; };
template <bool TR, bool STREAM> __global__ void dp_frag_kernel(DpFragArgs a) {
  qm_d4 T[2][2];
  if (a.tile) qm_frag_load_tile<2, 2, TR>(T, a.src, a.ld); else qm_frag_load<2, 2, TR>(T, a.src, a.ld, a.rows, a.cols);
  for (int I = 0; I < 2; ++I) for (int J = 0; J < 2; ++J) for (int r = 0; r < 4; ++r) a.regs[((2 * I + J) * 4 + r) * 64 + threadIdx.x] = T[I][J][r];
  qm_frag_store<2, 2, STREAM>(T, a.dst, a.ldd, a.rows, a.cols);
}
// P (16 IT x 16 JT) += (neg ? −1 : 1) Zᵀ Y over k-steps [k0, k1); Z is 16 KT x 16 IT, Y is 16 KT x 16 JT, all row-major and dense
struct DpGemmTnArgs { const double* Z; const double* Y; double* P; int k0, k1, neg; };
template <int KT, int IT, int JT> __global__ void dp_gemm_tn_kernel(DpGemmTnArgs a) {
  qm_d4 Z[KT][IT], Y[KT][JT], P[IT][JT];
  qm_frag_load<KT, IT, false>(Z, a.Z, 16 * IT, 16 * KT, 16 * IT); qm_frag_load<KT, JT, false>(Y, a.Y, 16 * JT, 16 * KT, 16 * JT); qm_frag_load<IT, JT, false>(P, a.P, 16 * JT, 16 * IT, 16 * JT);
  qm_gemm_tn<KT, IT, JT>(Z, Y, P, a.k0, a.k1, a.neg != 0);
  qm_frag_store<IT, JT>(P, a.P, 16 * JT, 16 * IT, 16 * JT);
}

// ---- (f) global -> LDS copy (one wave): the kernel fills DP_DMA_LDS doubles of LDS with `fill`, copies, waits, and writes the whole LDS image back with plain stores ----
#define DP_DMA_LDS 1024      /* 8 KB: the 4 KB segment lands at double 128, 3 KB of pre-filled LDS stay behind it */
#define DP_DMA_AT 128
struct DpDmaArgs { const double* g; int mode, lds_at; double fill; double* out; };
__global__ void dp_dma_kernel(DpDmaArgs a) {
  const int l = threadIdx.x;
  for (int i = l; i < DP_DMA_LDS; i += 64) qm_smem[i] = a.fill;
  qm_wave_sync();
  if (a.mode == 0) {      // a 4 KB segment, contiguous on both sides: one global base, one LDS base, four immediate offsets
    const char* g = (const char*)a.g + 16 * l; const qm_lds_ptr l3 = qm_lds(qm_smem + DP_DMA_AT);
    qm_dma16_at<0>(g, l3); qm_dma16_at<1024>(g, l3); qm_dma16_at<2048>(g, l3); qm_dma16_at<3072>(g, l3);
  } else qm_dma16(a.g + 2 * l, qm_smem + a.lds_at);      // one 1 KB chunk
  qm_dma_wait();
  for (int i = l; i < DP_DMA_LDS; i += 64) a.out[i] = qm_smem[i];
}

// ---- (g) small dense helpers: a rows x cols matrix through tile_load / tile_store (the tile image is returned too), a row and a column product per thread,
// and the 3 x 3 helpers on thread 0 ----
struct DpDenseArgs { const double* src; int rows, cols, sld, dld; const double* x; double fill; double* tile; double* dst; double* rowdot; double* coldot; const double* m3; double* m3out; };
__global__ void dp_dense_kernel(DpDenseArgs a) {
  double* T = qm_smem;
  for (int i = threadIdx.x; i < QM_TILE; i += blockDim.x) T[i] = a.fill;
  __syncthreads();
  tile_load(T, a.src, a.rows, a.cols, a.sld);
  __syncthreads();
  for (int i = threadIdx.x; i < QM_TILE; i += blockDim.x) a.tile[i] = T[i];
  tile_store(T, a.dst, a.rows, a.cols, a.dld);
  if ((int)threadIdx.x < a.rows) a.rowdot[threadIdx.x] = tile_row_dot(T, threadIdx.x, a.x, a.cols);
  if ((int)threadIdx.x < a.cols) a.coldot[threadIdx.x] = tile_col_dot(T, threadIdx.x, a.x, a.rows);
  if (threadIdx.x == 0) {      // m3: A (9), B (9), v (3), w (3)  ->  A B (9), A v (3), A⁻¹ (9), v x w (3)
    m3_mul(a.m3, a.m3 + 9, a.m3out); m3_mulv(a.m3, a.m3 + 18, a.m3out + 9); m3_inv(a.m3, a.m3out + 12); v3_cross(a.m3 + 18, a.m3 + 21, a.m3out + 21);
  }
}
