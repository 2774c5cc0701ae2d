// tests/devprim/devprim.hip — TEST INFRASTRUCTURE: extern "C" entry points of the device-primitive test library (tests/_build/libqm_devprim.so).
// Each takes HOST pointers, allocates, copies in (outputs too: the caller's canaries travel with them), launches ONE short kernel of devprim_kernels.h,
// copies the outputs back, frees, and returns the hipError_t as an int (0 = success).  tests/emu_prim/emu_prim_api.cpp compiles this same file for the
// host emulator with DEVPRIM_EMU defined: malloc / memcpy / emu::launch in place of the runtime calls.  Never linked into libqmhip.so.
#include "devprim_kernels.h"
#include <cstring>

#ifdef DEVPRIM_EMU
static int dp_malloc(void** p, size_t n) { *p = malloc(n ? n : 8); return *p ? 0 : 2; }
static int dp_in(void* d, const void* h, size_t n) { memcpy(d, h, n); return 0; }
static int dp_out(void* h, const void* d, size_t n) { memcpy(h, d, n); return 0; }
static void dp_free(void* p) { free(p); }
static int dp_sync() { return 0; }
#define DP_LAUNCH(kernel, grid, block, smem, args) emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); })
#else
static int dp_malloc(void** p, size_t n) { return (int)hipMalloc(p, n ? n : 8); }
static int dp_in(void* d, const void* h, size_t n) { return (int)hipMemcpy(d, h, n, hipMemcpyHostToDevice); }
static int dp_out(void* h, const void* d, size_t n) { return (int)hipMemcpy(h, d, n, hipMemcpyDeviceToHost); }
static void dp_free(void* p) { (void)hipFree(p); }
static int dp_sync() { const int e = (int)hipDeviceSynchronize(); const int l = (int)hipGetLastError(); return e ? e : l; }
#define DP_LAUNCH(kernel, grid, block, smem, args) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), smem, 0, args)
#endif

static int g_err = 0;
static void dp_note(int e) { if (e && !g_err) g_err = e; }
// a host array mirrored on the device for the length of one call
struct DpBuf {
  void* d = nullptr; void* host; size_t bytes;
  DpBuf(const void* h, size_t b) : host((void*)h), bytes(b) { dp_note(dp_malloc(&d, b)); if (!g_err) dp_note(dp_in(d, h, b)); }
  ~DpBuf() { if (d) dp_free(d); }
  void back() { if (!g_err) dp_note(dp_out(host, d, bytes)); }
  template <class T> T* as() const { return (T*)d; }
};
#define DP_BEGIN() g_err = 0
#define DP_RUN(kernel, grid, block, smem, args) do { if (!g_err) { DP_LAUNCH(kernel, grid, block, smem, args); dp_note(dp_sync()); } } while (0)

extern "C" {
int dp_scalar(int op, int n, int nin, int nout, const double* in, double* out) {
  DP_BEGIN(); if (op < 0 || op >= DP_N_SCALAR || n <= 0) return -1;
  DpBuf bi(in, (size_t)nin * n * 8), bo(out, (size_t)nout * n * 8);
  DpScalarArgs a; a.op = op; a.n = n; a.in = bi.as<double>(); a.out = bo.as<double>();
  DP_RUN(dp_scalar_kernel, (n + 255) / 256, 256, 0, a); bo.back(); return g_err;
}
// nblocks blocks of 256 threads; old / in / out: [nblocks * 256]
int dp_wave(int op, int src, int nblocks, const double* old, const double* in, double* out) {
  DP_BEGIN(); if (op < 0 || op >= DP_N_WAVE || src < 0 || src > 63 || nblocks <= 0) return -1;
  const size_t b = (size_t)nblocks * 256 * 8; DpBuf bo(old, b), bi(in, b), br(out, b);
  DpWaveArgs a; a.op = op; a.src = src; a.old = bo.as<double>(); a.in = bi.as<double>(); a.out = br.as<double>();
  DP_RUN(dp_wave_kernel, nblocks, 256, 0, a); br.back(); return g_err;
}
// src: [nrows][W]; lanes, vals: [64 nblocks][W]; dst: ndst doubles, row r at dst_off + r * stride; mask: [nblocks] (the caller clears the bits of rows >= nrows)
int dp_rows(int W, long nrows, int nblocks, long stride, const double* src, double* lanes, const double* vals, double* dst, long ndst, long dst_off, const unsigned long long* mask) {
  DP_BEGIN(); if (nblocks <= 0 || stride < W || dst_off < 0 || dst_off + ((long)64 * nblocks - 1) * stride + W > ndst) return -1;
  DpBuf bs(src, (size_t)(nrows > 0 ? nrows : 1) * W * 8), bl(lanes, (size_t)nblocks * 64 * W * 8), bv(vals, (size_t)nblocks * 64 * W * 8), bd(dst, (size_t)ndst * 8), bm(mask, (size_t)nblocks * 8);
  DpRowsArgs a; a.nrows = (size_t)nrows; a.stride = (size_t)stride; a.src = bs.as<double>(); a.lanes = bl.as<double>(); a.vals = bv.as<double>(); a.dst = bd.as<double>() + dst_off; a.mask = bm.as<unsigned long long>();
  void (*k)(DpRowsArgs) = nullptr;
  switch (W) { case 1: k = dp_rows_kernel<1>; break; case 3: k = dp_rows_kernel<3>; break; case 8: k = dp_rows_kernel<8>; break; case 30: k = dp_rows_kernel<30>; break; default: return -1; }
  DP_RUN(k, nblocks, 64, QM_ROWS_LDS(W) * 8, a); bl.back(); bd.back(); return g_err;
}
// A, B: whole tile images [32][QM_LD]; C: [32][32] doubles, calls: [32][32] ints (both arrive initialised by the caller)
int dp_wg_gemm(int ta, int tb, int block, const double* A, const double* B, int mt, int nt, int ks0, int ks1, double* C, int* calls) {
  DP_BEGIN(); if ((block != 64 && block != 128 && block != 256) || mt < 1 || mt > 2 || nt < 1 || nt > 2 || ks0 < 0 || ks1 > 8) return -1;
  DpBuf bA(A, QM_TILE * 8), bB(B, QM_TILE * 8), bC(C, 1024 * 8), bn(calls, 1024 * 4);
  DpGemmArgs a; a.A = bA.as<double>(); a.B = bB.as<double>(); a.mt = mt; a.nt = nt; a.ks0 = ks0; a.ks1 = ks1; a.C = bC.as<double>(); a.calls = bn.as<int>();
  void (*k)(DpGemmArgs) = ta ? (tb ? dp_wg_gemm_kernel<true, true> : dp_wg_gemm_kernel<true, false>) : (tb ? dp_wg_gemm_kernel<false, true> : dp_wg_gemm_kernel<false, false>);
  DP_RUN(k, 1, block, 2 * QM_TILE * 8, a); bC.back(); bn.back(); return g_err;
}
// src: nsrc doubles; regs: [16][64]; dst: ndst doubles, the matrix at dst_off with leading dimension ldd
int dp_frag(int tr, int stream, int tile, const double* src, long nsrc, int ld, int rows, int cols, double* regs, double* dst, long ndst, long dst_off, int ldd) {
  DP_BEGIN();
  const long need = tile ? 31L * ld + 32 : (tr ? (long)(cols - 1) * ld + rows : (long)(rows - 1) * ld + cols);
  if (rows < 1 || cols < 1 || rows > 32 || cols > 32 || need > nsrc || dst_off < 0 || dst_off + (long)(rows - 1) * ldd + cols > ndst || cols > ldd) return -1;
  DpBuf bs(src, (size_t)nsrc * 8), br(regs, 16 * 64 * 8), bd(dst, (size_t)ndst * 8);
  DpFragArgs a; a.src = bs.as<double>(); a.ld = ld; a.rows = rows; a.cols = cols; a.tile = tile; a.regs = br.as<double>(); a.dst = bd.as<double>() + dst_off; a.ldd = ldd;
  void (*k)(DpFragArgs) = tr ? (stream ? dp_frag_kernel<true, true> : dp_frag_kernel<true, false>) : (stream ? dp_frag_kernel<false, true> : dp_frag_kernel<false, false>);
  DP_RUN(k, 1, 64, 0, a); br.back(); bd.back(); return g_err;
}
// Z: [16 kt][16 it], Y: [16 kt][16 jt], P: [16 it][16 jt] (in and out)
int dp_gemm_tn(int kt, int it, int jt, const double* Z, const double* Y, double* P, int k0, int k1, int neg) {
  DP_BEGIN();
  DpBuf bZ(Z, (size_t)256 * kt * it * 8), bY(Y, (size_t)256 * kt * jt * 8), bP(P, (size_t)256 * it * jt * 8);
  DpGemmTnArgs a; a.Z = bZ.as<double>(); a.Y = bY.as<double>(); a.P = bP.as<double>(); a.k0 = k0; a.k1 = k1; a.neg = neg;
  void (*k)(DpGemmTnArgs) = nullptr; const int shape = 100 * kt + 10 * it + jt;
  switch (shape) {      // every shape the library instantiates (tests/devprim_cases.py GEMM_TN_SHAPES)
    case 222: k = dp_gemm_tn_kernel<2, 2, 2>; break; case 221: k = dp_gemm_tn_kernel<2, 2, 1>; break; case 212: k = dp_gemm_tn_kernel<2, 1, 2>; break; case 211: k = dp_gemm_tn_kernel<2, 1, 1>; break;
    case 112: k = dp_gemm_tn_kernel<1, 1, 2>; break; case 111: k = dp_gemm_tn_kernel<1, 1, 1>; break; case 122: k = dp_gemm_tn_kernel<1, 2, 2>; break; case 322: k = dp_gemm_tn_kernel<3, 2, 2>; break; default: return -1;
  }
  DP_RUN(k, 1, 64, 0, a); bP.back(); return g_err;
}
// mode 0: the 4 KB segment at g + g_off doubles -> LDS double DP_DMA_AT, by qm_dma16_at<0 / 1024 / 2048 / 3072>; mode 1: the 1 KB chunk at g + g_off -> LDS double lds_at, by qm_dma16.
// out: the whole LDS image, DP_DMA_LDS doubles
int dp_dma(int mode, const double* g, long ng, long g_off, int lds_at, double fill, double* out) {
  DP_BEGIN(); const long len = mode == 0 ? 512 : 128;
  if (g_off < 0 || (g_off & 1) || g_off + len > ng || (lds_at & 1) || lds_at < 0 || lds_at + 128 > DP_DMA_LDS) return -1;
  DpBuf bg(g, (size_t)ng * 8), bo(out, DP_DMA_LDS * 8);
  DpDmaArgs a; a.g = bg.as<double>() + g_off; a.mode = mode; a.lds_at = lds_at; a.fill = fill; a.out = bo.as<double>();
  DP_RUN(dp_dma_kernel, 1, 64, DP_DMA_LDS * 8, a); bo.back(); return g_err;
}
// src: [rows][sld]; x: [32]; tile: [32][QM_LD]; dst: ndst doubles, the matrix at dst_off with leading dimension dld; rowdot, coldot: [32]; m3: 24 doubles in, m3out: 24 out
int dp_dense(int block, const double* src, int rows, int cols, int sld, int dld, const double* x, double fill, double* tile, double* dst, long ndst, long dst_off, double* rowdot, double* coldot, const double* m3, double* m3out) {
  DP_BEGIN(); if (rows < 1 || cols < 1 || rows > 32 || cols > 32 || cols > sld || cols > dld || block < 32 || dst_off < 0 || dst_off + (long)(rows - 1) * dld + cols > ndst) return -1;
  DpBuf bs(src, (size_t)rows * sld * 8), bx(x, 32 * 8), bt(tile, QM_TILE * 8), bd(dst, (size_t)ndst * 8), br(rowdot, 32 * 8), bc(coldot, 32 * 8), bm(m3, 24 * 8), bo(m3out, 24 * 8);
  DpDenseArgs a; a.src = bs.as<double>(); a.rows = rows; a.cols = cols; a.sld = sld; a.dld = dld; a.x = bx.as<double>(); a.fill = fill; a.tile = bt.as<double>(); a.dst = bd.as<double>() + dst_off;
  a.rowdot = br.as<double>(); a.coldot = bc.as<double>(); a.m3 = bm.as<double>(); a.m3out = bo.as<double>();
  DP_RUN(dp_dense_kernel, 1, block, QM_TILE * 8, a); bt.back(); bd.back(); br.back(); bc.back(); bo.back(); return g_err;
}
// name of the device the kernels ran on ("emulator" on the host build)
int dp_device_name(char* buf, int n) {
#ifdef DEVPRIM_EMU
  strncpy(buf, "emulator", n); buf[n - 1] = 0; return 0;
#else
  hipDeviceProp_t p; const int e = (int)hipGetDeviceProperties(&p, 0); if (e) return e; strncpy(buf, p.name, n); buf[n - 1] = 0; return 0;
#endif
}
}
