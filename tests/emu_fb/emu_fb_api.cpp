// tests/emu_fb/emu_fb_api.cpp — TEST INFRASTRUCTURE: the feedback-policy kernels (qm_policy_fb_kernel, qm_feedback_gather_kernel; csrc/kernels/k_policy.h) on the host
// emulator, launched through the pipeline calls the product uses (QmWbcPipeline::policy_eval_feedback / feedback_gather), on caller-owned solver buffers.
// Never linked into the product.
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"

struct EmuFbBackend {
  int launches = 0; const void* last = nullptr;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { ++launches; last = (const void*)kernel; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
  void* alloc(size_t n) { return malloc(n ? n : 8); }
  void free(void* p) { ::free(p); }
  void zero(void* p, size_t n) { memset(p, 0, n); }
  void to_device(void* d, const void* s, size_t n) { memcpy(d, s, n); }
  void to_host(void* d, const void* s, size_t n) { memcpy(d, s, n); }
};

static QmMpcBuffers buffers(int Bmax, int nmax, int nev, const int* n_nodes, const double* node_t, const int* node_ev, const double* xs, const double* us, const double* ev, const int* modes, const double* stage) {
  QmMpcBuffers d; d.Bmax = Bmax; d.nmax = nmax; d.nev = nev; d.n_nodes = (int*)n_nodes; d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.xs = (double*)xs; d.us = (double*)us;
  d.ev = (double*)ev; d.modes = (int*)modes; d.stage = (double*)stage; return d;
}

extern "C" {
// offsets of the stage-record fields the feedback kernels read
int emu_fb_layout(int which) { const int v[] = {SR_SIZE, SR_PP, SR_PX, SR_SWG, SR_MODEF, SR_SCAL}; return which >= 0 && which < 6 ? v[which] : -1; }
// QmWbcPipeline::policy_eval_feedback: node-major solver buffers [nmax][B][k], stage records [B][nmax][SR_SIZE]; x null: the feed-forward policy.
// Returns 1 when the launch was qm_policy_fb_kernel, 0 for qm_policy_kernel
int emu_fb_policy(int B, int nmax, int nev, const int* n_nodes, const double* node_t, const int* node_ev, const double* xs, const double* us, const double* ev, const int* modes,
                  const double* stage, const double* t, const double* x, double* x_des, double* u_des, int* mode) {
  EmuFbBackend bk; QmWbcPipeline<EmuFbBackend> wbc(bk); wbc.allocate(B);
  const QmMpcBuffers d = buffers(B, nmax, nev, n_nodes, node_t, node_ev, xs, us, ev, modes, stage);
  wbc.policy_eval_feedback(d, B, t, x);
  memcpy(x_des, wbc.w.x_des, (size_t)B * 30 * 8); memcpy(u_des, wbc.w.u_des, (size_t)B * 30 * 8); memcpy(mode, wbc.w.mode, (size_t)B * 4);
  const int fb = bk.last == (const void*)qm_policy_fb_kernel; wbc.release(); return fb;
}
// QmWbcPipeline::feedback_gather for the instances b0 .. b0 + nb - 1: gain [nb][nmax][30][30], uff [nb][nmax][30]
void emu_fb_gather(int B, int nmax, const int* n_nodes, const int* node_ev, const double* xs, const double* us, const double* stage, int b0, int nb, double* gain, double* uff) {
  EmuFbBackend bk; QmWbcPipeline<EmuFbBackend> wbc(bk);
  const QmMpcBuffers d = buffers(B, nmax, 0, n_nodes, nullptr, node_ev, xs, us, nullptr, nullptr, stage);
  wbc.feedback_gather(d, B, b0, nb, gain, uff);
}
}
