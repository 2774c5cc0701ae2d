// tests/emu_plan/emu_plan_api.cpp — TEST INFRASTRUCTURE: the task-space plan kernels (qm_plan_nodes_kernel, qm_plan_states_kernel, qm_plan_footholds_kernel;
// csrc/kernels/k_plan.h) on the host emulator, launched through the pipeline calls the product uses (QmPlanPipeline::task_space / footholds / eval).
// Never linked into the product.
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_plan_pipeline.h"

// one queue: copies are memcpy, the event orders nothing (the data dependencies are the launch order)
struct EmuPlanBackend {
  int launches = 0, waits = 0;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { if (grid <= 0) return; ++launches; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
  void* alloc(size_t n) { void* p = nullptr; if (posix_memalign(&p, 64, n ? n : 8)) return nullptr; memset(p, 0xff, n ? n : 8); return p; }      // a fresh buffer holds NaNs (ints: -1): a word never written shows
  void free(void* p) { ::free(p); }
  void zero(void* p, size_t n) { memset(p, 0, n); }
  void* alloc_pinned(size_t n) { return alloc(n); }
  void free_pinned(void* p) { ::free(p); }
  void* io_event() { return malloc(8); }
  void io_event_free(void* e) { ::free(e); }
  void stream_select(int) {}
  void copy_in(void* d, const void* s, size_t n, int) { memcpy(d, s, n); }
  void copy_back(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); }
  void io_wait(void*) { ++waits; }
};

extern "C" {
int emu_plan_layout(int which) {
  const int v[] = {QM_PLAN_BYTES, QM_PLAN_WORDS, QM_FOOTHOLD_BYTES, PT_TIME, PT_MODE, PT_BASE_POS, PT_BASE_ZYX, PT_FOOT_POS, PT_FOOT_VEL, PT_FOOT_FORCE, PT_EE_POS, PT_EE_QUAT, PT_EE_ERR, PT_COP, PT_SPARE, QM_PLAN_LDS_BYTES,
                   (int)sizeof(qmhip_plan_record), (int)sizeof(qmhip_foothold)};
  return which >= 0 && which < 18 ? v[which] : -1;
}
// caller-owned solver buffers of a batch of B (node-major [nmax][B][k], strided by B as after a solve of B instances) -> records [B][nmax], node counts, footholds.
// Returns launches * 100 + host waits of the three calls together
int emu_plan_solution(const double* mb, int B, int nmax, int nev, const int* n_nodes, const double* node_t, const int* node_ev, const int* node_mode, const double* xs, const double* us, const double* eeref,
                      const double* ev, const int* modes, void* rec, int* nn, int cap, void* footholds, int* count) {
  EmuPlanBackend bk; QmPlanPipeline<EmuPlanBackend> plan(bk);
  QmMpcBuffers d; d.Bmax = B; d.nmax = nmax; d.nev = nev; d.mb = (double*)mb; d.n_nodes = (int*)n_nodes; d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.node_mode = (int*)node_mode;
  d.xs = (double*)xs; d.us = (double*)us; d.eeref = (double*)eeref; d.ev = (double*)ev; d.modes = (int*)modes;
  if (rec) plan.task_space(d, B, rec, nn);
  if (count) plan.footholds(d, B, cap, footholds, count);
  plan.release(); return bk.launches * 100 + bk.waits;
}
// caller-supplied rows (u, ee may be null)
void emu_plan_eval(const double* mb, int R, const double* x, const double* u, const int* mode, const double* ee, void* rec) {
  EmuPlanBackend bk; QmPlanPipeline<EmuPlanBackend> plan(bk); plan.eval(mb, R, x, u, mode, ee, rec); plan.release();
}
}
