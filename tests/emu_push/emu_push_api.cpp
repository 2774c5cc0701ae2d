// tests/emu_push/emu_push_api.cpp — TEST INFRASTRUCTURE: the plant with scheduled external wrenches (csrc/kernels/k_sim.h: qm_sim_push_kernel; csrc/host/qm_sim_pipeline.h) on the
// host emulator, in one context with the two device loops (qm_closed_loop_sim_ticks / _pipelined) that step it, for pytest through ctypes.  Never linked into the product.
#include <cstddef>
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_sim_pipeline.h"

struct EmuPushBackend {
  int plain = 0, pushed = 0;      // launches of qm_sim_kernel / qm_sim_push_kernel
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) {
    if ((const void*)kernel == (const void*)qm_sim_kernel) ++plain;
    if ((const void*)kernel == (const void*)qm_sim_push_kernel) ++pushed;
    emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); });
  }
  void* alloc(size_t n) { return malloc(n ? n : 8); }
  void free(void* p) { ::free(p); }
  void zero(void* p, size_t n) { memset(p, 0, n); }
  void to_device(void* d, const void* s, size_t n) { memcpy(d, s, n); }
  void to_host(void* d, const void* s, size_t n) { memcpy(d, s, n); }
  void sync() {}
  void* alloc_mapped(size_t n, void** host_view) { void* p = malloc(n ? n : 8); *host_view = p; return p; }
  void free_mapped(void* p) { ::free(p); }
  void wait_flag(volatile int*, int) {}
  void wbc_inputs_next() {}
  void stream_select(int) {}
  void stream_order(int, int) {}
  void copy_dd(void* d, const void* s, size_t n) { memcpy(d, s, n); }
};

struct EmuPushCtx {
  EmuPushBackend bk; QmMpcPipeline<EmuPushBackend> mpc; QmWbcPipeline<EmuPushBackend> wbc; QmSimPipeline<EmuPushBackend> sim; long sim_ticks = 0; int Bmax = 0; int wbc_only = 0;
  EmuPushCtx() : mpc(bk), wbc(bk), sim(bk) {}
};
enum { OK = 0, ERR_ARG = -1, ERR_STATE = -5 };      // QMHIP_OK, QMHIP_ERR_ARG, QMHIP_ERR_STATE (include/qmhip.h)

extern "C" {
int emu_push_bytes() { return (int)sizeof(qmhip_push); }
int emu_push_offset(int k) {
#define O(f) offsetof(qmhip_push, f)
  const size_t o[] = {O(t_on), O(t_off), O(base_force), O(base_torque), O(ee_force), O(spare)};
#undef O
  return k >= 0 && k < (int)(sizeof(o) / sizeof(o[0])) ? (int)o[k] : -1;
}
void* emu_push_create(const double* mb, const double* st, int Bmax, int nmax, int nref, int nev) {
  EmuPushCtx* c = new EmuPushCtx(); c->Bmax = Bmax; c->mpc.allocate(mb, st, Bmax, nmax, nref, nev, false); c->wbc.allocate(Bmax); return c;      // (the plant allocates on demand, as in the product)
}
void emu_push_destroy(void* h) { EmuPushCtx* c = (EmuPushCtx*)h; c->mpc.release(); c->wbc.release(); c->sim.release(); delete c; }
void emu_push_set_wbc_only(void* h, int on) { ((EmuPushCtx*)h)->wbc_only = on; }      // stands for a context of qmhip_create_wbc_context
void emu_push_upload(void* h, int B, const double* t0, const double* x0, const double* ref_t, const double* ref_x, const double* ev, const int* modes) { ((EmuPushCtx*)h)->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); }
void emu_push_counts(void* h, int* plain, int* pushed) { EmuPushCtx* c = (EmuPushCtx*)h; *plain = c->bk.plain; *pushed = c->bk.pushed; }
// ---- what qmhip_sim_reset / _set_command / _step / _get_state and the two loops do ----
void emu_push_sim_reset(void* h, int B, const double* q, const double* v, const double* time) {
  EmuPushCtx* c = (EmuPushCtx*)h; c->sim.allocate(c->Bmax); c->sim.reset(B, q, v, time); c->sim_ticks = 0; c->mpc.solved_B = 0; c->wbc.reset(); c->sim.step(c->mpc.d.mb, B, 0.0, 0);
}
void emu_push_sim_command(void* h, int B, const double* cmd /*[B][90]: posDes velDes kp kd ff*/) { ((EmuPushCtx*)h)->sim.set_command(B, cmd); }
void emu_push_sim_step(void* h, int B, double period, int nsub) { EmuPushCtx* c = (EmuPushCtx*)h; c->sim.step(c->mpc.d.mb, B, period, nsub); }
void emu_push_closed_loop(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int pipelined) {
  EmuPushCtx* c = (EmuPushCtx*)h;
  if (pipelined) qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {});
  else qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, false);
}
void emu_push_readback(void* h, int B, double* q, double* v, double* time, double* rbd, int* contact, double* force, int* sim_status, int* qp_status, int* mpc_status) {
  EmuPushCtx* c = (EmuPushCtx*)h; const QmSimBuffers& s = c->sim.s; const size_t N = (size_t)B;
  memcpy(q, s.q, N * 192); memcpy(v, s.v, N * 192); memcpy(time, s.time, N * 8); memcpy(rbd, s.rbd, N * QM_NRBD * 8); memcpy(contact, s.contact, N * 16); memcpy(force, s.force, N * 96); memcpy(sim_status, s.status, N * 4);
  memcpy(qp_status, c->wbc.w.qp_status, N * 12);
  for (int b = 0; b < B; ++b) mpc_status[b] = qm_mpc_status(c->mpc.d.status[b], c->mpc.d.step_info + (size_t)b * 4, false);
}
// ---- the calls behind qmhip_sim_set_pushes / qmhip_sim_get_push: the same checks in the same order, the same pipeline calls ----
int emu_push_set_pushes(void* h, int B, int K, const qmhip_push* p) {
  EmuPushCtx* c = (EmuPushCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  const bool off = K == 0 || !p;
  if (K < 0 || K > QM_SIM_MAX_PUSH || (!off && (B <= 0 || B > c->Bmax))) return ERR_ARG;
  if (!off && !qm_pushes_valid(B, K, (const double*)p)) return ERR_ARG;
  c->sim.allocate(c->Bmax); c->sim.set_pushes(B, off ? 0 : K, (const double*)p); return OK;
}
int emu_push_get_push(void* h, int B, double* wrench, int* mask) {
  EmuPushCtx* c = (EmuPushCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  if (B <= 0 || B > c->Bmax) return ERR_ARG;
  if (!c->sim.s.Bmax) return ERR_STATE;
  if (wrench) memcpy(wrench, c->sim.s.push_out, (size_t)B * 72); if (mask) memcpy(mask, c->sim.s.push_mask, (size_t)B * 4);
  return OK;
}
}
