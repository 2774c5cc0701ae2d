// tests/emu_tick/emu_tick_api.cpp — TEST INFRASTRUCTURE: the streamed controller tick (csrc/host/qm_tick_pipeline.h, csrc/kernels/k_tick.h) on the host emulator, in one
// context with the plant and the device loop (qm_closed_loop_sim_ticks) it is checked against, for pytest through ctypes.  Never linked into the product.
#include <cstddef>
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_sim_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_tick_pipeline.h"

struct EmuTickBackend {
  int launches = 0, copies_in = 0, copies_back = 0;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { ++launches; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
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
  void* alloc_pinned(size_t n) { return malloc(n ? n : 8); }
  void free_pinned(void* p) { ::free(p); }
  void* io_event() { return malloc(8); }
  void io_event_free(void* e) { ::free(e); }
  void copy_in(void* d, const void* s, size_t n, int) { ++copies_in; memcpy(d, s, n); }
  void copy_back(void* d, const void* s, size_t n, void*) { ++copies_back; memcpy(d, s, n); }
  void io_wait(void*) {}
};

struct EmuTickCtx {
  EmuTickBackend bk; QmMpcPipeline<EmuTickBackend> mpc; QmWbcPipeline<EmuTickBackend> wbc; QmSimPipeline<EmuTickBackend> sim; QmTickPipeline<EmuTickBackend> tick; long sim_ticks = 0; int Bmax = 0;
  EmuTickCtx() : mpc(bk), wbc(bk), sim(bk), tick(bk) {}
};

extern "C" {
int emu_tick_record_bytes() { return (int)sizeof(qmhip_tick_record); }
// byte offset of the k-th field of struct qmhip_tick_record, in declaration order
int emu_tick_record_offset(int k) {
#define O(f) offsetof(qmhip_tick_record, f)
  const size_t o[] = {O(cmd), O(x_obs), O(x_des), O(u_des), O(wbc_out), O(perf), O(mode), O(mode_meas), O(mpc_status), O(n_nodes), O(qp_status), O(safety), O(stopped), O(mpc_ran), O(tick), O(reserved)};
#undef O
  return k >= 0 && k < 16 ? (int)o[k] : -1;
}
void* emu_tick_create(const double* mb, const double* st, int Bmax, int nmax, int nref, int nev) {
  EmuTickCtx* c = new EmuTickCtx(); c->Bmax = Bmax; c->mpc.allocate(mb, st, Bmax, nmax, nref, nev, false); c->wbc.allocate(Bmax); c->sim.allocate(Bmax); c->tick.allocate(Bmax); return c;
}
void emu_tick_destroy(void* h) { EmuTickCtx* c = (EmuTickCtx*)h; c->mpc.release(); c->wbc.release(); c->sim.release(); c->tick.release(); delete c; }
void emu_tick_upload(void* h, int B, const double* t0, const double* x0, const double* ref_t, const double* ref_x, const double* ev, const int* modes) { ((EmuTickCtx*)h)->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); }
// ---- the plant, carried by the host: qmhip_sim_reset / _set_command / _step / _get_state / _get_rbd ----
void emu_tick_sim_reset(void* h, int B, const double* q, const double* v, const double* time, int controller) {
  EmuTickCtx* c = (EmuTickCtx*)h; c->sim.controller = controller; c->sim.reset(B, q, v, time); c->sim_ticks = 0; c->mpc.solved_B = 0; c->wbc.reset(); c->sim.step(c->mpc.d.mb, B, 0.0, 0);
}
void emu_tick_sim_command(void* h, int B, const double* cmd90) { ((EmuTickCtx*)h)->sim.set_command(B, cmd90); }
void emu_tick_sim_step(void* h, int B, double period, int nsub) { EmuTickCtx* c = (EmuTickCtx*)h; c->sim.step(c->mpc.d.mb, B, period, nsub); }
void emu_tick_sim_get(void* h, int B, double* q, double* v, double* time, double* rbd, int* contact) {
  const QmSimBuffers& s = ((EmuTickCtx*)h)->sim.s;
  memcpy(q, s.q, (size_t)B * 24 * 8); memcpy(v, s.v, (size_t)B * 24 * 8); memcpy(time, s.time, (size_t)B * 8); memcpy(rbd, s.rbd, (size_t)B * QM_NRBD * 8); memcpy(contact, s.contact, (size_t)B * 16);
}
// the device loop the tick is checked against: qm_closed_loop_sim_ticks as qmhip_closed_loop_sim calls it (one SQP iteration per MPC call: the shipped sqp.sqpIteration)
void emu_tick_closed_loop(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int feedback) {
  EmuTickCtx* c = (EmuTickCtx*)h;
  qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, feedback != 0);
}
// what both paths leave in the solver's / the WBC's buffers
void emu_tick_results(void* h, int B, double* wbc_out, int* qp_status, int* mpc_status) {
  EmuTickCtx* c = (EmuTickCtx*)h; memcpy(wbc_out, c->wbc.w.out, (size_t)B * QM_NWBC_OUT * 8); memcpy(qp_status, c->wbc.w.qp_status, (size_t)B * 12);
  for (int b = 0; b < B; ++b) mpc_status[b] = qm_mpc_status(c->mpc.d.status[b], c->mpc.d.step_info + (size_t)b * 4, false);
}
// ---- the tick: the calls qmhip_tick_reset / _submit / _collect / qmhip_observe make ----
void emu_tick_reset(void* h, int B, int controller, double arm_kp, double arm_kd, int mpc_every) {
  EmuTickCtx* c = (EmuTickCtx*)h; c->tick.reset(B, controller, arm_kp, arm_kd, mpc_every); c->wbc.reset(); c->mpc.solved_B = 0;
}
// returns launches * 10000 + input copies * 100 + output copies of this tick
int emu_tick_submit(void* h, const double* time, const double* rbd, const int* contact, double horizon, double period, int feedback) {
  EmuTickCtx* c = (EmuTickCtx*)h; const int l0 = c->bk.launches, i0 = c->bk.copies_in, o0 = c->bk.copies_back;
  c->tick.submit(c->mpc, c->wbc, time, rbd, contact, horizon, period, 1, []() {}, feedback != 0, false);
  return (c->bk.launches - l0) * 10000 + (c->bk.copies_in - i0) * 100 + (c->bk.copies_back - o0);
}
int emu_tick_collect(void* h, void* rec) { EmuTickCtx* c = (EmuTickCtx*)h; if (!c->tick.in_flight) return -1; c->tick.collect(rec); return 0; }
void emu_tick_observe(void* h, int B, const double* rbd, double* x) { EmuTickCtx* c = (EmuTickCtx*)h; c->tick.observe_host(c->mpc.d, B, rbd, x); }
// qm_observe_kernel alone on caller-owned buffers (what the tick's observation is compared with)
void emu_tick_observe_kernel(void* h, int B, const double* rbd, const double* time, double* x0, double* t0) {
  EmuTickCtx* c = (EmuTickCtx*)h; QmObserveArgs o; o.mb = c->mpc.d.mb; o.B = B; o.rbd = rbd; o.time = time; o.x0 = x0; o.t0 = t0; c->bk.launch(qm_observe_kernel, (B + 63) / 64, 64, 0, o);
}
// tick-owned controller state: arm_hold [B][6], arm_last [B][6], yaw_last [B], stopped [B]
void emu_tick_state(void* h, int B, double* arm_hold, double* arm_last, double* yaw_last, int* stopped) {
  const QmTickBuffers& t = ((EmuTickCtx*)h)->tick.t;
  memcpy(arm_hold, t.arm_hold, (size_t)B * 48); memcpy(arm_last, t.arm_last, (size_t)B * 48); memcpy(yaw_last, t.yaw_last, (size_t)B * 8); memcpy(stopped, t.stopped, (size_t)B * 4);
}
}
