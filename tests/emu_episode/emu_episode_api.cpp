// tests/emu_episode/emu_episode_api.cpp — TEST INFRASTRUCTURE: the episode monitor (csrc/host/qm_episode_pipeline.h, csrc/kernels/k_episode.h) on the host emulator, in one
// context with the plant and the two device loops (qm_closed_loop_sim_ticks / _pipelined) it observes, for pytest through ctypes.  Never linked into the product.
#include <cstddef>
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_sim_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_episode_pipeline.h"

struct EmuEpBackend {
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
typedef QmEpisodePipeline<EmuEpBackend> EmuEpisode;

struct EmuEpCtx {
  EmuEpBackend bk; QmMpcPipeline<EmuEpBackend> mpc; QmWbcPipeline<EmuEpBackend> wbc; QmSimPipeline<EmuEpBackend> sim; EmuEpisode ep; long sim_ticks = 0; int Bmax = 0;
  EmuEpCtx() : mpc(bk), wbc(bk), sim(bk), ep(bk) {}
};

extern "C" {
// sizes / byte offsets of the two records as the compiler lays the structs out: k-th field in declaration order, -1 behind the last
int emu_episode_bytes(int which) { return which == 0 ? (int)sizeof(struct qmhip_episode_summary) : (int)sizeof(qmhip_episode_sample); }
int emu_episode_summary_offset(int k) {
#define O(f) offsetof(struct qmhip_episode_summary, f)
  const size_t o[] = {O(t_first), O(t_last), O(t_fall), O(min_base_z), O(max_abs_roll), O(max_abs_pitch), O(max_base_speed), O(max_ee_pos_dev), O(sum_sq_ee_pos_dev), O(max_ee_ang_dev), O(max_tau_ratio),
                      O(max_friction_ratio), O(max_normal_force), O(joint_work), O(spare), O(ticks), O(fall_tick), O(fall_cause), O(sim_bad_ticks), O(mpc_calls), O(mpc_fail_calls), O(mpc_warn_or), O(mpc_last_fail),
                      O(mpc_first_fail_tick), O(reserved), O(wbc_bad_ticks), O(airborne_ticks), O(contact_mismatch_ticks), O(touchdowns), O(tau_over_ticks), O(ispare)};
#undef O
  return k >= 0 && k < (int)(sizeof(o) / sizeof(o[0])) ? (int)o[k] : -1;
}
int emu_episode_sample_offset(int k) {
#define O(f) offsetof(qmhip_episode_sample, f)
  const size_t o[] = {O(time), O(rbd), O(force_z), O(tick), O(mode), O(contact_mask), O(mpc_status), O(qp_status), O(sim_status)};
#undef O
  return k >= 0 && k < (int)(sizeof(o) / sizeof(o[0])) ? (int)o[k] : -1;
}
void* emu_episode_create(const double* mb, const double* st, int Bmax, int nmax, int nref, int nev) {
  EmuEpCtx* c = new EmuEpCtx(); c->Bmax = Bmax; c->mpc.allocate(mb, st, Bmax, nmax, nref, nev, false); c->wbc.allocate(Bmax); c->sim.allocate(Bmax); return c;
}
void emu_episode_destroy(void* h) { EmuEpCtx* c = (EmuEpCtx*)h; c->ep.release(); c->mpc.release(); c->wbc.release(); c->sim.release(); delete c; }
void emu_episode_upload(void* h, int B, const double* t0, const double* x0, const double* ref_t, const double* ref_x, const double* ev, const int* modes) { ((EmuEpCtx*)h)->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); }
int emu_episode_launches(void* h) { return ((EmuEpCtx*)h)->bk.launches; }
const char* emu_episode_why(void* h) { return ((EmuEpCtx*)h)->ep.why; }
// ---- what qmhip_sim_reset / qmhip_closed_loop_sim / _pipelined do, the monitor passed as the product passes it ----
void emu_episode_sim_reset(void* h, int B, const double* q, const double* v, const double* time, int controller) {
  EmuEpCtx* c = (EmuEpCtx*)h; c->sim.controller = controller; c->sim.reset(B, q, v, time); c->sim_ticks = 0; c->mpc.solved_B = 0; c->wbc.reset(); c->sim.step(c->mpc.d.mb, B, 0.0, 0);
  if (c->ep.on) c->ep.start(B, c->sim.s.rbd, c->sim.s.contact);
}
void emu_episode_closed_loop(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int pipelined) {
  EmuEpCtx* c = (EmuEpCtx*)h; EmuEpisode* ep = c->ep.on ? &c->ep : nullptr;
  if (pipelined) qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, (QmNoPublish*)nullptr, ep);
  else qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, false, ep);
}
// the same loops as a caller without the feature writes them (no monitor argument: QmNoEpisode) — the launch count the monitor-off path has to reproduce
void emu_episode_closed_loop_plain(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int pipelined) {
  EmuEpCtx* c = (EmuEpCtx*)h;
  if (pipelined) qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {});
  else qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, false);
}
// per-tick readback through what exists without the monitor: plant state, rbd, contact, forces, plant status, WBC output / status, the policy's mode, the MPC status word
void emu_episode_readback(void* h, int B, double* q, double* v, double* time, double* rbd, int* contact, double* force, int* sim_status, double* wbc_out, int* qp_status, int* mode, int* mpc_status) {
  EmuEpCtx* c = (EmuEpCtx*)h; const QmSimBuffers& s = c->sim.s; const size_t N = (size_t)B;
  memcpy(q, s.q, N * 192); memcpy(v, s.v, N * 192); memcpy(time, s.time, N * 8); memcpy(rbd, s.rbd, N * QM_NRBD * 8); memcpy(contact, s.contact, N * 16); memcpy(force, s.force, N * 96); memcpy(sim_status, s.status, N * 4);
  memcpy(wbc_out, c->wbc.w.out, N * QM_NWBC_OUT * 8); memcpy(qp_status, c->wbc.w.qp_status, N * 12); memcpy(mode, c->wbc.w.mode, N * 4);
  for (int b = 0; b < B; ++b) mpc_status[b] = qm_mpc_status(c->mpc.d.status[b], c->mpc.d.step_info + (size_t)b * 4, false);
}
// the primal solution the loop left (what qmhip_mpc_download hands out, node-major as it lies): xs, us [nmax][Bmax][30]
void emu_episode_solution(void* h, double* xs, double* us) { EmuEpCtx* c = (EmuEpCtx*)h; const size_t n = (size_t)c->mpc.d.nmax * c->mpc.d.Bmax * 30 * 8; memcpy(xs, c->mpc.d.xs, n); memcpy(us, c->mpc.d.us, n); }
// ---- the calls behind qmhip_episode_monitor / _set_anchor / _summary / _trace / _fold ----
int emu_episode_monitor(void* h, int on, double min_base_z, double max_tilt, int trace_every, int trace_cap) {
  EmuEpCtx* c = (EmuEpCtx*)h; QmEpisodeParams p{min_base_z, max_tilt, trace_every, trace_cap}; return c->ep.monitor(c->Bmax, on ? &p : nullptr);
}
int emu_episode_set_anchor(void* h, int B, const double* ee) { return ((EmuEpCtx*)h)->ep.set_anchor(B, ee); }
int emu_episode_summary(void* h, int B, void* out) { return ((EmuEpCtx*)h)->ep.read_summary(B, out); }
int emu_episode_trace(void* h, int B, int cap, void* out, int* count) { return ((EmuEpCtx*)h)->ep.read_trace(B, cap, out, count); }
int emu_episode_fold(void* h, int B, int tick, double period, const double* time, const double* rbd, const int* contact, const double* force, const int* mode, const double* wbc_out, const int* qp_status,
                     const int* sim_status, const int* mpc_status) {
  EmuEpCtx* c = (EmuEpCtx*)h; return c->ep.fold(c->mpc.d.mb, B, tick, period, time, rbd, contact, force, mode, wbc_out, qp_status, sim_status, mpc_status);
}
}
