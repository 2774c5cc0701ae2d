// tests/emu_terrain/emu_terrain_api.cpp — TEST INFRASTRUCTURE: the plant on per-robot terrain (csrc/kernels/k_sim.h: qm_sim_terrain_kernel, qm_sim_terrain_push_kernel,
// qm_terrain_eval_kernel; csrc/host/qm_sim_pipeline.h) on the host emulator, in one context with pushes, sensors and the two device loops (qm_closed_loop_sim_ticks /
// _pipelined) that step it, for pytest through ctypes.  Never linked into the product.
#include <cstddef>
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_sim_pipeline.h"

struct EmuTerrainBackend {
  int n[5] = {0, 0, 0, 0, 0};      // launches of qm_sim_kernel, qm_sim_push_kernel, qm_sim_terrain_kernel, qm_sim_terrain_push_kernel, qm_terrain_eval_kernel
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) {
    const void* k = (const void*)kernel;
    if (k == (const void*)qm_sim_kernel) ++n[0];
    if (k == (const void*)qm_sim_push_kernel) ++n[1];
    if (k == (const void*)qm_sim_terrain_kernel) ++n[2];
    if (k == (const void*)qm_sim_terrain_push_kernel) ++n[3];
    if (k == (const void*)qm_terrain_eval_kernel) ++n[4];
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

struct EmuTerrainCtx {
  EmuTerrainBackend bk; QmMpcPipeline<EmuTerrainBackend> mpc; QmWbcPipeline<EmuTerrainBackend> wbc; QmSimPipeline<EmuTerrainBackend> sim; long sim_ticks = 0; int Bmax = 0; int wbc_only = 0;
  EmuTerrainCtx() : mpc(bk), wbc(bk), sim(bk) {}
};
enum { OK = 0, ERR_ARG = -1, ERR_STATE = -5 };      // QMHIP_OK, QMHIP_ERR_ARG, QMHIP_ERR_STATE (include/qmhip.h)

extern "C" {
int emu_terrain_bytes() { return (int)sizeof(qmhip_terrain); }
int emu_terrain_offset(int k) {
#define O(f) offsetof(qmhip_terrain, f)
  const size_t o[] = {O(x0), O(y0), O(dx), O(dy)};
#undef O
  return k >= 0 && k < (int)(sizeof(o) / sizeof(o[0])) ? (int)o[k] : -1;
}
int emu_terrain_max() { return QM_TERRAIN_MAX; }
void* emu_terrain_create(const double* mb, const double* st, int Bmax, int nmax, int nref, int nev) {
  EmuTerrainCtx* c = new EmuTerrainCtx(); c->Bmax = Bmax; c->mpc.allocate(mb, st, Bmax, nmax, nref, nev, false); c->wbc.allocate(Bmax); return c;      // (the plant allocates on demand, as in the product)
}
void emu_terrain_destroy(void* h) { EmuTerrainCtx* c = (EmuTerrainCtx*)h; c->mpc.release(); c->wbc.release(); c->sim.release(); delete c; }
void emu_terrain_set_wbc_only(void* h, int on) { ((EmuTerrainCtx*)h)->wbc_only = on; }      // stands for a context of qmhip_create_wbc_context
void emu_terrain_upload(void* h, int B, const double* t0, const double* x0, const double* ref_t, const double* ref_x, const double* ev, const int* modes) { ((EmuTerrainCtx*)h)->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); }
void emu_terrain_counts(void* h, int* n /*[5]*/) { EmuTerrainCtx* c = (EmuTerrainCtx*)h; for (int i = 0; i < 5; ++i) n[i] = c->bk.n[i]; }
int emu_terrain_allocated(void* h) { return ((EmuTerrainCtx*)h)->sim.s.ter_h != nullptr; }
// ---- what qmhip_sim_reset / _set_command / _step / _get_state and the two loops do ----
void emu_terrain_sim_reset(void* h, int B, const double* q, const double* v, const double* time) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h; c->sim.allocate(c->Bmax); c->sim.reset(B, q, v, time); c->sim_ticks = 0; c->mpc.solved_B = 0; c->wbc.reset(); c->sim.step(c->mpc.d.mb, B, 0.0, 0);
}
void emu_terrain_sim_command(void* h, int B, const double* cmd /*[B][90]: posDes velDes kp kd ff*/) { ((EmuTerrainCtx*)h)->sim.set_command(B, cmd); }
void emu_terrain_sim_step(void* h, int B, double period, int nsub) { EmuTerrainCtx* c = (EmuTerrainCtx*)h; c->sim.step(c->mpc.d.mb, B, period, nsub); }
void emu_terrain_closed_loop(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int pipelined) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (pipelined) qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {});
  else qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, false);
}
void emu_terrain_readback(void* h, int B, double* q, double* v, double* time, double* rbd, int* contact, double* force, int* sim_status, int* qp_status, int* mpc_status) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h; const QmSimBuffers& s = c->sim.s; const size_t N = (size_t)B;
  memcpy(q, s.q, N * 192); memcpy(v, s.v, N * 192); memcpy(time, s.time, N * 8); memcpy(rbd, s.rbd, N * QM_NRBD * 8); memcpy(contact, s.contact, N * 16); memcpy(force, s.force, N * 96); memcpy(sim_status, s.status, N * 4);
  memcpy(qp_status, c->wbc.w.qp_status, N * 12);
  for (int b = 0; b < B; ++b) mpc_status[b] = qm_mpc_status(c->mpc.d.status[b], c->mpc.d.step_info + (size_t)b * 4, false);
}
// ---- pushes and sensors beside the terrain: the calls behind qmhip_sim_set_pushes / qmhip_sim_set_sensors ----
int emu_terrain_set_pushes(void* h, int B, int K, const qmhip_push* p) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  const bool off = K == 0 || !p;
  if (K < 0 || K > QM_SIM_MAX_PUSH || (!off && (B <= 0 || B > c->Bmax))) return ERR_ARG;
  if (!off && !qm_pushes_valid(B, K, (const double*)p)) return ERR_ARG;
  c->sim.allocate(c->Bmax); c->sim.set_pushes(B, off ? 0 : K, (const double*)p); return OK;
}
int emu_terrain_set_sensors(void* h, int B, const qmhip_sensor* s) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  if (s && (B <= 0 || B > c->Bmax)) return ERR_ARG;
  if (s && !qm_sensors_valid(B, s)) return ERR_ARG;
  c->sim.allocate(c->Bmax); c->sim.set_sensors(c->mpc.d.mb, B, s); return OK;
}
// ---- the calls behind qmhip_sim_set_terrain / qmhip_sim_get_ground / qmhip_terrain_eval: the same checks in the same order, the same pipeline calls ----
int emu_terrain_set_terrain(void* h, int B, int nx, int ny, const qmhip_terrain* hdr, const double* height, const double* mu) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  if (hdr && (B <= 0 || B > c->Bmax)) return ERR_ARG;
  if (hdr && !qm_terrain_valid(B, nx, ny, hdr, height, mu)) return ERR_ARG;
  c->sim.allocate(c->Bmax); c->sim.set_terrain(B, nx, ny, hdr, height, mu); return OK;
}
int emu_terrain_get_ground(void* h, int B, double* ground) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  if (B <= 0 || B > c->Bmax) return ERR_ARG;
  if (!c->sim.s.Bmax) return ERR_STATE;
  if (ground) memcpy(ground, c->sim.s.ground, (size_t)B * 24 * 8);
  return OK;
}
int emu_terrain_eval(void* h, int B, int n, const double* xy, double* out) {
  EmuTerrainCtx* c = (EmuTerrainCtx*)h;
  if (c->wbc_only) return ERR_STATE;
  if (B <= 0 || B > c->Bmax || n <= 0 || !xy || !out) return ERR_ARG;
  if (!c->sim.s.ter_on) return ERR_STATE;
  c->sim.terrain_eval(B, n, xy, out); return OK;
}
}
