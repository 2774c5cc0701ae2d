// tests/emu_pub/emu_pub_api.cpp — TEST INFRASTRUCTURE: the published-policy kernels (qm_policy_publish_kernel, qm_policy_fb_pub_kernel; csrc/kernels/k_publish.h) on the
// host emulator, launched through the pipeline calls the product uses (QmPublishPipeline::publish / eval_args / tick_policy, qm_closed_loop_sim_pipelined with a publisher).
// Never linked into the product.
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_wbc_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_sim_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_publish_pipeline.h"

// one queue: the events of the published policy order nothing here (the data dependencies are the launch order); they are counted
struct EmuPubBackend {
  int launches = 0, waits = 0, records = 0; const void* last = nullptr;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { ++launches; last = (const void*)kernel; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
  void* alloc(size_t n) { void* p = nullptr; if (posix_memalign(&p, 64, n ? n : 8)) return nullptr; memset(p, 0xff, n ? n : 8); return p; }      // a fresh buffer holds NaNs (ints: -1): a read of something never written shows
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
  void* pub_event() { return malloc(8); }
  void pub_event_free(void* e) { ::free(e); }
  void pub_wait(void*) { ++waits; }
  void pub_record(void*) { ++records; }
};

struct EmuPubCtx {
  EmuPubBackend bk; QmMpcPipeline<EmuPubBackend> mpc; QmWbcPipeline<EmuPubBackend> wbc; QmSimPipeline<EmuPubBackend> sim; QmPublishPipeline<EmuPubBackend> pub; long ticks = 0;
  EmuPubCtx() : mpc(bk), wbc(bk), sim(bk), pub(bk) {}
};

extern "C" {
int emu_pub_layout(int which) { const int v[] = {SR_SIZE, SR_PP, SR_PX, SR_SWG, SR_MODEF, SR_SCAL, PR_SIZE, PR_PP, PR_PX, PR_SWG, PR_MODEF, PR_SCAL}; return which >= 0 && which < 12 ? v[which] : -1; }

// ---- the two kernels on caller-owned solver buffers (node-major [nmax][B][k], stage records [B][nmax][SR_SIZE]) ----
// publish with a window of W nodes into a pipeline allocated for B + 1 instances (the last instance's records are never written: the slot's unused tail), then evaluate the
// active slot at (t, x); x null: the feed-forward policy.  n_pub publications are made (the same data every time: the slots alternate).  pub_out (may be null): the active
// slot's records [B + 1][W][PR_SIZE].  Returns the sequence number of the evaluated publication
long emu_pub_publish_eval(int B, int nmax, int nev, int W, int n_pub, const int* n_nodes, const double* node_t, const int* node_ev, const double* xs, const double* us, const double* ev, const int* modes,
                          const double* stage, const double* t, const double* x, double* x_des, double* u_des, int* mode, int* covered, double* pub_out) {
  EmuPubBackend bk; QmPublishPipeline<EmuPubBackend> pub(bk);
  QmMpcBuffers d; d.Bmax = B + 1; d.nmax = nmax; d.nev = nev; d.n_nodes = (int*)n_nodes; d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.xs = (double*)xs; d.us = (double*)us;
  d.ev = (double*)ev; d.modes = (int*)modes; d.stage = (double*)stage;
  pub.set_window(d, W); long seq = 0;
  for (int k = 0; k < n_pub; ++k) seq = pub.publish(d, B, true);
  int act = -1; pub.book.info(nullptr, nullptr, &act, nullptr);
  bk.launch(qm_policy_fb_pub_kernel, B, 64, 0, pub.eval_args(act, B, t, x, x_des, u_des, mode, covered, nullptr));
  if (pub_out) memcpy(pub_out, pub.slot[act].gains, (size_t)(B + 1) * W * PR_SIZE * 8);
  pub.release(); return seq;
}

// ---- the pipelined loop around the plant (the calls of tests/emu/emu_api.cpp, with a publisher) ----
void* emu_pub_create(const double* mb, const double* st, int Bmax, int nmax, int nref, int nev) { EmuPubCtx* c = new EmuPubCtx(); c->mpc.allocate(mb, st, Bmax, nmax, nref, nev, false); c->wbc.allocate(Bmax, false); return c; }
void emu_pub_destroy(void* h) { EmuPubCtx* c = (EmuPubCtx*)h; c->pub.release(); c->mpc.release(); c->wbc.release(); c->sim.release(); delete c; }
void emu_pub_set_window(void* h, int W) { EmuPubCtx* c = (EmuPubCtx*)h; c->pub.set_window(c->mpc.d, W); }
void emu_pub_upload_grid(void* h, int B, const double* t0, const double* x0, const double* ref_t, const double* ref_x, const double* ev, const int* modes, double horizon) {
  EmuPubCtx* c = (EmuPubCtx*)h; c->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); c->mpc.grid(B, horizon);
}
void emu_pub_sim_start(void* h, int B, const double* params7, const double* q, const double* v, const double* time) {
  EmuPubCtx* c = (EmuPubCtx*)h; QmSimParams& p = c->sim.p; p.k_n = params7[0]; p.d_n = params7[1]; p.mu = params7[2]; p.v_eps = params7[3]; p.foot_radius = params7[4]; p.delay = params7[5]; p.saturate = params7[6] != 0.0;
  c->wbc.reset(); c->sim.allocate(c->mpc.d.Bmax); c->sim.reset(B, q, v, time); c->pub.reset_counters(); c->ticks = 0; c->sim.s.p_valid = false; c->sim.step(c->mpc.d.mb, B, 0.0, 0);
}
// feedback: the publisher is handed to the loop (what qmhip_closed_loop_sim_pipelined does with a window and ST_FEEDBACK_POLICY = 1)
void emu_pub_loop(void* h, int B, int n_ticks, double period, int nsub, int mpc_every, double horizon, double arm_kp, double arm_kd, int feedback) {
  EmuPubCtx* c = (EmuPubCtx*)h;
  qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->ticks, B, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, 1, []() {}, feedback ? &c->pub : (QmPublishPipeline<EmuPubBackend>*)nullptr);
}
void emu_pub_state(void* h, int B, double* q, double* v, double* wbc_out, int* qp_status, int* mpc_status, double* u_des, int* uncovered, long* seq) {
  EmuPubCtx* c = (EmuPubCtx*)h; memcpy(q, c->sim.s.q, (size_t)B * 24 * 8); memcpy(v, c->sim.s.v, (size_t)B * 24 * 8); memcpy(wbc_out, c->wbc.w.out, (size_t)B * QM_NWBC_OUT * 8);
  memcpy(qp_status, c->wbc.w.qp_status, (size_t)B * 12); memcpy(mpc_status, c->mpc.d.status, (size_t)B * 4); memcpy(u_des, c->wbc.w.u_des, (size_t)B * 30 * 8);
  if (c->pub.uncovered) memcpy(uncovered, c->pub.uncovered, (size_t)B * 4); else memset(uncovered, 0, (size_t)B * 4);
  c->pub.book.info(seq, nullptr, nullptr, nullptr);
}
// the feed-forward policy of the ACTIVE publication at the plant time (the feedback term of the last tick = wbc u_des − this, evaluated before the plant moved on is not
// available afterwards: the tests take the feedback term from the oracle loop instead); launches and event calls so far
void emu_pub_counts(void* h, int* launches, int* waits, int* records) { EmuPubCtx* c = (EmuPubCtx*)h; *launches = c->bk.launches; *waits = c->bk.waits; *records = c->bk.records; }
}
