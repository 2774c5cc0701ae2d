// tests/emu_rollout/emu_rollout_api.cpp — TEST INFRASTRUCTURE: the policy rollout kernel (qm_policy_rollout_kernel, csrc/kernels/k_rollout.h) on the host emulator, behind
// the pipeline calls and the admission check the product uses (QmRolloutPipeline::enqueue / wait / hand_over, qm_rollout_admit; csrc/host/qm_rollout_pipeline.h), and —
// for the published source — behind QmPublishPipeline::publish.  Never linked into the product.
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_publish_pipeline.h"
#include "../../qm_control_amd/csrc/host/qm_rollout_pipeline.h"
#include <string>

// one queue: copies are memcpy, the wait orders nothing (the data dependencies are the launch order); everything is counted.  A fresh buffer holds NaNs (ints: -1)
struct EmuRolloutQueue {
  int launches = 0, waits = 0, allocs = 0, copies_in = 0, copies_out = 0;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { if (grid <= 0) return; ++launches; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
  void* alloc(size_t n) { ++allocs; void* p = nullptr; if (posix_memalign(&p, 64, n ? n : 8)) return nullptr; memset(p, 0xff, n ? n : 8); return p; }
  void free(void* p) { ::free(p); }
  void* alloc_pinned(size_t n) { return alloc(n); }
  void free_pinned(void* p) { ::free(p); }
  void ro_in(void* d, const void* s, size_t n) { ++copies_in; memcpy(d, s, n); }
  void ro_out(void* d, const void* s, size_t n) { ++copies_out; memcpy(d, s, n); }
  void ro_wait() { ++waits; }
  // what QmPublishPipeline asks of a backend
  void zero(void* p, size_t n) { memset(p, 0, n); }
  void copy_dd(void* d, const void* s, size_t n) { memcpy(d, s, n); }
  void* pub_event() { return malloc(8); }
  void pub_event_free(void* e) { ::free(e); }
  void pub_wait(void*) {}
  void pub_record(void*) {}
};

// a "context": caller-owned solver buffers of a batch of B (node-major [nmax][B][k], stage records [B][nmax][SR_SIZE]) as after a solve, optionally a publication of them
struct EmuRolloutCtx {
  EmuRolloutQueue q; QmRolloutPipeline<EmuRolloutQueue> ro; QmPublishPipeline<EmuRolloutQueue> pub; QmMpcBuffers d; QmRolloutSource solve, publication; long seq = 0; std::string error;
  EmuRolloutCtx() : ro(q), pub(q) {}
};

// the step alone: ilqr_rk2_lane (k_ilqr.h) and its restatement qm_ro_rk2_lane (k_rollout.h) on the same wave, lane-distributed as the kernels hold x and u
struct EmuStepArgs { const double* mb; const double* x; const double* u; double dt; double* a; double* b; };
static void emu_step_kernel(EmuStepArgs s) {
  const int l = threadIdx.x & 63; const double xl = l < 30 ? s.x[l] : 0.0, ul = l < 30 ? s.u[l] : 0.0;
  const double a = ilqr_rk2_lane(s.mb, xl, ul, s.dt, l), b = qm_ro_rk2_lane(s.mb, xl, ul, s.dt, l);
  if (l < 30) { s.a[l] = a; s.b[l] = b; }
}

extern "C" {
void emu_rollout_step_pair(const double* mb, const double* x, const double* u, double dt, double* a, double* b) {
  EmuStepArgs s; s.mb = mb; s.x = x; s.u = u; s.dt = dt; s.a = a; s.b = b; emu::launch(dim3(1), dim3(64), [&]() { emu_step_kernel(s); });
}
int emu_rollout_layout(int which) {
  const int v[] = {SR_SIZE, SR_PP, SR_PX, SR_SWG, SR_MODEF, SR_SCAL, QM_RS_BYTES, QM_RT_BYTES, (int)sizeof(struct qmhip_rollout_summary), (int)sizeof(qmhip_rollout_sample), (int)sizeof(QmRolloutParams), ST_FRIC_COEF, ST_SQP_DT};
  return which >= 0 && which < 13 ? v[which] : -1;
}
void* emu_rollout_create(const double* mb, const double* st, int B, int nmax, int nev, const int* n_nodes, const double* node_t, const int* node_ev, const double* xs, const double* us, const double* ev,
                         const int* modes, const double* stage) {
  EmuRolloutCtx* c = new EmuRolloutCtx(); QmMpcBuffers& d = c->d;
  d.mb = (double*)mb; d.st = (double*)st; d.Bmax = B; d.nmax = nmax; d.nev = nev; d.n_nodes = (int*)n_nodes; d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.xs = (double*)xs; d.us = (double*)us;
  d.ev = (double*)ev; d.modes = (int*)modes; d.stage = (double*)stage; c->solve.B = B;
  return c;
}
void emu_rollout_destroy(void* h) { EmuRolloutCtx* c = (EmuRolloutCtx*)h; c->ro.release(); c->pub.release(); delete c; }
// the state the entry point's admission looks at: solver slot, a step in flight, a solve since the last upload
void emu_rollout_set_state(void* h, int solver, int in_flight, int have_solution) { EmuRolloutCtx* c = (EmuRolloutCtx*)h; c->solve.solver = solver; c->solve.in_flight = in_flight != 0; c->solve.have_solution = have_solution != 0; }
// qmhip_policy_set_publish_window + qmhip_policy_publish on the held buffers; gains 0: a publication made with ST_FEEDBACK_POLICY = 0
long emu_rollout_publish(void* h, int W, int gains) {
  EmuRolloutCtx* c = (EmuRolloutCtx*)h; if (c->pub.W != W) c->pub.set_window(c->d, W);
  c->seq = c->pub.publish(c->d, c->solve.B, gains != 0); c->publication.published = c->seq > 0; c->publication.gains = gains != 0; c->publication.B = c->solve.B; return c->seq;
}
const char* emu_rollout_last_error(void* h) { return ((EmuRolloutCtx*)h)->error.c_str(); }
// qmhip_policy_rollout: the same admission, the same pipeline calls, the same hand-over
int emu_rollout(void* h, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* p, double* x_end, double* u_end, int32_t* mode_end, void* summary, void* trace,
                int32_t* count, int64_t* seq) {
  EmuRolloutCtx* c = (EmuRolloutCtx*)h; const bool pubsrc = p && p->source == 1; const QmRolloutSource& src = pubsrc ? c->publication : c->solve;
  const char* msg = nullptr; const int adm = qm_rollout_admit(src, R, inst, t0, x0, t_end, p, x_end, u_end, mode_end, trace, &msg);
  if (adm != QM_RO_OK) { c->error = std::string("qmhip_policy_rollout: ") + msg; return adm; }
  const QmMpcBuffers& d = c->d;
  if (pubsrc) {
    int act = -1; c->pub.book.info(nullptr, nullptr, &act, nullptr);
    const QmPolicyFbPubArgs pa = c->pub.eval_args(act, src.B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    c->ro.enqueue(d.mb, d.st, pa.p, c->pub.slot[act].gains, c->pub.W, true, R, inst, t0, x0, t_end, *p);
  } else {
    QmPolicyArgs pa; pa.mb = d.mb; pa.B = src.B; pa.nmax = d.nmax; pa.nev = d.nev; pa.n_nodes = d.n_nodes; pa.node_t = d.node_t; pa.node_ev = d.node_ev; pa.xs = d.xs; pa.us = d.us; pa.ev = d.ev; pa.modes = d.modes;
    c->ro.enqueue(d.mb, d.st, pa, d.stage, d.nmax, false, R, inst, t0, x0, t_end, *p);
  }
  c->ro.wait(); c->ro.hand_over(x_end, u_end, mode_end, summary, trace, count); if (pubsrc && seq) *seq = c->seq;
  return QM_RO_OK;
}
// launches, host waits, allocations (device + pinned), copies in, copies out so far
void emu_rollout_counts(void* h, int* out5) { EmuRolloutCtx* c = (EmuRolloutCtx*)h; out5[0] = c->q.launches; out5[1] = c->q.waits; out5[2] = c->q.allocs; out5[3] = c->q.copies_in; out5[4] = c->q.copies_out; }
}
