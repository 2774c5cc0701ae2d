// qm_rollout_pipeline.h — policy rollout (qmhip_policy_rollout): the launch of k_rollout.h, its row buffers and the hand-over to the host.  Templated on a QUEUE like
// qm_plan_pipeline.h is on its backend: the product drives it with one queue on the MPC stream (source 0: the last solve's stage records, under the context lock) and one
// on the published policy's stream (source 1: a publication slot, under the publication mutex), tests/emu_rollout with the host emulator.  Each queue has a pipeline —
// and so a set of row buffers — of its own: the two sources may run side by side.
//
// One device buffer and its pinned mirror hold every array of a call, inputs first.  They grow on demand and are kept: a repeat call with the same or a smaller R (and trace)
// allocates nothing.  Inputs go up and results come back with ONE copy per array; the host waits once.
// `Q` provides:  void* alloc(size_t);  void free(void*);  void* alloc_pinned(size_t);  void free_pinned(void*);
//   void ro_in(void* dev, const void* pinned, size_t)      asynchronous, in order on the queue
//   template launch(kernel, grid, block, lds, args)         in order on the queue
//   void ro_out(void* pinned, const void* dev, size_t)     asynchronous, in order on the queue
//   void ro_wait()                                          the only host wait
#pragma once
#include <cstdint>
#include <cstring>
#include "../kernels/k_rollout.h"

struct QmRolloutParams { double max_step; int32_t max_steps, source, feedback, trace_cap; };      // struct qmhip_rollout_params (include/qmhip.h)

template <class Q>
struct QmRolloutPipeline {
  Q& q; char* dev = nullptr; char* pin = nullptr; size_t cap = 0; int allocations = 0;
  struct Lay { size_t t0, te, x0, inst, xe, ue, sum, mode, cnt, tr, total; } lay; int R = 0, tcap = 0;
  explicit QmRolloutPipeline(Q& qq) : q(qq) {}
  static size_t up(size_t n) { return (n + 63) & ~(size_t)63; }
  static Lay layout(int R, int tcap) {
    Lay y; size_t o = 0; auto take = [&](size_t n) { const size_t at = o; o += up(n); return at; };
    y.t0 = take((size_t)R * 8); y.te = take((size_t)R * 8); y.x0 = take((size_t)R * 240); y.inst = take((size_t)R * 4);
    y.xe = take((size_t)R * 240); y.ue = take((size_t)R * 240); y.sum = take((size_t)R * QM_RS_BYTES); y.mode = take((size_t)R * 4); y.cnt = take((size_t)R * 4);
    y.tr = take((size_t)R * tcap * QM_RT_BYTES); y.total = o; return y;
  }
  void release() { if (dev) q.free(dev); if (pin) q.free_pinned(pin); dev = pin = nullptr; cap = 0; }
  void reserve(size_t bytes) { if (cap >= bytes) return; release(); dev = (char*)q.alloc(bytes); pin = (char*)q.alloc_pinned(bytes); cap = bytes; ++allocations; }

  // stages the rows, enqueues copies, launch and copy-back; nothing is waited for.  p: grid / primal solution / schedule of the solve or the slot (its batch in p.B);
  // gains: stage records (pub false, W = nmax) or a slot's published records (pub true).  inst null: row r = instance r
  void enqueue(const double* mb, const double* st, const QmPolicyArgs& p, const double* gains, int W, bool pub, int R_, const int32_t* inst, const double* t0, const double* x0, const double* t_end,
               const QmRolloutParams& prm) {
    R = R_; tcap = prm.trace_cap; lay = layout(R, tcap); reserve(lay.total);
    memcpy(pin + lay.t0, t0, (size_t)R * 8); memcpy(pin + lay.te, t_end, (size_t)R * 8); memcpy(pin + lay.x0, x0, (size_t)R * 240);
    int32_t* ih = (int32_t*)(pin + lay.inst); for (int r = 0; r < R; ++r) ih[r] = inst ? inst[r] : r;
    q.ro_in(dev + lay.t0, pin + lay.t0, (size_t)R * 8); q.ro_in(dev + lay.te, pin + lay.te, (size_t)R * 8); q.ro_in(dev + lay.x0, pin + lay.x0, (size_t)R * 240); q.ro_in(dev + lay.inst, pin + lay.inst, (size_t)R * 4);
    QmPolicyRolloutArgs a; a.mb = mb; a.st = st; a.p = p; a.p.t = nullptr; a.p.x_des = nullptr; a.p.u_des = nullptr; a.p.mode = nullptr; a.gains = gains; a.W = W;
    a.R = R; a.inst = (const int*)(dev + lay.inst); a.t0 = (const double*)(dev + lay.t0); a.x0 = (const double*)(dev + lay.x0); a.t_end = (const double*)(dev + lay.te);
    a.max_step = prm.max_step; a.max_steps = prm.max_steps; a.feedback = prm.feedback; a.trace_cap = tcap;
    a.x_end = (double*)(dev + lay.xe); a.u_end = (double*)(dev + lay.ue); a.mode_end = (int*)(dev + lay.mode); a.summary = (double*)(dev + lay.sum); a.trace = tcap ? (double*)(dev + lay.tr) : nullptr; a.count = (int*)(dev + lay.cnt);
    if (pub) q.launch(qm_policy_rollout_kernel<QmFbPubView, PR_SIZE, true>, R, 64, 0, a); else q.launch(qm_policy_rollout_kernel<QmFbStageView, SR_SIZE, false>, R, 64, 0, a);
    q.ro_out(pin + lay.xe, dev + lay.xe, (size_t)R * 240); q.ro_out(pin + lay.ue, dev + lay.ue, (size_t)R * 240); q.ro_out(pin + lay.sum, dev + lay.sum, (size_t)R * QM_RS_BYTES);
    q.ro_out(pin + lay.mode, dev + lay.mode, (size_t)R * 4); q.ro_out(pin + lay.cnt, dev + lay.cnt, (size_t)R * 4);
    if (tcap) q.ro_out(pin + lay.tr, dev + lay.tr, (size_t)R * tcap * QM_RT_BYTES);
  }
  void wait() { q.ro_wait(); }
  // after wait(): the results into the caller's arrays.  Trace slots at or behind a row's count are left alone
  void hand_over(double* x_end, double* u_end, int32_t* mode_end, void* summary, void* trace, int32_t* count) const {
    memcpy(x_end, pin + lay.xe, (size_t)R * 240); memcpy(u_end, pin + lay.ue, (size_t)R * 240); memcpy(mode_end, pin + lay.mode, (size_t)R * 4);
    if (summary) memcpy(summary, pin + lay.sum, (size_t)R * QM_RS_BYTES);
    const int32_t* ch = (const int32_t*)(pin + lay.cnt); if (count) memcpy(count, ch, (size_t)R * 4);
    if (trace && tcap) for (int r = 0; r < R; ++r) { const int ns = ch[r] < tcap ? (ch[r] < 0 ? 0 : ch[r]) : tcap; memcpy((char*)trace + (size_t)r * tcap * QM_RT_BYTES, pin + lay.tr + (size_t)r * tcap * QM_RT_BYTES, (size_t)ns * QM_RT_BYTES); }
  }
};

// what a call may run on, as the entry point sees it when it holds the lock of its source: the last solve (source 0) or the active publication (source 1)
enum { QM_RO_OK = 0, QM_RO_ERR_ARG = -1, QM_RO_ERR_STATE = -5 };      // QMHIP_OK / QMHIP_ERR_ARG / QMHIP_ERR_STATE (include/qmhip.h)
struct QmRolloutSource {
  int solver = 0; bool in_flight = false, have_solution = false;      // source 0: ST_SOLVER, a streamed step or tick in flight, a solve since the last upload / reset / solver switch
  bool published = false, gains = false;                              // source 1: a publication exists, it carries gains
  int B = 0;                                                          // batch of the solve / publication
};
inline const char* qm_rollout_check(int B, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* p, const double* x_end, const double* u_end,
                                    const int32_t* mode_end, const void* trace);
// the decision of qmhip_policy_rollout, shared by the product and the emulator binding: QM_RO_OK, or the error code with its message in *msg.  Nothing is written anywhere
inline int qm_rollout_admit(const QmRolloutSource& s, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* p, const double* x_end, const double* u_end,
                            const int32_t* mode_end, const void* trace, const char** msg) {
  if (!p) { *msg = "bad argument: a required pointer is NULL (p)"; return QM_RO_ERR_ARG; }
  if (p->source != 0 && p->source != 1) { *msg = "bad argument: source is 0 (the last solve) or 1 (the active publication)"; return QM_RO_ERR_ARG; }
  if (p->feedback != 0 && p->feedback != 1) { *msg = "bad argument: feedback is 0 or 1"; return QM_RO_ERR_ARG; }
  if (p->source == 0) {
    if (p->feedback && s.solver != 0 && s.solver != 2) { *msg = "bad argument: the feedback policy exists for the multiple-shooting solver slots only (ST_SOLVER 0 / 2), not for the discrete iLQR (1) or the interior-point method (3); feedback = 0 rolls the feed-forward policy out"; return QM_RO_ERR_ARG; }
    if (s.in_flight) { *msg = "a qmhip_step_submit / qmhip_tick_submit is in flight (collect it first: its solve rewrites the plan and the stage records the rollout reads)"; return QM_RO_ERR_STATE; }
    if (!s.have_solution || s.B <= 0) { *msg = "no policy received yet (no solve on this context since its creation, the last upload, reset or solver switch)"; return QM_RO_ERR_STATE; }
  } else {
    if (!s.published) { *msg = "no policy published yet (qmhip_policy_set_publish_window, then qmhip_policy_publish after a solve)"; return QM_RO_ERR_STATE; }
    if (p->feedback && !s.gains) { *msg = "the active publication carries no gains (it was made with ST_FEEDBACK_POLICY = 0); pass feedback = 0 for its feed-forward policy"; return QM_RO_ERR_STATE; }
  }
  if (const char* bad = qm_rollout_check(s.B, R, inst, t0, x0, t_end, p, x_end, u_end, mode_end, trace)) { *msg = bad; return QM_RO_ERR_ARG; }
  return QM_RO_OK;
}

// argument check: 0 ok, otherwise the message of the QMHIP_ERR_ARG.  B: the batch of the solve / publication
inline const char* qm_rollout_check(int B, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* p, const double* x_end, const double* u_end,
                                    const int32_t* mode_end, const void* trace) {
  if (R < 1) return "bad argument: R < 1";
  if (!t0 || !x0 || !t_end || !p || !x_end || !u_end || !mode_end) return "bad argument: a required pointer is NULL (t0, x0, t_end, p, x_end, u_end, mode_end)";
  if (!(p->max_step > 0.0) || !(p->max_step < __builtin_inf())) return "bad argument: max_step must be a positive finite number";
  if (p->max_steps < 1) return "bad argument: max_steps < 1";
  if (p->source != 0 && p->source != 1) return "bad argument: source is 0 (the last solve) or 1 (the active publication)";
  if (p->feedback != 0 && p->feedback != 1) return "bad argument: feedback is 0 or 1";
  if (p->trace_cap < 0 || (p->trace_cap > 0 && !trace)) return "bad argument: trace_cap < 0, or trace_cap > 0 without a trace array";
  if (!inst && R > B) return "bad argument: inst == NULL needs R <= the batch of the solve / publication (row r = instance r)";
  for (int r = 0; r < R; ++r) {
    if (inst && (inst[r] < 0 || inst[r] >= B)) return "bad argument: an inst entry lies outside the batch of the solve / publication";
    if (!(t0[r] - t0[r] == 0.0) || !(t_end[r] - t_end[r] == 0.0) || t_end[r] < t0[r]) return "bad argument: t0 / t_end must be finite with t_end >= t0";
  }
  return nullptr;
}
