// qm_episode_pipeline.h — the episode monitor (qmhip_episode_*, include/qmhip.h): buffers, launches of k_episode.h and the hand-over to the host.  Backend-templated like
// qm_plan_pipeline.h / qm_tick_pipeline.h: the product drives it with the HIP backend, tests/emu_episode with the host emulator — the argument checks live HERE, so the
// emulator answers with the codes the product answers with.
//
// The device loops (qm_sim_pipeline.h) take a pointer to it (null / QmNoEpisode: the loops launch what they launched without it): tick_fold() behind sim.step of every
// tick, mpc_fold() behind every MPC call.  Nothing is allocated while the monitor is off.  Reads (summary / trace) are ONE copy each, in order on the MPC stream — the
// stream the synchronous loop's ticks run on; the pipelined loop has joined its streams when it returns — and the host waits for ONE event on that stream.
// `BK` provides what qm_plan_pipeline.h lists.
#pragma once
#include <cmath>
#include <cstring>
#include "qm_pipeline.h"
#include "qm_wbc_pipeline.h"
#include "../kernels/k_episode.h"

enum { QM_EP_OK = 0, QM_EP_ERR_ARG = -1, QM_EP_ERR_STATE = -5 };      // the values of QMHIP_OK / QMHIP_ERR_ARG / QMHIP_ERR_STATE (include/qmhip.h; qmhip.hip asserts it)
struct QmEpisodeParams { double min_base_z, max_tilt; int trace_every, trace_cap; };      // struct qmhip_episode_params

template <class BK>
struct QmEpisodePipeline {
  static constexpr bool enabled = true;
  BK& bk; bool on = false; QmEpisodeParams p{0.0, 0.0, 0, 0}; int Bmax = 0;
  int B = 0;                      // batch of the running episode; 0: none started
  bool anchor_set = false; int strict = 0; int slots = 0;      // slots: highest sampled trace slot + 1 (keeps counting behind trace_cap)
  double* summary = nullptr; double* anchor = nullptr; int* flags = nullptr; double* trace = nullptr; char* in_dev = nullptr;
  char* pin = nullptr; size_t pin_cap = 0; void* event = nullptr; const char* why = "";
  explicit QmEpisodePipeline(BK& b) : bk(b) {}
  int fail(int rc, const char* m) { why = m; return rc; }
  // bytes of the inputs of one qmhip_episode_fold for a batch of n: time | rbd | force | wbc_out | contact | mode | qp_status | sim_status | mpc_status
  static size_t in_bytes(int n) { return (size_t)n * ((1 + QM_NRBD + 12 + QM_NWBC_OUT) * 8 + (4 + 1 + 3 + 1 + 1) * 4); }
  void release() {
    void* ps[] = {summary, anchor, flags, trace, in_dev}; for (void* q : ps) if (q) bk.free(q);
    if (pin) bk.free_pinned(pin); if (event) bk.io_event_free(event);
    summary = anchor = trace = nullptr; flags = nullptr; in_dev = pin = nullptr; event = nullptr; pin_cap = 0; on = false; B = 0; Bmax = 0; anchor_set = false; slots = 0;
  }
  // qmhip_episode_monitor: prm null switches the monitor off and frees its buffers; otherwise (re)allocates and waits for an episode to start
  int monitor(int max_batch, const QmEpisodeParams* prm) {
    if (!prm) { release(); return QM_EP_OK; }
    if (!std::isfinite(prm->min_base_z) || !std::isfinite(prm->max_tilt) || prm->trace_every < 0 || prm->trace_cap < 0 || ((prm->trace_every == 0) != (prm->trace_cap == 0)))
      return fail(QM_EP_ERR_ARG, "qmhip_episode_monitor: thresholds must be finite, trace_every and trace_cap >= 0 and both zero or both positive");
    release(); p = *prm; Bmax = max_batch; bk.stream_select(0);
    summary = (double*)bk.alloc((size_t)Bmax * QM_EP_BYTES); anchor = (double*)bk.alloc((size_t)Bmax * 7 * 8); flags = (int*)bk.alloc((size_t)Bmax * 2 * 4); in_dev = (char*)bk.alloc(in_bytes(Bmax));
    bk.zero(summary, (size_t)Bmax * QM_EP_BYTES); bk.zero(anchor, (size_t)Bmax * 7 * 8); bk.zero(flags, (size_t)Bmax * 2 * 4);
    if (p.trace_cap > 0) trace = (double*)bk.alloc((size_t)p.trace_cap * Bmax * QM_ES_BYTES);
    event = bk.io_event(); on = true;
    return QM_EP_OK;
  }
  void reserve_pin(size_t bytes) { if (pin_cap >= bytes) return; if (pin) bk.free_pinned(pin); pin = (char*)bk.alloc_pinned(bytes); pin_cap = bytes; }
  // a new episode of n instances on the current stream.  rbd / contact (device): the reset state — its end-effector pose becomes the anchor, its flags are the
  // contact flags before the first tick; null: the anchor is the caller's (set_anchor), the first folded tick has no transition
  void start(int n, const double* rbd_dev, const int* contact_dev) {
    B = n; slots = 0; if (rbd_dev) anchor_set = true;
    if (trace) bk.zero(trace, (size_t)p.trace_cap * n * QM_ES_BYTES);      // slots never sampled read as zeros
    QmEpisodeStartArgs a; a.B = n; a.rbd = rbd_dev; a.contact = contact_dev; a.summary = summary; a.anchor = anchor; a.flags = flags;
    bk.launch(qm_episode_start_kernel, (n + 63) / 64, 64, 0, a);
  }
  int set_anchor(int n, const double* ee_pose) {
    if (!on) return fail(QM_EP_ERR_STATE, "qmhip_episode_set_anchor: the monitor is off (qmhip_episode_monitor)");
    if (n <= 0 || n > Bmax || !ee_pose) return fail(QM_EP_ERR_ARG, "qmhip_episode_set_anchor: bad argument (0 < B <= max_batch, ee_pose not null)");
    reserve_pin((size_t)n * 56); memcpy(pin, ee_pose, (size_t)n * 56); bk.stream_select(0); bk.copy_in(anchor, pin, (size_t)n * 56, 0); bk.copy_back(pin, anchor, 8, event); bk.io_wait(event);      // (the staging is free again when this returns)
    anchor_set = true; return QM_EP_OK;
  }
  // behind sim.step of tick `tick`: the plant's buffers hold the state behind the tick, the WBC's what the tick computed
  void tick_launch(const double* mb, int n, int tick, double period, const double* time, const double* rbd, const int* contact, const double* force, const int* mode,
                   const double* wbc_out, const int* qp_status, const int* sim_status) {
    QmEpisodeTickArgs a; a.mb = mb; a.B = n; a.tick = tick; a.trace_every = p.trace_every; a.trace_cap = p.trace_cap; a.period = period; a.min_base_z = p.min_base_z; a.max_tilt = p.max_tilt;
    a.time = time; a.rbd = rbd; a.contact = contact; a.force = force; a.mode = mode; a.wbc_out = wbc_out; a.qp_status = qp_status; a.sim_status = sim_status;
    a.summary = summary; a.anchor = anchor; a.flags = flags; a.trace = trace;
    bk.launch(qm_episode_tick_kernel, n, 64, 0, a);      // one wavefront per instance
    if (p.trace_every > 0 && tick % p.trace_every == 0 && tick / p.trace_every + 1 > slots) slots = tick / p.trace_every + 1;
  }
  template <class SimBuffers>
  void tick_fold(const double* mb, int n, long tick, double period, const SimBuffers& s, const QmWbcBuffers& w) {
    if (n != B) return;      // (a loop on another batch than the reset's: not this episode)
    tick_launch(mb, n, (int)tick, period, s.time, s.rbd, s.contact, s.force, w.mode, w.out, w.qp_status, s.status);
  }
  // behind an MPC call that observed at tick `tick` (the solver's status / step_info are final on the current stream)
  void mpc_fold(const QmMpcBuffers& d, int n, long tick) {
    if (n != B) return;
    QmEpisodeMpcArgs a; a.B = n; a.tick = (int)tick; a.strict = strict; a.status = d.status; a.step_info = d.step_info; a.summary = summary; a.flags = flags;
    bk.launch(qm_episode_mpc_kernel, (n + 63) / 64, 64, 0, a);
  }
  // qmhip_episode_fold: one tick of a plant the caller owns, through the same kernels
  int fold(const double* mb, int n, int tick, double period, const double* time, const double* rbd, const int* contact, const double* force, const int* mode, const double* wbc_out,
           const int* qp_status, const int* sim_status, const int* mpc_status) {
    if (!on) return fail(QM_EP_ERR_STATE, "qmhip_episode_fold: the monitor is off (qmhip_episode_monitor)");
    if (n <= 0 || n > Bmax || tick < 0 || !time || !rbd || !contact || !force || !mode || !wbc_out || !qp_status) return fail(QM_EP_ERR_ARG, "qmhip_episode_fold: bad argument (0 < B <= max_batch, tick >= 0; only sim_status and mpc_status may be null)");
    if (B != 0 && n != B) return fail(QM_EP_ERR_ARG, "qmhip_episode_fold: B differs from the batch of the running episode");
    if (B == 0 && !anchor_set) return fail(QM_EP_ERR_STATE, "qmhip_episode_fold: the first fold starts the episode and needs the anchor (qmhip_episode_set_anchor)");
    bk.stream_select(0);
    if (B == 0) start(n, nullptr, nullptr);
    const size_t N = (size_t)n; reserve_pin(in_bytes(n));
    double* t_h = (double*)pin; double* r_h = t_h + N; double* f_h = r_h + N * QM_NRBD; double* w_h = f_h + N * 12; int* c_h = (int*)(w_h + N * QM_NWBC_OUT); int* m_h = c_h + N * 4; int* q_h = m_h + N; int* s_h = q_h + N * 3; int* st_h = s_h + N;
    memcpy(t_h, time, N * 8); memcpy(r_h, rbd, N * QM_NRBD * 8); memcpy(f_h, force, N * 96); memcpy(w_h, wbc_out, N * QM_NWBC_OUT * 8); memcpy(c_h, contact, N * 16); memcpy(m_h, mode, N * 4); memcpy(q_h, qp_status, N * 12);
    if (sim_status) memcpy(s_h, sim_status, N * 4); if (mpc_status) memcpy(st_h, mpc_status, N * 4);
    bk.copy_in(in_dev, pin, in_bytes(n), 0);
    const char* dv = in_dev; auto D = [&](const void* h) { return dv + ((const char*)h - pin); };
    if (mpc_status) { QmEpisodeMpcArgs a; a.B = n; a.tick = tick; a.strict = 0; a.status = (const int*)D(st_h); a.step_info = nullptr; a.summary = summary; a.flags = flags; bk.launch(qm_episode_mpc_kernel, (n + 63) / 64, 64, 0, a); }
    tick_launch(mb, n, tick, period, (const double*)D(t_h), (const double*)D(r_h), (const int*)D(c_h), (const double*)D(f_h), (const int*)D(m_h), (const double*)D(w_h), (const int*)D(q_h),
                sim_status ? (const int*)D(s_h) : nullptr);
    bk.copy_back(pin, flags, 8, event); bk.io_wait(event);      // the staging may be rewritten by the next call
    return QM_EP_OK;
  }
  int read_summary(int n, void* out) {
    if (!on) return fail(QM_EP_ERR_STATE, "qmhip_episode_summary: the monitor is off (qmhip_episode_monitor)");
    if (n <= 0 || n > Bmax || !out) return fail(QM_EP_ERR_ARG, "qmhip_episode_summary: bad argument (0 < B <= max_batch, out not null)");
    if (n != B) return fail(QM_EP_ERR_STATE, "qmhip_episode_summary: B differs from the batch of the running episode (none has started, or it was started for another B)");
    const size_t bytes = (size_t)n * QM_EP_BYTES; reserve_pin(bytes); bk.copy_back(pin, summary, bytes, event); bk.io_wait(event); memcpy(out, pin, bytes);
    return QM_EP_OK;
  }
  // out [min(count, cap, trace_cap)][B], sample-major as on the device: one contiguous copy; what lies behind in `out` is not touched
  int read_trace(int n, int cap, void* out, int32_t* count) {
    if (!on) return fail(QM_EP_ERR_STATE, "qmhip_episode_trace: the monitor is off (qmhip_episode_monitor)");
    if (n <= 0 || n > Bmax || cap < 0 || (cap > 0 && !out) || !count) return fail(QM_EP_ERR_ARG, "qmhip_episode_trace: bad argument (0 < B <= max_batch, cap >= 0, out not null with cap > 0, count not null)");
    if (n != B) return fail(QM_EP_ERR_STATE, "qmhip_episode_trace: B differs from the batch of the running episode (none has started, or it was started for another B)");
    *count = slots; int m = slots < cap ? slots : cap; if (m > p.trace_cap) m = p.trace_cap;
    if (m <= 0) return QM_EP_OK;
    const size_t bytes = (size_t)m * n * QM_ES_BYTES; reserve_pin(bytes); bk.copy_back(pin, trace, bytes, event); bk.io_wait(event); memcpy(out, pin, bytes);
    return QM_EP_OK;
  }
};
