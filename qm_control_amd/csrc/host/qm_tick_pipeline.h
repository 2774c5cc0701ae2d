// qm_tick_pipeline.h — the streamed controller tick for a plant on the host (qmhip_tick_reset / _submit / _collect, qmhip_observe): measured rbd state in, hybrid joint
// command out, the controller's state resident between ticks.  Backend-templated like qm_io_pipeline.h / qm_sim_pipeline.h: the product drives it with the HIP backend,
// tests/emu_tick with the host emulator.
//
// A tick launches what a tick of qm_closed_loop_sim_ticks (qm_sim_pipeline.h) launches — the same kernels in the same order on the same kind of data, so the same bits —
// with the plant's part replaced by one input copy in front and one output copy behind, qm_command_kernel by qm_tick_pack_kernel on tick-owned state, and
// qm_tick_state_kernel (k_tick.h) behind the observation.  Depth is one: a tick is collected before the next is submitted.
// `BK` provides, beyond what qm_pipeline.h lists:  void* alloc_pinned(size_t);  void free_pinned(void*);  void* io_event();  void io_event_free(void*);
//   void copy_in(void* dev, const void* pinned, size_t, int stream)     asynchronous, in order on that stream (0: the stream the tick runs on)
//   void copy_back(void* pinned, const void* dev, size_t, void* event)  asynchronous, in order behind the tick's last kernel; then records `event`
//   void io_wait(void* event)                                           the ONLY host wait of the pair
#pragma once
#include <cstring>
#include "qm_wbc_pipeline.h"
#include "../kernels/k_loop.h"
#include "../kernels/k_tick.h"

struct QmTickBuffers {
  int Bmax = 0;
  char* in_pin = nullptr; char* in_dev = nullptr;        // [time B | rbd B x 55 | contact B x 4 (int32)] of the tick's batch: one copy
  char* rec_dev = nullptr; char* rec_pin = nullptr; void* event = nullptr;
  double* x_est = nullptr; double* t_est = nullptr;      // observation of a tick without an MPC call ([B][30], [B])
  double* cmd = nullptr; double* arm_hold = nullptr; double* arm_last = nullptr; double* yaw_last = nullptr; int* stopped = nullptr; int* flags = nullptr;
};

template <class BK>
struct QmTickPipeline {
  BK& bk; QmTickBuffers t;
  int B = 0, controller = 0, mpc_every = 1, in_flight = 0; long tick = 0; double arm_kp = 0.0, arm_kd = 0.0;      // B = 0: no qmhip_tick_reset yet
  explicit QmTickPipeline(BK& b) : bk(b) {}
  template <class T> T* A(size_t n) { T* p = (T*)bk.alloc(n * sizeof(T)); bk.zero(p, n * sizeof(T)); return p; }
  static size_t in_bytes(int B) { return (size_t)B * ((1 + QM_NRBD) * sizeof(double) + 4 * sizeof(int)); }
  // allocated by the first use: a context that never ticks pays nothing
  void allocate(int Bmax) {
    if (t.Bmax) return; t.Bmax = Bmax;
    t.in_pin = (char*)bk.alloc_pinned(in_bytes(Bmax)); t.in_dev = (char*)bk.alloc(in_bytes(Bmax)); t.rec_dev = (char*)bk.alloc((size_t)Bmax * QM_TICK_BYTES); t.rec_pin = (char*)bk.alloc_pinned((size_t)Bmax * QM_TICK_BYTES);
    t.event = bk.io_event(); t.x_est = A<double>((size_t)Bmax * 30); t.t_est = A<double>(Bmax);
    t.cmd = A<double>((size_t)Bmax * 90); t.arm_hold = A<double>((size_t)Bmax * 6); t.arm_last = A<double>((size_t)Bmax * 6); t.yaw_last = A<double>(Bmax); t.stopped = A<int>(Bmax); t.flags = A<int>((size_t)Bmax * QM_TICK_FLAGS);
  }
  void release() {
    if (t.in_pin) bk.free_pinned(t.in_pin); if (t.rec_pin) bk.free_pinned(t.rec_pin); if (t.event) bk.io_event_free(t.event);
    void* ps[] = {t.in_dev, t.rec_dev, t.x_est, t.t_est, t.cmd, t.arm_hold, t.arm_last, t.yaw_last, t.stopped, t.flags}; for (void* p : ps) if (p) bk.free(p);
    t = QmTickBuffers(); B = 0; in_flight = 0; tick = 0;
  }
  // sections of the input buffer for a batch of B
  template <class P> static double* in_time(P base, int) { return (double*)base; }
  template <class P> static double* in_rbd(P base, int B) { return (double*)base + B; }
  template <class P> static int* in_contact(P base, int B) { return (int*)((double*)base + (size_t)B * (1 + QM_NRBD)); }
  // QMController::starting: zeroed observation (previous yaw 0), nothing commanded yet, not stopped; the MPC / WBC side of the reset is the caller's
  void reset(int B_, int controller_, double kp, double kd, int every) {
    B = B_; controller = controller_; arm_kp = kp; arm_kd = kd; mpc_every = every; tick = 0;
    bk.zero(t.cmd, (size_t)t.Bmax * 90 * 8); bk.zero(t.arm_hold, (size_t)t.Bmax * 6 * 8); bk.zero(t.arm_last, (size_t)t.Bmax * 6 * 8); bk.zero(t.yaw_last, (size_t)t.Bmax * 8); bk.zero(t.stopped, (size_t)t.Bmax * 4);
  }
  bool mpc_tick() const { return (tick % mpc_every) == 0; }
  void observe(const QmMpcBuffers& d, int n, double* x, double* t0) { QmObserveArgs o; o.mb = d.mb; o.B = n; o.rbd = in_rbd(t.in_dev, n); o.time = in_time(t.in_dev, n); o.x0 = x; o.t0 = t0; bk.launch(qm_observe_kernel, (n + 63) / 64, 64, 0, o); }
  // computeCentroidalStateFromRbdModel of host states, stateless (qmhip_observe): the observation kernel alone, through the tick's staging
  void observe_host(const QmMpcBuffers& d, int n, const double* rbd_host, double* x_host) {
    bk.to_device(in_rbd(t.in_dev, n), rbd_host, (size_t)n * QM_NRBD * 8); observe(d, n, t.x_est, t.t_est); bk.to_host(x_host, t.x_est, (size_t)n * 30 * 8);
  }
  // One QMController::update for the batch, everything enqueued, nothing waited for.  pre_mpc: the gait front-end's schedule refresh; feedback: ST_FEEDBACK_POLICY
  template <class PreMpc>
  void submit(QmMpcPipeline<BK>& mpc, QmWbcPipeline<BK>& wbc, const double* time, const double* rbd, const int* contact, double horizon, double period, int sqp_iters, PreMpc pre_mpc, bool feedback, bool strict) {
    const QmMpcBuffers& d = mpc.d; const bool run_mpc = mpc_tick();
    memcpy(in_time(t.in_pin, B), time, (size_t)B * 8); memcpy(in_rbd(t.in_pin, B), rbd, (size_t)B * QM_NRBD * 8); if (contact) memcpy(in_contact(t.in_pin, B), contact, (size_t)B * 16);
    bk.copy_in(t.in_dev, t.in_pin, in_bytes(B), 0);
    const double* time_dev = in_time(t.in_dev, B); const double* rbd_dev = in_rbd(t.in_dev, B);
    double* x_obs = run_mpc ? d.x0 : t.x_est;      // as QmSimPipeline::observe / estimate: the solver's (x0, t0) only on a tick that calls the MPC
    observe(d, B, x_obs, run_mpc ? d.t0 : t.t_est);
    QmTickStateArgs s; s.B = B; s.x = x_obs; s.contact = contact ? in_contact(t.in_dev, B) : nullptr; s.yaw_last = t.yaw_last; s.stopped = t.stopped; s.flags = t.flags;
    bk.launch(qm_tick_state_kernel, (B + 63) / 64, 64, 0, s);
    if (run_mpc) { pre_mpc(); mpc.grid(B, horizon, true); for (int it = 0; it < sqp_iters; ++it) mpc.sqp_iteration(B, 14, it + 1 == sqp_iters); }      // the MPC call of qm_closed_loop_sim_ticks
    if (feedback) wbc.policy_fb(d, B, time_dev, x_obs); else bk.launch(qm_policy_kernel, (B + 63) / 64, 64, 0, wbc.pargs(d, B, time_dev));
    if (tick == 0) bk.copy_dd(wbc.w.input_last, wbc.w.u_des, (size_t)B * 30 * 8);      // inputLast_ primed with the planned input, as the device loop does
    wbc.step(d, B, period, controller == 1 ? 1 : 0, rbd_dev, time_dev);
    QmTickPackArgs p; p.B = B; p.controller = controller; p.tick = (int)tick; p.mpc_ran = run_mpc ? 1 : 0; p.strict = strict ? 1 : 0; p.arm_kp = arm_kp; p.arm_kd = arm_kd;
    p.x_obs = x_obs; p.x_des = wbc.w.x_des; p.u_des = wbc.w.u_des; p.mode = wbc.w.mode; p.wbc_out = wbc.w.out; p.qp_status = wbc.w.qp_status;
    p.out_perf = d.out_perf; p.status = d.status; p.step_info = d.step_info; p.n_nodes = d.n_nodes; p.rbd = rbd_dev; p.time = time_dev; p.flags = t.flags;
    p.cmd = t.cmd; p.arm_hold = t.arm_hold; p.arm_last = t.arm_last; p.rec = (double*)t.rec_dev;
    bk.launch(qm_tick_pack_kernel, B, QM_TICK_LANES, 0, p);
    bk.copy_back(t.rec_pin, t.rec_dev, (size_t)B * QM_TICK_BYTES, t.event);
    ++tick; in_flight = 1;
  }
  void collect(void* rec) { bk.io_wait(t.event); memcpy(rec, t.rec_pin, (size_t)B * QM_TICK_BYTES); in_flight = 0; }
};
