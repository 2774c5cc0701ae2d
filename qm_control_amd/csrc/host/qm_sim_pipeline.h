// qm_sim_pipeline.h — launches of the batched rigid-body plant (backend-templated like qm_pipeline.h)
#pragma once
#include "qm_pipeline.h"
#include "qm_wbc_pipeline.h"
#include "../kernels/k_sim.h"
#include "../kernels/k_sense.h"
#include "../kernels/k_loop.h"

struct QmSimBuffers {
  int Bmax = 0;
  double* q = nullptr; double* v = nullptr; double* time = nullptr; double* cmd = nullptr; double* ring = nullptr; int* ring_n = nullptr;
  double* rbd = nullptr; int* contact = nullptr; double* force = nullptr; int* status = nullptr;
  double* arm_hold = nullptr; double* arm_last = nullptr;     // QMMpcController: held arm position commands and last_time_ per joint ([B][6])
  // published policy (pipelined loop): what evaluatePolicy reads while the MPC writes its next solution — OCS2 guards this buffer with a mutex, here it is a copy
  int p_nmax = 0, p_nev = 0; double* p_xs = nullptr; double* p_us = nullptr; double* p_node_t = nullptr; int* p_node_ev = nullptr; int* p_n_nodes = nullptr; double* p_ev = nullptr; int* p_modes = nullptr;
  bool p_valid = false;
  double* x_est = nullptr; double* t_est = nullptr;      // feedback policy: the tick's estimated centroidal state ([B][30]) on the ticks without an MPC call
  // plant disturbances (qmhip_sim_set_pushes): the schedule [push_B][push_K] of struct qmhip_push (push_K = 0: none, the plain plant kernel runs), what the last
  // sub-step applied ([Bmax][9]) and which slots were active ([Bmax])
  double* push = nullptr; int push_K = 0, push_B = 0; double* push_out = nullptr; int* push_mask = nullptr;
  // sensor model (qmhip_sim_set_sensors): the records [sense_B] of struct qmhip_sensor (sense_on false: off, nothing of k_sense.h is launched and the controller reads rbd),
  // the truth of the last samples [Bmax][QM_SENSE_SLOTS][55], the index of the last sample [Bmax], what the controller is told [Bmax][55]; plant_B: batch of the last reset
  // terrain (qmhip_sim_set_terrain): headers [ter_B] of struct qmhip_terrain, heights and friction [ter_B][ter_ny][ter_nx] — allocated by the first set_terrain for Bmax
  // instances of QM_TERRAIN_MAX² vertices (ter_on false: the plane z = 0, the plant kernels without terrain run) — and the per-foot ground records [Bmax][4][6]
  double* ter_hdr = nullptr; double* ter_h = nullptr; double* ter_mu = nullptr; bool ter_on = false, ter_has_mu = false; int ter_B = 0, ter_nx = 0, ter_ny = 0; double* ground = nullptr;
  unsigned long long* sense = nullptr; bool sense_on = false; int sense_B = 0; double* sense_ring = nullptr; int* sense_n = nullptr; double* rbd_meas = nullptr; int plant_B = 0;
};

// what qmhip_sim_set_pushes accepts: times may be infinite (a permanent load) but not NaN, every force / torque component is finite
static_assert(sizeof(qmhip_push) == QM_PUSH_WORDS * 8, "the plant kernel reads struct qmhip_push as QM_PUSH_WORDS doubles");
inline bool qm_pushes_valid(int B, int K, const double* p) {
  for (size_t i = 0; i < (size_t)B * K; ++i) {
    const double* r = p + i * QM_PUSH_WORDS;
    if (r[0] != r[0] || r[1] != r[1]) return false;
    for (int j = 2; j < 11; ++j) if (!(r[j] - r[j] == 0.0)) return false;      // inf - inf and NaN - NaN are NaN
  }
  return true;
}

// what qmhip_sim_set_terrain accepts: 2 <= nx, ny <= QM_TERRAIN_MAX, finite headers with dx, dy > 0, finite heights, friction coefficients that are finite and not negative
static_assert(sizeof(qmhip_terrain) == QM_TERRAIN_WORDS * 8, "the plant kernel reads struct qmhip_terrain as QM_TERRAIN_WORDS doubles");
inline bool qm_terrain_valid(int B, int nx, int ny, const qmhip_terrain* hdr, const double* height, const double* mu) {
  if (nx < 2 || ny < 2 || nx > QM_TERRAIN_MAX || ny > QM_TERRAIN_MAX || !height) return false;
  for (int b = 0; b < B; ++b) {
    const double r[4] = {hdr[b].x0, hdr[b].y0, hdr[b].dx, hdr[b].dy};
    for (int j = 0; j < 4; ++j) if (!(r[j] - r[j] == 0.0)) return false;
    if (!(r[2] > 0.0 && r[3] > 0.0)) return false;
  }
  for (size_t i = 0; i < (size_t)B * ny * nx; ++i) { if (!(height[i] - height[i] == 0.0)) return false; if (mu && !(mu[i] >= 0.0 && mu[i] - mu[i] == 0.0)) return false; }
  return true;
}

// what qmhip_sim_set_sensors accepts: a lag of 0 .. QM_SENSE_MAX_LAG samples, standard deviations that are finite and not negative
static_assert(sizeof(qmhip_sensor) == QM_SENSE_WORDS * 8, "the sensor kernel reads struct qmhip_sensor as QM_SENSE_WORDS 8-byte words");
inline bool qm_sensors_valid(int B, const qmhip_sensor* r) {
  for (int b = 0; b < B; ++b) {
    if (r[b].lag < 0 || r[b].lag > QM_SENSE_MAX_LAG) return false;
    for (int g = 0; g < QM_SENSE_GROUPS; ++g) if (!(r[b].sigma[g] >= 0.0 && r[b].sigma[g] - r[b].sigma[g] == 0.0 && r[b].bias_sigma[g] >= 0.0 && r[b].bias_sigma[g] - r[b].bias_sigma[g] == 0.0)) return false;
  }
  return true;
}

template <class BK>
struct QmSimPipeline {
  BK& bk; QmSimBuffers s; QmSimParams p;
  int controller = 0;       // 0: QMController (HierarchicalWbc, arm torque + PD), 1: QMMpcController (HierarchicalMpcWbc, arm position commands at 100 Hz)
  explicit QmSimPipeline(BK& b) : bk(b) { p.k_n = 4.0e4; p.d_n = 200.0; p.mu = 0.8; p.v_eps = 1.0e-2; p.foot_radius = 0.02; p.delay = 0.009; p.saturate = 1; }
  template <class T> T* A(size_t n) { T* ptr = (T*)bk.alloc(n * sizeof(T)); bk.zero(ptr, n * sizeof(T)); return ptr; }
  void allocate(int Bmax) {
    if (s.Bmax) return;
    s.Bmax = Bmax; s.q = A<double>((size_t)Bmax * 24); s.v = A<double>((size_t)Bmax * 24); s.time = A<double>(Bmax); s.cmd = A<double>((size_t)Bmax * (QM_SIM_CMD - 1));
    s.ring = A<double>((size_t)Bmax * QM_SIM_SLOTS * QM_SIM_CMD); s.ring_n = A<int>((size_t)Bmax * 2); s.rbd = A<double>((size_t)Bmax * QM_NRBD); s.contact = A<int>((size_t)Bmax * 4);
    s.force = A<double>((size_t)Bmax * 12); s.status = A<int>(Bmax);
    s.arm_hold = A<double>((size_t)Bmax * 6); s.arm_last = A<double>((size_t)Bmax * 6); s.x_est = A<double>((size_t)Bmax * 30); s.t_est = A<double>(Bmax);
    s.push = A<double>((size_t)Bmax * QM_SIM_MAX_PUSH * QM_PUSH_WORDS); s.push_out = A<double>((size_t)Bmax * 9); s.push_mask = A<int>(Bmax);
    s.ground = A<double>((size_t)Bmax * 24);
    s.sense = A<unsigned long long>((size_t)Bmax * QM_SENSE_WORDS); s.sense_ring = A<double>((size_t)Bmax * QM_SENSE_SLOTS * QM_NRBD); s.sense_n = A<int>(Bmax); s.rbd_meas = A<double>((size_t)Bmax * QM_NRBD);
  }
  void release() { void* ps[] = {s.q, s.v, s.time, s.cmd, s.ring, s.ring_n, s.rbd, s.contact, s.force, s.status, s.arm_hold, s.arm_last, s.p_xs, s.p_us, s.p_node_t, s.p_node_ev, s.p_n_nodes, s.p_ev, s.p_modes, s.x_est, s.t_est, s.push, s.push_out, s.push_mask, s.sense, s.sense_ring, s.sense_n, s.rbd_meas, s.ter_hdr, s.ter_h, s.ter_mu, s.ground}; for (void* ptr : ps) if (ptr) bk.free(ptr); s = QmSimBuffers(); }
  // "Simulation reset" of QMHWSim::writeSim: state set, delay buffer and held command cleared
  void reset(int B, const double* q_host, const double* v_host, const double* time_host) {
    s.p_valid = false; s.plant_B = B;
    bk.to_device(s.q, q_host, (size_t)B * 24 * 8); bk.to_device(s.v, v_host, (size_t)B * 24 * 8); bk.to_device(s.time, time_host, (size_t)B * 8);
    bk.zero(s.ring_n, (size_t)s.Bmax * 2 * sizeof(int)); bk.zero(s.cmd, (size_t)s.Bmax * (QM_SIM_CMD - 1) * 8);
    bk.zero(s.push_out, (size_t)s.Bmax * 9 * 8); bk.zero(s.push_mask, (size_t)s.Bmax * sizeof(int));      // nothing applied yet; the schedule itself (absolute plant time) stays
    bk.zero(s.ground, (size_t)s.Bmax * 24 * 8);      // no sub-step yet; the terrain itself stays
    QmArmResetArgs r; r.B = B; r.q = s.q; r.time = s.time; r.arm_hold = s.arm_hold; r.arm_last = s.arm_last; bk.launch(qm_arm_reset_kernel, (B * 6 + 63) / 64, 64, 0, r);
  }
  // schedule of external wrenches, [B][K] records of QM_PUSH_WORDS doubles (validated by the caller); K = 0 or a null pointer switches them off
  void set_pushes(int B, int K, const double* host) {
    if (K <= 0 || !host) { s.push_K = 0; s.push_B = 0; bk.zero(s.push_out, (size_t)s.Bmax * 9 * 8); bk.zero(s.push_mask, (size_t)s.Bmax * sizeof(int)); return; }
    bk.to_device(s.push, host, (size_t)B * K * QM_PUSH_WORDS * 8); s.push_K = K; s.push_B = B;
  }
  // ground of B instances (validated by the caller), a null header switches the terrain off.  The three buffers are sized for Bmax instances of the largest grid on the
  // first call (32 MB at Bmax = 8192: not worth holding for a plant that never leaves the plane)
  void set_terrain(int B, int nx, int ny, const qmhip_terrain* hdr, const double* height, const double* mu) {
    if (!hdr) { s.ter_on = false; s.ter_has_mu = false; s.ter_B = 0; bk.zero(s.ground, (size_t)s.Bmax * 24 * 8); return; }
    const size_t cap = (size_t)s.Bmax * QM_TERRAIN_MAX * QM_TERRAIN_MAX, n = (size_t)B * ny * nx;
    if (!s.ter_h) { s.ter_hdr = A<double>((size_t)s.Bmax * QM_TERRAIN_WORDS); s.ter_h = A<double>(cap); s.ter_mu = A<double>(cap); }
    bk.to_device(s.ter_hdr, hdr, (size_t)B * QM_TERRAIN_BYTES); bk.to_device(s.ter_h, height, n * 8); if (mu) bk.to_device(s.ter_mu, mu, n * 8);
    s.ter_on = true; s.ter_has_mu = mu != nullptr; s.ter_B = B; s.ter_nx = nx; s.ter_ny = ny;
  }
  QmTerrainArgs terrain_args() const { QmTerrainArgs t; t.hdr = s.ter_hdr; t.nx = s.ter_nx; t.ny = s.ter_ny; t.nB = s.ter_B; t.height = s.ter_h; t.mu = s.ter_has_mu ? s.ter_mu : nullptr; t.ground = s.ground; return t; }
  // the plant's lookup at n points per instance (host arrays; a terrain is set — the caller checks)
  void terrain_eval(int B, int n, const double* xy_host, double* out_host) {
    const size_t N = (size_t)B * n; double* xy = (double*)bk.alloc(N * 2 * 8); double* out = (double*)bk.alloc(N * 4 * 8);
    bk.to_device(xy, xy_host, N * 2 * 8);
    QmTerrainEvalArgs e; e.ter = terrain_args(); e.B = B; e.n = n; e.mu_default = p.mu; e.xy = xy; e.out = out;
    bk.launch(qm_terrain_eval_kernel, (int)((N + 63) / 64), 64, 0, e);
    bk.to_host(out_host, out, N * 4 * 8); bk.free(xy); bk.free(out);
  }
  // sensor records [B] (validated by the caller), a null pointer switches the model off.  The sample count starts over: a plant that has been reset hands sample 0 over
  // from its current state at once (one launch of the sensor kernel, none of the plant)
  void set_sensors(const double* mb_dev, int B, const qmhip_sensor* host) {
    if (!host) { s.sense_on = false; s.sense_B = 0; bk.zero(s.sense_n, (size_t)s.Bmax * sizeof(int)); return; }
    bk.to_device(s.sense, host, (size_t)B * QM_SENSE_BYTES); s.sense_on = true; s.sense_B = B;
    if (s.plant_B > 0) sense(mb_dev, s.plant_B, true);
  }
  // the state the controller is given: the sensor model's output, or the plant's state itself
  const double* meas_rbd() const { return s.sense_on ? s.rbd_meas : s.rbd; }
  void sense(const double* mb_dev, int B, bool restart) {
    QmSenseArgs g; g.mb = mb_dev; g.B = B; g.nB = s.sense_B; g.restart = restart ? 1 : 0; g.rec = s.sense; g.rbd = s.rbd; g.ring = s.sense_ring; g.n = s.sense_n; g.meas = s.rbd_meas;
    bk.launch(qm_sense_kernel, B, 64, SENSE_LDS_BYTES, g);      // one wavefront per instance
  }
  void set_command(int B, const double* cmd_host) { bk.to_device(s.cmd, cmd_host, (size_t)B * (QM_SIM_CMD - 1) * 8); }
  // copy of the solver's primal solution + grid + mode schedule into the published-policy buffers
  void publish_policy(const QmMpcBuffers& d) {
    const size_t NB = (size_t)d.nmax * d.Bmax;
    if (!s.p_xs) { s.p_nmax = d.nmax; s.p_nev = d.nev; s.p_xs = A<double>(NB * 30); s.p_us = A<double>(NB * 30); s.p_node_t = A<double>(NB); s.p_node_ev = A<int>(NB); s.p_n_nodes = A<int>(d.Bmax);
                   s.p_ev = A<double>((size_t)d.Bmax * d.nev); s.p_modes = A<int>((size_t)d.Bmax * (d.nev + 1)); }
    bk.copy_dd(s.p_xs, d.xs, NB * 30 * 8); bk.copy_dd(s.p_us, d.us, NB * 30 * 8); bk.copy_dd(s.p_node_t, d.node_t, NB * 8); bk.copy_dd(s.p_node_ev, d.node_ev, NB * 4); bk.copy_dd(s.p_n_nodes, d.n_nodes, (size_t)d.Bmax * 4);
    bk.copy_dd(s.p_ev, d.ev, (size_t)d.Bmax * d.nev * 8); bk.copy_dd(s.p_modes, d.modes, (size_t)d.Bmax * (d.nev + 1) * 4);
    s.p_valid = true;
  }
  // currentObservation_ of the MPC (x0, t0) from the plant state
  void observe(const QmMpcBuffers& d, int B) { QmObserveArgs o; o.mb = d.mb; o.B = B; o.rbd = meas_rbd(); o.time = s.time; o.x0 = d.x0; o.t0 = d.t0; bk.launch(qm_observe_kernel, (B + 63) / 64, 64, 0, o); }
  // the same estimate on a tick between two MPC calls (feedback policy): the observation stays out of the solver's x0 / t0
  void estimate(const QmMpcBuffers& d, int B) { QmObserveArgs o; o.mb = d.mb; o.B = B; o.rbd = meas_rbd(); o.time = s.time; o.x0 = s.x_est; o.t0 = s.t_est; bk.launch(qm_observe_kernel, (B + 63) / 64, 64, 0, o); }
  // hybrid joint command from the evaluated policy and the WBC torques
  void command(int B, const double* x_des, const double* u_des, const double* wbc_out, double arm_kp, double arm_kd) {
    QmCommandArgs c; c.B = B; c.x_des = x_des; c.u_des = u_des; c.wbc_out = wbc_out; c.time = s.time; c.arm_kp = arm_kp; c.arm_kd = arm_kd; c.cmd = s.cmd;
    c.controller = controller; c.rbd = meas_rbd(); c.arm_hold = s.arm_hold; c.arm_last = s.arm_last;
    bk.launch(qm_command_kernel, (B * QM_NJ + 63) / 64, 64, 0, c);
  }
  // rbd state / contact flags of the current plant state without advancing it (nsub = 0 is not a step: the delay buffer is left alone)
  void step(const double* mb_dev, int B, double period, int nsub) {
    QmSimArgs a; a.mb = mb_dev; a.B = B; a.nsub = nsub; a.h = nsub > 0 ? period / nsub : 0.0; a.p = p; a.q = s.q; a.v = s.v; a.time = s.time; a.cmd = s.cmd; a.ring = s.ring; a.ring_n = s.ring_n;
    a.rbd = s.rbd; a.contact = s.contact; a.force = s.force; a.status = s.status;
    if (s.ter_on) {                                      // a terrain is set: the two instances of the kernel that look the ground up
      if (s.push_K > 0) {
        QmSimTerrainPushArgs ta; ta.sim = a; ta.push.push = s.push; ta.push.K = s.push_K; ta.push.nB = s.push_B; ta.push.push_out = s.push_out; ta.push.push_mask = s.push_mask; ta.ter = terrain_args();
        bk.launch(qm_sim_terrain_push_kernel, B, 64, SIM_LDS_BYTES, ta);
      } else { QmSimTerrainArgs ta; ta.sim = a; ta.ter = terrain_args(); bk.launch(qm_sim_terrain_kernel, B, 64, SIM_LDS_BYTES, ta); }
    } else
    if (s.push_K > 0) {                                  // a schedule is set: the instance of the kernel that applies it
      QmSimPushArgs pa; pa.sim = a; pa.push.push = s.push; pa.push.K = s.push_K; pa.push.nB = s.push_B; pa.push.push_out = s.push_out; pa.push.push_mask = s.push_mask;
      bk.launch(qm_sim_push_kernel, B, 64, SIM_LDS_BYTES, pa);
    } else bk.launch(qm_sim_kernel, B, 64, SIM_LDS_BYTES, a);   // one wavefront per instance
    if (s.sense_on) sense(mb_dev, B, nsub == 0);         // sensors are on: one sample behind the step; the hand-over of a reset is sample 0
  }
};

// n_ticks of the whole controller around the plant (QMController::update + the body of mpcThread_, qm_controllers/src/QMController.cpp:128-175, 315-332), all on
// resident data: state estimate (the plant's state) -> every mpc_every ticks an MPC call on that observation (pre_mpc: the gait front-end's schedule refresh,
// then a warm-started solve with sqp_iters SQP iterations) -> policy at the plant time -> WBC on the measured state -> hybrid joint command -> simulation step.
// Shared by the product (qmhip_closed_loop_sim) and the host emulator of the tests.
// feedback (ST_FEEDBACK_POLICY; multiple-shooting solvers only — the caller checks): the tick evaluates the SQP's linear controller at its estimated centroidal state
// (evaluatePolicy(time, currentObservation_.state, ...), QMController.cpp:139-142, with sqp.useFeedbackPolicy) in place of the feed-forward policy: the observation the MPC
// call of this tick was given, or the same estimate built for this tick alone
// epi (a QmEpisodePipeline<BK> that is switched on, qm_episode_pipeline.h): the episode monitor folds every MPC call behind its solve and every tick behind its simulation
// step, reading the buffers the tick left.  Without it (QmNoEpisode, a null pointer, a monitor that is off) the loop launches what it launches without the feature
struct QmNoEpisode { static constexpr bool enabled = false; };
template <class BK, class PreMpc, class Epi = QmNoEpisode>
void qm_closed_loop_sim_ticks(BK& bk, QmMpcPipeline<BK>& mpc, QmWbcPipeline<BK>& wbc, QmSimPipeline<BK>& sim, long& sim_ticks, int B, int n_ticks, double period, int n_substeps,
                              int mpc_every, double horizon, double arm_kp, double arm_kd, int sqp_iters, PreMpc pre_mpc, bool feedback = false, Epi* epi = nullptr) {
  for (int k = 0; k < n_ticks; ++k) {
    const bool mpc_tick = (sim_ticks % mpc_every) == 0;
    if (mpc_tick) {
      sim.observe(mpc.d, B);
      pre_mpc();
      mpc.grid(B, horizon, true); for (int it = 0; it < sqp_iters; ++it) mpc.sqp_iteration(B, 14, it + 1 == sqp_iters);
      if constexpr (Epi::enabled) { if (epi && epi->on) epi->mpc_fold(mpc.d, B, sim_ticks); }
    }
    if (feedback) { if (!mpc_tick) sim.estimate(mpc.d, B); wbc.policy_fb(mpc.d, B, sim.s.time, mpc_tick ? mpc.d.x0 : sim.s.x_est); }
    else bk.launch(qm_policy_kernel, (B + 63) / 64, 64, 0, wbc.pargs(mpc.d, B, sim.s.time));
    // first tick after a reset: inputLast_ primed with the planned input (the reference's WBC has been running since time 0 when the legs are switched on at
    // time 10): zero joint acceleration
    if (sim_ticks == 0) bk.copy_dd(wbc.w.input_last, wbc.w.u_des, (size_t)B * 30 * 8);
    wbc.step(mpc.d, B, period, sim.controller == 1 ? 1 : 0, sim.meas_rbd(), sim.s.time);      // QMMpcController::setupWbc installs HierarchicalMpcWbc (QMController.cpp:410-414)
    sim.command(B, wbc.w.x_des, wbc.w.u_des, wbc.w.out, arm_kp, arm_kd);
    sim.step(mpc.d.mb, B, period, n_substeps);
    if constexpr (Epi::enabled) { if (epi && epi->on) epi->tick_fold(mpc.d.mb, B, sim_ticks, period, sim.s, wbc.w); }
    ++sim_ticks;
  }
}

// The same loop with the MPC beside the control ticks, as the reference's mpcThread_ runs beside QMController::update: the MPC call triggered at a tick observes
// the plant at that tick and computes on its own stream while the next mpc_every ticks run on the other one with the policy published before; its solution is
// published (copied into the policy buffers evaluatePolicy reads) when those ticks are done, i.e. it is used one MPC period after its observation.  The very
// first call is synchronous (there is no policy yet).  n_ticks and the tick counter must be multiples of mpc_every.  BK::stream_select(s) makes stream s (0: MPC,
// 1: ticks) the target of the following launches, BK::stream_order(a, b) orders everything launched so far on a before everything launched later on b; the
// host emulator runs the same sequence on one queue (identical results: the data dependencies are the same).
// pub (a QmPublishPipeline<BK> with a window, qm_publish_pipeline.h; ST_FEEDBACK_POLICY = 1 — the caller checks both): the publication also snapshots the first nodes' gain
// records, and every tick evaluates the published LINEAR controller at its estimated centroidal state, as the synchronous loop does on the live records.  Without it
// (QmNoPublish) the loop is the feed-forward one, launch for launch
// epi: the episode monitor as above; an MPC call is folded on the TICK stream behind its publication — behind stream_order(0, 1), never while a solve runs on the other
// stream — with the tick it observed at
struct QmNoPublish { static constexpr bool enabled = false; };
template <class BK, class PreMpc, class Pub = QmNoPublish, class Epi = QmNoEpisode>
void qm_closed_loop_sim_pipelined(BK& bk, QmMpcPipeline<BK>& mpc, QmWbcPipeline<BK>& wbc, QmSimPipeline<BK>& sim, long& sim_ticks, int B, int n_ticks, double period, int n_substeps,
                                  int mpc_every, double horizon, double arm_kp, double arm_kd, int sqp_iters, PreMpc pre_mpc, Pub* pub = nullptr, Epi* epi = nullptr) {
  auto solve = [&]() { pre_mpc(); mpc.grid(B, horizon, true); for (int it = 0; it < sqp_iters; ++it) mpc.sqp_iteration(B, 14, it + 1 == sqp_iters); };
  auto publish = [&]() {
    if constexpr (Pub::enabled) { if (pub) { pub->publish(mpc.d, B, true); sim.s.p_valid = true; return; } }
    sim.publish_policy(mpc.d);
  };
  auto policy = [&]() {
    if constexpr (Pub::enabled) { if (pub) { sim.estimate(mpc.d, B); pub->tick_policy(wbc, B, sim.s.time, sim.s.x_est); return; } }
    QmPolicyArgs pa = wbc.pargs(mpc.d, B, sim.s.time); pa.n_nodes = sim.s.p_n_nodes; pa.node_t = sim.s.p_node_t; pa.node_ev = sim.s.p_node_ev; pa.xs = sim.s.p_xs; pa.us = sim.s.p_us; pa.ev = sim.s.p_ev; pa.modes = sim.s.p_modes;
    bk.launch(qm_policy_kernel, (B + 63) / 64, 64, 0, pa);
  };
  auto ticks = [&]() {
    for (int k = 0; k < mpc_every; ++k) {
      policy();
      if (sim_ticks == 0) bk.copy_dd(wbc.w.input_last, wbc.w.u_des, (size_t)B * 30 * 8);
      wbc.step(mpc.d, B, period, sim.controller == 1 ? 1 : 0, sim.meas_rbd(), sim.s.time);
      sim.command(B, wbc.w.x_des, wbc.w.u_des, wbc.w.out, arm_kp, arm_kd);
      sim.step(mpc.d.mb, B, period, n_substeps);
      if constexpr (Epi::enabled) { if (epi && epi->on) epi->tick_fold(mpc.d.mb, B, sim_ticks, period, sim.s, wbc.w); }
      ++sim_ticks;
    }
  };
  auto fold_mpc = [&](long t_obs) { if constexpr (Epi::enabled) { if (epi && epi->on) epi->mpc_fold(mpc.d, B, t_obs); } };
  for (int p = 0; p < n_ticks / mpc_every; ++p) {
    const long t_obs = sim_ticks;
    bk.stream_select(1); sim.observe(mpc.d, B); bk.stream_order(1, 0);
    bool have = sim.s.p_valid && sim.s.p_xs != nullptr;
    if constexpr (Pub::enabled) { if (pub) { int k = -1; pub->book.info(nullptr, nullptr, &k, nullptr); have = sim.s.p_valid && k >= 0; } }      // (the two kinds of loop publish into buffers of their own)
    if (!have) {                                // no policy yet: solve first, then run the ticks of this period on it
      bk.stream_select(0); solve(); bk.stream_order(0, 1);
      bk.stream_select(1); publish(); fold_mpc(t_obs); ticks();
    } else {
      bk.stream_select(1); ticks();             // enqueued first: they run while the host waits inside the solve's line search
      bk.stream_select(0); solve(); bk.stream_order(0, 1);
      bk.stream_select(1); publish(); fold_mpc(t_obs);
    }
    bk.stream_order(1, 0);                      // the next solve must not overwrite the solution before it has been published
  }
  bk.stream_select(0);
}
