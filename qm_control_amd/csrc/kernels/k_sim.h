// k_sim.h — K8: batched rigid-body plant behind the controller, ONE WAVEFRONT PER INSTANCE.
//
// Stands where Gazebo + qm_gazebo::QMHWSim stand in the reference:
//   * hybrid joint command with the command delay of the simulated hardware interface — QMHWSim::writeSim
//     (qm_gazebo/src/QMHWSim.cpp:98-116): every simulation step pushes the current command (stamp, posDes, velDes, kp, kd, ff) into a
//     per-joint buffer, drops the commands older than `delay` (qm_gazebo/config/default.yaml:2, 9 ms) and applies the OLDEST remaining one:
//     tau_j = kp (posDes − q_j) + kd (velDes − qd_j) + ff; the effort is saturated at the URDF limit as gazebo_ros_control's
//     DefaultRobotHWSim::writeSim [upstream] does through its joint-limits interface;
//   * forward dynamics of the 24-dof floating-base tree:  M(q) vdot = Sᵀ tau − nle(q, v) + Σ_i J_iᵀ f_i  (same recursive world-frame
//     passes as the WBC, qm_dev_rbd.h; generalized velocity = [pdot_world, zyx rates, joint rates]), dense Cholesky of M per step;
//   * ground contact of the four feet.  Gazebo's ODE contact solver is not part of the reference's sources and is not reproduced: the plant
//     uses a stated penalty model on the plane z = 0 — normal force max(0, k pen − d vz) with pen = foot_radius − p_z > 0, regularised Coulomb
//     friction −mu f_n v_t / sqrt(|v_t|² + v_eps²) — parameters in QmSimParams;
//   * semi-implicit Euler: v+ = v + h vdot, q+ = q + h v+ (the coordinates' rates ARE the velocities: Translation + SphericalZYX root);
//   * QMHWSim::readSim (QMHWSim.cpp:60-75): joint / base state and the contact flags; the state is handed over in the estimator's
//     rbd layout (qm_estimation/src/StateEstimateBase.cpp:41-103) so that the WBC and the MPC observation read it like the reference's
//     "ground truth" estimator (FromTopiceEstimate).
//   * external wrenches (no counterpart in the reference's sources): qm_sim_push_kernel, the second instance of the step's body, applies a schedule of base forces,
//     base torques and end-effector forces (QmPushArgs); qm_sim_kernel is the instance without them.
//   * terrain (no counterpart in the reference's sources): qm_sim_terrain_kernel / qm_sim_terrain_push_kernel, two further instances of the step's body, put every foot
//     on a per-robot grid of heights and friction coefficients (QmTerrainArgs; the model: qmhip.h "plant terrain") instead of the plane z = 0.
// Joint position limits and self collision are not modelled.
#pragma once
#include "qm_dev_rbd.h"
#include "qm_dev_kin.h"

#define QM_SIM_SLOTS 16                 /* command delay ring: delay / period + 1 entries are ever live (9 ms / 1 ms); a full ring drops its oldest entry */
#define QM_SIM_CMD 91                   /* stamp, posDes(18), velDes(18), kp(18), kd(18), ff(18) */
struct QmSimParams { double k_n, d_n, mu, v_eps, foot_radius, delay; int saturate; };

struct QmSimArgs {
  const double* mb;
  int B; int nsub; double h;            // one call = one writeSim + nsub integration sub-steps of length h
  QmSimParams p;
  double* q; double* v; double* time;   // [B][24], [B][24], [B] plant state (Pinocchio coordinates)
  const double* cmd;                    // [B][QM_SIM_CMD - 1] command the controller holds (HybridJointHandle::setCommand): posDes velDes kp kd ff
  double* ring; int* ring_n;            // [B][QM_SIM_SLOTS][QM_SIM_CMD] delay buffer, newest first in ring order; [B][2] = head, count
  double* rbd; int* contact;            // [B][55] state in the estimator's layout, [B][4] contact flags (LF RF LH RH)
  double* force;                        // [B][12] contact forces of the last sub-step (world frame)
  int* status;                          // [B] 0 ok, 1 mass matrix not positive definite
};
// scheduled external wrenches (struct qmhip_push, qmhip_layout.h; semantics: qmhip.h "plant disturbances"): slot k of instance b is active in a sub-step iff
// t_on <= t_s < t_off with t_s the plant time at the START of the sub-step; the applied wrench is the sum over the active slots in ascending slot order from +0.0
#define QM_PUSH_WORDS (QM_PUSH_BYTES / 8)   /* t_on, t_off, base_force(3), base_torque(3), ee_force(3), spare */
struct QmPushArgs {
  const double* push; int K; int nB;    // [nB][K][QM_PUSH_WORDS] schedule (world frame, absolute plant time); instances at or beyond nB have none
  double* push_out;                     // [B][9] applied base force, base torque, end-effector force of the last sub-step
  int* push_mask;                       // [B] bit k: slot k was active in the last sub-step
};
struct QmSimPushArgs { QmSimArgs sim; QmPushArgs push; };      // (one argument record per launch: the backends' launch() takes one)
// per-robot ground (struct qmhip_terrain, qmhip_layout.h; the model: qmhip.h "plant terrain"): ny x nx vertices of height and friction in the world frame
#define QM_TERRAIN_WORDS (QM_TERRAIN_BYTES / 8)   /* x0, y0, dx, dy */
struct QmTerrainArgs {
  const double* hdr; int nx, ny, nB;    // [nB][QM_TERRAIN_WORDS] grid origin and spacing; 2 <= nx, ny <= QM_TERRAIN_MAX; instances at or beyond nB stand on the plane z = 0 with p.mu
  const double* height;                 // [nB][ny][nx]
  const double* mu;                     // [nB][ny][nx], or null: p.mu everywhere
  double* ground;                       // [B][4][6] per foot h, n_x, n_y, n_z, mu, pen of the last sub-step
};
struct QmSimTerrainArgs { QmSimArgs sim; QmTerrainArgs ter; };
struct QmSimTerrainPushArgs { QmSimArgs sim; QmPushArgs push; QmTerrainArgs ter; };

// ---- the grid lookup, shared by the plant instances and qm_terrain_eval_kernel.  The cell of a point: clamped to the grid (beyond it the ground continues at the edge's
//      height with zero slope along the clamped coordinate), at s == nx - 1 exactly the last cell ----
struct QmTerrainCell { int i, j; double u, w; bool cx, cy; };
__device__ __forceinline__ void qm_terrain_axis(double x, double x0, double dx, int n, int& i, double& u, bool& c) {
  double s = (x - x0) / dx; c = (s < 0.0 || s > (double)(n - 1)); s = fmin(fmax(s, 0.0), (double)(n - 1));      // (fmax / fmin: a NaN coordinate lands on vertex 0, never outside the array)
  const int k = (int)floor(s); i = k < n - 2 ? k : n - 2; u = s - (double)i;
}
__device__ __forceinline__ QmTerrainCell qm_terrain_cell(const double* hdr, int nx, int ny, double x, double y) {
  QmTerrainCell c; qm_terrain_axis(x, hdr[0], hdr[2], nx, c.i, c.u, c.cx); qm_terrain_axis(y, hdr[1], hdr[3], ny, c.j, c.w, c.cy); return c;
}
// corner k = 0..3 of the cell is vertex (i + (k & 1), j + (k >> 1)): 00, 10, 01, 11
__device__ __forceinline__ size_t qm_terrain_corner(const QmTerrainCell& c, int nx, int k) { return (size_t)(c.j + (k >> 1)) * nx + (size_t)(c.i + (k & 1)); }
__device__ __forceinline__ double qm_terrain_blend(const QmTerrainCell& c, const double* k4) { return (1.0 - c.w) * ((1.0 - c.u) * k4[0] + c.u * k4[1]) + c.w * ((1.0 - c.u) * k4[2] + c.u * k4[3]); }
__device__ __forceinline__ void qm_terrain_slope(const QmTerrainCell& c, const double* hdr, const double* h4, double& gx, double& gy) {
  gx = c.cx ? 0.0 : ((1.0 - c.w) * (h4[1] - h4[0]) + c.w * (h4[3] - h4[2])) / hdr[2];
  gy = c.cy ? 0.0 : ((1.0 - c.u) * (h4[2] - h4[0]) + c.u * (h4[3] - h4[1])) / hdr[3];
}

// ---- LDS carve (doubles) ----
#define SL_M     0                      /* [24][24] */
#define SL_NLE   576
#define SL_JF    600                    /* [12][24] */
#define SL_ACC   888                    /* [6][20] */
#define SL_TIP   1008                   /* feet p(3) v(3) x 4, arm p(3) R(9) */
#define SL_Q     1044
#define SL_V     1068
#define SL_RHS   1092
#define SL_F     1116                   /* [12] */
#define SL_TAU   1128                   /* [18] */
#define SL_JDUM  1146                   /* [6][24] sink of the arm Jacobian (not needed by the plant; its push instance keeps it: J_ee of an end-effector force) */
#define SL_COMP  1290                   /* [19 x 6][6] per-joint subtree composites of the six chain lanes (lane interleaved; registers would spill) */
#define SL_TOTAL (SL_COMP + 19 * 6 * 6)
#define SIM_LDS_BYTES (SL_TOTAL * 8)
#define SL_TER   (SL_ACC + 16)          /* terrain instances: [2][16] corner heights and friction of the four feet (the accumulators are free between two calls of sim_dynamics_terms) */

// measured pass of one chain per lane (lanes 0-3 legs, 4 arm, 5 root body) + base block: M, nle, foot Jacobians, tips
// PUSH: the arm lane keeps its tip Jacobian too — SL_JDUM is zeroed and then holds [lin(3); ang(3)][24], the linear rows with their base columns (the rows J_ee of an
// end-effector force)
template <bool PUSH>
__device__ __forceinline__ void sim_dynamics_terms(const double* mb, double* S, const int l, const bool want_m) {
  double* M = S + SL_M; double* nle = S + SL_NLE; double* Jf = S + SL_JF; const double* q = S + SL_Q; const double* v = S + SL_V;
  for (int i = l; i < SL_TIP; i += 64) S[i] = 0.0;
  if constexpr (PUSH) { if (want_m) for (int i = l; i < 6 * QM_NQ; i += 64) S[SL_JDUM + i] = 0.0; }
  qm_wave_sync();
  if (l < 6) {
    RbdBase Bb; rbd_base(q, v, Bb);
    double cm = 0.0, ch[3] = {0, 0, 0}, cI[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, F[3] = {0, 0, 0}, NO[3] = {0, 0, 0};
    if (l < 5) {
      const bool leg = l < 4; const int contact = leg ? chain_to_contact(l) : 4;
      RbdJsink Jt; Jt.rows = leg ? Jf + 3 * contact * QM_NQ : S + SL_JDUM; Jt.nrows = leg ? 3 : 6; Jt.dummy = 0.0;
      RbdTip tip;
      RbdCompLds comp; comp.base = S + SL_COMP + l; comp.stride = 6;
      rbd_chain<6, double*, RbdJsink, RbdCompLds>(mb, leg ? 3 * l : 12, contact, q, v, Bb, M, nle, want_m, cm, ch, cI, F, NO, (RbdSums*)nullptr, tip, Jt, want_m && (PUSH || leg), leg ? 3 : 6, comp);
      if (PUSH || leg) {
        if (want_m) {
          double* Jr = Jt.rows;
          for (int r = 0; r < 3; ++r) Jr[r * QM_NQ + r] = 1.0;
          for (int k = 0; k < 3; ++k) { const double e[3] = {Bb.E[k], Bb.E[3 + k], Bb.E[6 + k]}, d[3] = {tip.p[0] - Bb.p[0], tip.p[1] - Bb.p[1], tip.p[2] - Bb.p[2]}; double cr[3]; v3_cross(e, d, cr);
            for (int r = 0; r < 3; ++r) Jr[r * QM_NQ + 3 + k] = cr[r]; }
        }
      }
      if (leg) {
        for (int i = 0; i < 3; ++i) { S[SL_TIP + 6 * contact + i] = tip.p[i]; S[SL_TIP + 6 * contact + 3 + i] = tip.v[i]; }
      } else { for (int i = 0; i < 3; ++i) S[SL_TIP + 24 + i] = tip.p[i]; for (int i = 0; i < 9; ++i) S[SL_TIP + 27 + i] = tip.R[i]; }
    } else {
      const double zero3[3] = {0.0, 0.0, 0.0}; double c[3], Iw[9], vc[3], ac[3];
      body_state(mb, 0, Bb.R, Bb.p, Bb.vlin, Bb.w, zero3, Bb.al, c, Iw, vc, ac);
      add_body(mb[MB_MASS], c, Iw, vc, Bb.w, ac, Bb.al, cm, ch, cI, F, NO, (RbdSums*)nullptr);
    }
    double* acc = S + SL_ACC + l * 20;
    acc[0] = cm; for (int i = 0; i < 3; ++i) { acc[1 + i] = ch[i]; acc[13 + i] = F[i]; acc[16 + i] = NO[i]; } for (int i = 0; i < 9; ++i) acc[4 + i] = cI[i];
  }
  qm_wave_sync();
  if (want_m && l < 6) {   // base block of M and base rows of nle from the whole-tree composite (lane = base dof)
    RbdBase Bm; rbd_base(q, v, Bm);
    double cm = 0.0, ch[3] = {0, 0, 0}, cI[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, F[3] = {0, 0, 0}, NO[3] = {0, 0, 0};
    for (int s2 = 0; s2 < 6; ++s2) { const double* acc = S + SL_ACC + s2 * 20; cm += acc[0]; for (int i = 0; i < 3; ++i) { ch[i] += acc[1 + i]; F[i] += acc[13 + i]; NO[i] += acc[16 + i]; } for (int i = 0; i < 9; ++i) cI[i] += acc[4 + i]; }
    double w[3], vO[3]; rbd_S_base(Bm, l, w, vO);
    double wh[3], hv3[3], Iw_[3]; v3_cross(w, ch, wh); v3_cross(ch, vO, hv3); m3_mulv(cI, w, Iw_);
    const double f[3] = {cm * vO[0] + wh[0], cm * vO[1] + wh[1], cm * vO[2] + wh[2]}, nO[3] = {Iw_[0] + hv3[0], Iw_[1] + hv3[1], Iw_[2] + hv3[2]};
    for (int e = 0; e < 6; ++e) { double w2b[3], vO2[3]; rbd_S_base(Bm, e, w2b, vO2); M[e * QM_NQ + l] = w2b[0] * nO[0] + w2b[1] * nO[1] + w2b[2] * nO[2] + vO2[0] * f[0] + vO2[1] * f[1] + vO2[2] * f[2]; }
    nle[l] = w[0] * NO[0] + w[1] * NO[1] + w[2] * NO[2] + vO[0] * F[0] + vO[1] * F[1] + vO[2] * F[2];
  }
  qm_wave_sync();
}

// ground under the four feet at the tips of SL_TIP: ONE round of loads, lane 4 f + c fetches corner c of foot f from both arrays into SL_TER; lanes f < 4 then combine
// their four corners in the stated order.  Every lane of the wave calls it.  g = {h, gx, gy, mu} on lanes 0-3
__device__ __forceinline__ void sim_ground(const QmSimArgs& a, const QmTerrainArgs& ta, double* S, const int b, const int l, double* g) {
  const bool has = b < ta.nB; const double* hdr = ta.hdr + (size_t)(has ? b : 0) * QM_TERRAIN_WORDS;
  if (has && l < 16) {
    const double* tp = S + SL_TIP + 6 * (l >> 2); const QmTerrainCell c = qm_terrain_cell(hdr, ta.nx, ta.ny, tp[0], tp[1]);
    const size_t at = (size_t)b * ta.ny * ta.nx + qm_terrain_corner(c, ta.nx, l & 3);
    S[SL_TER + l] = ta.height[at]; if (ta.mu) S[SL_TER + 16 + l] = ta.mu[at];
  }
  qm_wave_sync();
  if (l < 4) {
    g[0] = 0.0; g[1] = 0.0; g[2] = 0.0; g[3] = a.p.mu;
    if (has) {
      const double* tp = S + SL_TIP + 6 * l; const QmTerrainCell c = qm_terrain_cell(hdr, ta.nx, ta.ny, tp[0], tp[1]);
      g[0] = qm_terrain_blend(c, S + SL_TER + 4 * l); qm_terrain_slope(c, hdr, S + SL_TER + 4 * l, g[1], g[2]);
      if (ta.mu) g[3] = qm_terrain_blend(c, S + SL_TER + 16 + 4 * l);
    }
  }
}
// tangent plane under a foot: unit normal n and penetration of the sphere of radius r at centre height pz
__device__ __forceinline__ double sim_ground_pen(const double* g, double r, double pz, double* n) {
  const double sq = sqrt(1.0 + g[1] * g[1] + g[2] * g[2]); n[0] = -g[1] / sq; n[1] = -g[2] / sq; n[2] = 1.0 / sq;
  return r - (pz - g[0]) * n[2];
}

template <bool PUSH, bool TERRAIN>
__device__ __forceinline__ void sim_step_body(const QmSimArgs& a, const QmPushArgs& pa, const QmTerrainArgs& ta) {
  extern __shared__ double qm_smem[];
  double* S = qm_smem;
  const int b = blockIdx.x, l = threadIdx.x & 63;
  if (b >= a.B) return;
  const double* mb = qm_table(a.mb);
  double* M = S + SL_M; double* nle = S + SL_NLE; double* Jf = S + SL_JF; double* q = S + SL_Q; double* v = S + SL_V; double* rhs = S + SL_RHS; double* fc = S + SL_F; double* tau = S + SL_TAU;
  if (l < 24) { q[l] = a.q[(size_t)b * 24 + l]; v[l] = a.v[(size_t)b * 24 + l]; }
  double time = a.time[b];
  int head = a.ring_n[b * 2], cnt = a.ring_n[b * 2 + 1];
  double* ring = a.ring + (size_t)b * QM_SIM_SLOTS * QM_SIM_CMD;
  int bad = 0;
  double pw = 0.0; int pmask = 0;         // PUSH: lane l < 9 keeps component l of the applied wrench (base force, base torque, end-effector force); active slots
  double gr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // TERRAIN: lane l < 4 keeps its foot's ground record of the last sub-step (nsub == 0: zeros)
  qm_wave_sync();
  // ---- delay buffer (QMHWSim.cpp:100-110), once per call like writeSim once per simulation step: drop what is older than `delay`, push the held
  //      command with the current time stamp, apply the oldest survivor during this step ----
  if (a.nsub > 0) {                       // nsub == 0: hand-over of the current state only (after a reset), not a simulation step
    while (cnt > 0 && ring[((head + cnt - 1) % QM_SIM_SLOTS) * QM_SIM_CMD] + a.p.delay < time) --cnt;
    head = (head + QM_SIM_SLOTS - 1) % QM_SIM_SLOTS; if (cnt < QM_SIM_SLOTS) ++cnt;
    { double* slot = ring + head * QM_SIM_CMD; if (l == 0) slot[0] = time; for (int i = l; i < QM_SIM_CMD - 1; i += 64) slot[1 + i] = a.cmd[(size_t)b * (QM_SIM_CMD - 1) + i]; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    qm_wave_sync();
  }
  const double* use = ring + ((head + (cnt > 0 ? cnt : 1) - 1) % QM_SIM_SLOTS) * QM_SIM_CMD;
  for (int s = 0; s < a.nsub; ++s) {
    if constexpr (PUSH) {                 // the slots are tested at the time the sub-step STARTS at
      pw = 0.0; pmask = 0;
      if (b < pa.nB) for (int k = 0; k < pa.K; ++k) {
        const double* P = pa.push + ((size_t)b * pa.K + k) * QM_PUSH_WORDS;
        if (P[0] <= time && time < P[1]) { pmask |= 1 << k; if (l < 9) pw += P[2 + l]; }
      }
    }
    time += a.h;
    sim_dynamics_terms<PUSH>(mb, S, l, true);
    if (l >= 6 && l < 24) {
      const int j = l - 6;
      double t = use[1 + 36 + j] * (use[1 + j] - q[l]) + use[1 + 54 + j] * (use[1 + 18 + j] - v[l]) + use[1 + 72 + j];   // kp (posDes − q) + kd (velDes − qd) + ff
      const double tm = mb[MB_TAUMAX + j];
      if (a.p.saturate) t = fmin(tm, fmax(-tm, t));
      tau[j] = t;
    }
    if constexpr (TERRAIN) {              // contact against the tangent plane of the ground under the foot
      double g[4]; sim_ground(a, ta, S, b, l, g);
      if (l < 4) {
        const double* tp = S + SL_TIP + 6 * l; double n[3]; const double pen = sim_ground_pen(g, a.p.foot_radius, tp[2], n);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (pen > 0.0) {
          const double vn = tp[3] * n[0] + tp[4] * n[1] + tp[5] * n[2]; const double fn = fmax(0.0, a.p.k_n * pen - a.p.d_n * vn);
          const double vt[3] = {tp[3] - vn * n[0], tp[4] - vn * n[1], tp[5] - vn * n[2]};
          const double sc = -g[3] * fn / sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2] + a.p.v_eps * a.p.v_eps);
          fx = fn * n[0] + sc * vt[0]; fy = fn * n[1] + sc * vt[1]; fz = fn * n[2] + sc * vt[2];
        }
        fc[3 * l] = fx; fc[3 * l + 1] = fy; fc[3 * l + 2] = fz;
        gr[0] = g[0]; gr[1] = n[0]; gr[2] = n[1]; gr[3] = n[2]; gr[4] = g[3]; gr[5] = pen;
      }
    } else if (l < 4) {
      const double* tp = S + SL_TIP + 6 * l; const double pen = a.p.foot_radius - tp[2];
      double fx = 0.0, fy = 0.0, fz = 0.0;
      if (pen > 0.0) {
        fz = fmax(0.0, a.p.k_n * pen - a.p.d_n * tp[5]);
        const double sc = -a.p.mu * fz / sqrt(tp[3] * tp[3] + tp[4] * tp[4] + a.p.v_eps * a.p.v_eps);
        fx = sc * tp[3]; fy = sc * tp[4];
      }
      fc[3 * l] = fx; fc[3 * l + 1] = fy; fc[3 * l + 2] = fz;
    }
    if constexpr (PUSH) { if (l < 9) S[SL_ACC + l] = pw; }      // (the accumulators of sim_dynamics_terms are free between two of its calls)
    qm_wave_sync();
    if (l < 24) { double r = ((l >= 6) ? tau[l - 6] : 0.0) - nle[l]; for (int k = 0; k < 12; ++k) r += Jf[k * QM_NQ + l] * fc[k];
      if constexpr (PUSH) {               // generalized force of the wrench: F on the base translation, Eᵀ n on the zyx rates, J_eeᵀ f on every dof
        const double* w = S + SL_ACC; const double* Je = S + SL_JDUM;
        if (l < 3) r += w[l];
        else if (l < 6) { double E[9]; euler_E<true>(q[3], q[4], E);
          for (int k = 0; k < 3; ++k) if (l == 3 + k) r += E[k] * w[3] + E[3 + k] * w[4] + E[6 + k] * w[5]; }
        for (int i = 0; i < 3; ++i) r += Je[i * QM_NQ + l] * w[6 + i];
      }
      rhs[l] = r; }
    qm_wave_sync();
    // ---- M = L Lᵀ in place (lower triangle), right-looking; lane i owns row i ----
    for (int k = 0; k < 24; ++k) {
      const double dkk = M[k * 24 + k];
      if (!(dkk > 0.0)) bad = 1;
      const double inv = 1.0 / sqrt(dkk > 0.0 ? dkk : 1.0);
      qm_wave_sync();
      if (l >= k && l < 24) M[l * 24 + k] *= inv;                     // column k (the diagonal becomes sqrt(dkk))
      qm_wave_sync();
      if (l > k && l < 24) { const double lik = M[l * 24 + k]; for (int j = k + 1; j <= l; ++j) M[l * 24 + j] -= lik * M[j * 24 + k]; }
      qm_wave_sync();
    }
    // L y = rhs, Lᵀ x = y: lane i keeps its own entry, the resolved ones are published through LDS
    { double r = (l < 24) ? rhs[l] : 0.0;
      for (int k = 0; k < 24; ++k) { if (l == k) rhs[k] = r / M[k * 24 + k]; qm_wave_sync(); if (l > k && l < 24) r -= M[l * 24 + k] * rhs[k]; }
      qm_wave_sync();
      r = (l < 24) ? rhs[l] : 0.0;
      for (int k = 23; k >= 0; --k) { if (l == k) rhs[k] = r / M[k * 24 + k]; qm_wave_sync(); if (l < k) r -= M[k * 24 + l] * rhs[k]; }
      qm_wave_sync(); }
    if (l < 24) { const double vn = v[l] + a.h * rhs[l]; v[l] = vn; q[l] += a.h * vn; }
    qm_wave_sync();
  }
  // ---- hand-over: plant state, estimator-layout rbd state (FK of the arm tip at the final state), contact flags ----
  sim_dynamics_terms<PUSH>(mb, S, l, false);
  if (l < 24) { a.q[(size_t)b * 24 + l] = q[l]; a.v[(size_t)b * 24 + l] = v[l]; }
  double* r = a.rbd + (size_t)b * QM_NRBD;
  if (l < 3) { r[l] = q[3 + l]; r[3 + l] = q[l]; r[27 + l] = v[l]; }
  if (l == 3) { double E[9]; euler_E(q[3], q[4], E); const double thd[3] = {v[3], v[4], v[5]}; double w[3]; m3_mulv(E, thd, w); for (int i = 0; i < 3; ++i) r[24 + i] = w[i]; }
  if (l >= 6 && l < 24) { r[l] = q[l]; r[24 + l] = v[l]; }
  if (l == 4) { double qq[4]; mat_to_quat(S + SL_TIP + 27, qq); for (int i = 0; i < 3; ++i) r[48 + i] = S[SL_TIP + 24 + i]; for (int i = 0; i < 4; ++i) r[51 + i] = qq[i]; }
  if constexpr (TERRAIN) {
    double g[4]; sim_ground(a, ta, S, b, l, g);
    if (l < 4) { double n[3]; a.contact[b * 4 + l] = (sim_ground_pen(g, a.p.foot_radius, S[SL_TIP + 6 * l + 2], n) > 0.0) ? 1 : 0;
      for (int i = 0; i < 6; ++i) ta.ground[(size_t)b * 24 + 6 * l + i] = gr[i]; }
  } else
  if (l < 4) a.contact[b * 4 + l] = (a.p.foot_radius - S[SL_TIP + 6 * l + 2] > 0.0) ? 1 : 0;
  if (l < 12) a.force[(size_t)b * 12 + l] = (a.nsub > 0) ? fc[l] : 0.0;
  if (l == 0) { a.time[b] = time; a.ring_n[b * 2] = head; a.ring_n[b * 2 + 1] = cnt; a.status[b] = bad; }
  if constexpr (PUSH) { if (l < 9) pa.push_out[(size_t)b * 9 + l] = pw; if (l == 0) pa.push_mask[b] = pmask; }      // nsub == 0 (hand-over): nothing applied
}

__global__ void __launch_bounds__(64) qm_sim_kernel(QmSimArgs a) { sim_step_body<false, false>(a, QmPushArgs(), QmTerrainArgs()); }
// the same step with the scheduled wrenches of QmPushArgs applied (one wavefront per instance, the same LDS carve)
__global__ void __launch_bounds__(64) qm_sim_push_kernel(QmSimPushArgs a) { sim_step_body<true, false>(a.sim, a.push, QmTerrainArgs()); }
// the same two steps on the ground of QmTerrainArgs (one wavefront per instance, the same LDS carve)
__global__ void __launch_bounds__(64) qm_sim_terrain_kernel(QmSimTerrainArgs a) { sim_step_body<false, true>(a.sim, QmPushArgs(), a.ter); }
__global__ void __launch_bounds__(64) qm_sim_terrain_push_kernel(QmSimTerrainPushArgs a) { sim_step_body<true, true>(a.sim, a.push, a.ter); }

// the lookup at arbitrary points, one thread per point: out = {h, gx, gy, mu} with mu = mu_default where the terrain carries no friction grid
struct QmTerrainEvalArgs { QmTerrainArgs ter; int B, n; double mu_default; const double* xy; double* out; };      // xy [B][n][2], out [B][n][4]
__global__ void __launch_bounds__(64) qm_terrain_eval_kernel(QmTerrainEvalArgs a) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= (size_t)a.B * a.n) return;
  const int b = (int)(t / a.n); const QmTerrainArgs& ta = a.ter; double* o = a.out + 4 * t;
  if (b >= ta.nB) { o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = a.mu_default; return; }
  const double* hdr = ta.hdr + (size_t)b * QM_TERRAIN_WORDS; const QmTerrainCell c = qm_terrain_cell(hdr, ta.nx, ta.ny, a.xy[2 * t], a.xy[2 * t + 1]);
  const size_t base = (size_t)b * ta.ny * ta.nx; double h4[4], m4[4];
  for (int k = 0; k < 4; ++k) { const size_t at = base + qm_terrain_corner(c, ta.nx, k); h4[k] = ta.height[at]; m4[k] = ta.mu ? ta.mu[at] : a.mu_default; }
  o[0] = qm_terrain_blend(c, h4); qm_terrain_slope(c, hdr, h4, o[1], o[2]); o[3] = ta.mu ? qm_terrain_blend(c, m4) : a.mu_default;
}
