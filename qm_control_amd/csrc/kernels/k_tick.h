// k_tick.h — the two kernels the streamed controller tick (qmhip_tick_submit / qmhip_tick_collect, include/qmhip.h) adds around the existing ones.  One tick of
// QMController::update (qm_controllers/src/QMController.cpp:128-175) for a plant the library does not own is
//   input copy -> qm_observe_kernel (k_loop.h, as it is) -> qm_tick_state_kernel -> [MPC call] -> qm_policy_kernel / qm_policy_fb_kernel -> qm_wbc_kernel -> qm_tick_pack_kernel -> output copy
// The observation, the policy and the WBC are NOT restated here: the same function inlined into two kernels may contract its FMAs differently, and the
// tick has to reproduce the device loop's bits (tests/test_emu_tick.py, check (B)).
//
//   qm_tick_state_kernel  one thread per instance, behind the observation: the two statements of the reference's tick the device loop leaves out —
//                         the yaw unwrapping of updateStateEstimation (QMController.cpp:239-242) in place on the observation, and SafetyChecker::checkOrientation
//                         (SafetyChecker.h:25-32, call site QMController.cpp:159-162) with its sticky stop — plus the measured mode (stanceLeg2ModeNumber)
//   qm_tick_pack_kernel   one workgroup per instance: updateControlLaw (the law and per-joint arm state of qm_command_kernel, k_loop.h) on TICK-OWNED state, the stop
//                         masking, and the instance's 2048-byte record (struct qmhip_tick_record, include/qmhip_layout.h)
// Both are glue: no LDS, no private segment, no atomics.
#pragma once
#include "k_grid.h"

#define QM_TICK_TWO_PI 6.283185307179586      /* 2 * M_PI, exactly */
#define QM_TICK_HALF_PI 1.5707963267948966    /* M_PI_2 */
#define QM_TICK_FLAGS 4                       /* per-instance words the state kernel leaves for the pack kernel: measured mode, safety, stopped at the START of the tick, spare */
#define QM_TICK_LANES 256                     /* threads per record (>= 18 law lanes + 172 copied doubles + 24 status words) */

__host__ __device__ inline int qm_mpc_status(int k0_status, const double* step_info4, bool strict);      // csrc/host/qm_pipeline.h

// Yaw unwrapping: yaw + 2 pi k with k = nearbyint((yawLast − yaw) / 2 pi) — the reference's yawLast + shortest_angular_distance(yawLast, yaw) up to rounding; a yaw
// that does not wrap (k = 0) is handed through UNCHANGED, −0.0 included, so a plant whose Euler angles never wrap sees the device loop's observation bit for bit.
struct QmTickStateArgs {
  int B; double* x;                 // [B][30] the observation qm_observe_kernel wrote (the solver's x0 on a tick with an MPC call, the tick's own estimate otherwise)
  const int* contact;               // [B][4] LF RF LH RH, or null
  double* yaw_last; int* stopped;   // [B] tick-owned state: previous observation's yaw, sticky stop flag
  int* flags;                       // [B][QM_TICK_FLAGS]
};
__global__ void qm_tick_state_kernel(QmTickStateArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  double* x = a.x + (size_t)b * 30;
  double yaw = x[9]; const double k = nearbyint((a.yaw_last[b] - yaw) / QM_TICK_TWO_PI);
  if (k != 0.0) { yaw = yaw + QM_TICK_TWO_PI * k; x[9] = yaw; }
  const int unsafe = (x[11] > QM_TICK_HALF_PI || x[11] < -QM_TICK_HALF_PI) ? 1 : 0;      // pose(5): the reference's strict comparison, exactly +-pi/2 passes
  const int was_stopped = a.stopped[b];
  int mode = -1;
  if (a.contact) { const int* c = a.contact + (size_t)b * 4; mode = (c[0] ? 8 : 0) + (c[1] ? 4 : 0) + (c[2] ? 2 : 0) + (c[3] ? 1 : 0); }
  int* f = a.flags + (size_t)b * QM_TICK_FLAGS; f[0] = mode; f[1] = unsafe; f[2] = was_stopped; f[3] = 0;
  if (!was_stopped) { a.yaw_last[b] = yaw; if (unsafe) a.stopped[b] = 1; }      // a stopped instance's controller state is frozen; the failing tick itself still issues its command (QMController.cpp:165)
}

struct QmTickPackArgs {
  int B, controller, tick, mpc_ran, strict; double arm_kp, arm_kd;
  const double* x_obs; const double* x_des; const double* u_des; const int* mode; const double* wbc_out; const int* qp_status;      // observation, QmWbcBuffers
  const double* out_perf; const int* status; const double* step_info; const int* n_nodes;                                            // QmMpcBuffers
  const double* rbd; const double* time; const int* flags;                                                                           // measured state of this tick, qm_tick_state_kernel's words
  double* cmd; double* arm_hold; double* arm_last;      // tick-owned controller state: held command [B][90], QMMpcController's held arm positions / publication times [B][6]
  double* rec;                                          // [B][256] 8-byte words
};
__global__ void qm_tick_pack_kernel(QmTickPackArgs a) {
  const int b = blockIdx.x, f = threadIdx.x;
  if (b >= a.B) return;
  double* r = a.rec + (size_t)b * (QM_TICK_BYTES / 8);
  const bool stopped = a.flags[(size_t)b * QM_TICK_FLAGS + 2] != 0;
  if (f < QM_NJ) {      // updateControlLaw for joint f (qm_command_kernel's law), then the joint's five words of the held command into the record
    const int j = f; double* c = a.cmd + (size_t)b * 90;
    if (!stopped) {
      const double pos = a.x_des[(size_t)b * 30 + 12 + j], vel = a.u_des[(size_t)b * 30 + 12 + j], tau = a.wbc_out[(size_t)b * QM_NWBC_OUT + 36 + j], t = a.time[b];
      if (a.controller == 1) {
        if (j < 12) { c[j] = pos; c[18 + j] = vel; c[36 + j] = 0.0; c[54 + j] = 3.0; c[72 + j] = tau; }
        else {
          const int k = b * 6 + (j - 12); const double q = a.rbd[(size_t)b * QM_NRBD + 6 + j];
          if (a.tick == 0) { a.arm_hold[k] = q; a.arm_last[k] = t; }      // QMController::starting (QMController.cpp:127): hold the measured arm pose, last_time_ = the first observation's time
          double hold = a.arm_hold[k];
          if (t - a.arm_last[k] > 1.0 / 100.0) { hold = q + vel * 1.0 / 100.0; a.arm_hold[k] = hold; a.arm_last[k] = t; }
          c[j] = hold; c[18 + j] = 0.0; c[36 + j] = a.arm_kp; c[54 + j] = a.arm_kd; c[72 + j] = 0.0;
        }
      } else if (j < 12) { if (t > 10.0) { c[j] = pos; c[18 + j] = vel; c[36 + j] = 0.0; c[54 + j] = 3.0; c[72 + j] = tau; } }
      else { c[j] = pos; c[18 + j] = 0.0; c[36 + j] = a.arm_kp; c[54 + j] = a.arm_kd; c[72 + j] = tau; }
    }
    for (int k = 0; k < 5; ++k) r[QM_TICK_CMD + 18 * k + j] = c[18 * k + j];
    return;
  }
  const int g = f - QM_NJ + QM_TICK_XOBS;      // word of the record behind cmd
  if (g < QM_TICK_XDES) r[g] = a.x_obs[(size_t)b * 30 + g - QM_TICK_XOBS];
  else if (g < QM_TICK_UDES) r[g] = a.x_des[(size_t)b * 30 + g - QM_TICK_XDES];
  else if (g < QM_TICK_WBC) r[g] = a.u_des[(size_t)b * 30 + g - QM_TICK_UDES];
  else if (g < QM_TICK_PERF) r[g] = a.wbc_out[(size_t)b * QM_NWBC_OUT + g - QM_TICK_WBC];
  else if (g < QM_TICK_DOUBLES) r[g] = a.mpc_ran ? a.out_perf[(size_t)b * 10 + g - QM_TICK_PERF] : 0.0;
  else if (g < QM_TICK_DOUBLES + QM_TICK_INTS) {
    const int i = g - QM_TICK_DOUBLES; const int* fl = a.flags + (size_t)b * QM_TICK_FLAGS; int v = 0;
    if (i == QM_TICK_I_MODE) v = a.mode[b]; else if (i == QM_TICK_I_MEAS) v = fl[0];
    else if (i == QM_TICK_I_STATUS) v = qm_mpc_status(a.status[b], a.step_info + (size_t)b * 4, a.strict != 0); else if (i == QM_TICK_I_NODES) v = a.n_nodes[b];
    else if (i >= QM_TICK_I_QP && i < QM_TICK_I_QP + 3) v = a.qp_status[(size_t)b * 3 + i - QM_TICK_I_QP];
    else if (i == QM_TICK_I_SAFETY) v = fl[1]; else if (i == QM_TICK_I_STOPPED) v = fl[2]; else if (i == QM_TICK_I_MPCRAN) v = a.mpc_ran; else if (i == QM_TICK_I_TICK) v = a.tick;
    ((int*)(r + QM_TICK_DOUBLES))[i] = v;
  }
}
