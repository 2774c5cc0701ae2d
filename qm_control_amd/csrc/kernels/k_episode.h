// k_episode.h — the episode monitor (qmhip_episode_*, include/qmhip.h): running statistics of every instance of a device loop, folded behind every tick from what
// the tick left resident (plant: rbd / contact / force / status; WBC: out / qp_status; the policy's mode; the MPC's status words), and a decimated trace of raw samples.
// Records: struct qmhip_episode_summary (32 words) and struct qmhip_episode_sample (64 words), include/qmhip_layout.h.  The kernels READ the loop's buffers and write
// only the monitor's own: a loop computes the same bits with the monitor on.
//
//   qm_episode_start_kernel  one thread per instance: the summary's initial values, the anchor pose and the contact flags "before the first tick"
//   qm_episode_tick_kernel   one WAVEFRONT per instance (grid = B, 64 threads; thread-per-instance glue of this loop is pure latency): lane l holds word l of
//                            rbd (55), of the WBC output (54) and of the summary (32); the per-tick quantities are wave reductions (qm_wave_sum / qm_wave_max: DPP, a
//                            FIXED lane order, so a rerun gives the same bits) whose results every lane holds; lane l then updates summary word l and stores it.  A sample
//                            is one 64-lane, 512-byte store.  No LDS, no barrier, no atomics, no private segment
//   qm_episode_mpc_kernel    one thread per instance, once per MPC call: the call's status word (qm_mpc_status) into the four MPC words of the summary
//
// Fall rule: the fall check comes first.  An instance that has fallen (on this tick or before) advances `ticks` and `t_last` only; the tick that trips the check is NOT
// folded into maxima, sums and counters — so a non-finite state never reaches an accumulator.
#pragma once
#include <cfloat>
#include "qm_dev_common.h"

__host__ __device__ inline int qm_mpc_status(int k0_status, const double* step_info4, bool strict);      // csrc/host/qm_pipeline.h

// two int32 in one 8-byte word (lo at the lower address) and back
__device__ __forceinline__ double qm_ep_pack(int lo, int hi) {
  const unsigned long long v = (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32); double d; __builtin_memcpy(&d, &v, 8); return d;
}
__device__ __forceinline__ int qm_ep_lo(double d) { unsigned long long v; __builtin_memcpy(&v, &d, 8); return (int)(unsigned)(v & 0xffffffffull); }
__device__ __forceinline__ int qm_ep_hi(double d) { unsigned long long v; __builtin_memcpy(&v, &d, 8); return (int)(unsigned)(v >> 32); }

// initial values of an episode.  rbd: the state the anchor is taken from (its end-effector pose rbd[48:55]) or null: the anchor stays as qmhip_episode_set_anchor left
// it.  contact: the flags "before the first tick" or null: flags[0] = -1, the first folded tick then takes its own flags (no transition on it)
struct QmEpisodeStartArgs { int B; const double* rbd; const int* contact; double* summary; double* anchor; int* flags; };
__global__ void __launch_bounds__(64) qm_episode_start_kernel(QmEpisodeStartArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  double* s = a.summary + (size_t)b * QM_EP_WORDS;
  for (int k = 0; k < QM_EP_WORDS; ++k) s[k] = 0.0;
  s[EP_MIN_BASE_Z] = (double)INFINITY;
  s[EP_INTS + EP_I_TICKS / 2] = qm_ep_pack(0, -1);                 // ticks | fall_tick
  s[EP_INTS + EP_I_MPC_FIRST_FAIL / 2] = qm_ep_pack(-1, 0);        // mpc_first_fail_tick | reserved
  if (a.rbd) for (int k = 0; k < 7; ++k) a.anchor[(size_t)b * 7 + k] = a.rbd[(size_t)b * QM_NRBD + 48 + k];
  int m = -1;
  if (a.contact) { m = 0; for (int k = 0; k < 4; ++k) m |= a.contact[(size_t)b * 4 + k] != 0 ? (8 >> k) : 0; }
  a.flags[2 * b] = m; a.flags[2 * b + 1] = 0;                      // contact mask before the first tick | the last folded MPC status
}

struct QmEpisodeTickArgs {
  const double* mb; int B, tick, trace_every, trace_cap;      // tick: index of the folded tick since the episode's start; trace_every 0: no trace
  double period, min_base_z, max_tilt;
  const double* time; const double* rbd; const int* contact; const double* force;      // the plant BEHIND the tick: [B], [B][55], [B][4], [B][12]
  const int* mode; const double* wbc_out; const int* qp_status;                         // what the tick's policy / WBC returned: [B], [B][54], [B][3]
  const int* sim_status;                                                                // [B] or null
  double* summary; const double* anchor; int* flags; double* trace;                     // [B][32], [B][7], [B][2], [trace_cap][B][64]
};
__global__ void __launch_bounds__(64) qm_episode_tick_kernel(QmEpisodeTickArgs a) {
  const int b = blockIdx.x, l = threadIdx.x & 63;
  if (b >= a.B) return;
  const double* rb = a.rbd + (size_t)b * QM_NRBD; const double* fo = a.force + (size_t)b * 12; double* sm = a.summary + (size_t)b * QM_EP_WORDS;
  const bool jl = l >= 36 && l < 54, fl = l < 4, al = l >= 48 && l < 55;      // lane of joint l - 36 (its torque is word l of the WBC output) / of foot l / of end-effector word l - 48
  double r = 0.0, wv = 0.0, w = 0.0, qd = 0.0, tmax = 1.0, an = 0.0, fx = 0.0, fy = 0.0, fz = 0.0; int ct = 0;
  if (l < QM_NRBD) r = rb[l];
  if (l < QM_NWBC_OUT) wv = a.wbc_out[(size_t)b * QM_NWBC_OUT + l];
  if (l < QM_EP_WORDS) w = sm[l];
  if (jl) { qd = rb[l - 6]; tmax = a.mb[MB_TAUMAX + l - 36]; }                 // rbd[30 + j]
  if (al) an = a.anchor[(size_t)b * 7 + l - 48];
  if (fl) { fx = fo[3 * l]; fy = fo[3 * l + 1]; fz = fo[3 * l + 2]; ct = a.contact[(size_t)b * 4 + l]; }
  const double time = a.time[b]; const int mode = a.mode[b], simst = a.sim_status ? a.sim_status[b] : 0;
  const int qp0 = a.qp_status[(size_t)b * 3], qp1 = a.qp_status[(size_t)b * 3 + 1], qp2 = a.qp_status[(size_t)b * 3 + 2];
  const int prev_raw = a.flags[2 * b], last_status = a.flags[2 * b + 1];
  const double hdr = qm_bcast(w, EP_INTS); const int ticks = qm_ep_lo(hdr), fall_tick = qm_ep_hi(hdr);

  // measured contact mask 8 LF + 4 RF + 2 LH + RH
  const unsigned long long cb = __ballot(fl && ct != 0);
  const int mask = (int)(((cb & 1ull) << 3) | ((cb & 2ull) << 1) | ((cb & 4ull) >> 1) | ((cb & 8ull) >> 3));
  const int prev = prev_raw < 0 ? mask : prev_raw;

  // ---- fall check (strict comparisons; a NaN compares false and is caught by the finiteness test) ----
  const bool nonfinite = __ballot(!(fabs(r) <= DBL_MAX)) != 0ull;
  const double z = qm_bcast(r, 5), roll = fabs(qm_bcast(r, 2)), pitch = fabs(qm_bcast(r, 1));
  const int cause = (z < a.min_base_z ? QM_FALL_HEIGHT : 0) | (roll > a.max_tilt ? QM_FALL_ROLL : 0) | (pitch > a.max_tilt ? QM_FALL_PITCH : 0) | (nonfinite ? QM_FALL_NONFINITE : 0);
  const bool newly = fall_tick < 0 && cause != 0, live = fall_tick < 0 && cause == 0;

  // ---- the tick's quantities, in every lane ----
  const double speed = sqrt(qm_wave_sum((l >= 27 && l < 30) ? r * r : 0.0));
  const double dp = (l >= 48 && l < 51) ? r - an : 0.0; const double ee2 = qm_wave_sum(dp * dp), eed = sqrt(ee2);
  const bool ql = l >= 51 && l < 55; const double dm = ql ? r - an : 0.0, dq = ql ? r + an : 0.0;
  const double ang = 4.0 * asin(0.5 * sqrt(fmin(qm_wave_sum(dm * dm), qm_wave_sum(dq * dq))));      // rotation angle between q and ±q_a, well conditioned near zero
  const double tau_ratio = qm_wave_max(jl ? fabs(wv) / tmax : 0.0);
  const double work = a.period * qm_wave_sum(jl ? fabs(wv * qd) : 0.0);
  const double friction = qm_wave_max((fl && fz > 0.0) ? sqrt(fx * fx + fy * fy) / fz : 0.0);
  const double normal = qm_wave_max(fl ? fz : 0.0);      // (the maximum starts at 0)
  const int mismatch = mask ^ (mode & 15), touchdown = mask & ~prev & 15;

  // ---- lane l: summary word l ----
  double nw = w;
  if (l == EP_T_FIRST && ticks == 0) nw = time;
  if (l == EP_T_LAST) nw = time;
  if (l == EP_T_FALL && newly) nw = time;
  if (live) {
    if (l == EP_MIN_BASE_Z) nw = fmin(w, z);
    if (l == EP_MAX_ROLL) nw = fmax(w, roll);
    if (l == EP_MAX_PITCH) nw = fmax(w, pitch);
    if (l == EP_MAX_SPEED) nw = fmax(w, speed);
    if (l == EP_MAX_EE_POS) nw = fmax(w, eed);
    if (l == EP_SUMSQ_EE_POS) nw = w + ee2;
    if (l == EP_MAX_EE_ANG) nw = fmax(w, ang);
    if (l == EP_MAX_TAU_RATIO) nw = fmax(w, tau_ratio);
    if (l == EP_MAX_FRICTION) nw = fmax(w, friction);
    if (l == EP_MAX_NORMAL) nw = fmax(w, normal);
    if (l == EP_JOINT_WORK) nw = w + work;
  }
  if (l >= EP_INTS) {
    int lo = qm_ep_lo(w), hi = qm_ep_hi(w); const int k = 2 * (l - EP_INTS);      // index of this word's lower int32 (the MPC words EP_I_MPC_CALLS .. EP_I_RESERVED keep their values)
    if (k == EP_I_TICKS) { lo += 1; if (newly) hi = a.tick; }
    if (k == EP_I_FALL_CAUSE) { if (newly) lo = cause; if (live && simst != 0) hi += 1; }
    if (live) {
      if (k == EP_I_WBC_BAD) { lo += qp0 != 0; hi += qp1 != 0; }
      if (k == EP_I_WBC_BAD + 2) { lo += qp2 != 0; hi += mask == 0; }
      if (k == EP_I_MISMATCH) { lo += (mismatch >> 3) & 1; hi += (mismatch >> 2) & 1; }
      if (k == EP_I_MISMATCH + 2) { lo += (mismatch >> 1) & 1; hi += mismatch & 1; }
      if (k == EP_I_TOUCHDOWN) { lo += (touchdown >> 3) & 1; hi += (touchdown >> 2) & 1; }
      if (k == EP_I_TOUCHDOWN + 2) { lo += (touchdown >> 1) & 1; hi += touchdown & 1; }
      if (k == EP_I_TAU_OVER) lo += tau_ratio > 1.0;
    }
    nw = qm_ep_pack(lo, hi);
  }
  if (l < QM_EP_WORDS) sm[l] = nw;
  if (l == 0 && live) a.flags[2 * b] = mask;

  // ---- trace: a raw copy of the tick, fallen or not ----
  if (a.trace_every > 0 && a.tick % a.trace_every == 0 && a.tick / a.trace_every < a.trace_cap) {
    double v;
    if (l == ES_TIME) v = time;
    else if (l < ES_FORCE_Z) v = rb[l - ES_RBD];
    else if (l < ES_INTS) v = fo[3 * (l - ES_FORCE_Z) + 2];
    else v = l == ES_INTS ? qm_ep_pack(a.tick, mode) : l == ES_INTS + 1 ? qm_ep_pack(mask, last_status) : l == ES_INTS + 2 ? qm_ep_pack(qp0, qp1) : qm_ep_pack(qp2, simst);
    a.trace[((size_t)(a.tick / a.trace_every) * a.B + b) * QM_ES_WORDS + l] = v;
  }
}

// One MPC call, folded behind it.  tick: the tick the call observed at; the call counts iff the instance had not fallen BEFORE that tick — the same rule in the
// synchronous loop (folded on the MPC tick, before that tick's fold) and in the pipelined one (folded an MPC period later, behind the publication).  step_info null:
// `status` already holds the status words (qmhip_episode_fold).  flags[1], the status the samples carry, is a raw copy: written fallen or not
struct QmEpisodeMpcArgs { int B, tick, strict; const int* status; const double* step_info; double* summary; int* flags; };
__global__ void __launch_bounds__(64) qm_episode_mpc_kernel(QmEpisodeMpcArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const int s = a.step_info ? qm_mpc_status(a.status[b], a.step_info + (size_t)b * 4, a.strict != 0) : a.status[b];
  a.flags[2 * b + 1] = s;
  int* si = (int*)(a.summary + (size_t)b * QM_EP_WORDS + EP_INTS);
  const int ft = si[EP_I_FALL_TICK];
  if (ft != -1 && ft < a.tick) return;
  si[EP_I_MPC_CALLS] += 1;
  if (s < 0) { si[EP_I_MPC_FAILS] += 1; si[EP_I_MPC_LAST_FAIL] = s; if (si[EP_I_MPC_FIRST_FAIL] == -1) si[EP_I_MPC_FIRST_FAIL] = a.tick; }
  else if (s > 0) si[EP_I_MPC_WARN_OR] |= s;
}
