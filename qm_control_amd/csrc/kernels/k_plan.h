// k_plan.h — a plan in task space (qmhip_plan_task_space / qmhip_plan_footholds / qmhip_task_space_eval, include/qmhip.h): the arithmetic of qm::QmVisualizer
// (qm_interface/src/visualization/qm_visualization.cpp:72-317) without its messages.  Per (state, input, mode) one 64-word record (struct qmhip_plan_record,
// include/qmhip_layout.h): the four feet — position, velocity as the zero- / normal-velocity constraints see it, contact force —, the arm's end-effector pose and
// its error against a reference, the centre of pressure.  The kinematics is NOT restated: kin_base / kin_leg / kin_arm / foot_velocity / ee_error_arm (qm_dev_kin.h)
// as K1a (k_lq.h) and qm_measured_body (k_policy.h) call them.
//
//   qm_plan_nodes_kernel      one thread per (node, instance) of the primal solution [nmax][B][30]; K1a's mapping: a wave's 64 consecutive rows come in together
//                             through a [64][31] LDS tile (kin_rows_in) and its 64 records leave as whole 64-byte lines through a [64][9] tile
//   qm_plan_states_kernel     the same rows routine on caller-supplied rows [R][30] (target knots, an observation)
//   qm_plan_footholds_kernel  one thread per (instance, schedule event): the plan interpolated at the event, the landing feet's positions
// The two row kernels are ONE inlined routine behind two entry points, so a state evaluated through either gets the same bits (the same function inlined into two
// different kernels may contract its FMAs differently: ADVICE.md, k_tick.h).  No atomics, no s_barrier (wave-level ordering only), no private-segment traffic.
#pragma once
#include "k_grid.h"
#include "k_lq.h"      /* kin_rows_in */
#include "qm_dev_kin.h"

#ifndef QM_PLAN_WAVES
#define QM_PLAN_WAVES 2      /* waves per SIMD the row kernels are built for (256 registers) */
#endif
#define QM_PLAN_SLACK 64     /* records behind the last row of a record buffer: a wave stores whole 64-record blocks */
#define QM_PLAN_TILE (64 * 31)                              /* [64][31]: the wave's states on their way in, then each thread's input row for the whole kernel */
#define QM_PLAN_LDS_BYTES ((QM_PLAN_TILE + 64 * 9) * 8)     /* + the [64][9] hand-over tile of the record stores: 20 KB per wave */

// two int32 in one 8-byte word (lo at the lower address)
__device__ __forceinline__ double qm_plan_pack2(int lo, int hi) {
  const unsigned long long v = (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32); double d; __builtin_memcpy(&d, &v, 8); return d;
}
// bit i = foot i (LF RF LH RH) in stance: modeNumber2StanceLeg [upstream ocs2_legged_robot MotionPhaseDefinition] as a mask
__device__ __forceinline__ int qm_plan_contact_mask(int mode) { int m = 0; for (int k = 0; k < 4; ++k) m |= mode_flag(mode, k) ? (1 << k) : 0; return m; }

// One record from one (state, input, mode): w[QM_PLAN_WORDS] thread-private, every index static (it lives in registers).  x in registers, u anywhere (an LDS row in
// the row kernels).  ee: the reference pose [pos(3), quat xyzw(4)] or null.  feet: mask of the feet whose kinematics is wanted (the words of the others and, without
// `arm`, the end-effector words stay as the caller left them) — the row kernels pass all four, the foothold kernel the landing feet.  PT_TIME is the caller's, set
// before the call.  Ordered for a small live set (two waves per SIMD, like K1a): the legs one at a time, then leave(0, 5) — words [0, 40) are final and the caller may
// hand them over, which frees the feet's registers —, then the arm, then leave(5, 8)
template <class Leave>
__device__ __forceinline__ void qm_plan_body(const double* mb, const double (&x)[30], const double* u, const int mode, const double* ee, double (&w)[QM_PLAN_WORDS], Leave leave, const int feet = 15, const bool arm = true) {
  double K[KW_SIZE];
  const int mask = qm_plan_contact_mask(mode);
  w[PT_MODE] = qm_plan_pack2(mode, mask);
  _Pragma("unroll") for (int q = 0; q < 3; ++q) { w[PT_BASE_POS + q] = x[6 + q]; w[PT_BASE_ZYX + q] = x[9 + q]; }
  kin_base<true>(mb, x, K);
  // centre of pressure over the stance feet, in foot order ([upstream getCenterOfPressureMarker, recalled]): Σ f_z p_xy / Σ f_z; without a positive Σ f_z (flight
  // phase, a pulling plan) the point is the origin and cop[2] keeps the sum
  double sx = 0.0, sy = 0.0, sz = 0.0;
  _Pragma("unroll") for (int k = 0; k < 4; ++k) {
    if ((feet >> k) & 1) {
      kin_leg<true>(mb, contact_to_chain(k), x, u, K);
      const double* p = kin_foot(K, k); double v[3]; foot_velocity(x, K, k, v);
      _Pragma("unroll") for (int q = 0; q < 3; ++q) { w[PT_FOOT_POS + 3 * k + q] = p[q]; w[PT_FOOT_VEL + 3 * k + q] = v[q]; }
      const double fz = u[3 * k + 2];
      if ((mask >> k) & 1) { sx += fz * p[0]; sy += fz * p[1]; sz += fz; }
    }
    _Pragma("unroll") for (int q = 0; q < 3; ++q) w[PT_FOOT_FORCE + 3 * k + q] = u[3 * k + q];
    __builtin_amdgcn_sched_barrier(0);      // one leg at a time (k_ls.h: scheduled together, the four chains' temporaries do not fit)
  }
  const bool press = sz > 0.0; const double isz = 1.0 / (press ? sz : 1.0);
  w[PT_COP] = press ? sx * isz : 0.0; w[PT_COP + 1] = press ? sy * isz : 0.0; w[PT_COP + 2] = sz;
  leave(0, 5);
  __builtin_amdgcn_sched_barrier(0);
  if (arm) {
    kin_arm<true>(mb, x, K);
    double qee[4], g6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ee) ee_error_arm(K + KW_ARM, ee, ee + 3, qee, g6); else mat_to_quat(K + KW_ARM + 39, qee);
    _Pragma("unroll") for (int q = 0; q < 3; ++q) w[PT_EE_POS + q] = K[KW_ARM + 36 + q];
    _Pragma("unroll") for (int q = 0; q < 4; ++q) w[PT_EE_QUAT + q] = qee[q];
    _Pragma("unroll") for (int q = 0; q < 6; ++q) w[PT_EE_ERR + q] = g6[q];
  }
  _Pragma("unroll") for (int q = 0; q < 4; ++q) w[PT_SPARE + q] = 0.0;
  leave(5, 8);
}

// rows [nrows][30] -> records [nrows][64].  Node-major solver arrays: row g = i B + b is node i of instance b and holds zeros at or behind n_nodes[b]; caller-supplied
// rows: n_nodes null (every row counts), B = 1
struct QmPlanRowsArgs {
  const double* mb; long long nrows; int B;
  const double* x; const double* u;      // [nrows][30]; u null: zero inputs
  const int* mode;                       // [nrows]
  const double* ee;                      // [nrows][7] or null: no reference, ee_err = 0
  const double* time;                    // [nrows] or null: 0
  const int* n_nodes;                    // [B] or null
  double* rec;                           // [nrows + QM_PLAN_SLACK][QM_PLAN_WORDS]
};
// One THREAD per row, the wave's rows moved together.  No thread leaves before the last cooperative access: a thread without a row of its own (behind the arrays' end,
// behind its instance's last node) helps to move data and hands over zeros.  A wave none of whose rows counts stores its zeros and leaves at once
__device__ __forceinline__ void qm_plan_rows(const QmPlanRowsArgs& a) {
  const int l = threadIdx.x & 63;
  const size_t g0 = (size_t)blockIdx.x * 64, nrows = (size_t)a.nrows;      // first row of this wave's block (blockDim.x == 64)
  if (g0 >= nrows) return;
  size_t g = g0 + l; const bool inrange = g < nrows; if (!inrange) g = nrows - 1;
  const int i = (int)(g / a.B), b = (int)(g - (size_t)i * a.B);
  const bool valid = inrange && (!a.n_nodes || i < a.n_nodes[b]);
  if (__ballot(valid) == 0ull) {
    _Pragma("unroll 8") for (int k = 0; k < 64; ++k) { const size_t r = g0 + k; if (r < nrows) a.rec[r * QM_PLAN_WORDS + l] = 0.0; }      // lane l: word l of every record of the block
    return;
  }
  const double* mb = qm_table(a.mb);
  extern __shared__ double qm_smem[];                  // QM_PLAN_LDS_BYTES
  double* rows = qm_smem; double* tile = qm_smem + QM_PLAN_TILE; double* u = rows + l * 31;
  double x[30], w[QM_PLAN_WORDS];
  kin_rows_in(rows, a.x, g0, nrows, l); qm_wave_sync();
  _Pragma("unroll") for (int q = 0; q < 30; ++q) x[q] = u[q];
  qm_wave_sync();
  if (a.u) kin_rows_in(rows, a.u, g0, nrows, l); else { for (int q = 0; q < 30; ++q) u[q] = 0.0; }
  qm_wave_sync();
  // the records leave in eight pieces of eight words: thread l puts its piece into row l of the [64][9] tile, then lanes 8 r' + j store word j of the piece of record
  // 8 k + r' — every store instruction writes eight whole 64-byte lines, unmasked (kin_emit, k_lq.h: exec masks around the stores cost this kernel 190 registers and
  // 772 bytes of scratch): the record buffer carries QM_PLAN_SLACK records behind its last row for the last wave of a launch
  const int j = l & 7, rr = l >> 3;
  auto leave = [&](const int p0, const int p1) {
    _Pragma("unroll") for (int p = p0; p < p1; ++p) {
      _Pragma("unroll") for (int q = 0; q < 8; ++q) tile[l * 9 + q] = valid ? w[8 * p + q] : 0.0;
      qm_wave_sync();
      _Pragma("unroll") for (int k = 0; k < 8; ++k) { const int r = 8 * k + rr; a.rec[(g0 + r) * QM_PLAN_WORDS + 8 * p + j] = tile[r * 9 + j]; }
      qm_wave_sync();
    }
  };
  w[PT_TIME] = a.time ? a.time[g] : 0.0;
  qm_plan_body(mb, x, u, a.mode[g], a.ee ? a.ee + g * 7 : nullptr, w, leave);
}
__global__ void __launch_bounds__(64, QM_PLAN_WAVES) qm_plan_nodes_kernel(QmPlanRowsArgs a) { qm_plan_rows(a); }
__global__ void __launch_bounds__(64, QM_PLAN_WAVES) qm_plan_states_kernel(QmPlanRowsArgs a) { qm_plan_rows(a); }

// "Future footholds" (qm_visualization.cpp:150-182).  Thread (b, e): schedule event e of instance b, handled when t_first < ev[e] < t_last of the instance's grid (the
// two strict inequalities of qm_visualization.cpp:163): the state interpolated linearly at ev[e] (grid_policy_segment: the bracketing of qm_policy_kernel, i.e.
// LinearInterpolation::interpolate; event nodes are identity jumps, so either side of a duplicated time gives the same state) and kin_leg of each foot that is off in
// modes[e] and on in modes[e + 1].  The slot of a landing is COMPUTED — landings of the earlier events + lower landing feet of this one, the prefix recounted from
// the mode pairs (nev is small) — so the list is ordered by (event, foot) without atomics.  count[b] is the full number; slots >= cap are not written
struct QmPlanFootArgs {
  const double* mb; int B, nmax, nev, cap;
  const int* n_nodes; const double* node_t; const int* node_ev; const double* xs;      // grid + primal solution, node-major
  const double* ev; const int* modes;                                                   // schedule [B][nev], [B][nev + 1]
  double* out;      // [B][cap][5] 8-byte words: time | leg, event (int32) | pos[3]  (struct qmhip_foothold)
  int* count;       // [B]
};
__device__ __forceinline__ int qm_plan_landing(const int* modes, int e) { const int m0 = modes[e], m1 = modes[e + 1]; return ~qm_plan_contact_mask(m0) & qm_plan_contact_mask(m1) & 15; }
__global__ void __launch_bounds__(64) qm_plan_footholds_kernel(QmPlanFootArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.B * a.nev) return;
  const int b = g / a.nev, e = g - b * a.nev;
  const int n = a.n_nodes[b]; const double* ev = a.ev + (size_t)b * a.nev; const int* modes = a.modes + (size_t)b * (a.nev + 1);
  const bool has = n >= 1 && n <= a.nmax;
  const double t_first = has ? a.node_t[b] : 0.0, t_last = has ? a.node_t[(size_t)(n - 1) * a.B + b] : 0.0;
  int slot = 0;
  for (int k = 0; k < e; ++k) if (has && t_first < ev[k] && ev[k] < t_last) slot += __popcll((unsigned long long)qm_plan_landing(modes, k));
  const double te = ev[e]; const bool in = has && t_first < te && te < t_last;
  const int land = in ? qm_plan_landing(modes, e) : 0;
  if (e == a.nev - 1) a.count[b] = slot + __popcll((unsigned long long)land);
  if (land == 0 || slot >= a.cap) return;
  int idx; double al; grid_policy_segment(a.node_t, a.node_ev, n, a.B, b, te, &idx, &al);
  const size_t i0 = (size_t)idx * a.B + b, i1 = (size_t)(n > 1 ? idx + 1 : idx) * a.B + b;
  double x[30], u[30], w[QM_PLAN_WORDS];
  _Pragma("unroll") for (int q = 0; q < 30; ++q) { x[q] = al * a.xs[i0 * 30 + q] + (1.0 - al) * a.xs[i1 * 30 + q]; u[q] = 0.0; }
  qm_plan_body(qm_table(a.mb), x, u, modes[e + 1], nullptr, w, [](int, int) {}, land, false);
  _Pragma("unroll") for (int k = 0; k < 4; ++k) if ((land >> k) & 1) {
    if (slot < a.cap) { double* o = a.out + ((size_t)b * a.cap + slot) * (QM_FOOTHOLD_BYTES / 8); o[0] = te; o[1] = qm_plan_pack2(k, e); o[2] = w[PT_FOOT_POS + 3 * k]; o[3] = w[PT_FOOT_POS + 3 * k + 1]; o[4] = w[PT_FOOT_POS + 3 * k + 2]; }
    ++slot;
  }
}
