// k_rollout.h — POLICY ROLLOUT (qmhip_policy_rollout, include/qmhip.h): MPC_MRT_Interface::rolloutPolicy [upstream, recalled] — the rollout QMController initialises at
// qm_controllers/src/QMController.cpp:311 (initRollout(&qmInterface_->getRollout()), a TimeTriggeredRollout over QMDynamicsAD, qm_interface/src/QMInterface.cpp:73,136-137,
// task.info:127-136) — batched: the SRBD flow map integrated forward from a state that is NOT the plan's, under the feed-forward policy or the SQP's linear controller, with a
// summary folded over the evaluation points.  Not upstream's adaptive ODE45: the input is held over a step (zero-order hold) and the step is the transcription's Heun rule
// (ilqr_rk2_lane, k_ilqr.h) — the discrete model the Riccati gains were computed for.
//
// Row r (instance b = inst[r], start t0[r], x0[r], final time t_end[r]).  Evaluation points k = 0 .. K:
//   t_0 = t0,  t_{k+1} = min(t_k + max_step, e, t_end),  e = the first event time of b's schedule strictly greater than t_k          (accumulated exactly like this)
//   tau_k = t_k + QM_WEAK_EPS when t_k equals an event time bit for bit (a step that starts on an event sees the mode and the PostEvent node behind it), else t_k
//   x_des, u_ff = the feed-forward policy at tau_k;  mode_k = modes[grid_find_index(ev, tau_k)];  u_k = u_ff, or the linear controller at (tau_k, x_k) — the expressions of
//   qm_policy_fb_kernel / qm_policy_fb_pub_kernel through the same qm_fb_source_node / qm_fb_du<View>, an uncovered point of a publication falling back to u_ff
//   x_{k+1} = ilqr_rk2_lane(x_k, u_k, t_{k+1} − t_k) (as qm_ro_rk2_lane, below);  a non-finite x_{k+1} ends the rollout at point k.
// ONE WAVEFRONT per row (launch: R workgroups of 64), lanes < 30 carry the state / input components as in qm_ilqr_rollout_kernel.  Time is monotone: the event index and
// the grid bracket are carried forward, never rescanned.  The bracket of point k + 1 depends on time only and is formed (scalar work) in front of step k.
//
// Registers decide the rest.  The kernel is held to the 256 registers of two waves per SIMD (QM_MAX_VGPRS) without a private segment.  ilqr_rk2_lane as it stands does not
// fit: qm_ilqr_rollout_kernel takes 262 registers, and under the cap it spills 28 bytes per lane, as this kernel did with it — so the step is restated below
// (qm_ro_rk2_lane: same terms, same order, the base block's wave-uniform values in scalar registers; bit equality with ilqr_rk2_lane is tested on the host emulator).
// Beside that the kernel keeps its own state across a step small: NOTHING per lane but x_k and u_k stays in registers — the two fold registers are parked in 1 KB of LDS
// (each lane reads back its own slot: no barrier), the running time lives in scalar registers, and a bracket's six doubles per lane of the primal solution are loaded behind
// the step, next to the 60 - 120 doubles per lane of K and Px that qm_fb_du reads there anyway, not prefetched in front of it.  What derives from the lane index or from the
// model table is formed inside the loop (QM_LANE_OPAQUE, qm_table per step): hoisted out of it, it costs 70 more registers.  The fold runs per lane — a maximum over points
// of a maximum over lanes is the maximum over lanes of the per-lane maxima — in TWO registers: lanes 0 .. 29 fold |x − x_des| and |u − u_ff| of their component, lanes
// 32 .. 43 the cone margin, the normal force and the swing force of foot l & 3 (minima as maxima of the negated value); nine wave reductions ONCE, behind the last point.
// No atomics, no workgroup barrier, vector stores from lanes < 34 and lane 0.
#pragma once
#include "k_ilqr.h"
#include "k_publish.h"

struct QmPolicyRolloutArgs {
  const double* mb; const double* st;
  QmPolicyArgs p;                       // grid, primal solution and schedule of the solve (source 0) or of one publication slot (source 1); p.t / p.x_des / p.u_des / p.mode unused
  const double* gains; int W;           // stage records [B][nmax][SR_SIZE] (W = nmax) or published records [B][W][PR_SIZE]
  int R; const int* inst; const double* t0; const double* x0; const double* t_end;      // rows: [R], [R], [R][30], [R]
  double max_step; int max_steps, feedback, trace_cap;
  double* x_end; double* u_end; int* mode_end;      // [R][30], [R][30], [R]
  double* summary; double* trace; int* count;       // [R][QM_RS_WORDS], [R][trace_cap][QM_RT_WORDS] (null with trace_cap 0), [R]
};

// grid_policy_segment (k_grid.h) with the scan for `part` continued from the caller's last one: the same comparisons on the same nudged node times, hence the same segment
// and the same alpha as a scan from node 0; *outside: t lies outside [first, last] nudged node time.  *part is reset when the time went backwards (a step shorter than weakEpsilon behind an event)
__device__ __forceinline__ void qm_ro_segment(const double* node_t, const int* node_ev, int n, int B, int b, double t, int* part_io, int* index, double* alpha, bool* outside) {
  auto tt = [&](int i) { const int e = node_ev[i * B + b]; return node_t[i * B + b] + (e == QM_EV_POST ? QM_LIMIT_EPS : (e == QM_EV_PRE ? -QM_LIMIT_EPS : 0.0)); };
  int part = *part_io; if (part > n) part = n;
  if (part > 0 && !(tt(part - 1) < t)) part = 0;
  while (part < n && tt(part) < t) ++part;
  *part_io = part;
  *outside = part >= n || (part == 0 && !(t == tt(0)));      // behind the last node / in front of the first: the segment below clamps
  const int interval = (part == 0 && t == tt(0)) ? 0 : part - 1; const int last = n - 1;
  if (n <= 1) { *index = 0; *alpha = 1.0; }
  else if (interval >= 0) {
    if (interval < last) { const double len = tt(interval + 1) - tt(interval), till = tt(interval + 1) - t; *index = interval; *alpha = (len > 2.0 * QM_WEAK_EPS) ? till / len : ((till > 0.5 * len) ? 1.0 : 0.0); }
    else { *index = (last - 1 > 0) ? last - 1 : 0; *alpha = 0.0; }
  } else { *index = 0; *alpha = 1.0; }
}

// ilqr_flow_lane / ilqr_rk2_lane (k_ilqr.h) restated for two waves per SIMD: the same terms in the same order — the same bits — with the WAVE-UNIFORM values of the base
// block (rotation, centre of mass, angular velocity, Euler rates: 21 doubles every lane would hold in 42 vector registers) handed to scalar registers as soon as kin_base has
// formed them (qm_bcast of lane 0: two v_readlane, no arithmetic).  Scalar registers that do not fit are kept in the lanes of ONE vector register by the compiler, so the
// step fits 256 vector registers without a private segment; ilqr_flow_lane itself needs 262 and spills 28 bytes per lane under that cap
__device__ __forceinline__ double qm_ro_flow_lane(const double* mb, double xl, double ul, int l) {
  double xb[12], Kb[KW_LEG];
#pragma unroll
  for (int i = 0; i < 12; ++i) xb[i] = qm_bcast(xl, i);                 // momentum + base pose: wave-uniform
  kin_base<true>(mb, xb, Kb);
  double RB[9], COM[3], OM[3], RW[3], THD[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) RB[i] = qm_bcast(Kb[KW_RB + i], 0);
#pragma unroll
  for (int i = 0; i < 3; ++i) { COM[i] = qm_bcast(Kb[KW_COM + i], 0); OM[i] = qm_bcast(Kb[KW_OM + i], 0); RW[i] = qm_bcast(Kb[KW_RW + i], 0); THD[i] = qm_bcast(Kb[KW_THD + i], 0); }
  const int c = l & 3, frame = chain_to_contact(c);
  double q3[3];
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) q3[jj] = __shfl(xl, 12 + 3 * c + jj, 64);
  double Rp[9], pp[3], Rj[9], Rq[9], Rn[9], p[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rp[i] = RB[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) pp[i] = xb[6 + i];
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    const int j = 3 * c + jj;
    double t[3]; m3_mulv(Rp, mb + MB_JP + 3 * j, t);
    for (int i = 0; i < 3; ++i) pp[i] += t[i];
    m3_mul(Rp, mb + MB_JR + 9 * j, Rj);
    rot_axis_angle<true>(mb + MB_AXIS + 3 * j, q3[jj], Rq);
    m3_mul(Rj, Rq, Rn);
    for (int i = 0; i < 9; ++i) Rp[i] = Rn[i];
  }
  { double t[3]; m3_mulv(Rp, mb + MB_FP + 3 * frame, t); for (int i = 0; i < 3; ++i) p[i] = pp[i] + t[i]; }
  const double m = mb[MB_ROBOTMASS], im = 1.0 / m;
  double lin[3] = {0.0, 0.0, -9.81 * m}, ang[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                         // contacts in order, as flow_from_kin
    const int src = contact_to_chain(i);
    const double pf[3] = {qm_bcast(p[0], src), qm_bcast(p[1], src), qm_bcast(p[2], src)};
    const double F[3] = {qm_bcast(ul, 3 * i), qm_bcast(ul, 3 * i + 1), qm_bcast(ul, 3 * i + 2)};
    const double d[3] = {pf[0] - COM[0], pf[1] - COM[1], pf[2] - COM[2]};
    double cr[3]; v3_cross(d, F, cr);
    for (int k = 0; k < 3; ++k) { lin[k] += F[k]; ang[k] += cr[k]; }
  }
  double wr[3]; v3_cross(OM, RW, wr);
  double f12[12];
#pragma unroll
  for (int k = 0; k < 3; ++k) { f12[k] = lin[k] * im; f12[3 + k] = ang[k] * im; f12[6 + k] = xb[k] + wr[k]; f12[9 + k] = THD[k]; }
  double fl = (l < 30) ? ul : 0.0;                                      // joint rows: qdot_j = u_j
#pragma unroll
  for (int k = 0; k < 12; ++k) fl = (l == k) ? f12[k] : fl;
  return fl;
}
__device__ __forceinline__ double qm_ro_rk2_lane(const double* mb, double xl, double ul, double dt, int l) {
  const double f1 = qm_ro_flow_lane(mb, xl, ul, l);
  const double x2 = xl + dt * f1;
  const double f2 = qm_ro_flow_lane(mb, x2, ul, l);
  return xl + 0.5 * dt * f1 + 0.5 * dt * f2;
}

// V: the gain record's view (QmFbStageView / QmFbPubView), REC its size in doubles, PUB: the records are a publication's window (coverage predicate of qm_policy_fb_pub_kernel)
template <class V, int REC, bool PUB>
__global__ void __launch_bounds__(64) QM_MAX_VGPRS(256) qm_policy_rollout_kernel(QmPolicyRolloutArgs a) {
  __shared__ double park[2 * 64];      // the two fold registers of every lane across a step
  const int r = blockIdx.x, l = threadIdx.x & 63; const QmPolicyArgs& p = a.p;
  if (r >= a.R) return;
  const int b = a.inst[r];
  const int n = p.n_nodes[b]; const int B = p.B, nev = p.nev;
  const double* ev = p.ev + (size_t)b * nev; const int* modes = p.modes + (size_t)b * (nev + 1);
  const double t_end = a.t_end[r], fric = a.st[ST_FRIC_COEF], inf = __builtin_inf();
  const int wn = PUB ? ((a.W < n) ? a.W : n) : n;
  double t = a.t0[r], tn = t, e_next = inf;
  double xc = (l < 30) ? a.x0[(size_t)r * 30 + l] : 0.0, uc = 0.0;
  int k = 0, ke = 0, part = 0, events = 0, uncovered = 0, flags = 0, mode_k = 0; bool first = true, ended = false;
  // the folds: fa = |x − x_des| (lanes < 30), − cone margin (32 .. 35), − F_z (36 .. 39), swing |F|_inf (40 .. 43) of foot l & 3;  fb = |u − u_ff| (lanes < 30)
  double fa = (l >= 32 && l < 40) ? -inf : 0.0, fb = 0.0;
  for (;;) {
    // the lane index as the loop body sees it: opaque, so that what derives from it (component masks, rows and columns of the gain records, the leg chain of the flow map)
    // is formed where it is used — hoisted out of the loop it is spilled: 100 - 200 bytes of scratch per lane
    int le = l; QM_LANE_OPAQUE(le);
    const bool lx = le < 30; const int lq = lx ? le : 0, foot = le & 3, grp = le >> 2;      // grp 8: cone, 9: normal force, 10: swing force
    // ---- what depends on the time tn only (wave-uniform): query time, mode, next event, bracket ----
    while (ke < nev && ev[ke] < tn) ++ke;                                  // lower bound of tn, carried
    const bool on_event = ke < nev && ev[ke] == tn;
    const double tau = on_event ? tn + QM_WEAK_EPS : tn;
    int km = ke; while (km < nev && ev[km] < tau) ++km;                     // grid_find_index(ev, nev, tau)
    const int mode_n = modes[km];
    int kg = ke; while (kg < nev && ev[kg] <= tn) ++kg;                     // the first event strictly behind tn
    const double e_n = (kg < nev) ? ev[kg] : inf;
    int idx; double al; bool outside; qm_ro_segment(p.node_t, p.node_ev, n, B, b, tau, &part, &idx, &al, &outside);
    // ---- step k: x_{k+1} = RK2(x_k, u_k, t_{k+1} − t_k), u_k held ----
    if (!first) {
      park[le] = fa; park[64 + le] = fb;
      const double* mb = qm_table(a.mb);      // (formed per step: the model table's entries are loaded where the flow map uses them, not hoisted out of the loop and spilled)
      int ls = le; QM_LANE_OPAQUE(ls);
      double xn = qm_ro_rk2_lane(mb, xc, uc, tn - t, ls); xn = lx ? xn : 0.0;
      fa = park[le]; fb = park[64 + le];
      if (__ballot(!(fabs(xn) < inf)) != 0ull) { flags |= QM_ROLLOUT_NONFINITE; break; }      // x_end stays the last finite state, t the time reached
      xc = xn; t = tn; ++k; events += ended ? 1 : 0;
    }
    first = false; mode_k = mode_n; e_next = e_n;
    if (outside) flags |= QM_ROLLOUT_OUTSIDE;
    // ---- evaluation point k: the policy at (tau_k, x_k) ----
    const int i0 = idx, i1 = (n > 1) ? idx + 1 : idx;
    const size_t o0 = ((size_t)i0 * B + b) * 30 + lq, o1 = ((size_t)i1 * B + b) * 30 + lq;
    const double xs0 = p.xs[o0], xs1 = p.xs[o1], us0 = p.us[o0], us1 = p.us[o1];
    const bool cov = i0 < wn && i1 < wn;
    if (PUB && !cov) ++uncovered;
    const double xdes = al * xs0 + (1.0 - al) * xs1, uff = al * us0 + (1.0 - al) * us1;
    double un = uff;
    if (a.feedback != 0 && cov) {                                           // qm_policy_fb_kernel, statement for statement
      const int j0 = qm_fb_source_node(p.node_ev, n, B, b, i0), j1 = qm_fb_source_node(p.node_ev, n, B, b, i1);      // wave-uniform
      double u0 = us0, u1 = us1, du0 = 0.0;
      if (j0 >= 0) { const double dxl = lx ? xc - p.xs[((size_t)j0 * B + b) * 30 + lq] : 0.0; du0 = qm_fb_du<V>(a.gains + ((size_t)b * a.W + j0) * REC, dxl, le); u0 += du0; }
      if (j1 == j0) u1 += du0;
      else if (j1 >= 0) { const double dxl = lx ? xc - p.xs[((size_t)j1 * B + b) * 30 + lq] : 0.0; u1 += qm_fb_du<V>(a.gains + ((size_t)b * a.W + j1) * REC, dxl, le); }
      un = al * u0 + (1.0 - al) * u1;
    }
    uc = lx ? un : 0.0;
    // ---- fold ----
    { const double Fx = __shfl(uc, 3 * foot, 64), Fy = __shfl(uc, 3 * foot + 1, 64), Fz = __shfl(uc, 3 * foot + 2, 64); const bool st = mode_flag(mode_k, foot);
      const double vc = st ? -(fric * Fz - sqrt(Fx * Fx + Fy * Fy)) : -inf, vz = st ? -Fz : -inf, vs = st ? 0.0 : fmax(fabs(Fx), fmax(fabs(Fy), fabs(Fz)));
      const double va = lx ? fabs(xc - xdes) : ((grp == 8) ? vc : ((grp == 9) ? vz : ((grp == 10) ? vs : 0.0)));
      fa = fmax(fa, va); fb = fmax(fb, lx ? fabs(uc - uff) : 0.0); }
    // ---- trace: one sample per point k < trace_cap ----
    if (k < a.trace_cap) {
      double* s = a.trace + ((size_t)r * a.trace_cap + k) * QM_RT_WORDS;
      if (lx) { s[QM_RT_X + le] = xc; s[QM_RT_U + le] = uc; }
      // lane 30: the time, lane 31: mode | covered as one word, lanes 32, 33: the two spare words — one store with a per-lane address (stores of constants from one lane are merged
      // into a wide store of a constant vector, which is hoisted out of the loop and spilled)
      union { int i[2]; double d; } mc; mc.i[0] = mode_k; mc.i[1] = (!PUB || cov) ? 1 : 0;
      if (le >= 30 && le < 34) s[(le == 30) ? QM_RT_TIME : QM_RT_INTS + (le - 31)] = (le == 30) ? t : ((le == 31) ? mc.d : 0.0);
    }
    if (!(t < t_end)) break;
    if (k >= a.max_steps) { flags |= QM_ROLLOUT_MAX_STEPS; break; }
    tn = qm_bcast(fmin(fmin(t + a.max_step, e_next), t_end), 0); ended = tn == e_next;      // (wave-uniform, and kept in scalar registers: the vector ALU forms it)
  }
  // ---- results: x_K, u_K, mode_K, the folds reduced across the wave ----
  const int grp = l >> 2;
  if (l < 30) { a.x_end[(size_t)r * 30 + l] = xc; a.u_end[(size_t)r * 30 + l] = uc; }
  const double dv0 = qm_wave_max(l < 6 ? fa : 0.0), dv1 = qm_wave_max((l >= 6 && l < 12) ? fa : 0.0), dv2 = qm_wave_max((l >= 12 && l < 24) ? fa : 0.0), dv3 = qm_wave_max((l >= 24 && l < 30) ? fa : 0.0);
  const double fb0 = qm_wave_max(l < 12 ? fb : 0.0), fb1 = qm_wave_max((l >= 12 && l < 30) ? fb : 0.0);
  const double mc = -qm_wave_max(grp == 8 ? fa : -inf), mz = -qm_wave_max(grp == 9 ? fa : -inf), ms = qm_wave_max(grp == 10 ? fa : 0.0);
  if (l == 0) {
    a.mode_end[r] = mode_k; a.count[r] = k + 1;
    double* s = a.summary + (size_t)r * QM_RS_WORDS;
    s[QM_RS_T_END] = t; s[QM_RS_MAX_DEV] = dv0; s[QM_RS_MAX_DEV + 1] = dv1; s[QM_RS_MAX_DEV + 2] = dv2; s[QM_RS_MAX_DEV + 3] = dv3; s[QM_RS_MAX_FB] = fb0; s[QM_RS_MAX_FB + 1] = fb1;
    s[QM_RS_MIN_CONE] = mc; s[QM_RS_MIN_FZ] = mz; s[QM_RS_MAX_SWING] = ms; s[QM_RS_SPARE] = 0.0; s[QM_RS_SPARE + 1] = 0.0;
    int* si = (int*)(s + QM_RS_INTS); si[QM_RS_I_STEPS] = k; si[QM_RS_I_EVENTS] = events; si[QM_RS_I_UNCOVERED] = uncovered; si[QM_RS_I_FLAGS] = flags;
    si[QM_RS_I_SPARE] = 0; si[QM_RS_I_SPARE + 1] = 0; si[QM_RS_I_SPARE + 2] = 0; si[QM_RS_I_SPARE + 3] = 0;
  }
}
typedef void (*QmPolicyRolloutFn)(QmPolicyRolloutArgs);
