// k_policy.h — K5: policy evaluation (MPC_MRT_Interface::evaluatePolicy [upstream], call site
// qm_controllers/src/QMController.cpp:139-142) and the synthetic measured state of the benchmark step.
// One thread per instance.
#pragma once
#include "k_grid.h"
#include "qm_dev_kin.h"

struct QmPolicyArgs {
  const double* mb;
  int B, nmax, nev;
  const int* n_nodes; const double* node_t; const int* node_ev;   // grid
  const double* xs; const double* us;                              // primal solution [nmax][B][30]
  const double* ev; const int* modes;                              // schedule [B][nev], [B][nev+1]
  const double* t;                                                 // [B] evaluation time (t0 for the benchmark step)
  double* x_des; double* u_des; int* mode;                         // [B][30], [B][30], [B]
};

__device__ __forceinline__ void qm_policy_body(const QmPolicyArgs& a, const int b) {
  const int n = a.n_nodes[b]; const double t = a.t[b];
  int idx; double al; grid_policy_segment(a.node_t, a.node_ev, n, a.B, b, t, &idx, &al);
  const int i0 = idx * a.B + b, i1 = ((n > 1 ? idx + 1 : idx)) * a.B + b;
  for (int q = 0; q < 30; ++q) { a.x_des[(size_t)b * 30 + q] = al * a.xs[i0 * 30 + q] + (1.0 - al) * a.xs[i1 * 30 + q]; a.u_des[(size_t)b * 30 + q] = al * a.us[i0 * 30 + q] + (1.0 - al) * a.us[i1 * 30 + q]; }
  a.mode[b] = a.modes[(size_t)b * (a.nev + 1) + grid_find_index(a.ev + (size_t)b * a.nev, a.nev, t)];
}
__global__ void qm_policy_kernel(QmPolicyArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  qm_policy_body(a, b);
}

// measured rbd state (55) built from x0: zero velocities, EE pose by FK (layout of
// qm_estimation/src/StateEstimateBase.cpp:41-103)
struct QmMeasArgs { const double* mb; int B; const double* x0; double time; double* rbd; double* time_out; };
__device__ __forceinline__ void qm_measured_body(const QmMeasArgs& a, const int b) {
  const double* x = a.x0 + (size_t)b * 30; double* r = a.rbd + (size_t)b * QM_NRBD;
  for (int q = 0; q < QM_NRBD; ++q) r[q] = 0.0;
  for (int q = 0; q < 3; ++q) { r[q] = x[9 + q]; r[3 + q] = x[6 + q]; }
  for (int j = 0; j < QM_NJ; ++j) r[6 + j] = x[12 + j];
  double K[KW_SIZE]; kin_base(a.mb, x, K); kin_arm(a.mb, x, K);
  double qq[4]; mat_to_quat(K + KW_ARM + 39, qq);
  for (int q = 0; q < 3; ++q) r[48 + q] = K[KW_ARM + 36 + q];
  for (int q = 0; q < 4; ++q) r[51 + q] = qq[q];
  a.time_out[b] = a.time;
}
__global__ void qm_measured_kernel(QmMeasArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  qm_measured_body(a, b);
}
// the benchmark / closed-loop step evaluates the policy at t0 and builds the measured state in one launch (one thread per instance each:
// the first B threads take the policy, the next B the measured state)
struct QmPolicyMeasArgs { QmPolicyArgs p; QmMeasArgs m; };
__global__ void qm_policy_measured_kernel(QmPolicyMeasArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < a.p.B) qm_policy_body(a.p, g); else if (g - a.p.B < a.m.B) qm_measured_body(a.m, g - a.p.B);
}

// hand-over of the solver's node-major arrays [nmax][B][k] in the C ABI's instance-major layout [B][nmax][k] (qmhip_mpc_download): transposed on the DEVICE into one
// staging buffer per call, so that the host sees ONE contiguous copy per array instead of B x nmax strided pieces.  Thread per 8-byte word (k doubles, or one int widened)
struct QmGatherArgs { int B, nmax, k; const double* src_d; const int* src_i; double* dst_d; int* dst_i; };
__global__ void qm_gather_kernel(QmGatherArgs a) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)a.B * a.nmax * a.k;
  if (g >= total) return;
  const int q = (int)(g % a.k); const size_t bi = g / a.k; const int i = (int)(bi % a.nmax), b = (int)(bi / a.nmax);      // destination index (b, i, q): coalesced writes
  const size_t s = ((size_t)i * a.B + b) * a.k + q;
  if (a.src_d) a.dst_d[g] = a.src_d[s]; else a.dst_i[g] = a.src_i[s];
}

// ---- feedback policy (sqp.useFeedbackPolicy, task.info:89): the SQP's linear controller u(t, x) = uff(t) + K(t) x evaluated at a MEASURED state
// ([upstream ocs2_sqp multiple_shooting::toPrimalSolution with feedback + LinearController::computeInput, recalled]; call site
// qm_controllers/src/QMController.cpp:139-142: evaluatePolicy(time, currentObservation_.state, ...)).  At a node j with an input of its own
//   K_full,j = Px_j + Pu_j K_j,   uff_j = u*_j − K_full,j x*_j
// with K_j the Riccati gain K3 left in the stage record of the LAST SQP iteration (SR_PP), Px_j the constraint projection's state part (its twelve non-zero rows at
// SR_PX + 360) and Pu_j the null-space basis, applied as the gather it is (unit columns + the swing legs' 3 x 2 blocks, SR_SWG / SR_MODEF — what K3's rollout does).
// A node without an input (PreEvent, terminal) carries the pair of the node its `us` was copied from (qm_ls_apply_kernel, k_ls.h).  Bias and gain are interpolated
// linearly like the feed-forward policy; each term is evaluated as u*_j + K_full,j (x − x*_j): the same value without the cancellation of K x − K x*.
// Nothing is assembled per solve: a tick touches the records of its two bracketing nodes only.

// the node whose input (and stage record) node i of instance b's n-node grid carries; -1: none (a grid without an interval)
__device__ __forceinline__ int qm_fb_source_node(const int* node_ev, int n, int B, int b, int i) {
  int j = (i == n - 1) ? n - 2 : i;
  if (j < 0) return -1;
  while (j > 0 && node_ev[j * B + b] == QM_EV_PRE) --j;
  return (node_ev[j * B + b] == QM_EV_PRE) ? -1 : j;
}
// row r of Pu under contact mode md: its (at most two) non-zero entries sit in columns col, col + 1 with weights w1, w2.  Column order of K1b's projector: three force
// components per stance foot, two null-space directions per swing leg, six arm joint velocities (contacts in the order LF RF LH RH)
// (the record's fields are addressed through a view — QmFbView: the offsets of K, the virtual base of Px, the swing blocks, the mode and m — so that the same code reads
// a stage record, QmFbStageView, and the compact published record of k_publish.h)
template <int PP, int PX, int SWG, int MODEF, int SCAL> struct QmFbView { static constexpr int pp = PP, px = PX, swg = SWG, modef = MODEF, scal = SCAL; };
typedef QmFbView<SR_PP, SR_PX, SR_SWG, SR_MODEF, SR_SCAL> QmFbStageView;
template <class V = QmFbStageView>
__device__ __forceinline__ void qm_fb_pu_row(const double* rec, int md, int r, int* col, double* w1, double* w2) {
  int nst = 0; for (int k = 0; k < 4; ++k) nst += mode_flag(md, k) ? 1 : 0;
  const int kk = (r < 12) ? r / 3 : ((r < 24) ? chain_to_contact((r - 12) / 3) : 0), r3 = (r < 12) ? r % 3 : ((r < 24) ? (r - 12) % 3 : r - 24);
  int before_st = 0, before_sw = 0; for (int k = 0; k < 4; ++k) if (k < kk) { before_st += mode_flag(md, k) ? 1 : 0; before_sw += mode_flag(md, k) ? 0 : 1; }
  const bool stf = mode_flag(md, kk);
  *col = (r < 12) ? 3 * before_st + r3 : ((r < 24) ? 3 * nst + 2 * before_sw : 3 * nst + 2 * (4 - nst) + r3);
  if (r < 12) { *w1 = stf ? 1.0 : 0.0; *w2 = 0.0; }
  else if (r < 24) { const double s1 = rec[V::swg + 6 * kk + r3], s2 = rec[V::swg + 6 * kk + 3 + r3]; *w1 = stf ? 0.0 : s1; *w2 = stf ? 0.0 : s2; }
  else { *w1 = 1.0; *w2 = 0.0; }
}
// lane l (< 30): component l of K_full dx = Px dx + Pu (K dx) from one stage record; dxl = the lane's component of dx (0 in lanes >= 30).  One row of K and one of Px per lane
template <class V = QmFbStageView>
__device__ __forceinline__ double qm_fb_du(const double* rec, const double dxl, const int l) {
  const int m = (int)rec[V::scal], md = (int)rec[V::modef];
  const int r = (l < 30) ? l : 0; const bool hasPx = r >= 12 && r < 24, hasK = l < m; const int lr = hasK ? l : 0, pr = hasPx ? r : 12;
  double w[30], px[30];      // every record entry the lane needs is requested before the first dependent use
#pragma unroll
  for (int q = 0; q < 30; ++q) { w[q] = rec[V::pp + lr * 30 + q]; px[q] = rec[V::px + pr * 30 + q]; }
  double v = 0.0, s = 0.0;
#pragma unroll
  for (int q = 0; q < 30; ++q) { const double d = qm_bcast(dxl, q); v += (hasK ? w[q] : 0.0) * d; s += (hasPx ? px[q] : 0.0) * d; }      // uniform control flow around the broadcasts
  int col; double w1, w2; qm_fb_pu_row<V>(rec, md, r, &col, &w1, &w2);
  const double v1 = __shfl(v, col & 63, 64), v2 = __shfl(v, (col + 1) & 63, 64);      // (lanes >= m hold 0: a unit row whose column is m − 1 reads a zero beside it)
  return s + w1 * v1 + w2 * v2;
}

struct QmPolicyFbArgs { QmPolicyArgs p; const double* x; const double* stage; };      // x [B][30]: the state the policy is evaluated at; stage [B][nmax][SR_SIZE]
// ONE WAVEFRONT per instance (launch: B workgroups of 64): a thread per instance would walk two 18 x 30 matrices at a 30 KB stride per lane
__global__ void __launch_bounds__(64) qm_policy_fb_kernel(QmPolicyFbArgs a) {
  const int b = blockIdx.x, l = threadIdx.x; const QmPolicyArgs& p = a.p;
  if (b >= p.B) return;
  const int n = p.n_nodes[b]; const double t = p.t[b];
  int idx; double al; grid_policy_segment(p.node_t, p.node_ev, n, p.B, b, t, &idx, &al);
  const int i0 = idx, i1 = (n > 1) ? idx + 1 : idx; const bool lx = l < 30; const int lq = lx ? l : 0;
  const size_t o0 = ((size_t)i0 * p.B + b) * 30 + lq, o1 = ((size_t)i1 * p.B + b) * 30 + lq;
  const double xm = a.x[(size_t)b * 30 + lq];
  const int j0 = qm_fb_source_node(p.node_ev, n, p.B, b, i0), j1 = qm_fb_source_node(p.node_ev, n, p.B, b, i1);      // wave-uniform
  double u0 = p.us[o0], u1 = p.us[o1], du0 = 0.0;
  if (j0 >= 0) { const double dxl = lx ? xm - p.xs[((size_t)j0 * p.B + b) * 30 + lq] : 0.0; du0 = qm_fb_du(a.stage + ((size_t)b * p.nmax + j0) * SR_SIZE, dxl, l); u0 += du0; }
  if (j1 == j0) u1 += du0;                                                           // both nodes carry the same pair (an event node, the terminal node, t outside the grid)
  else if (j1 >= 0) { const double dxl = lx ? xm - p.xs[((size_t)j1 * p.B + b) * 30 + lq] : 0.0; u1 += qm_fb_du(a.stage + ((size_t)b * p.nmax + j1) * SR_SIZE, dxl, l); }
  if (lx) { p.x_des[(size_t)b * 30 + l] = al * p.xs[o0] + (1.0 - al) * p.xs[o1]; p.u_des[(size_t)b * 30 + l] = al * u0 + (1.0 - al) * u1; }
  if (l == 0) p.mode[b] = p.modes[(size_t)b * (p.nev + 1) + grid_find_index(p.ev + (size_t)b * p.nev, p.nev, t)];
}

// hand-over of the linear controller to the host (qmhip_mpc_download_feedback; ocs2::LinearController's gainArray_ / biasArray_): one wavefront per (instance, node)
// of the instances b0 .. b0 + nb − 1, K_full and uff written instance-major into a staging buffer ([nb][nmax][30][30], [nb][nmax][30]) that travels in one contiguous
// copy per array — the pattern of qm_gather_kernel.  Nodes behind the instance's grid hold zeros.  Runs only when asked
struct QmFbGatherArgs { int B, nmax, b0, nb; const int* n_nodes; const int* node_ev; const double* xs; const double* us; const double* stage; double* gain; double* uff; };
__global__ void __launch_bounds__(64) qm_feedback_gather_kernel(QmFbGatherArgs a) {
  const int g = blockIdx.x, l = threadIdx.x; const int bl = g / a.nmax, i = g - bl * a.nmax, b = a.b0 + bl;
  if (bl >= a.nb || b >= a.B) return;
  double* G = a.gain + (size_t)g * 900; double* F = a.uff + (size_t)g * 30;
  const int n = a.n_nodes[b]; const int j = (i < n) ? qm_fb_source_node(a.node_ev, n, a.B, b, i) : -1;
  if (j < 0) { for (int e = l; e < 900; e += 64) G[e] = 0.0; if (l < 30) F[l] = 0.0; return; }
  const double* rec = a.stage + ((size_t)b * a.nmax + j) * SR_SIZE; const int m = (int)rec[SR_SCAL], md = (int)rec[SR_MODEF];
  auto entry = [&](int r, int q, int col, double w1, double w2) {      // K_full[r][q] = Px[r][q] + w1 K[col][q] + w2 K[col + 1][q]
    double v = (r >= 12 && r < 24) ? rec[SR_PX + r * 30 + q] : 0.0;
    if (w1 != 0.0 && col < m) v += w1 * rec[SR_PP + col * 30 + q];
    if (w2 != 0.0 && col + 1 < m) v += w2 * rec[SR_PP + (col + 1) * 30 + q];
    return v;
  };
  for (int e = l; e < 900; e += 64) { const int r = e / 30, q = e - 30 * r; int col; double w1, w2; qm_fb_pu_row(rec, md, r, &col, &w1, &w2); G[e] = entry(r, q, col, w1, w2); }      // consecutive lanes, consecutive doubles
  if (l < 30) {
    int col; double w1, w2; qm_fb_pu_row(rec, md, l, &col, &w1, &w2);
    const double* xj = a.xs + ((size_t)j * a.B + b) * 30; double s = 0.0;
    for (int q = 0; q < 30; ++q) s += entry(l, q, col, w1, w2) * xj[q];
    F[l] = a.us[((size_t)i * a.B + b) * 30 + l] - s;
  }
}
