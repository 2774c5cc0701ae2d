// k_publish.h — the PUBLISHED feedback policy (qmhip_policy_publish / qmhip_policy_eval_published, include/qmhip.h): what MPC_MRT_Interface's policy buffer is for the
// reference's control thread (updatePolicy + evaluatePolicy(time, currentObservation_.state, ...), qm_controllers/src/QMController.cpp:133-148) while mpcThread_ already
// computes the next solution (QMController.cpp:315-333).  The linear controller's gains live in the stage records, which K1b rewrites as soon as the next solve starts;
// a tick looks at the two nodes bracketing its time, and that time stays within one or two MPC periods of t0.  So a publication copies, for the first W nodes of every
// instance, the 926 doubles of a 3840-double record the feedback kernels read (PR_*, include/qmhip_layout.h) into one of two slots, next to the primal snapshot.
#pragma once
#include "k_policy.h"

typedef double qm_d2 __attribute__((ext_vector_type(2)));
typedef QmFbView<PR_PP, PR_PX, PR_SWG, PR_MODEF, PR_SCAL> QmFbPubView;
static_assert(PR_PX + 360 == PR_PP + 540 && PR_SWG == PR_PX + 720 && PR_MODEF == PR_SWG + 24 && PR_SCAL == PR_MODEF + 2 && PR_SIZE == PR_SCAL + 2 && PR_SIZE % 2 == 0 && PR_SIZE <= 1024, "published gain record");
static_assert((PR_SIZE / 2 - 1) / 64 == PR_MODEF / 2 / 64, "the mode / m pieces sit in the last row of pieces"); static_assert(SR_PP % 2 == 0 && (SR_PX + 360) % 2 == 0 && SR_SWG % 2 == 0 && SR_MODEF % 2 == 0 && SR_SCAL % 2 == 0 && SR_SIZE % 2 == 0, "the published fields start on 16-byte boundaries of the stage record");

// ONE WAVEFRONT per (instance, node i < W) (launch: B * W workgroups of 64): the PR_* fields of node i's stage record -> pub[b][i].  Consecutive lanes move consecutive
// 16-byte pieces (464 per record: eight per lane, all loads in flight before the first store); both sides are streamed once, hence the non-temporal hint (QM_STREAM_ST).
// A node without a record of its own — PreEvent, terminal, behind the instance's grid — gets zeros: qm_fb_source_node never points at it, and it always points at a node
// j <= i, i.e. inside the window whenever i is
struct QmPublishArgs { int B, nmax, W; const int* n_nodes; const int* node_ev; const double* stage; double* pub; };      // stage [B][nmax][SR_SIZE], pub [B][W][PR_SIZE]
__global__ void __launch_bounds__(64) qm_policy_publish_kernel(QmPublishArgs a) {
  const int g = blockIdx.x, l = threadIdx.x; const int b = g / a.W, i = g - b * a.W;
  if (b >= a.B) return;
  const int n = a.n_nodes[b]; const bool own = i < n - 1 && a.node_ev[i * a.B + b] != QM_EV_PRE;      // wave-uniform
  const qm_d2* src = (const qm_d2*)(a.stage + ((size_t)b * a.nmax + i) * SR_SIZE); qm_d2* dst = (qm_d2*)(a.pub + ((size_t)b * a.W + i) * PR_SIZE);
  constexpr int NP = PR_SIZE / 2, NT = (NP + 63) / 64;
  // piece p of the published record is piece p + d of the stage record, d constant per field: branch-free selects (the last workgroup-row of pieces is clamped, not masked)
  constexpr int D_PP = SR_PP / 2 - PR_PP / 2, D_PX = (SR_PX + 360) / 2 - (PR_PX + 360) / 2, D_SWG = SR_SWG / 2 - PR_SWG / 2, D_MODEF = SR_MODEF / 2 - PR_MODEF / 2, D_SCAL = SR_SCAL / 2 - PR_SCAL / 2;
  qm_d2 v[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) v[t] = qm_d2{0.0, 0.0};
  if (own) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int p0 = t * 64 + l, p = p0 < NP ? p0 : NP - 1;
      const int d = (p < (PR_PX + 360) / 2) ? D_PP : ((p < PR_SWG / 2) ? D_PX : ((p < PR_MODEF / 2) ? D_SWG : ((p < PR_SCAL / 2) ? D_MODEF : D_SCAL)));
      v[t] = __builtin_nontemporal_load(src + p + d);
    }
    if ((NT - 1) * 64 + l >= PR_MODEF / 2) v[NT - 1].y = 0.0;      // (behind the mode: dt; behind m: cp — not part of the published record)
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) { const int p = t * 64 + l; if (p < NP) __builtin_nontemporal_store(v[t], dst + p); }
}

// The linear controller on ONE SLOT of the published policy: qm_policy_fb_kernel (k_policy.h) on the published primal arrays (a.p) and the PR_* records — the same
// expressions in the same order, through the same qm_fb_du.  ONE WAVEFRONT per instance.  covered[b] = both bracketing nodes lie inside min(W, n); an instance that is not
// covered, and every instance when x is null, gets the feed-forward policy from qm_policy_body itself — what qm_policy_kernel runs — and no part of a feedback term.  uncovered (may be null):
// per-instance count of the evaluations at a state that were not covered
struct QmPolicyFbPubArgs { QmPolicyArgs p; const double* x; const double* pub; int W; int* covered; int* uncovered; };      // x [B][30] or null; pub [B][W][PR_SIZE]
__global__ void __launch_bounds__(64) qm_policy_fb_pub_kernel(QmPolicyFbPubArgs a) {
  const int b = blockIdx.x, l = threadIdx.x; const QmPolicyArgs& p = a.p;
  if (b >= p.B) return;
  const int n = p.n_nodes[b]; const double t = p.t[b];
  int idx; double al; grid_policy_segment(p.node_t, p.node_ev, n, p.B, b, t, &idx, &al);
  const int i0 = idx, i1 = (n > 1) ? idx + 1 : idx; const bool lx = l < 30; const int lq = lx ? l : 0;
  const int wn = (a.W < n) ? a.W : n; const bool cov = i0 < wn && i1 < wn, fb = cov && a.x != nullptr;      // wave-uniform
  if (l == 0) { if (a.covered) a.covered[b] = cov ? 1 : 0; if (a.uncovered && a.x != nullptr && !cov) a.uncovered[b] += 1; }
  if (!fb) { if (l == 0) qm_policy_body(p, b); return; }      // the feed-forward policy as qm_policy_kernel computes it: the same function on the same arrays, so the same bits
  // from here on: qm_policy_fb_kernel, statement for statement, on the published arrays and records
  const size_t o0 = ((size_t)i0 * p.B + b) * 30 + lq, o1 = ((size_t)i1 * p.B + b) * 30 + lq;
  const double xm = a.x[(size_t)b * 30 + lq];
  const int j0 = qm_fb_source_node(p.node_ev, n, p.B, b, i0), j1 = qm_fb_source_node(p.node_ev, n, p.B, b, i1);      // wave-uniform
  double u0 = p.us[o0], u1 = p.us[o1], du0 = 0.0;
  if (j0 >= 0) { const double dxl = lx ? xm - p.xs[((size_t)j0 * p.B + b) * 30 + lq] : 0.0; du0 = qm_fb_du<QmFbPubView>(a.pub + ((size_t)b * a.W + j0) * PR_SIZE, dxl, l); u0 += du0; }
  if (j1 == j0) u1 += du0;
  else if (j1 >= 0) { const double dxl = lx ? xm - p.xs[((size_t)j1 * p.B + b) * 30 + lq] : 0.0; u1 += qm_fb_du<QmFbPubView>(a.pub + ((size_t)b * a.W + j1) * PR_SIZE, dxl, l); }
  if (lx) { p.x_des[(size_t)b * 30 + l] = al * p.xs[o0] + (1.0 - al) * p.xs[o1]; p.u_des[(size_t)b * 30 + l] = al * u0 + (1.0 - al) * u1; }
  if (l == 0) p.mode[b] = p.modes[(size_t)b * (p.nev + 1) + grid_find_index(p.ev + (size_t)b * p.nev, p.nev, t)];
}
