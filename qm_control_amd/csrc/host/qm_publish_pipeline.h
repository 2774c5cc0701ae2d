// qm_publish_pipeline.h — the published policy (qmhip_policy_publish / qmhip_policy_eval_published; backend-templated like qm_pipeline.h): two slots, each a snapshot of the
// primal solution + grid + mode schedule (what QmSimPipeline::publish_policy copies) and of the first W nodes' gain records (k_publish.h).  Bookkeeping: qm_publish_book.h.
// The backend supplies events: pub_event() / pub_event_free(e), pub_wait(e) (the current stream waits for e), pub_record(e) (e is recorded on the current stream).
#pragma once
#include "qm_pipeline.h"
#include "qm_wbc_pipeline.h"
#include "qm_publish_book.h"
#include "../kernels/k_publish.h"

struct QmPubSlot {
  double* xs = nullptr; double* us = nullptr; double* node_t = nullptr; int* node_ev = nullptr; int* n_nodes = nullptr; double* ev = nullptr; int* modes = nullptr;
  double* gains = nullptr;                            // [Bmax][W][PR_SIZE]
  void* ev_pub = nullptr; void* ev_eval = nullptr;    // "the snapshot is complete" / "the last evaluation enqueued on this slot is done"
};

template <class BK>
struct QmPublishPipeline {
  static constexpr bool enabled = true;
  BK& bk; QmPubBook book; QmPubSlot slot[2]; int W = 0, Bmax = 0, nmax = 0, nev = 0;
  int* covered = nullptr; int* uncovered = nullptr;      // [Bmax] each: of the loop's ticks (the sticky counter of qmhip_policy_published_info)
  explicit QmPublishPipeline(BK& b) : bk(b) {}
  template <class T> T* A(size_t n) { T* p = (T*)bk.alloc(n * sizeof(T)); bk.zero(p, n * sizeof(T)); return p; }
  void release() {
    for (QmPubSlot& s : slot) { void* ps[] = {s.xs, s.us, s.node_t, s.node_ev, s.n_nodes, s.ev, s.modes, s.gains}; for (void* p : ps) if (p) bk.free(p); if (s.ev_pub) bk.pub_event_free(s.ev_pub); if (s.ev_eval) bk.pub_event_free(s.ev_eval); s = QmPubSlot(); }
    if (covered) bk.free(covered); if (uncovered) bk.free(uncovered); covered = uncovered = nullptr; W = 0; book.reset(0);
  }
  // nodes 0: off, nothing allocated; otherwise two slots for the solver's Bmax instances.  The caller has made sure that nothing is in flight on the old slots
  void set_window(const QmMpcBuffers& d, int nodes) {
    release(); if (nodes <= 0) return;
    W = nodes; Bmax = d.Bmax; nmax = d.nmax; nev = d.nev; const size_t NB = (size_t)nmax * Bmax;
    for (QmPubSlot& s : slot) {
      s.xs = A<double>(NB * 30); s.us = A<double>(NB * 30); s.node_t = A<double>(NB); s.node_ev = A<int>(NB); s.n_nodes = A<int>(Bmax); s.ev = A<double>((size_t)Bmax * nev); s.modes = A<int>((size_t)Bmax * (nev + 1));
      s.gains = (double*)bk.alloc((size_t)Bmax * W * PR_SIZE * sizeof(double));      // (every record an evaluation can reach is written by the publication in front of it)
      s.ev_pub = bk.pub_event(); s.ev_eval = bk.pub_event();
    }
    covered = A<int>(Bmax); uncovered = A<int>(Bmax); book.reset(W);
  }
  void reset_counters() { if (uncovered) bk.zero(uncovered, (size_t)Bmax * sizeof(int)); }
  // snapshot of the solver's last solution of a batch of B into the inactive slot, on the backend's current stream (behind the solve, in front of the next one), then that
  // slot is the active one.  gains: also the first W nodes' gain records.  Returns the publication's sequence number, -1 when publishing is off
  long publish(const QmMpcBuffers& d, int B, bool gains) {
    bool wait_eval = false; const int t = book.begin_publish(&wait_eval); if (t < 0) return -1;
    QmPubSlot& s = slot[t]; const size_t nb = (size_t)d.nmax * B;      // node-major arrays are strided by the batch of the solve
    if (wait_eval) bk.pub_wait(s.ev_eval);
    bk.copy_dd(s.xs, d.xs, nb * 30 * 8); bk.copy_dd(s.us, d.us, nb * 30 * 8); bk.copy_dd(s.node_t, d.node_t, nb * 8); bk.copy_dd(s.node_ev, d.node_ev, nb * 4); bk.copy_dd(s.n_nodes, d.n_nodes, (size_t)B * 4);
    bk.copy_dd(s.ev, d.ev, (size_t)B * d.nev * 8); bk.copy_dd(s.modes, d.modes, (size_t)B * (d.nev + 1) * 4);
    if (gains) { QmPublishArgs a; a.B = B; a.nmax = d.nmax; a.W = W; a.n_nodes = d.n_nodes; a.node_ev = d.node_ev; a.stage = d.stage; a.pub = s.gains; bk.launch(qm_policy_publish_kernel, B * W, 64, 0, a); }
    bk.pub_record(s.ev_pub);
    return book.end_publish(B, gains);
  }
  // arguments of qm_policy_fb_pub_kernel on slot k (launch: B workgroups of 64); x_dev null: the feed-forward policy for every instance
  QmPolicyFbPubArgs eval_args(int k, int B, const double* t_dev, const double* x_dev, double* x_des, double* u_des, int* mode, int* covered_dev, int* uncovered_dev) const {
    const QmPubSlot& s = slot[k]; QmPolicyFbPubArgs a; QmPolicyArgs& p = a.p;
    p.mb = nullptr; p.B = B; p.nmax = nmax; p.nev = nev; p.n_nodes = s.n_nodes; p.node_t = s.node_t; p.node_ev = s.node_ev; p.xs = s.xs; p.us = s.us; p.ev = s.ev; p.modes = s.modes;
    p.t = t_dev; p.x_des = x_des; p.u_des = u_des; p.mode = mode; a.x = x_dev; a.pub = s.gains; a.W = W; a.covered = covered_dev; a.uncovered = uncovered_dev; return a;
  }
  // a tick of the pipelined loop: the linear controller of the ACTIVE slot at (t_dev, x_dev) into the WBC's inputs, on the current stream — the stream the loop publishes
  // on, so the order is the stream's (the loop owns the context: there is no other publisher)
  void tick_policy(QmWbcPipeline<BK>& wbc, int B, const double* t_dev, const double* x_dev) {
    int k = -1; book.info(nullptr, nullptr, &k, nullptr); if (k < 0) return;
    bk.launch(qm_policy_fb_pub_kernel, B, 64, 0, eval_args(k, B, t_dev, x_dev, wbc.w.x_des, wbc.w.u_des, wbc.w.mode, covered, uncovered));
  }
};
