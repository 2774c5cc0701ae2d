// qm_plan_pipeline.h — planned task-space trajectories (qmhip_plan_task_space / qmhip_plan_footholds / qmhip_task_space_eval): the launches of k_plan.h, their buffers
// and the hand-over to the host.  Backend-templated like qm_tick_pipeline.h: the product drives it with the HIP backend, tests/emu_plan with the host emulator.
//
// Everything runs in order on the MPC stream behind whatever that stream holds (the last solve's apply included) and the host waits for ONE event on that stream.
// Nothing is allocated before the first call: the node records of a context for B = 1024 x 101 nodes are 53 MB, twice (node-major + the instance-major hand-over).
// `BK` provides, beyond what qm_pipeline.h lists:  void* alloc_pinned(size_t);  void free_pinned(void*);  void* io_event();  void io_event_free(void*);  void stream_select(int);
//   void copy_in(void* dev, const void* host, size_t, int stream)       in order on that stream (0: the MPC stream)
//   void copy_back(void* pinned, const void* dev, size_t, void* event)  in order on the MPC stream; then records `event`
//   void io_wait(void* event)                                           the only host wait
#pragma once
#include <cstring>
#include "qm_pipeline.h"
#include "../kernels/k_policy.h"
#include "../kernels/k_plan.h"

template <class BK>
struct QmPlanPipeline {
  BK& bk;
  double* rec = nullptr; double* stage = nullptr; size_t rows_cap = 0;      // node-major records [rows + QM_PLAN_SLACK][64] (the row kernels store whole 64-record blocks) and their instance-major copy
  char* in_dev = nullptr; size_t in_cap = 0;                                // rows of qmhip_task_space_eval: [x R x 30 | u R x 30 | ee R x 7 | mode R (int32)]
  char* out_dev = nullptr; size_t out_cap = 0;                              // footholds [B][cap][5 words] | count [B] (int32)
  char* pin = nullptr; size_t pin_cap = 0; void* event = nullptr;
  explicit QmPlanPipeline(BK& b) : bk(b) {}
  void release() {
    void* ps[] = {rec, stage, in_dev, out_dev}; for (void* p : ps) if (p) bk.free(p);
    if (pin) bk.free_pinned(pin); if (event) bk.io_event_free(event);
    rec = stage = nullptr; in_dev = out_dev = pin = nullptr; event = nullptr; rows_cap = in_cap = out_cap = pin_cap = 0;
  }
  void reserve_rows(size_t rows) { if (rows_cap >= rows) return; if (rec) bk.free(rec); if (stage) bk.free(stage); rec = (double*)bk.alloc((rows + QM_PLAN_SLACK) * QM_PLAN_BYTES); stage = (double*)bk.alloc(rows * QM_PLAN_BYTES); rows_cap = rows; }
  void reserve_pin(size_t bytes) { if (!event) event = bk.io_event(); if (pin_cap >= bytes) return; if (pin) bk.free_pinned(pin); pin = (char*)bk.alloc_pinned(bytes); pin_cap = bytes; }
  static void reserve_dev(BK& bk, char*& p, size_t& cap, size_t bytes) { if (cap >= bytes) return; if (p) bk.free(p); p = (char*)bk.alloc(bytes); cap = bytes; }
  void fetch(const void* dev, size_t bytes) { bk.copy_back(pin, dev, bytes, event); bk.io_wait(event); }

  // publishOptimizedStateTrajectory (qm_visualization.cpp:90-189): records of the primal solution of the last solve of B instances -> rec_out [B][nmax], nn_out [B] (may be null)
  void task_space(const QmMpcBuffers& d, int B, void* rec_out, int32_t* nn_out) {
    const size_t rows = (size_t)d.nmax * B, bytes = rows * QM_PLAN_BYTES; reserve_rows((size_t)d.nmax * d.Bmax); reserve_pin(bytes + (size_t)B * 4); bk.stream_select(0);
    QmPlanRowsArgs a; a.mb = d.mb; a.nrows = (long long)rows; a.B = B; a.x = d.xs; a.u = d.us; a.mode = d.node_mode; a.ee = d.eeref; a.time = d.node_t; a.n_nodes = d.n_nodes; a.rec = rec;
    bk.launch(qm_plan_nodes_kernel, (int)((rows + 63) / 64), 64, QM_PLAN_LDS_BYTES, a);
    // node-major [nmax][B][64] -> instance-major [B][nmax][64] on the device (qm_gather_kernel, k_policy.h): the host sees ONE contiguous copy
    QmGatherArgs g; g.B = B; g.nmax = d.nmax; g.k = QM_PLAN_WORDS; g.src_d = rec; g.src_i = nullptr; g.dst_d = stage; g.dst_i = nullptr;
    bk.launch(qm_gather_kernel, (int)((rows * QM_PLAN_WORDS + 255) / 256), 256, 0, g);
    if (nn_out) bk.copy_back(pin + bytes, d.n_nodes, (size_t)B * 4, event);
    fetch(stage, bytes);
    memcpy(rec_out, pin, bytes); if (nn_out) memcpy(nn_out, pin + bytes, (size_t)B * 4);
  }
  // the "Future footholds" of qm_visualization.cpp:150-182 -> out [B][cap] qmhip_foothold (may be null with cap == 0), count [B]
  void footholds(const QmMpcBuffers& d, int B, int cap, void* out, int32_t* count) {
    const size_t fb = (size_t)B * cap * QM_FOOTHOLD_BYTES, bytes = fb + (size_t)B * 4; reserve_dev(bk, out_dev, out_cap, bytes); reserve_pin(bytes); bk.stream_select(0);
    bk.zero(out_dev, bytes);      // slots behind an instance's count read as zeros
    QmPlanFootArgs a; a.mb = d.mb; a.B = B; a.nmax = d.nmax; a.nev = d.nev; a.cap = cap; a.n_nodes = d.n_nodes; a.node_t = d.node_t; a.node_ev = d.node_ev; a.xs = d.xs; a.ev = d.ev; a.modes = d.modes;
    a.out = (double*)out_dev; a.count = (int*)(out_dev + fb);
    bk.launch(qm_plan_footholds_kernel, (B * d.nev + 63) / 64, 64, 0, a);
    fetch(out_dev, bytes);
    if (out && fb) memcpy(out, pin, fb); memcpy(count, pin + fb, (size_t)B * 4);
  }
  // publishDesiredTrajectory / publishObservation (qm_visualization.cpp:194-251, 267-283): R caller-supplied rows -> rec_out [R]
  void eval(const double* mb, int R, const double* x, const double* u, const int32_t* mode, const double* ee, void* rec_out) {
    const size_t xb = (size_t)R * 30 * 8, eb = (size_t)R * 7 * 8, ib = 2 * xb + eb + (size_t)R * 4, bytes = (size_t)R * QM_PLAN_BYTES;
    reserve_rows((size_t)R); reserve_dev(bk, in_dev, in_cap, ib); reserve_pin(bytes); bk.stream_select(0);
    char* xd = in_dev; char* ud = in_dev + xb; char* ed = in_dev + 2 * xb; char* md = in_dev + 2 * xb + eb;      // (x and u start on 16-byte boundaries: the rows come in as double2)
    bk.copy_in(xd, x, xb, 0); if (u) bk.copy_in(ud, u, xb, 0); if (ee) bk.copy_in(ed, ee, eb, 0); bk.copy_in(md, mode, (size_t)R * 4, 0);
    QmPlanRowsArgs a; a.mb = mb; a.nrows = R; a.B = 1; a.x = (const double*)xd; a.u = u ? (const double*)ud : nullptr; a.mode = (const int*)md; a.ee = ee ? (const double*)ed : nullptr; a.time = nullptr; a.n_nodes = nullptr; a.rec = rec;
    bk.launch(qm_plan_states_kernel, (R + 63) / 64, 64, QM_PLAN_LDS_BYTES, a);
    fetch(rec, bytes);
    memcpy(rec_out, pin, bytes);
  }
};
