// qm_io_pipeline.h — streamed control-step I/O (qmhip_step_submit / qmhip_step_collect): two slots, so that the result of step k travels to the host while step
// k + 1 computes.  Backend-templated like qm_pipeline.h: the product drives it with the HIP backend, tests/emu_io with the host emulator.
//
// A slot owns: pinned input staging [t0 | x0 | rbd | time], one device buffer [B records of 1024 bytes | trajectory part] written by qm_step_pack_kernel (k_io.h),
// its pinned host mirror, and the event that says "the mirror is complete".
// `BK` provides, beyond what qm_pipeline.h lists:  void* alloc_pinned(size_t);  void free_pinned(void*);  void* io_event();  void io_event_free(void*);
//   void copy_in(void* dev, const void* pinned, size_t, int stream /*0 MPC, 1 WBC*/)      asynchronous, in order on that stream
//   void copy_out(void* pinned, const void* dev, size_t, void* event, bool wbc)            on the copy stream, behind what the MPC (and WBC) stream holds so far; then records `event`
//   void io_wait(void* event)                                                               the ONLY host wait of the pair
#pragma once
#include <cstring>
#include "qm_wbc_pipeline.h"
#include "../kernels/k_io.h"

struct QmIoSlot {
  double* in_pin = nullptr; char* dev = nullptr; char* out_pin = nullptr; void* event = nullptr; size_t cap = 0;
  int B = 0, ncap = 0; unsigned flags = 0;      // of the step in flight in this slot
};

template <class BK>
struct QmIoPipeline {
  BK& bk; QmIoSlot slot[2]; int Bmax = 0, oldest = 0, in_flight = 0;
  explicit QmIoPipeline(BK& b) : bk(b) {}
  static size_t slot_bytes(int B, int ncap, bool traj) { return (size_t)B * QM_STEP_BYTES + (traj ? qm_pack_traj_words(B, ncap) * 8 : 0); }
  // allocated by the first submit: a context that never streams pays nothing; the record part for max_batch instances, the trajectory part on demand (reserve)
  void allocate(int Bmax_) {
    if (Bmax) return; Bmax = Bmax_;
    for (QmIoSlot& s : slot) { s.in_pin = (double*)bk.alloc_pinned((size_t)Bmax * (1 + 30 + QM_NRBD + 1) * 8); s.event = bk.io_event(); reserve(s, slot_bytes(Bmax, 0, false)); }
  }
  void release() {
    for (QmIoSlot& s : slot) { if (s.in_pin) bk.free_pinned(s.in_pin); if (s.out_pin) bk.free_pinned(s.out_pin); if (s.dev) bk.free(s.dev); if (s.event) bk.io_event_free(s.event); s = QmIoSlot(); }
    Bmax = 0; oldest = 0; in_flight = 0;
  }
  void reserve(QmIoSlot& s, size_t bytes) {      // only ever called on a slot with nothing in flight
    if (s.cap >= bytes) return;
    if (s.dev) bk.free(s.dev); if (s.out_pin) bk.free_pinned(s.out_pin);
    s.dev = (char*)bk.alloc(bytes); s.out_pin = (char*)bk.alloc_pinned(bytes); s.cap = bytes;
  }
  QmIoSlot& next() { return slot[(oldest + in_flight) & 1]; }
  QmIoSlot& front() { return slot[oldest]; }
  double* in_t0(QmIoSlot& s) const { return s.in_pin; }
  double* in_x0(QmIoSlot& s) const { return s.in_pin + Bmax; }
  double* in_rbd(QmIoSlot& s) const { return s.in_pin + (size_t)Bmax * 31; }
  double* in_time(QmIoSlot& s) const { return s.in_pin + (size_t)Bmax * (31 + QM_NRBD); }

  // caller's observation -> the slot's pinned staging -> device, nothing waited for: (t0, x0) on the MPC stream, in order behind the previous step's readers;
  // the measured state (when given) into the WBC's input buffer on the WBC stream, in order behind the previous WBC
  void upload(QmIoSlot& s, QmMpcBuffers& d, QmWbcBuffers& w, int B, const double* t0, const double* x0, const double* rbd, double time) {
    memcpy(in_t0(s), t0, (size_t)B * 8); memcpy(in_x0(s), x0, (size_t)B * 30 * 8);
    bk.copy_in(d.t0, in_t0(s), (size_t)B * 8, 0); bk.copy_in(d.x0, in_x0(s), (size_t)B * 30 * 8, 0);
    if (rbd) {
      memcpy(in_rbd(s), rbd, (size_t)B * QM_NRBD * 8); for (int b = 0; b < B; ++b) in_time(s)[b] = time;
      bk.copy_in(w.rbd, in_rbd(s), (size_t)B * QM_NRBD * 8, 1); bk.copy_in(w.time, in_time(s), (size_t)B * 8, 1);
    }
  }
  // one launch of the pack kernel on the backend's current stream (k_io.h, "Parts")
  void pack(const QmMpcBuffers& d, const QmWbcBuffers& w, int B, int ncap, int parts, bool strict, char* dev) {
    QmStepPackArgs a; a.B = B; a.nmax = d.nmax; a.ncap = ncap; a.parts = parts; a.strict = strict ? 1 : 0;
    a.x_des = w.x_des; a.u_des = w.u_des; a.mode = w.mode; a.wbc_out = w.out; a.qp_status = w.qp_status;
    a.out_perf = d.out_perf; a.status = d.status; a.step_info = d.step_info; a.n_nodes = d.n_nodes;
    a.node_t = d.node_t; a.node_ev = d.node_ev; a.node_mode = d.node_mode; a.xs = d.xs; a.us = d.us;
    a.rec = (double*)dev; a.traj = (double*)(dev + (size_t)B * QM_STEP_BYTES);
    bk.launch(qm_step_pack_kernel, (int)((qm_pack_threads(B, ncap, parts) + 255) / 256), 256, 0, a);
  }
  // the slot's device buffer -> its pinned mirror on the copy stream; the step is in flight from here on
  void download(QmIoSlot& s, int B, int ncap, unsigned flags, bool traj, bool wbc) {
    s.B = B; s.ncap = ncap; s.flags = flags;
    bk.copy_out(s.out_pin, s.dev, slot_bytes(B, ncap, traj), s.event, wbc); ++in_flight;
  }
  // wait for the OLDEST slot's mirror only, hand it to the caller: records as they are; of the trajectory arrays ([B][nmax_out][k], any may be null) the first
  // n_nodes[b] nodes of every instance, the caller's memory behind them stays untouched
  void collect(void* rec, int nmax_out, double* ot, int32_t* oev, int32_t* omode, double* ox, double* ou) {
    QmIoSlot& s = front(); bk.io_wait(s.event);
    const int B = s.B, nc = s.ncap; memcpy(rec, s.out_pin, (size_t)B * QM_STEP_BYTES);
    if (ot || oev || omode || ox || ou) {
      const size_t BN = (size_t)B * nc; const double* tj = (const double*)(s.out_pin + (size_t)B * QM_STEP_BYTES);
      const double* t = tj; const double* x = tj + BN; const double* u = tj + BN * 31; const int32_t* ev = (const int32_t*)(tj + BN * 61); const int32_t* mo = ev + 2 * qm_pack_pairs(B, nc);
      for (int b = 0; b < B; ++b) {
        int n = ((const qmhip_step_record*)s.out_pin)[b].n_nodes; if (n > nc) n = nc; if (n > nmax_out) n = nmax_out; if (n <= 0) continue;
        const size_t src = (size_t)b * nc, dst = (size_t)b * nmax_out;
        if (ot) memcpy(ot + dst, t + src, (size_t)n * 8); if (oev) memcpy(oev + dst, ev + src, (size_t)n * 4); if (omode) memcpy(omode + dst, mo + src, (size_t)n * 4);
        if (ox) memcpy(ox + dst * 30, x + src * 30, (size_t)n * 30 * 8); if (ou) memcpy(ou + dst * 30, u + src * 30, (size_t)n * 30 * 8);
      }
    }
    oldest ^= 1; --in_flight;
  }
};
