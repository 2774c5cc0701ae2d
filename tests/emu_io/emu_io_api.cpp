// tests/emu_io/emu_io_api.cpp — TEST INFRASTRUCTURE: the step-I/O pipeline (qm_io_pipeline.h) and its pack kernel (k_io.h) on the host emulator, for pytest through ctypes.
// Never linked into the product.
#include <cstddef>
#include "hip_emu.h"
#include "../../qm_control_amd/csrc/host/qm_io_pipeline.h"

struct EmuIoBackend {
  int launches = 0;
  template <class K, class A> void launch(K kernel, int grid, int block, size_t, const A& args) { ++launches; emu::launch(dim3(grid), dim3(block), [&]() { kernel(args); }); }
  void* alloc(size_t n) { return malloc(n ? n : 8); }
  void free(void* p) { ::free(p); }
  void zero(void* p, size_t n) { memset(p, 0, n); }
  void* alloc_pinned(size_t n) { return malloc(n ? n : 8); }
  void free_pinned(void* p) { ::free(p); }
  void* io_event() { return malloc(8); }
  void io_event_free(void* e) { ::free(e); }
  void copy_in(void* d, const void* s, size_t n, int) { memcpy(d, s, n); }
  void copy_out(void* d, const void* s, size_t n, void*, bool) { memcpy(d, s, n); }
  void io_wait(void*) {}
};

extern "C" {
int emu_io_record_bytes() { return (int)sizeof(qmhip_step_record); }
// byte offset of the k-th field of struct qmhip_step_record, in declaration order
int emu_io_record_offset(int k) {
  const size_t o[] = {offsetof(qmhip_step_record, x_des), offsetof(qmhip_step_record, u_des), offsetof(qmhip_step_record, wbc_out), offsetof(qmhip_step_record, perf), offsetof(qmhip_step_record, mode),
                      offsetof(qmhip_step_record, mpc_status), offsetof(qmhip_step_record, n_nodes), offsetof(qmhip_step_record, qp_status), offsetof(qmhip_step_record, reserved)};
  return k >= 0 && k < 9 ? (int)o[k] : -1;
}
int emu_io_status_host(int k0_status, const double* step_info4, int strict) { return qm_mpc_status(k0_status, step_info4, strict != 0); }
long emu_io_slot_bytes(int B, int ncap, int traj) { return (long)QmIoPipeline<EmuIoBackend>::slot_bytes(B, ncap, traj != 0); }
// one launch of qm_step_pack_kernel with `parts` on caller-owned buffers; `slot` holds slot_bytes(B, ncap, traj) bytes and keeps what the launch does not write
void emu_io_pack(int B, int nmax, int ncap, int parts, int strict, const double* x_des, const double* u_des, const int* mode, const double* wbc_out, const int* qp_status,
                 const double* out_perf, const int* status, const double* step_info, const int* n_nodes, const double* node_t, const int* node_ev, const int* node_mode,
                 const double* xs, const double* us, void* slot) {
  EmuIoBackend bk; QmIoPipeline<EmuIoBackend> io(bk); QmMpcBuffers d; QmWbcBuffers w;
  d.nmax = nmax; d.out_perf = (double*)out_perf; d.status = (int*)status; d.step_info = (double*)step_info; d.n_nodes = (int*)n_nodes;
  d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.node_mode = (int*)node_mode; d.xs = (double*)xs; d.us = (double*)us;
  w.x_des = (double*)x_des; w.u_des = (double*)u_des; w.mode = (int*)mode; w.out = (double*)wbc_out; w.qp_status = (int*)qp_status;
  io.pack(d, w, B, ncap, parts, strict != 0, (char*)slot);
}
// the whole way of a step's results through the pipeline: pack (MPC half, WBC half or the zero fill) -> slot -> mirror -> collect into the caller's arrays [B][nmax_out][k]
int emu_io_roundtrip(int Bmax, int B, int nmax, int ncap, int with_wbc, int traj, int strict, const double* x_des, const double* u_des, const int* mode, const double* wbc_out, const int* qp_status,
                     const double* out_perf, const int* status, const double* step_info, const int* n_nodes, const double* node_t, const int* node_ev, const int* node_mode,
                     const double* xs, const double* us, void* rec, int nmax_out, double* ot, int* oev, int* omode, double* ox, double* ou) {
  EmuIoBackend bk; QmIoPipeline<EmuIoBackend> io(bk); QmMpcBuffers d; QmWbcBuffers w;
  d.nmax = nmax; d.out_perf = (double*)out_perf; d.status = (int*)status; d.step_info = (double*)step_info; d.n_nodes = (int*)n_nodes;
  d.node_t = (double*)node_t; d.node_ev = (int*)node_ev; d.node_mode = (int*)node_mode; d.xs = (double*)xs; d.us = (double*)us;
  w.x_des = (double*)x_des; w.u_des = (double*)u_des; w.mode = (int*)mode; w.out = (double*)wbc_out; w.qp_status = (int*)qp_status;
  io.allocate(Bmax);
  for (int k = 0; k < 3; ++k) {      // three steps through the two slots; the last one is handed out
    QmIoSlot& s = io.next(); io.reserve(s, QmIoPipeline<EmuIoBackend>::slot_bytes(B, ncap, traj != 0)); memset(s.dev, 0xA5, s.cap);
    io.pack(d, w, B, ncap, QM_PACK_MPC | (traj ? QM_PACK_TRAJ : 0) | (with_wbc ? 0 : QM_PACK_NOWBC), strict != 0, s.dev);
    if (with_wbc) io.pack(d, w, B, ncap, QM_PACK_WBC, strict != 0, s.dev);
    io.download(s, B, ncap, 0, traj != 0, with_wbc != 0);
    if (io.in_flight == 2) { std::vector<char> drop((size_t)B * QM_STEP_BYTES); io.collect(drop.data(), nmax_out, nullptr, nullptr, nullptr, nullptr, nullptr); }
  }
  io.collect(rec, nmax_out, ot, oev, omode, ox, ou);
  const int left = io.in_flight; io.release();
  return left * 100 + bk.launches;
}
}
