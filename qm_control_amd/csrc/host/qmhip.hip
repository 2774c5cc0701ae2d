// qmhip.hip — libqmhip.so: HIP backend of the launch sequence (qm_pipeline.h) + the C ABI of include/qmhip.h.
// gfx950 only.  One context = one device, one HIP stream, all buffers resident in HBM for max_batch instances.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../../include/qmhip.h"
#include "qm_model_io.h"
#define QM_LQ_KERNELS_EXTERN 1      /* K1b's instances live in qmhip_lq.hip */
#include "qm_pipeline.h"
#include "qm_wbc_pipeline.h"
#include "qm_sim_pipeline.h"
#include "qm_front_pipeline.h"
#include "qm_hoqp_pipeline.h"
#include "qm_io_pipeline.h"
#include "qm_tick_pipeline.h"
#include "qm_publish_pipeline.h"
#include "qm_plan_pipeline.h"
#include "qm_episode_pipeline.h"
#include "qm_rollout_pipeline.h"
static_assert(QM_RO_OK == QMHIP_OK && QM_RO_ERR_ARG == QMHIP_ERR_ARG && QM_RO_ERR_STATE == QMHIP_ERR_STATE, "qm_rollout_pipeline.h restates the error codes of qmhip.h");
static_assert(QM_EP_OK == QMHIP_OK && QM_EP_ERR_ARG == QMHIP_ERR_ARG && QM_EP_ERR_STATE == QMHIP_ERR_STATE && sizeof(QmEpisodeParams) == sizeof(qmhip_episode_params), "qm_episode_pipeline.h restates the error codes and the parameter struct of qmhip.h");

static thread_local std::string g_create_error;      // per calling thread: qmhip_last_error(NULL) is the error of THIS thread's last failed create

// every entry point that takes a context serialises on it: calls from several threads are safe and run one after another (include/qmhip.h, "Threads")
#define QM_GUARD(c) std::unique_lock<std::recursive_mutex> qm_lk_; if (c) qm_lk_ = std::unique_lock<std::recursive_mutex>(const_cast<qmhip_ctx*>(c)->mu)
// entry points that touch horizon / front-end / plant buffers refuse a WBC-only context
#define QM_NEED_MPC(c) do { if ((c) && (c)->wbc_only) { const_cast<qmhip_ctx*>(c)->fail(std::string(__func__) + ": not available on a WBC-only context (qmhip_create_wbc_context)"); return QMHIP_ERR_STATE; } } while (0)
#define HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (ctx)->fail(std::string(#expr) + ": " + hipGetErrorString(e_)); return QMHIP_ERR_HIP; } } while (0)

struct HipBackend {
  hipStream_t stream = nullptr;            // MPC stream (K0..K5); host copies
  hipStream_t stream_b = nullptr;          // WBC stream: the WBC of step k runs beside the MPC kernels of step k + 1 (the reference runs them in two threads too)
  hipStream_t stream_c = nullptr;          // copy stream of the streamed step I/O (qm_io_pipeline.h): the record of step k travels to the host beside the kernels of step k + 1; carries copies only; created by the first qmhip_step_submit
  hipStream_t cur = nullptr;               // stream the next launch / memset goes to
  hipEvent_t ev_in = nullptr, ev_wbc = nullptr; bool wbc_pending = false;
  int profiling = 0;   // 0 off, 1 HIP-event span around every launch, 2 only around the modelled kernels (lq, riccati, wbc), 3 only around the LQ kernel (the dominant one: what the bench's timed region carries): two event records cost ≈ a launch
  std::string error;
  struct Span { std::string name; hipEvent_t a, b; };
  std::vector<Span> spans; std::vector<hipEvent_t> pool;
  std::map<std::string, std::pair<double, int>> acc;
  std::map<const void*, int> lds_set;
  std::map<std::string, int> lds_pad;      // profiling only (occupancy sweep, tools/occupancy_sweep.py): extra dynamic LDS per workgroup of a kernel group -> fewer resident workgroups per CU
  hipEvent_t ev() { if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; } hipEvent_t e = nullptr; check(hipEventCreate(&e), "hipEventCreate"); return e; }
  void check(hipError_t e, const char* what) { if (e != hipSuccess && error.empty()) error = std::string(what) + ": " + hipGetErrorString(e); }
  template <class K> const char* name_of(K k) {
    const void* p = (const void*)k;
    if (p == (const void*)qm_grid_kernel || p == (const void*)qm_grid_nodes_kernel || p == (const void*)qm_save_grid_kernel || p == (const void*)qm_advance_kernel) return "grid"; if (p == (const void*)qm_lq_kernel || p == (const void*)qm_lq_dbg_kernel || p == (const void*)qm_lq_ipm_kernel) return "lq"; if (p == (const void*)qm_lq_m18_kernel) return "lq_m18"; if (p == (const void*)qm_lq_kin_kernel) return "lq_kin"; if (p == (const void*)qm_riccati_kernel || p == (const void*)qm_riccati_prof_kernel) return "riccati";
    if (p == (const void*)qm_ls_eval_kernel || p == (const void*)qm_ls_eval_dense_kernel || p == (const void*)qm_ls_eval_ipm_kernel) return "ls_eval";
    if (p == (const void*)qm_ipm_init_kernel || p == (const void*)qm_ipm_dir_kernel || p == (const void*)qm_ipm_alpha_kernel || p == (const void*)qm_ipm_commit_kernel || p == (const void*)qm_ipm_barrier_kernel) return "ipm"; if (p == (const void*)qm_ilqr_rollout_kernel || p == (const void*)(QmPolicyRolloutFn)qm_policy_rollout_kernel<QmFbStageView, SR_SIZE, false> || p == (const void*)(QmPolicyRolloutFn)qm_policy_rollout_kernel<QmFbPubView, PR_SIZE, true>) return "rollout"; if (p == (const void*)qm_sim_kernel || p == (const void*)qm_sim_push_kernel || p == (const void*)qm_sim_terrain_kernel || p == (const void*)qm_sim_terrain_push_kernel) return "sim"; if (p == (const void*)qm_terrain_eval_kernel) return "terrain_eval"; if (p == (const void*)qm_sense_kernel) return "sense"; if (p == (const void*)qm_wbc_kernel || p == (const void*)qm_wbc_prof_kernel) return "wbc"; if (p == (const void*)qm_policy_kernel || p == (const void*)qm_policy_measured_kernel) return "policy"; if (p == (const void*)qm_policy_fb_kernel || p == (const void*)qm_policy_fb_pub_kernel) return "policy_fb"; if (p == (const void*)qm_policy_publish_kernel) return "publish"; if (p == (const void*)qm_hoqp_kernel) return "hoqp"; if (p == (const void*)qm_step_pack_kernel) return "io"; if (p == (const void*)qm_tick_state_kernel || p == (const void*)qm_tick_pack_kernel) return "tick"; if (p == (const void*)qm_plan_nodes_kernel) return "plan_nodes"; if (p == (const void*)qm_plan_states_kernel) return "plan_states"; if (p == (const void*)qm_plan_footholds_kernel) return "plan_footholds"; if (p == (const void*)qm_episode_tick_kernel || p == (const void*)qm_episode_mpc_kernel || p == (const void*)qm_episode_start_kernel) return "episode";
    return "ls_misc";
  }
  template <class K, class A> void launch(K kernel, int grid, int block, size_t lds, const A& args) {
    if (grid <= 0) return;
    if (!lds_pad.empty()) { auto it = lds_pad.find(name_of(kernel)); if (it != lds_pad.end()) lds += (size_t)it->second; }
    if (lds > 48 * 1024) {
      const void* p = (const void*)kernel; auto it = lds_set.find(p);
      if (it == lds_set.end() || it->second < (int)lds) { check(hipFuncSetAttribute(p, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute"); lds_set[p] = (int)lds; }
    }
    const void* kp_ = (const void*)kernel;
    const bool is_lq_ = kp_ == (const void*)qm_lq_kernel || kp_ == (const void*)qm_lq_m18_kernel || kp_ == (const void*)qm_lq_ipm_kernel;
    const bool span = profiling == 1 || (profiling == 3 && is_lq_) || (profiling == 2 && (kp_ == (const void*)qm_lq_kernel || kp_ == (const void*)qm_lq_m18_kernel || kp_ == (const void*)qm_lq_ipm_kernel || kp_ == (const void*)qm_riccati_kernel || kp_ == (const void*)qm_wbc_kernel));      // (lq_m18: launched only on workloads with a phase of three or four stance feet; bench.py prices lq + lq_m18 together)
    Span s; if (span) { s.name = name_of(kernel); s.a = ev(); s.b = ev(); check(hipEventRecord(s.a, cur), "hipEventRecord"); }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, cur, args);
    check(hipGetLastError(), "kernel launch");
    if (span) { check(hipEventRecord(s.b, cur), "hipEventRecord"); spans.push_back(s); }
  }
  void resolve() {
    if (spans.empty()) return;
    hipStreamSynchronize(stream); hipStreamSynchronize(stream_b);
    for (auto& s : spans) { float ms = 0; hipEventElapsedTime(&ms, s.a, s.b); auto& a = acc[s.name]; a.first += ms; a.second += 1; pool.push_back(s.a); pool.push_back(s.b); }
    spans.clear();
  }
  void* alloc(size_t n) { void* p = nullptr; check(hipMalloc(&p, n ? n : 8), "hipMalloc"); return p; }
  void free(void* p) { hipFree(p); }
  void zero(void* p, size_t n) { check(hipMemsetAsync(p, 0, n, cur), "hipMemsetAsync"); }
  // host copies see the results of BOTH streams and never run beside device work of either (they are not on the hot path)
  void to_device(void* d, const void* s, size_t n) { sync(); check(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, stream), "H2D"); check(hipStreamSynchronize(stream), "sync"); }
  void to_host(void* d, const void* s, size_t n) { sync(); check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, stream), "D2H"); check(hipStreamSynchronize(stream), "sync"); }
  void sync() { check(hipStreamSynchronize(stream), "sync"); check(hipStreamSynchronize(stream_b), "sync"); wbc_pending = false; }
  // host-visible (pinned, mapped) memory for flags a kernel publishes: returns the device-side address, *host_view the host-side one
  hipEvent_t ev_order = nullptr;
  void stream_select(int s) { cur = s ? stream_b : stream; }
  void stream_order(int a, int b) { if (!ev_order) check(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming), "hipEventCreate"); check(hipEventRecord(ev_order, a ? stream_b : stream), "hipEventRecord"); check(hipStreamWaitEvent(b ? stream_b : stream, ev_order, 0), "hipStreamWaitEvent"); }
  void copy_dd(void* d, const void* s, size_t n) { check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, cur), "D2D"); }
  void* alloc_mapped(size_t n, void** host_view) { void* h = nullptr; void* dv = nullptr; check(hipHostMalloc(&h, n ? n : 8, hipHostMallocMapped), "hipHostMalloc"); check(hipHostGetDevicePointer(&dv, h, 0), "hipHostGetDevicePointer"); *host_view = h; return dv; }
  void free_mapped(void* host_view) { hipHostFree(host_view); }
  // streamed step I/O (qm_io_pipeline.h): pinned staging, asynchronous copies, one event per slot
  hipEvent_t ev_io_a = nullptr, ev_io_b = nullptr;
  void* alloc_pinned(size_t n) { void* h = nullptr; check(hipHostMalloc(&h, n ? n : 8, hipHostMallocDefault), "hipHostMalloc"); return h; }
  void free_pinned(void* p) { hipHostFree(p); }
  void* io_event() { hipEvent_t e = nullptr; check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate"); return (void*)e; }
  void io_event_free(void* e) { hipEventDestroy((hipEvent_t)e); }
  void copy_in(void* d, const void* s, size_t n, int on) { check(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, on ? stream_b : stream), "H2D"); }
  void copy_out(void* d, const void* s, size_t n, void* done, bool wbc) {
    if (!ev_io_a) { check(hipEventCreateWithFlags(&ev_io_a, hipEventDisableTiming), "hipEventCreate"); check(hipEventCreateWithFlags(&ev_io_b, hipEventDisableTiming), "hipEventCreate"); }
    check(hipEventRecord(ev_io_a, stream), "hipEventRecord"); check(hipStreamWaitEvent(stream_c, ev_io_a, 0), "hipStreamWaitEvent");
    if (wbc) { check(hipEventRecord(ev_io_b, stream_b), "hipEventRecord"); check(hipStreamWaitEvent(stream_c, ev_io_b, 0), "hipStreamWaitEvent"); }
    check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, stream_c), "D2H"); check(hipEventRecord((hipEvent_t)done, stream_c), "hipEventRecord");
  }
  void copy_back(void* d, const void* s, size_t n, void* done) { check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, stream), "D2H"); check(hipEventRecord((hipEvent_t)done, stream), "hipEventRecord"); }      // streamed controller tick (qm_tick_pipeline.h): depth one, so the record travels on the stream that produced it
  // published policy (qm_publish_pipeline.h): one event per slot and direction, on whichever stream is current
  void* pub_event() { return io_event(); }
  void pub_event_free(void* e) { io_event_free(e); }
  void pub_wait(void* e) { check(hipStreamWaitEvent(cur, (hipEvent_t)e, 0), "hipStreamWaitEvent"); }
  void pub_record(void* e) { check(hipEventRecord((hipEvent_t)e, cur), "hipEventRecord"); }
  void io_wait(void* done) { check(hipEventSynchronize((hipEvent_t)done), "hipEventSynchronize"); }
  // wait for a host-visible word a kernel already launched on `cur` overwrites (anything but `pending`): a BOUNDED spin — a stream synchronisation costs 10-30 us of
  // wake-up latency, which matters for a line-search trial of a few tens of microseconds, but a solve must not hold a host core beside the ros_control thread for its
  // whole length — of at most spin_us microseconds (the trial kernels of a 1024-batch take ≈ 0.25 ms), then the stream synchronisation
  int spin_us = 400;
  void wait_flag(volatile int* word, int pending) {
    if (*word != pending) return;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      for (int k = 0; k < 256; ++k) if (*word != pending) return;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
    }
    check(hipStreamSynchronize(stream), "sync"); if (cur != stream) check(hipStreamSynchronize(cur), "sync");
    if (*word == pending && error.empty()) error = "a kernel did not publish its host-visible word";
  }
  // WBC of the current step on stream_b: its inputs were produced on `stream` (ev_in); the next producers on `stream` wait for ev_wbc
  void wbc_inputs_next() { if (wbc_pending) { check(hipStreamWaitEvent(stream, ev_wbc, 0), "hipStreamWaitEvent"); wbc_pending = false; } }
  void wbc_begin() { check(hipEventRecord(ev_in, stream), "hipEventRecord"); check(hipStreamWaitEvent(stream_b, ev_in, 0), "hipStreamWaitEvent"); cur = stream_b; }
  void wbc_end() { check(hipEventRecord(ev_wbc, stream_b), "hipEventRecord"); cur = stream; wbc_pending = true; }
};

// the two queues of the policy rollout (qm_rollout_pipeline.h).  Source 0: the MPC stream through the backend (profiling spans, the backend's error word), under the context
// lock.  Source 1: the published policy's stream with raw calls and an error word of its own: it runs under the publication mutex and must not touch the backend's state
struct RolloutQueueMpc {
  HipBackend& bk;
  void* alloc(size_t n) { return bk.alloc(n); }
  void free(void* p) { bk.free(p); }
  void* alloc_pinned(size_t n) { return bk.alloc_pinned(n); }
  void free_pinned(void* p) { bk.free_pinned(p); }
  void ro_in(void* d, const void* s, size_t n) { bk.check(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, bk.stream), "H2D"); }
  template <class K, class A> void launch(K kernel, int grid, int block, size_t lds, const A& args) { bk.cur = bk.stream; bk.launch(kernel, grid, block, lds, args); }
  void ro_out(void* d, const void* s, size_t n) { bk.check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, bk.stream), "D2H"); }
  void ro_wait() { bk.check(hipStreamSynchronize(bk.stream), "sync"); }
};
struct RolloutQueuePub {
  hipStream_t* sp; std::string error;
  void check(hipError_t e, const char* what) { if (e != hipSuccess && error.empty()) error = std::string(what) + ": " + hipGetErrorString(e); }
  void* alloc(size_t n) { void* p = nullptr; check(hipMalloc(&p, n ? n : 8), "hipMalloc"); return p; }
  void free(void* p) { hipFree(p); }
  void* alloc_pinned(size_t n) { void* h = nullptr; check(hipHostMalloc(&h, n ? n : 8, hipHostMallocDefault), "hipHostMalloc"); return h; }
  void free_pinned(void* p) { hipHostFree(p); }
  void ro_in(void* d, const void* s, size_t n) { check(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, *sp), "H2D"); }
  template <class K, class A> void launch(K kernel, int grid, int block, size_t lds, const A& args) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, *sp, args); check(hipGetLastError(), "kernel launch"); }
  void ro_out(void* d, const void* s, size_t n) { check(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, *sp), "D2H"); }
  void ro_wait() { check(hipStreamSynchronize(*sp), "sync"); }
};

struct qmhip_ctx {
  int device = 0, max_batch = 0, max_nodes = 0, max_ref = 0, max_ev = 0;
  double mb[MB_SIZE], st[ST_SIZE];
  HipBackend bk; QmMpcPipeline<HipBackend> mpc; QmWbcPipeline<HipBackend> wbc; QmFrontPipeline<HipBackend> front; QmSimPipeline<HipBackend> sim; QmHoqpPipeline<HipBackend> hoqp; QmIoPipeline<HipBackend> io; QmTickPipeline<HipBackend> tick; QmPublishPipeline<HipBackend> pub; QmPlanPipeline<HipBackend> plan; QmEpisodePipeline<HipBackend> episode;
  // qmhip_policy_eval_published: a stream, staging and device buffers of its own, serialised among evaluators by eval_mu — an evaluation never takes `mu` below
  std::mutex eval_mu; hipStream_t stream_p = nullptr; char* pe_pin = nullptr; char* pe_dev = nullptr;
  // qmhip_policy_rollout: source 0 on the MPC stream under `mu`, source 1 on stream_p under eval_mu — a queue and row buffers each (qm_rollout_pipeline.h)
  RolloutQueueMpc ro_q{bk}; RolloutQueuePub ro_qp{&stream_p, std::string()}; QmRolloutPipeline<RolloutQueueMpc> rollout{ro_q}; QmRolloutPipeline<RolloutQueuePub> rollout_p{ro_qp};
  std::recursive_mutex mu;      // serialises the entry points of this context
  bool wbc_only = false;        // created by qmhip_create_wbc_context: carries the model + the WBC buffers, no horizon buffers
  void* dl_dev = nullptr; void* dl_pin = nullptr; size_t dl_cap = 0;      // staging of qmhip_mpc_download (device transpose buffer + its pinned host mirror), allocated on first use
  char* tick_pin = nullptr;     // pinned host staging of the control-tick path (qmhip_wbc_step): [inputs of max_batch instances | outputs]
  std::string error; int lastB = 0; bool have_solution = false; int front_B = 0; long sim_ticks = 0;
  hipEvent_t ev_meas = nullptr; bool meas_pending = false;      // streamed step I/O: "the synthetic measured state of the last submitted step has read x0" (the next submit's copy of x0 waits for it on the device)
  qmhip_ctx() : mpc(bk), wbc(bk), front(bk), sim(bk), hoqp(bk), io(bk), tick(bk), pub(bk), plan(bk), episode(bk) {}
  void fail(const std::string& m) { error = m; }
  // getModeSchedule on the device GaitSchedule -> the solver's schedule buffers; from here on its sticky status speaks for the schedule of this batch (until the host supplies one)
  void gait_schedule(int B, double horizon) { front.gait_schedule(mpc.d, B, horizon); mpc.front_status = front.f.gs_status; mpc.front_B = B; }
  // sqp.sqpIteration (task.info:79, shipped 1): SQP iterations per MPC call [upstream SqpSolver::runImpl loop]; every instance of the batch runs all of
  // them (an instance whose line search finds no step just keeps its iterate)
  int sqp_iterations() const { const int n = (int)qm_ms_param(st, ST_SQP_ITER); return n < 1 ? 1 : (n > 50 ? 50 : n); }      // ipm.ipmIteration with solver 2
  bool fused_policy = true;      // the policy at t0 comes from the line search's deciding kernels and the batch's apply runs behind the WBC launch (qm_pipeline.h); false: qm_policy_kernel behind the apply (rounds 1-5; qmhip_debug_set "fused_policy")
  // One control step on resident data, everything enqueued, nothing waited for:
  //   WBC stream: the synthetic measured state of this step (a function of x0 only) — early, beside the MPC kernels
  //   MPC stream: K0 .. K4; the kernels that DECIDE the step length also write the policy at t0 (what evaluatePolicy(t0) reads from x + alpha dx)
  //   WBC stream: waits for that decision, then the WBC;   MPC stream: the batch's apply (the primal solution on every node) runs beside it, then the next step
  // Rounds 1-5 had apply -> policy kernel -> WBC on the critical path: 2 launches and ~ 60 us of a 2.7 ms step.
  // streamed (qmhip_step_submit only): the caller's x0 arrives by an asynchronous copy, so the step notes when its measured-state kernel has read x0; meas_given: the
  // caller supplied the measured state (already on its way into w.rbd / w.time on the WBC stream) — no synthetic one
  void control_step(int B, double horizon, double period, double time, bool warm, bool streamed = false, bool meas_given = false) {
    if (!meas_given) { bk.stream_order(0, 1); bk.cur = bk.stream_b; wbc.measured_from_x0(mpc.d, B, time); bk.cur = bk.stream; }      // (x0 is final on the MPC stream at this point; the previous WBC on this stream has read its rbd)
    if (streamed && !meas_given) { bk.check(hipEventRecord(ev_meas, bk.stream_b), "hipEventRecord"); meas_pending = true; }
    mpc.p0_x = wbc.w.x_des; mpc.p0_u = wbc.w.u_des; mpc.p0_mode = wbc.w.mode;
    mpc.grid(B, horizon, warm);
    for (int it = 0, ni = sqp_iterations(); it < ni; ++it) { const bool last_it = it + 1 == ni; mpc.p0_enable = fused_policy && last_it; mpc.defer_apply = fused_policy && last_it; mpc.sqp_iteration(B, 14, last_it); }
    mpc.p0_enable = false; mpc.defer_apply = false; lastB = B; have_solution = true;
    if (!mpc.p0_done) { mpc.apply_pending(); bk.wbc_inputs_next(); wbc.policy_eval_at_t0(mpc.d, B); }      // iLQR / interior-point solver / host-driven line search: the policy kernel on the applied primal solution
    bk.wbc_begin(); wbc.step(mpc.d, B, period, 0); bk.wbc_end();
    mpc.apply_pending();
  }
  // the MPC half of a control step alone (qmhip_step_submit without QMHIP_STEP_WBC): K0, the SQP iterations, the policy at t0 — no measured state, no WBC launch
  void mpc_step(int B, double horizon, bool warm) {
    mpc.p0_x = wbc.w.x_des; mpc.p0_u = wbc.w.u_des; mpc.p0_mode = wbc.w.mode;
    mpc.grid(B, horizon, warm);
    for (int it = 0, ni = sqp_iterations(); it < ni; ++it) { const bool last_it = it + 1 == ni; mpc.p0_enable = fused_policy && last_it; mpc.sqp_iteration(B, 14, last_it); }
    mpc.p0_enable = false; lastB = B; have_solution = true;
    if (!mpc.p0_done) { bk.wbc_inputs_next(); wbc.policy_eval_at_t0(mpc.d, B); }
  }
  int hipstate() { if (!bk.error.empty()) { error = bk.error; bk.error.clear(); return QMHIP_ERR_HIP; } return QMHIP_OK; }
};

// ---- FP64 micro-benchmarks (roofline denominators) ----
__global__ void qm_bench_fma_kernel(double* out, int iters) {
  double a0 = threadIdx.x * 1e-9, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7; const double m = 1.0000001, c = 1e-9;
  for (int i = 0; i < iters; ++i) { a0 = fma(a0, m, c); a1 = fma(a1, m, c); a2 = fma(a2, m, c); a3 = fma(a3, m, c); a4 = fma(a4, m, c); a5 = fma(a5, m, c); a6 = fma(a6, m, c); a7 = fma(a7, m, c); }
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}
__global__ void qm_bench_mfma_kernel(double* out, int iters) {
  qm_d4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0; const double a = 1.0 + threadIdx.x * 1e-9, b = 1e-9;
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0); c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c2, 0, 0, 0); c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c3, 0, 0, 0);
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
}

// settings whose value the kernels' loop bounds depend on (K0 walks t0 + k dt up to the horizon)
static bool setting_ok(int idx, double v) {
  if (idx == ST_SQP_DT || idx == ST_IPM_DT) return v > 0.0 && std::isfinite(v);
  if (idx == ST_GRID_DT_MIN) return v >= 0.0 && std::isfinite(v);
  if (idx == ST_RICCATI_STRICT || idx == ST_IPM_PRIMAL_FOR_DUAL || idx == ST_FEEDBACK_POLICY) return v == 0.0 || v == 1.0;
  // interior-point solver (slot 3, k_ipm.h): the barrier parameter and the slack / dual floors are divided by and go through log(); the margin and the linear factor are fractions
  if (idx == ST_IPM_MU || idx == ST_IPM_MU_TARGET || idx == ST_IPM_SLACK_LB || idx == ST_IPM_DUAL_LB) return v > 0.0 && std::isfinite(v);
  if (idx == ST_IPM_FTB_MARGIN || idx == ST_IPM_MU_LINEAR) return v > 0.0 && v < 1.0;
  if (idx == ST_IPM_MU_POWER) return v > 1.0 && std::isfinite(v);
  if (idx == ST_IPM_SLACK_MARGIN || idx == ST_IPM_DUAL_MARGIN) return v >= 0.0 && std::isfinite(v);
  return true;
}
// the slots the interior-point solver reads: all of them must hold before solver 3 may run (a blob of the 1048-double layout has zeros there: division by zero in qm_ipm_dir_kernel, log(0) in the merit)
static const int kIpmSlots[] = {ST_IPM_DT, ST_IPM_MU, ST_IPM_MU_TARGET, ST_IPM_MU_LINEAR, ST_IPM_MU_POWER, ST_IPM_FTB_MARGIN, ST_IPM_PRIMAL_FOR_DUAL, ST_IPM_SLACK_LB, ST_IPM_DUAL_LB, ST_IPM_SLACK_MARGIN, ST_IPM_DUAL_MARGIN};
static bool ipm_settings_ok(const double* st) { for (int i : kIpmSlots) if (!setting_ok(i, st[i])) return false; return true; }

static int create_common(const double* mb, const double* st, int device, int max_batch, int max_nodes, int max_ref, int max_ev, qmhip_ctx** out, bool wbc_only = false) {
  if (!out || max_batch <= 0 || max_nodes < 3 || max_nodes > RW_MAXNODES || max_ref < 1 || max_ev < 1) { g_create_error = "qmhip_create: bad argument (max_nodes must be in [3, 512])"; return QMHIP_ERR_ARG; }
  std::string err; if (!qmio::validateModelBlob(mb, err)) { g_create_error = err; return QMHIP_ERR_MODEL; }
  if (!setting_ok(ST_SQP_DT, st[ST_SQP_DT])) { g_create_error = "settings blob: sqp.dt must be a positive finite number"; return QMHIP_ERR_MODEL; }
  // a blob of an older layout (no size / version stamp travels with it) would put garbage into the slots added since: check the ones a kernel's control flow depends on
  if (!setting_ok(ST_GRID_DT_MIN, st[ST_GRID_DT_MIN])) { g_create_error = "settings blob: the time grid's minimum step (ST_GRID_DT_MIN) must be a non-negative finite number - is the blob of an older layout (ST_SIZE)?"; return QMHIP_ERR_MODEL; }
  if (st[ST_RICCATI_STRICT] != 0.0 && st[ST_RICCATI_STRICT] != 1.0) { g_create_error = "settings blob: ST_RICCATI_STRICT must be 0 or 1 - is the blob of an older layout (ST_SIZE)?"; return QMHIP_ERR_MODEL; }
  if (st[ST_FEEDBACK_POLICY] != 0.0 && st[ST_FEEDBACK_POLICY] != 1.0) { g_create_error = "settings blob: ST_FEEDBACK_POLICY must be 0 or 1 - is the blob of an older layout (ST_SIZE)?"; return QMHIP_ERR_MODEL; }
  if (st[ST_SOLVER] != 0.0 && st[ST_SOLVER] != 1.0 && st[ST_SOLVER] != 2.0 && st[ST_SOLVER] != 3.0) { g_create_error = "settings blob: ST_SOLVER must be 0, 1, 2 or 3"; return QMHIP_ERR_MODEL; }
  if (st[ST_SOLVER] == 3.0 && !ipm_settings_ok(st)) { g_create_error = "settings blob: ST_SOLVER = 3 needs the ipm block's slots (ST_IPM_*: barrier parameters, slack / dual floors > 0, margin and linear factor in (0, 1), power > 1) - is the blob of an older layout (ST_SIZE)?"; return QMHIP_ERR_MODEL; }
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device available (libqmhip has no CPU fallback)"; return QMHIP_ERR_HIP; }
  if (device < 0 || device >= ndev) { g_create_error = "device index out of range"; return QMHIP_ERR_ARG; }
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return QMHIP_ERR_HIP; }
  qmhip_ctx* c = new qmhip_ctx(); c->device = device; c->max_batch = max_batch; c->max_nodes = max_nodes; c->max_ref = max_ref; c->max_ev = max_ev;
  memcpy(c->mb, mb, sizeof(c->mb)); memcpy(c->st, st, sizeof(c->st));
  int lo = 0, hi = 0; hipDeviceGetStreamPriorityRange(&lo, &hi); const bool sb_ok = hipStreamCreateWithPriority(&c->bk.stream_b, hipStreamDefault, hi) == hipSuccess;      // the WBC / control-tick stream at the highest priority: its waves get the SIMDs first (- 0.4 % of the pipelined step, profiles/r06_ab_wbc_schedule.log)
  if (hipStreamCreate(&c->bk.stream) != hipSuccess || !sb_ok) { g_create_error = "hipStreamCreate failed"; delete c; return QMHIP_ERR_HIP; }
  c->bk.cur = c->bk.stream; hipEventCreateWithFlags(&c->bk.ev_in, hipEventDisableTiming); hipEventCreateWithFlags(&c->bk.ev_wbc, hipEventDisableTiming);
  c->wbc_only = wbc_only;
  c->mpc.allocate(c->mb, c->st, wbc_only ? 1 : max_batch, max_nodes, max_ref, max_ev, false); c->mpc.solver = (int)st[ST_SOLVER];
  c->wbc.allocate(max_batch);
  if (!wbc_only) c->front.allocate(max_batch);
  { void* h = nullptr; c->bk.check(hipHostMalloc(&h, QmWbcPipeline<HipBackend>::in_bytes(max_batch) + QmWbcPipeline<HipBackend>::out_bytes(max_batch), hipHostMallocDefault), "hipHostMalloc"); c->tick_pin = (char*)h; }
  c->bk.sync();
  if (!c->bk.error.empty()) { g_create_error = c->bk.error; c->mpc.release(); c->wbc.release(); c->front.release(); if (c->tick_pin) hipHostFree(c->tick_pin); hipStreamDestroy(c->bk.stream); hipStreamDestroy(c->bk.stream_b); delete c; return QMHIP_ERR_HIP; }
  *out = c; return QMHIP_OK;
}

extern "C" {

int qmhip_parse_model(const char* urdf, const char* task, const char* ref, double* mb, double* st) {
  if (!urdf || !task || !ref || !mb || !st) { g_create_error = "qmhip_parse_model: null argument"; return QMHIP_ERR_ARG; }
  // same checks (and order) as QMInterface's constructor, QMInterface.cpp:40-62
  if (!qmio::fileExists(task)) { g_create_error = std::string("[QMInterface] Task file not found: ") + task; return QMHIP_ERR_FILE; }
  if (!qmio::fileExists(urdf)) { g_create_error = std::string("[QMInterface] URDF file not found: ") + urdf; return QMHIP_ERR_FILE; }
  if (!qmio::fileExists(ref)) { g_create_error = std::string("[QMInterface] targetCommand file not found: ") + ref; return QMHIP_ERR_FILE; }
  std::string ee, err;
  if (!qmio::loadEeFrameName(task, ee, err) || !qmio::buildModelBlob(urdf, ref, ee, mb, nullptr, err) || !qmio::buildSettingsBlob(task, mb, st, err)) { g_create_error = err; return QMHIP_ERR_MODEL; }
  return QMHIP_OK;
}
int qmhip_create(const char* urdf, const char* task, const char* ref, int device, int max_batch, int max_nodes, int max_ref, int max_ev, qmhip_ctx** out) {
  std::vector<double> mb(MB_SIZE), st(ST_SIZE);
  const int rc = qmhip_parse_model(urdf, task, ref, mb.data(), st.data()); if (rc != QMHIP_OK) return rc;
  return create_common(mb.data(), st.data(), device, max_batch, max_nodes, max_ref, max_ev, out);
}
int qmhip_create_from_blobs(const double* mb, const double* st, int device, int max_batch, int max_nodes, int max_ref, int max_ev, qmhip_ctx** out) {
  if (!mb || !st) { g_create_error = "qmhip_create_from_blobs: null blob"; return QMHIP_ERR_ARG; }
  return create_common(mb, st, device, max_batch, max_nodes, max_ref, max_ev, out);
}
int qmhip_create_wbc_context(const qmhip_ctx* c, int max_batch, qmhip_ctx** out) { QM_GUARD(c);
  if (!c || !out || max_batch <= 0) { g_create_error = "qmhip_create_wbc_context: bad argument"; return QMHIP_ERR_ARG; }
  return create_common(c->mb, c->st, c->device, max_batch, 3, 1, 1, out, true);      // same model / settings values, own device copies, own streams: nothing mutable is shared
}
void qmhip_destroy(qmhip_ctx* c) {
  if (!c) return; hipSetDevice(c->device); c->bk.sync(); if (c->bk.stream_c) hipStreamSynchronize(c->bk.stream_c); c->io.release(); c->tick.release(); if (c->stream_p) hipStreamSynchronize(c->stream_p); c->pub.release(); c->plan.release(); c->episode.release(); c->rollout.release(); c->rollout_p.release(); if (c->pe_pin) hipHostFree(c->pe_pin); if (c->pe_dev) hipFree(c->pe_dev); if (c->stream_p) hipStreamDestroy(c->stream_p); if (c->ev_meas) hipEventDestroy(c->ev_meas); if (c->bk.ev_io_a) { hipEventDestroy(c->bk.ev_io_a); hipEventDestroy(c->bk.ev_io_b); } if (c->dl_dev) hipFree(c->dl_dev); if (c->dl_pin) hipHostFree(c->dl_pin); if (c->tick_pin) hipHostFree(c->tick_pin); c->mpc.release(); c->wbc.release(); c->front.release(); c->sim.release(); c->hoqp.release();
  for (auto e : c->bk.pool) hipEventDestroy(e); if (c->bk.ev_order) hipEventDestroy(c->bk.ev_order); hipEventDestroy(c->bk.ev_in); hipEventDestroy(c->bk.ev_wbc); hipStreamDestroy(c->bk.stream); hipStreamDestroy(c->bk.stream_b); if (c->bk.stream_c) hipStreamDestroy(c->bk.stream_c); delete c;
}
// the text is copied under the context lock into a per-thread buffer: the pointer stays valid (until this THREAD's next qmhip_last_error) even if another thread's
// failing call on the same context replaces the context's message meanwhile
const char* qmhip_last_error(const qmhip_ctx* c) { static thread_local std::string copy; QM_GUARD(c); if (!c) return g_create_error.c_str(); copy = c->error; return copy.c_str(); }
int qmhip_export_blobs(const qmhip_ctx* c, double* mb, double* st) { QM_GUARD(c); if (!c) return QMHIP_ERR_ARG; if (mb) memcpy(mb, c->mb, sizeof(c->mb)); if (st) memcpy(st, c->st, sizeof(c->st)); return QMHIP_OK; }
// name of a field of qm_wbc::WbcWeightConfig (cfg/wbcWigeht.cfg:7-47) -> settings slot of the gain WbcBase::dynamicCallback stores it in (WbcBase.cpp:69-116)
int qmhip_wbc_gain_index(const char* name) {
  if (!name) return -1;
  static const struct { const char* name; int idx; } scalars[] = {{"kp_swing", ST_KP_SWING}, {"kd_swing", ST_KD_SWING}, {"baseHeightKp", ST_KP_BASE_H}, {"baseHeightKd", ST_KD_BASE_H},
    {"kp_base_linear", ST_KP_BASE_LIN}, {"kd_base_linear", ST_KD_BASE_LIN}, {"kp_base_angular", ST_KP_BASE_ANG}, {"kd_base_angular", ST_KD_BASE_ANG}};
  for (const auto& e : scalars) if (!strcmp(name, e.name)) return e.idx;
  static const struct { const char* prefix; int base; } joints[] = {{"kp_arm_joint_", ST_KP_ARM_J}, {"kd_arm_joint_", ST_KD_ARM_J}};
  for (const auto& e : joints) { const size_t n = strlen(e.prefix); if (!strncmp(name, e.prefix, n) && name[n] >= '1' && name[n] <= '6' && name[n + 1] == 0) return e.base + (name[n] - '1'); }
  static const struct { const char* prefix; int base; } axes[] = {{"kp_ee_linear_", ST_KP_EE_LIN}, {"kd_ee_linear_", ST_KD_EE_LIN}, {"kp_ee_angular_", ST_KP_EE_ANG}, {"kd_ee_angular_", ST_KD_EE_ANG}};
  for (const auto& e : axes) { const size_t n = strlen(e.prefix); if (!strncmp(name, e.prefix, n) && name[n] >= 'x' && name[n] <= 'z' && name[n + 1] == 0) return e.base + (name[n] - 'x'); }
  return -1;
}
int qmhip_set_setting(qmhip_ctx* c, int idx, double v) { QM_GUARD(c);
  if (!c || idx < 0 || idx >= ST_SIZE) return QMHIP_ERR_ARG;
  if (!setting_ok(idx, v)) { c->fail("qmhip_set_setting: sqp.dt / ipm.dt must be a positive finite number, the grid's minimum step a non-negative one, ST_RICCATI_STRICT and ST_FEEDBACK_POLICY 0 or 1; ipm block: barrier parameters and slack / dual floors > 0, margin and linear decrease factor in (0, 1), superlinear power > 1, margin rates >= 0"); return QMHIP_ERR_ARG; }
  if (idx == ST_SOLVER && v == 3.0 && !ipm_settings_ok(c->st)) { c->fail("qmhip_set_setting: solver 3 needs valid ipm settings (ST_IPM_*) - is the settings blob of an older layout?"); return QMHIP_ERR_ARG; }
  if (idx == ST_SOLVER && v >= 2.0 && !setting_ok(ST_IPM_DT, c->st[ST_IPM_DT])) { c->fail("qmhip_set_setting: solvers 2 / 3 need a positive finite ipm.dt"); return QMHIP_ERR_ARG; }
  if (idx == ST_SOLVER) { if (v != 0.0 && v != 1.0 && v != 2.0 && v != 3.0) { c->fail("qmhip_set_setting: ST_SOLVER is 0 (SQP), 1 (discrete iLQR), 2 (the SQP step on the `ipm` block's parameters) or 3 (interior-point method with hard friction cones / arm boxes)"); return QMHIP_ERR_ARG; } c->mpc.solver = (int)v; c->mpc.solved_B = 0; c->have_solution = false; c->mpc.ipm_fresh = true; }      // (a solver switch starts the interior-point state over: slack / dual / barrier parameter of an earlier solve are not carried across)
  hipSetDevice(c->device); c->st[idx] = v; c->bk.to_device(c->mpc.d.st + idx, &v, 8); c->mpc.note_settings(c->st); return c->hipstate();
}

int qmhip_mpc_upload(qmhip_ctx* c, int B, const double* t0, const double* x0, int n_ref, const double* ref_t, const double* ref_x, int n_ev, const double* ev, const int32_t* modes) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (B <= 0 || B > c->max_batch || n_ref != c->max_ref || n_ev != c->max_ev || !t0 || !x0 || !ref_t || !ref_x || !ev || !modes) { c->fail("qmhip_mpc_upload: bad argument (B <= max_batch, n_ref == max_ref_knots, n_events == max_events required)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->mpc.upload_inputs(B, t0, x0, ref_t, ref_x, ev, modes); c->mpc.solved_B = 0; c->lastB = B; c->have_solution = false;
  c->mpc.front_status = nullptr; c->mpc.front_B = 0;      // the schedule now comes from the host: a failed device GaitSchedule update no longer speaks for it (re-attached by the next qmhip_gait_update_resident)
 return c->hipstate();
}
int qmhip_mpc_solve_resident(qmhip_ctx* c, int B, double horizon) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !(horizon > 0)) { if (c) c->fail("qmhip_mpc_solve_resident: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->mpc.grid(B, horizon); for (int it = 0, ni = c->sqp_iterations(); it < ni; ++it) c->mpc.sqp_iteration(B, 14, it + 1 == ni); c->lastB = B; c->have_solution = true; return c->hipstate();
}
int qmhip_mpc_set_initial(qmhip_ctx* c, int B, const double* t0, const double* x0) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !t0 || !x0) { if (c) c->fail("qmhip_mpc_set_initial: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->bk.to_device(c->mpc.d.t0, t0, (size_t)B * 8); c->bk.to_device(c->mpc.d.x0, x0, (size_t)B * 30 * 8); return c->hipstate();
}
int qmhip_mpc_update_references(qmhip_ctx* c, int B, int n_ref, const double* ref_t, const double* ref_x, int n_ev, const double* ev, const int32_t* modes) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (B <= 0 || B != c->lastB || (!ref_t != !ref_x) || (!ev != !modes) || (ref_t && n_ref != c->max_ref) || (ev && n_ev != c->max_ev)) {
    c->fail("qmhip_mpc_update_references: bad argument (B == batch of the last upload, n_ref == max_ref_knots, n_events == max_events required; arrays come in pairs)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device);
  if (ref_t) { c->bk.to_device(c->mpc.d.ref_t, ref_t, (size_t)B * n_ref * 8); c->bk.to_device(c->mpc.d.ref_x, ref_x, (size_t)B * n_ref * QM_NREF * 8); }
  if (ev) { c->bk.to_device(c->mpc.d.ev, ev, (size_t)B * n_ev * 8); c->bk.to_device(c->mpc.d.modes, modes, (size_t)B * (n_ev + 1) * 4); c->mpc.front_status = nullptr; c->mpc.front_B = 0; }
  return c->hipstate();
}
int qmhip_mpc_solve_resident_warm(qmhip_ctx* c, int B, double horizon) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !(horizon > 0)) { if (c) c->fail("qmhip_mpc_solve_resident_warm: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->mpc.grid(B, horizon, true); for (int it = 0, ni = c->sqp_iterations(); it < ni; ++it) c->mpc.sqp_iteration(B, 14, it + 1 == ni); c->lastB = B; c->have_solution = true; return c->hipstate();
}
int qmhip_mpc_advance_resident(qmhip_ctx* c, int B, double dt) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_mpc_advance_resident: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->have_solution || c->mpc.solved_B != B) { c->fail("qmhip_mpc_advance_resident: no solution of this batch to advance along"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->mpc.advance(B, dt); return c->hipstate();
}
int qmhip_closed_loop_resident(qmhip_ctx* c, int B, int n_steps, double mpc_dt, double horizon, double period, double time0) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || n_steps <= 0 || !(horizon > 0) || !(period > 0)) { if (c) c->fail("qmhip_closed_loop_resident: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device);
  for (int k = 0; k < n_steps; ++k) {
    if (k > 0) c->mpc.advance(B, mpc_dt);
    if (c->front_B == B) c->gait_schedule(B, horizon);     // device-resident GaitSchedule active: modifyReferences before every MPC call
    c->control_step(B, horizon, period, time0 + k * mpc_dt, true);
  }
  return c->hipstate();
}
// ---- reference / gait front-end ----
int qmhip_gait_set_templates(qmhip_ctx* c, int n_gaits, const int32_t* n_phases, const double* switching_times, const int32_t* mode_sequence) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || n_gaits <= 0 || !n_phases || !switching_times || !mode_sequence) { if (c) c->fail("qmhip_gait_set_templates: bad argument"); return QMHIP_ERR_ARG; }
  for (int g = 0; g < n_gaits; ++g) if (n_phases[g] < 0 || n_phases[g] > QM_GAIT_MAX_PHASES) { c->fail("qmhip_gait_set_templates: a template has more than QMHIP_GAIT_MAX_PHASES phases"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->front.set_templates(n_gaits, n_phases, switching_times, mode_sequence); return c->hipstate();
}
int qmhip_gait_reset(qmhip_ctx* c, int B, int n_events, const double* event_times, const int32_t* mode_sequence, int default_template) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || n_events < 1 || n_events > QM_GAIT_EVENT_SLOTS || !event_times || !mode_sequence || default_template < 0 || default_template >= c->front.f.n_gaits) {
    if (c) c->fail("qmhip_gait_reset: bad argument (templates must be set first; the initial schedule needs at least one event)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->front.phase_transition_stance_time = c->st[ST_PHASE_TRANS_STANCE];
  c->front.gait_reset(B, n_events, event_times, mode_sequence, default_template); c->front_B = B; c->mpc.front_status = c->front.f.gs_status; c->mpc.front_B = B; return c->hipstate();
}
int qmhip_gait_insert_template(qmhip_ctx* c, int B, const int32_t* template_id, const double* start_time, const double* final_time) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B != c->front_B || !template_id || !start_time || !final_time) { if (c) c->fail("qmhip_gait_insert_template: bad argument (B must be the batch of qmhip_gait_reset)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->front.gait_insert(B, template_id, start_time, final_time); return c->hipstate();
}
int qmhip_gait_update_resident(qmhip_ctx* c, int B, double horizon) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B != c->front_B || !(horizon > 0)) { if (c) c->fail("qmhip_gait_update_resident: bad argument (B must be the batch of qmhip_gait_reset)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->gait_schedule(B, horizon); return c->hipstate();
}
int qmhip_gait_download(qmhip_ctx* c, int B, int32_t* n_events, double* event_times, int32_t* mode_sequence, int32_t* template_id, int32_t* status) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B != c->front_B || !n_events || !event_times || !mode_sequence || !template_id || !status) return QMHIP_ERR_ARG;
  hipSetDevice(c->device); c->front.gait_download(B, n_events, event_times, mode_sequence, template_id, status); return c->hipstate();
}
int qmhip_schedule_download(qmhip_ctx* c, int B, double* ev, int32_t* modes) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !ev || !modes) return QMHIP_ERR_ARG;
  if (B != c->lastB && B != c->front_B) { c->fail("qmhip_schedule_download: B differs from the batch size the schedule buffers were filled for"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.to_host(ev, c->mpc.d.ev, (size_t)B * c->max_ev * 8); c->bk.to_host(modes, c->mpc.d.modes, (size_t)B * (c->max_ev + 1) * 4); return c->hipstate();
}
int qmhip_target_reset(qmhip_ctx* c, int B, const double* last_ee_target) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !last_ee_target) return QMHIP_ERR_ARG;
  hipSetDevice(c->device); c->front.target_reset(B, last_ee_target); return c->hipstate();
}
int qmhip_target_from_command(qmhip_ctx* c, int B, const int32_t* kind, const double* cmd, const double* ee_state, int ee_through_float, const qmhip_target_params* p) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !kind || !cmd || !p || !(p->target_displacement_velocity > 0) || !(p->target_rotation_velocity > 0) || c->max_ref < 2) {
    if (c) c->fail("qmhip_target_from_command: bad argument (max_ref_knots >= 2 required)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device);
  c->front.target_from_command(c->mpc.d, B, kind, cmd, ee_state, ee_through_float, p->time_to_target, p->target_displacement_velocity, p->target_rotation_velocity, p->com_height);
  return c->hipstate();
}
int qmhip_target_download(qmhip_ctx* c, int B, double* ref_t, double* ref_x, double* last_ee_target) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) return QMHIP_ERR_ARG;
  hipSetDevice(c->device);
  if (ref_t) c->bk.to_host(ref_t, c->mpc.d.ref_t, (size_t)B * c->max_ref * 8);
  if (ref_x) c->bk.to_host(ref_x, c->mpc.d.ref_x, (size_t)B * c->max_ref * QM_NREF * 8);
  if (last_ee_target) c->bk.to_host(last_ee_target, c->front.f.last_ee, (size_t)B * 7 * 8);
  return c->hipstate();
}
int qmhip_mpc_download(qmhip_ctx* c, int B, int32_t* nn, double* ot, int32_t* oev, int32_t* omode, double* ox, double* ou, double* operf, int32_t* status) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) return QMHIP_ERR_ARG;
  if (!c->have_solution) { c->fail("qmhip_mpc_download: no solution available"); return QMHIP_ERR_STATE; }
  if (B != c->mpc.solved_B) { c->fail("qmhip_mpc_download: B differs from the batch size of the last solve (the solver buffers are strided by it)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); const int nm = c->max_nodes; const QmMpcBuffers& d = c->mpc.d;
  std::vector<int> n_h(B), st_h(B); c->bk.to_host(n_h.data(), d.n_nodes, (size_t)B * 4); c->bk.to_host(st_h.data(), d.status, (size_t)B * 4);
  std::vector<double> si((size_t)B * 4); c->bk.to_host(si.data(), d.step_info, si.size() * 8);
  for (int b = 0; b < B; ++b) { st_h[b] = qm_mpc_status(st_h[b], si.data() + (size_t)b * 4, c->st[ST_RICCATI_STRICT] != 0.0);      /* zeroed pivots of the degenerate stage: a warning; NaN / indefinite: -4 (qm_pipeline.h) */
    if (nn) nn[b] = n_h[b]; if (status) status[b] = st_h[b]; }
  // node-major [nmax][B][k] -> instance-major [B][nmax][k]: transposed by a kernel into a device staging buffer, copied through pinned memory (one contiguous
  // transfer per array; the per-node host loops this replaces took 20 ms of a 24 ms hand-over at B = 1024, bench.py `pcie_inclusive`)
  const size_t words = (size_t)nm * B * 30;
  if (c->dl_cap < words) { if (c->dl_dev) hipFree(c->dl_dev); if (c->dl_pin) hipHostFree(c->dl_pin); c->dl_dev = nullptr; c->dl_pin = nullptr; c->dl_cap = 0;
    HIP_TRY(c, hipMalloc(&c->dl_dev, words * 8)); HIP_TRY(c, hipHostMalloc(&c->dl_pin, words * 8, hipHostMallocDefault)); c->dl_cap = words; }
  auto gather = [&](const double* dev_d, const int* dev_i, int k, void* out) {
    if (!out) return; const size_t n = (size_t)nm * B * k, bytes = n * (dev_d ? 8 : 4);
    QmGatherArgs g; g.B = B; g.nmax = nm; g.k = k; g.src_d = dev_d; g.src_i = dev_i; g.dst_d = (double*)c->dl_dev; g.dst_i = (int*)c->dl_dev;
    c->bk.sync(); c->bk.launch(qm_gather_kernel, (int)((n + 255) / 256), 256, 0, g);
    c->bk.check(hipMemcpyAsync(c->dl_pin, c->dl_dev, bytes, hipMemcpyDeviceToHost, c->bk.stream), "D2H"); c->bk.check(hipStreamSynchronize(c->bk.stream), "sync");
    memcpy(out, c->dl_pin, bytes);
  };
  auto gather_d = [&](const double* dev, int k, double* out) { gather(dev, nullptr, k, out); };
  auto gather_i = [&](const int* dev, int32_t* out) { gather(nullptr, dev, 1, out); };
  gather_d(d.node_t, 1, ot); gather_i(d.node_ev, oev); gather_i(d.node_mode, omode); gather_d(d.xs, 30, ox); gather_d(d.us, 30, ou);
  if (operf) c->bk.to_host(operf, d.out_perf, (size_t)B * 10 * 8);
  return c->hipstate();
}
int qmhip_mpc_step(qmhip_ctx* c, int B, const double* t0, const double* x0, int n_ref, const double* ref_t, const double* ref_x, int n_ev, const double* ev, const int32_t* modes, double horizon,
                   int32_t* nn, double* ot, int32_t* oev, int32_t* omode, double* ox, double* ou, double* operf, int32_t* status) { QM_GUARD(c);
  int rc = qmhip_mpc_upload(c, B, t0, x0, n_ref, ref_t, ref_x, n_ev, ev, modes); if (rc) return rc;
  rc = qmhip_mpc_solve_resident(c, B, horizon); if (rc) return rc;
  return qmhip_mpc_download(c, B, nn, ot, oev, omode, ox, ou, operf, status);
}

int qmhip_policy_eval(qmhip_ctx* c, int B, const double* t, double* xd, double* ud, int32_t* mode) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !t) return QMHIP_ERR_ARG;
  if (!c->have_solution) { c->fail("qmhip_policy_eval: no policy received yet"); return QMHIP_ERR_STATE; }
  if (B != c->mpc.solved_B) { c->fail("qmhip_policy_eval: B differs from the batch size of the last solve"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->wbc.policy_eval(c->mpc.d, B, t);
  if (xd) c->bk.to_host(xd, c->wbc.w.x_des, (size_t)B * 30 * 8); if (ud) c->bk.to_host(ud, c->wbc.w.u_des, (size_t)B * 30 * 8); if (mode) c->bk.to_host(mode, c->wbc.w.mode, (size_t)B * 4);
  return c->hipstate();
}
// the feedback entry points read the stage records of the last SQP iteration: they exist for the multiple-shooting solver slots only, from the end of a solve until the
// next one starts (K1b rewrites the records), and not while a streamed step is in flight (its solve may be rewriting them)
static int feedback_ready(qmhip_ctx* c, int B, const char* fn) {
  if (c->mpc.solver != 0 && c->mpc.solver != 2) { c->fail(std::string(fn) + ": the feedback policy exists for the multiple-shooting solver slots only (ST_SOLVER 0 / 2), not for the discrete iLQR (1) or the interior-point method (3)"); return QMHIP_ERR_ARG; }
  if (c->io.in_flight > 0) { c->fail(std::string(fn) + ": a qmhip_step_submit is in flight (qmhip_step_collect it first: its solve rewrites the stage records the gains are read from)"); return QMHIP_ERR_STATE; }
  if (c->tick.in_flight > 0) { c->fail(std::string(fn) + ": a qmhip_tick_submit is in flight (qmhip_tick_collect it first)"); return QMHIP_ERR_STATE; }
  if (!c->have_solution) { c->fail(std::string(fn) + ": no policy received yet (no solve on this context since its creation, the last upload, reset or solver switch)"); return QMHIP_ERR_STATE; }
  if (B != c->mpc.solved_B) { c->fail(std::string(fn) + ": B differs from the batch size of the last solve"); return QMHIP_ERR_STATE; }
  return QMHIP_OK;
}
int qmhip_policy_eval_feedback(qmhip_ctx* c, int B, const double* t, const double* x, double* xd, double* ud, int32_t* mode) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !t) { if (c) c->fail("qmhip_policy_eval_feedback: bad argument"); return QMHIP_ERR_ARG; }
  if (!x) return qmhip_policy_eval(c, B, t, xd, ud, mode);
  const int rc = feedback_ready(c, B, "qmhip_policy_eval_feedback"); if (rc != QMHIP_OK) return rc;
  hipSetDevice(c->device); c->wbc.policy_eval_feedback(c->mpc.d, B, t, x);
  if (xd) c->bk.to_host(xd, c->wbc.w.x_des, (size_t)B * 30 * 8); if (ud) c->bk.to_host(ud, c->wbc.w.u_des, (size_t)B * 30 * 8); if (mode) c->bk.to_host(mode, c->wbc.w.mode, (size_t)B * 4);
  return c->hipstate();
}
int qmhip_mpc_download_feedback(qmhip_ctx* c, int B, double* gain, double* uff) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_mpc_download_feedback: bad argument"); return QMHIP_ERR_ARG; }
  const int rc = feedback_ready(c, B, "qmhip_mpc_download_feedback"); if (rc != QMHIP_OK) return rc;
  if (!gain && !uff) return QMHIP_OK;
  hipSetDevice(c->device); const int nm = c->max_nodes;
  // assembled on the device for a slice of the batch at a time (<= 64 MB of staging: one instance-node pair is 930 doubles), each slice one contiguous copy per array
  const size_t per = (size_t)nm * 930 * 8; int nb = (int)((64u << 20) / per); nb = nb < 1 ? 1 : (nb > B ? B : nb);
  double* stg = nullptr; HIP_TRY(c, hipMalloc((void**)&stg, (size_t)nb * per)); double* stg_u = stg + (size_t)nb * nm * 900;
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int k = (B - b0 < nb) ? B - b0 : nb;
    c->bk.sync(); c->wbc.feedback_gather(c->mpc.d, B, b0, k, stg, stg_u);
    if (gain) c->bk.to_host(gain + (size_t)b0 * nm * 900, stg, (size_t)k * nm * 900 * 8);
    if (uff) c->bk.to_host(uff + (size_t)b0 * nm * 30, stg_u, (size_t)k * nm * 30 * 8);
  }
  c->bk.sync(); hipFree(stg);
  return c->hipstate();
}

// ---- published feedback policy (include/qmhip.h): a double-buffered snapshot of the last solve — primal solution, grid, schedule and the first W nodes' gain records —
// that stays valid while the next solve rewrites the stage records; evaluated on a stream of its own under the publication mutex, never the context lock ----
static size_t pe_bytes(int B) { return (size_t)B * ((1 + 30 + 30 + 30) * 8 + 2 * 4); }      // [t | x | x_des | u_des | mode | covered]
int qmhip_policy_set_publish_window(qmhip_ctx* c, int nodes) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (nodes != 0 && (nodes < 2 || nodes > c->max_nodes)) { c->fail("qmhip_policy_set_publish_window: the window is 0 (off) or 2 ... max_nodes nodes"); return QMHIP_ERR_ARG; }
  std::lock_guard<std::mutex> ev(c->eval_mu);      // no evaluation is under way, and none starts, while the slots are replaced
  hipSetDevice(c->device); c->bk.sync(); if (c->stream_p) c->bk.check(hipStreamSynchronize(c->stream_p), "sync");
  c->bk.cur = c->bk.stream; c->pub.set_window(c->mpc.d, nodes);
  if (nodes && !c->stream_p) {
    HIP_TRY(c, hipStreamCreate(&c->stream_p)); HIP_TRY(c, hipHostMalloc((void**)&c->pe_pin, pe_bytes(c->max_batch), hipHostMallocDefault)); HIP_TRY(c, hipMalloc((void**)&c->pe_dev, pe_bytes(c->max_batch)));
  }
  c->bk.sync(); return c->hipstate();
}
int qmhip_policy_publish(qmhip_ctx* c, int B) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_policy_publish: bad argument"); return QMHIP_ERR_ARG; }
  if (c->pub.W == 0) { c->fail("qmhip_policy_publish: no publish window (qmhip_policy_set_publish_window has not been called, or with 0)"); return QMHIP_ERR_STATE; }
  const bool gains = c->st[ST_FEEDBACK_POLICY] != 0.0;
  if (gains && c->mpc.solver != 0 && c->mpc.solver != 2) { c->fail("qmhip_policy_publish: ST_FEEDBACK_POLICY = 1 needs a multiple-shooting solver slot (ST_SOLVER 0 / 2): the discrete iLQR (1) and the interior-point method (3) hand out no feedback policy"); return QMHIP_ERR_ARG; }
  if (!c->have_solution || c->mpc.solved_B != B) { c->fail("qmhip_policy_publish: no policy received yet (no solve of this batch on this context since its creation, the last upload, reset or solver switch)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.cur = c->bk.stream;      // behind the solve (or the streamed step) that produced the solution, in front of the next one: the stream's order
  if (c->pub.publish(c->mpc.d, B, gains) < 0) { c->fail("qmhip_policy_publish: no publish window"); return QMHIP_ERR_STATE; }
  return c->hipstate();
}
int qmhip_policy_eval_published(qmhip_ctx* c, int B, const double* t, const double* x, double* xd, double* ud, int32_t* mode, int32_t* covered, int64_t* seq) {
  if (!c) return QMHIP_ERR_ARG;
  int rc = QMHIP_OK; std::string msg;
  if (c->wbc_only) { rc = QMHIP_ERR_STATE; msg = "qmhip_policy_eval_published: not available on a WBC-only context (qmhip_create_wbc_context)"; }
  else if (B <= 0 || B > c->max_batch || !t) { rc = QMHIP_ERR_ARG; msg = "qmhip_policy_eval_published: bad argument"; }
  else {
    std::lock_guard<std::mutex> ev(c->eval_mu);
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == QMHIP_OK) { rc = QMHIP_ERR_HIP; msg = std::string("qmhip_policy_eval_published: ") + what + ": " + hipGetErrorString(e); } };
    QmPubBook::Eval tk;
    if (!c->pub.book.begin_eval(tk)) { rc = QMHIP_ERR_STATE; msg = "qmhip_policy_eval_published: no policy published yet (qmhip_policy_set_publish_window, then qmhip_policy_publish after a solve)"; }
    else if (B != tk.B) { c->pub.book.end_eval(tk, false); rc = QMHIP_ERR_STATE; msg = "qmhip_policy_eval_published: B differs from the batch size of the publication"; }
    else if (x && !tk.gains) { c->pub.book.end_eval(tk, false); rc = QMHIP_ERR_STATE; msg = "qmhip_policy_eval_published: the active publication carries no gains (it was made with ST_FEEDBACK_POLICY = 0); pass x = NULL for its feed-forward policy"; }
    else {
      hip(hipSetDevice(c->device), "hipSetDevice");
      char* h = c->pe_pin; char* d = c->pe_dev; const size_t o_x = (size_t)B * 8, o_xd = o_x + (size_t)B * 240, o_ud = o_xd + (size_t)B * 240, o_mode = o_ud + (size_t)B * 240, o_cov = o_mode + (size_t)B * 4;
      memcpy(h, t, (size_t)B * 8); if (x) memcpy(h + o_x, x, (size_t)B * 240);
      const QmPubSlot& s = c->pub.slot[tk.slot]; hipStream_t sp = c->stream_p;
      hip(hipStreamWaitEvent(sp, (hipEvent_t)s.ev_pub, 0), "hipStreamWaitEvent");
      hip(hipMemcpyAsync(d, h, x ? o_xd : o_x, hipMemcpyHostToDevice, sp), "H2D");
      if (rc == QMHIP_OK) {
        const QmPolicyFbPubArgs a = c->pub.eval_args(tk.slot, B, (const double*)d, x ? (const double*)(d + o_x) : nullptr, (double*)(d + o_xd), (double*)(d + o_ud), (int*)(d + o_mode), (int*)(d + o_cov), nullptr);
        hipLaunchKernelGGL(qm_policy_fb_pub_kernel, dim3(B), dim3(64), 0, sp, a); hip(hipGetLastError(), "kernel launch");
      }
      hip(hipMemcpyAsync(h + o_xd, d + o_xd, pe_bytes(B) - o_xd, hipMemcpyDeviceToHost, sp), "D2H");
      hip(hipEventRecord((hipEvent_t)s.ev_eval, sp), "hipEventRecord");
      c->pub.book.end_eval(tk, true);      // enqueued: from here on a publication may go ahead (it is ordered behind this evaluation by the slot's event)
      hip(hipStreamSynchronize(sp), "sync");
      if (rc == QMHIP_OK) {
        if (xd) memcpy(xd, h + o_xd, (size_t)B * 240); if (ud) memcpy(ud, h + o_ud, (size_t)B * 240); if (mode) memcpy(mode, h + o_mode, (size_t)B * 4); if (covered) memcpy(covered, h + o_cov, (size_t)B * 4);
        if (seq) *seq = (int64_t)tk.seq;
      }
    }
  }
  if (rc != QMHIP_OK) { QM_GUARD(c); c->fail(msg); }      // (the context lock only for the error text, with nothing else held)
  return rc;
}
int qmhip_policy_published_info(qmhip_ctx* c, int64_t* seq, int32_t* window, int32_t* uncovered) { QM_GUARD(c);
  if (!c) return QMHIP_ERR_ARG;
  long sq = 0; int w = 0, B = 0; c->pub.book.info(&sq, &w, nullptr, &B);
  if (seq) *seq = (int64_t)sq; if (window) *window = w;
  if (uncovered && B > 0) { hipSetDevice(c->device); c->bk.to_host(uncovered, c->pub.uncovered, (size_t)B * 4); }
  return c->hipstate();
}
int qmhip_wbc_reset(qmhip_ctx* c) { QM_GUARD(c); if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device); c->bk.cur = c->bk.stream_b; c->wbc.reset(); c->bk.cur = c->bk.stream; return c->hipstate(); }   // ordered with the WBC launches
// The control-tick path (WbcBase::update on the ros_control thread, QMController.cpp:145-147).  Everything it enqueues goes to the WBC stream and the host waits for
// THAT stream only: inputs staged in pinned memory -> asynchronous copies -> qm_wbc_kernel -> asynchronous copy of [out | qp_status] -> one stream synchronisation.
// On a context that also runs the MPC the WBC stream first waits (on the device, not the host) for what the MPC stream has enqueued so far, because the resident
// step shares the WBC's input buffers; on a WBC-only context (qmhip_create_wbc_context) there is nothing to wait for and a tick never sees the MPC.
int qmhip_wbc_step(qmhip_ctx* c, int B, const double* xd, const double* ud, const double* rbd, const int32_t* mode, double period, const double* time, int variant, double* out, int32_t* qps) { QM_GUARD(c);
  if (!c || B <= 0 || B > c->max_batch || !xd || !ud || !rbd || !mode || !time || !(period > 0)) { if (c) c->fail("qmhip_wbc_step: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); HipBackend& bk = c->bk; QmWbcBuffers& w = c->wbc.w; typedef QmWbcPipeline<HipBackend> WP;
  // host staging, sections in the device buffers' order: [x_des | u_des | rbd | time | mode]
  char* hin = c->tick_pin; char* hout = c->tick_pin + WP::in_bytes(c->max_batch);
  double* h_xd = (double*)hin; double* h_ud = h_xd + (size_t)B * 30; double* h_rbd = h_ud + (size_t)B * 30; double* h_time = h_rbd + (size_t)B * QM_NRBD; int* h_mode = (int*)(h_time + B);
  memcpy(h_xd, xd, (size_t)B * 30 * 8); memcpy(h_ud, ud, (size_t)B * 30 * 8); memcpy(h_rbd, rbd, (size_t)B * QM_NRBD * 8); memcpy(h_time, time, (size_t)B * 8); memcpy(h_mode, mode, (size_t)B * 4);
  hipStream_t sb = bk.stream_b;
  if (!c->wbc_only) { bk.check(hipEventRecord(bk.ev_in, bk.stream), "hipEventRecord"); bk.check(hipStreamWaitEvent(sb, bk.ev_in, 0), "hipStreamWaitEvent"); }
  if (B == w.Bmax) bk.check(hipMemcpyAsync(w.x_des, hin, WP::in_bytes(B), hipMemcpyHostToDevice, sb), "H2D");
  else {
    bk.check(hipMemcpyAsync(w.x_des, h_xd, (size_t)B * 30 * 8, hipMemcpyHostToDevice, sb), "H2D"); bk.check(hipMemcpyAsync(w.u_des, h_ud, (size_t)B * 30 * 8, hipMemcpyHostToDevice, sb), "H2D");
    bk.check(hipMemcpyAsync(w.rbd, h_rbd, (size_t)B * QM_NRBD * 8, hipMemcpyHostToDevice, sb), "H2D"); bk.check(hipMemcpyAsync(w.time, h_time, (size_t)B * 8, hipMemcpyHostToDevice, sb), "H2D");
    bk.check(hipMemcpyAsync(w.mode, h_mode, (size_t)B * 4, hipMemcpyHostToDevice, sb), "H2D");
  }
  bk.cur = sb; c->wbc.step(c->mpc.d, B, period, variant); bk.wbc_end();
  double* h_out = (double*)hout; int* h_qps = (int*)(h_out + (size_t)B * QM_NWBC_OUT);
  if (B == w.Bmax) bk.check(hipMemcpyAsync(hout, w.out, WP::out_bytes(B), hipMemcpyDeviceToHost, sb), "D2H");
  else { bk.check(hipMemcpyAsync(h_out, w.out, (size_t)B * QM_NWBC_OUT * 8, hipMemcpyDeviceToHost, sb), "D2H"); bk.check(hipMemcpyAsync(h_qps, w.qp_status, (size_t)B * 3 * 4, hipMemcpyDeviceToHost, sb), "D2H"); }
  bk.check(hipStreamSynchronize(sb), "sync");
  if (out) memcpy(out, h_out, (size_t)B * QM_NWBC_OUT * 8); if (qps) memcpy(qps, h_qps, (size_t)B * 3 * 4);
  return c->hipstate();
}
// qm::HoQp on arbitrary task hierarchies (HoQp.h:17-36): B independent cascades of the same shape, solved by the general kernel (k_hoqp.h)
int qmhip_hoqp_solve(qmhip_ctx* c, int B, int n_levels, int n, const int32_t* ma, const int32_t* md, const double* A, const double* b, const double* D, const double* f, double* x, int32_t* status) { QM_GUARD(c);
  if (!c || B <= 0 || !ma || !md || !x || !status || !QmHoqpPipeline<HipBackend>::shapes_ok(n_levels, n, ma, md)) {
    if (c) c->fail("qmhip_hoqp_solve: bad argument (1 <= n <= 36 variables, <= 8 levels, <= 36 equality and <= 64 inequality rows per level, <= 128 inequality rows in total)"); return QMHIP_ERR_ARG; }
  int sa = 0, sd = 0; for (int k = 0; k < n_levels; ++k) { sa += ma[k]; sd += md[k]; }
  if ((sa && (!A || !b)) || (sd && (!D || !f))) { c->fail("qmhip_hoqp_solve: null task array"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->hoqp.solve(B, n_levels, n, ma, md, A, b, D, f, x, status); return c->hipstate();
}
int qmhip_wbc_download(qmhip_ctx* c, int B, double* out, int32_t* qps) { QM_GUARD(c);
  if (!c || B <= 0 || B > c->max_batch) return QMHIP_ERR_ARG; hipSetDevice(c->device);
  if (out) c->bk.to_host(out, c->wbc.w.out, (size_t)B * QM_NWBC_OUT * 8); if (qps) c->bk.to_host(qps, c->wbc.w.qp_status, (size_t)B * 3 * 4);
  return c->hipstate();
}
int qmhip_control_step_resident(qmhip_ctx* c, int B, double horizon, double period, double time) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !(horizon > 0)) { if (c) c->fail("qmhip_control_step_resident: bad argument"); return QMHIP_ERR_ARG; }
  // the WBC goes to its own stream: back-to-back steps overlap WBC(k) — one wave per SIMD whose run time is that of the instance with the most
  // active-set iterations — with the MPC kernels of step k + 1, which fill the SIMDs the finished WBC waves leave behind
  hipSetDevice(c->device); c->control_step(B, horizon, period, time, false);
  return c->hipstate();
}

// ---- streamed control-step I/O (include/qmhip.h): observation in, packed record out, two steps in flight ----
// submit enqueues and returns: pinned staging -> asynchronous copies -> the control step as qmhip_closed_loop_resident runs it -> qm_step_pack_kernel (k_io.h) in order on
// the stream(s) that produce what it reads -> ONE copy of the slot into its pinned mirror on the copy stream -> the slot's event.  collect waits for the oldest slot's
// event only: the MPC and the WBC stream are never synchronised, so a step submitted meanwhile keeps running.
int qmhip_step_submit(qmhip_ctx* c, int B, const double* t0, const double* x0, const double* rbd_meas, double horizon, double period, double time, unsigned flags) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (B <= 0 || B > c->max_batch || B != c->lastB || !t0 || !x0 || !(horizon > 0) || !(period > 0) || (flags & ~(unsigned)(QMHIP_STEP_WBC | QMHIP_STEP_TRAJ))) {
    c->fail("qmhip_step_submit: bad argument (B == batch of the last qmhip_mpc_upload, t0 / x0 not null, horizon > 0, period > 0, flags of QMHIP_STEP_*)"); return QMHIP_ERR_ARG; }
  if (c->io.in_flight >= 2) { c->fail("qmhip_step_submit: two steps are in flight already (qmhip_step_collect the oldest first)"); return QMHIP_ERR_STATE; }
  if (c->tick.in_flight > 0) { c->fail("qmhip_step_submit: a qmhip_tick_submit is in flight (qmhip_tick_collect it first)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); HipBackend& bk = c->bk; const bool wbc = (flags & QMHIP_STEP_WBC) != 0, traj = (flags & QMHIP_STEP_TRAJ) != 0;
  if (!c->io.Bmax) { HIP_TRY(c, hipStreamCreate(&bk.stream_c)); HIP_TRY(c, hipEventCreateWithFlags(&c->ev_meas, hipEventDisableTiming)); c->io.allocate(c->max_batch); }      // first use: a context that never streams has the two streams it always had
  QmIoSlot& s = c->io.next(); bk.cur = bk.stream;
  if (c->meas_pending) { bk.check(hipStreamWaitEvent(bk.stream, c->ev_meas, 0), "hipStreamWaitEvent"); c->meas_pending = false; }
  c->io.upload(s, c->mpc.d, c->wbc.w, B, t0, x0, wbc ? rbd_meas : nullptr, time);
  if (c->front_B == B) c->gait_schedule(B, horizon);      // device-resident GaitSchedule active: modifyReferences before every MPC call, as qmhip_closed_loop_resident does
  if (wbc) c->control_step(B, horizon, period, time, true, true, rbd_meas != nullptr); else c->mpc_step(B, horizon, true);      // warm when a solution of this batch exists (QmMpcPipeline::grid)
  const int ncap = c->mpc.ncap > 0 && c->mpc.ncap <= c->max_nodes ? c->mpc.ncap : c->max_nodes;
  c->io.reserve(s, QmIoPipeline<HipBackend>::slot_bytes(B, ncap, traj));
  const bool strict = c->st[ST_RICCATI_STRICT] != 0.0;
  c->io.pack(c->mpc.d, c->wbc.w, B, ncap, QM_PACK_MPC | (traj ? QM_PACK_TRAJ : 0) | (wbc ? 0 : QM_PACK_NOWBC), strict, s.dev);      // MPC stream: behind the batch's apply, in front of the next K0
  if (wbc) { bk.cur = bk.stream_b; c->io.pack(c->mpc.d, c->wbc.w, B, ncap, QM_PACK_WBC, strict, s.dev); bk.cur = bk.stream; }      // WBC stream: behind this step's WBC, in front of the next
  c->io.download(s, B, ncap, flags, traj, wbc);
  return c->hipstate();
}
int qmhip_step_collect(qmhip_ctx* c, int B, qmhip_step_record* rec, double* ot, int32_t* oev, int32_t* omode, double* ox, double* ou) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (c->io.in_flight == 0) { c->fail("qmhip_step_collect: no step in flight"); return QMHIP_ERR_STATE; }
  const QmIoSlot& s = c->io.front();
  if (B != s.B || !rec) { c->fail("qmhip_step_collect: bad argument (B == batch of the oldest step in flight, rec not null)"); return QMHIP_ERR_ARG; }
  if ((ot || oev || omode || ox || ou) && !(s.flags & QMHIP_STEP_TRAJ)) { c->fail("qmhip_step_collect: trajectory outputs requested, but the step was submitted without QMHIP_STEP_TRAJ"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->io.collect(rec, c->max_nodes, ot, oev, omode, ox, ou);
  return c->hipstate();
}
int qmhip_step_in_flight(const qmhip_ctx* c) { QM_GUARD(c); return c ? c->io.in_flight : 0; }


// ---- planned task-space trajectories (k_plan.h, qm_plan_pipeline.h): the arithmetic of qm::QmVisualizer, qm_interface/src/visualization/qm_visualization.cpp ----
static int plan_ready(qmhip_ctx* c, int B, const char* fn) {
  if (!c->have_solution) { c->fail(std::string(fn) + ": no solution available (no solve on this context since its creation, the last upload, reset or solver switch)"); return QMHIP_ERR_STATE; }
  if (B != c->mpc.solved_B) { c->fail(std::string(fn) + ": B differs from the batch size of the last solve (the solver buffers are strided by it)"); return QMHIP_ERR_STATE; }
  return QMHIP_OK;
}
// publishOptimizedStateTrajectory, qm_visualization.cpp:90-189
int qmhip_plan_task_space(qmhip_ctx* c, int B, qmhip_plan_record* rec, int32_t* nn) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !rec) { if (c) c->fail("qmhip_plan_task_space: bad argument"); return QMHIP_ERR_ARG; }
  const int rc = plan_ready(c, B, "qmhip_plan_task_space"); if (rc != QMHIP_OK) return rc;
  hipSetDevice(c->device); c->plan.task_space(c->mpc.d, B, rec, nn); return c->hipstate();
}
// its "Future footholds", qm_visualization.cpp:150-182
int qmhip_plan_footholds(qmhip_ctx* c, int B, int cap, qmhip_foothold* out, int32_t* count) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || cap < 0 || (cap > 0 && !out) || !count) { if (c) c->fail("qmhip_plan_footholds: bad argument"); return QMHIP_ERR_ARG; }
  const int rc = plan_ready(c, B, "qmhip_plan_footholds"); if (rc != QMHIP_OK) return rc;
  hipSetDevice(c->device); c->plan.footholds(c->mpc.d, B, cap, out, count); return c->hipstate();
}
// publishDesiredTrajectory, qm_visualization.cpp:194-251 (the target knots) and publishObservation, qm_visualization.cpp:267-283 (the observation)
int qmhip_task_space_eval(qmhip_ctx* c, int R, const double* x, const double* u, const int32_t* mode, const double* ee_ref, qmhip_plan_record* rec) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || R <= 0 || (long long)R > (long long)c->max_batch * c->max_nodes || !x || !mode || !rec) { if (c) c->fail("qmhip_task_space_eval: bad argument (1 <= R <= max_batch * max_nodes; x, mode and rec required)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->plan.eval(c->mpc.d.mb, R, x, u, mode, ee_ref, rec); return c->hipstate();
}

// ---- policy rollout (k_rollout.h, qm_rollout_pipeline.h): MPC_MRT_Interface::rolloutPolicy [upstream, recalled], batched; the rollout QMController.cpp:311 initialises ----
static_assert(sizeof(QmRolloutParams) == sizeof(qmhip_rollout_params) && offsetof(QmRolloutParams, trace_cap) == offsetof(qmhip_rollout_params, trace_cap), "qm_rollout_pipeline.h restates the parameter struct of qmhip.h");
// source 0: the last solve's stage records, under the context lock on the MPC stream — the validity window of qmhip_policy_eval_feedback
static int rollout_solve(qmhip_ctx* c, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* prm, double* x_end, double* u_end, int32_t* mode_end,
                         struct qmhip_rollout_summary* summary, qmhip_rollout_sample* trace, int32_t* count) { QM_GUARD(c);
  QmRolloutSource src; src.solver = c->mpc.solver; src.in_flight = c->io.in_flight > 0 || c->tick.in_flight > 0; src.have_solution = c->have_solution; src.B = c->mpc.solved_B;
  const char* msg = nullptr; const int adm = qm_rollout_admit(src, R, inst, t0, x0, t_end, prm, x_end, u_end, mode_end, trace, &msg);
  if (adm != QM_RO_OK) { c->fail(std::string("qmhip_policy_rollout: ") + msg); return adm; }
  hipSetDevice(c->device); const QmMpcBuffers& d = c->mpc.d;
  QmPolicyArgs p; p.mb = d.mb; p.B = src.B; p.nmax = d.nmax; p.nev = d.nev; p.n_nodes = d.n_nodes; p.node_t = d.node_t; p.node_ev = d.node_ev; p.xs = d.xs; p.us = d.us; p.ev = d.ev; p.modes = d.modes;
  c->rollout.enqueue(d.mb, d.st, p, d.stage, d.nmax, false, R, inst, t0, x0, t_end, *prm); c->rollout.wait();
  const int rc = c->hipstate(); if (rc != QMHIP_OK) return rc;
  c->rollout.hand_over(x_end, u_end, mode_end, summary, trace, count); return QMHIP_OK;
}
// source 1: the active publication, exactly the path of qmhip_policy_eval_published — the publication mutex, its stream, the slot's two events, *seq
static int rollout_published(qmhip_ctx* c, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const QmRolloutParams* prm, double* x_end, double* u_end, int32_t* mode_end,
                             struct qmhip_rollout_summary* summary, qmhip_rollout_sample* trace, int32_t* count, int64_t* seq) {
  int rc = QMHIP_OK; std::string msg; const std::string fn = "qmhip_policy_rollout: ";
  {
    std::lock_guard<std::mutex> ev(c->eval_mu);
    QmPubBook::Eval tk; QmRolloutSource src; src.published = c->pub.book.begin_eval(tk); src.gains = tk.gains; src.B = tk.B;
    const char* why = nullptr; rc = qm_rollout_admit(src, R, inst, t0, x0, t_end, prm, x_end, u_end, mode_end, trace, &why);
    if (rc != QM_RO_OK) { if (src.published) c->pub.book.end_eval(tk, false); msg = fn + why; }
    else {
      RolloutQueuePub& q = c->ro_qp; q.error.clear(); q.check(hipSetDevice(c->device), "hipSetDevice");
      const QmPubSlot& s = c->pub.slot[tk.slot];
      q.check(hipStreamWaitEvent(c->stream_p, (hipEvent_t)s.ev_pub, 0), "hipStreamWaitEvent");
      const QmPolicyFbPubArgs pa = c->pub.eval_args(tk.slot, tk.B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
      c->rollout_p.enqueue(c->mpc.d.mb, c->mpc.d.st, pa.p, s.gains, c->pub.W, true, R, inst, t0, x0, t_end, *prm);
      q.check(hipEventRecord((hipEvent_t)s.ev_eval, c->stream_p), "hipEventRecord");
      c->pub.book.end_eval(tk, true);      // enqueued: from here on a publication may go ahead (it is ordered behind this rollout by the slot's event)
      c->rollout_p.wait();
      if (!q.error.empty()) { rc = QMHIP_ERR_HIP; msg = fn + q.error; }
      else { c->rollout_p.hand_over(x_end, u_end, mode_end, summary, trace, count); if (seq) *seq = (int64_t)tk.seq; }
    }
  }
  if (rc != QMHIP_OK) { QM_GUARD(c); c->fail(msg); }      // (the context lock only for the error text, with nothing else held)
  return rc;
}
int qmhip_policy_rollout(qmhip_ctx* c, int R, const int32_t* inst, const double* t0, const double* x0, const double* t_end, const qmhip_rollout_params* p, double* x_end, double* u_end, int32_t* mode_end,
                         struct qmhip_rollout_summary* summary, qmhip_rollout_sample* trace, int32_t* count, int64_t* seq) {
  if (!c) return QMHIP_ERR_ARG;
  if (c->wbc_only) { QM_GUARD(c); c->fail("qmhip_policy_rollout: not available on a WBC-only context (qmhip_create_wbc_context)"); return QMHIP_ERR_STATE; }
  QmRolloutParams copy; if (p) { copy.max_step = p->max_step; copy.max_steps = p->max_steps; copy.source = p->source; copy.feedback = p->feedback; copy.trace_cap = p->trace_cap; }
  const QmRolloutParams* prm = p ? &copy : nullptr;
  if (p && p->source == 1) return rollout_published(c, R, inst, t0, x0, t_end, prm, x_end, u_end, mode_end, summary, trace, count, seq);
  return rollout_solve(c, R, inst, t0, x0, t_end, prm, x_end, u_end, mode_end, summary, trace, count);
}

// ---- streamed controller tick for a plant on the host (include/qmhip.h): measured rbd state in, hybrid joint command out ----
// tick_submit enqueues one QMController::update for the batch on the MPC stream — the stream qmhip_closed_loop_sim runs its ticks on, with the same launches
// (qm_tick_pipeline.h) — and returns; tick_collect waits for the one event behind the record's copy.
int qmhip_tick_reset(qmhip_ctx* c, int B, int controller, double arm_kp, double arm_kd, int mpc_every) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (B <= 0 || B > c->max_batch || (controller != 0 && controller != 1) || mpc_every < 1) { c->fail("qmhip_tick_reset: bad argument (0 < B <= max_batch, controller 0 / 1, mpc_every >= 1)"); return QMHIP_ERR_ARG; }
  if (c->tick.in_flight > 0 || c->io.in_flight > 0) { c->fail("qmhip_tick_reset: a tick or a step is in flight (collect it first)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.sync(); c->bk.cur = c->bk.stream; c->tick.allocate(c->max_batch);
  c->tick.reset(B, controller, arm_kp, arm_kd, mpc_every); c->wbc.reset();      // (on the MPC stream: the ticks' WBC launches run there)
  c->mpc.solved_B = 0; c->have_solution = false;      // a new episode starts cold, like qmhip_sim_reset
  return c->hipstate();
}
int qmhip_tick_submit(qmhip_ctx* c, int B, const double* time, const double* rbd_meas, const int32_t* contact, double horizon, double period) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (c->tick.B == 0) { c->fail("qmhip_tick_submit: qmhip_tick_reset has not been called"); return QMHIP_ERR_STATE; }
  if (B != c->tick.B || !time || !rbd_meas || !(horizon > 0) || !(period > 0)) { c->fail("qmhip_tick_submit: bad argument (B == batch of qmhip_tick_reset, time / rbd_meas not null, horizon > 0, period > 0)"); return QMHIP_ERR_ARG; }
  if (c->tick.in_flight > 0) { c->fail("qmhip_tick_submit: a tick is in flight already (qmhip_tick_collect it first)"); return QMHIP_ERR_STATE; }
  if (c->io.in_flight > 0) { c->fail("qmhip_tick_submit: a qmhip_step_submit is in flight (qmhip_step_collect it first)"); return QMHIP_ERR_STATE; }
  const bool feedback = c->st[ST_FEEDBACK_POLICY] != 0.0;
  if (feedback && c->mpc.solver != 0 && c->mpc.solver != 2) { c->fail("qmhip_tick_submit: ST_FEEDBACK_POLICY = 1 needs a multiple-shooting solver slot (ST_SOLVER 0 / 2): the discrete iLQR (1) and the interior-point method (3) hand out no feedback policy"); return QMHIP_ERR_ARG; }
  if (!c->tick.mpc_tick() && (!c->have_solution || c->mpc.solved_B != B)) { c->fail("qmhip_tick_submit: no policy of this batch to evaluate on a tick without an MPC call (dropped by an upload, reset or solver switch since the last MPC tick)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.cur = c->bk.stream; c->bk.wbc_inputs_next();      // behind a WBC another entry point left on the WBC stream: the tick rewrites its inputs
  const bool ran = c->tick.mpc_tick();
  c->tick.submit(c->mpc, c->wbc, time, rbd_meas, (const int*)contact, horizon, period, c->sqp_iterations(), [&]() { if (c->front_B == B) c->gait_schedule(B, horizon); }, feedback, c->st[ST_RICCATI_STRICT] != 0.0);
  if (ran) { c->lastB = B; c->have_solution = true; }
  return c->hipstate();
}
int qmhip_tick_collect(qmhip_ctx* c, int B, qmhip_tick_record* rec) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (c->tick.in_flight == 0) { c->fail("qmhip_tick_collect: no tick in flight"); return QMHIP_ERR_STATE; }
  if (B != c->tick.B || !rec) { c->fail("qmhip_tick_collect: bad argument (B == batch of the tick in flight, rec not null)"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->tick.collect(rec);
  return c->hipstate();
}
int qmhip_observe(qmhip_ctx* c, int B, const double* rbd, double* x) { QM_GUARD(c);
  if (!c || B <= 0 || B > c->max_batch || !rbd || !x) { if (c) c->fail("qmhip_observe: bad argument"); return QMHIP_ERR_ARG; }
  if (c->tick.in_flight > 0) { c->fail("qmhip_observe: a qmhip_tick_submit is in flight (it shares the tick's staging; qmhip_tick_collect it first)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.cur = c->bk.stream; c->tick.allocate(c->max_batch); c->tick.observe_host(c->mpc.d, B, rbd, x);
  return c->hipstate();
}

// ---- batched rigid-body plant (QMHWSim.cpp:60-116) ----
int qmhip_sim_set_params(qmhip_ctx* c, const double* p, int n) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || !p || n < 1 || n > 7) { if (c) c->fail("qmhip_sim_set_params: bad argument"); return QMHIP_ERR_ARG; }
  QmSimParams& q = c->sim.p; double* f[6] = {&q.k_n, &q.d_n, &q.mu, &q.v_eps, &q.foot_radius, &q.delay};
  for (int i = 0; i < n && i < 6; ++i) *f[i] = p[i]; if (n == 7) q.saturate = p[6] != 0.0;
  if (!(q.k_n >= 0) || !(q.d_n >= 0) || !(q.mu >= 0) || !(q.v_eps > 0) || !(q.delay >= 0)) { c->fail("qmhip_sim_set_params: negative parameter"); return QMHIP_ERR_ARG; }
  return QMHIP_OK;
}
int qmhip_sim_set_controller(qmhip_ctx* c, int controller) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || (controller != 0 && controller != 1)) { if (c) c->fail("qmhip_sim_set_controller: 0 (QMController) or 1 (QMMpcController)"); return QMHIP_ERR_ARG; }
  c->sim.controller = controller; return QMHIP_OK;
}
int qmhip_sim_reset(qmhip_ctx* c, int B, const double* q, const double* v, const double* time) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !q || !v || !time) { if (c) c->fail("qmhip_sim_reset: bad argument"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->sim.allocate(c->max_batch); c->sim.reset(B, q, v, time); c->sim_ticks = 0; c->pub.reset_counters();
  c->mpc.solved_B = 0; c->have_solution = false;      // a new episode starts cold, like the reference after "Simulation reset" (no warm start from the previous episode's trajectory)
  c->sim.step(c->mpc.d.mb, B, 0.0, 0);   // rbd / contact of the reset state
  if (c->episode.on) c->episode.start(B, c->sim.s.rbd, c->sim.s.contact);      // episode monitor: a new episode, anchored at the reset state's end-effector pose
  return c->hipstate();
}
int qmhip_sim_set_command(qmhip_ctx* c, int B, const double* pos_des, const double* vel_des, const double* kp, const double* kd, const double* ff) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !pos_des || !vel_des || !kp || !kd || !ff) { if (c) c->fail("qmhip_sim_set_command: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_set_command: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  std::vector<double> cmd((size_t)B * (QM_SIM_CMD - 1)); const double* src[5] = {pos_des, vel_des, kp, kd, ff};
  for (int b = 0; b < B; ++b) for (int k = 0; k < 5; ++k) for (int j = 0; j < 18; ++j) cmd[(size_t)b * (QM_SIM_CMD - 1) + 18 * k + j] = src[k][(size_t)b * 18 + j];
  hipSetDevice(c->device); c->sim.set_command(B, cmd.data()); return c->hipstate();
}
int qmhip_sim_step(qmhip_ctx* c, int B, double period, int n_substeps, double* rbd, int32_t* contact) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || !(period > 0) || n_substeps < 1) { if (c) c->fail("qmhip_sim_step: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_step: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->sim.step(c->mpc.d.mb, B, period, n_substeps);
  if (rbd) c->bk.to_host(rbd, c->sim.s.rbd, (size_t)B * QM_NRBD * 8); if (contact) c->bk.to_host(contact, c->sim.s.contact, (size_t)B * 4 * 4);
  return c->hipstate();
}
int qmhip_sim_get_state(qmhip_ctx* c, int B, double* q, double* v, double* time, double* force, int32_t* status) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_sim_get_state: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_get_state: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device);
  if (q) c->bk.to_host(q, c->sim.s.q, (size_t)B * 24 * 8); if (v) c->bk.to_host(v, c->sim.s.v, (size_t)B * 24 * 8); if (time) c->bk.to_host(time, c->sim.s.time, (size_t)B * 8);
  if (force) c->bk.to_host(force, c->sim.s.force, (size_t)B * 12 * 8); if (status) c->bk.to_host(status, c->sim.s.status, (size_t)B * 4);
  return c->hipstate();
}
// the estimator-layout state / contact flags of the plant's CURRENT state (what the last qmhip_sim_step or qmhip_sim_reset left), without stepping
int qmhip_sim_get_rbd(qmhip_ctx* c, int B, double* rbd, int32_t* contact) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_sim_get_rbd: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_get_rbd: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device);
  if (rbd) c->bk.to_host(rbd, c->sim.s.rbd, (size_t)B * QM_NRBD * 8); if (contact) c->bk.to_host(contact, c->sim.s.contact, (size_t)B * 4 * 4);
  return c->hipstate();
}
// plant disturbances (qmhip.h): the schedule of external wrenches the next steps of the plant apply, and what the last sub-step applied
int qmhip_sim_set_pushes(qmhip_ctx* c, int B, int K, const qmhip_push* p) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  const bool off = K == 0 || !p;
  if (K < 0 || K > QM_SIM_MAX_PUSH || (!off && (B <= 0 || B > c->max_batch))) { c->fail("qmhip_sim_set_pushes: bad argument (1 <= B <= max_batch, 0 <= K <= QM_SIM_MAX_PUSH)"); return QMHIP_ERR_ARG; }
  if (!off && !qm_pushes_valid(B, K, (const double*)p)) { c->fail("qmhip_sim_set_pushes: a NaN time or a non-finite force / torque component"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->sim.allocate(c->max_batch); c->sim.set_pushes(B, off ? 0 : K, (const double*)p); return c->hipstate();
}
int qmhip_sim_get_push(qmhip_ctx* c, int B, double* wrench, int32_t* mask) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_sim_get_push: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_get_push: neither qmhip_sim_reset nor qmhip_sim_set_pushes has been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device);
  if (wrench) c->bk.to_host(wrench, c->sim.s.push_out, (size_t)B * 9 * 8); if (mask) c->bk.to_host(mask, c->sim.s.push_mask, (size_t)B * 4);
  return c->hipstate();
}
// plant terrain (qmhip.h): the per-robot ground grids the next steps of the plant stand on, the ground records of the last sub-step, the lookup itself
int qmhip_sim_set_terrain(qmhip_ctx* c, int B, int nx, int ny, const qmhip_terrain* hdr, const double* height, const double* mu) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (hdr && (B <= 0 || B > c->max_batch)) { c->fail("qmhip_sim_set_terrain: bad argument (1 <= B <= max_batch)"); return QMHIP_ERR_ARG; }
  if (hdr && !qm_terrain_valid(B, nx, ny, hdr, height, mu)) { c->fail("qmhip_sim_set_terrain: nx / ny outside [2, QM_TERRAIN_MAX], a non-finite header entry, dx / dy <= 0, a non-finite height or a negative / non-finite mu"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->sim.allocate(c->max_batch); c->sim.set_terrain(B, nx, ny, hdr, height, mu); return c->hipstate();
}
int qmhip_sim_get_ground(qmhip_ctx* c, int B, double* ground) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_sim_get_ground: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_get_ground: neither qmhip_sim_reset nor qmhip_sim_set_terrain has been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device);
  if (ground) c->bk.to_host(ground, c->sim.s.ground, (size_t)B * 24 * 8);
  return c->hipstate();
}
int qmhip_terrain_eval(qmhip_ctx* c, int B, int n, const double* xy, double* out) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || n <= 0 || !xy || !out) { if (c) c->fail("qmhip_terrain_eval: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.ter_on) { c->fail("qmhip_terrain_eval: no terrain is set (qmhip_sim_set_terrain)"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device); c->bk.cur = c->bk.stream; c->sim.terrain_eval(B, n, xy, out); return c->hipstate();
}
// sensor model (qmhip.h): the records of the measurement model between the plant and the controller, and what the controller is told
int qmhip_sim_set_sensors(qmhip_ctx* c, int B, const qmhip_sensor* s) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  if (s && (B <= 0 || B > c->max_batch)) { c->fail("qmhip_sim_set_sensors: bad argument (1 <= B <= max_batch)"); return QMHIP_ERR_ARG; }
  if (s && !qm_sensors_valid(B, s)) { c->fail("qmhip_sim_set_sensors: a lag outside [0, QM_SENSE_MAX_LAG] or a negative / non-finite sigma / bias_sigma"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->sim.allocate(c->max_batch); c->sim.set_sensors(c->mpc.d.mb, B, s); return c->hipstate();
}
int qmhip_sim_get_measured(qmhip_ctx* c, int B, double* rbd, int32_t* samples) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch) { if (c) c->fail("qmhip_sim_get_measured: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_sim_get_measured: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  hipSetDevice(c->device);
  if (rbd) c->bk.to_host(rbd, c->sim.meas_rbd(), (size_t)B * QM_NRBD * 8);
  if (samples) { if (c->sim.s.sense_on) c->bk.to_host(samples, c->sim.s.sense_n, (size_t)B * 4); else for (int b = 0; b < B; ++b) samples[b] = 0; }
  return c->hipstate();
}

// device-resident control loop around the plant: per tick [state estimate (ground truth) -> MPC call every mpc_every ticks (warm-started SQP on the observation)
// -> policy at the plant time -> WBC on the measured state -> hybrid joint command -> one simulation step]; QMController::update + mpcThread_
// (qm_controllers/src/QMController.cpp:128-175, 315-332), the MPC synchronous with the tick it is triggered on
int qmhip_closed_loop_sim(qmhip_ctx* c, int B, int n_ticks, double period, int n_substeps, int mpc_every, double horizon, double arm_kp, double arm_kd) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || n_ticks <= 0 || !(period > 0) || n_substeps < 1 || mpc_every < 1 || !(horizon > 0)) { if (c) c->fail("qmhip_closed_loop_sim: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_closed_loop_sim: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  const bool feedback = c->st[ST_FEEDBACK_POLICY] != 0.0;      // sqp.useFeedbackPolicy: the ticks evaluate the SQP's linear controller at the estimated state
  if (feedback && c->mpc.solver != 0 && c->mpc.solver != 2) { c->fail("qmhip_closed_loop_sim: ST_FEEDBACK_POLICY = 1 needs a multiple-shooting solver slot (ST_SOLVER 0 / 2): the discrete iLQR (1) and the interior-point method (3) hand out no feedback policy"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->bk.sync(); c->episode.strict = c->st[ST_RICCATI_STRICT] != 0.0 ? 1 : 0;
  qm_closed_loop_sim_ticks(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, n_substeps, mpc_every, horizon, arm_kp, arm_kd, c->sqp_iterations(),
                           [&]() { if (c->front_B == B) c->gait_schedule(B, horizon); }, feedback, c->episode.on ? &c->episode : (QmEpisodePipeline<HipBackend>*)nullptr);
  c->lastB = B; c->have_solution = true;
  return c->hipstate();
}

int qmhip_closed_loop_sim_pipelined(qmhip_ctx* c, int B, int n_ticks, double period, int n_substeps, int mpc_every, double horizon, double arm_kp, double arm_kd) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c || B <= 0 || B > c->max_batch || n_ticks <= 0 || !(period > 0) || n_substeps < 1 || mpc_every < 1 || !(horizon > 0)) { if (c) c->fail("qmhip_closed_loop_sim_pipelined: bad argument"); return QMHIP_ERR_ARG; }
  if (!c->sim.s.Bmax) { c->fail("qmhip_closed_loop_sim_pipelined: qmhip_sim_reset has not been called"); return QMHIP_ERR_STATE; }
  // the pipelined ticks evaluate a PUBLISHED COPY of the policy while the next solve rewrites the stage records the gains live in; the copy holds the primal solution only
  // without a publish window (qmhip_policy_set_publish_window) that copy holds the primal solution only
  const bool feedback = c->st[ST_FEEDBACK_POLICY] != 0.0;
  if (feedback && c->pub.W == 0) { c->fail("qmhip_closed_loop_sim_pipelined: ST_FEEDBACK_POLICY = 1 is not supported by the pipelined loop without a publish window (the published policy carries no gains); call qmhip_policy_set_publish_window, use qmhip_closed_loop_sim or set it to 0"); return QMHIP_ERR_ARG; }
  if (feedback && c->mpc.solver != 0 && c->mpc.solver != 2) { c->fail("qmhip_closed_loop_sim_pipelined: ST_FEEDBACK_POLICY = 1 needs a multiple-shooting solver slot (ST_SOLVER 0 / 2): the discrete iLQR (1) and the interior-point method (3) hand out no feedback policy"); return QMHIP_ERR_ARG; }
  if (n_ticks % mpc_every || c->sim_ticks % mpc_every) { c->fail("qmhip_closed_loop_sim_pipelined: n_ticks and the tick counter must be multiples of mpc_every"); return QMHIP_ERR_ARG; }
  hipSetDevice(c->device); c->bk.sync(); c->episode.strict = c->st[ST_RICCATI_STRICT] != 0.0 ? 1 : 0;
  qm_closed_loop_sim_pipelined(c->bk, c->mpc, c->wbc, c->sim, c->sim_ticks, B, n_ticks, period, n_substeps, mpc_every, horizon, arm_kp, arm_kd, c->sqp_iterations(),
                               [&]() { if (c->front_B == B) c->gait_schedule(B, horizon); }, feedback ? &c->pub : (QmPublishPipeline<HipBackend>*)nullptr,
                               c->episode.on ? &c->episode : (QmEpisodePipeline<HipBackend>*)nullptr);
  c->lastB = B; c->have_solution = true; c->bk.sync();
  return c->hipstate();
}

// ---- episode monitor (k_episode.h, qm_episode_pipeline.h): per-tick statistics and traces of the two loops above; the argument checks are the pipeline's ----
static int episode_rc(qmhip_ctx* c, int rc) { if (rc != QMHIP_OK) { c->fail(c->episode.why); return rc; } return c->hipstate(); }
int qmhip_episode_monitor(qmhip_ctx* c, const qmhip_episode_params* p) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG;
  hipSetDevice(c->device); c->bk.sync(); c->bk.cur = c->bk.stream; c->episode.strict = c->st[ST_RICCATI_STRICT] != 0.0 ? 1 : 0;
  return episode_rc(c, c->episode.monitor(c->max_batch, (const QmEpisodeParams*)p));
}
int qmhip_episode_set_anchor(qmhip_ctx* c, int B, const double* ee_pose) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device); return episode_rc(c, c->episode.set_anchor(B, ee_pose));
}
int qmhip_episode_summary(qmhip_ctx* c, int B, struct qmhip_episode_summary* out) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device); return episode_rc(c, c->episode.read_summary(B, out));
}
int qmhip_episode_trace(qmhip_ctx* c, int B, int cap, qmhip_episode_sample* out, int32_t* count) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device); return episode_rc(c, c->episode.read_trace(B, cap, out, count));
}
int qmhip_episode_fold(qmhip_ctx* c, int B, int tick, double period, const double* time, const double* rbd, const int32_t* contact, const double* force, const int32_t* mode, const double* wbc_out,
                       const int32_t* qp_status, const int32_t* sim_status, const int32_t* mpc_status) { QM_GUARD(c); QM_NEED_MPC(c);
  if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device);
  const int rc = c->episode.fold(c->mpc.d.mb, B, tick, period, time, rbd, (const int*)contact, force, (const int*)mode, wbc_out, (const int*)qp_status, (const int*)sim_status, (const int*)mpc_status);
  c->bk.cur = c->bk.stream; return episode_rc(c, rc);
}

int qmhip_set_profiling(qmhip_ctx* c, int en) { QM_GUARD(c); if (!c) return QMHIP_ERR_ARG; c->bk.resolve(); c->bk.profiling = (en == 2 || en == 3) ? en : (en != 0); return QMHIP_OK; }
int qmhip_get_kernel_ms(qmhip_ctx* c, const char* name, double* ms, int* launches) { QM_GUARD(c);
  if (!c || !name) return QMHIP_ERR_ARG; hipSetDevice(c->device); c->bk.resolve(); auto it = c->bk.acc.find(name);
  if (ms) *ms = it == c->bk.acc.end() ? 0.0 : it->second.first; if (launches) *launches = it == c->bk.acc.end() ? 0 : it->second.second; return QMHIP_OK;
}
int qmhip_reset_kernel_ms(qmhip_ctx* c) { QM_GUARD(c); if (!c) return QMHIP_ERR_ARG; c->bk.resolve(); c->bk.acc.clear(); return QMHIP_OK; }
int qmhip_synchronize(qmhip_ctx* c) { QM_GUARD(c); if (!c) return QMHIP_ERR_ARG; hipSetDevice(c->device); c->bk.sync(); return c->hipstate(); }
int qmhip_last_ls_trials(const qmhip_ctx* c) { QM_GUARD(c); if (!c) return -1; hipSetDevice(c->device); return const_cast<qmhip_ctx*>(c)->mpc.ls_trials(); }      // (after a device-side line search: one synchronising read of the trial counters)
int qmhip_debug_set(qmhip_ctx* c, const char* key, int value) { QM_GUARD(c); if (!c || !key) return QMHIP_ERR_ARG; if (!strcmp(key, "riccati_skip")) { c->mpc.riccati_skip = value; return QMHIP_OK; } if (!strcmp(key, "wbc_stop")) { c->wbc.wbc_stop = value; return QMHIP_OK; } if (!strcmp(key, "lq_prof")) { c->mpc.lq_prof = value; return QMHIP_OK; }
  if (!strcmp(key, "r_dense")) { c->mpc.r_force_dense = value != 0; return QMHIP_OK; }      // 1: the dense instances of the trial evaluation and of K1b's R0 (u − u_nom) although R is block diagonal (tests: same bits)
  if (!strcmp(key, "fused_policy")) { c->fused_policy = value != 0; return QMHIP_OK; }      // 0: apply -> qm_policy_kernel -> WBC as in rounds 1-5 (A/B, tests)
  if (!strcmp(key, "ls_device_tail")) { c->mpc.device_tail = value != 0; return QMHIP_OK; }      // 0: the host-driven line-search trial loop of rounds 1-5 (A/B, tests); 1 (default): the trials after the first in one launch (k_ls.h)
  if (!strncmp(key, "lds_pad:", 8)) {   // profiling only: "lds_pad:<kernel group>" (lq, lq_kin, riccati, ls_eval, wbc, ...) = extra dynamic LDS bytes per workgroup; 0 removes it
    if (value < 0 || value > 160 * 1024) return QMHIP_ERR_ARG; if (value) c->bk.lds_pad[key + 8] = value; else c->bk.lds_pad.erase(key + 8); return QMHIP_OK; }
  if (!strcmp(key, "lq_debug")) {      // parity tests: K1b additionally writes the UNPROJECTED LQ model of every interval (buffer "lqdbg", [B][max_nodes][LQ_DBG_SIZE]) and Pu / the zero rows of Px into the stage record
    QM_NEED_MPC(c); hipSetDevice(c->device); c->bk.sync();
    if (value && !c->mpc.d.lqdbg) c->mpc.d.lqdbg = c->mpc.A<double>((size_t)c->max_nodes * c->max_batch * LQ_DBG_SIZE);
    if (!value && c->mpc.d.lqdbg) { c->bk.free(c->mpc.d.lqdbg); c->mpc.d.lqdbg = nullptr; }
    c->bk.sync(); return c->hipstate();
  }
  return QMHIP_ERR_ARG; }
int qmhip_debug_get(const qmhip_ctx* c, const char* key, int* value) { QM_GUARD(c);
  if (!c || !key || !value) return QMHIP_ERR_ARG;
  if (!strcmp(key, "riccati_skip")) { *value = c->mpc.riccati_skip; return QMHIP_OK; } if (!strcmp(key, "wbc_stop")) { *value = c->wbc.wbc_stop; return QMHIP_OK; } if (!strcmp(key, "lq_prof")) { *value = c->mpc.lq_prof; return QMHIP_OK; }
  if (!strcmp(key, "lq_debug")) { *value = c->mpc.d.lqdbg ? 1 : 0; return QMHIP_OK; }
  if (!strcmp(key, "lds_pad")) { *value = (int)c->bk.lds_pad.size(); return QMHIP_OK; }      // number of kernel groups running with padded LDS
  if (!strcmp(key, "ls_device_tail")) { *value = c->mpc.device_tail ? 1 : 0; return QMHIP_OK; } if (!strcmp(key, "fused_policy")) { *value = c->fused_policy ? 1 : 0; return QMHIP_OK; }      // launch-order switches (A/B, tests): 1 is the product's order
  if (!strcmp(key, "r_dense")) { *value = c->mpc.r_force_dense ? 1 : 0; return QMHIP_OK; } if (!strcmp(key, "r_blocks")) { *value = c->mpc.rblk() ? 1 : 0; return QMHIP_OK; }      // r_blocks: the structured instances are the ones that run
  if (!strcmp(key, "wbc_defer") || !strcmp(key, "filler_at_lq")) { *value = 0; return QMHIP_OK; }      // retired scheduling experiments: always off, still answered for bench.py's switch guard
  return QMHIP_ERR_ARG;
}
int qmhip_debug_read(qmhip_ctx* c, const char* name, void* dst, size_t bytes) { QM_GUARD(c);
  if (!c || !name || !dst) return QMHIP_ERR_ARG; hipSetDevice(c->device); const QmMpcBuffers& d = c->mpc.d; const void* p = nullptr;
#define F(n) if (!strcmp(name, #n)) p = d.n;
  if (c->wbc_only) { p = c->wbc.buffer(name); if (!p) { c->fail("qmhip_debug_read: a WBC-only context only has the wbc_* buffers"); return QMHIP_ERR_ARG; } c->bk.to_host(dst, p, bytes); return c->hipstate(); }
  if (!strcmp(name, "sim_rbd")) p = c->sim.s.rbd; if (!strcmp(name, "sim_cmd")) p = c->sim.s.cmd;
  F(lqdbg) F(n_nodes) F(node_t) F(node_ts) F(node_dt) F(node_ev) F(node_mode) F(zvel) F(zpos) F(xref) F(eeref) F(status) F(x) F(u) F(dx) F(du) F(stage) F(perf) F(base_sum) F(perf_sum) F(step_info) F(alpha) F(done) F(xs) F(us) F(out_perf) F(t0) F(x0) F(ipm_s) F(ipm_l) F(ipm_ds) F(ipm_dl) F(ipm_info)
#undef F
  if (!p) p = c->wbc.buffer(name);
  if (!p) { c->fail(std::string("qmhip_debug_read: unknown buffer ") + name); return QMHIP_ERR_ARG; }
  c->bk.to_host(dst, p, bytes); return c->hipstate();
}
int qmhip_microbench_fp64(qmhip_ctx* c, int use_mfma, double* tflops) { QM_GUARD(c);
  if (!c || !tflops) return QMHIP_ERR_ARG; hipSetDevice(c->device);
  const int blocks = 256 * 8, threads = 256, iters = 20000; double* out = (double*)c->bk.alloc((size_t)blocks * threads * 8);
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  for (int rep = 0; rep < 2; ++rep) {
    hipEventRecord(a, c->bk.stream);
    if (use_mfma) hipLaunchKernelGGL(qm_bench_mfma_kernel, dim3(blocks), dim3(threads), 0, c->bk.stream, out, iters);
    else hipLaunchKernelGGL(qm_bench_fma_kernel, dim3(blocks), dim3(threads), 0, c->bk.stream, out, iters);
    hipEventRecord(b, c->bk.stream); hipEventSynchronize(b);
  }
  float ms = 0; hipEventElapsedTime(&ms, a, b);
  const double flops = use_mfma ? (double)blocks * (threads / 64) * iters * 4.0 * (2.0 * 16 * 16 * 4) : (double)blocks * threads * iters * 8.0 * 2.0;
  *tflops = flops / (ms * 1e-3) / 1e12; hipEventDestroy(a); hipEventDestroy(b); c->bk.free(out); return c->hipstate();
}

}  // extern "C"
