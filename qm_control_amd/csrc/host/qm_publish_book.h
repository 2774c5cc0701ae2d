// qm_publish_book.h — slot / sequence / mutex bookkeeping of the published policy (qm_publish_pipeline.h).  Plain C++, no device code: the stand-alone host program
// tests/pub_book/pub_book_main.cpp runs it under the address, undefined-behaviour and thread sanitizers.
//
// Two slots.  ONE publisher at a time (the context lock, or the loop that owns the context) fills the slot that is NOT active and then makes it active; any number of
// evaluators read the active slot.  The small mutex `mu` is all an evaluator takes — never the context lock — and it holds it only while it ENQUEUES: ordering on the
// device is by events, which the caller owns (one "published" and one "last evaluation" event per slot):
//   evaluator:  begin_eval (locks; picks the active slot)  ->  wait for the slot's publication event, enqueue, record the slot's evaluation event  ->  end_eval (unlocks)
//   publisher:  begin_publish (the inactive slot; tells whether evaluations were enqueued on it since it was last filled: then the publishing stream first waits for that
//               slot's evaluation event — final by now, because evaluators only ever pick the active slot)  ->  enqueue the snapshot, record the publication event
//               ->  end_publish (the slot becomes active, the sequence number advances)
// Nothing here spins or waits for the device.
#pragma once
#include <mutex>

struct QmPubBook {
  std::mutex mu;
  int window = 0;             // nodes per instance a slot's gain window holds; 0: publishing is off (nothing allocated)
  int active = -1;            // slot evaluations read; -1: nothing published yet
  long seq = 0;               // publications so far (the active slot's is `seq`)
  struct Slot { long seq = 0; int B = 0; bool gains = false; bool eval_pending = false; } slot[2];
  bool publishing = false; int target = -1;

  void reset(int w) { std::lock_guard<std::mutex> g(mu); window = w; active = -1; seq = 0; slot[0] = Slot(); slot[1] = Slot(); publishing = false; target = -1; }
  // -> the slot to fill, -1 when publishing is off or a publication is already under way; *wait_eval: order the snapshot behind the slot's evaluation event
  int begin_publish(bool* wait_eval) {
    std::lock_guard<std::mutex> g(mu);
    if (window <= 0 || publishing) return -1;
    target = active < 0 ? 0 : 1 - active; publishing = true;
    *wait_eval = slot[target].eval_pending; slot[target].eval_pending = false;
    return target;
  }
  long end_publish(int B, bool gains) {
    std::lock_guard<std::mutex> g(mu);
    if (!publishing) return -1;
    Slot& s = slot[target]; s.seq = ++seq; s.B = B; s.gains = gains; active = target; publishing = false;
    return seq;
  }
  struct Eval { std::unique_lock<std::mutex> lk; int slot = -1; long seq = 0; int B = 0; bool gains = false; };
  // false (nothing locked): nothing published yet
  bool begin_eval(Eval& e) {
    e.lk = std::unique_lock<std::mutex>(mu);
    if (window <= 0 || active < 0) { e.lk.unlock(); return false; }
    const Slot& s = slot[active]; e.slot = active; e.seq = s.seq; e.B = s.B; e.gains = s.gains;
    return true;
  }
  // enqueued: the evaluation's event has been recorded on the slot (false: the evaluator gave up before enqueuing anything)
  void end_eval(Eval& e, bool enqueued) { if (enqueued) slot[e.slot].eval_pending = true; e.lk.unlock(); }
  void info(long* seq_out, int* window_out, int* active_out, int* B_out) { std::lock_guard<std::mutex> g(mu); if (seq_out) *seq_out = seq; if (window_out) *window_out = window; if (active_out) *active_out = active; if (B_out) *B_out = active < 0 ? 0 : slot[active].B; }
};
