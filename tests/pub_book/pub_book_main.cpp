// tests/pub_book/pub_book_main.cpp — TEST INFRASTRUCTURE: the slot / sequence / mutex bookkeeping of the published policy (csrc/host/qm_publish_book.h) in a stand-alone
// host program with a stub "device": no GPU, no kernels.  Built and run by tests/test_publish_book.py with the address + undefined-behaviour sanitizers and with the
// thread sanitizer.  One publisher thread and three evaluator threads share a QmPubBook; the stub executes every "enqueued" operation at once on the calling thread, so the
// sanitizers see exactly the accesses the protocol allows to overlap: the publisher fills the INACTIVE slot outside the mutex while evaluators read the ACTIVE one inside it.
// A slot that is read while it is written is a data race (thread sanitizer) and a torn stamp (the checks below).  Exit status 0: every check held.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "../../qm_control_amd/csrc/host/qm_publish_book.h"

enum { WORDS = 512 };
struct StubSlot { long data[WORDS]; long pub_events = 0, eval_events = 0, waited_for_eval = 0; };      // data: the publication's stamp in every word
static StubSlot g_slot[2];
static std::atomic<int> g_fail{0};
#define CHECK(c) do { if (!(c)) { if (!g_fail.exchange(1)) fprintf(stderr, "pub_book_main: check failed at line %d: %s\n", __LINE__, #c); } } while (0)

int main(int argc, char** argv) {
  const int n_pub = argc > 1 ? atoi(argv[1]) : 2000;
  QmPubBook book;
  // before a window / before a publication: nothing to publish into, nothing to evaluate
  { bool w = false; QmPubBook::Eval e; CHECK(book.begin_publish(&w) == -1); CHECK(!book.begin_eval(e)); CHECK(book.end_publish(1, true) == -1); }
  book.reset(8);
  { QmPubBook::Eval e; CHECK(!book.begin_eval(e)); long s = -1; int w = 0, a = 0, B = -1; book.info(&s, &w, &a, &B); CHECK(s == 0 && w == 8 && a == -1 && B == 0); }
  // a second publication cannot start while one is under way
  { bool w = true; const int t = book.begin_publish(&w); CHECK(t == 0 && !w); bool w2 = false; CHECK(book.begin_publish(&w2) == -1); for (long& x : g_slot[t].data) x = 1; CHECK(book.end_publish(3, false) == 1); }
  { QmPubBook::Eval e; CHECK(book.begin_eval(e)); CHECK(e.slot == 0 && e.seq == 1 && e.B == 3 && !e.gains); book.end_eval(e, false);      // gave up: no evaluation event on the slot
    bool w = true; const int t = book.begin_publish(&w); CHECK(t == 1 && !w); for (long& x : g_slot[t].data) x = 2; CHECK(book.end_publish(3, true) == 2);
    CHECK(book.begin_eval(e)); CHECK(e.slot == 1 && e.seq == 2 && e.gains); book.end_eval(e, true);
    const int t2 = book.begin_publish(&w); CHECK(t2 == 0 && !w); for (long& x : g_slot[t2].data) x = 3; CHECK(book.end_publish(3, true) == 3);      // slot 0 had no evaluation enqueued
    const int t3 = book.begin_publish(&w); CHECK(t3 == 1 && w); for (long& x : g_slot[t3].data) x = 4; CHECK(book.end_publish(3, true) == 4);                                   // slot 1 had one: wait for its event, once
    const int t4 = book.begin_publish(&w); CHECK(t4 == 0 && !w); for (long& x : g_slot[t4].data) x = 5; CHECK(book.end_publish(3, true) == 5); }
  const long seq0 = 5;
  std::atomic<bool> stop{false}; std::atomic<long> evals{0}; std::vector<long> distinct(3, 0);
  std::thread publisher([&]() {
    for (int k = 0; k < n_pub; ++k) {
      bool wait_eval = false; const int t = book.begin_publish(&wait_eval); CHECK(t == 0 || t == 1); if (t < 0) break;
      StubSlot& s = g_slot[t];
      if (wait_eval) { s.waited_for_eval++; }                     // the publishing stream waits for the slot's evaluation event
      const long stamp = seq0 + k + 1; for (long& x : s.data) x = stamp;      // the snapshot: outside the mutex, into the inactive slot
      s.pub_events++;                                            // the slot's publication event
      CHECK(book.end_publish(1 + k % 4, (k & 1) != 0) == stamp);
    }
    stop = true;
  });
  std::vector<std::thread> evaluators;
  for (int id = 0; id < 3; ++id) evaluators.emplace_back([&, id]() {
    long last = 0;
    while (!stop) {
      QmPubBook::Eval e; if (!book.begin_eval(e)) { CHECK(false); break; }
      CHECK(e.seq >= last);                                       // the sequence number never goes back
      if (e.seq != last) distinct[id]++; last = e.seq;
      const StubSlot& s = g_slot[e.slot]; bool torn = false; for (long x : s.data) torn |= x != e.seq;      // the evaluation reads the slot it was handed: all of one publication
      CHECK(!torn); CHECK(e.B == 1 + (int)((e.seq - seq0 - 1) % 4) || e.seq <= seq0); CHECK(e.gains == (((e.seq - seq0 - 1) & 1) != 0) || e.seq <= seq0);
      g_slot[e.slot].eval_events++;                              // the slot's evaluation event, recorded under the mutex
      book.end_eval(e, (evals.fetch_add(1) % 5) != 0);           // (every fifth evaluator gives up before enqueuing)
    }
  });
  publisher.join(); for (auto& t : evaluators) t.join();
  long s = 0; int w = 0, a = -1, B = 0; book.info(&s, &w, &a, &B);
  CHECK(s == seq0 + n_pub && w == 8 && (a == 0 || a == 1) && g_slot[a].data[0] == s && g_slot[1 - a].data[WORDS - 1] == s - 1);
  CHECK(g_slot[0].pub_events + g_slot[1].pub_events == n_pub);
  book.reset(0); { QmPubBook::Eval e; bool wq = false; CHECK(!book.begin_eval(e)); CHECK(book.begin_publish(&wq) == -1); }
  printf("pub_book_main: publications %ld evaluations %ld distinct_seq_seen %ld %ld %ld waits_for_eval %ld result %s\n", s, evals.load(), distinct[0], distinct[1], distinct[2],
         g_slot[0].waited_for_eval + g_slot[1].waited_for_eval, g_fail ? "FAIL" : "ok");
  return g_fail ? 1 : 0;
}
