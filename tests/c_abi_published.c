/* tests/c_abi_published.c — the reference's policy hand-over between its two threads, driven through the C ABI from plain C + pthreads (compiled by
 * tests/test_gpu_published_policy.py):
 *   thread A = mpcThread_   (qm_controllers/src/QMController.cpp:315-333): observation -> warm MPC solve -> qmhip_policy_publish (the policy buffer swap), 100 times;
 *   thread B = the control tick (QMController.cpp:133-148): updatePolicy + evaluatePolicy(time, state) = qmhip_policy_eval_published at about 1 kHz with a perturbed state,
 *             on the SAME context — it takes the publication mutex only, never the context lock — logging (seq, t, x, x_des, u_des, mode, covered).
 * Afterwards the same solve sequence is replayed single-threaded and every logged query is evaluated again on the publication with its sequence number: the same kernel on
 * the same data, so every output must be bit-identical.  Single robot (B = 1), trot, N = 100, window 8.  Any failed call ends the program with a
 * non-zero status; nothing is retried.
 * usage: c_abi_published robot.urdf task.info reference.info */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "qmhip.h"

enum { MAXN = 160, NREF = 2, NEV = 24, SOLVES = 100, WINDOW = 8, MAXQ = 4000 };
static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
static void sleep_until(double t) { struct timespec ts; ts.tv_sec = (time_t)t; ts.tv_nsec = (long)((t - (double)ts.tv_sec) * 1e9); clock_nanosleep(CLOCK_MONOTONIC, TIMER_ABSTIME, &ts, NULL); }

typedef struct { int64_t seq; double t, x[QM_NX], xd[QM_NX], ud[QM_NU]; int32_t mode, covered; } query;
static query qlog[MAXQ]; static int n_queries = 0;
static double x0[QM_NX], horizon, t_first;
static volatile int mpc_done = 0, mpc_err = 0, tick_err = 0;
static qmhip_ctx* ctx = NULL;

static double t0_of(int k) { return t_first + 0.0013 + 0.002 * k; }      /* never exactly on a gait event; stays inside the uploaded schedule */
static int solve_and_publish(int k) {
  const double t0 = t0_of(k); int rc = qmhip_mpc_set_initial(ctx, 1, &t0, x0);
  if (rc == QMHIP_OK) rc = qmhip_mpc_solve_resident_warm(ctx, 1, horizon);
  if (rc == QMHIP_OK) rc = qmhip_policy_publish(ctx, 1);
  if (rc != QMHIP_OK) fprintf(stderr, "solve %d failed (%d): %s\n", k, rc, qmhip_last_error(ctx));
  return rc;
}
static void* mpc_thread(void* p) {
  (void)p; const double t_begin = now_s();
  for (int k = 0; k < SOLVES && !tick_err; ++k) { sleep_until(t_begin + 0.006 * k); if (solve_and_publish(k) != QMHIP_OK) { mpc_err = 1; break; } }
  mpc_done = 1; return NULL;
}
static void* tick_thread(void* p) {
  (void)p; const double t_begin = now_s();
  for (int i = 0; !mpc_done && i < MAXQ; ++i) {
    sleep_until(t_begin + 0.001 * i);
    query* q = &qlog[n_queries]; q->t = t_first + 0.005 + 0.002 * (i % 110);      /* in front of, inside and behind the window of whichever publication is active */
    for (int j = 0; j < QM_NX; ++j) q->x[j] = x0[j] + (j < 6 ? 0.02 : 0.01) * sin(0.37 * i + 0.9 * j);
    const int rc = qmhip_policy_eval_published(ctx, 1, &q->t, q->x, q->xd, q->ud, &q->mode, &q->covered, &q->seq);
    if (rc != QMHIP_OK) { fprintf(stderr, "qmhip_policy_eval_published failed (%d): %s\n", rc, qmhip_last_error(ctx)); tick_err = 1; break; }
    n_queries++;
  }
  return NULL;
}
static int setup(void) {
  static double mb[MB_SIZE], st[ST_SIZE]; qmhip_export_blobs(ctx, mb, st);
  horizon = 100 * st[ST_SQP_DT]; t_first = 0.1; memcpy(x0, st + ST_XINIT, sizeof(x0));
  double ev[NEV]; int32_t modes[NEV + 1]; ev[0] = 0.0; modes[0] = QM_MODE_STANCE;
  for (int k = 1; k < NEV; ++k) { ev[k] = ev[k - 1] + 0.35; modes[k] = (k & 1) ? QM_MODE_LF_RH : QM_MODE_RF_LH; }
  modes[NEV] = QM_MODE_STANCE;
  double ref_t[NREF] = {t_first, t_first + horizon}, ref_x[NREF][QM_NREF]; const double ee[7] = {0.52, 0.09, 0.38 + 0.4, 0.5, -0.5, 0.5, -0.5};
  for (int k = 0; k < NREF; ++k) {
    memset(ref_x[k], 0, sizeof(ref_x[k]));
    for (int i = 0; i < 6; ++i) ref_x[k][6 + i] = x0[6 + i];
    ref_x[k][8] = 0.4; ref_x[k][10] = ref_x[k][11] = 0.0;
    if (k == 1) ref_x[k][6] += 0.3;
    for (int q = 0; q < QM_NJ; ++q) ref_x[k][12 + q] = mb[MB_QNOM + q];
    memcpy(ref_x[k] + 30, ee, sizeof(ee));
  }
  /* the episode's start: publications restart at sequence number 1, the first solve is cold */
  if (qmhip_policy_set_publish_window(ctx, WINDOW) != QMHIP_OK || qmhip_mpc_upload(ctx, 1, &t_first, x0, NREF, ref_t, &ref_x[0][0], NEV, ev, modes) != QMHIP_OK ||
      qmhip_mpc_solve_resident(ctx, 1, horizon) != QMHIP_OK) { fprintf(stderr, "setup: %s\n", qmhip_last_error(ctx)); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s robot.urdf task.info reference.info\n", argv[0]); return 2; }
  if (qmhip_create(argv[1], argv[2], argv[3], 0, 1, MAXN, NREF, NEV, &ctx) != QMHIP_OK) { fprintf(stderr, "qmhip_create: %s\n", qmhip_last_error(NULL)); return 1; }
  if (qmhip_set_setting(ctx, ST_FEEDBACK_POLICY, 1.0) != QMHIP_OK || setup()) { fprintf(stderr, "setup: %s\n", qmhip_last_error(ctx)); return 1; }
  if (solve_and_publish(0) != QMHIP_OK) return 1;      /* the control thread starts on a policy, as the reference's does (QMController::starting waits for the first one) */
  pthread_t ta, tb; pthread_create(&ta, NULL, mpc_thread, NULL); pthread_create(&tb, NULL, tick_thread, NULL);
  pthread_join(ta, NULL); pthread_join(tb, NULL);
  if (mpc_err || tick_err) { qmhip_destroy(ctx); printf("result: FAIL (a call failed)\n"); return 1; }
  int64_t last = 0; int distinct = 0, covered = 0; for (int i = 0; i < n_queries; ++i) { if (qlog[i].seq != last) distinct++; last = qlog[i].seq; covered += qlog[i].covered; }
  /* replay, single-threaded: publication s of the replay is publication s of the threaded run (the first solve_and_publish(0) above is s = 1, thread A's k-th s = k + 2) */
  int mismatches = 0, errors = 0, checked = 0;
  if (setup()) return 1;
  for (int s = 1; s <= SOLVES + 1 && !errors; ++s) {
    if (solve_and_publish(s == 1 ? 0 : s - 2) != QMHIP_OK) { errors++; break; }
    for (int i = 0; i < n_queries; ++i) if (qlog[i].seq == s) {
      query r = qlog[i]; memset(r.xd, 0, sizeof(r.xd)); memset(r.ud, 0, sizeof(r.ud)); r.mode = -1; r.covered = -1; r.seq = -1;
      if (qmhip_policy_eval_published(ctx, 1, &r.t, r.x, r.xd, r.ud, &r.mode, &r.covered, &r.seq) != QMHIP_OK) { fprintf(stderr, "replay: %s\n", qmhip_last_error(ctx)); errors++; break; }
      checked++;
      if (r.seq != s || r.mode != qlog[i].mode || r.covered != qlog[i].covered || memcmp(r.xd, qlog[i].xd, sizeof(r.xd)) || memcmp(r.ud, qlog[i].ud, sizeof(r.ud))) mismatches++;
    }
  }
  if (checked != n_queries) mismatches += n_queries - checked;
  printf("published: solves %d publications %d queries %d distinct_seq %d covered %d mismatches %d errors %d\n", SOLVES, SOLVES, n_queries, distinct, covered, mismatches, errors);
  qmhip_destroy(ctx);
  const int fail = mismatches || errors || distinct < 20;
  printf("result: %s\n", fail ? "FAIL" : "ok");
  return fail ? 3 : 0;
}
