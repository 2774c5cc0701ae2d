// k_sense.h — K8b: sensor model between the batched plant and the controller (include/qmhip.h, "sensor model"), ONE WAVEFRONT PER INSTANCE.
//
// The reference's simulation feeds its controller the plant's exact state ("ground truth" estimator, FromTopiceEstimate); this kernel stands where a real robot's
// sensors and estimator would hand over something imperfect.  Behind every plant step it takes one SAMPLE of the plant's rbd state (k_sim.h's hand-over, the
// estimator's layout, qm_estimation/src/StateEstimateBase.cpp:41-103), keeps it in a per-instance ring of QM_SENSE_MAX_LAG + 1 samples, and writes what the
// controller is told: the truth of `lag` samples ago, plus a constant bias and white noise per group of the state (struct qmhip_sensor, qmhip_layout.h).  The
// end-effector pose rbd[48:55] of a noisy instance is forward kinematics of the MEASURED configuration, as StateEstimateBase::updateArmEE computes it from the
// estimate (StateEstimateBase.cpp:80-103), with the routine the plant's hand-over uses (the arm lane of rbd_chain + mat_to_quat).
// The generator is integer arithmetic up to one conversion and one product, the corruption four individually rounded operations: numpy, the host emulator and the
// device agree bit for bit.
#pragma once
#include "qm_dev_rbd.h"
#include "qm_dev_kin.h"

#define QM_SENSE_SLOTS (QM_SENSE_MAX_LAG + 1)
#define QM_SENSE_WORDS (QM_SENSE_BYTES / 8)   /* seed, {lag, spare0}, sigma(6), bias_sigma(6), spare(2) */
#define QM_SENSE_COMPS 48                     /* corrupted components: the rbd state without the end-effector pose */
struct QmSenseArgs {
  const double* mb;
  int B; int nB; int restart;           // instances of the step; instances with a record (the others are copied); 1: this is sample 0 (hand-over of a reset, new records)
  const unsigned long long* rec;        // [nB][QM_SENSE_WORDS] struct qmhip_sensor as 8-byte words
  const double* rbd;                    // [B][55] the plant's state (truth)
  double* ring;                         // [B][QM_SENSE_SLOTS][55] truth of the last samples, sample n in slot n % QM_SENSE_SLOTS
  int* n;                               // [B] index of the last sample taken
  double* meas;                         // [B][55] what the controller is told
};

// ---- LDS carve (doubles) ----
#define SN_REC   0                      /* [16] the record's words */
#define SN_X     16                     /* [55] the measured state */
#define SN_Q     72                     /* [24] measured configuration in the plant's coordinates */
#define SN_V     96                     /* [24] zeros: the pose needs no velocity */
#define SN_COMP  120                    /* [6][19] the arm chain's per-joint composites (one lane: stride 1) */
#define SN_TOTAL (SN_COMP + 6 * RBD_COMP)
#define SENSE_LDS_BYTES (SN_TOTAL * 8)

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long sense_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
// word w of component c of sample n (n = 2^64 - 1: the bias draw); all arithmetic mod 2^64
__device__ __forceinline__ unsigned long long sense_word(unsigned long long seed, unsigned long long n, int c, int w) {
  const unsigned long long G = 0x9E3779B97F4A7C15ull;
  return sense_mix(sense_mix(seed + G * (n + 1ull)) + G * (unsigned long long)(2 * c + w + 1));
}
// eight-term Irwin-Hall variable of unit variance from the sixteen-bit fields of two words; |nu| <= 8 * 65535 * C = 4.8989...
__device__ __forceinline__ double sense_nu(unsigned long long seed, unsigned long long n, int c) {
  int s = 0;
  for (int w = 0; w < 2; ++w) { const unsigned long long x = sense_word(seed, n, c, w); for (int k = 0; k < 4; ++k) s += (int)((x >> (16 * k)) & 0xFFFFull); }
  return (double)(2 * s - 8 * 65535) * 0x1.3988e1412ed76p-17;      // the double nearest 1 / sqrt(8 (65536^2 - 1) / 3)
}
// (x + bias_sigma nu_bias) + sigma nu: two products, the inner sum, the outer sum, each rounded on its own (no fused multiply-add)
__device__ __forceinline__ double sense_corrupt(double x, double bias_sigma, double sigma, unsigned long long seed, unsigned long long n, int c) {
#pragma clang fp contract(off)
  const double pb = bias_sigma * sense_nu(seed, ~0ull, c);
  const double pn = sigma * sense_nu(seed, n, c);
  const double t = x + pb;
  return t + pn;
}
__device__ __forceinline__ int sense_group(int c) { return c < 3 ? 0 : c < 6 ? 1 : c < 24 ? 2 : c < 27 ? 3 : c < 30 ? 4 : 5; }

__global__ void __launch_bounds__(64) qm_sense_kernel(QmSenseArgs a) {
  extern __shared__ double qm_smem[];
  double* S = qm_smem;
  const int b = blockIdx.x, l = threadIdx.x & 63;
  if (b >= a.B) return;
  const double* mb = qm_table(a.mb);
  unsigned long long* R = (unsigned long long*)(S + SN_REC);      // (this part of the carve is only ever read and written as 8-byte integers)
  double* X = S + SN_X; double* Q = S + SN_Q; double* V = S + SN_V;
  if (l < QM_SENSE_WORDS) R[l] = (b < a.nB) ? a.rec[(size_t)b * QM_SENSE_WORDS + l] : 0ull;      // no record: identity (copied)
  if (l < 24) V[l] = 0.0;
  const int n = a.restart ? 0 : a.n[b] + 1;
  qm_wave_sync();
  const unsigned long long seed = R[0];
  int lag = (int)(unsigned)(R[1] & 0xFFFFFFFFull); lag = lag < 0 ? 0 : (lag > QM_SENSE_MAX_LAG ? QM_SENSE_MAX_LAG : lag);      // (validated by the host; the ring has no other slots)
  bool noisy = false;
  for (int g = 0; g < 2 * QM_SENSE_GROUPS; ++g) noisy = noisy || __builtin_bit_cast(double, R[2 + g]) != 0.0;
  const int m = n - (lag < n ? lag : n);      // the source sample: before `lag` samples exist, the oldest one
  double* ring = a.ring + (size_t)b * QM_SENSE_SLOTS * QM_NRBD;
  if (l < QM_NRBD) {
    const double x = a.rbd[(size_t)b * QM_NRBD + l];
    ring[(n % QM_SENSE_SLOTS) * QM_NRBD + l] = x;
    double y = (m == n) ? x : ring[(m % QM_SENSE_SLOTS) * QM_NRBD + l];
    if (l < QM_SENSE_COMPS) {
      const int g = sense_group(l);
      const double sg = __builtin_bit_cast(double, R[2 + g]), bs = __builtin_bit_cast(double, R[2 + QM_SENSE_GROUPS + g]);
      if (sg != 0.0 || bs != 0.0) y = sense_corrupt(y, bs, sg, seed, (unsigned long long)n, l);      // a clean group is copied, not added to
    }
    X[l] = y;
  }
  qm_wave_sync();
  if (noisy) {                          // (wave-uniform) end-effector pose of the measured configuration; a clean instance keeps the delayed truth's
    if (l < 3) { Q[l] = X[3 + l]; Q[3 + l] = X[l]; }
    if (l >= 6 && l < 24) Q[l] = X[l];
    qm_wave_sync();
    if (l == 0) {
      RbdBase Bb; rbd_base(Q, V, Bb);
      double cm = 0.0, ch[3] = {0, 0, 0}, cI[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, F[3] = {0, 0, 0}, NO[3] = {0, 0, 0};
      RbdJsink Jt; Jt.rows = nullptr; Jt.nrows = 0; Jt.dummy = 0.0;
      RbdTip tip; RbdCompLds comp; comp.base = S + SN_COMP; comp.stride = 1;
      rbd_chain<6, double*, RbdJsink, RbdCompLds>(mb, 12, 4, Q, V, Bb, (double*)nullptr, (double*)nullptr, false, cm, ch, cI, F, NO, (RbdSums*)nullptr, tip, Jt, false, 6, comp);
      double qq[4]; mat_to_quat(tip.R, qq);
      for (int i = 0; i < 3; ++i) X[48 + i] = tip.p[i];
      for (int i = 0; i < 4; ++i) X[51 + i] = qq[i];
    }
    qm_wave_sync();
  }
  if (l < QM_NRBD) a.meas[(size_t)b * QM_NRBD + l] = X[l];
  if (l == 0) a.n[b] = n;
}
