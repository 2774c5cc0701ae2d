// k_io.h — hand-over of one control step in ONE buffer (qmhip_step_submit / qmhip_step_collect, include/qmhip.h): per instance a fixed 1024-byte record
// (struct qmhip_step_record, include/qmhip_layout.h: policy at t0, WBC output, perf, status words) and, on request, the primal solution compacted and transposed:
// node-major [nmax][B][k] -> instance-major [B][ncap][k] with ncap = the batch's largest node count (what K0 publishes), not max_nodes.
//
// A plain bandwidth kernel: one thread per 8-byte destination word (destination-indexed like qm_gather_kernel, k_policy.h: coalesced stores, reads in runs of k doubles),
// no LDS, no private segment, no atomics.  The eight status words of a record are stored as 4-byte words: the MPC half and the WBC half of a record are
// written by two launches (below) and n_nodes / qp_status[0] share an 8-byte slot.
//
// Parts.  What a record holds becomes final at two different places of a control step: the MPC fields and the policy at t0 behind the MPC stream's last kernel (the
// batch's apply), the WBC fields behind the WBC on its own stream — and the NEXT step's K0 overwrites n_nodes / status / the node arrays first thing.  One launch
// behind the WBC would therefore hold K0 of step k + 1 back until WBC(k) is through, which is exactly the overlap the two streams exist for.  So the kernel takes a
// mask of parts and a step with the WBC launches it twice, each IN ORDER on the stream that produces what it reads: nothing of the next step can overtake it, and
// no event is needed between the pack and the producers of step k + 1.
#pragma once
#include "k_grid.h"

#define QM_PACK_MPC   1   /* x_des, u_des, perf, mode, mpc_status, n_nodes, reserved words */
#define QM_PACK_WBC   2   /* wbc_out, qp_status from the WBC's buffers */
#define QM_PACK_NOWBC 4   /* wbc_out, qp_status = 0: the step ran without the WBC */
#define QM_PACK_TRAJ  8   /* node_t, xs, us, node_ev, node_mode -> instance-major, ncap nodes per instance; nodes >= n_nodes[b] are zero */
#define QM_PACK_LANES (QM_STEP_DOUBLES + QM_STEP_INTS)   /* threads per record: one per double, one per status word */

__host__ __device__ inline int qm_mpc_status(int k0_status, const double* step_info4, bool strict);      // csrc/host/qm_pipeline.h: the function qmhip_mpc_download runs on the host

struct QmStepPackArgs {
  int B, nmax, ncap, parts, strict;
  const double* x_des; const double* u_des; const int* mode; const double* wbc_out; const int* qp_status;      // QmWbcBuffers
  const double* out_perf; const int* status; const double* step_info; const int* n_nodes;                       // QmMpcBuffers, per instance
  const double* node_t; const int* node_ev; const int* node_mode; const double* xs; const double* us;           // QmMpcBuffers, node-major [nmax][B][k]
  double* rec;      // [B][128] 8-byte words
  double* traj;     // [B][ncap] t | [B][ncap][30] x | [B][ncap][30] u | [B][ncap] event (int32, padded to 8 bytes) | [B][ncap] mode (int32, padded)
};
// 8-byte words of the trajectory part and of its sections (host and device agree through these)
__host__ __device__ inline size_t qm_pack_pairs(int B, int ncap) { return ((size_t)B * ncap + 1) / 2; }
__host__ __device__ inline size_t qm_pack_traj_words(int B, int ncap) { return (size_t)B * ncap * 61 + 2 * qm_pack_pairs(B, ncap); }
__host__ __device__ inline size_t qm_pack_threads(int B, int ncap, int parts) { return (size_t)B * QM_PACK_LANES + ((parts & QM_PACK_TRAJ) ? qm_pack_traj_words(B, ncap) : 0); }

__global__ void qm_step_pack_kernel(QmStepPackArgs a) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nrec = (size_t)a.B * QM_PACK_LANES;
  if (g < nrec) {
    const int b = (int)(g / QM_PACK_LANES), f = (int)(g % QM_PACK_LANES);
    double* r = a.rec + (size_t)b * (QM_STEP_BYTES / 8);
    if (f < QM_STEP_WBC) { if (a.parts & QM_PACK_MPC) r[f] = f < QM_STEP_UDES ? a.x_des[(size_t)b * 30 + f] : a.u_des[(size_t)b * 30 + f - QM_STEP_UDES]; }
    else if (f < QM_STEP_PERF) { if (a.parts & QM_PACK_WBC) r[f] = a.wbc_out[(size_t)b * QM_NWBC_OUT + f - QM_STEP_WBC]; else if (a.parts & QM_PACK_NOWBC) r[f] = 0.0; }
    else if (f < QM_STEP_DOUBLES) { if (a.parts & QM_PACK_MPC) r[f] = a.out_perf[(size_t)b * 10 + f - QM_STEP_PERF]; }
    else {
      const int j = f - QM_STEP_DOUBLES; int* ri = (int*)(r + QM_STEP_DOUBLES);
      if (j >= QM_STEP_I_QP && j < QM_STEP_I_QP + 3) { if (a.parts & QM_PACK_WBC) ri[j] = a.qp_status[(size_t)b * 3 + j - QM_STEP_I_QP]; else if (a.parts & QM_PACK_NOWBC) ri[j] = 0; }
      else if (a.parts & QM_PACK_MPC)
        ri[j] = j == QM_STEP_I_MODE ? a.mode[b] : j == QM_STEP_I_STATUS ? qm_mpc_status(a.status[b], a.step_info + (size_t)b * 4, a.strict != 0) : j == QM_STEP_I_NODES ? a.n_nodes[b] : 0;
    }
    return;
  }
  if (!(a.parts & QM_PACK_TRAJ)) return;
  size_t h = g - nrec; const size_t BN = (size_t)a.B * a.ncap;
  if (h < BN) {      // node times
    const int b = (int)(h / a.ncap), i = (int)(h % a.ncap);
    a.traj[h] = i < a.n_nodes[b] ? a.node_t[(size_t)i * a.B + b] : 0.0; return;
  }
  h -= BN;
  if (h < BN * 60) {      // state, then input trajectory: destination (b, i, q), coalesced stores, reads in runs of 30 doubles
    const bool is_x = h < BN * 30; const size_t e = is_x ? h : h - BN * 30;
    const int q = (int)(e % 30); const size_t bi = e / 30; const int b = (int)(bi / a.ncap), i = (int)(bi % a.ncap);
    const double* src = is_x ? a.xs : a.us;
    a.traj[BN + h] = i < a.n_nodes[b] ? src[((size_t)i * a.B + b) * 30 + q] : 0.0; return;
  }
  h -= BN * 60; const size_t np = qm_pack_pairs(a.B, a.ncap);
  if (h < 2 * np) {      // event tags, then modes: two int32 per thread, one 8-byte store
    const int* src = h < np ? a.node_ev : a.node_mode; const size_t p = h < np ? h : h - np; unsigned v[2] = {0u, 0u};
    for (int k = 0; k < 2; ++k) { const size_t e = 2 * p + k; if (e < BN) { const int b = (int)(e / a.ncap), i = (int)(e % a.ncap); if (i < a.n_nodes[b]) v[k] = (unsigned)src[(size_t)i * a.B + b]; } }
    ((unsigned long long*)(a.traj + BN * 61))[h] = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
  }
}
