"""tools/plan_task_space_demo.py — a plan seen in task space (qmhip_plan_task_space / qmhip_plan_footholds).

  * a trot solve of four instances: the foothold list of instance 0 and the apex height of each of its feet along the horizon;
  * per-launch time of qm_plan_nodes_kernel at B = 1024, N = 100 (C3) next to qm_lq_kin_kernel — K1a — of the same context in the same run (HIP-event spans around
    the launches, qmhip_get_kernel_ms), written to profiles/plan_task_space.json.

    python tools/plan_task_space_demo.py [--batch 1024] [--reps 5] [--out profiles/plan_task_space.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FEET = ("LF", "RF", "LH", "RH")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--intervals", type=int, default=100); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_task_space.json"))
    a = ap.parse_args()
    from qm_control_amd import api, scenarios
    blobs = scenarios.load_blobs()

    cfg = scenarios.make_config("C3", batch=4, n_intervals=60)
    itf = api.QMInterface(blobs=blobs, max_batch=4, max_nodes=80, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    rec, nn = mpc.plan_task_space(); fh, cnt = mpc.plan_footholds(16); n = int(nn[0])
    print("instance 0: %d nodes, t = %.3f ... %.3f s, %d landings inside the horizon" % (n, rec["time"][0, 0], rec["time"][0, n - 1], cnt[0]))
    for s in range(min(int(cnt[0]), 16)):
        print("  t = %.3f s  %s lands at (%.4f, %.4f, %.4f)  [schedule event %d]" % (fh["time"][0, s], FEET[fh["leg"][0, s]], *fh["pos"][0, s], fh["event"][0, s]))
    for k, name in enumerate(FEET):
        z = rec["foot_pos"][0, :n, k, 2]; i = int(np.argmax(z)); print("  %s apex %.4f m at t = %.3f s" % (name, z[i], rec["time"][0, i]))
    print("  end effector: start (%.3f, %.3f, %.3f), end (%.3f, %.3f, %.3f), largest position error against its reference %.2e m" %
          (*rec["ee_pos"][0, 0], *rec["ee_pos"][0, n - 1], np.abs(rec["ee_err"][0, :n, :3]).max()))
    itf.close()

    B, N = a.batch, a.intervals; cfg = scenarios.make_config("C3", batch=B, n_intervals=N)
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=N + 28, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); mpc.plan_task_space()      # warm-up: buffers, code objects
    itf.set_profiling(True); itf.reset_kernel_ms()
    for _ in range(a.reps):
        mpc.solve_resident(cfg["horizon"], warm=True); rec, nn = mpc.plan_task_space()
    itf.synchronize(); plan_ms, plan_n = itf.kernel_ms("plan_nodes"); kin_ms, kin_n = itf.kernel_ms("lq_kin"); itf.set_profiling(False)
    out = dict(workload="C3", batch=B, intervals=N, max_nodes=itf.max_nodes, nodes_max=int(nn.max()), reps=a.reps,
               qm_plan_nodes_kernel_ms=plan_ms / max(plan_n, 1), qm_plan_nodes_launches=plan_n, qm_lq_kin_kernel_ms=kin_ms / max(kin_n, 1), qm_lq_kin_launches=kin_n,
               rows_plan=itf.max_nodes * B, rows_lq_kin=int(nn.max()) * B,
               note="HIP-event spans around each launch (qmhip_set_profiling 1) in one run on one device; the node kernel covers all max_nodes rows per instance (it writes the zero records), K1a the batch's largest node count")
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as fh_:
        json.dump(out, fh_, indent=1); fh_.write("\n")
    itf.close()


if __name__ == "__main__":
    main()
