"""tools/policy_rollout_demo.py — where does the controller take the robot from where it really is? (qmhip_policy_rollout)

For B robots (trot, C3-style random instances) 64 perturbed starts per robot — the plan's first state off by +-0.05 (momentum), +-0.01 (base pose), +-0.05 (joints), random
signs — are rolled over the horizon at steps of sqp.dt under both policies: the feed-forward plan and the SQP's linear controller.  Printed: the share of rollouts whose
smallest friction-cone margin goes negative and the quantiles of the largest state deviation.  Timed: the call (host clock around SqpMpc.rollout_policy) and the kernel
(HIP-event spans, qmhip_get_kernel_ms "rollout"); written with the build's register count to profiles/policy_rollout.json.

    python tools/policy_rollout_demo.py [--batch 16] [--intervals 20] [--reps 5] [--out profiles/policy_rollout.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STARTS = 64
PERTURB = np.concatenate([np.full(6, 0.05), np.full(6, 0.01), np.full(18, 0.05)])


def kernel_registers():
    """vector registers of the built qm_policy_rollout_kernel instances (kernel metadata of the library's gfx950 code object)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_kernel_budgets as kb
        return {n: v["vgpr"] for n, v in kb._kernels().items() if "qm_policy_rollout_kernel" in n and n != "qm_policy_rollout_kernel"}
    except Exception as e:      # (no llvm-readelf on this machine)
        return {"unavailable": str(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16); ap.add_argument("--intervals", type=int, default=20); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gait", default="trot"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_rollout.json"))
    a = ap.parse_args()
    from qm_control_amd import api, layout as L, scenarios
    B, N = a.batch, a.intervals; cfg = scenarios.gait_config(a.gait, batch=B, n_intervals=N, seed=7)
    itf = api.QMInterface(blobs=scenarios.load_blobs(), max_batch=B, max_nodes=N + 28, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); d = mpc.download(); assert (d["status"] >= 0).all()
    rng = np.random.default_rng(1); R = B * STARTS; inst = np.repeat(np.arange(B, dtype=np.int32), STARTS)
    t0 = cfg["t0"][inst]; x0 = d["x"][inst, 0] + rng.choice([-1.0, 1.0], (R, 30)) * PERTURB; t_end = t0 + cfg["horizon"]
    res = {}; timing = {}
    for name, fb in (("feed-forward", False), ("linear controller", True)):
        itf.set_profiling(True)
        for _ in range(2): mpc.rollout_policy(t0, x0, t_end, inst, feedback=fb)      # warm-up: row buffers, code object, the profiling events
        itf.reset_kernel_ms(); w0 = time.perf_counter()
        for _ in range(a.reps): r = mpc.rollout_policy(t0, x0, t_end, inst, feedback=fb)
        wall = (time.perf_counter() - w0) / a.reps; itf.synchronize(); ms, n = itf.kernel_ms("rollout"); itf.set_profiling(False)
        s = r["summary"]; dev = s["max_dev"].max(axis=1); pts = int((s["steps"] + 1).sum()); res[name] = s
        q = np.quantile(dev, [0.5, 0.9, 1.0])
        print("%-17s: %5.1f %% of %d rollouts leave the friction cone (min_cone < 0), %4.1f %% end non-finite; largest state deviation median %.3f, 90 %% %.3f, max %.3f; %d evaluation points" %
              (name, 100.0 * (s["min_cone"] < 0).mean(), R, 100.0 * ((s["flags"] & api.ROLLOUT_NONFINITE) != 0).mean(), q[0], q[1], q[2], pts))
        timing[name] = dict(call_ms=1e3 * wall, kernel_ms=ms / max(n, 1), launches=n, rows_per_s=R / wall, points_per_s=pts / wall, points=pts,
                            share_min_cone_negative=float((s["min_cone"] < 0).mean()), max_dev_quantiles_50_90_100=[float(v) for v in q])
    out = dict(workload="gait:" + a.gait, batch=B, starts_per_robot=STARTS, rows=R, intervals=N, max_step=float(itf.settings_blob[L.ST_SQP_DT]), reps=a.reps, policies=timing, kernel_vgprs=kernel_registers(),
               note="call_ms: host clock around SqpMpc.rollout_policy (staging, four copies up, the launch, five copies back, one stream wait), mean of reps after two warm-up calls; "
                    "kernel_ms: HIP-event span around the launch (qmhip_set_profiling 1), mean per launch, same run, one device")
    print(json.dumps(out, indent=1))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1); fh.write("\n")
    itf.close()


if __name__ == "__main__":
    main()
