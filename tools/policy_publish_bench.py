"""tools/policy_publish_bench.py — what the published feedback policy costs (profiles/policy_publish.json).

  * per-launch time of qm_policy_publish_kernel and qm_policy_fb_pub_kernel at B = 1024, W = 8 (HIP-event spans around the launches of the pipelined loop);
  * wall time per tick of qmhip_closed_loop_sim_pipelined (1024 instances, stance -> trot, an MPC call every 8 ticks) with the window on, at ST_FEEDBACK_POLICY 0 and 1,
    and without a window — the loop every earlier build has: `--lib PATH --baseline` runs that one on another build's libqmhip.so for a same-box comparison.
Warm-up loops first, then `--reps` repetitions of `--ticks` ticks each from the same reset; median, minimum and maximum are reported.

    python tools/policy_publish_bench.py [--ticks 320] [--reps 5] [--out profiles/policy_publish.json]
    python tools/policy_publish_bench.py --lib /path/to/parent/libqmhip.so --baseline --out parent.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--window", type=int, default=8); ap.add_argument("--ticks", type=int, default=320)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--lib", default=None); ap.add_argument("--baseline", action="store_true"); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from qm_control_amd import api, layout as L
    if a.lib: api.LIB_PATH = a.lib
    from sim_closed_loop_demo import setup
    B, W, horizon, t_start, every = a.batch, a.window, 0.6, 20.3, 8
    c = setup("trot", B, horizon, t_start=t_start); q0 = c["xbar"][6:30].copy(); q0[2] = 0.385; blobs = (c["mb"], c["st"])
    assert a.ticks % every == 0

    def run(feedback, window, profile=False):
        itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=64, max_ref_knots=2, max_events=c["ev"].shape[1])
        mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True)
        if feedback: itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0)
        if window: itf.set_publish_window(window)
        mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"])
        ms = []; kern = {}
        for rep in range(a.reps + 1):      # the first one is the warm-up
            wbc.reset(); sim.reset(np.tile(q0, (B, 1)), np.zeros((B, 24)), t_start); itf.synchronize()
            if profile and rep == 1: itf.set_profiling(1); itf.reset_kernel_ms()
            t0 = time.perf_counter(); sim.closed_loop(a.ticks, 0.001, horizon, n_substeps=2, mpc_every=every, pipelined=True); itf.synchronize(); dt = time.perf_counter() - t0
            if rep: ms.append(1e3 * dt / a.ticks)
        if profile:
            for name in ("publish", "policy_fb", "policy", "wbc", "sim"):
                tot, n = itf.kernel_ms(name); kern[name] = dict(launches=n, us_per_launch=(1e3 * tot / n if n else None))
        st = sim.state()["status"]; unc = itf.published_info(B)[2] if window else np.zeros(B, np.int32)
        itf.close()
        return dict(ms_per_tick=spread(ms), plant_status_nonzero=int((st != 0).sum()), uncovered_ticks=int(unc.sum()), kernels=kern)

    import torch
    res = dict(tool="tools/policy_publish_bench.py", device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown", batch=B, window=W, ticks=a.ticks, reps=a.reps, mpc_every=every,
               horizon=horizon, lib=os.path.basename(os.path.dirname(os.path.dirname(api.LIB_PATH))) if a.lib else "this build", loop_no_window_feedback0=run(False, 0))
    if not a.baseline:
        res["loop_window_feedback0"] = run(False, W); res["loop_window_feedback1"] = run(True, W)
        prof = run(True, W, profile=True); res["kernels_us_per_launch_at_B%d_W%d" % (B, W)] = prof["kernels"]
        res["published_bytes_per_instance"] = W * L.PR_SIZE * 8
    line = json.dumps(res); print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh: fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
