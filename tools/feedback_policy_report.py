"""tools/feedback_policy_report.py — what the feedback policy (ST_FEEDBACK_POLICY, sqp.useFeedbackPolicy) costs and does on one MI355X; writes profiles/feedback_policy.json.
  (a) time per launch of qm_policy_fb_kernel next to qm_policy_kernel at B = 1024 (qmhip_get_kernel_ms, same process);
  (b) instance-ticks/s of the loop around the plant (bench.py's closed_loop_plant cell: 30 ticks, MPC every 10th) with the setting off, on, off again;
  (c) the figures of tools/sim_robustness.py (upright count, base travel, end-effector deviation) off / on at the demo's mpc_every (10) and at twice that.
Reported, not gated.  Usage: python tools/feedback_policy_report.py [ticks] [batch]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from qm_control_amd import api, layout as L
from sim_closed_loop_demo import setup

ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 3000; B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
horizon = 1.0; out = {"batch": B, "ticks": ticks}


def episode(feedback, mpc_every, n_ticks, timed=False):
    """one episode of tools/sim_robustness.py (same seed, same perturbations) with the setting `feedback`"""
    rng = np.random.default_rng(7); c = setup("trot", B, horizon)
    q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; q[:, 6:18] += 0.03 * rng.normal(size=(B, 12)); q[:, 18:] += 0.1 * rng.normal(size=(B, 6)); q[:, 5] += 0.1 * rng.normal(size=B)
    itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True, feedback_policy=feedback)
    sim.reset(q, np.zeros((B, 24)), 20.0); rbd0, _ = sim.step(1e-9, 1)
    for b in range(B):
        c["ref_x"][b, :, 30:37] = rbd0[b, 48:55]; c["ref_x"][b, :, 11] = q[b, 5]; c["ref_x"][b, :, 9] = 0.0
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset(); sim.reset(q, np.zeros((B, 24)), 20.0)
    if timed:      # (b): the bench cell — 10 ticks of warm-up, 30 timed
        sim.closed_loop(10, 0.001, horizon, n_substeps=2, mpc_every=10); itf.synchronize()
        t = time.perf_counter(); sim.closed_loop(30, 0.001, horizon, n_substeps=2, mpc_every=10); itf.synchronize(); t = time.perf_counter() - t
        itf.close(); return B * 30 / t
    bad_mpc = np.zeros(B, bool); bad_wbc = np.zeros(B, bool); dev = np.zeros(B)
    for k in range(0, n_ticks, 100):
        sim.closed_loop(100, 0.001, horizon, n_substeps=2, mpc_every=mpc_every)
        res = mpc.download(); _, st3 = wbc.download(B); rbd = itf.debug_read("sim_rbd", (B, 55))
        bad_mpc |= res["status"] != 0; bad_wbc |= (st3 != 0).any(1); dev = np.maximum(dev, np.linalg.norm(rbd[:, 48:51] - rbd0[:, 48:51], axis=1))
    s = sim.state(); up = np.isfinite(s["q"]).all(1) & (np.abs(s["q"][:, 3:5]).max(1) < 0.3) & (s["q"][:, 2] > 0.3)
    r = dict(upright=int(up.sum()), mpc_status_nonzero=int(bad_mpc.sum()), wbc_status_nonzero=int(bad_wbc.sum()))
    if up.any():
        r.update(base_travel_mean_m=float(s["q"][up, 0].mean()), base_travel_min_m=float(s["q"][up, 0].min()), base_travel_max_m=float(s["q"][up, 0].max()),
                 ee_dev_median_mm=float(1e3 * np.median(dev[up])), ee_dev_p95_mm=float(1e3 * np.percentile(dev[up], 95)), ee_dev_max_mm=float(1e3 * dev[up].max()))
    itf.close(); return r


# (a) kernel time per launch
c = setup("trot", B, horizon); itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1]); mpc = api.SqpMpc(itf)
mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); mpc.solve_resident(horizon)
rng = np.random.default_rng(1); t = c["t0"] + rng.uniform(0.0, horizon, B); x = c["x0"] + 1e-2 * rng.normal(size=(B, 30))
for _ in range(3): mpc.evaluate_policy(t, x); mpc.evaluatePolicy(t)
itf.set_profiling(1); itf.reset_kernel_ms()
for _ in range(50): mpc.evaluate_policy(t, x); mpc.evaluatePolicy(t)
(ms_fb, n_fb), (ms_ff, n_ff) = itf.kernel_ms("policy_fb"), itf.kernel_ms("policy"); itf.set_profiling(0); itf.close()
out["kernel_us_per_launch"] = {"qm_policy_fb_kernel": 1e3 * ms_fb / max(n_fb, 1), "qm_policy_kernel": 1e3 * ms_ff / max(n_ff, 1), "launches": [n_fb, n_ff]}
# (b) loop throughput off / on / off
out["closed_loop_plant_instance_ticks_per_s"] = {k: episode(f, 10, 0, timed=True) for k, f in (("off", False), ("on", True), ("off_again", False))}
# (c) robustness figures
out["robustness"] = {"mpc_every_%d_%s" % (me, "on" if f else "off"): episode(f, me, ticks) for me in (10, 20) for f in (False, True)}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "feedback_policy.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
print(json.dumps(out, indent=1, sort_keys=True))
