"""Host-visible rate of a control step whose observation comes from host memory and whose results go back to it — the workload of bench.py's `pcie_inclusive` leg
(C4 shard 0, B = 1024, N = 100) and one robot (C2, B = 1), same process, same context per batch size, three hand-overs:

  (a) old      qmhip_mpc_set_initial + qmhip_closed_loop_resident(n_steps 1) + qmhip_mpc_download + qmhip_wbc_download: the synchronous copies of the C ABI
  (b) depth 1  qmhip_step_submit + qmhip_step_collect back to back
  (c) depth 2  step k + 1 submitted before step k is collected (the record of step k travels while step k + 1 computes)

(b) and (c) are taken twice: with the record only (QMHIP_STEP_WBC: what a control loop needs, 1 KB per instance) and with the primal solution as well (| QMHIP_STEP_TRAJ:
everything (a) moves).  Every step is the same warm-started solve on the same observation, so the three legs do identical device work.

Method: warm-up excluded; wall clock around a loop that ends with the last collect (or download); the legs alternate inside every repetition, >= 3 repetitions, min / median /
max over them reported.  B = 1 additionally: the wall time of every call of one long loop per leg — p50 / p99 / max, call 0 listed separately.
Writes profiles/step_io.json (or --out).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qm_control_amd import api, record_model, scenarios      # noqa: E402


def _commit():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return os.environ.get("QM_COMMIT")      # a tree copied without its history: the caller names the commit it was taken from


class Legs:
    def __init__(self, cfg, max_nodes):
        self.cfg = cfg; self.B = cfg["B"]
        self.itf = api.QMInterface(blobs=scenarios.load_blobs(), max_batch=self.B, max_nodes=max_nodes, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1])
        self.mpc = api.SqpMpc(self.itf); self.wbc = api.HierarchicalWbc(self.itf)
        self.mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); self.wbc.reset()
        self.kw = dict(horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"])
        self.ok = True

    def _check(self, status, qps):
        self.ok = self.ok and bool((status >= 0).all() and (qps == 0).all())

    def old(self, n, per_call=None):
        c = self.cfg
        for _ in range(n):
            t = time.perf_counter()
            self.mpc.set_initial(c["t0"], c["x0"]); self.mpc.closed_loop_resident(1, 0.01, c["horizon"], c["period"], c["time"])
            r = self.mpc.download(); out, qps = self.wbc.download(self.B)
            if per_call is not None:
                per_call.append(time.perf_counter() - t)
        self._check(r["status"], qps)

    def depth1(self, n, flags, per_call=None):
        c = self.cfg
        for _ in range(n):
            t = time.perf_counter()
            self.mpc.step_submit(c["t0"], c["x0"], None, flags=flags, **self.kw); r = self.mpc.step_collect()
            if per_call is not None:
                per_call.append(time.perf_counter() - t)
        self._check(r["status"], r["qp_status"])

    def depth2(self, n, flags, per_call=None):
        c = self.cfg
        self.mpc.step_submit(c["t0"], c["x0"], None, flags=flags, **self.kw)
        for k in range(n):
            t = time.perf_counter()
            if k + 1 < n:
                self.mpc.step_submit(c["t0"], c["x0"], None, flags=flags, **self.kw)
            r = self.mpc.step_collect()
            if per_call is not None:
                per_call.append(time.perf_counter() - t)
        self._check(r["status"], r["qp_status"])


def measure(cfg, max_nodes, steps, reps, warmup, per_call_n=0):
    L = Legs(cfg, max_nodes); B = L.B; W, WT = api.STEP_WBC, api.STEP_WBC | api.STEP_TRAJ
    legs = [("a_old", lambda n, pc=None: L.old(n, pc)), ("b_depth1", lambda n, pc=None: L.depth1(n, W, pc)), ("c_depth2", lambda n, pc=None: L.depth2(n, W, pc)),
            ("b_depth1_traj", lambda n, pc=None: L.depth1(n, WT, pc)), ("c_depth2_traj", lambda n, pc=None: L.depth2(n, WT, pc))]
    for _, f in legs:
        f(warmup)
    L.itf.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, f in legs:
            L.itf.synchronize(); t = time.perf_counter(); f(steps); times[name].append((time.perf_counter() - t) / steps)
    # the resident rate of the same step on the same context, for scale: nothing crosses the boundary, one synchronisation at the end
    L.itf.synchronize(); t = time.perf_counter(); L.mpc.closed_loop_resident(steps, 0.0, cfg["horizon"], cfg["period"], cfg["time"]); L.itf.synchronize(); resident = (time.perf_counter() - t) / steps
    out = {"B": B, "max_nodes": max_nodes, "steps_per_repetition": steps, "repetitions": reps, "warmup_steps_per_leg": warmup, "all_status_ok": None, "legs": {},
           "resident_same_context": {"ms_per_step": resident * 1e3, "steps_per_s": B / resident, "note": "qmhip_closed_loop_resident(n_steps) with a zero advance: no host data movement"}}
    for name, _ in legs:
        v = np.array(times[name]); med = float(np.median(v))
        out["legs"][name] = {"ms_per_step": med * 1e3, "steps_per_s": B / med, "ms_per_step_min": float(v.min()) * 1e3, "ms_per_step_max": float(v.max()) * 1e3, "ms_per_step_all": [float(x) * 1e3 for x in v]}
    if per_call_n:
        for name, f in legs:
            pc = []; L.itf.synchronize(); f(per_call_n, pc); a = np.array(pc[1:]) * 1e3
            out["legs"][name]["per_call_ms"] = {"calls": per_call_n, "call_0": pc[0] * 1e3, "p50": float(np.percentile(a, 50)), "p99": float(np.percentile(a, 99)), "max": float(a.max()),
                                                "note": "call 0 of the loop apart; depth 2: one call = submit of step k + 1 and collect of step k"}
    g = out["legs"]; out["all_status_ok"] = L.ok
    out["gate"] = {"b_not_slower_than_a": g["b_depth1"]["ms_per_step"] <= g["a_old"]["ms_per_step"], "c_not_slower_than_b": g["c_depth2"]["ms_per_step"] <= g["b_depth1"]["ms_per_step"],
                   "b_traj_not_slower_than_a": g["b_depth1_traj"]["ms_per_step"] <= g["a_old"]["ms_per_step"], "c_traj_not_slower_than_b_traj": g["c_depth2_traj"]["ms_per_step"] <= g["b_depth1_traj"]["ms_per_step"],
                   "c_over_resident": resident / (g["c_depth2"]["ms_per_step"] * 1e-3)}
    L.itf.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--n-intervals", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls-b1", type=int, default=400); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_io.json"))
    a = ap.parse_args()
    assert a.steps >= 2 and a.reps >= 1
    res = {"tool": "tools/step_io_bench.py", "commit": _commit(), "kernel_source_hash": record_model.kernel_source_hash(), "unit": "ms per control step of the whole batch, host wall clock; steps_per_s = B / that",
           "record_bytes_per_instance": api.STEP_RECORD.itemsize, "input_bytes_per_instance": 8 * 31}
    res["B%d" % a.batch] = dict(measure(scenarios.make_config("C4", batch=a.batch, n_intervals=a.n_intervals), a.n_intervals + 28, a.steps, a.reps, a.warmup),
                                 workload="C4 shard 0: trot, N = %d, %d instances (bench.py's pcie_inclusive workload)" % (a.n_intervals, a.batch))
    res["B1"] = dict(measure(scenarios.make_config("C2"), 128, max(a.steps, 100), a.reps, a.warmup, per_call_n=a.calls_b1), workload="C2: one robot, trot, N = 100")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: ({n: round(v["ms_per_step"], 4) for n, v in res[k]["legs"].items()}, res[k]["gate"], res[k]["all_status_ok"]) for k in res if k.startswith("B")}))


if __name__ == "__main__":
    main()
