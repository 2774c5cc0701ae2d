"""tools/episode_monitor_bench.py — what the episode monitor costs: B = 1024 instances, 1000 ticks, an MPC call every 10, two sub-steps, horizon 1.0 (the set-up of
tools/sim_robustness.py), both device loops, monitor off / on without a trace / on with trace_every 10.  Per configuration: ticks/s (wall clock around the loop call, a
synchronisation behind it) from an unprofiled run, and the "episode", "sim", "wbc" kernel ms per tick from a second, profiled run (profiling adds two event records per
launch: its wall clock is not reported).  Writes one JSON object.  The tool also runs on the parent commit's package (no monitor there: only "off" is measured);
--merge FILE... folds such outputs of both into profiles/episode_monitor.json: the parent's run-to-run spread, every configuration of this commit, their ratios to the
parent's median.  Usage: python tools/episode_monitor_bench.py [--out FILE] [--ticks N] [--batch B] [--repeat R] [--label NAME] | --merge FILE... [--out FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

ap = argparse.ArgumentParser(); ap.add_argument("--merge", nargs="+"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_monitor.json")); ap.add_argument("--ticks", type=int, default=1000)
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--repeat", type=int, default=3); ap.add_argument("--label", default="this")
a = ap.parse_args(); B, ticks, horizon = a.batch, a.ticks, 1.0
if a.merge:
    runs = [json.load(open(f)) for f in a.merge]; parent = [r for r in runs if not r["has_monitor"]]; this = [r for r in runs if r["has_monitor"]]; out = dict({k: runs[0][k] for k in ("batch", "ticks", "mpc_every", "n_substeps", "horizon")}, loops={})
    for loop in ("synchronous", "pipelined"):
        pa = [t for r in parent for t in r["loops"][loop]["off"]["ticks_per_s"]]; med = float(np.median(pa)); e = dict(parent=dict(runs=len(parent), ticks_per_s_min=min(pa), ticks_per_s_median=med, ticks_per_s_max=max(pa),
                 kernel_ms_per_tick={k: float(np.median([r["loops"][loop]["off"]["kernel_ms_per_tick"][k] for r in parent])) for k in ("sim", "wbc")}))
        for cfg in ("off", "on", "on_trace10"):
            v = [t for r in this if cfg in r["loops"][loop] for t in r["loops"][loop][cfg]["ticks_per_s"]]; ms = [r["loops"][loop][cfg]["kernel_ms_per_tick"] for r in this if cfg in r["loops"][loop]]
            e[cfg] = dict(runs=len(ms), ticks_per_s_min=min(v), ticks_per_s_median=float(np.median(v)), ticks_per_s_max=max(v), ratio_to_parent_median=float(np.median(v)) / med,
                          kernel_ms_per_tick={k: float(np.median([m[k] for m in ms])) for k in ("episode", "sim", "wbc")})
        out["loops"][loop] = e
    json.dump(out, open(a.out, "w"), indent=1); print(json.dumps(out, indent=1)); sys.exit(0)
from qm_control_amd import api
from sim_closed_loop_demo import setup
has_monitor = hasattr(api.QMHWSim, "monitor")
c = setup("trot", B, horizon); rng = np.random.default_rng(7)
q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; q[:, 6:18] += 0.03 * rng.normal(size=(B, 12)); q[:, 18:] += 0.1 * rng.normal(size=(B, 6))
itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True)


def run(pipelined, monitor, profile):
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset()
    if has_monitor:
        sim.monitor(None) if monitor is None else sim.monitor(0.3, 0.3, *monitor)
    sim.reset(q, np.zeros((B, 24)), 20.0); itf.set_profiling(1 if profile else 0); itf.reset_kernel_ms(); itf.synchronize()
    t = time.perf_counter(); sim.closed_loop(ticks, 0.001, horizon, n_substeps=2, mpc_every=10, pipelined=pipelined); itf.synchronize(); dt = time.perf_counter() - t
    ms = {n: itf.kernel_ms(n) for n in ("episode", "sim", "wbc")} if profile else None; itf.set_profiling(0)
    return dt, ms


configs = [("off", None)] + ([("on", (0, 0)), ("on_trace10", (10, ticks // 10))] if has_monitor else [])
res = dict(label=a.label, batch=B, ticks=ticks, mpc_every=10, n_substeps=2, horizon=horizon, has_monitor=has_monitor, loops={})
run(False, None, False)      # warm-up: first launches, allocations
for pipelined in (False, True):
    loop = {}
    for name, mon in configs:
        walls = [run(pipelined, mon, False)[0] for _ in range(a.repeat)]; _, ms = run(pipelined, mon, True)
        per = {k: (v[0] / ticks if isinstance(v, (tuple, list)) else float(v) / ticks) for k, v in ms.items()}
        loop[name] = dict(ticks_per_s=[ticks / w for w in walls], ticks_per_s_median=float(ticks / np.median(walls)), kernel_ms_per_tick=per)
        print("pipelined" if pipelined else "synchronous", name, "ticks/s", ["%.1f" % (ticks / w) for w in walls], "ms/tick", {k: round(v, 4) for k, v in per.items()}, flush=True)
    res["loops"]["pipelined" if pipelined else "synchronous"] = loop
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(res, open(a.out, "w"), indent=1); print("wrote", a.out)
