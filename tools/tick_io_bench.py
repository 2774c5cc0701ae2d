"""Host time of one controller tick for a plant the library does not own — the device plant stepped through the host stands in for an external one — two ways:

  (i)  hand-built from the entry points that existed before the streamed tick: the observation in numpy (computeCentroidalStateFromRbdModel), on MPC ticks
       qmhip_mpc_set_initial + qmhip_mpc_solve_resident_warm, on every tick qmhip_policy_eval + qmhip_wbc_step, updateControlLaw in numpy.  This is the baseline.
  (ii) qmhip_tick_submit + qmhip_tick_collect (api.QMController.update).

B = 1 and B = 1024, mpc_every 5, QMController's law (controller 0), trot.  Timed: the controller's part of every tick (the plant's step and its hand-over are common to both
and outside the clock); warm-up ticks excluded; both paths run the same episode from the same reset on contexts of their own.  Reported per path: ticks/s (of the whole
batch), mean / max host time per tick, the same split into ticks with and without an MPC call.  Writes profiles/tick_io.json (or --out).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
from qm_control_amd import api, record_model, scenarios      # noqa: E402
from sim_closed_loop_demo import setup                        # noqa: E402

PERIOD, NSUB, HORIZON, MPC_EVERY, T_START = 0.002, 2, 1.0, 5, 20.0


def _rot_zyx(z, y, x):
    cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
    return np.stack([np.stack([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx], -1), np.stack([sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], -1), np.stack([-sy, cy * sx, cy * cx], -1)], -2)


def observe_numpy(mb, rbd):
    """computeCentroidalStateFromRbdModel for a batch, vectorised (what a caller without the library's observation has to write)"""
    R = _rot_zyx(rbd[:, 0], rbd[:, 1], rbd[:, 2]); Inom = mb[scenarios.MB_INOM:scenarios.MB_INOM + 9].reshape(3, 3); rnom = mb[scenarios.MB_RNOM:scenarios.MB_RNOM + 3]; m = mb[scenarios.MB_ROBOTMASS]
    w = rbd[:, 24:27]; x = np.zeros((len(rbd), 30))
    x[:, 0:3] = rbd[:, 27:30] + np.cross(R @ rnom, w); x[:, 3:6] = np.einsum("bij,jk,blk,bl->bi", R, Inom, R, w) / m; x[:, 6:9] = rbd[:, 3:6]; x[:, 9:12] = rbd[:, 0:3]; x[:, 12:30] = rbd[:, 6:24]
    return x


class Episode:
    def __init__(self, B):
        self.B = B; c = self.c = setup("trot", B, HORIZON, t_start=T_START)
        self.itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
        self.mpc = api.SqpMpc(self.itf); self.wbc = api.HierarchicalWbc(self.itf); self.sim = api.QMHWSim(self.itf, robust_grid=True)
        self.mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); self.wbc.reset()
        q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; self.sim.reset(q, np.zeros((B, 24)), T_START)
        self.rbd, self.contact = self.sim.rbd(); self.time = self.sim.state()["time"]; self.ok = True

    def plant(self, cmd):
        self.sim.setCommand(*[np.ascontiguousarray(cmd[:, i]) for i in range(5)]); self.rbd, self.contact = self.sim.step(PERIOD, NSUB); self.time = self.time + PERIOD

    def close(self):
        self.itf.close()


def run_hand_built(B, ticks, warmup):
    e = Episode(B); mb = e.c["mb"]; cmd = np.zeros((B, 5, 18)); dt = []
    for k in range(warmup + ticks):
        t = time.perf_counter()
        if k % MPC_EVERY == 0:
            e.mpc.set_initial(e.time, observe_numpy(mb, e.rbd)); e.mpc.solve_resident(HORIZON, warm=True)
        xd, ud, mode = e.mpc.evaluatePolicy(e.time)
        if k == 0:
            e.wbc.reset()      # (inputLast_ cannot be primed with the planned input from the host: no entry point sets it)
        out, qps = e.wbc.update(xd, ud, e.rbd, mode, PERIOD, e.time)
        legs = e.time > 10.0
        cmd[legs, 0, :12] = xd[legs, 12:24]; cmd[legs, 1, :12] = ud[legs, 12:24]; cmd[legs, 2, :12] = 0.0; cmd[legs, 3, :12] = 3.0; cmd[legs, 4, :12] = out[legs, 36:48]
        cmd[:, 0, 12:] = xd[:, 24:30]; cmd[:, 1, 12:] = 0.0; cmd[:, 2, 12:] = 0.0; cmd[:, 3, 12:] = 0.5; cmd[:, 4, 12:] = out[:, 48:54]
        dt.append(time.perf_counter() - t); e.ok = e.ok and bool((qps == 0).all())
        e.plant(cmd)
    e.ok = e.ok and bool((e.mpc.download()["status"] >= 0).all()) and bool(np.isfinite(e.rbd).all()); ok = e.ok; e.close()
    return np.array(dt[warmup:]), ok


def run_streamed(B, ticks, warmup):
    e = Episode(B); ctl = api.QMController(e.itf, B, 0, 0.0, 0.5, MPC_EVERY); ctl.starting(); dt = []
    for k in range(warmup + ticks):
        t = time.perf_counter()
        rec = ctl.update(e.time, e.rbd, e.contact, horizon=HORIZON, period=PERIOD)
        dt.append(time.perf_counter() - t); e.ok = e.ok and bool((rec["qp_status"] == 0).all() and (rec["mpc_status"] >= 0).all())
        e.plant(rec["cmd"].reshape(B, 5, 18))
    ok = e.ok and bool(np.isfinite(e.rbd).all()); e.close()
    return np.array(dt[warmup:]), ok


def stats(dt, B, warmup):
    k = (np.arange(len(dt)) + warmup) % MPC_EVERY == 0
    f = lambda a: {"mean_ms": float(a.mean()) * 1e3, "max_ms": float(a.max()) * 1e3, "median_ms": float(np.median(a)) * 1e3, "ticks": int(a.size)}
    return dict(f(dt), ticks_per_s=float(len(dt) / dt.sum()), instance_ticks_per_s=float(B * len(dt) / dt.sum()), mpc_ticks=f(dt[k]), other_ticks=f(dt[~k]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ticks", type=int, default=200); ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024]); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tick_io.json"))
    a = ap.parse_args(); assert a.warmup % MPC_EVERY == 0
    res = {"tool": "tools/tick_io_bench.py", "kernel_source_hash": record_model.kernel_source_hash(), "unit": "host wall clock of the controller's part of one tick of the whole batch",
           "mpc_every": MPC_EVERY, "period": PERIOD, "horizon": HORIZON, "gait": "trot", "ticks": a.ticks, "warmup_ticks": a.warmup, "repetitions": a.reps,
           "paths": {"i_hand_built": "numpy observation + qmhip_mpc_set_initial + qmhip_mpc_solve_resident_warm (MPC ticks) + qmhip_policy_eval + qmhip_wbc_step + numpy control law (baseline)",
                     "ii_streamed": "qmhip_tick_submit + qmhip_tick_collect"}}
    for B in a.batches:
        runs = {"i_hand_built": [], "ii_streamed": []}; ok = True
        for _ in range(a.reps):      # the paths alternate inside every repetition; the repetition with the smaller mean is reported, all means are listed
            for name, fn in (("i_hand_built", run_hand_built), ("ii_streamed", run_streamed)):
                dt, good = fn(B, a.ticks, a.warmup); runs[name].append(dt); ok = ok and good
        out = {"all_status_ok": ok}
        for name, v in runs.items():
            best = min(v, key=lambda d: d.mean()); out[name] = dict(stats(best, B, a.warmup), mean_ms_all_repetitions=[float(d.mean()) * 1e3 for d in v])
        out["ii_over_i_mean_time"] = out["ii_streamed"]["mean_ms"] / out["i_hand_built"]["mean_ms"]; out["ii_not_slower_than_i"] = out["ii_over_i_mean_time"] <= 1.0
        res["B%d" % B] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: {"i_mean_ms": round(v["i_hand_built"]["mean_ms"], 4), "ii_mean_ms": round(v["ii_streamed"]["mean_ms"], 4), "i_max_ms": round(v["i_hand_built"]["max_ms"], 4), "ii_max_ms": round(v["ii_streamed"]["max_ms"], 4),
                          "ratio": round(v["ii_over_i_mean_time"], 4), "ok": v["all_status_ok"]} for k, v in res.items() if k.startswith("B")}))


if __name__ == "__main__":
    main()
