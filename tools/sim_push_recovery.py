"""tools/sim_push_recovery.py — how hard can the robot be shoved?  The stance -> trot scenario of tools/sim_robustness.py with scheduled wrenches on the plant
(QMHWSim.set_pushes): per instance one base impulse — a horizontal force of 0.1 s, its direction on a ring of 16, its magnitude on a ladder of 32 (0, 25, ... 775 N) — and
on every second block of 512 instances a steady 15 N downward load on the end effector.  Falls and deviations come from the episode monitor.  Prints, and writes to
profiles/sim_push.json: the largest surviving impulse per direction, the end-effector deviation under load, and the time of a plant step (B = 1024, 1 ms, 2 sub-steps)
without pushes and with K = 1 / K = 8 active slots from the "sim" profiling span.
Usage: python tools/sim_push_recovery.py [ticks] [batch]      |      python tools/sim_push_recovery.py --step-ms   (the step times alone, one JSON line; QM_AB_LIB names
another build of the library on the same box — one without the push calls reports the plain step only)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from qm_control_amd import api
if os.environ.get("QM_AB_LIB"): api.LIB_PATH = os.path.join(ROOT, os.environ["QM_AB_LIB"])
from sim_closed_loop_demo import setup

NDIR, NMAG, DF, T_PUSH, DT_PUSH, LOAD = 16, 32, 25.0, 21.0, 0.1, 15.0


def step_ms(blobs, B=1024, steps=200, warmup=20):
    """ms per plant step from the "sim" span: {"plain", "k1", "k8"} (the pushed ones None on a library without qmhip_sim_set_pushes)"""
    st = blobs[1]; q0 = np.array(st[936:960], float); q0[2] = 0.385; rng = np.random.default_rng(3); q = np.tile(q0, (B, 1)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18))
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf); out = {}
    kp = np.concatenate([np.full(12, 300.0), np.full(6, 20.0)]); kd = np.concatenate([np.full(12, 3.0), np.full(6, 0.5)])
    for name, K in (("plain", 0), ("k1", 1), ("k8", 8)):
        if K and not hasattr(itf.lib, "qmhip_sim_set_pushes"):
            out[name] = None; continue
        if K:
            p = np.zeros((B, K), api.PUSH); p["t_on"] = -np.inf; p["t_off"] = np.inf; p["base_force"][:, :, 0] = 8.0 / K; p["ee_force"][:, :, 2] = -8.0 / K; sim.set_pushes(p)      # every slot active
        sim.reset(q, np.zeros((B, 24)), 0.0); sim.setCommand(q[:, 6:], 0.0, kp, kd, 0.0)
        for _ in range(warmup):
            sim.step(0.001, 2, download=False)
        itf.synchronize(); itf.set_profiling(1); itf.reset_kernel_ms()
        for _ in range(steps):
            sim.step(0.001, 2, download=False)
        itf.synchronize(); ms, n = itf.kernel_ms("sim"); itf.set_profiling(0); assert n == steps, (n, steps)
        s = sim.state(); assert (s["status"] == 0).all() and np.isfinite(s["q"]).all()
        out[name] = ms / n
    itf.close()
    return out


def main():
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 3000; B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    horizon = 1.0; rng = np.random.default_rng(7); c = setup("trot", B, horizon)
    q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; q[:, 6:18] += 0.01 * rng.normal(size=(B, 12))
    i = np.arange(B); d = i % NDIR; m = (i // NDIR) % NMAG; loaded = ((i // (NDIR * NMAG)) % 2) == 1; ang = 2.0 * np.pi * d / NDIR; mag = DF * m
    p = np.zeros((B, 2), api.PUSH); p["t_on"][:, 0] = T_PUSH; p["t_off"][:, 0] = T_PUSH + DT_PUSH; p["base_force"][:, 0, 0] = mag * np.cos(ang); p["base_force"][:, 0, 1] = mag * np.sin(ang)
    p["t_on"][loaded, 1] = -np.inf; p["t_off"][loaded, 1] = np.inf; p["ee_force"][loaded, 1, 2] = -LOAD
    itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True)
    sim.reset(q, np.zeros((B, 24)), 20.0); rbd0, _ = sim.rbd()
    for b in range(B):
        c["ref_x"][b, :, 30:37] = rbd0[b, 48:55]
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset()
    sim.set_pushes(p); sim.monitor(min_base_z=0.3, max_tilt=0.3); sim.reset(q, np.zeros((B, 24)), 20.0)
    t = time.time()
    for _ in range(0, ticks, 100):
        sim.closed_loop(100, 0.001, horizon, n_substeps=2, mpc_every=10)
    ep = sim.episode_summary(); wall = time.time() - t; fell = ep["fall_tick"] >= 0
    print("%d instances x %d ticks in %.2f s; impulse of %.1f s at t = %.1f; fallen %d" % (B, ticks, wall, DT_PUSH, T_PUSH, fell.sum()))
    res = dict(batch=B, ticks=ticks, push_time=T_PUSH, push_duration=DT_PUSH, ee_load_N=LOAD, fallen=int(fell.sum()), directions=[])
    print("direction [deg] | largest surviving impulse [N s], every smaller one surviving too: no load | %g N on the end effector" % LOAD)
    for k in range(NDIR):
        row = dict(deg=360.0 * k / NDIR)
        for name, ld in (("free", False), ("loaded", True)):
            sel = (d == k) & (loaded == ld); order = np.argsort(mag[sel]); f = fell[sel][order]; ms = mag[sel][order]
            n_ok = int(np.argmax(f)) if f.any() else len(f); row[name] = float(ms[n_ok - 1] * DT_PUSH) if n_ok > 0 else None
        res["directions"].append(row); print("  %6.1f | %s | %s" % (row["deg"], row["free"], row["loaded"]))
    up = ~fell; rest = up & (m == 0)
    for name, sel in (("free", rest & ~loaded), ("loaded", rest & loaded), ("free_pushed", up & ~loaded & (m > 0)), ("loaded_pushed", up & loaded & (m > 0))):
        v = ep["max_ee_pos_dev"][sel]; res["ee_dev_mm_" + name] = dict(n=int(sel.sum()), median=float(1e3 * np.median(v)) if sel.any() else None, max=float(1e3 * v.max()) if sel.any() else None)
        print("end-effector deviation from the start pose, %s: %s" % (name, res["ee_dev_mm_" + name]))
    itf.close()
    res["step_ms"] = step_ms((c["mb"], c["st"])); print("plant step [ms], B = 1024, 2 sub-steps:", res["step_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim_push.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    if "--step-ms" in sys.argv:
        from qm_control_amd import scenarios
        print(json.dumps(dict(lib=os.environ.get("QM_AB_LIB", "qm_control_amd/libqmhip.so"), **step_ms(scenarios.load_blobs()))))
    else:
        main()
