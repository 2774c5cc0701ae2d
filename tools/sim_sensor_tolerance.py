"""tools/sim_sensor_tolerance.py — how bad may the state estimate get before the controller falls over?  The stance -> trot scenario of tools/sim_robustness.py with the
sensor model between the plant and the controller (QMHWSim.set_sensors): the instances are spread over a grid of noise scale x latency — sigma = scale x (2e-3 rad base
angles, 2e-3 m base position, 1e-3 rad joints, 2e-2 rad/s base angular velocity, 2e-2 m/s base linear velocity, 5e-2 rad/s joint rates), bias_sigma = sigma / 2, lag in whole
1 ms samples — with batch / 64 seeds per cell.  Falls and end-effector deviations come from the episode monitor, which reads the TRUE state.  Prints, and writes to
profiles/sim_sensor.json: per cell the share fallen and the RMS end-effector deviation from the start pose of the survivors (median over the cell), and an A/B of the tick
time of both device loops (wall clock around one loop call as tools/episode_monitor_bench.py takes it, plus the "sense" / "sim" / "wbc" spans of a profiled run) with the
model off, on with identity records (the kernel's own cost: the controller sees the same bits) and on with noise (what the noisy state costs the controller on top).
Usage: python tools/sim_sensor_tolerance.py [ticks] [batch]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from qm_control_amd import api
from sim_closed_loop_demo import setup

SIGMA = np.array([2e-3, 2e-3, 1e-3, 2e-2, 2e-2, 5e-2])
SCALES = [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0]
LAGS = [0, 1, 2, 3, 4, 5, 6, 8]
AB_TICKS, AB_REPEAT = 1000, 3


def records(B, rng):
    i = np.arange(B); si = i % len(SCALES); li = (i // len(SCALES)) % len(LAGS)
    s = np.zeros(B, api.SENSOR); s["seed"] = rng.integers(0, 2 ** 64, B, dtype=np.uint64); s["lag"] = np.array(LAGS)[li]
    s["sigma"] = np.array(SCALES)[si, None] * SIGMA[None, :]; s["bias_sigma"] = 0.5 * s["sigma"]
    return s, si, li


def main():
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 3000; B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    horizon = 1.0; rng = np.random.default_rng(7); c = setup("trot", B, horizon)
    q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; q[:, 6:18] += 0.01 * rng.normal(size=(B, 12))
    s, si, li = records(B, rng)
    itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True)
    sim.reset(q, np.zeros((B, 24)), 20.0); rbd0, _ = sim.rbd()
    for b in range(B):
        c["ref_x"][b, :, 30:37] = rbd0[b, 48:55]

    def start(sensors, monitor):
        mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset()
        sim.set_sensors(sensors); sim.monitor(0.3, 0.3) if monitor else sim.monitor(None); sim.reset(q, np.zeros((B, 24)), 20.0)

    start(s, True); t = time.time()
    for _ in range(0, ticks, 100):
        sim.closed_loop(100, 0.001, horizon, n_substeps=2, mpc_every=10)
    ep = sim.episode_summary(); wall = time.time() - t; fell = ep["fall_tick"] >= 0; _, n = sim.measured(); assert (n == ticks).all()
    rms = 1e3 * np.sqrt(ep["sum_sq_ee_pos_dev"] / np.maximum(ep["ticks"], 1))
    print("%d instances x %d ticks in %.2f s; %d per cell; fallen %d" % (B, ticks, wall, B // (len(SCALES) * len(LAGS)), fell.sum()))
    res = dict(batch=B, ticks=ticks, sigma_unit=SIGMA.tolist(), bias_over_sigma=0.5, scales=SCALES, lags=LAGS, fallen=int(fell.sum()), cells=[])
    print("share fallen | median RMS end-effector deviation of the survivors [mm]; rows: noise scale, columns: lag " + " ".join("%d" % l for l in LAGS))
    for a, sc in enumerate(SCALES):
        row = []
        for b, lag in enumerate(LAGS):
            sel = (si == a) & (li == b); up = sel & ~fell
            cell = dict(scale=sc, lag=lag, n=int(sel.sum()), fallen_share=float(fell[sel].mean()) if sel.any() else None, ee_rms_mm_median=float(np.median(rms[up])) if up.any() else None)
            res["cells"].append(cell); row.append("%.2f|%s" % (cell["fallen_share"], "%.1f" % cell["ee_rms_mm_median"] if up.any() else "-"))
        print("  %5.2f  %s" % (sc, "  ".join(row)))
    # ---- what the sensor kernel costs: the tick time with the model off, on with identity records, on with scale 1 and lag 2 on every instance; monitor off ----
    one = np.zeros(B, api.SENSOR); one["seed"] = s["seed"]; one["lag"] = 2; one["sigma"] = SIGMA; one["bias_sigma"] = 0.5 * SIGMA; res["tick_ab"] = dict(ticks=AB_TICKS, repeat=AB_REPEAT, loops={})
    for pipelined in (False, True):
        loop = {}
        for name, sensors in (("off", None), ("identity", np.zeros(B, api.SENSOR)), ("on", one)):
            walls = []
            for r in range(AB_REPEAT + 2):      # run 0 warms up, the last one is profiled (two event records per launch: its wall clock is not reported)
                prof = r == AB_REPEAT + 1; start(sensors, False); itf.set_profiling(1 if prof else 0); itf.reset_kernel_ms(); itf.synchronize()
                t = time.perf_counter(); sim.closed_loop(AB_TICKS, 0.001, horizon, n_substeps=2, mpc_every=10, pipelined=pipelined); itf.synchronize(); dt = time.perf_counter() - t
                if 0 < r <= AB_REPEAT:
                    walls.append(dt)
            ms = {k: itf.kernel_ms(k)[0] / AB_TICKS for k in ("sense", "sim", "wbc")}; itf.set_profiling(0)
            loop[name] = dict(ticks_per_s=[AB_TICKS / w for w in walls], ticks_per_s_median=float(AB_TICKS / np.median(walls)), kernel_ms_per_tick=ms)
            print("pipelined" if pipelined else "synchronous", name, "ticks/s", ["%.1f" % (AB_TICKS / w) for w in walls], "ms/tick", {k: round(v, 4) for k, v in ms.items()}, flush=True)
        loop["identity_over_off"] = loop["identity"]["ticks_per_s_median"] / loop["off"]["ticks_per_s_median"]; loop["on_over_off"] = loop["on"]["ticks_per_s_median"] / loop["off"]["ticks_per_s_median"]; res["tick_ab"]["loops"]["pipelined" if pipelined else "synchronous"] = loop
    itf.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim_sensor.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
