"""tools/sim_terrain_tolerance.py — how uneven and how slippery may the floor be before the blind controller falls?  The stance -> trot scenario of tools/sim_robustness.py
on per-robot terrain (QMHWSim.set_terrain): every robot stands on its own random 16 x 16 grid of 0.1 m cells centred under it — heights uniform in +-amplitude, the mean of
the vertices under the footprint (|x| < 0.45 m, |y| < 0.3 m around the base) subtracted, one friction coefficient on the whole grid; beyond the grid the ground continues
at the edge's height — and the instances are spread over a grid of roughness amplitude x friction with batch / 64 robots per cell.  The MPC and the WBC know nothing of the
ground.  Falls come from the episode monitor (base height below 0.3 m absolute, roll or pitch beyond 0.3 rad), which reads the true state.  Prints, and writes to
profiles/sim_terrain.json: per cell the share fallen and the RMS end-effector deviation from the start pose of the survivors (median over the cell), and the time per launch
of the plant kernel without and with terrain (HIP events around every launch of a plant step of the whole batch while standing, alternating rounds in one process, the first
round of each discarded).
Usage: python tools/sim_terrain_tolerance.py [ticks] [batch]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from qm_control_amd import api
from sim_closed_loop_demo import setup

AMPS = [0.0, 0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08]      # [m]
MUS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8, 1.0]
N, CELL = 16, 0.1
KT_ROUNDS, KT_LAUNCHES = 5, 200


def grids(q, rng):
    B = len(q); i = np.arange(B); ai = i % len(AMPS); mi = (i // len(AMPS)) % len(MUS)
    hdr = np.zeros(B, api.TERRAIN); hdr["dx"] = CELL; hdr["dy"] = CELL; hdr["x0"] = q[:, 0] - 0.5 * (N - 1) * CELL; hdr["y0"] = q[:, 1] - 0.5 * (N - 1) * CELL
    H = np.array(AMPS)[ai, None, None] * rng.uniform(-1.0, 1.0, (B, N, N)); c = (np.arange(N) - 0.5 * (N - 1)) * CELL
    under = (np.abs(c)[None, :] < 0.45) & (np.abs(c)[:, None] < 0.3); H -= H[:, under].mean(axis=1)[:, None, None]
    return hdr, H, np.broadcast_to(np.array(MUS)[mi, None, None], (B, N, N)).copy(), ai, mi


def kernel_time(itf, sim, q, terrain):
    """median over the rounds of the mean HIP-event span of one plant launch [us], and all rounds; every round starts from the reset standing pose under a PD command"""
    B = len(q); kp = np.concatenate([np.full(12, 300.0), np.full(6, 20.0)]); kd = np.concatenate([np.full(12, 3.0), np.full(6, 0.5)]); rounds = {"plain": [], "terrain": []}
    for r in range(KT_ROUNDS + 1):
        for name in ("plain", "terrain"):
            sim.set_terrain(*terrain) if name == "terrain" else sim.set_terrain(None)
            sim.reset(q, np.zeros((B, 24)), 0.0); sim.setCommand(q[:, 6:], 0.0, kp, kd, 0.0); itf.set_profiling(1); itf.reset_kernel_ms(); itf.synchronize()
            for _ in range(KT_LAUNCHES):
                sim.step(0.001, 2, download=False)
            itf.synchronize(); ms, n = itf.kernel_ms("sim"); itf.set_profiling(0); assert n == KT_LAUNCHES, n
            if r > 0:
                rounds[name].append(1e3 * ms / n)
    return {k: dict(us_per_launch=v, us_per_launch_median=float(np.median(v))) for k, v in rounds.items()}


def main():
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 3000; B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    horizon = 1.0; rng = np.random.default_rng(7); c = setup("trot", B, horizon)
    q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385; q[:, 6:18] += 0.01 * rng.normal(size=(B, 12))
    hdr, H, MU, ai, mi = grids(q, rng)
    itf = api.QMInterface(blobs=(c["mb"], c["st"]), max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True)
    sim.reset(q, np.zeros((B, 24)), 20.0); rbd0, _ = sim.rbd()
    for b in range(B):
        c["ref_x"][b, :, 30:37] = rbd0[b, 48:55]
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset()
    sim.set_terrain(hdr, H, MU); sim.monitor(0.3, 0.3); sim.reset(q, np.zeros((B, 24)), 20.0); t = time.time()
    for _ in range(0, ticks, 100):
        sim.closed_loop(100, 0.001, horizon, n_substeps=2, mpc_every=10)
    ep = sim.episode_summary(); wall = time.time() - t; fell = ep["fall_tick"] >= 0
    rms = 1e3 * np.sqrt(ep["sum_sq_ee_pos_dev"] / np.maximum(ep["ticks"], 1))
    print("%d instances x %d ticks in %.2f s; %d per cell; fallen %d" % (B, ticks, wall, B // (len(AMPS) * len(MUS)), fell.sum()))
    res = dict(batch=B, ticks=ticks, grid=[N, N], cell_m=CELL, amplitudes_m=AMPS, frictions=MUS, fallen=int(fell.sum()), cells=[])
    print("share fallen | median RMS end-effector deviation of the survivors [mm]; rows: roughness amplitude [mm], columns: friction " + " ".join("%.1f" % m for m in MUS))
    for a, amp in enumerate(AMPS):
        row = []
        for b, mu in enumerate(MUS):
            sel = (ai == a) & (mi == b); up = sel & ~fell
            cell = dict(amplitude_m=amp, friction=mu, n=int(sel.sum()), fallen_share=float(fell[sel].mean()) if sel.any() else None, ee_rms_mm_median=float(np.median(rms[up])) if up.any() else None)
            res["cells"].append(cell); row.append("%.2f|%s" % (cell["fallen_share"], "%.1f" % cell["ee_rms_mm_median"] if up.any() else "-"))
        print("  %5.1f  %s" % (1e3 * amp, "  ".join(row)))
    # ---- what the lookup costs: the plant kernel's time per launch without and with terrain, the whole batch standing on its grids; monitor off ----
    sim.monitor(None); qs = q.copy(); res["kernel_time"] = dict(rounds=KT_ROUNDS, launches_per_round=KT_LAUNCHES, substeps=2, **kernel_time(itf, sim, qs, (hdr, H, MU)))
    kt = res["kernel_time"]; kt["terrain_over_plain"] = kt["terrain"]["us_per_launch_median"] / kt["plain"]["us_per_launch_median"]
    print("plant kernel, us per launch at B = %d: plain %s, terrain %s, ratio of the medians %.3f" % (B, ["%.1f" % x for x in kt["plain"]["us_per_launch"]], ["%.1f" % x for x in kt["terrain"]["us_per_launch"]], kt["terrain_over_plain"]))
    itf.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim_terrain.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
