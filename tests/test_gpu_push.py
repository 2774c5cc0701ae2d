"""Plant disturbances on the MI355X through the C ABI (qmhip_sim_set_pushes / qmhip_sim_get_push, api.QMHWSim.set_pushes / push_state): the checks of tests/test_push.py
with the same shapes and the same assertions (tests/push_ref.py), the host-carried plant against the device loop, the pipelined loop, one full batch."""
import numpy as np
import pytest

import push_ref as pr
from test_push import check_loop, loop_setup, loop_schedule, N_TICKS, EVERY, HORIZON

pytestmark = pytest.mark.gpu


def test_pushed_plant_vs_reference(blobs, oracle):
    p = pr.DevPlant(blobs, 6); pr.check_plant_vs_reference(p, oracle, "device plant"); p.close()


def test_window_edges_exact(blobs, oracle):
    p = pr.DevPlant(blobs, 4); pr.check_window_edges(p, oracle); p.close()


def test_slot_sum(blobs, oracle):
    pr.check_slot_sum(lambda B: pr.DevPlant(blobs, B), oracle)


def test_isolation_and_off(blobs, oracle):
    pr.check_isolation_and_off(lambda B: pr.DevPlant(blobs, B), oracle, "device plant")


def test_error_codes_leave_the_schedule_untouched(blobs, oracle):
    pr.check_errors(lambda B: pr.DevPlant(blobs, B), oracle)


def test_python_front(blobs, oracle):
    """api.QMHWSim.set_pushes takes [B] as [B][1], None switches off, a refused schedule raises; push_state() returns (wrench, mask)"""
    from qm_control_amd import api
    cases = pr.plant_cases(oracle, pr._ost())[:2]; itf = api.QMInterface(blobs=blobs, max_batch=2, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf)
    p = np.zeros(2, api.PUSH); p["t_off"] = pr.INF; p["base_force"][1] = (1.0, 2.0, 3.0); sim.set_pushes(p)
    sim.reset(pr._arr(cases, "q"), pr._arr(cases, "v"), 1.0); sim.setCommand(*[pr._arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); sim.step(0.001, 2, download=False)
    w, m = sim.push_state(); assert m.tolist() == [1, 1] and np.array_equal(w[1], [1.0, 2.0, 3.0, 0, 0, 0, 0, 0, 0]) and not w[0].any()
    sim.set_pushes(None); sim.step(0.001, 2, download=False); w, m = sim.push_state(); assert not m.any() and not w.any()
    p["t_on"][0] = np.nan
    with pytest.raises(api.QmhipError, match="NaN time"):
        sim.set_pushes(p)
    itf.close()


def test_host_carried_plant_reproduces_closed_loop_sim_with_pushes(blobs):
    """after test_host_carried_plant_reproduces_closed_loop_sim (tests/test_gpu_tick.py): QMHWSim.closed_loop against the same ticks carried by hand — QMController.update,
    sim.setCommand, sim.step — with the same schedule set, bit for bit"""
    from qm_control_amd import api
    from test_gpu_tick import _set_command
    c, q0, t_start = loop_setup(); B = 2; p = loop_schedule(t_start); v0 = np.zeros((B, 24))

    def ctx():
        d = pr.DevPlant(blobs, B, nev=c["ev"].shape[1], nmax=128, c=c); assert d.set_pushes(p) == pr.OK; d.reset(q0, v0, t_start)
        return d
    a = ctx(); ref = []
    for k in range(N_TICKS):
        s = a.closed_loop(1, pr.PERIOD, HORIZON, pr.NSUB, EVERY); assert (s["mpc_status"] >= 0).all() and (s["qp_status"] == 0).all(), k
        ref.append((s["q"], s["v"], a.push_state()[2].copy()))
    a.close()
    b = ctx(); ctl = api.QMController(b.itf, B, 0, 0.0, 0.5, EVERY); ctl.starting(); rbd, contact = b.sim.rbd()
    for k in range(N_TICKS):
        rec = ctl.update(b.sim.state()["time"], rbd, contact, horizon=HORIZON, period=pr.PERIOD); _set_command(b.sim, rec); rbd, contact = b.sim.step(pr.PERIOD, pr.NSUB); s = b.sim.state()
        assert np.array_equal(s["q"], ref[k][0]) and np.array_equal(s["v"], ref[k][1]) and np.array_equal(b.push_state()[2], ref[k][2]), k
    assert [int(r[2][1]) for r in ref] == [2] * 4 + [3] * 11 + [2] * 9 and not any(r[2][0] for r in ref)      # the lateral force over ticks 4-14, the load throughout
    b.close()


def test_pipelined_loop_picks_the_schedule_up(blobs):
    check_loop(lambda c: pr.DevPlant(blobs, 2, nev=c["ev"].shape[1], nmax=128, c=c), True, "device pipelined loop")


def test_full_batch(blobs, oracle):
    """B = 1024, K = QM_SIM_MAX_PUSH, 20 plant steps while standing (the second half of test_command_delay_and_full_batch, tests/test_gpu_sim.py) under random windows and
    base forces of at most 100 N: everything stays finite, status 0, the masks are the numpy expectation"""
    from test_sim import nominal_q, stand_height
    mb, st = blobs; B, K, steps = 1024, pr.KMAX, 20; rng = np.random.default_rng(3); z0 = stand_height(oracle, st)
    q = np.tile(nominal_q(st, z0 - 0.002), (B, 1)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18))
    ts, _ = pr.substep_times(0.0, pr.PERIOD, pr.NSUB, steps); grid = np.concatenate([ts.ravel(), [-pr.INF, pr.INF, 1.0]])      # window ends on the sub-step raster itself, and off it
    p = pr.pushes(B, K); p["t_on"] = rng.choice(grid, (B, K)) + rng.choice([0.0, 1e-4], (B, K)); p["t_off"] = rng.choice(grid, (B, K)) + rng.choice([0.0, 1e-4], (B, K))
    f = rng.normal(size=(B, K, 3)); p["base_force"] = f / np.linalg.norm(f, axis=2, keepdims=True) * rng.uniform(0.0, 100.0 / K, (B, K, 1))      # at most 100 N with every slot open
    d = pr.DevPlant(blobs, B); assert d.set_pushes(p) == pr.OK; d.reset(q, np.zeros((B, 24)), 0.0)
    kp = np.concatenate([np.full(12, 300.0), np.full(6, 20.0)]); kd = np.concatenate([np.full(12, 3.0), np.full(6, 0.5)]); d.command(q[:, 6:], 0.0, kp, kd, 0.0)
    seen = np.zeros(B, np.int64)
    for k in range(steps):
        d.sim.step(pr.PERIOD, pr.NSUB, download=False); rc, w, m = d.push_state(); t = ts[k, -1]
        on = (p["t_on"] <= t) & (t < p["t_off"]); want = (on * (1 << np.arange(K))).sum(axis=1)
        assert rc == pr.OK and np.array_equal(m, want.astype(np.int32)), k
        ww = np.zeros((B, 3))
        for j in range(K):      # ascending slot order from +0.0, inactive slots skipped
            ww = np.where(on[:, j, None], ww + p["base_force"][:, j], ww)
        assert np.array_equal(w[:, 0:3], ww) and not w[:, 3:].any() and np.linalg.norm(ww, axis=1).max() <= 100.0, k
        seen |= want
    s = d.state()
    assert (s["status"] == 0).all() and np.isfinite(s["q"]).all() and np.isfinite(s["v"]).all() and np.isfinite(s["rbd"]).all() and np.isfinite(s["force"]).all()
    assert (seen != 0).sum() > B // 2 and len(set(seen.tolist())) > 50      # most instances were pushed, in many patterns
    d.close()
