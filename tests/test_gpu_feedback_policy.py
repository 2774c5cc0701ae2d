"""Feedback policy on the MI355X through the C ABI (qmhip_policy_eval_feedback, qmhip_mpc_download_feedback, qmhip_closed_loop_sim with ST_FEEDBACK_POLICY) against the
oracle's gains (tests/feedback_ref.py) and the loop built from the oracle's pieces with the numpy linear controller in the tick."""
import numpy as np
import pytest

import feedback_ref as fr
from conftest import assert_blocks, block_errs, rel_err
from qm_control_amd import layout as L

pytestmark = pytest.mark.gpu


def _perturbed(rng, x):
    dx = rng.normal(size=30)
    for sl in (slice(0, 6), slice(6, 12), slice(12, 30)): dx[sl] *= 10.0 ** rng.uniform(-3, -1)
    return x + dx


def _check_against_oracle(mpc, oracle, results, what, rng):
    """results[b]: the oracle's solve of instance b, taken while the oracle still held it, with its gains (K, uff, src).  Gains and biases of qmhip_mpc_download_feedback per
    block within feedback_ref.GAIN_TOL; qmhip_policy_eval_feedback at node times, between them and outside the grid, at states 1e-3 ... 1e-1 off the plan: u_des 1e-6 per block"""
    B = mpc.B; got = mpc.download(); gain, uff = mpc.feedback(); worst = {}; bad = []
    assert (got["status"] == 0).all(), got["status"]
    for b in range(B):
        r = results[b]; n = len(r["t"]); assert got["num_nodes"][b] == n
        assert not gain[b, n:].any() and not uff[b, n:].any()
        for i in range(n):
            for k, v in fr.gain_block_errs(gain[b, i], r["K"][i]).items():
                worst[k] = max(worst.get(k, 0.0), v)
                if not v <= fr.GAIN_TOL: bad.append((b, i, k, v))
            xj = got["x"][b, r["src"][i]]; scale = (np.abs(gain[b, i]) @ np.abs(xj) + np.abs(got["u"][b, i])).max()
            assert (np.abs(uff[b, i] + gain[b, i] @ xj - got["u"][b, i]) <= 1e-12 * scale).all(), (what, b, i)
    print("%s: worst gain block errors vs the oracle %s (bound %.1e)" % (what, {k: "%.2e" % v for k, v in worst.items()}, fr.GAIN_TOL))
    worst_u = {}
    for rnd in range(6):
        t = np.zeros(B); xm = np.zeros((B, 30)); ref = np.zeros((B, 30))
        for b in range(B):
            r = results[b]; n = len(r["t"])
            t[b] = (r["t"][rng.integers(0, n)] if rnd % 2 == 0 else rng.uniform(r["t"][0] - 0.01, r["t"][-1] + 0.01))
            xo, _, _ = _policy_ref(r, t[b]); xm[b] = _perturbed(rng, xo); ref[b] = fr.linear_policy(r, r["K"], r["src"], t[b], xm[b])
        xd, ud, mode = mpc.evaluate_policy(t, xm); xf, uf, mf = mpc.evaluate_policy(t)
        assert np.array_equal(xd, xf) and np.array_equal(mode, mf) and np.abs(ud - uf).max() > 1e-3
        x0, u0, m0 = mpc.evaluatePolicy(t); assert np.array_equal(xf, x0) and np.array_equal(uf, u0) and np.array_equal(mf, m0)      # x == NULL is qmhip_policy_eval
        for k, v in block_errs(ud, ref, "u").items(): worst_u[k] = max(worst_u.get(k, 0.0), v)
    print("%s: worst u_des block errors vs the numpy linear controller on the oracle's gains %s" % (what, {k: "%.2e" % v for k, v in worst_u.items()}))
    assert max(worst_u.values()) <= 1e-6, (what, worst_u)
    assert not bad, "%s: gain blocks above %.1e (instance, node, block, error): %s" % (what, fr.GAIN_TOL, bad[:8])


def _policy_ref(r, t):
    import interp_cases as ic
    x, u = ic.policy_reference(r["t"], r["ev"], r["x"], r["u"], t); return x, u, None


def _oracle_solve(oracle, cfg, b, how, t1=None, x1=None):
    oracle.set_schedule(cfg["ev"][b], cfg["modes"][b]); oracle.set_target(cfg["ref_t"][b], cfg["ref_x"][b]); t0 = float(cfg["t0"][b])
    r = oracle.mpc_step(t0, t0 + cfg["horizon"], cfg["x0"][b])
    if how == "warm": r = oracle.mpc_step(float(t1[b]), float(t1[b]) + cfg["horizon"], x1[b], warm=True)
    if how == "two iterations": r = oracle.mpc_step(t0, t0 + cfg["horizon"], cfg["x0"][b], warm="iterate")
    assert r["warn"] == 0
    r["K"], r["uff"], r["src"] = fr.oracle_gains(oracle, r)
    return r


@pytest.mark.parametrize("name,batch,N", [("C1", 1, 12), ("C2", 1, 30), ("C3", 6, 20), ("C5", 4, 40)])
@pytest.mark.parametrize("how", ["cold", "warm", "two iterations"])
def test_feedback_gains_and_policy_vs_oracle(blobs, oracle, name, batch, N, how):
    """qmhip_mpc_download_feedback and qmhip_policy_eval_feedback after cold, warm and two-iteration solves on C1, C2, a C3 batch and C5.  Measured on the MI355X (worst over
    these cases): gains within 1.8e-12 per block of the oracle's (forces / momentum, C3 cold) where the bound carried over from the CPU pin is 5.6e-12,
    u_des within 2.8e-13 per block of the numpy linear controller (bound 1e-6)"""
    from qm_control_amd import api, scenarios
    rng = np.random.default_rng(17); cfg = scenarios.make_config(name, batch=batch, n_intervals=N); B = batch
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=N + 16, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    if how == "two iterations": itf.set_setting(L.ST_SQP_ITER, 2.0)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    t1 = x1 = None
    if how == "warm":
        t1 = cfg["t0"] + 0.02; x1, _, _ = mpc.evaluatePolicy(t1); x1 = x1 + 1e-3 * rng.normal(size=x1.shape)
        mpc.set_initial(t1, x1); mpc.solve_resident(cfg["horizon"], warm=True)
    results = [_oracle_solve(oracle, cfg, b, how, t1, x1) for b in range(B)]
    _check_against_oracle(mpc, oracle, results, "%s %s" % (name, how), rng)
    itf.close()


def _oracle_feedback_loop(oracle, mb, cfg, q0, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, time0):
    """tests/test_sim.py::_oracle_closed_loop (QMController) with the linear controller in the tick: u_des = the numpy policy on the oracle's gains at the tick's estimated
    centroidal state"""
    from test_sim import centroidal_from_rbd
    old = oracle.set_setting(L.ST_GRID_DT_MIN, L.QM_GRID_DT_MIN_ROBUST)
    try:
        oracle.set_schedule(cfg["ev"][0], cfg["modes"][0]); oracle.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
        oracle.wbc_reset(); oracle.sim_params(); oracle.sim_reset(q0, np.zeros(24), time0); oracle.sim_command(0, 0, 0, 0, 0)
        rbd = oracle.rbd_from_q(q0, np.zeros(24)); time = time0; log = []; pos = np.zeros(18); vel = np.zeros(18); kp = np.zeros(18); kd = np.zeros(18); ff = np.zeros(18)
        for k in range(n_ticks):
            x_est = centroidal_from_rbd(mb, rbd)
            if k % mpc_every == 0:
                r = oracle.mpc_step(time, time + horizon, x_est, warm=(k > 0)); K, _, src = fr.oracle_gains(oracle, r)
            xd, uff, mode = oracle.eval_policy(time); ud = fr.linear_policy(r, K, src, time, x_est)
            if k == 0: oracle.wbc_set_input_last(ud)
            out, wst = oracle.wbc(xd, ud, rbd, mode, period, time)
            if time > 10.0: pos[:12] = xd[12:24]; vel[:12] = ud[12:24]; kp[:12] = 0.0; kd[:12] = 3.0; ff[:12] = out[36:48]
            pos[12:] = xd[24:30]; vel[12:] = 0.0; kp[12:] = arm_kp; kd[12:] = arm_kd; ff[12:] = out[48:54]
            oracle.sim_command(pos, vel, kp, kd, ff); s = oracle.sim_step(period, nsub); rbd = s["rbd"]; time = s["time"]
            log.append(dict(q=s["q"].copy(), v=s["v"].copy(), tau=out[36:].copy(), wbc_status=list(wst), du=float(np.abs(ud - uff).max())))
        return log
    finally:
        oracle.set_setting(L.ST_GRID_DT_MIN, old)


def _device_loop(blobs, c, q0, B, horizon, t_start, n_ticks, feedback, toggle=False):
    from qm_control_amd import api
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True, feedback_policy=feedback)
    if toggle: itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0); itf.set_setting(L.ST_FEEDBACK_POLICY, 0.0)
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset(); sim.reset(np.tile(q0, (B, 1)), np.zeros((B, 24)), t_start)
    dev = []
    for k in range(n_ticks):
        sim.closed_loop(1, 0.001, horizon, n_substeps=2, mpc_every=8); s = sim.state(); out, st3 = wbc.download(B); s["out"] = out; s["tau"] = out[:, 36:]; s["wbc_status"] = st3; s["mpc_status"] = mpc.download()["status"]
        s["u_des"] = itf.debug_read("wbc_u_des", (B, 30)); dev.append(s)
    itf.close()
    return dev


@pytest.mark.parametrize("gait", ["stance", "trot"])
def test_closed_loop_with_the_feedback_policy_vs_oracle(blobs, oracle, gait):
    """qmhip_closed_loop_sim with ST_FEEDBACK_POLICY = 1, 24 ticks, an MPC call every 8 (stance; stance -> trot with the first gait event inside the horizon), against the
    oracle-built loop with the numpy linear controller: the bounds of test_closed_loop_around_the_plant_vs_oracle (tau 1e-5, q 1e-7, v 1e-5).  With the setting off — never
    set, or set and cleared again — every output is bit-equal"""
    import os, sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    mb, st = blobs
    B = 2; horizon = 0.6; t_start = 20.0 if gait == "stance" else 20.3; c = setup(gait, B, horizon, t_start=t_start); n_ticks = 24
    q0 = c["xbar"][6:30].copy(); q0[2] = 0.385
    dev = _device_loop(blobs, c, q0, B, horizon, t_start, n_ticks, True)
    log = _oracle_feedback_loop(oracle, mb, c, q0, n_ticks, 0.001, 2, 8, horizon, 0.0, 0.5, t_start)
    assert max(l["du"] for l in log) > 1e-3                      # the plant drifts off the plan between two solves: the feedback term is not zero
    worst = dict(tau=0.0, q=0.0, v=0.0)
    for k in range(n_ticks):
        assert (dev[k]["mpc_status"] == 0).all() and (dev[k]["wbc_status"] == 0).all() and log[k]["wbc_status"] == [0, 0, 0], k
        for b in range(B):
            for key in worst: worst[key] = max(worst[key], rel_err(dev[k][key][b], log[k][key]))
    print("feedback loop (%s): worst errors vs the oracle loop %s" % (gait, {k: "%.2e" % v for k, v in worst.items()}))
    assert worst["tau"] < 1e-5 and worst["q"] < 1e-7 and worst["v"] < 1e-5, worst
    off = _device_loop(blobs, c, q0, B, horizon, t_start, n_ticks, False); off2 = _device_loop(blobs, c, q0, B, horizon, t_start, n_ticks, False, toggle=True)
    for k in range(n_ticks):
        for key in ("q", "v", "out", "force", "u_des"): assert np.array_equal(off[k][key], off2[k][key]), (k, key)
    assert any(not np.array_equal(off[k]["u_des"], dev[k]["u_des"]) for k in range(n_ticks))


def test_feedback_error_paths(blobs):
    """solver slots 1 and 3, before any solve, with a submit in flight, the pipelined loop with the setting on, a setting other than 0 / 1: errors with a message, never a
    feed-forward answer"""
    from qm_control_amd import api, scenarios
    B = 2; cfg = scenarios.make_config("C3", batch=B, n_intervals=20)
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=40, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); x = cfg["x0"].copy()
    for call in (lambda: mpc.evaluate_policy(cfg["t0"], x), mpc.feedback):
        with pytest.raises(api.QmhipError, match="no policy received yet"): call()
    mpc.solve_resident(cfg["horizon"]); mpc.evaluate_policy(cfg["t0"], x); mpc.feedback()
    for solver in (1.0, 3.0):
        itf.set_setting(L.ST_SOLVER, solver); mpc.solve_resident(cfg["horizon"]); mpc.evaluatePolicy(cfg["t0"])
        for call in (lambda: mpc.evaluate_policy(cfg["t0"], x), mpc.feedback):
            with pytest.raises(api.QmhipError, match="multiple-shooting"): call()
    itf.set_setting(L.ST_SOLVER, 0.0)
    with pytest.raises(api.QmhipError, match="no policy received yet"): mpc.evaluate_policy(cfg["t0"], x)      # a solver switch drops the solution
    mpc.solve_resident(cfg["horizon"])
    mpc.step_submit(cfg["t0"], cfg["x0"], horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"])
    for call in (lambda: mpc.evaluate_policy(cfg["t0"], x), mpc.feedback):
        with pytest.raises(api.QmhipError, match="in flight"): call()
    mpc.step_collect(); mpc.evaluate_policy(cfg["t0"], x)
    with pytest.raises(api.QmhipError): itf.set_setting(L.ST_FEEDBACK_POLICY, 2.0)
    st = blobs[1].copy(); st[L.ST_FEEDBACK_POLICY] = 0.5
    with pytest.raises(api.QmhipError, match="ST_FEEDBACK_POLICY"): api.QMInterface(blobs=(blobs[0], st), max_batch=1, max_nodes=8)
    sim = api.QMHWSim(itf, feedback_policy=True); q = np.tile(np.concatenate([[0, 0, 0.385, 0, 0, 0], blobs[0][L.MB_QNOM:L.MB_QNOM + 18]]), (B, 1)); sim.reset(q, np.zeros((B, 24)), float(cfg["t0"][0]))
    with pytest.raises(api.QmhipError, match="pipelined"): sim.closed_loop(8, 0.001, cfg["horizon"], mpc_every=8, pipelined=True)
    itf.set_setting(L.ST_SOLVER, 1.0)
    with pytest.raises(api.QmhipError, match="multiple-shooting"): sim.closed_loop(1, 0.001, cfg["horizon"], mpc_every=8)
    itf.close()
