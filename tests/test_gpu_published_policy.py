"""Published feedback policy on the MI355X through the C ABI (qmhip_policy_set_publish_window / _publish / _eval_published / _published_info, qmhip_closed_loop_sim_pipelined
with a window): the snapshot against the live records it was taken from, the window's edge, the pipelined loop against the oracle-built loop, the error paths, and the
reference's two-thread layout (tests/c_abi_published.c)."""
import os
import subprocess

import numpy as np
import pytest

import published_ref as pr
from conftest import ROOT, assert_blocks, block_errs, rel_err
from qm_control_amd import layout as L

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "tests", "data")


def _perturbed(rng, x):
    dx = rng.normal(size=x.shape)
    for sl in (slice(0, 6), slice(6, 12), slice(12, 30)): dx[:, sl] *= 10.0 ** rng.uniform(-3, -1, size=(x.shape[0], 1))
    return x + dx


def _queries(rng, mpc, got, n_sets, t_hi=None):
    """(t [B], x [B][30]) sets: node times, times between nodes, outside the grid; states 1e-3 ... 1e-1 off the plan"""
    B = mpc.B; out = []
    for k in range(n_sets):
        t = np.zeros(B)
        for b in range(B):
            n = int(got["num_nodes"][b]); tn = got["t"][b, :n]; hi = tn[-1] if t_hi is None else t_hi[b]
            t[b] = tn[rng.integers(0, n)] if k % 3 == 0 else (rng.uniform(tn[0], hi) if k % 3 == 1 else rng.uniform(tn[0] - 0.01, hi + 0.01))
        xp, _, _ = mpc.evaluatePolicy(t); out.append((t, _perturbed(rng, xp)))
    return out


@pytest.mark.parametrize("name,batch,N", [("C3", 6, 20), ("C2", 1, 30)])
def test_snapshot_survives_the_next_solve(blobs, name, batch, N):
    """solve, record the live feedback policy at six (t, x) sets, publish; then a warm solve from another observation and a qmhip_step_submit left in flight rewrite the stage
    records: qmhip_policy_eval_published still returns the recorded x_des and mode bit for bit and u_des within 1e-13 of the block's largest entry (the allowance for one
    function inlined into two kernels; whether the bits were in fact equal is printed — DESIGN.md section 6).  seq advances by one per publication; a second publication
    hands out the second solution"""
    from qm_control_amd import api, scenarios
    rng = np.random.default_rng(23); cfg = scenarios.make_config(name, batch=batch, n_intervals=N); B = batch
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=N + 16, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0); itf.set_publish_window(N + 16); assert itf.published_info()[:2] == (0, N + 16)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    q1 = _queries(rng, mpc, mpc.download(), 6); rec1 = [mpc.evaluate_policy(t, x) for t, x in q1]; ff1 = [mpc.evaluatePolicy(t) for t, _ in q1]
    mpc.publish_policy()
    t1 = cfg["t0"] + 0.02; x1, _, _ = mpc.evaluatePolicy(t1); x1 = x1 + 1e-2 * rng.normal(size=x1.shape)
    mpc.set_initial(t1, x1); mpc.solve_resident(cfg["horizon"], warm=True)
    assert any(not np.array_equal(mpc.evaluate_policy(t, x)[1], r[1]) for (t, x), r in zip(q1, rec1))      # the live records have moved on
    mpc.step_submit(t1 + 0.01, x1, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"]); assert mpc.steps_in_flight() == 1
    worst = {}; bit_equal = True
    for (t, x), (xd0, ud0, m0), (xf0, uf0, mf0) in zip(q1, rec1, ff1):
        xd, ud, mode, cov, seq = mpc.evaluate_published(t, x)
        assert seq == 1 and (cov == 1).all() and np.array_equal(xd, xd0) and np.array_equal(mode, m0)
        for k, v in block_errs(ud, ud0, "u").items(): worst[k] = max(worst.get(k, 0.0), v)
        bit_equal &= np.array_equal(ud, ud0)
        xf, uf, mf, _, _ = mpc.evaluate_published(t); assert np.array_equal(xf, xf0) and np.array_equal(uf, uf0) and np.array_equal(mf, mf0)      # x == NULL: the feed-forward bits
        assert np.abs(ud - uf).max() > 1e-3
    print("%s: published vs live feedback policy, worst u_des block errors %s, bit-equal: %s" % (name, {k: "%.1e" % v for k, v in worst.items()}, bit_equal))
    assert max(worst.values()) <= 1e-13, worst
    mpc.step_collect()
    mpc.set_initial(t1, x1); mpc.solve_resident(cfg["horizon"], warm=True)      # (the streamed step moved the solution on once more: solve the recorded problem again, warm from another start)
    q3 = _queries(rng, mpc, mpc.download(), 3); rec3 = [mpc.evaluate_policy(t, x) for t, x in q3]
    mpc.publish_policy(); assert itf.published_info()[0] == 2
    mpc.solve_resident(cfg["horizon"], warm=True)
    for (t, x), (xd0, ud0, m0) in zip(q3, rec3):
        xd, ud, mode, cov, seq = mpc.evaluate_published(t, x)
        assert seq == 2 and np.array_equal(xd, xd0) and np.array_equal(mode, m0); assert_blocks(ud, ud0, "u", 1e-13, "second publication")
    mpc.publish_policy(); assert mpc.evaluate_published(q3[0][0], q3[0][1])[4] == 3
    itf.close()


def test_window_edge(blobs):
    """W = 2 on C2: times in the first interval are covered and carry the live feedback values; times behind node 1 are not covered and are array_equal to qmhip_policy_eval"""
    from qm_control_amd import api, scenarios
    rng = np.random.default_rng(5); cfg = scenarios.make_config("C2", batch=1, n_intervals=30)
    itf = api.QMInterface(blobs=blobs, max_batch=1, max_nodes=46, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0); itf.set_publish_window(2)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); mpc.publish_policy()
    got = mpc.download(); n = int(got["num_nodes"][0]); tn = got["t"][0, :n]
    inside = [tn[0], np.nextafter(tn[0], np.inf), 0.5 * (tn[0] + tn[1]), np.nextafter(tn[1], -np.inf), tn[1], tn[0] - 0.01]
    behind = [np.nextafter(tn[1], np.inf), tn[1] + 1e-6, 0.5 * (tn[1] + tn[2]), tn[2], tn[5], tn[-1], tn[-1] + 0.01]
    for t in inside + behind:
        t = np.array([t]); xp, _, _ = mpc.evaluatePolicy(t); x = _perturbed(rng, xp)
        xd, ud, mode, cov, seq = mpc.evaluate_published(t, x); xl, ul, ml = mpc.evaluate_policy(t, x); xf, uf, mf = mpc.evaluatePolicy(t)
        assert np.array_equal(xd, xf) and np.array_equal(mode, mf) and seq == 1
        if any(t[0] == s for s in inside):
            assert cov[0] == 1, t; assert_blocks(ud, ul, "u", 1e-13, "inside the window"); assert np.abs(ud - uf).max() > 1e-3
        else:
            assert cov[0] == 0 and np.array_equal(ud, uf), t
    itf.close()


def _device_loop(blobs, c, q0, B, horizon, t_start, periods, feedback, window):
    from qm_control_amd import api
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=128, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True, feedback_policy=feedback, publish_window=window)
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset(); sim.reset(np.tile(q0, (B, 1)), np.zeros((B, 24)), t_start)
    dev = []
    for p in range(periods):
        sim.closed_loop(8, 0.001, horizon, n_substeps=2, mpc_every=8, pipelined=True); s = sim.state(); out, st3 = wbc.download(B); s["out"] = out; s["tau"] = out[:, 36:]
        s["wbc_status"] = st3; s["mpc_status"] = mpc.download()["status"]; s["u_des"] = itf.debug_read("wbc_u_des", (B, 30)); s["info"] = itf.published_info(B); dev.append(s)
    itf.close()
    return dev


def test_pipelined_loop_with_the_published_feedback_policy_vs_oracle(blobs, oracle):
    """qmhip_closed_loop_sim_pipelined with ST_FEEDBACK_POLICY = 1 and a window of 8 nodes, stance -> trot, 4 periods of 8 ticks, B = 2, against the oracle-built loop with the
    same latency and the numpy linear controller (published_ref.oracle_pipelined_feedback_loop): the bounds of test_gpu_sim.py::test_pipelined_loop_vs_oracle (tau 1e-4,
    q 1e-7, v 1e-4); no tick is uncovered.  With the window on and the setting 0 the loop is bit-equal to the loop without a window"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    mb, st = blobs; B = 2; horizon = 0.6; t_start = 20.3; c = setup("trot", B, horizon, t_start=t_start); q0 = c["xbar"][6:30].copy(); q0[2] = 0.385
    dev = _device_loop(blobs, c, q0, B, horizon, t_start, 4, True, 8)
    log = pr.oracle_pipelined_feedback_loop(oracle, mb, c, q0, 32, 0.001, 2, 8, horizon, 0.0, 0.5, t_start)
    assert max(l["du"] for l in log) > 1e-3 and max(l["node"] for l in log) < 8
    worst = dict(tau=0.0, q=0.0, v=0.0)
    for p in range(4):
        k = 8 * p + 7; seq, window, unc = dev[p]["info"]
        assert (dev[p]["mpc_status"] == 0).all() and (dev[p]["wbc_status"] == 0).all() and log[k]["wbc_status"] == [0, 0, 0], p
        assert seq == p + 1 and window == 8 and (unc == 0).all(), (p, dev[p]["info"])
        for b in range(B):
            for key in worst: worst[key] = max(worst[key], rel_err(dev[p][key][b], log[k][key]))
    print("pipelined feedback loop: worst errors vs the oracle loop %s" % {k: "%.2e" % v for k, v in worst.items()})
    assert worst["tau"] < 1e-4 and worst["q"] < 1e-7 and worst["v"] < 1e-4, worst
    off = _device_loop(blobs, c, q0, B, horizon, t_start, 4, False, None); on = _device_loop(blobs, c, q0, B, horizon, t_start, 4, False, 8)
    for p in range(4):
        for key in ("q", "v", "out", "force", "u_des"): assert np.array_equal(off[p][key], on[p][key]), (p, key)
    assert any(not np.array_equal(off[p]["u_des"], dev[p]["u_des"]) for p in range(4))


def test_published_policy_error_paths(blobs):
    """evaluation / publication before any solve or publication, window 1, a window above max_nodes, solver slots 1 and 3 with the setting on, x on a publication without
    gains, the pipelined loop with the setting on and no window: errors with a message, never a feed-forward answer"""
    from qm_control_amd import api, scenarios
    B = 2; cfg = scenarios.make_config("C3", batch=B, n_intervals=20)
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=40, max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); x = cfg["x0"].copy()
    with pytest.raises(api.QmhipError, match="no publish window"): mpc.publish_policy()
    with pytest.raises(api.QmhipError, match="no policy published yet"): mpc.evaluate_published(cfg["t0"], x)
    for bad in (1, -3, 41):
        with pytest.raises(api.QmhipError, match="window"): itf.set_publish_window(bad)
    itf.set_publish_window(8)
    with pytest.raises(api.QmhipError, match="no policy received yet"): mpc.publish_policy()
    with pytest.raises(api.QmhipError, match="no policy published yet"): mpc.evaluate_published(cfg["t0"], x)
    mpc.solve_resident(cfg["horizon"]); mpc.publish_policy()      # ST_FEEDBACK_POLICY = 0: the primal part only
    xf, uf, mf, cov, seq = mpc.evaluate_published(cfg["t0"]); x0, u0, m0 = mpc.evaluatePolicy(cfg["t0"]); assert seq == 1 and np.array_equal(uf, u0) and np.array_equal(xf, x0) and np.array_equal(mf, m0)
    with pytest.raises(api.QmhipError, match="carries no gains"): mpc.evaluate_published(cfg["t0"], x)
    itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0)
    for solver in (1.0, 3.0):
        itf.set_setting(L.ST_SOLVER, solver); mpc.solve_resident(cfg["horizon"])
        with pytest.raises(api.QmhipError, match="multiple-shooting"): mpc.publish_policy()
    itf.set_setting(L.ST_SOLVER, 0.0)
    with pytest.raises(api.QmhipError, match="no policy received yet"): mpc.publish_policy()      # a solver switch drops the solution
    mpc.solve_resident(cfg["horizon"]); mpc.publish_policy(); assert mpc.evaluate_published(cfg["t0"], x)[4] == 2
    with pytest.raises(api.QmhipError, match="batch size"):
        t1 = cfg["t0"][:1].copy(); itf._check(itf.lib.qmhip_policy_eval_published(itf.h, 1, api._p(t1), None, None, None, None, None, None), "qmhip_policy_eval_published")
    itf.set_publish_window(0)
    with pytest.raises(api.QmhipError, match="no policy published yet"): mpc.evaluate_published(cfg["t0"], x)
    sim = api.QMHWSim(itf); q = np.tile(np.concatenate([[0, 0, 0.385, 0, 0, 0], blobs[0][L.MB_QNOM:L.MB_QNOM + 18]]), (B, 1)); sim.reset(q, np.zeros((B, 24)), float(cfg["t0"][0]))
    with pytest.raises(api.QmhipError, match="pipelined"): sim.closed_loop(8, 0.001, cfg["horizon"], mpc_every=8, pipelined=True)
    itf.set_publish_window(8); itf.set_setting(L.ST_SOLVER, 1.0)
    with pytest.raises(api.QmhipError, match="multiple-shooting"): sim.closed_loop(8, 0.001, cfg["horizon"], mpc_every=8, pipelined=True)
    itf.close()


def test_control_thread_evaluates_beside_the_mpc_thread():
    """tests/c_abi_published.c (B = 1): thread A runs 100 warm solves, each followed by a publication; thread B calls qmhip_policy_eval_published at about 1 kHz with a
    perturbed state.  The same solve sequence replayed single-threaded reproduces every logged answer on the publication with its sequence number bit for bit, and B saw at
    least 20 distinct publications.  Run once, under a time limit"""
    exe = os.path.join(ROOT, "tests", "_build", "c_abi_published"); os.makedirs(os.path.dirname(exe), exist_ok=True); libdir = os.path.join(ROOT, "qm_control_amd")
    subprocess.check_call(["gcc", "-O1", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi_published.c"),
                           "-L" + libdir, "-lqmhip", "-Wl,-rpath," + libdir, "-lm", "-lpthread", "-o", exe])
    p = subprocess.run([exe] + [os.path.join(DATA, f) for f in ("robot.urdf", "task.info", "reference.info")], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    row = [l for l in p.stdout.splitlines() if l.startswith("published:")][0].split(); v = {row[i]: float(row[i + 1]) for i in range(1, len(row), 2)}
    assert v["solves"] == 100 and v["publications"] == 100 and v["mismatches"] == 0 and v["errors"] == 0 and v["distinct_seq"] >= 20 and v["queries"] >= v["distinct_seq"], v
