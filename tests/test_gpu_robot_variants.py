"""Every kernel on perturbed robots (tests/robot_variants.py) on the MI355X.  The robot comes from FILES — api.QMInterface(task.info, the variant's URDF, reference.info) —
so the product's own ingestion runs on the GPU machine too, and its blobs are asserted bit-equal to robot_variants.blobs(name) first.  Then what tests/test_robot_variants.py
pins on the host emulator, on the device: the FAST sincos instances, the LDS / MFMA fragment layouts of K1b and K3, the workspace placements.  Every tolerance is the one
the project states for the same quantity on the shipped robot; shapes are the smallest that reach every code path; the worst error per block is printed."""
import numpy as np
import pytest

import lq_record_check as LC
import robot_variants as rv
from conftest import assert_blocks
from blocks import block_errs
from qm_control_amd import layout as L
from test_robot_variants import config, oracle_solve, check_plant, rollout_rows

pytestmark = pytest.mark.gpu
TOL = 1e-6
HEAVY = ("skew", "strong")


def interface(name, **kw):
    """a device context built from the variant's files; its blobs are the ones the CPU tests ran on, bit for bit"""
    from qm_control_amd import api
    itf = api.QMInterface(rv.TASK, rv.urdf(name), rv.REFI, **kw)
    mb, st = rv.blobs(name)
    assert np.array_equal(itf.model_blob, mb) and np.array_equal(itf.settings_blob, st)
    return itf


@pytest.mark.parametrize("cname,N", [("C2", 26), ("C1", 10)])
@pytest.mark.parametrize("name", HEAVY)
def test_lq_and_stage_records_entrywise(name, cname, N):
    """test_gpu_lq_records on the variant at small shapes: lq_debug 1, riccati_skip 20 then 0, <= 1e-10 per block.  C1: the m = 18 stance path, two tile rows, the lq_m18
    instance; C2: swing legs, whose 3 x 2 null-space blocks depend on the now general foot Jacobian.  The product instances return the debug instances' solution"""
    from qm_control_amd import api
    from test_gpu_mpc import _compare
    o = rv.oracle(name); cfg = config(cname, 1, N)
    r = oracle_solve(o, cfg); n = len(r["t"]); nm = n + 3; assert r["warn"] == 0
    itf = interface(name, max_batch=1, max_nodes=nm, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    itf.debug_set("lq_debug", 1); assert itf.debug_get("lq_debug") == 1
    SRN, DBN = LC.SR["SR_SIZE"], LC.DBG["LQ_DBG_SIZE"]; recs = {}
    for skip in (20, 0):
        itf.debug_set("riccati_skip", skip)
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
        recs[skip] = (itf.debug_read("stage", (nm, SRN)), itf.debug_read("lqdbg", (nm, DBN)), int(itf.debug_read("n_nodes", (1,), np.int32)[0]))
    itf.debug_set("riccati_skip", 0); itf.debug_set("lq_debug", 0); assert itf.debug_get("lq_debug") == 0
    res_dbg = mpc.download()
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); res = mpc.download()
    itf.close()
    for skip in (20, 0):
        stage, dbg, nn = recs[skip]; assert nn == n; worst = {}
        for i in range(n - 1):
            if r["ev"][i] == 1:
                continue
            for k, v in LC.check_interval(stage[i], dbg[i], o.node_lq(i), o.node_proj(i), after_riccati=(skip == 0)).items():
                worst[k] = max(worst.get(k, 0.0), v)
        print(name, cname, "riccati_skip", skip, {k: "%.1e" % v for k, v in worst.items()})
        bad = {k: v for k, v in worst.items() if not v <= 1e-10}
        assert not bad, (name, cname, skip, bad, worst)
    _compare(res_dbg, 0, r)
    assert np.array_equal(res["x"], res_dbg["x"]) and np.array_equal(res["u"], res_dbg["u"])


@pytest.mark.parametrize("cname,B,N", [("C3", 4, 20), ("C5", 2, 30), ("gait:dynamic_walk", 4, 30)])
@pytest.mark.parametrize("name", HEAVY)
def test_whole_control_step(name, cname, B, N):
    """control_step_resident — MPC iteration, policy at t0, WBC — against pyoracle.batch_step: 1e-6 per block, all statuses 0.  dynamic_walk: three-leg support (m = 17)"""
    import pyoracle
    from qm_control_amd import api
    cfg = config(cname, B, N)
    itf = interface(name, max_batch=B, max_nodes=N + 28, max_ref_knots=2, max_events=cfg["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); wbc.reset()
    mpc.control_step_resident(cfg["horizon"], cfg["period"], cfg["time"])
    out, st = wbc.download(B); res = mpc.download(); xp, up, _ = mpc.evaluatePolicy(cfg["t0"])
    itf.close()
    bad, xf, uf, w = pyoracle.batch_step(*rv.oracle_blobs(name), 2, cfg["t0"], cfg["horizon"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"], cfg["period"], cfg["time"])
    assert bad == 0                                                                   # gate
    assert (res["status"] == 0).all() and (st == 0).all(), (res["status"], st)
    assert np.array_equal(res["x"][:, 0], cfg["x0"]) and np.abs(res["u"][:, 0, 12:]).max() > 1e-6
    errs = {}
    for b in range(B):
        for what, got, ref, kind in (("wbc", out[b], w[b], "wbc"), ("policy u", res["u"][b, 0], uf[b], "u"), ("policy x", xp[b], xf[b], "x"), ("policy u (eval)", up[b], uf[b], "u")):
            for k, v in block_errs(got, ref, kind).items(): errs[what + " " + k] = max(errs.get(what + " " + k, 0.0), v)
    print(name, cname, {k: "%.1e" % v for k, v in errs.items()})
    for b in range(B):
        assert_blocks(out[b], w[b], "wbc", TOL, b); assert_blocks(res["u"][b, 0], uf[b], "u", TOL, b); assert_blocks(xp[b], xf[b], "x", TOL, b); assert_blocks(up[b], uf[b], "u", TOL, b)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", HEAVY)
def test_wbc_alone(name, variant):
    """wbc_cases.random_wbc_inputs (12) and hard_wbc_inputs (8), the cases of the emulator test: statuses equal to the oracle's [0, 0, 0], 1e-6 per block"""
    from qm_control_amd import api
    from wbc_cases import random_wbc_inputs, hard_wbc_inputs
    o = rv.oracle(name); bl = rv.blobs(name)
    itf = interface(name, max_batch=12, max_nodes=8, max_ref_knots=2, max_events=2); wbc = api.HierarchicalWbc(itf, mpc_variant=bool(variant))
    sets = (("random", random_wbc_inputs(o, bl, 12, 31 + variant, 0.05)), ("hard", hard_wbc_inputs(o, bl, 8, 131 + variant))); got = []
    for what, cases in sets:
        arr = lambda k: np.array([c[k] for c in cases])
        wbc.reset(); wbc.update(arr("xd"), arr("il"), arr("rbd"), arr("mode"), 0.002, arr("time"))       # primes inputLast_
        got.append(wbc.update(arr("xd"), arr("ud"), arr("rbd"), arr("mode"), 0.002, arr("time")))
    itf.close()
    for (what, cases), (out, st) in zip(sets, got):
        errs = {}
        for b, c in enumerate(cases):
            o.wbc_reset(); o.wbc(c["xd"], c["il"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant))
            ref, sto = o.wbc(c["xd"], c["ud"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant))
            assert list(sto) == [0, 0, 0], (what, b, sto)                              # gate
            assert list(st[b]) == list(sto), (what, b, st[b])
            for k, v in block_errs(out[b], ref, "wbc").items(): errs[k] = max(errs.get(k, 0.0), v)
            assert_blocks(out[b], ref, "wbc", TOL, (what, b))
        print(name, "variant", variant, what, {k: "%.1e" % v for k, v in errs.items()})


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name", HEAVY)
def test_plant(name, nsub):
    """test_gpu_sim.test_plant_vs_oracle on the variant: 4 cases x 12 steps, the same bounds (q 1e-9, v 1e-7, forces 1e-6, rbd 1e-7, time 1e-12, contact flags equal)"""
    from qm_control_amd import api
    from test_sim import random_cases
    o = rv.oracle(name); mb, st = rv.blobs(name)
    cases = random_cases(o, st, 4, 5); arr = lambda k: np.array([c[k] for c in cases])
    itf = interface(name, max_batch=4, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf)
    sim.reset(arr("q"), arr("v"), 1.0); sim.setCommand(arr("pos"), arr("vel"), arr("kp"), arr("kd"), arr("ff"))
    steps = 12; out = []
    for _ in range(steps):
        rbd, contact = sim.step(0.001, nsub); s = sim.state(); s["rbd"] = rbd; s["contact"] = contact; out.append(s)
    itf.close()
    check_plant(o, cases, out, steps, nsub, name)


@pytest.mark.parametrize("name", HEAVY)
def test_policy_rollout(name):
    """qmhip_policy_rollout on a C2 solve (N = 20) of the device, the downloaded plan and gains as the reference's plan (test_gpu_policy_rollout): rollout_ref.check_rows
    on the variant's oracle, feed-forward and feedback — the private forward kinematics of k_rollout.h"""
    import rollout_ref as rr
    from qm_control_amd import api
    o = rv.oracle(name); cfg = config("C2", 1, 20)
    itf = interface(name, max_batch=1, max_nodes=36, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    d = mpc.download(); gain, _ = mpc.feedback(); assert (d["status"] == 0).all()
    n = int(d["num_nodes"][0]); res = dict(t=d["t"][0, :n], ev=d["event"][0, :n], x=d["x"][0, :n], u=d["u"][0, :n])
    plans = [rr.Plan(res, gain[0, :n], cfg["ev"][0], cfg["modes"][0])]; rows = rollout_rows(plans); outs = {}
    for feedback in (0, 1):
        rc, outs[feedback], _ = rr.call(itf.lib.qmhip_policy_rollout, itf.h, rows, rr.DT, 4096, feedback, cap=40); assert rc == 0, itf.lib.qmhip_last_error(itf.h).decode()
    fric = float(itf.settings_blob[L.ST_FRIC_COEF]); itf.close()
    for feedback in (0, 1):
        out = outs[feedback]
        worst = rr.check_rows(o, plans, fric, rows, out, rr.DT, 4096, feedback, 0, "%s feedback %d" % (name, feedback))
        print(name, "rollout feedback", feedback, {k: "%.2e" % v for k, v in worst.items()})
        if feedback: assert out["summary"]["max_fb"].max() > 1e-3
        else: assert not out["summary"]["max_fb"].any()
        assert out["summary"]["events"].max() >= 1 and out["summary"]["steps"].max() >= 6


@pytest.mark.parametrize("name", HEAVY)
def test_plan_task_space_footholds_and_observe(name):
    """qmhip_plan_task_space / qmhip_plan_footholds on a trot and a flying-trot solve, qmhip_task_space_eval on 48 random state rows (random attitude, every mode) —
    plan_ref.compare / compare_footholds on the variant's oracle (positions 1e-12, velocities 1e-9); qmhip_observe (rbd -> centroidal: INOM, RNOM of the variant) on
    measured states of the variant's oracle against test_sim.centroidal_from_rbd, 1e-12 (test_gpu_tick)"""
    import plan_ref as pf
    from qm_control_amd import api, scenarios
    from test_gpu_plan_task_space import _pad, _check_plan
    from test_sim import centroidal_from_rbd, random_cases
    o = rv.oracle(name); bl = rv.blobs(name)
    cfg = _pad([scenarios.gait_config(g, batch=1, n_intervals=20, seed=sd) for g, sd in (("trot", 7), ("flying_trot", 9))])
    itf = interface(name, max_batch=8, max_nodes=36, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    got = mpc.download(); rec, nn = mpc.plan_task_space(); fh, cnt = mpc.plan_footholds(16)
    R = 48; x, u, mode, ee = pf.random_states(bl, R, 3); rows = itf.task_space(x, u, mode, ee)
    cases = random_cases(o, bl[1], 8, 5); rng = np.random.default_rng(4)
    rbd = np.array([o.rbd_from_q(c["q"], c["v"]) for c in cases]); rbd[:, 0] = rng.uniform(-3.1, 3.1, 8); rbd[:, 1:3] += rng.uniform(-0.4, 0.4, (8, 2)); rbd[:, 24:30] = rng.normal(size=(8, 6))
    xo = itf.observe(rbd)
    itf.close()
    assert (got["status"] == 0).all()
    mx = _check_plan(o, cfg, got, rec, nn, name + " trot + flying trot"); mf = 0.0
    live = np.concatenate([rec[b, :nn[b]] for b in range(2)]); assert (live["contact_mask"] == 0).any() and (live["cop"][:, 2] > 1.0).any()
    for b in range(2):
        n = int(nn[b]); ref = pf.footholds(o, got["t"][b, :n], got["x"][b, :n], cfg["ev"][b], cfg["modes"][b])
        mf = max(mf, pf.compare_footholds(fh[b], cnt[b], ref, 16, "%s instance %d" % (name, b)))
    assert cnt.sum() > 0
    ref = np.array([pf.record(o, x[r], u[r], mode[r], (ee[r, :3], ee[r, 3:])) for r in range(R)])
    mr = pf.compare(rows, ref, name + " state rows")
    eo = float(np.abs(xo - np.array([centroidal_from_rbd(bl[0], r) for r in rbd])).max())
    print(name, "state rows", {k: "%.1e" % v for k, v in sorted(mr.items())}, "footholds %.1e (%d landings)" % (mf, cnt.sum()), "observe %.1e" % eo)
    assert eo < 1e-12


@pytest.mark.parametrize("name", HEAVY)
def test_sensor_model_recomputes_the_end_effector_pose(name):
    """sense_ref.check_measurement on the variant: B = 4 records of sense_ref.plant_records (identity; noise; lag 3; noise + bias + the largest lag), 12 steps — the
    measured components bit for bit, and the end-effector pose the sensor kernel recomputes from the measured configuration against the variant's oracle (1e-7)"""
    import sense_ref as sr
    from qm_control_amd import api
    from test_sim import random_cases
    o = rv.oracle(name); mb, st = rv.blobs(name)
    cases = random_cases(o, st, 4, 5); arr = lambda k: np.array([c[k] for c in cases]); s = sr.plant_records()
    itf = interface(name, max_batch=4, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf)
    sim.set_sensors(s); sim.reset(arr("q"), arr("v"), 1.0); sim.setCommand(arr("pos"), arr("vel"), arr("kp"), arr("kd"), arr("ff"))
    truths = [sim.rbd()[0]]; meas = [sim.measured()]
    for k in range(12):
        rbd, _ = sim.step(0.001, 2); truths.append(rbd); meas.append(sim.measured())
    status = sim.state()["status"]; itf.close()
    assert (status == 0).all(); worst = [0.0, np.inf]
    for k, (m, n) in enumerate(meas):
        sr.check_measurement(m, n, truths, s, k, o, worst)
    print(name, "sensor model: end-effector pose of the measured configuration vs the oracle %.1e; least distance from the truth's pose %.1e" % tuple(worst))
    assert worst[1] < np.inf                                                           # the noisy records were compared


@pytest.mark.parametrize("name", HEAVY)
def test_ilqr_and_ipm_solves(name):
    """one discrete-iLQR solve (ST_SOLVER = 1: the nonlinear rollouts of k_ilqr.h carry a forward kinematics of their own) at the tolerances of
    test_gpu_mpc.test_discrete_ilqr_solver and one interior-point solve (ST_SOLVER = 3, ST_IPM_MU = 1e-2) at those of test_gpu_mpc.test_ipm_hard_cones, C2 with N = 20"""
    import pyoracle
    from qm_control_amd import api
    o = rv.oracle(name); omb, ost = rv.oracle_blobs(name); cfg = config("C2", 1, 20); N = 20
    itf = interface(name, max_batch=1, max_nodes=N + 16, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    itf.set_setting(L.ST_SOLVER, 1.0)
    res = mpc.run(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"], cfg["horizon"])
    ost = ost.copy()
    for idx, v in ((L.ST_IPM_MU, 1e-2), (L.ST_SOLVER, 3.0)):
        itf.set_setting(idx, v); ost[idx] = v
    ipm = mpc.run(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"], cfg["horizon"])
    info = itf.debug_read("ipm_info", (1, 8)); nm = itf.max_nodes; s_dev = itf.debug_read("ipm_s", (nm, 1, 28)); l_dev = itf.debug_read("ipm_l", (nm, 1, 28))
    itf.close()
    # ---- iLQR ----
    o.set_schedule(cfg["ev"][0], cfg["modes"][0]); o.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
    r = o.ilqr_step(cfg["t0"][0], cfg["t0"][0] + cfg["horizon"], cfg["x0"][0]); n = len(r["t"]); assert r["warn"] == 0 and r["alpha"] > 0.0
    assert res["status"][0] == 0 and res["num_nodes"][0] == n and np.array_equal(res["mode"][0, :n], r["mode"]) and res["perf"][0, 8] == r["alpha"]
    print(name, "iLQR", {k: "%.1e" % v for k, v in {**block_errs(res["x"][0, :n], r["x"], "x"), **block_errs(res["u"][0, :n], r["u"], "u")}.items()}, "alpha", r["alpha"])
    assert_blocks(res["x"][0, :n], r["x"], "x", TOL, "iLQR"); assert_blocks(res["u"][0, :n], r["u"], "u", TOL, "iLQR")
    # ---- IPM ----
    o3 = pyoracle.Oracle(omb, ost); o3.set_schedule(cfg["ev"][0], cfg["modes"][0]); o3.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
    r = o3.ipm_step(cfg["t0"][0], cfg["t0"][0] + cfg["horizon"], cfg["x0"][0]); n = len(r["t"]); assert r["warn"] == 0
    assert ipm["status"][0] == 0 and ipm["num_nodes"][0] == n and np.array_equal(ipm["t"][0, :n], r["t"]) and np.array_equal(ipm["event"][0, :n], r["ev"]) and np.array_equal(ipm["mode"][0, :n], r["mode"])
    print(name, "IPM", {k: "%.1e" % v for k, v in {**block_errs(ipm["x"][0, :n], r["x"], "x"), **block_errs(ipm["u"][0, :n], r["u"], "u")}.items()}, "alpha", r["alpha"])
    assert_blocks(ipm["x"][0, :n], r["x"], "x", TOL, "IPM x*"); assert_blocks(ipm["u"][0, :n], r["u"], "u", TOL, "IPM u*")
    assert ipm["perf"][0, 8] == pytest.approx(r["alpha"], rel=1e-9) and info[0, 1] == pytest.approx(r["alpha_primal_max"], rel=1e-6) and info[0, 2] == pytest.approx(r["alpha_dual_max"], rel=1e-6)
    assert info[0, 4] == pytest.approx(r["barrier"], rel=1e-12) and np.abs(ipm["perf"][0, :8] - r["perf"][:8]).max() <= 1e-6 * max(1.0, np.abs(r["perf"][:8]).max())
    for i in range(n - 1):
        if r["ev"][i] == 1:
            continue
        p = o3.ipm_node(i); on = p["on"] == 1
        assert (s_dev[i, 0][on] > 0.0).all() and (l_dev[i, 0][on] > 0.0).all(), i
        assert np.abs(s_dev[i, 0][on] - p["slack"][on]).max() <= 1e-6 * max(1.0, np.abs(p["slack"][on]).max()) and np.abs(l_dev[i, 0][on] - p["dual"][on]).max() <= 1e-6 * max(1e-3, np.abs(p["dual"][on]).max()), i
