"""GPU parity away from the nominal pose (tests/offnominal_cases.py): the LQ / stage records entry by entry at all 16 contact modes — m = 14 .. 18, so also the single-row
second tile of [Pp | rp] and Rp at m = 17 and the 15- and 14-row first tiles — at headings and attitudes where the rotation matrices are far from identity, the device's
own equivariance under a turn about z, four gait templates, the WBC and the plant at the eight poses.  Single kernel-level calls; the oracle is pinned at these poses by
tests/test_offnominal.py, which also runs the same comparisons on the host emulator."""
import numpy as np
import pytest
from conftest import assert_blocks, rel_err
import lq_record_check as LC
import offnominal_cases as OC

pytestmark = pytest.mark.gpu
TOL = 1e-6


def test_lq_and_stage_records_at_all_modes_offnominal(blobs, oracle):
    """One batch of seven instances through qmhip_debug_read (lq_debug 1; riccati_skip 20, then 0): all modes at the nominal pose, all modes at POSES[0], all modes
    reversed and held 0.045 s at POSES[1], stance at POSES[2] (its line search backtracks), and the twin of each moved one (psi = 0, origin; same schedule, pitch, roll).

    a. every non-event interval of every instance <= 1e-10 per block against the oracle (lq_record_check.check_interval), status 0, integers and node times bit-exact,
       x*, u*, perf, alpha as test_gpu_mpc._compare; m takes each of 14 .. 18 at least twice and all 16 modes occur; the product kernels give the same x*, u* bit for bit.
       The record buffers are [instance][node] (k_lq.h: a.stage + (b * nmax + i) * SR_SIZE, a.dbg likewise) — unlike the node arrays and ipm_s / ipm_l, which are
       [node][instance].
    b. the device's A_d, B_d, b_d and equality rows C, D, e of a moved instance equal Gx A Gx', Gx B Gu', Gx b, Gc C Gx', Gc D Gu', Gc e of its twin within 100 x the
       oracle's own residual for the same pair and block (offnominal_cases.ORACLE_EQUIVARIANCE, measured by test_offnominal.test_oracle_lq_model_is_equivariant:
       A, B <= 4.4e-16, C, D, e <= 2.7e-14, b <= 3.8e-13), 1e-10 at most."""
    from qm_control_amd import api
    from test_gpu_mpc import _compare
    inst = OC.lq_instances(); cfg = OC.stack_configs([c for _, c, _ in inst]); B = len(inst)
    sols = []
    for _, c, _ in inst:
        sols.append(OC.oracle_solve(oracle, c))
    nm = max(len(r["t"]) for r in sols) + 3
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=nm, max_ref_knots=2, max_events=cfg["ev"].shape[1])
    mpc = api.SqpMpc(itf)
    itf.debug_set("lq_debug", 1); assert itf.debug_get("lq_debug") == 1
    SRN, DBN = LC.SR["SR_SIZE"], LC.DBG["LQ_DBG_SIZE"]
    recs = {}
    for skip in (20, 0):
        itf.debug_set("riccati_skip", skip)
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
        recs[skip] = (itf.debug_read("stage", (B, nm, SRN)), itf.debug_read("lqdbg", (B, nm, DBN)), itf.debug_read("n_nodes", (B,), np.int32))
    itf.debug_set("riccati_skip", 0); itf.debug_set("lq_debug", 0); assert itf.debug_get("lq_debug") == 0
    res_dbg = mpc.download()
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); res = mpc.download()
    itf.close()
    # ---- a ----
    all_m = []; all_modes = set()
    for b, (name, c, _) in enumerate(inst):
        r = OC.oracle_solve(oracle, c); assert np.array_equal(r["x"], sols[b]["x"])      # (again: node_lq / node_proj answer for the last solve)
        for skip in (20, 0):
            stage, dbg, nn = recs[skip]
            assert nn[b] == len(r["t"]), (name, nn[b], len(r["t"]))
            worst, ms = OC.check_records(stage[b], dbg[b], oracle, r, after_riccati=(skip == 0))
            print(name, "riccati_skip", skip, {k: "%.1e" % v for k, v in worst.items()})
            bad = {k: v for k, v in worst.items() if not v <= 1e-10}
            assert not bad, (name, skip, bad, worst)
        all_m += ms; all_modes |= set(r["mode"].tolist())
        _compare(res_dbg, b, r)
    assert all(all_m.count(m) >= 2 for m in (14, 15, 16, 17, 18)), {m: all_m.count(m) for m in set(all_m)}
    assert sorted(all_modes) == list(range(16))
    assert np.array_equal(res["x"], res_dbg["x"]) and np.array_equal(res["u"], res_dbg["u"])      # the debug records change nothing
    # ---- b ----
    dbg = recs[20][1]
    for k, (name, c, twin) in enumerate(inst):
        if twin is None:
            continue
        j, psi = twin; r = sols[k]
        assert np.array_equal(sols[j]["ev"], r["ev"]) and np.array_equal(sols[j]["mode"], r["mode"])
        worst = {}
        for i in range(len(r["t"]) - 1):
            if r["ev"][i] == 1:
                continue
            for key, v in OC.equivariance_errs(OC.lq_blocks(dbg[k, i]), OC.lq_blocks(dbg[j, i]), int(r["mode"][i]), psi).items():
                worst[key] = max(worst.get(key, 0.0), v)
        print(name, "device equivariance", {key: "%.1e" % v for key, v in worst.items()})
        bad = {key: (v, OC.equivariance_bound(j, key)) for key, v in worst.items() if not v <= OC.equivariance_bound(j, key)}
        assert not bad, (name, bad)


@pytest.mark.parametrize("gait,poses", [("static_walk", (0, 1)), ("flying_trot", (2, 3)), ("pawup", (0, 1)), ("standing_pace", (2, 3))])
def test_gait_templates_offnominal(blobs, oracle, gait, poses):
    """test_gpu_mpc.test_every_gait_template with both instances moved to BASE_XY and two of the first four poses: three-leg support, flight, one foot up, lateral pairs"""
    from qm_control_amd import scenarios
    from test_gpu_mpc import _compare, _gpu_solve, _oracle_solve
    cfg = scenarios.gait_config(gait, batch=2, n_intervals=24)
    for b, p in enumerate(poses):
        OC.move_problem(cfg, b, OC.POSES[p][0], OC.BASE_XY, OC.POSES[p][1], OC.POSES[p][2])
    itf, mpc, res = _gpu_solve(blobs, cfg, 2, 96)
    for b in range(2):
        r = _oracle_solve(oracle, cfg, b); assert r["warn"] == 0
        _compare(res, b, r)
    itf.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_wbc_offnominal(blobs, oracle, variant):
    """16 cases at the eight poses (random, then hard; modes 15, 9, 6, 7, 14, 3, 12, 15), status [0, 0, 0] on both sides, 1e-6 per block; then the eight unmoved cases and
    their quarter-turn copies: the device's torques of the two agree within 2e-6 — two comparisons at the project's 1e-6, the oracle's own are invariant to 1.1e-11
    (test_offnominal.test_oracle_wbc_torques_are_invariant_under_quarter_turns, where the reason is written down)"""
    from qm_control_amd import api
    itf = api.QMInterface(blobs=blobs, max_batch=16, max_nodes=8, max_ref_knots=2, max_events=2)
    wbc = api.HierarchicalWbc(itf, mpc_variant=bool(variant))

    def run(cases):
        arr = lambda k: np.array([c[k] for c in cases])
        wbc.reset(); wbc.update(arr("xd"), arr("il"), arr("rbd"), arr("mode"), 0.002, arr("time"))       # primes inputLast_
        return wbc.update(arr("xd"), arr("ud"), arr("rbd"), arr("mode"), 0.002, arr("time"))

    cases = OC.wbc_offnominal_cases(oracle, blobs, OC.WBC_SEED + variant, OC.WBC_HARD_SEED + variant)
    out, st = run(cases)
    base = OC.wbc_base_cases(oracle, blobs, 8, OC.WBC_SEED + variant)
    out2, st2 = run(base + [OC.move_wbc_case(oracle, c, np.pi / 2, OC.BASE_XY) for c in base])
    itf.close()
    assert len(cases) == 16
    for b, c in enumerate(cases):
        ref, sto = OC.oracle_wbc(oracle, c, variant)
        assert list(sto) == [0, 0, 0], (b, sto)
        assert list(st[b]) == [0, 0, 0], (b, st[b])
        assert_blocks(out[b], ref, "wbc", TOL, b)
    assert (st2 == 0).all()
    errs = [OC.torque_err(out2[8 + b], out2[b]) for b in range(8)]
    print("variant", variant, "device torques under a quarter turn:", ["%.1e" % e for e in errs])
    assert max(errs) <= 2e-6, errs


@pytest.mark.parametrize("nsub", [1, 2])
def test_plant_offnominal(blobs, oracle, nsub):
    """test_gpu_sim.test_plant_vs_oracle at the eight yaws and BASE_XY (pitch and roll x 0.3: the feet stay near the ground), 12 steps, same bounds"""
    from qm_control_amd import api
    mb, st = blobs
    cases = OC.plant_offnominal_cases(oracle, st, OC.PLANT_SEED)
    B = len(cases); arr = lambda k: np.array([c[k] for c in cases])
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=8, max_ref_knots=2, max_events=2)
    sim = api.QMHWSim(itf)
    sim.reset(arr("q"), arr("v"), 1.0); sim.setCommand(arr("pos"), arr("vel"), arr("kp"), arr("kd"), arr("ff"))
    steps = 12; out = []
    for _ in range(steps):
        rbd, contact = sim.step(0.001, nsub); s = sim.state(); s["rbd"] = rbd; s["contact"] = contact; out.append(s)
    itf.close()
    for b, c in enumerate(cases):
        oracle.sim_params(); oracle.sim_reset(c["q"], c["v"], 1.0); oracle.sim_command(c["pos"], c["vel"], c["kp"], c["kd"], c["ff"])
        for k in range(steps):
            r = oracle.sim_step(0.001, nsub)
            assert r["status"] == 0 and out[k]["status"][b] == 0
            assert rel_err(out[k]["q"][b], r["q"]) < 1e-9 and rel_err(out[k]["v"][b], r["v"]) < 1e-7, (b, k)
            assert rel_err(out[k]["force"][b], r["force"]) < 1e-6 and list(out[k]["contact"][b]) == list(r["contact"]), (b, k)
            assert rel_err(out[k]["rbd"][b], r["rbd"]) < 1e-7 and abs(out[k]["time"][b] - r["time"]) < 1e-12, (b, k)
        assert r["contact"].any()
