"""Away from the nominal pose, on the CPU: pins of the oracle at the poses of tests/offnominal_cases.py (everything in test_gpu_offnominal.py trusts it there) and the
host-emulator twins of the GPU tests — LQ / stage records at all 16 contact modes (m = 14 .. 18), WBC and plant at the eight poses."""
import functools
import numpy as np
from qm_control_amd import layout as L
import pytest
from conftest import assert_blocks, rel_err
import offnominal_cases as OC

TOL = 1e-6


def test_movers_reproduce_the_unmoved_inputs(blobs, oracle):
    """psi = 0, d = 0, pitch = roll = 0: bit for bit what the unmoved call uses"""
    from qm_control_amd import scenarios
    from test_sim import random_cases
    for cfg in (scenarios.make_config("C3", batch=2, n_intervals=10), scenarios.gait_config("pawup", batch=2, n_intervals=24)):
        ref = {k: cfg[k].copy() for k in ("x0", "ref_x")}
        OC.move_problem(cfg, 1, 0.0, (0.0, 0.0), 0.0, 0.0)
        assert np.array_equal(cfg["x0"], ref["x0"]) and np.array_equal(cfg["ref_x"], ref["ref_x"])
    from wbc_cases import random_wbc_inputs
    for c, c0 in zip(OC.wbc_base_cases(oracle, blobs, 4, 3, modes=(15, 9, 6, 15, 9, 6)), random_wbc_inputs(oracle, blobs, 4, 3, 0.05)):
        assert all(np.array_equal(c[k], c0[k]) for k in c0) and np.array_equal(oracle.rbd_from_q(c["q"], c["v"]), c0["rbd"])      # the recorded (q, v) are the unmoved call's
        m = OC.move_wbc_case(oracle, c, 0.0)
        assert all(np.array_equal(m[k], c[k]) for k in ("rbd", "xd", "ud", "il", "q", "v")) and m["mode"] == c["mode"] and m["time"] == c["time"]
    for c in random_cases(oracle, blobs[1], 2, 5):
        m = OC.move_plant_case(c, 0.0)
        assert all(np.array_equal(m[k], c[k]) for k in c)
    assert np.array_equal(OC.Gx(0.0), np.eye(30)) and np.array_equal(OC.Gu(0.0), np.eye(30)) and np.array_equal(OC.Gc(9, 0.0), np.eye(14))
    # ... and a moved instance really is somewhere else
    cfg = OC.move_problem(scenarios.make_config("C3", batch=1, n_intervals=10), 0, 2.5, OC.BASE_XY, 0.3, -0.25)
    assert abs(cfg["x0"][0, 6] - 40.0) < 0.1 and abs(cfg["x0"][0, 9] - 2.5) < 0.1 and abs(cfg["ref_x"][0, 1, 10] - 0.3) < 1e-12
    ev, modes = OC.all_modes_schedule(0.2, 0.03)
    assert sorted(set(modes.tolist())) == list(range(16)) and len(ev) == 16 and abs(ev[0] - 0.21) < 1e-15 and abs(ev[-1] - ev[0] - 15 * 0.03) < 1e-12


# ---------------------------------------------------------------- oracle pins ----------------------------------------------------------------

def _xu(blobs, seed=0):
    rng = np.random.default_rng(seed)
    x = blobs[1][L.ST_XINIT:L.ST_XINIT + 30] + 0.05 * rng.normal(size=30); u = rng.normal(size=30); u[2:12:3] += 70
    return x, u


@pytest.mark.parametrize("pose", [OC.POSES[0], OC.POSES[2], OC.POSES[4]])
def test_oracle_flow_map_jacobians_vs_finite_differences_offnominal(blobs, oracle, pose):
    """test_oracle.test_flow_map_jacobians_vs_finite_differences at BASE_XY and three of the poses, same bound"""
    x, u = _xu(blobs); x = OC.move_state(x, pose[0], OC.BASE_XY, pose[1], pose[2]); u = OC.move_input(u, pose[0])
    f, A, B = oracle.flow_map(x, u, jac=True)
    eps = 1e-6; worst = 0.0
    for k in range(30):
        d = np.zeros(30); d[k] = eps
        worst = max(worst, np.abs((oracle.flow_map(x + d, u) - oracle.flow_map(x - d, u)) / (2 * eps) - A[:, k]).max(), np.abs((oracle.flow_map(x, u + d) - oracle.flow_map(x, u - d)) / (2 * eps) - B[:, k]).max())
    print(pose, "finite-difference residual %.1e" % worst)
    assert worst < 1e-6
    assert np.abs(A[9:12, 3:6]).max() > 0.1 and np.abs(A[9:12, 9:12]).max() > 1e-3      # the Euler-rate map and its derivative ARE exercised here


@pytest.mark.parametrize("psi", [np.pi / 2, 2.5, -3.1, 3.14159, 7.0])
def test_oracle_flow_map_is_equivariant(blobs, oracle, psi):
    """a turn by psi about the world's z axis plus a translation in the ground plane is a symmetry of the continuous flow map: f' = Gx f, A' = Gx A Gx', B' = Gx B Gu',
    at pitch 0.4, roll -0.35.  Measured: f <= 2.2e-14, A <= 4.3e-16, B <= 3.6e-16 relative; bound 1e-12 (about 40 x the worst, rounding only)."""
    x, u = _xu(blobs); x[10] += 0.4; x[11] -= 0.35
    f, A, B = oracle.flow_map(x, u, jac=True)
    f2, A2, B2 = oracle.flow_map(OC.move_state(x, psi, OC.BASE_XY, 0.0, 0.0), OC.move_input(u, psi), jac=True)
    gx, gu = OC.Gx(psi), OC.Gu(psi)
    errs = (rel_err(f2, gx @ f), rel_err(A2, gx @ A @ gx.T), rel_err(B2, gx @ B @ gu.T))
    print("psi %.5f: f %.1e A %.1e B %.1e" % ((psi,) + errs))
    assert max(errs) < 1e-12
    assert rel_err(f2, f) > 1e-2 and rel_err(A2, A) > 1e-3                      # ... and it is not the identity


from offnominal_cases import oracle_wbc as _oracle_wbc, torque_err      # noqa: E402


@pytest.mark.parametrize("variant", [0, 1])
def test_oracle_wbc_torques_are_invariant_under_quarter_turns(blobs, oracle, variant):
    """The joint torques of the oracle's WBC do not change when the whole problem is turned by a quarter turn about z and translated — measured over the eight base cases
    of the off-nominal batch and psi in {pi/2, -pi/2, pi}: <= 3.1e-13 (variant 0), <= 1.1e-11 (variant 1) on the torque block's scale (tests/blocks.py); asserted at
    100 x the measured worst: 3.1e-11 and 1.1e-9.

    At psi = 2.5 they change by 18 - 88 % (the cases below), and that is neither a defect of the oracle nor of the kernels.  Every term of oracle/src/wbc.h turns with the problem (the gains of
    the base and end-effector tasks are isotropic: kp / kd 3000 / 75 and 2000 / 75 on all three axes) except one: the friction constraint of level 0 is the reference's
    four-sided PYRAMID |Fx| <= mu Fz, |Fy| <= mu Fz with its sides along the WORLD's x and y axes (WbcBase::formulateFrictionConeTask builds the same 5 x 3 block), and a
    square maps onto itself under quarter turns only.  The pyramid binds in most of these cases (the level-1 tasks ask, with their gains, for far larger tangential forces
    than mu = 0.3 allows), so the solution depends on the heading; with mu raised the difference at psi = 2.5 falls like 1 / mu.  The cases with time = 5.0 are
    invariant at psi = 2.5 too in variant 0 (<= 1e-11): before t = 10 its level 1 is the arm's joint task alone, nothing asks for tangential force beyond the plan and
    no side of the pyramid is active (in variant 1 the time plays no part and they change like the others).  Both facts are asserted below."""
    base = OC.wbc_base_cases(oracle, blobs, 8, OC.WBC_SEED + variant)
    ref = [_oracle_wbc(oracle, c, variant) for c in base]
    assert all(list(s) == [0, 0, 0] for _, s in ref)
    worst = 0.0
    for psi in (np.pi / 2, -np.pi / 2, np.pi):
        for c, (out, _) in zip(base, ref):
            o2, s2 = _oracle_wbc(oracle, OC.move_wbc_case(oracle, c, psi, OC.BASE_XY), variant)
            assert list(s2) == [0, 0, 0]
            worst = max(worst, torque_err(o2, out))
    print("variant", variant, "quarter turns: worst torque change %.1e" % worst)
    assert worst <= (3.1e-11, 1.1e-9)[variant]
    at25 = [torque_err(_oracle_wbc(oracle, OC.move_wbc_case(oracle, c, 2.5, OC.BASE_XY), variant)[0], out) for c, (out, _) in zip(base, ref)]
    print("variant", variant, "psi 2.5:", ["%.1e" % e for e in at25])
    assert max(at25) > 1e-2                                                        # the pyramid is felt
    if variant == 0:
        assert all(e < 1e-10 for c, e in zip(base, at25) if c["time"] < 10.0) and any(c["time"] < 10.0 for c in base)
    mu = oracle.set_setting(L.ST_WBC_FRIC, 1e5)                                    # a pyramid too wide to bind away from Fz = 0: what is left falls like 1 / mu
    try:
        wide = [torque_err(_oracle_wbc(oracle, OC.move_wbc_case(oracle, c, 2.5, OC.BASE_XY), 0)[0], _oracle_wbc(oracle, c, 0)[0]) for c in base]
    finally:
        oracle.set_setting(L.ST_WBC_FRIC, mu)
    print("mu 1e5, psi 2.5:", ["%.1e" % e for e in wide])
    assert max(wide) < 1e-3 * max(at25)


@functools.lru_cache(maxsize=None)
def _instances():
    return OC.lq_instances()


def test_all_modes_schedule_reaches_every_mode_and_every_m(oracle):
    """what the entrywise tests rely on: the oracle solves the all-modes problem cleanly (no warning, full step) at the nominal pose and away from it, all 16 modes
    are on the horizon and the number of free inputs m takes each of 14 .. 18 at least twice"""
    for name, cfg, _ in _instances()[:3]:
        r = OC.oracle_solve(oracle, cfg); n = len(r["t"])
        ms = [oracle.node_proj(i)["m"] for i in range(n - 1) if r["ev"][i] != 1]
        assert r["warn"] == 0 and r["alpha"] == 1.0, (name, r["warn"], r["alpha"])
        assert sorted(set(r["mode"].tolist())) == list(range(16)), name
        assert {m: ms.count(m) for m in sorted(set(ms))} == {14: 2, 15: 8, 16: 12, 17: 8, 18: 5}, name


def test_oracle_lq_model_is_equivariant(oracle):
    """the discrete LQ model of every interval — A_d, B_d, b_d and the equality rows C, D, e — of a moved instance against its twin (same schedule, pitch and roll;
    psi = 0 at the origin): A' = Gx A Gx', B' = Gx B Gu', b' = Gx b, C' = Gc C Gx', D' = Gc D Gu', e' = Gc e.  Every row group turned out equivariant: a stance leg's three
    zero-velocity rows and a swing leg's three zero-force rows turn with Rz, its normal-velocity row stays (offnominal_cases.Gc); none is left out.
    Measured (offnominal_cases.ORACLE_EQUIVARIANCE): A, B <= 4.4e-16, C, D, e <= 2.7e-14, b <= 3.8e-13 (differences of positions near 40 m on the scale of b); asserted
    at 100 x the measured value of each pair and block."""
    inst = _instances()
    for k, (name, cfg, twin) in enumerate(inst):
        if twin is None:
            continue
        j, psi = twin
        r = OC.oracle_solve(oracle, cfg); n = len(r["t"]); lq_t = [oracle.node_lq(i) for i in range(n - 1)]
        r2 = OC.oracle_solve(oracle, inst[j][1]); lq_m = [oracle.node_lq(i) for i in range(n - 1)]
        assert np.array_equal(r["t"], r2["t"]) and np.array_equal(r["mode"], r2["mode"])
        worst = {}
        for i in range(n - 1):
            if r["ev"][i] == 1:
                continue
            for key, v in OC.equivariance_errs(lq_t[i], lq_m[i], int(r["mode"][i]), psi).items():
                worst[key] = max(worst.get(key, 0.0), v)
        print(name, {key: "%.1e" % v for key, v in worst.items()})
        bad = {key: v for key, v in worst.items() if not v <= 100.0 * OC.ORACLE_EQUIVARIANCE[j][key]}
        assert not bad, (name, bad)
        assert rel_err(lq_m[0]["A"], lq_t[0]["A"]) > 1e-3                          # not the identity


# ---------------------------------------------------------------- emulator twins of the GPU tests ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _emulated(k, skip):
    """instance k of lq_instances() through the emulated MPC iteration: (status, n_nodes, node_t, node_ev, node_mode, xs, us, perf, stage records, debug records)"""
    import emu_harness
    from qm_control_amd import scenarios
    cfg = _instances()[k][1]; blobs = scenarios.load_blobs(); nm = 56
    e = emu_harness.Emu(blobs[0], blobs[1], 1, nm, 2, cfg["ev"].shape[1]); e.set_riccati_skip(skip)
    e.mpc_step(cfg)
    n = int(e.buf("n_nodes", (1,), np.int32)[0])
    return dict(status=int(e.buf("status", (1,), np.int32)[0]), n=n, t=e.node_arr("node_t", 1)[:n, 0].copy(), ev=e.node_arr("node_ev", 1, np.int32)[:n, 0].copy(), mode=e.node_arr("node_mode", 1, np.int32)[:n, 0].copy(),
                xs=e.node_arr("xs", 30)[:n, 0].copy(), us=e.node_arr("us", 30)[:n, 0].copy(), perf=e.buf("out_perf", (10,)).copy(),
                stage=np.stack([e.stage(0, i) for i in range(n)]), dbg=np.stack([e.lqdbg(0, i) for i in range(n)]))


@pytest.mark.parametrize("skip", [20, 0])
@pytest.mark.parametrize("k", [0, 1])
def test_emulated_lq_records_at_all_modes(oracle, k, skip):
    """test_emu_kernels.test_lq_records_entrywise on the all-modes schedule, at the nominal pose (k = 0) and at POSES[0] (k = 1): <= 1e-10 per block, m = 14 .. 18"""
    name, cfg, _ = _instances()[k]
    r = OC.oracle_solve(oracle, cfg); n = len(r["t"]); d = _emulated(k, skip)
    assert d["status"] == 0 and d["n"] == n and np.array_equal(d["t"], r["t"]) and np.array_equal(d["ev"], r["ev"]) and np.array_equal(d["mode"], r["mode"])
    worst, ms = OC.check_records(d["stage"], d["dbg"], oracle, r, after_riccati=(skip == 0))
    print(name, "riccati_skip", skip, {key: "%.1e" % v for key, v in worst.items()})
    bad = {key: v for key, v in worst.items() if not v <= 1e-10}
    assert not bad, (name, skip, bad)
    assert all(ms.count(m) >= 2 for m in (14, 15, 16, 17, 18))
    if skip == 0:
        assert_blocks(d["xs"], r["x"], "x", TOL); assert_blocks(d["us"], r["u"], "u", TOL)
        assert d["perf"][8] == r["alpha"] and rel_err(d["perf"][:8], r["perf"][:8]) <= 1e-6


def test_emulated_lq_model_is_equivariant(oracle):
    """the device's A_d, B_d, b_d, C, D, e of the moved all-modes instance against its twin's, at the bound the GPU test uses (100 x the oracle's own residual, <= 1e-10)"""
    inst = _instances(); j, psi = inst[2][2]; assert j == 1
    tw, mv = _emulated(2, 20), _emulated(1, 20)
    assert np.array_equal(tw["ev"], mv["ev"]) and np.array_equal(tw["mode"], mv["mode"])
    worst = {}
    for i in range(tw["n"] - 1):
        if tw["ev"][i] == 1:
            continue
        for key, v in OC.equivariance_errs(OC.lq_blocks(tw["dbg"][i]), OC.lq_blocks(mv["dbg"][i]), int(tw["mode"][i]), psi).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print({key: "%.1e" % v for key, v in worst.items()})
    bad = {key: v for key, v in worst.items() if not v <= OC.equivariance_bound(j, key)}
    assert not bad, bad


@pytest.mark.parametrize("variant", [0, 1])
def test_emulated_wbc_offnominal(blobs, oracle, variant):
    """the WBC kernel at the eight poses: one batch of eight of the GPU test's sixteen cases (the emulated kernel takes most of a second per case) — four random ones at
    POSES[0..3] (modes 15, 9, 6, 7) and four hard ones at POSES[4..7] (modes 14, 3, 12, 15)"""
    import emu_harness
    e = emu_harness.Emu(blobs[0], blobs[1], 8, 8, 2, 2)
    cases = OC.wbc_offnominal_cases(oracle, blobs, OC.WBC_SEED + variant, OC.WBC_HARD_SEED + variant); cases = cases[0:4] + cases[12:16]
    arr = lambda k: np.array([c[k] for c in cases])
    e.wbc_reset(); e.wbc_step(arr("xd"), arr("il"), arr("rbd"), arr("mode"), 0.002, arr("time"), variant)
    out, st, _ = e.wbc_step(arr("xd"), arr("ud"), arr("rbd"), arr("mode"), 0.002, arr("time"), variant)
    for b, c in enumerate(cases):
        ref, sto = _oracle_wbc(oracle, c, variant)
        assert list(sto) == [0, 0, 0] and list(st[b]) == [0, 0, 0], (b, sto, st[b])
        assert_blocks(out[b], ref, "wbc", TOL, b)


def test_oracle_ends_every_offnominal_wbc_case_cleanly(blobs, oracle):
    """the seeds of the GPU test's WBC batch were chosen so that the oracle alone ends all sixteen cases of both variants with status [0, 0, 0]: no case has to be dropped there"""
    for variant in (0, 1):
        cases = OC.wbc_offnominal_cases(oracle, blobs, OC.WBC_SEED + variant, OC.WBC_HARD_SEED + variant)
        assert len(cases) == 16 and [c["mode"] for c in cases] == 2 * list(OC.WBC_MODES)
        for b, c in enumerate(cases):
            assert abs(c["rbd"][3] - 40.0) < 0.5 and abs(c["rbd"][0] - OC.POSES[b % 8][0]) < 0.5
            assert list(_oracle_wbc(oracle, c, variant)[1]) == [0, 0, 0], (variant, b)


@pytest.mark.parametrize("nsub", [1, 2])
def test_emulated_plant_offnominal(blobs, oracle, nsub):
    """test_sim.test_emulated_plant_vs_oracle at the eight yaws and BASE_XY, same bounds"""
    import emu_harness
    mb, st = blobs
    cases = OC.plant_offnominal_cases(oracle, st, OC.PLANT_SEED)
    arr = lambda k: np.array([c[k] for c in cases])
    e = emu_harness.Emu(mb, st, 8, 8, 2, 2)
    e.sim_params(); e.sim_reset(arr("q"), arr("v"), 1.0); e.sim_command(arr("pos"), arr("vel"), arr("kp"), arr("kd"), arr("ff"))
    steps = 12
    out = [e.sim_step(0.001, nsub) for _ in range(steps)]
    for b, c in enumerate(cases):
        oracle.sim_params(); oracle.sim_reset(c["q"], c["v"], 1.0); oracle.sim_command(c["pos"], c["vel"], c["kp"], c["kd"], c["ff"])
        for k in range(steps):
            r = oracle.sim_step(0.001, nsub)
            assert r["status"] == 0 and out[k]["status"][b] == 0
            assert rel_err(out[k]["q"][b], r["q"]) < 1e-9 and rel_err(out[k]["v"][b], r["v"]) < 1e-7, (b, k)
            assert rel_err(out[k]["force"][b], r["force"]) < 1e-6 and list(out[k]["contact"][b]) == list(r["contact"]), (b, k)
            assert rel_err(out[k]["rbd"][b], r["rbd"]) < 1e-7, (b, k)
        assert r["contact"].any()                                                  # the feet did stay near the ground
