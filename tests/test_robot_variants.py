"""Every kernel on perturbed robots (tests/robot_variants.py), on the CPU: the two ingestions on URDFs neither has seen, proof that the variants leave the special structure
of the shipped robot (JR = I on the legs, coordinate joint axes, feet straight below the knee, diagonal arm inertias, mirror-image legs), the oracle's clean solves of every
configuration used here and on the device, and the host-emulator twins of tests/test_gpu_robot_variants.py at the tolerances the project states for the same quantities on
the shipped robot.  The product side always runs on the product's ingestion of the variant, the oracle on the numpy front-end's."""
import numpy as np
import pytest

import robot_variants as rv
from conftest import assert_blocks, rel_err
from qm_control_amd import layout as L, scenarios

TOL = 1e-6
ALL = ("mild", "skew", "strong")
HEAVY = ("skew", "strong")
# the MPC problems of this file and of the GPU file: (scenario, batch, intervals)
MPC_CONFIGS = (("C2", 1, 26), ("C1", 1, 10), ("C3", 4, 20), ("C5", 2, 30), ("C2", 1, 20), ("gait:dynamic_walk", 4, 30))


def config(name, B, N):
    return scenarios.gait_config(name[5:], batch=B, n_intervals=N) if name.startswith("gait:") else scenarios.make_config(name, batch=B, n_intervals=N)


def oracle_solve(o, cfg, b=0):
    o.set_schedule(cfg["ev"][b], cfg["modes"][b]); o.set_target(cfg["ref_t"][b], cfg["ref_x"][b])
    return o.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b])


def check_plant(o, cases, out, steps, nsub, what=""):
    """out[k]: dict(q, v, force, contact, rbd, status [, time]) [B] after step k, against the oracle's plant stepped along — the bounds of
    test_sim.test_emulated_plant_vs_oracle / test_gpu_sim.test_plant_vs_oracle.  GATE on the oracle: status 0 throughout and a foot on the ground somewhere in the batch
    (the variants' legs differ in length: where the shipped robot touches down with four feet these cases stand on the longest leg)"""
    feet = np.zeros(4, int); worst = dict(q=0.0, v=0.0, force=0.0, rbd=0.0)
    for b, c in enumerate(cases):
        o.sim_params(); o.sim_reset(c["q"], c["v"], 1.0); o.sim_command(c["pos"], c["vel"], c["kp"], c["kd"], c["ff"])
        for k in range(steps):
            r = o.sim_step(0.001, nsub); feet += r["contact"]
            assert r["status"] == 0 and out[k]["status"][b] == 0, (b, k)
            for key in worst: worst[key] = max(worst[key], rel_err(out[k][key][b], r[key]))
            assert rel_err(out[k]["q"][b], r["q"]) < 1e-9 and rel_err(out[k]["v"][b], r["v"]) < 1e-7, (b, k)
            assert rel_err(out[k]["force"][b], r["force"]) < 1e-6 and list(out[k]["contact"][b]) == list(r["contact"]), (b, k)
            assert rel_err(out[k]["rbd"][b], r["rbd"]) < 1e-7, (b, k)
            if "time" in out[k]: assert abs(out[k]["time"][b] - r["time"]) < 1e-12, (b, k)
    print(what, "plant nsub", nsub, {k: "%.1e" % v for k, v in worst.items()}, "contact steps per foot", feet.tolist())
    assert feet.sum() > 0
    return worst


# ---------------------------------------------------------------- the variants themselves ----------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_both_ingestions_agree_on_the_variant(name, tmp_path):
    """test_layout_and_abi.test_oracle_blobs_come_from_the_numpy_front_end_and_check_the_product on a URDF neither ingestion has seen: <= 1e-13 absolute on both blobs —
    rpy composition through the fixed joints, inertia transport with rotated inertial origins, INOM / RNOM, R <- J' R12 J at a general feet Jacobian"""
    import front
    (mb, st), (omb, ost) = rv.blobs(name), rv.oracle_blobs(name)
    print(name, "model %.1e settings %.1e" % (np.abs(mb - omb).max(), np.abs(st - ost).max()))
    assert np.abs(mb - omb).max() <= 1e-13 and np.abs(st - ost).max() <= 1e-13
    for k in ("SQP_DT", "PHASE_TRANS_STANCE", "TIME_HORIZON", "SWING_TIME_SCALE"):
        assert st[front.ST[k]] == ost[front.ST[k]], k
    # the generator is deterministic and leaves the tree, the names and the committed file alone
    again = rv.write_variant(name, str(tmp_path))
    assert open(again, "rb").read() == open(rv.urdf(name), "rb").read()
    assert front.build_model(again, rv.REFI)[1] == front.build_model(rv.URDF, rv.REFI)[1]
    # what make_config / gait_config / the case generators read from the SHIPPED blobs is the same on the variant: its problems are the shipped problems
    smb, sst = scenarios.load_blobs()
    for a, b, n in ((L.MB_QLO, L.MB_QLO, 18), (L.MB_QHI, L.MB_QHI, 18), (L.MB_QNOM, L.MB_QNOM, 18)):
        assert np.array_equal(mb[a:a + n], smb[b:b + n])
    assert np.array_equal(st[L.ST_XINIT:L.ST_XINIT + 30], sst[L.ST_XINIT:L.ST_XINIT + 30]) and st[L.ST_SQP_DT] == sst[L.ST_SQP_DT]


@pytest.mark.parametrize("name", ALL)
def test_variant_leaves_the_special_structure(name):
    a, l, _ = rv.VARIANTS[name]; mb, st = rv.blobs(name); smb, _ = scenarios.load_blobs()
    JR = mb[L.MB_JR:L.MB_JR + 162].reshape(18, 3, 3); AX = mb[L.MB_AXIS:L.MB_AXIS + 54].reshape(18, 3); FP = mb[L.MB_FP:L.MB_FP + 15].reshape(5, 3)
    FR = mb[L.MB_FR:L.MB_FR + 45].reshape(5, 3, 3); IN = mb[L.MB_INERTIA:L.MB_INERTIA + 171].reshape(19, 3, 3); M = mb[L.MB_MASS:L.MB_MASS + 19]
    # (the shipped robot HAS the structure: the checks below are not vacuous)
    sJR = smb[L.MB_JR:L.MB_JR + 162].reshape(18, 3, 3); sAX = smb[L.MB_AXIS:L.MB_AXIS + 54].reshape(18, 3); sFP = smb[L.MB_FP:L.MB_FP + 15].reshape(5, 3)
    assert all(np.array_equal(sJR[j], np.eye(3)) for j in range(12)) and all(sorted(np.abs(v)) == [0.0, 0.0, 1.0] for v in sAX) and not sFP[:4, :2].any()
    assert max(np.abs(JR[j] - np.eye(3)).max() for j in range(12)) > a / 4
    unit = [s * e for e in np.eye(3) for s in (1.0, -1.0)]
    assert all(min(np.linalg.norm(v - e) for e in unit) > 1e-3 for v in AX[:12])                 # no leg axis is a coordinate axis ...
    assert all(abs(np.linalg.norm(v) - 1.0) <= 1e-15 for v in AX)                                # ... and all are unit vectors
    assert all(abs(FP[f, 0]) > 1e-4 and abs(FP[f, 1]) > 1e-4 for f in range(4))
    assert max(np.abs(FR[f] - np.eye(3)).max() for f in range(4)) > a / 4 and all(np.abs(FR[f] - np.eye(3)).max() > 0.0 for f in range(5))
    for b in range(13, 19):                                                                     # arm bodies (chain 4: bodies 13 .. 18)
        assert min(abs(IN[b][0, 1]), abs(IN[b][0, 2]), abs(IN[b][1, 2])) > 1e-9, b
    for b in range(19):
        assert np.abs(IN[b] - IN[b].T).max() <= 1e-18 + 1e-15 * np.abs(IN[b]).max() and np.linalg.eigvalsh(0.5 * (IN[b] + IN[b].T)).min() > 0.0 and M[b] > 0.0, b
    # bodies in the order LF, LH, RF, RH (hip, thigh, calf): LF_thigh = body 2, RF_thigh = body 8
    import front
    names = front.build_model(rv.urdf(name), rv.REFI)[1]
    assert names[1] == "LF_HFE" and names[7] == "RF_HFE" and abs(M[2] - M[8]) > 1e-3 * M[2]
    # mirror symmetry of JP and COM between LF and RF (y flipped) is gone
    JP = mb[L.MB_JP:L.MB_JP + 54].reshape(18, 3); flip = np.array([1.0, -1.0, 1.0])
    assert all(np.abs(JP[j] - flip * JP[6 + j]).max() > l / 100 for j in range(3))
    # the blob validator's topology checks (qm_model_io.cpp validateModelBlob; the parse itself applies them to the URDF's tree)
    par = mb[L.MB_PARENT:L.MB_PARENT + 18].astype(int); fpar = mb[L.MB_FPARENT:L.MB_FPARENT + 5].astype(int)
    assert list(par) == [0 if (j % 3 == 0 if j < 12 else j == 12) else j for j in range(18)] and list(fpar) == [3, 9, 6, 12, 18] and mb[L.MB_ROBOTMASS] > 0.0
    assert abs(mb[L.MB_ROBOTMASS] - M.sum()) <= 1e-12 * M.sum()


@pytest.mark.parametrize("name", ALL)
def test_input_weight_stays_block_diagonal(name):
    """R <- J' R12 J with the feet Jacobian of the variant keeps one 3 x 3 block per leg (a foot moves with its own leg's joints only), so the STRUCTURED instances of K1b's
    mat-vec and of the trial evaluation are the ones the variants run (qm_r_is_block_diagonal, asked of the emulator's pipeline); the leg blocks are full"""
    import emu_harness
    mb, st = rv.blobs(name)
    assert emu_harness.Emu(mb, st, 1, 8, 2, 2).r_blocks()
    R = st[L.ST_R:L.ST_R + 900].reshape(30, 30)
    for c in range(4):
        assert np.count_nonzero(R[12 + 3 * c:15 + 3 * c, 12 + 3 * c:15 + 3 * c]) == 9, c


@pytest.mark.parametrize("name", ALL)
def test_oracle_solves_every_configuration_cleanly(name):
    """GATES on the oracle alone, for every MPC problem of this file and of the GPU file: batch_step bad == 0, mpc_step warn == 0, a step accepted.  A variant that breaks
    one gets another seed (robot_variants.VARIANTS), never a skip or a wider bound.  (The WBC and plant gates — statuses [0, 0, 0], plant status 0 with a contact — are
    asserted on the oracle inside the tests of those kernels.)"""
    import pyoracle
    o = rv.oracle(name)
    for cname, B, N in MPC_CONFIGS:
        cfg = config(cname, B, N)
        bad, _, _, _ = pyoracle.batch_step(*rv.oracle_blobs(name), 2, cfg["t0"], cfg["horizon"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"], cfg["period"], cfg["time"])
        assert bad == 0, (name, cname)
        for b in range(B):
            r = oracle_solve(o, cfg, b); assert r["warn"] == 0 and r["alpha"] > 0.0, (name, cname, b, r["warn"], r["alpha"])


# ---------------------------------------------------------------- emulator twins of the GPU tests ----------------------------------------------------------------

@pytest.mark.parametrize("skip", [20, 0])
@pytest.mark.parametrize("cname,N", [("C2", 26), ("C1", 10)])
@pytest.mark.parametrize("name", HEAVY)
def test_emulated_lq_records_entrywise(name, cname, N, skip):
    """test_emu_kernels.test_lq_records_entrywise on the variant: <= 1e-10 per block.  C2: swing legs, whose 3 x 2 null-space blocks and normal-velocity rows depend on
    the now general foot Jacobian; C1: m = 18"""
    import emu_harness, lq_record_check as LC
    o = rv.oracle(name); mb, st = rv.blobs(name); cfg = config(cname, 1, N)
    r = oracle_solve(o, cfg); n = len(r["t"]); assert r["warn"] == 0
    e = emu_harness.Emu(mb, st, 1, n + 3, 2, cfg["ev"].shape[1]); e.set_riccati_skip(skip)
    e.mpc_step(cfg)
    assert e.buf("status", (1,), np.int32)[0] == 0 and e.buf("n_nodes", (1,), np.int32)[0] == n
    worst = {}
    for i in range(n - 1):
        if r["ev"][i] == 1:
            continue
        for k, v in LC.check_interval(e.stage(0, i), e.lqdbg(0, i), o.node_lq(i), o.node_proj(i), after_riccati=(skip == 0)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(name, cname, "riccati_skip", skip, {k: "%.1e" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 1e-10}
    assert not bad, (bad, worst)
    if skip == 0:
        assert_blocks(e.node_arr("xs", 30)[:n, 0], r["x"], "x", TOL); assert_blocks(e.node_arr("us", 30)[:n, 0], r["u"], "u", TOL)
        perf = e.buf("out_perf", (10,)); assert perf[8] == r["alpha"] and rel_err(perf[:8], r["perf"][:8]) <= 1e-6


@pytest.mark.parametrize("name", HEAVY)
def test_emulated_control_step(name):
    """C3, B = 4, N = 20: MPC iteration, policy at t0 and WBC against pyoracle.batch_step — 1e-6 per block, all statuses 0"""
    import emu_harness, pyoracle
    mb, st = rv.blobs(name); cfg = config("C3", 4, 20)
    e = emu_harness.Emu(mb, st, 4, 40, 2, cfg["ev"].shape[1])
    out, qps, _ = e.control_step(cfg)
    bad, xf, uf, w = pyoracle.batch_step(*rv.oracle_blobs(name), 2, cfg["t0"], cfg["horizon"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"], cfg["period"], cfg["time"])
    assert bad == 0 and (qps == 0).all() and (e.buf("status", (4,), np.int32) == 0).all()
    xd, ud = e.buf("wbc_x_des", (4, 30)), e.buf("wbc_u_des", (4, 30))
    assert np.array_equal(xd, cfg["x0"]) and np.abs(ud[:, 12:]).max() > 1e-6
    for b in range(4):
        assert_blocks(out[b], w[b], "wbc", TOL, b); assert_blocks(ud[b], uf[b], "u", TOL, b); assert_blocks(xd[b], xf[b], "x", TOL, b)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", HEAVY)
def test_emulated_wbc(name, variant):
    """wbc_cases.random_wbc_inputs (12) and hard_wbc_inputs (8) on the variant's oracle and blobs, both WBC variants: statuses [0, 0, 0] on both sides, 1e-6 per block;
    M, nle, J of the random cases as test_emu_kernels.test_wbc_kernel_vs_oracle holds them (1e-12)"""
    import emu_harness
    from wbc_cases import random_wbc_inputs, hard_wbc_inputs
    import offnominal_cases as OC
    o = rv.oracle(name); bl = rv.blobs(name)
    e = emu_harness.Emu(bl[0], bl[1], 12, 8, 2, 2)
    for what, cases in (("random", random_wbc_inputs(o, bl, 12, 31 + variant, 0.05)), ("hard", hard_wbc_inputs(o, bl, 8, 131 + variant))):
        arr = lambda k: np.array([c[k] for c in cases])
        e.wbc_reset(); e.wbc_step(arr("xd"), arr("il"), arr("rbd"), arr("mode"), 0.002, arr("time"), variant)
        out, st, dbg = e.wbc_step(arr("xd"), arr("ud"), arr("rbd"), arr("mode"), 0.002, arr("time"), variant)
        for b, c in enumerate(cases):
            o.wbc_reset(); o.wbc(c["xd"], c["il"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant))
            ref, sto, d = o.wbc(c["xd"], c["ud"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant), debug=True)
            assert list(sto) == [0, 0, 0], (what, b, sto)                              # gate
            assert list(st[b]) == list(sto), (what, b, st[b])
            assert rel_err(dbg[b]["M"], d["M"]) < 1e-12 and rel_err(dbg[b]["nle"], d["nle"]) < 1e-12 and rel_err(dbg[b]["J"], d["J"]) < 1e-12, (what, b)
            assert_blocks(out[b], ref, "wbc", TOL, (what, b))


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name", HEAVY)
def test_emulated_plant(name, nsub):
    """test_sim.test_emulated_plant_vs_oracle on the variant: 4 cases x 12 steps, the same bounds; the oracle's status is 0 and every case sees a contact"""
    import emu_harness
    from test_sim import random_cases
    o = rv.oracle(name); mb, st = rv.blobs(name)
    cases = random_cases(o, st, 4, 5); arr = lambda k: np.array([c[k] for c in cases])
    e = emu_harness.Emu(mb, st, 4, 8, 2, 2)
    e.sim_params(); e.sim_reset(arr("q"), arr("v"), 1.0); e.sim_command(arr("pos"), arr("vel"), arr("kp"), arr("kd"), arr("ff"))
    steps = 12; out = [e.sim_step(0.001, nsub) for _ in range(steps)]
    check_plant(o, cases, out, steps, nsub)


@pytest.mark.parametrize("name", HEAVY)
def test_emulated_ilqr_solve(name):
    """test_emu_kernels.test_ilqr_iteration_vs_oracle (cold call) on the variant, C2 with N = 20: the nonlinear rollouts of k_ilqr.h carry a forward kinematics of their own"""
    import emu_harness
    o = rv.oracle(name); mb, st = rv.blobs(name); cfg = config("C2", 1, 20)
    o.set_schedule(cfg["ev"][0], cfg["modes"][0]); o.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
    t0 = float(cfg["t0"][0]); r = o.ilqr_step(t0, t0 + cfg["horizon"], cfg["x0"][0]); n = len(r["t"]); assert r["warn"] == 0
    e = emu_harness.Emu(mb, st, 1, n + 4, 2, cfg["ev"].shape[1]); e.set_solver(1)
    trials = e.mpc_step(cfg)
    assert e.buf("status", (1,), np.int32)[0] == 0 and e.buf("n_nodes", (1,), np.int32)[0] == n
    perf = e.buf("out_perf", (10,))
    assert trials == r["ls_trials"] and perf[8] == r["alpha"] and r["alpha"] > 0.0
    assert_blocks(e.node_arr("xs", 30)[:n, 0], r["x"], "x", TOL); assert_blocks(e.node_arr("us", 30)[:n, 0], r["u"], "u", TOL)
    assert rel_err(perf[[0, 1, 3, 4, 5, 7]], r["perf"][[0, 1, 3, 4, 5, 7]]) < 1e-8 and abs(perf[2]) < 1e-12 and abs(perf[6]) < 1e-12


@pytest.mark.parametrize("name", HEAVY)
def test_emulated_ipm_solve(name):
    """test_ipm.test_product_ipm_on_the_emulator_vs_oracle (first iteration) on the variant, C2 with N = 20, ST_SOLVER = 3, ST_IPM_MU = 1e-2"""
    import emu_harness, pyoracle
    omb, ost = rv.oracle_blobs(name); mb, st = rv.blobs(name); ost = ost.copy(); st = st.copy()
    for s in (ost, st): s[L.ST_SOLVER] = 3.0; s[L.ST_IPM_MU] = 1e-2
    o = pyoracle.Oracle(omb, ost); cfg = config("C2", 1, 20); N = 20
    o.set_schedule(cfg["ev"][0], cfg["modes"][0]); o.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
    t0 = cfg["t0"][0]; r = o.ipm_step(t0, t0 + cfg["horizon"], cfg["x0"][0]); n = len(r["t"]); assert r["warn"] == 0
    e = emu_harness.Emu(mb, st, 1, N + 12, 2, cfg["ev"].shape[1]); e.set_solver(3)
    trials = e.mpc_step(cfg)
    assert e.buf("n_nodes", (1,), np.int32)[0] == n and e.buf("status", (1,), np.int32)[0] == 0
    info = e.buf("ipm_info", (1, 8))[0]; perf = e.buf("out_perf", (10,))
    assert trials == r["ls_trials"] and perf[8] == pytest.approx(r["alpha"], rel=1e-9)
    assert info[1] == pytest.approx(r["alpha_primal_max"], rel=1e-7) and info[2] == pytest.approx(r["alpha_dual_max"], rel=1e-7) and info[3] == pytest.approx(r["alpha_dual"], rel=1e-7) and info[4] == pytest.approx(r["barrier"], rel=1e-12)
    assert np.abs(perf[:8] - r["perf"][:8]).max() <= 1e-7 * max(1.0, np.abs(r["perf"][:8]).max())
    assert_blocks(e.node_arr("xs", 30)[:n, 0], r["x"], "x", TOL); assert_blocks(e.node_arr("us", 30)[:n, 0], r["u"], "u", TOL)
    s_dev = e.node_arr("ipm_s", 28)[:n - 1, 0]; l_dev = e.node_arr("ipm_l", 28)[:n - 1, 0]
    for i in range(n - 1):
        if r["ev"][i] == 1:
            continue
        p = o.ipm_node(i); on = p["on"] == 1
        assert np.abs(s_dev[i][on] - p["slack"][on]).max() <= 1e-6 * max(1.0, np.abs(p["slack"][on]).max()) and np.abs(l_dev[i][on] - p["dual"][on]).max() <= 1e-6 * max(1e-3, np.abs(p["dual"][on]).max()), i


# ---- the kernels with forward kinematics of their own: policy rollout (k_rollout.h), planned task space (k_plan.h) ----

def rollout_rows(plans):
    """the shapes of rollout_ref.row_set that ONE short plan can form (C2, N = 20: one gait event inside, so no span crosses two) — start on node 0 / mid-interval /
    exactly on the event / t_end == t0 / a longer span / t_end beyond the plan / late in the plan — and one that crosses the event, from half a step before it to half a
    step behind; each from a state off the plan by +-PERTURB, by a tenth of that, and not at all, in scrambled order.  Returns dict(inst, t0, x0, t_end, shape)"""
    import rollout_ref as rr
    pl, = plans; rng = np.random.default_rng(11); t = pl.res["t"]; tf = float(t[-1]); span = 6 * rr.DT
    te, = [float(e) for e in pl.ev_t if t[0] < e < tf]
    shapes = [("node0", float(t[0]), float(t[0]) + span), ("mid", float(t[0]) + 0.004, float(t[0]) + 0.004 + span), ("event", te, min(te + span, tf)),
              ("empty", float(t[3]) + 0.001, float(t[3]) + 0.001), ("long", float(t[0]) + 0.002, float(t[0]) + 0.002 + 1.5 * span), ("beyond", tf - 2.5 * rr.DT, tf + 1.5 * rr.DT),
              ("late", float(t[5]) + 0.007, float(t[5]) + 0.007 + span), ("across the event", te - 0.5 * rr.DT, te + 0.5 * rr.DT)]
    rows = []
    for what, a, e in shapes:
        for scale in (1.0, -1.0, 0.1, 0.0):
            xp, _ = pl.feed_forward(pl.query_time(a)); rows.append((a, xp + scale * rng.choice([-1.0, 1.0], 30) * rr.PERTURB, e, what))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return dict(inst=np.zeros(len(rows), np.int32), t0=np.array([r[0] for r in rows]), x0=np.array([r[1] for r in rows]), t_end=np.array([r[2] for r in rows]), shape=[r[3] for r in rows])


class RolloutWorld:
    """test_policy_rollout.World for one config: the oracle's solve laid out in the device's layout (node-major [nmax][B][k], stage records from
    feedback_ref.device_records) behind one context of tests/emu_rollout — the oracle on its blobs, the kernel on `blobs`"""
    NMAX = 36

    def __init__(self, lib, o, blobs, cfg):
        import ctypes as C
        import feedback_ref as fr, rollout_ref as rr
        self.lib = lib; self.mb = np.ascontiguousarray(blobs[0], float); self.st = np.ascontiguousarray(blobs[1], float); self.fric = float(self.st[L.ST_FRIC_COEF])
        lay = [lib.emu_rollout_layout(i) for i in range(6)]; nm = self.NMAX; ne = cfg["ev"].shape[1]
        r = oracle_solve(o, cfg); assert r["warn"] == 0
        K, _, _ = fr.oracle_gains(o, r); n = len(r["t"]); assert n + 3 <= nm
        self.n_nodes = np.array([n], np.int32); self.node_t = np.zeros((nm, 1)); self.node_ev = np.zeros((nm, 1), np.int32); self.xs = np.full((nm, 1, 30), np.nan); self.us = np.full((nm, 1, 30), np.nan)
        self.node_t[:n, 0] = r["t"]; self.node_ev[:n, 0] = r["ev"]; self.xs[:n, 0] = r["x"]; self.us[:n, 0] = r["u"]
        self.stage = np.ascontiguousarray(fr.device_records(o, r, lay, nm)[None]); self.ev = np.ascontiguousarray(cfg["ev"][:1], float); self.modes = np.ascontiguousarray(cfg["modes"][:1], np.int32)
        self.plans = [rr.Plan(r, K, self.ev[0], self.modes[0])]; p = rr.ptr
        self.h = C.c_void_p(lib.emu_rollout_create(p(self.mb), p(self.st), 1, nm, ne, p(self.n_nodes), p(self.node_t), p(self.node_ev), p(self.xs), p(self.us), p(self.ev), p(self.modes), p(self.stage)))
        lib.emu_rollout_set_state(self.h, 0, 0, 1)
        self.rows = rollout_rows(self.plans)

    def call(self, rows, max_step, max_steps, feedback, **kw):
        import rollout_ref as rr
        return rr.call(self.lib.emu_rollout, self.h, rows, max_step, max_steps, feedback, **kw)

    def error(self):
        return self.lib.emu_rollout_last_error(self.h).decode()


@pytest.mark.parametrize("feedback", [0, 1])
@pytest.mark.parametrize("name", HEAVY)
def test_emulated_policy_rollout(name, feedback):
    """test_policy_rollout.test_rows_against_the_reference on a C2 plan (N = 20) of the variant's oracle, the kernel on the product's blobs: rollout_ref.check_rows at
    the default step, feed-forward and feedback"""
    import rollout_ref as rr
    o = rv.oracle(name)
    w = RolloutWorld(rr.emu_lib(), o, rv.blobs(name), config("C2", 1, 20))
    try:
        max_step, max_steps, what = rr.CALLS[0]
        rc, out, _ = w.call(w.rows, max_step, max_steps, feedback, cap=40); assert rc == 0, w.error()
        worst = rr.check_rows(o, w.plans, w.fric, w.rows, out, max_step, max_steps, feedback, 0, "%s %s, feedback %d" % (name, what, feedback))
        print(name, what, "feedback", feedback, {k: "%.2e" % v for k, v in worst.items()})
        if feedback: assert out["summary"]["max_fb"].max() > 1e-3
        else: assert not out["summary"]["max_fb"].any()
        assert out["summary"]["events"].max() >= 1 and out["summary"]["steps"].max() >= 6 and (out["summary"]["steps"] == 0).any()
    finally:
        w.lib.emu_rollout_destroy(w.h)


def emulated_plan(lib, o, mb, gaits, cap):
    """test_plan_task_space.Batch for the solves of `gaits` [(template, intervals, seed)], one instance each: the oracle's solves in the device's layout (NaN / -1 where the
    solver would hold stale data) through emu_plan_solution on the model blob `mb`.  Returns (solves, records [B][nmax], num_nodes, footholds [B][cap], count)"""
    import plan_ref as pf
    from qm_control_amd import api
    solves = []
    for gait, N, seed in gaits:
        cfg = scenarios.gait_config(gait, batch=1, n_intervals=N, seed=seed); r = oracle_solve(o, cfg); n = len(r["t"]); assert r["warn"] == 0
        ee = np.array([np.concatenate(o.desired_state(t)[1:]) for t in r["t"]])
        solves.append(dict(cfg=cfg, res=r, n=n, ee=ee, ref=pf.plan(o, cfg["ref_t"][0], cfg["ref_x"][0], r["t"], r["x"], r["u"], r["mode"]), fh=pf.footholds(o, r["t"], r["x"], cfg["ev"][0], cfg["modes"][0])))
    B = len(solves); nm = max(s["n"] for s in solves) + 3; ne = max(s["cfg"]["ev"].shape[1] for s in solves)
    n_nodes = np.zeros(B, np.int32); node_t = np.full((nm, B), np.nan); node_ev = np.full((nm, B), -1, np.int32); node_mode = np.full((nm, B), -1, np.int32)
    xs = np.full((nm, B, 30), np.nan); us = np.full((nm, B, 30), np.nan); eeref = np.full((nm, B, 7), np.nan); ev = np.zeros((B, ne)); modes = np.full((B, ne + 1), 15, np.int32)
    for b, s in enumerate(solves):
        r = s["res"]; n = s["n"]; e = s["cfg"]["ev"][0]; m = s["cfg"]["modes"][0]
        n_nodes[b] = n; node_t[:n, b] = r["t"]; node_ev[:n, b] = r["ev"]; node_mode[:n, b] = r["mode"]; xs[:n, b] = r["x"]; us[:n, b] = r["u"]; eeref[:n, b] = s["ee"]
        ev[b, :len(e)] = e; ev[b, len(e):] = e[-1] + 1e3 * np.arange(1, ne - len(e) + 1); modes[b, :len(m)] = m; modes[b, len(m):] = m[-1]
    rec = np.zeros((B, nm), api.PLAN_RECORD); rec.view(np.uint8)[:] = 0xff; nn = np.full(B, -7, np.int32); fh = np.zeros((B, cap), api.FOOTHOLD); cnt = np.full(B, -7, np.int32)
    lib.emu_plan_solution(pf.ptr(mb), B, nm, ne, pf.ptr(n_nodes), pf.ptr(node_t), pf.ptr(node_ev), pf.ptr(node_mode), pf.ptr(xs), pf.ptr(us), pf.ptr(eeref), pf.ptr(ev), pf.ptr(modes), pf.ptr(rec), pf.ptr(nn), cap, pf.ptr(fh), pf.ptr(cnt))
    assert np.array_equal(nn, n_nodes)
    return solves, rec, nn, fh, cnt


@pytest.mark.parametrize("name", HEAVY)
def test_emulated_plan_task_space_and_footholds(name):
    """test_plan_task_space on the variant: node records and footholds of a trot and a flying-trot solve (both CoP branches), and 48 random state rows (random base
    attitude, every mode) — plan_ref.compare / compare_footholds on the variant's oracle, the kernels on the product's model blob"""
    import plan_ref as pf
    from qm_control_amd import api
    o = rv.oracle(name); bl = rv.blobs(name); lib = pf.emu_lib(); mb = np.ascontiguousarray(bl[0])
    solves, rec, nn, fh, cnt = emulated_plan(lib, o, mb, [("trot", 20, 7), ("flying_trot", 20, 9)], 16); mx = {}; mf = 0.0
    for b, s in enumerate(solves):
        n = s["n"]; assert not rec[b, n:].tobytes().strip(b"\0"), b
        mx = pf.merge(mx, pf.compare(rec[b, :n], s["ref"], "%s instance %d" % (name, b))); mf = max(mf, pf.compare_footholds(fh[b], cnt[b], s["fh"], 16, "%s instance %d" % (name, b)))
    live = np.concatenate([rec[b, :s["n"]] for b, s in enumerate(solves)])
    assert (live["contact_mask"] == 0).any() and (live["cop"][:, 2] > 1.0).any() and cnt.sum() > 0
    R = 48; x, u, mode, ee = pf.random_states(bl, R, 3)
    got = np.zeros(R, api.PLAN_RECORD); got.view(np.uint8)[:] = 0xff
    lib.emu_plan_eval(pf.ptr(mb), R, pf.ptr(np.ascontiguousarray(x)), pf.ptr(u), pf.ptr(np.ascontiguousarray(mode, np.int32)), pf.ptr(ee), pf.ptr(got))
    ref = np.array([pf.record(o, x[r], u[r], mode[r], (ee[r, :3], ee[r, 3:])) for r in range(R)])
    mx = pf.merge(mx, pf.compare(got, ref, name + " state rows"))
    print(name, "plan records: max abs differences", {k: "%.1e" % v for k, v in sorted(mx.items())}, "footholds %.1e (%d landings)" % (mf, cnt.sum()))
