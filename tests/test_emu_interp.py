"""Grid, target and policy interpolation at their edges: K0b (qm_grid_nodes_kernel), K5 (qm_policy_kernel) and qm_advance_kernel on the host emulator
against the oracle (CPU twin of tests/test_gpu_interp.py; cases in tests/interp_cases.py).

Measured on the emulator, K0b's largest errors over every node of every case (scaled by max(|oracle value|, 1)): zpos 5.6e-17, zvel 8.9e-16, xref 1.2e-16,
eeref 1.1e-16 (the tolerance is 1e-12).  The policy is held to 1e-15 relative against the numpy restatement on the emulator's own primal solution."""
import numpy as np
import pytest
import emu_harness
import interp_cases as ic
from blocks import assert_blocks


def _emu(blobs, B, nmax, nref, nev):
    return emu_harness.Emu(blobs[0], blobs[1], B, nmax, nref, nev)


def _k0b(e, B):
    return ic.read_k0b(lambda name, k, dt: e.buf(name, (B,), dt) if k == 0 else e.node_arr(name, k, dt), B)


def _solution(e, B):
    n = e.buf("n_nodes", (B,), np.int32); t = e.node_arr("node_t", 1); ev = e.node_arr("node_ev", 1, np.int32); md = e.node_arr("node_mode", 1, np.int32)
    xs = e.node_arr("xs", 30); us = e.node_arr("us", 30)
    return [dict(t=t[:n[b], b], ev=ev[:n[b], b], mode=md[:n[b], b], x=xs[:n[b], b], u=us[:n[b], b]) for b in range(B)]


def _check_solve(res, ora, what, tol=1e-6):
    assert np.array_equal(res["t"], ora["t"]) and np.array_equal(res["ev"], ora["ev"]) and np.array_equal(res["mode"], ora["mode"]), what
    assert_blocks(res["x"], ora["x"], "x", tol, what); assert_blocks(res["u"], ora["u"], "u", tol, what)


def test_case_builders():
    """the cases take the branches they are named after"""
    d = ic.slerp_dots(); one = 1.0 - ic.LIMIT_EPS
    assert abs(d["identical"]) >= one and d["negated"] <= -one
    assert d["dot_negative"] < 0.0 and -one < d["near_antipodal"] < -(1.0 - 1e-8) and abs(d["near_pi"]) < 1e-3 and 1.0 - 1e-14 < d["tiny_angle"] < one
    cfg = ic.base_config(); cases = ic.target_cases(cfg)
    t, e = ic.node_grid(float(cfg["t0"][0]), float(cfg["horizon"]), cfg["ev"][0])
    ts = np.where(e == 2, t + ic.WEAK_EPS, t)
    rt = cases["k6_dup"][0]
    assert rt[0] == rt[1] == cfg["t0"][0]                                                 # node 0 in the zero-length interval 0 (till == len == 0)
    gaps = np.diff(rt); near = [k for k in range(len(gaps)) if 0.0 < gaps[k] <= 2 * ic.WEAK_EPS]
    assert near and any(np.any((ts > rt[k]) & (ts <= rt[k + 1]) & (rt[k + 1] - ts < 0.5 * gaps[k])) for k in near)      # a node past the midpoint
    rt2 = cases["k6_near"][0]; g2 = np.diff(rt2); near2 = [k for k in range(len(g2)) if 0.0 < g2[k] <= 2 * ic.WEAK_EPS]
    assert any(np.any((ts > rt2[k]) & (ts <= rt2[k + 1]) & (rt2[k + 1] - ts > 0.5 * g2[k])) for k in near2)               # a node before the midpoint
    assert np.isin(rt, ts[e == 2]).any() and np.isin(rt2, t[e == 0]).any()                # knots on a PostEvent ts and on a plain node time
    assert cases["k3_inside"][0][0] > t[0] and cases["k3_inside"][0][-1] < t[-1] and cases["k3_late"][0][0] > t[0] and cases["k3_early"][0][-1] < t[-1]
    t0, dt = ic.warm_chain_to_event(); assert t0 + dt == ic.EVENT


def test_oracle_sign_flip_invariance(oblobs):
    """negating knot quaternions negates the oracle's EE orientation error g and leaves the Gauss-Newton cost, gradient and Hessian unchanged: x*, u* bit-identical"""
    cfg = ic.base_config(); cases = ic.target_cases(cfg)
    mb, st = oblobs
    import pyoracle
    o = pyoracle.Oracle(mb, st)
    x = cfg["x0"][0]; rt, rx = cases["k3"]
    for q in (rx[1, 33:37], cases["k2_dot_negative"][1][1, 33:37]):
        assert np.array_equal(o.ee_pose_error(x, rx[1, 30:33], -q)[3:], -o.ee_pose_error(x, rx[1, 30:33], q)[3:])
    for name in ("k3", "k6_dup"):
        rt, rx = cases[name]; sols = []
        for flip in (None, [1], "all"):
            o.set_schedule(cfg["ev"][0], cfg["modes"][0]); o.set_target(rt, rx if flip is None else ic.flip_quats(rx, flip))
            sols.append(o.mpc_step(cfg["t0"][0], cfg["t0"][0] + cfg["horizon"], x))
        for s in sols[1:]:
            assert np.array_equal(s["x"], sols[0]["x"]) and np.array_equal(s["u"], sols[0]["u"]), name


# the target matrix by context size: (max_ref_knots, cases); cases with fewer knots are padded by repeating their last knot
NREF_GROUPS = [(1, ["k1"]), (2, ["k2_identical", "k2_negated", "k2_dot_negative", "k2_near_antipodal", "k2_near_pi", "k2_tiny_angle"]),
               (3, ["k3", "k3_inside", "k3_late", "k3_early", "k2_tiny_angle"]), (6, ["k6_dup", "k6_near", "k1", "k2_near_antipodal", "k3_late", "k3_inside"])]
SOLVE_SUBSET = {1: ["k1"], 2: ["k2_dot_negative", "k2_near_pi"], 3: ["k3_inside", "k2_tiny_angle"], 6: ["k6_dup", "k6_near", "k3_inside"]}


@pytest.mark.parametrize("nref,names", NREF_GROUPS, ids=["nref%d" % g[0] for g in NREF_GROUPS])
def test_k0b_target_matrix(blobs, oblobs, nref, names):
    """K0b's per-node outputs of every target case against the oracle entry by entry (integers and node_ts / node_dt bit-exact, references to 1e-12); the
    iteration leaves them as K0b wrote them; whole solves of a subset against the oracle on the unpadded knots (x*, u* 1e-6 per block, integers exact)"""
    cfg1 = ic.base_config(); cases = ic.target_cases(cfg1)
    cfg = ic.batch_of(cfg1, [ic.pad_target(*cases[k], nref) for k in names]); B = cfg["B"]
    e = _emu(blobs, B, 64, nref, cfg["ev"].shape[1])
    e.grid_only(cfg); out = _k0b(e, B)
    for b, k in enumerate(names):
        ic.check_k0b(ic.oracle_for(oblobs, cfg, b), cfg, out, b, "%s (nref %d)" % (k, nref))      # the oracle holds the same (padded) knots
    sub = [b for b, k in enumerate(names) if k in SOLVE_SUBSET[nref]]
    cs = {k: (v[sub] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in cfg.items()}; cs["B"] = len(sub)
    e2 = _emu(blobs, len(sub), 64, nref, cfg["ev"].shape[1]); e2.mpc_step(cs)
    after = _k0b(e2, len(sub)); first = {k: (v[..., sub] if v.ndim == 1 else v[:, sub]) for k, v in out.items()}
    for k in first:
        assert np.array_equal(after[k], first[k]), k                                     # no later kernel overwrites K0b's outputs
    res = _solution(e2, len(sub))
    for j, b in enumerate(sub):
        o = ic.oracle_for(oblobs, dict(cfg, ref_t=[cases[names[b]][0]] * B, ref_x=[cases[names[b]][1]] * B), b)      # the unpadded knots
        _check_solve(res[j], o.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b]), "%s (nref %d)" % (names[b], nref))


def test_k0b_gait_templates_and_c5(blobs, oblobs):
    """K0b on all 12 gait templates (4 instances each, N = 60) and on C5 (trot - stance - trot, rotated EE targets, N = 150) against the oracle"""
    from qm_control_amd import scenarios
    cfgs = [scenarios.gait_config(g, batch=4, n_intervals=60) for g in scenarios.load_gaits()] + [scenarios.make_config("C5", batch=16)]
    for cfg in cfgs:
        B = cfg["B"]; e = _emu(blobs, B, 200, cfg["ref_t"].shape[1], cfg["ev"].shape[1]); e.grid_only(cfg); out = _k0b(e, B)
        st = e.buf("status", (B,), np.int32)
        for b in range(B):
            assert st[b] == 0, (cfg["name"], b)
            ic.check_k0b(ic.oracle_for(oblobs, cfg, b), cfg, out, b, "%s #%d" % (cfg["name"], b))


def test_quaternion_sign_flip_invariance(blobs):
    """negating one knot's quaternion, or all of them, leaves the product's x*, u* bit-identical (the EE cost is even in the orientation error): a check that
    does not lean on the oracle"""
    cfg1 = ic.base_config(); cases = ic.target_cases(cfg1)
    rt, rx = cases["k6_dup"]; rt3, rx3 = ic.pad_target(*cases["k3"], 6)
    tg = [(rt, rx), (rt, ic.flip_quats(rx, [2])), (rt, ic.flip_quats(rx, "all")), (rt3, rx3), (rt3, ic.flip_quats(rx3, [1]))]
    cfg = ic.batch_of(cfg1, tg); e = _emu(blobs, 5, 64, 6, cfg["ev"].shape[1]); e.mpc_step(cfg)
    res = _solution(e, 5); ee = e.node_arr("eeref", 7)
    for b, ref in ((1, 0), (2, 0), (4, 3)):
        assert np.array_equal(res[b]["x"], res[ref]["x"]) and np.array_equal(res[b]["u"], res[ref]["u"]), b
        assert np.array_equal(np.abs(ee[:, b]), np.abs(ee[:, ref])), b                   # the interpolated quaternion only changes sign


def _sweep(e, cfg, oblobs, b=0):
    """K5 at every sweep time: against the oracle (1e-6 per block, modes exact) and against the numpy restatement on the product's own primal solution"""
    B = e.B; sol = _solution(e, B)[b]
    o = ic.oracle_for(oblobs, cfg, b); t0 = float(cfg["t0"][b]); tf = t0 + float(cfg["horizon"])
    ora = o.mpc_step(t0, tf, cfg["x0"][b])
    times = ic.policy_times(sol["t"], sol["ev"], cfg["ev"][b], t0, tf)
    worst = 0.0
    for t in times:
        tv = np.full(B, t); xd, ud, md = e.policy_eval(tv)
        xo, uo, mo = o.eval_policy(t)
        assert md[b] == mo, t
        assert_blocks(xd[b], xo, "x", 1e-6, "policy x at %r" % t); assert_blocks(ud[b], uo, "u", 1e-6, "policy u at %r" % t)
        xr, ur = ic.policy_reference(sol["t"], sol["ev"], sol["x"], sol["u"], t)
        for d, r in ((xd[b], xr), (ud[b], ur)):
            worst = max(worst, float(np.abs(d - r).max() / np.abs(r).max()))
    assert worst <= 1e-15, worst
    return len(times)


def test_policy_sweep(blobs, oblobs):
    """C2 (N = 40): the policy at every node time with its neighbours and nudges, at every event time ±limitEpsilon / ±2 limitEpsilon / ±weakEpsilon, before t0
    and past tf"""
    cfg = ic.base_config(); e = _emu(blobs, 1, 64, 2, cfg["ev"].shape[1]); e.mpc_step(cfg)
    assert _sweep(e, cfg, oblobs) > 300


def test_policy_sweep_degenerate_grid(blobs, oblobs):
    """the sweep on a warned degenerate grid (a node 5e-7 s before a gait event: test_grid_fuzz.degenerate_cases)"""
    from test_grid_fuzz import degenerate_cases
    cfgd, cases = degenerate_cases(ic.base_config(), full=False)
    k = [c[1] for c in cases].index(-5e-7)
    cfg = {kk: (v[k:k + 1] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == cfgd["B"] else v) for kk, v in cfgd.items()}; cfg["B"] = 1
    e = _emu(blobs, 1, 64, 2, cfg["ev"].shape[1]); e.mpc_step(cfg)
    assert e.buf("step_info", (1, 4))[0, 3] == 1.0                                        # the warning bit (non-positive pivots zeroed)
    _sweep(e, cfg, oblobs)


def _event_cfg(cfg1, t0s):
    B = len(t0s)
    cfg = {k: (np.repeat(v[:1], B, axis=0) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 1 else v) for k, v in cfg1.items()}
    cfg["B"] = B; cfg["t0"] = np.array(t0s); cfg["ref_t"] = cfg1["ref_t"][0][None, :] + (cfg["t0"] - cfg1["t0"][0])[:, None]
    return cfg


def test_t0_on_event(blobs, oblobs):
    """cold solves with t0 on the trot event at 0.35 and next to it (0, ±limitEpsilon, ±5e-7, ±weakEpsilon): grid, K0b, x*, u* and the warning bit against the oracle"""
    cfg = _event_cfg(ic.base_config(), [t for _, t in ic.t0_on_event_cases()]); B = cfg["B"]
    assert cfg["t0"][0] == ic.EVENT and ic.EVENT in cfg["ev"][0]
    e = _emu(blobs, B, 64, 2, cfg["ev"].shape[1]); e.mpc_step(cfg)
    out = _k0b(e, B); res = _solution(e, B); si = e.buf("step_info", (B, 4))
    for b, (off, t0) in enumerate(ic.t0_on_event_cases()):
        what = "t0 = event %+g" % off; o = ic.oracle_for(oblobs, cfg, b)
        ora = o.mpc_step(t0, t0 + cfg["horizon"], cfg["x0"][b])
        ic.check_k0b(o, cfg, out, b, what)
        _check_solve(res[b], ora, what)
        assert (si[b, 3] == 1.0) == (ora["warn"] != 0), what
    assert si[[off for off, _ in ic.t0_on_event_cases()].index(-5e-7), 3] == 1.0


def test_warm_chain_lands_on_event(blobs, oblobs):
    """cold solve at t0, the perfect-tracking advance by dt with t0 + dt == the event exactly, then the warm-started K0: the advanced t0 / x0, the warm initial
    guess (entry by entry) and the warm solve against the oracle's"""
    t0, dt = ic.warm_chain_to_event()
    cfg = _event_cfg(ic.base_config(), [t0]); hz = cfg["horizon"]
    e = _emu(blobs, 1, 64, 2, cfg["ev"].shape[1])
    e.grid_only(cfg)
    o = ic.oracle_for(oblobs, cfg, 0); o.mpc_step(t0, t0 + hz, cfg["x0"][0])
    xg, ug = o.initial_guess(); n = len(xg)
    assert_blocks(e.node_arr("x", 30)[:n, 0], xg, "x", 0.0, "cold guess x"); assert_blocks(e.node_arr("u", 30)[:n - 1, 0], ug, "u", 0.0, "cold guess u")
    e.mpc_iterate(); sol0 = _solution(e, 1)[0]
    e.advance(dt)
    t1 = e.buf("t0", (1,))[0]; x1 = e.buf("x0", (1, 30))[0]
    assert t1 == ic.EVENT
    xr, _ = ic.policy_reference(sol0["t"], sol0["ev"], sol0["x"], sol0["u"], t1)
    assert np.array_equal(x1, xr)                                                          # qm_advance_kernel: the policy state at the new t0
    e.grid_warm(hz)
    ora = o.mpc_step(t1, t1 + hz, x1, warm=True); xg, ug = o.initial_guess(); n = len(xg)
    out = _k0b(e, 1); ic.check_k0b(o, dict(cfg, t0=np.array([t1])), out, 0, "warm on the event")
    assert_blocks(e.node_arr("x", 30)[:n, 0], xg, "x", 1e-6, "warm guess x"); assert_blocks(e.node_arr("u", 30)[:n - 1, 0], ug, "u", 1e-6, "warm guess u")
    e.mpc_iterate(); _check_solve(_solution(e, 1)[0], ora, "warm solve on the event")


def test_batch_layout_grid(blobs, oblobs):
    """K0 / K0b per-instance outputs bit-identical whether an instance runs alone or at batch positions that straddle 64-lane boundaries (B = 1, 63, 65, 130),
    with the longest grid in the last, partial wave and max_nodes equal to its node count"""
    cfg, nmax = ic.layout_instances(); ref = []
    for b in range(cfg["B"]):
        c1 = {k: (v[b:b + 1] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == cfg["B"] else v) for k, v in cfg.items()}
        c1["B"] = 1; e = _emu(blobs, 1, nmax, 6, cfg["ev"].shape[1]); e.grid_only(c1); out = _k0b(e, 1)
        if b == cfg["B"] - 1:
            ic.check_k0b(ic.oracle_for(oblobs, c1, 0), c1, out, 0, "event burst")
        out["x"] = e.node_arr("x", 30); out["u"] = e.node_arr("u", 30)
        ref.append({k: (v[0] if v.ndim == 1 else v[:int(out["n_nodes"][0]), 0]) for k, v in out.items()})
    assert int(ref[-1]["n_nodes"]) == nmax
    for B, pos in ic.LAYOUTS.items():
        if pos is None: continue
        e = _emu(blobs, B, nmax, 6, cfg["ev"].shape[1]); e.grid_only(ic.place(cfg, B, pos)); out = _k0b(e, B)
        out["x"] = e.node_arr("x", 30); out["u"] = e.node_arr("u", 30)
        for j, b in enumerate(pos):
            for k, v in out.items():
                assert np.array_equal(v[b] if v.ndim == 1 else v[:int(out["n_nodes"][b]), b], ref[j][k]), (B, b, k)
