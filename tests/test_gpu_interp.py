"""Grid, target and policy interpolation at their edges on the device: K0b (qm_grid_nodes_kernel), K5 (qm_policy_kernel) and qm_advance_kernel through the
C ABI against the oracle (cases in tests/interp_cases.py; host-emulated twin: tests/test_emu_interp.py).

The device differs from the emulator in its libm (ocml acos / sin in the slerp) and in floating-point contraction.  Measured on an MI355X, K0b's largest
errors over the target matrix, the 12 gait templates, C5, the t0-on-event cases and the event burst (scaled by max(|oracle value|, 1)): zpos 1.1e-16,
zvel 1.6e-15, xref 0, eeref 2.2e-16 (the tolerance is 1e-12); the policy against the numpy restatement on the device's own primal solution: 2.1e-16
relative (tolerance 1e-15).  Run with -s to print the maxima."""
import numpy as np
import pytest
import interp_cases as ic
from blocks import assert_blocks

pytestmark = pytest.mark.gpu

class Ctx:
    def __init__(self, blobs, B, nmax, nref, nev):
        from qm_control_amd import api
        self.itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=nmax, max_ref_knots=nref, max_events=nev)
        self.mpc = api.SqpMpc(self.itf); self.nmax = nmax

    def solve(self, cfg, B=None):
        B = cfg["B"] if B is None else B
        self.mpc.set_problem(cfg["t0"][:B], cfg["x0"][:B], cfg["ref_t"][:B], cfg["ref_x"][:B], cfg["ev"][:B], cfg["modes"][:B])
        self.mpc.solve_resident(cfg["horizon"])
        return self.mpc.download()

    def node(self, name, k, dt=np.float64):
        B = self.mpc.B
        if k == 0: return self.itf.debug_read(name, (B,), dt)
        return self.itf.debug_read(name, (self.nmax, B) if k == 1 else (self.nmax, B, k), dt)

    def k0b(self):
        out = ic.read_k0b(self.node, self.mpc.B); out["x"] = self.node("x", 30); out["u"] = self.node("u", 30)      # x / u: the initial guess (one SQP iteration: never committed)
        return out

    def close(self):
        self.itf.close()


def _sol(res, b):
    n = int(res["num_nodes"][b])
    return dict(t=res["t"][b, :n], ev=res["event"][b, :n], mode=res["mode"][b, :n], x=res["x"][b, :n], u=res["u"][b, :n], status=int(res["status"][b]))


def _check_solve(r, ora, what):
    assert np.array_equal(r["t"], ora["t"]) and np.array_equal(r["ev"], ora["ev"]) and np.array_equal(r["mode"], ora["mode"]), what
    assert_blocks(r["x"], ora["x"], "x", 1e-6, what); assert_blocks(r["u"], ora["u"], "u", 1e-6, what)


_MAX = {}


def _record(mx):
    for k, v in mx.items(): _MAX[k] = max(_MAX.get(k, 0.0), v)
    print("K0b scaled maxima so far: " + ", ".join("%s %.1e" % kv for kv in sorted(_MAX.items())))


def _sub(cfg, idx):
    out = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == cfg["B"] else v) for k, v in cfg.items()}; out["B"] = len(idx)
    return out


NREF_GROUPS = [(1, ["k1"]), (2, ["k2_identical", "k2_negated", "k2_dot_negative", "k2_near_antipodal", "k2_near_pi", "k2_tiny_angle"]),
               (3, ["k3", "k3_inside", "k3_late", "k3_early", "k2_tiny_angle", "k1"]),
               (6, ["k6_dup", "k6_near", "k1", "k2_negated", "k2_dot_negative", "k2_near_antipodal", "k2_near_pi", "k2_tiny_angle", "k3", "k3_inside", "k3_late", "k3_early"])]


@pytest.mark.parametrize("nref,names", NREF_GROUPS, ids=["nref%d" % g[0] for g in NREF_GROUPS])
def test_target_matrix(blobs, oblobs, nref, names):
    """every target case in a context of nref knot slots (fewer knots padded by repeating the last one): K0b's outputs entry by entry against the oracle after the
    solve (integers, node_ts, node_dt bit-exact; references to 1e-12), the cold initial guess exactly, x*, u* to 1e-6 per block against the oracle on the padded
    and on the unpadded knots"""
    cfg1 = ic.base_config(); cases = ic.target_cases(cfg1)
    cfg = ic.batch_of(cfg1, [ic.pad_target(*cases[k], nref) for k in names]); B = cfg["B"]
    c = Ctx(blobs, B, 64, nref, cfg["ev"].shape[1]); res = c.solve(cfg); out = c.k0b()
    for b, k in enumerate(names):
        what = "%s (nref %d)" % (k, nref)
        o = ic.oracle_for(oblobs, cfg, b)                                                    # the same (padded) knots
        _record(ic.check_k0b(o, cfg, out, b, what))
        ora = o.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b]); xg, ug = o.initial_guess(); n = len(xg)
        assert np.array_equal(out["x"][:n, b], xg) and np.array_equal(out["u"][:n - 1, b], ug), what
        assert res["status"][b] == 0, what
        _check_solve(_sol(res, b), ora, what)
        if len(cases[k][0]) < nref:                                                          # padding does not change the solve
            o1 = ic.oracle_for(oblobs, dict(cfg, ref_t=[cases[k][0]] * B, ref_x=[cases[k][1]] * B), b)
            _check_solve(_sol(res, b), o1.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b]), what + " vs the unpadded target")
    c.close()


def test_gait_templates_and_c5(blobs, oblobs):
    """K0b on all 12 gait templates (4 instances each, N = 60) and on C5 (64 instances, N = 150) against the oracle"""
    from qm_control_amd import scenarios
    cfgs = [scenarios.gait_config(g, batch=4, n_intervals=60) for g in scenarios.load_gaits()] + [scenarios.make_config("C5", batch=64)]
    for cfg in cfgs:
        B = cfg["B"]; c = Ctx(blobs, B, 200, cfg["ref_t"].shape[1], cfg["ev"].shape[1]); res = c.solve(cfg); out = c.k0b()
        for b in range(B):
            assert res["status"][b] >= 0, (cfg["name"], b)
            _record(ic.check_k0b(ic.oracle_for(oblobs, cfg, b), cfg, out, b, "%s #%d" % (cfg["name"], b)))
        c.close()


def test_quaternion_sign_flip_invariance(blobs):
    """negating one knot's quaternion, or all of them, leaves x*, u* bit-identical (the EE cost is even in the orientation error; a check independent of the oracle)"""
    cfg1 = ic.base_config(); cases = ic.target_cases(cfg1)
    tg, groups = [], []
    for name in ("k6_dup", "k6_near", "k3", "k2_dot_negative", "k2_near_antipodal"):
        rt, rx = ic.pad_target(*cases[name], 6); first = len(tg)
        tg += [(rt, rx), (rt, ic.flip_quats(rx, [len(cases[name][0]) // 2])), (rt, ic.flip_quats(rx, "all"))]; groups.append((name, first))
    cfg = ic.batch_of(cfg1, tg); c = Ctx(blobs, cfg["B"], 64, 6, cfg["ev"].shape[1]); res = c.solve(cfg); ee = c.node("eeref", 7)
    for name, f in groups:
        for b in (f + 1, f + 2):
            n = int(res["num_nodes"][f]); assert res["num_nodes"][b] == n and res["status"][b] == 0, (name, b)
            assert np.array_equal(res["x"][b, :n], res["x"][f, :n]) and np.array_equal(res["u"][b, :n], res["u"][f, :n]), (name, b)
            assert np.array_equal(np.abs(ee[:n, b]), np.abs(ee[:n, f])), (name, b)
    c.close()


def _sweep(c, res, cfg, oblobs, b=0):
    """K5 with one sweep time per instance (every instance holds the same solve): against the oracle (1e-6 per block, modes exact) and against the numpy
    restatement of timeSegment + the limitEpsilon nudges on the device's own downloaded t / event / x / u (<= 1e-15 relative)"""
    B = c.mpc.B; sol = _sol(res, b)
    n = len(sol["t"])
    for j in range(B):
        assert res["num_nodes"][j] == n and np.array_equal(res["x"][j, :n], sol["x"]) and np.array_equal(res["u"][j, :n], sol["u"])
    o = ic.oracle_for(oblobs, cfg, b); t0 = float(cfg["t0"][b]); tf = t0 + float(cfg["horizon"]); o.mpc_step(t0, tf, cfg["x0"][b])
    times = ic.policy_times(sol["t"], sol["ev"], cfg["ev"][b], t0, tf); worst = 0.0
    for s in range(0, len(times), B):
        tv = np.resize(times[s:s + B], B); xd, ud, md = c.mpc.evaluatePolicy(tv)
        for j in range(min(B, len(times) - s)):
            t = tv[j]; xo, uo, mo = o.eval_policy(t)
            assert md[j] == mo, t
            assert_blocks(xd[j], xo, "x", 1e-6, "policy x at %r" % t); assert_blocks(ud[j], uo, "u", 1e-6, "policy u at %r" % t)
            xr, ur = ic.policy_reference(sol["t"], sol["ev"], sol["x"], sol["u"], t)
            for d, r in ((xd[j], xr), (ud[j], ur)):
                worst = max(worst, float(np.abs(d - r).max() / np.abs(r).max()))
    print("policy vs restatement on the device's solution: %.1e relative" % worst)
    assert worst <= 1e-15, worst
    return len(times)


def test_policy_sweep(blobs, oblobs):
    """C2 (N = 40), 64 copies: the policy at every node time with its neighbours and nudges, at every event time ±limitEpsilon / ±2 limitEpsilon / ±weakEpsilon,
    before t0 and past tf"""
    cfg = ic.batch_of(ic.base_config(), [(ic.base_config()["ref_t"][0], ic.base_config()["ref_x"][0])] * 64)
    c = Ctx(blobs, 64, 64, 2, cfg["ev"].shape[1]); res = c.solve(cfg)
    assert (res["status"] == 0).all() and _sweep(c, res, cfg, oblobs) > 300
    c.close()


def test_policy_sweep_degenerate_grid(blobs, oblobs):
    """the sweep on a warned degenerate grid (a node 5e-7 s before a gait event: test_grid_fuzz.degenerate_cases)"""
    from test_grid_fuzz import degenerate_cases
    from qm_control_amd import layout as L
    cfgd, cases = degenerate_cases(ic.base_config(), full=False)
    k = [cc[1] for cc in cases].index(-5e-7); cfg = _sub(cfgd, [k] * 64)
    c = Ctx(blobs, 64, 64, 2, cfg["ev"].shape[1]); res = c.solve(cfg)
    assert (res["status"] == L.QM_MPC_WARN_PIVOT).all()
    _sweep(c, res, cfg, oblobs)
    c.close()


def _event_cfg(cfg1, t0s):
    cfg = _sub(cfg1, [0] * len(t0s)); cfg["t0"] = np.array(t0s); cfg["ref_t"] = cfg1["ref_t"][0][None, :] + (cfg["t0"] - cfg1["t0"][0])[:, None]
    return cfg


def test_t0_on_event(blobs, oblobs):
    """cold solves with t0 on the trot event at 0.35 and next to it (0, ±limitEpsilon, ±5e-7, ±weakEpsilon): K0b, x*, u* and the warning bit against the oracle"""
    from qm_control_amd import layout as L
    cfg = _event_cfg(ic.base_config(), [t for _, t in ic.t0_on_event_cases()]); B = cfg["B"]
    assert cfg["t0"][0] == ic.EVENT and ic.EVENT in cfg["ev"][0]
    c = Ctx(blobs, B, 64, 2, cfg["ev"].shape[1]); res = c.solve(cfg); out = c.k0b()
    for b, (off, t0) in enumerate(ic.t0_on_event_cases()):
        what = "t0 = event %+g" % off; o = ic.oracle_for(oblobs, cfg, b)
        ora = o.mpc_step(t0, t0 + cfg["horizon"], cfg["x0"][b])
        _record(ic.check_k0b(o, cfg, out, b, what))
        _check_solve(_sol(res, b), ora, what)
        assert res["status"][b] == (L.QM_MPC_WARN_PIVOT if ora["warn"] else 0), what
    assert res["status"][[off for off, _ in ic.t0_on_event_cases()].index(-5e-7)] == L.QM_MPC_WARN_PIVOT
    c.close()


def test_warm_chain_lands_on_event(blobs, oblobs):
    """cold solve at t0, qmhip_mpc_advance_resident by dt with t0 + dt == the event exactly, then the warm solve: the advanced t0 / x0, the warm initial guess
    entry by entry and the warm solve against the oracle's"""
    t0, dt = ic.warm_chain_to_event(); assert t0 + dt == ic.EVENT
    cfg = _event_cfg(ic.base_config(), [t0]); hz = cfg["horizon"]
    c = Ctx(blobs, 1, 64, 2, cfg["ev"].shape[1]); res0 = c.solve(cfg); sol0 = _sol(res0, 0)
    o = ic.oracle_for(oblobs, cfg, 0); _check_solve(sol0, o.mpc_step(t0, t0 + hz, cfg["x0"][0]), "cold")
    c.mpc.advance(dt)
    t1 = c.itf.debug_read("t0", (1,))[0]; x1 = c.itf.debug_read("x0", (1, 30))[0]
    assert t1 == ic.EVENT
    xr, _ = ic.policy_reference(sol0["t"], sol0["ev"], sol0["x"], sol0["u"], t1)
    assert np.abs(x1 - xr).max() <= 1e-15 * np.abs(xr).max()
    c.mpc.solve_resident(hz, warm=True); res1 = c.mpc.download(); out = c.k0b()
    ora = o.mpc_step(t1, t1 + hz, x1, warm=True); xg, ug = o.initial_guess(); n = len(xg)
    _record(ic.check_k0b(o, dict(cfg, t0=np.array([t1])), out, 0, "warm on the event"))
    assert_blocks(out["x"][:n, 0], xg, "x", 1e-6, "warm guess x"); assert_blocks(out["u"][:n - 1, 0], ug, "u", 1e-6, "warm guess u")
    _check_solve(_sol(res1, 0), ora, "warm solve on the event")
    c.close()


def _instance(out, b):
    """instance b's outputs on its own nodes (node-major K0b arrays, instance-major downloads)"""
    n = int(out["n_nodes"][b])
    return {k: (v[b] if k in ("n_nodes", "status") else v[b, :n] if k in ("xs", "us") else v[:n, b]) for k, v in out.items()}


def test_batch_layout(blobs, oblobs):
    """per-instance outputs (K0b's, the initial guess, x*, u*, status) bit-identical whether an instance runs alone or at batch positions that straddle 64-lane
    boundaries (B = 1, 63, 65, 130), with the longest grid (an event burst) in the last, partial wave and max_nodes equal to its node count"""
    cfg, nmax = ic.layout_instances(); ref = []
    for b in range(cfg["B"]):
        c1 = _sub(cfg, [b]); c = Ctx(blobs, 1, nmax, 6, cfg["ev"].shape[1]); res = c.solve(c1); out = c.k0b()
        if b == cfg["B"] - 1:
            assert int(out["n_nodes"][0]) == nmax
            _record(ic.check_k0b(ic.oracle_for(oblobs, c1, 0), c1, out, 0, "event burst"))
        out.update(xs=res["x"], us=res["u"], status=res["status"])
        ref.append(_instance(out, 0)); c.close()
    for B, pos in ic.LAYOUTS.items():
        if pos is None: continue
        c = Ctx(blobs, B, nmax, 6, cfg["ev"].shape[1]); res = c.solve(ic.place(cfg, B, pos)); out = c.k0b()
        out.update(xs=res["x"], us=res["u"], status=res["status"])
        for j, b in enumerate(pos):
            got = _instance(out, b)
            for k in got:
                assert np.array_equal(got[k], ref[j][k]), (B, b, k)
        c.close()
