"""tests/rollout_ref.py — TEST INFRASTRUCTURE of the policy rollout (include/qmhip.h "policy rollout"; qm_policy_rollout_kernel, csrc/kernels/k_rollout.h), shared by
tests/test_policy_rollout.py (host emulator) and tests/test_gpu_policy_rollout.py (device): the numpy reference of the semantics — evaluation times, query time, policy,
Heun step, fold — built from feedback_ref.linear_policy, interp_cases.time_segment, Oracle.flow_map and the schedule; the rows both tests roll out; the per-sample and
summary checks; the ctypes binding of tests/emu_rollout."""
import ctypes as C
import os
import subprocess

import numpy as np

import feedback_ref as fr
import interp_cases as ic
from blocks import assert_blocks, block_errs
from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
DT = ic.DT
ATOL_STEP = 1e-12        # plan_ref.ATOL_POS, the project's bound for pure kinematics: one Heun step from the device's own (x_k, u_k) adds rounding of order h * 1e-14
RTOL_U = 1e-6            # the project's bound per block of tests/blocks.py "u"
RTOL_SUMMARY = 1e-12     # of the field's scale
PERTURB = np.concatenate([np.full(6, 0.05), np.full(6, 0.01), np.full(18, 0.05)])      # momentum / base pose / joints: finite for 0.3 s under both policies (checked with the oracle)
FLAG_MAX_STEPS, FLAG_NONFINITE, FLAG_OUTSIDE = L.QM_ROLLOUT_MAX_STEPS, L.QM_ROLLOUT_NONFINITE, L.QM_ROLLOUT_OUTSIDE


class Params(C.Structure):
    _fields_ = [("max_step", C.c_double), ("max_steps", C.c_int32), ("source", C.c_int32), ("feedback", C.c_int32), ("trace_cap", C.c_int32)]


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the plan of one instance as the reference reads it ----
class Plan:
    """res: dict(t, ev, x, u) of the instance's n nodes; K [n][30][30]: K_full of the node each node's input was copied from; ev_t / modes: the instance's schedule
    (padding included, as the device holds it); W: publication window (None: source 0)"""

    def __init__(self, res, K, ev_t, modes, W=None):
        self.res = {k: np.asarray(res[k]) for k in ("t", "ev", "x", "u")}; self.K = K; self.ev_t = np.asarray(ev_t, float); self.modes = np.asarray(modes); self.W = W
        self.src = np.array([-1 if fr.source_node(self.res["ev"], i) is None else fr.source_node(self.res["ev"], i) for i in range(len(self.res["t"]))])
        self.ta = self.res["t"] + np.where(self.res["ev"] == 2, ic.LIMIT_EPS, np.where(self.res["ev"] == 1, -ic.LIMIT_EPS, 0.0))

    def query_time(self, t):
        return t + ic.WEAK_EPS if (self.ev_t == t).any() else t

    def mode_at(self, tau):
        return int(self.modes[int(np.searchsorted(self.ev_t, tau, side="left"))])      # grid_find_index: lower bound

    def covered(self, tau):
        if self.W is None: return 1
        n = len(self.ta); i, _ = ic.time_segment(self.ta, tau); j = i + 1 if n > 1 else i; wn = min(self.W, n)
        return int(i < wn and j < wn)

    def outside(self, tau):
        return bool(tau < self.ta[0] or tau > self.ta[-1])

    def feed_forward(self, tau):
        return ic.policy_reference(self.res["t"], self.res["ev"], self.res["x"], self.res["u"], tau)      # (x_des, u_ff)

    def policy(self, tau, x, feedback):
        """(u, u_ff, x_des, covered) at the query time tau and the state x"""
        xd, uff = self.feed_forward(tau); cov = self.covered(tau)
        u = fr.linear_policy(self.res, self.K, self.src, tau, x) if (feedback and cov) else uff
        return u, uff, xd, cov


def times(plan, t0, t_end, max_step, max_steps):
    """(t_k [K + 1], steps that ended on an event, max_steps flag): t_{k+1} = min(t_k + max_step, e, t_end), e the first event strictly behind t_k — in plain f64"""
    t = [float(t0)]; events = 0; cut = False
    while t[-1] < t_end:
        if len(t) - 1 >= max_steps: cut = True; break
        later = plan.ev_t[plan.ev_t > t[-1]]; e = float(later.min()) if len(later) else np.inf
        tn = min(min(t[-1] + max_step, e), float(t_end)); events += int(tn == e); t.append(tn)
    return np.array(t), events, cut


def heun(oracle, x, u, h):
    f1 = oracle.flow_map(x, u); f2 = oracle.flow_map(x + h * f1, u)
    return x + 0.5 * h * f1 + 0.5 * h * f2


def chain(oracle, plan, t0, x0, t_end, max_step, max_steps, feedback):
    """the whole rollout in numpy from x0: dict(t, x, u, mode)"""
    tk, _, _ = times(plan, t0, t_end, max_step, max_steps); x = np.array(x0, float); xs, us, ms = [], [], []
    for k, t in enumerate(tk):
        tau = plan.query_time(t); u, _, _, _ = plan.policy(tau, x, feedback); xs.append(x); us.append(u); ms.append(plan.mode_at(tau))
        if k + 1 < len(tk): x = heun(oracle, x, u, tk[k + 1] - t)
    return dict(t=tk, x=np.array(xs), u=np.array(us), mode=np.array(ms))


def fold(plan, fric, t, x, u, mode, source):
    """the summary of section 1 over samples (t_k, x_k, u_k, mode_k): a dict with the fields of struct qmhip_rollout_summary that depend on the samples"""
    dev = np.zeros(4); fb = np.zeros(2); cone = np.inf; fz = np.inf; swing = 0.0; unc = 0; outside = False
    for k in range(len(t)):
        tau = plan.query_time(t[k]); xd, uff = plan.feed_forward(tau); d = np.abs(x[k] - xd); g = np.abs(u[k] - uff)
        dev = np.maximum(dev, [d[0:6].max(), d[6:12].max(), d[12:24].max(), d[24:30].max()]); fb = np.maximum(fb, [g[0:12].max(), g[12:30].max()])
        for c in range(4):
            F = u[k][3 * c:3 * c + 3]
            if (int(mode[k]) >> (3 - c)) & 1: cone = min(cone, fric * F[2] - np.sqrt(F[0] * F[0] + F[1] * F[1])); fz = min(fz, F[2])
            else: swing = max(swing, np.abs(F).max())
        unc += int(source == 1 and not plan.covered(tau)); outside = outside or plan.outside(tau)
    return dict(max_dev=dev, max_fb=fb, min_cone=cone, min_fz=fz, max_swing_force=swing, uncovered=unc, outside=outside)


# ---- the rows both tests roll out ----
def row_set(plans, seed=11, R=70, span=6 * DT):
    """R rows over the instances in scrambled order, from the shapes: start on node 0 / mid-interval (t0 + 0.004) / exactly on an event / t_end == t0 / a span crossing two
    events / t_end beyond the plan, each from a state off the plan by +-PERTURB, by a tenth of that, and not at all.  Returns dict(inst, t0, x0, t_end, shape)"""
    rng = np.random.default_rng(seed); rows = []
    for b, pl in enumerate(plans):
        t = pl.res["t"]; tf = float(t[-1]); inside = [float(e) for e in pl.ev_t if t[0] < e < tf]
        shapes = [("node0", float(t[0]), float(t[0]) + span), ("mid", float(t[0]) + 0.004, float(t[0]) + 0.004 + span)]
        if inside: shapes.append(("event", inside[0], min(inside[0] + span, tf)))
        shapes.append(("empty", float(t[3]) + 0.001, float(t[3]) + 0.001))
        if len(inside) >= 2: shapes.append(("two events", inside[0] - 0.5 * DT, inside[1] + 0.5 * DT))
        else: shapes.append(("long", float(t[0]) + 0.002, float(t[0]) + 0.002 + 1.5 * span))
        shapes.append(("beyond", tf - 2.5 * DT, tf + 1.5 * DT)); shapes.append(("late", float(t[5]) + 0.007, float(t[5]) + 0.007 + span))
        for name, a, e in shapes:
            for scale in (1.0, -1.0, 0.1, 0.0):
                xp, _ = pl.feed_forward(pl.query_time(a)); sign = rng.choice([-1.0, 1.0], 30)
                rows.append((b, a, xp + scale * sign * PERTURB, e, name))
    order = rng.permutation(len(rows))[:R]; rows = [rows[i] for i in order]
    assert len(rows) == R and {"node0", "mid", "event", "empty", "two events", "beyond"} <= {r[4] for r in rows}
    return dict(inst=np.array([r[0] for r in rows], np.int32), t0=np.array([r[1] for r in rows]), x0=np.array([r[2] for r in rows]), t_end=np.array([r[3] for r in rows]), shape=[r[4] for r in rows])


# the calls of the row set: (max_step, max_steps, what); times both policies
CALLS = [(DT, 4096, "max_step = sqp.dt"), (0.05, 4096, "max_step = 0.05, beyond the event spacing"), (0.005, 4096, "max_step = 0.005"), (DT, 3, "max_steps = 3: cut short")]


def new_out(R, cap, fill=0xa5):
    """output arrays of a call, every byte `fill`: what a call leaves alone shows"""
    mk = lambda shape, dt: np.frombuffer(bytes([fill]) * int(np.prod(shape) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()
    return dict(x=mk((R, 30), np.float64), u=mk((R, 30), np.float64), mode=mk((R,), np.int32), summary=mk((R,), api.ROLLOUT_SUMMARY), trace=mk((R, max(cap, 1)), api.ROLLOUT_SAMPLE)[:, :cap], count=mk((R,), np.int32))


def untouched(out, fill=0xa5):
    return all(np.frombuffer(np.ascontiguousarray(v).tobytes(), np.uint8).min(initial=fill) == fill and np.frombuffer(np.ascontiguousarray(v).tobytes(), np.uint8).max(initial=fill) == fill for v in out.values())


# ---- checks ----
def check_rows(oracle, plans, fric, rows, out, max_step, max_steps, feedback, source, what, worst=None):
    """every assertion of the per-sample and summary lists on the result `out` (new_out filled by a call with trace_cap >= every count) of `rows`; returns the worst figures"""
    worst = worst if worst is not None else {}; bump = lambda k, v: worst.__setitem__(k, max(worst.get(k, 0.0), float(v)))
    R = len(rows["inst"]); cap = out["trace"].shape[1]
    for r in range(R):
        pl = plans[int(rows["inst"][r])]; tk, events, cut = times(pl, rows["t0"][r], rows["t_end"][r], max_step, max_steps); n = len(tk); tag = "%s row %d (%s)" % (what, r, rows["shape"][r])
        assert out["count"][r] == n <= cap, (tag, out["count"][r], n)
        s = out["trace"][r, :n]; sm = out["summary"][r]
        taus = [pl.query_time(t) for t in tk]
        assert np.array_equal(s["t"], tk), tag
        assert np.array_equal(s["mode"], [pl.mode_at(ta) for ta in taus]), tag
        assert np.array_equal(s["covered"], [pl.covered(ta) for ta in taus]), tag
        flags = (FLAG_MAX_STEPS if cut else 0) | (FLAG_OUTSIDE if any(pl.outside(ta) for ta in taus) else 0)
        assert (sm["steps"], sm["events"], sm["flags"], sm["t_end"]) == (n - 1, events, flags, tk[-1]), (tag, sm, n - 1, events, flags)
        assert np.isfinite(s["x"]).all() and np.isfinite(s["u"]).all(), tag
        uref = np.array([pl.policy(taus[k], s["x"][k], feedback)[0] for k in range(n)])
        for k, v in block_errs(s["u"], uref, "u").items(): bump("u " + k, v)
        assert_blocks(s["u"], uref, "u", RTOL_U, tag)
        for k in range(n - 1):
            h = tk[k + 1] - tk[k]; xr = heun(oracle, s["x"][k], s["u"][k], h); err = np.abs(s["x"][k + 1] - xr).max(); bump("heun step", err)
            assert err <= ATOL_STEP, (tag, k, err)
            # the joint rows are x_k + h u_k: 1e-15 relative to the larger of the two summands (the rounding of a sum scales with its operands, not with a cancelled result)
            jr = s["x"][k, 12:] + h * s["u"][k, 12:]; jerr = (np.abs(s["x"][k + 1, 12:] - jr) / np.maximum(np.maximum(np.abs(s["x"][k, 12:]), np.abs(h * s["u"][k, 12:])), 1e-300)).max(); bump("joint rows", jerr)
            assert jerr <= 1e-15, (tag, k, jerr)
        assert np.array_equal(s["x"][-1], out["x"][r]) and np.array_equal(s["u"][-1], out["u"][r]) and s["mode"][-1] == out["mode"][r], tag
        f = fold(pl, fric, tk, s["x"], s["u"], s["mode"], source)
        assert sm["uncovered"] == f["uncovered"] and (sm["ispare"] == 0).all() and (sm["spare"] == 0).all(), tag
        for name in ("max_dev", "max_fb", "min_cone", "min_fz", "max_swing_force"):
            got = np.atleast_1d(sm[name]).astype(float); ref = np.atleast_1d(f[name]).astype(float)
            for g, q in zip(got, ref):
                if np.isinf(q): assert g == q, (tag, name, g, q)
                else:
                    scale = max(abs(q), {"max_dev": 1.0, "max_fb": 1.0}.get(name, float(np.abs(s["u"][:, :12]).max()) + 1.0)); e = abs(g - q) / scale; bump("summary " + name, e)
                    assert e <= RTOL_SUMMARY, (tag, name, g, q)
    return worst


def merge_summaries(a, b):
    """the summary of a rollout split at a returned t_k from its two parts (maxima / minima / sums / OR; t_end of the second)"""
    m = a.copy(); m["t_end"] = b["t_end"]
    for k in ("max_dev", "max_fb", "max_swing_force"): m[k] = np.maximum(a[k], b[k])
    for k in ("min_cone", "min_fz"): m[k] = np.minimum(a[k], b[k])
    for k in ("steps", "events"): m[k] = a[k] + b[k]
    m["flags"] = a["flags"] | b["flags"]
    return m


# ---- the emulator binding (tests/emu_rollout) ----
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_rollout"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_rollout", "_build", "libqm_emu_rollout.so"))
    lib.emu_rollout_create.restype = C.c_void_p; lib.emu_rollout_last_error.restype = C.c_char_p; lib.emu_rollout_last_error.argtypes = [C.c_void_p]; lib.emu_rollout_publish.restype = C.c_long
    lib.emu_rollout_destroy.argtypes = [C.c_void_p]; lib.emu_rollout_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]; lib.emu_rollout_publish.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.emu_rollout_counts.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def call(fn, handle, rows, max_step, max_steps, feedback, source=0, cap=0, out=None, inst="rows", null=(), params=True):
    """one qmhip_policy_rollout-shaped call (`fn(handle, R, inst, t0, x0, t_end, p, x_end, u_end, mode_end, summary, trace, count, seq)`): (rc, out, seq).
    null: names among t0 / x0 / t_end / x / u / mode / trace to pass as NULL"""
    R = len(rows["t0"]); out = out if out is not None else new_out(R, cap); seq = C.c_int64(-1)
    a = {k: np.ascontiguousarray(rows[k], float) for k in ("t0", "x0", "t_end")}; ins = np.ascontiguousarray(rows["inst"], np.int32) if inst == "rows" else inst
    p = Params(float(max_step), int(max_steps), int(source), int(feedback), int(cap))
    g = lambda name, arr: None if name in null else ptr(arr)
    rc = fn(handle, C.c_int(rows.get("R", R)), ptr(ins), g("t0", a["t0"]), g("x0", a["x0"]), g("t_end", a["t_end"]), C.byref(p) if params else None, g("x", out["x"]), g("u", out["u"]), g("mode", out["mode"]),
            ptr(out["summary"]), g("trace", out["trace"]) if cap else None, ptr(out["count"]), C.byref(seq))
    return rc, out, seq.value
