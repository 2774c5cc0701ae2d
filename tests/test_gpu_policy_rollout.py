"""Policy rollout on the MI355X through the C ABI (qmhip_policy_rollout, SqpMpc.rollout_policy / rolloutPolicy): B = 3 (stance, trot, flying trot in one batch, 20
intervals), a cold solve, the downloaded plan and gains as the numpy reference's plan (tests/rollout_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import rollout_ref as rr
from blocks import block_errs
from conftest import assert_blocks
from qm_control_amd import api, layout as L, scenarios
from test_gpu_plan_task_space import _pad

pytestmark = pytest.mark.gpu
GAITS = (("stance", 3), ("trot", 4), ("flying_trot", 5))


class Solved:
    def __init__(self, blobs):
        self.cfg = cfg = _pad([scenarios.gait_config(g, batch=1, n_intervals=20, seed=sd) for g, sd in GAITS])
        self.itf = itf = api.QMInterface(blobs=blobs, max_batch=3, max_nodes=36, max_ref_knots=2, max_events=cfg["ev"].shape[1]); self.mpc = mpc = api.SqpMpc(itf)
        self.lib = itf.lib; self.fric = float(itf.settings_blob[L.ST_FRIC_COEF])
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
        d = mpc.download(); gain, _ = mpc.feedback(); assert (d["status"] >= 0).all()
        self.plans = []
        for b in range(3):
            n = int(d["num_nodes"][b]); res = dict(t=d["t"][b, :n], ev=d["event"][b, :n], x=d["x"][b, :n], u=d["u"][b, :n])
            self.plans.append(rr.Plan(res, gain[b, :n], cfg["ev"][b], cfg["modes"][b]))
        self.rows = rr.row_set(self.plans); self._whole = {}

    def call(self, rows, max_step, max_steps, feedback, **kw):
        return rr.call(self.lib.qmhip_policy_rollout, self.itf.h, rows, max_step, max_steps, feedback, **kw)

    def whole(self, feedback):
        if feedback not in self._whole:
            rc, out, _ = self.call(self.rows, rr.DT, 4096, feedback, cap=40); assert rc == 0, self.error(); self._whole[feedback] = out
        return self._whole[feedback]

    def error(self):
        return self.lib.qmhip_last_error(self.itf.h).decode()


@pytest.fixture(scope="module")
def solved(blobs):
    s = Solved(blobs); yield s; s.itf.close()


def _take(rows, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) else [v[i] for i in idx]) for k, v in rows.items()}


@pytest.mark.parametrize("feedback", [0, 1])
def test_rows_against_the_reference(solved, oracle, feedback):
    """the 70 rows of rollout_ref.row_set, every call of rollout_ref.CALLS, against the reference on the downloaded plan and gains: the per-sample and summary assertions of
    tests/test_policy_rollout.py; the measured maxima are printed"""
    w = solved; seen = set()
    for max_step, max_steps, what in rr.CALLS:
        if max_step == rr.DT and max_steps > 3: rows, out = w.rows, w.whole(feedback)
        else: rows = w.rows; rc, out, _ = w.call(rows, max_step, max_steps, feedback, cap=40); assert rc == 0, w.error()
        worst = rr.check_rows(oracle, w.plans, w.fric, rows, out, max_step, max_steps, feedback, 0, "%s, feedback %d" % (what, feedback))
        print(what, "feedback", feedback, {k: "%.2e" % v for k, v in worst.items()})
        seen |= {int(f) for f in out["summary"]["flags"]}
        if feedback: assert out["summary"]["max_fb"].max() > 1e-3
        else: assert not out["summary"]["max_fb"].any()
    assert {0, rr.FLAG_MAX_STEPS, rr.FLAG_OUTSIDE} <= seen and not any(f & rr.FLAG_NONFINITE for f in seen)


def test_every_sample_against_the_policy_entry_point(solved):
    """u_k of every sample against qmhip_policy_eval_feedback(tau_k, x_k) on the device — within 1e-13 of the block's largest entry, the allowance
    tests/test_gpu_published_policy.py gives two kernels that inline the same routine — and mode_k exact"""
    w = solved; out = w.whole(1); worst = 0.0
    kmax = int(out["count"].max())
    for k in range(kmax):
        rws = [r for r in range(70) if out["count"][r] > k]
        for b in range(3):      # one evaluation per instance at a time: the entry point takes one (t, x) per instance of the batch
            mine = [r for r in rws if w.rows["inst"][r] == b]
            for r in mine:
                s = out["trace"][r, k]; t = np.array([pl.res["t"][0] for pl in w.plans]); x = np.array([pl.res["x"][0] for pl in w.plans])
                t[b] = w.plans[b].query_time(s["t"]); x[b] = s["x"]
                _, ud, mode = w.mpc.evaluate_policy(t, x)
                assert mode[b] == s["mode"], (r, k)
                worst = max(worst, max(block_errs(s["u"][None], ud[b][None], "u").values())); assert_blocks(s["u"][None], ud[b][None], "u", 1e-13, "row %d point %d" % (r, k))
    print("largest block difference to qmhip_policy_eval_feedback: %.2e" % worst)


def test_rows_repeated_and_permuted(solved):
    """R = 130: the 70 rows repeated and permuted, inst out of order — every row equals its R = 70 result bit for bit; R = 1 equals the batch slot; a rollout split at a
    returned t_k and continued equals the whole, its summaries merged by max / min / sum the whole's"""
    w = solved; whole = w.whole(1); rng = np.random.default_rng(3); idx = rng.permutation(np.concatenate([np.arange(70), rng.integers(0, 70, 60)])); assert len(idx) == 130
    rc, big, _ = w.call(_take(w.rows, list(idx)), rr.DT, 4096, 1, cap=40); assert rc == 0
    for i, r in enumerate(idx):
        for k in ("x", "u", "mode", "summary", "count"): assert big[k][i].tobytes() == whole[k][r].tobytes(), (i, r, k)
        n = int(whole["count"][r]); assert big["trace"][i, :n].tobytes() == whole["trace"][r, :n].tobytes()
    for r in (0, 33, 69):
        rc, one, _ = w.call(_take(w.rows, [r]), rr.DT, 4096, 1, cap=40); assert rc == 0
        for k in ("x", "u", "mode", "summary", "count"): assert one[k][0].tobytes() == whole[k][r].tobytes(), (r, k)
    cand = [r for r in range(70) if whole["count"][r] >= 5]
    for r in cand[:8]:
        n = int(whole["count"][r]); k = n // 2; tr = whole["trace"][r]
        first = _take(w.rows, [r]); first["t_end"] = np.array([tr["t"][k]]); rc, a, _ = w.call(first, rr.DT, 4096, 1, cap=40); assert rc == 0 and a["count"][0] == k + 1
        second = _take(w.rows, [r]); second["t0"] = np.array([tr["t"][k]]); second["x0"] = a["x"].copy(); rc, b, _ = w.call(second, rr.DT, 4096, 1, cap=40); assert rc == 0 and b["count"][0] == n - k
        assert b["x"][0].tobytes() == whole["x"][r].tobytes() and b["u"][0].tobytes() == whole["u"][r].tobytes() and b["mode"][0] == whole["mode"][r]
        assert np.concatenate([a["trace"][0, :k], b["trace"][0, :n - k]]).tobytes() == tr[:n].tobytes(), r
        assert rr.merge_summaries(a["summary"][0], b["summary"][0]).tobytes() == whole["summary"][r].tobytes(), r
    sub = list(range(1, 70, 3)); rc, t3, _ = w.call(_take(w.rows, sub), rr.DT, 4096, 1, cap=3); assert rc == 0
    for i, r in enumerate(sub):
        assert t3["x"][i].tobytes() == whole["x"][r].tobytes() and t3["count"][i] == whole["count"][r]; assert set(t3["trace"][i, min(int(t3["count"][i]), 3):].tobytes()) <= {0xa5}


def test_rolloutPolicy_follows_the_upstream_name(solved):
    """rolloutPolicy(t, x, 0.002) equals rollout_policy with t_end = t + 0.002 under the policy ST_FEEDBACK_POLICY selects"""
    w = solved; t = np.array([pl.res["t"][2] + 0.003 for pl in w.plans]); x = np.array([pl.res["x"][2] + 0.2 * rr.PERTURB for pl in w.plans])
    for fb in (0.0, 1.0):
        w.itf.set_setting(L.ST_FEEDBACK_POLICY, fb)
        xs, us, mode = w.mpc.rolloutPolicy(t, x, 0.002); ref = w.mpc.rollout_policy(t, x, t + 0.002, feedback=bool(fb))
        assert np.array_equal(xs, ref["x"]) and np.array_equal(us, ref["u"]) and np.array_equal(mode, ref["mode"]) and (ref["summary"]["steps"] == 1).all() and np.abs(xs - x).max() > 0
    w.itf.set_setting(L.ST_FEEDBACK_POLICY, 0.0)


def test_published_source(blobs):
    """ST_FEEDBACK_POLICY = 1, a window of 8 nodes, publish, then a different solve on the context: a source 1 rollout over the first interval equals the source 0
    rollout taken before the second solve in x_end, mode, steps and uncovered == 0, u_end within 1e-13 of the block's largest entry, seq == 1; a rollout past the window has
    uncovered > 0 and its uncovered samples carry covered == 0 and the feed-forward input of qmhip_policy_eval_published bit for bit"""
    w = Solved(blobs); itf, mpc, cfg = w.itf, w.mpc, w.cfg
    try:
        itf.set_setting(L.ST_FEEDBACK_POLICY, 1.0); itf.set_publish_window(8)
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"]); mpc.publish_policy()
        t0 = np.array([pl.res["t"][0] for pl in w.plans]); x0 = np.array([pl.res["x"][0] + 0.5 * rr.PERTURB for pl in w.plans])
        a = mpc.rollout_policy(t0, x0, t0 + rr.DT, trace=4)
        t1 = cfg["t0"] + 0.02; x1, _, _ = mpc.evaluatePolicy(t1); mpc.set_initial(t1, x1 + 0.01); mpc.solve_resident(cfg["horizon"], warm=True)      # rewrites the stage records
        b = mpc.rollout_policy(t0, x0, t0 + rr.DT, source="published", trace=4)
        assert b["seq"] == 1 and np.array_equal(a["x"], b["x"]) and np.array_equal(a["mode"], b["mode"]) and np.array_equal(a["summary"]["steps"], b["summary"]["steps"]) and (b["summary"]["uncovered"] == 0).all()
        assert_blocks(b["u"], a["u"], "u", 1e-13, "published against the live records")
        c = mpc.rollout_policy(t0, x0, t0 + 12 * rr.DT, source="published", trace=40); assert (c["summary"]["uncovered"] > 0).all()
        for r in range(3):
            n = int(c["count"][r]); s = c["trace"][r, :n]; unc = np.flatnonzero(s["covered"] == 0); assert len(unc) == c["summary"]["uncovered"][r] and s["covered"][0] == 1
            for k in unc:
                t = t0.copy(); t[r] = w.plans[r].query_time(s["t"][k]); _, uf, _, _, _ = mpc.evaluate_published(t); assert np.array_equal(s["u"][k], uf[r]), (r, k)
    finally:
        itf.close()


def test_error_paths(blobs):
    """the error paths of the entry point on the device, before any solve included: code, message, the caller's output memory untouched"""
    cfg = _pad([scenarios.gait_config(g, batch=1, n_intervals=20, seed=sd) for g, sd in GAITS])
    itf = api.QMInterface(blobs=blobs, max_batch=3, max_nodes=36, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf); lib = itf.lib
    rows = dict(inst=np.array([2, 0, 1, 1], np.int32), t0=cfg["t0"][[2, 0, 1, 1]], x0=cfg["x0"][[2, 0, 1, 1]], t_end=cfg["t0"][[2, 0, 1, 1]] + 0.03, shape=["e"] * 4); ARG, STATE = -1, -5

    def bad(code, text, *a, rows_=rows, **kw):
        keep = rr.new_out(len(rows_["t0"]), max(kw.get("cap", 0), 0)); rc, out, _ = rr.call(lib.qmhip_policy_rollout, itf.h, rows_, *a, out=keep, **kw); err = lib.qmhip_last_error(itf.h).decode()
        assert rc == code, (rc, code, text, err); assert text in err, (text, err); assert rr.untouched(out), text

    ok = (rr.DT, 4096, 1)
    try:
        bad(STATE, "no policy received yet", *ok); bad(STATE, "no policy received yet", rr.DT, 4096, 0); bad(STATE, "no policy published yet", *ok, source=1)
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); bad(STATE, "no policy received yet", *ok)      # an upload is not a solve
        mpc.solve_resident(cfg["horizon"])
        r0 = dict(rows); r0["R"] = 0; bad(ARG, "R < 1", *ok, rows_=r0)
        for v in (-1, 3): ri = dict(rows); ri["inst"] = rows["inst"].copy(); ri["inst"][2] = v; bad(ARG, "outside the batch", *ok, rows_=ri)
        bad(ARG, "inst == NULL", *ok, inst=None)
        for name in ("t0", "x0", "t_end", "x", "u", "mode"): bad(ARG, "required pointer", *ok, null=(name,))
        bad(ARG, "required pointer", *ok, params=False)
        for v in (0.0, -0.01, np.inf, np.nan): bad(ARG, "max_step", v, 4096, 1)
        bad(ARG, "max_steps", rr.DT, 0, 1); bad(ARG, "trace_cap", *ok, cap=-1); bad(ARG, "trace_cap", *ok, cap=2, null=("trace",)); bad(ARG, "source", *ok, source=2); bad(ARG, "feedback", rr.DT, 4096, 2)
        rt = dict(rows); rt["t0"] = rows["t0"].copy(); rt["t0"][1] = np.nan; bad(ARG, "finite", *ok, rows_=rt)
        rt = dict(rows); rt["t_end"] = rows["t0"] - 1e-9; bad(ARG, "t_end >= t0", *ok, rows_=rt)
        mpc.step_submit(cfg["t0"] + 0.01, cfg["x0"], horizon=cfg["horizon"], period=0.002, time=20.0); bad(STATE, "in flight", *ok); mpc.step_collect()
        rc, _, _ = rr.call(lib.qmhip_policy_rollout, itf.h, rows, *ok); assert rc == 0
        itf.set_publish_window(8); mpc.publish_policy(); bad(STATE, "no gains", *ok, source=1)      # published with ST_FEEDBACK_POLICY = 0
        rc, _, seq = rr.call(lib.qmhip_policy_rollout, itf.h, rows, rr.DT, 4096, 0, source=1); assert rc == 0 and seq == 1
        for solver in (3.0, 1.0):
            itf.set_setting(L.ST_SOLVER, solver); bad(ARG, "multiple-shooting", *ok)
        mpc.solve_resident(cfg["horizon"]); bad(ARG, "multiple-shooting", *ok)                          # the discrete iLQR: no feedback policy,
        rc, _, _ = rr.call(lib.qmhip_policy_rollout, itf.h, rows, rr.DT, 4, 0); assert rc == 0          # but the feed-forward rollout works behind any solver slot
        itf.set_setting(L.ST_SOLVER, 0.0); bad(STATE, "no policy received yet", *ok)                    # a solver switch drops the solution
    finally:
        itf.close()
