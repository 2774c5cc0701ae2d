"""Planned task-space trajectories on the MI355X through the C ABI (qmhip_plan_task_space / qmhip_plan_footholds / qmhip_task_space_eval): every record against the
oracle-built reference of tests/plan_ref.py on the DOWNLOADED plan (kinematics and data movement, not solver parity), the zero fill, the foothold list and its
ordering, caller-supplied rows, the error paths."""
import numpy as np
import pytest

import plan_ref as pf
from qm_control_amd import layout as L

pytestmark = pytest.mark.gpu
B65 = 65      # one full wave of instances plus one row in the next: the smallest batch that crosses the cooperative tile's edge with a nearly empty wave


def _pad(cfgs):
    """single-instance configs -> one batch (schedules padded with far-future stance events, as scenarios._pad_schedules does)"""
    ne = max(c["ev"].shape[1] for c in cfgs); out = {k: np.concatenate([c[k] for c in cfgs]) for k in ("t0", "x0", "ref_t", "ref_x")}
    ev = np.zeros((len(cfgs), ne)); mo = np.full((len(cfgs), ne + 1), 15, np.int32)
    for b, c in enumerate(cfgs):
        n = c["ev"].shape[1]; ev[b, :n] = c["ev"][0]; ev[b, n:] = c["ev"][0, -1] + 1e3 * np.arange(1, ne - n + 1); mo[b, :n + 1] = c["modes"][0]; mo[b, n + 1:] = c["modes"][0, -1]
    out.update(ev=ev, modes=mo, horizon=cfgs[0]["horizon"]); return out


def _check_plan(oracle, cfg, got, rec, nn, what):
    """every record of every instance against plan_ref built from the downloaded x, u, t, mode; rows at or behind num_nodes[b] all zero"""
    assert np.array_equal(nn, got["num_nodes"]); mx = {}
    for b in range(len(nn)):
        n = int(nn[b]); assert (got["status"][b] >= 0) and n >= 3
        ref = pf.plan(oracle, cfg["ref_t"][b], cfg["ref_x"][b], got["t"][b, :n], got["x"][b, :n], got["u"][b, :n], got["mode"][b, :n])
        mx = pf.merge(mx, pf.compare(rec[b, :n], ref, "%s, instance %d" % (what, b)))
        assert not rec[b, n:].tobytes().strip(b"\0"), (what, b)
    print("%s: max abs differences %s" % (what, {k: "%.1e" % v for k, v in sorted(mx.items())}))
    return mx


@pytest.fixture(scope="module")
def trot65(blobs):
    """B = 65, trot, horizon 0.5 s, cold solve; t0 offset by multiples of 7 ms: different node counts, different event placement.  Solved once, shared, not modified"""
    from qm_control_amd import api, scenarios
    dt = blobs[1][L.ST_SQP_DT]; N = int(round(0.5 / dt)); cfg = scenarios.make_config("C3", batch=B65, n_intervals=N); cfg["horizon"] = 0.5
    cfg["t0"] = 0.1 + 0.007 * np.arange(B65); cfg["ref_t"] = np.stack([cfg["t0"], cfg["t0"] + 0.5], axis=1)
    itf = api.QMInterface(blobs=blobs, max_batch=B65, max_nodes=N + 14, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"])
    fh = np.full((B65, 2), 0, api.FOOTHOLD); cnt = np.full(B65, -7, np.int32); rec = np.zeros((B65, itf.max_nodes), api.PLAN_RECORD); rec.view(np.uint8)[:] = 0xa5
    rc = itf.lib.qmhip_plan_task_space(itf.h, B65, pf.ptr(rec), None); err = itf.lib.qmhip_last_error(itf.h).decode()      # the no-solve case, before anything has been solved
    rc2 = itf.lib.qmhip_plan_footholds(itf.h, B65, 2, pf.ptr(fh), pf.ptr(cnt))
    no_solve = dict(rc=rc, rc2=rc2, err=err, untouched=bool((rec.view(np.uint8) == 0xa5).all() and (cnt == -7).all()))
    mpc.solve_resident(0.5); got = mpc.download()
    yield dict(cfg=cfg, itf=itf, mpc=mpc, got=got, no_solve=no_solve)
    itf.close()


def test_no_solution_is_an_error_that_touches_nothing(trot65):
    """before any solve qmhip_plan_task_space / qmhip_plan_footholds return QMHIP_ERR_STATE with a message and leave the caller's memory as it was"""
    ns = trot65["no_solve"]; assert ns["rc"] == -5 and ns["rc2"] == -5 and "no solution" in ns["err"] and ns["untouched"], ns


def test_every_record_of_a_ragged_batch(trot65, oracle):
    s = trot65; rec, nn = s["mpc"].plan_task_space()
    assert len(set(nn.tolist())) > 1, nn      # the offsets do give different grids
    _check_plan(oracle, s["cfg"], s["got"], rec, nn, "B = 65 trot, cold")
    live = np.concatenate([rec[b, :nn[b]] for b in range(B65)]); assert np.array_equal(live["time"], np.concatenate([s["got"]["t"][b, :nn[b]] for b in range(B65)]))


def test_footholds_of_a_ragged_batch(trot65, oracle):
    """count, leg, event and time equal the reference's, positions within 1e-12, ordered by (event, foot); cap = 1: the same count, slot 0 only"""
    s = trot65; got = s["got"]; cfg = s["cfg"]; cap = 16; fh, cnt = s["mpc"].plan_footholds(cap); fh1, cnt1 = s["mpc"].plan_footholds(1); mx = 0.0
    for b in range(B65):
        n = int(got["num_nodes"][b]); ref = pf.footholds(oracle, got["t"][b, :n], got["x"][b, :n], cfg["ev"][b], cfg["modes"][b])
        mx = max(mx, pf.compare_footholds(fh[b], cnt[b], ref, cap, "instance %d" % b)); pf.compare_footholds(fh1[b], cnt1[b], ref, 1, "cap 1, instance %d" % b)
    assert cnt.sum() > 0 and len(set(cnt.tolist())) > 1 and np.array_equal(cnt1, cnt), cnt
    print("footholds: %d landings, per instance %s, max abs position difference %.1e" % (cnt.sum(), sorted(set(cnt.tolist())), mx))


def test_three_gaits_cold_and_warm(blobs, oracle):
    """B = 3: stance, trot, flying trot (its flight phase takes the cop[2] <= 0 branch), a cold solve and a warm-started second one"""
    from qm_control_amd import api, scenarios
    cfg = _pad([scenarios.gait_config(g, batch=1, n_intervals=20, seed=sd) for g, sd in (("stance", 3), ("trot", 4), ("flying_trot", 5))])
    itf = api.QMInterface(blobs=blobs, max_batch=3, max_nodes=36, max_ref_knots=2, max_events=cfg["ev"].shape[1]); mpc = api.SqpMpc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); mpc.solve_resident(cfg["horizon"])
    rec, nn = mpc.plan_task_space(); _check_plan(oracle, cfg, mpc.download(), rec, nn, "three gaits, cold")
    live = np.concatenate([rec[b, :nn[b]] for b in range(3)]); assert (live["contact_mask"] == 0).any() and (live["contact_mask"] == 15).any()
    t1 = cfg["t0"] + 0.02; x1, _, _ = mpc.evaluatePolicy(t1); mpc.set_initial(t1, x1); mpc.solve_resident(cfg["horizon"], warm=True)
    rec2, nn2 = mpc.plan_task_space(); _check_plan(oracle, cfg, mpc.download(), rec2, nn2, "three gaits, warm"); assert rec2.tobytes() != rec.tobytes()
    itf.close()


def test_task_space_eval(trot65, oracle, blobs):
    """R = 130 random states (joints inside their limits, random roll / pitch / yaw, every mode, random inputs and references) with and without inputs / references;
    node 0 of the plan evaluated as a row — the node's state, input, mode and the solver's own end-effector reference — gives record 0 BIT FOR BIT (the two row kernels
    are one routine, k_plan.h)"""
    s = trot65; itf = s["itf"]; R = 130; x, u, mode, ee = pf.random_states(blobs, R, 11); mx = {}
    for uu, ee_, what in ((u, ee, "u, ee"), (None, ee, "no u"), (u, None, "no ee"), (None, None, "neither")):
        ref = np.array([pf.record(oracle, x[r], None if uu is None else uu[r], mode[r], None if ee_ is None else (ee_[r, :3], ee_[r, 3:])) for r in range(R)])
        got = itf.task_space(x, uu, mode, ee_); mx = pf.merge(mx, pf.compare(got, ref, what)); assert not got["time"].any()
        if ee_ is None: assert not got["ee_err"].any()
        if uu is None: assert not got["foot_force"].any() and not got["cop"].any()
    print("task_space_eval: max abs differences %s" % {k: "%.1e" % v for k, v in sorted(mx.items())})
    rec, nn = s["mpc"].plan_task_space(); g = s["got"]; nm = itf.max_nodes; eeref = itf.debug_read("eeref", (nm, B65, 7))
    for b in (0, 64):
        row = itf.task_space(g["x"][b, 0], g["u"][b, 0], g["mode"][b, 0], eeref[0, b]); row["time"] = g["t"][b, 0]
        assert row.tobytes() == rec[b, :1].tobytes(), b
    for bad in (0, B65 * nm + 1):
        assert itf.lib.qmhip_task_space_eval(itf.h, bad, pf.ptr(x), None, pf.ptr(mode), None, pf.ptr(rec)) == -1
