"""Streamed control-step I/O (qmhip_step_submit / qmhip_step_collect, include/qmhip.h) against the entry points it stands beside.  The feature moves bits, it does not
recompute them: every comparison is np.array_equal.  Each test first asserts status >= 0 on the EXISTING path, so a bad input cannot pass as two failures agreeing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -7.25e300, -123456789      # what the caller's trajectory arrays hold before a collect
DT = 0.02
SHAPES = [dict(batch=64, n_intervals=40, max_nodes=80), dict(batch=4, n_intervals=20, max_nodes=48)]      # tests/test_gpu_mpc.py's batch, the smoke shape
KERNELS = ["grid", "lq_kin", "lq", "lq_m18", "riccati", "ls_eval", "ls_misc", "policy", "wbc", "sim", "rollout", "ipm", "hoqp", "io"]


def _ctx(blobs, shape, **kw):
    from qm_control_amd import api, scenarios
    cfg = scenarios.make_config("C3", batch=shape["batch"], n_intervals=shape["n_intervals"])
    itf = api.QMInterface(blobs=blobs, max_batch=shape["batch"], max_nodes=shape["max_nodes"], max_ref_knots=cfg["ref_t"].shape[1], max_events=cfg["ev"].shape[1], **kw)
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf)
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); wbc.reset()
    return cfg, itf, mpc, wbc


def _existing(mpc, wbc, t0, with_wbc=True):
    """what the existing entry points hand over after a step: download + wbc.download + the policy at t0"""
    B = mpc.B; r = mpc.download()
    out, qps = wbc.download(B) if with_wbc else (np.zeros((B, 54)), np.zeros((B, 3), np.int32))
    xd, ud, mode = mpc.evaluatePolicy(t0)
    assert (r["status"] >= 0).all(), r["status"]
    if with_wbc:
        assert (qps == 0).all(), qps
    r.update(wbc_out=out, qp_status=qps, x_des=xd, u_des=ud, mode_t0=mode)
    return r


def _sentinels(B, nm):
    return dict(t=np.full((B, nm), SENT_F), event=np.full((B, nm), SENT_I, np.int32), mode=np.full((B, nm), SENT_I, np.int32), x=np.full((B, nm, 30), SENT_F), u=np.full((B, nm, 30), SENT_F))


def _assert_record(got, ref, what=""):
    for k in ("num_nodes", "status", "perf", "wbc_out", "qp_status", "x_des", "u_des", "mode_t0"):
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)
    assert not got["record"]["reserved"].any()


def _assert_traj(got, ref, what=""):
    for b, n in enumerate(ref["num_nodes"]):
        for k in ("t", "event", "mode", "x", "u"):
            assert np.array_equal(got[k][b, :n], ref[k][b, :n]), (what, k, b)
            assert (got[k][b, n:] == (SENT_F if got[k].dtype == np.float64 else SENT_I)).all(), (what, k, b, "memory behind n_nodes was written")


def _observations(blobs, shape, steps):
    """(t0, x0, time) of `steps` MPC calls of a sequential closed loop on a context of its own (advance along the policy): recorded once, then fed to both paths from the host"""
    cfg, itf, mpc, wbc = _ctx(blobs, shape); B = shape["batch"]; obs = []
    for k in range(steps):
        if k > 0:
            mpc.advance(DT)
        obs.append((itf.debug_read("t0", (B,)), itf.debug_read("x0", (B, 30)), cfg["time"] + k * DT))
        mpc.closed_loop_resident(1, DT, cfg["horizon"], cfg["period"], obs[-1][2])
    assert (mpc.download()["status"] >= 0).all()
    itf.close()
    assert not np.array_equal(obs[0][1], obs[-1][1])
    return obs


@pytest.mark.parametrize("shape", SHAPES, ids=["B64_N40", "B4_N20"])
def test_cold_step_with_wbc_and_trajectories(blobs, shape):
    from qm_control_amd import api
    B, nm = shape["batch"], shape["max_nodes"]
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.control_step_resident(cfg["horizon"], cfg["period"], cfg["time"]); ref = _existing(mpc, wbc, cfg["t0"]); itf.close()
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    assert mpc.steps_in_flight() == 0
    mpc.step_submit(cfg["t0"], cfg["x0"], None, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"], flags=api.STEP_WBC | api.STEP_TRAJ)
    assert mpc.steps_in_flight() == 1
    got = mpc.step_collect(out=_sentinels(B, nm))
    assert mpc.steps_in_flight() == 0
    assert ref["num_nodes"].min() >= 3 and ref["num_nodes"].max() < nm and np.abs(ref["wbc_out"]).max() > 0
    _assert_record(got, ref); _assert_traj(got, ref)
    # the existing hand-over still works on the context that streamed, and sees the same solution
    again = mpc.download(); assert np.array_equal(again["x"], ref["x"]) and np.array_equal(again["u"], ref["u"])
    itf.close()


def _warm_chain_existing(blobs, shape, obs):
    cfg, itf, mpc, wbc = _ctx(blobs, shape); refs = []
    for t0, x0, time in obs:
        mpc.set_initial(t0, x0); mpc.closed_loop_resident(1, DT, cfg["horizon"], cfg["period"], time); refs.append(_existing(mpc, wbc, t0))
    itf.close()
    return cfg, refs


@pytest.mark.parametrize("shape", SHAPES, ids=["B64_N40", "B4_N20"])
def test_warm_chain_and_depth_two(blobs, shape):
    """6 steps on host-supplied observations: submit / collect per step equals set_initial + closed_loop_resident(1) + downloads at every step, and so does the chain
    with step k + 1 submitted BEFORE step k is collected — nothing of step k + 1 may overwrite what the pack of step k reads"""
    from qm_control_amd import api
    B, nm = shape["batch"], shape["max_nodes"]; steps = 6
    obs = _observations(blobs, shape, steps)
    cfg, refs = _warm_chain_existing(blobs, shape, obs)
    assert not np.array_equal(refs[0]["wbc_out"], refs[-1]["wbc_out"])
    flags = api.STEP_WBC | api.STEP_TRAJ; kw = dict(horizon=cfg["horizon"], period=cfg["period"])
    # depth 1
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    for k, (t0, x0, time) in enumerate(obs):
        mpc.step_submit(t0, x0, None, time=time, flags=flags, **kw); got = mpc.step_collect(out=_sentinels(B, nm))
        _assert_record(got, refs[k], k); _assert_traj(got, refs[k], k)
    itf.close()
    # depth 2
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.step_submit(obs[0][0], obs[0][1], None, time=obs[0][2], flags=flags, **kw)
    for k in range(steps):
        if k + 1 < steps:
            mpc.step_submit(obs[k + 1][0], obs[k + 1][1], None, time=obs[k + 1][2], flags=flags, **kw); assert mpc.steps_in_flight() == 2
        got = mpc.step_collect(out=_sentinels(B, nm))
        _assert_record(got, refs[k], ("depth 2", k)); _assert_traj(got, refs[k], ("depth 2", k))
    assert mpc.steps_in_flight() == 0
    itf.close()


def test_measured_state_supplied(blobs, oracle):
    from qm_control_amd import api
    from wbc_cases import random_wbc_inputs
    shape = SHAPES[0]; B = shape["batch"]
    rbd = np.array([c["rbd"] for c in random_wbc_inputs(oracle, blobs, B, 77, 0.3)])
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.set_initial(cfg["t0"], cfg["x0"]); mpc.solve_resident(cfg["horizon"], warm=True)
    assert (mpc.download()["status"] >= 0).all()
    xd, ud, mode = mpc.evaluatePolicy(cfg["t0"])
    out, qps = wbc.update(xd, ud, rbd, mode, cfg["period"], np.full(B, cfg["time"])); itf.close()
    assert (qps == 0).all() and np.abs(out).max() > 0
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.step_submit(cfg["t0"], cfg["x0"], rbd, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"], flags=api.STEP_WBC); got = mpc.step_collect()
    assert np.array_equal(got["wbc_out"], out) and np.array_equal(got["qp_status"], qps) and np.array_equal(got["x_des"], xd) and np.array_equal(got["u_des"], ud) and np.array_equal(got["mode_t0"], mode)
    # and it is the supplied state that was used, not the synthetic one
    mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); wbc.reset()
    mpc.step_submit(cfg["t0"], cfg["x0"], None, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"], flags=api.STEP_WBC)
    assert not np.array_equal(mpc.step_collect()["wbc_out"], out)
    itf.close()


def test_without_the_wbc_flag(blobs, oracle):
    from qm_control_amd import api
    from wbc_cases import random_wbc_inputs
    shape = SHAPES[0]; B, nm = shape["batch"], shape["max_nodes"]
    case = random_wbc_inputs(oracle, blobs, B, 78, 0.3)
    wargs = lambda cfg: (np.array([c["xd"] for c in case]), np.array([c["ud"] for c in case]), np.array([c["rbd"] for c in case]), np.array([c["mode"] for c in case], np.int32), cfg["period"], np.full(B, 20.0))
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.set_initial(cfg["t0"], cfg["x0"]); mpc.solve_resident(cfg["horizon"], warm=True); ref = _existing(mpc, wbc, cfg["t0"], with_wbc=False)
    out_ref, qps_ref = wbc.update(*wargs(cfg)); itf.close()
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    mpc.step_submit(cfg["t0"], cfg["x0"], None, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"], flags=api.STEP_TRAJ); got = mpc.step_collect(out=_sentinels(B, nm))
    assert not got["wbc_out"].any() and not got["qp_status"].any()
    _assert_record(got, ref); _assert_traj(got, ref)
    out, qps = wbc.update(*wargs(cfg))      # inputLast_ is as wbc.reset() left it: the first WBC update gives what it gives on a context that never streamed
    assert np.array_equal(out, out_ref) and np.array_equal(qps, qps_ref) and np.abs(out).max() > 0
    itf.close()


def test_error_returns(blobs):
    from qm_control_amd import api
    shape = SHAPES[1]; B, nm = shape["batch"], shape["max_nodes"]
    cfg, itf, mpc, wbc = _ctx(blobs, shape); lib = itf.lib
    t0 = np.ascontiguousarray(cfg["t0"]); x0 = np.ascontiguousarray(cfg["x0"]); rec = np.zeros(B, api.STEP_RECORD); tt = np.zeros((B, nm))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def submit(h=None, B_=B, t=t0, x=x0, horizon=cfg["horizon"], period=cfg["period"], flags=api.STEP_WBC):
        return lib.qmhip_step_submit(h or itf.h, B_, dp(t), dp(x), None, C.c_double(horizon), C.c_double(period), C.c_double(cfg["time"]), C.c_uint(flags))

    def collect(B_=B, r=rec, t=None):
        return lib.qmhip_step_collect(itf.h, B_, None if r is None else r.ctypes.data_as(C.c_void_p), dp(t), None, None, None, None)

    def failed(rc, want):
        assert rc == want, (rc, want)
        assert len(lib.qmhip_last_error(itf.h)) > 0
    ERR_ARG, ERR_STATE = -1, -5
    failed(collect(), ERR_STATE)                                      # nothing in flight
    failed(submit(B_=B - 1), ERR_ARG); failed(submit(B_=B + 1), ERR_ARG)      # not the upload's batch / beyond max_batch
    failed(submit(t=None), ERR_ARG); failed(submit(x=None), ERR_ARG)
    failed(submit(horizon=0.0), ERR_ARG); failed(submit(period=-1.0), ERR_ARG)
    assert lib.qmhip_step_in_flight(itf.h) == 0
    assert submit() == 0 and submit(flags=api.STEP_WBC | api.STEP_TRAJ) == 0 and lib.qmhip_step_in_flight(itf.h) == 2
    failed(submit(), ERR_STATE)                                       # a third step
    failed(collect(t=tt), ERR_STATE)                                  # trajectories of a step submitted without QMHIP_STEP_TRAJ
    failed(collect(B_=B - 1), ERR_ARG); failed(collect(r=None), ERR_ARG)
    assert lib.qmhip_step_in_flight(itf.h) == 2                        # a refused collect consumes nothing
    assert collect() == 0 and collect(t=tt) == 0 and lib.qmhip_step_in_flight(itf.h) == 0 and (rec["mpc_status"] >= 0).all() and tt.any()
    failed(collect(), ERR_STATE)
    # another entry point while a step is in flight orders itself behind it; the record stays collectable
    assert submit() == 0; r = mpc.download(); assert (r["status"] >= 0).all(); assert collect() == 0 and np.array_equal(rec["n_nodes"], r["num_nodes"])
    # WBC-only context
    witf = itf.wbc_context()
    rc = submit(h=witf.h); assert rc == ERR_STATE and len(lib.qmhip_last_error(witf.h)) > 0
    witf.close(); itf.close()


def test_resident_paths_launch_what_they_launched(blobs):
    """per-kernel launch counts of qmhip_control_step_resident on a context that has streamed equal those of a context that never did; the pack kernel has a name of its
    own ("io") and no launch there"""
    from qm_control_amd import api
    shape = SHAPES[1]

    def counts(itf, mpc, wbc, cfg):
        itf.set_profiling(1); itf.reset_kernel_ms()
        mpc.set_problem(cfg["t0"], cfg["x0"], cfg["ref_t"], cfg["ref_x"], cfg["ev"], cfg["modes"]); wbc.reset()
        mpc.control_step_resident(cfg["horizon"], cfg["period"], cfg["time"]); itf.synchronize()
        n = {k: itf.kernel_ms(k)[1] for k in KERNELS}; itf.set_profiling(0)
        assert (mpc.download()["status"] >= 0).all()
        return n
    cfg, itf, mpc, wbc = _ctx(blobs, shape); plain = counts(itf, mpc, wbc, cfg); itf.close()
    cfg, itf, mpc, wbc = _ctx(blobs, shape)
    itf.set_profiling(1)
    for k in range(2):
        mpc.step_submit(cfg["t0"], cfg["x0"], None, horizon=cfg["horizon"], period=cfg["period"], time=cfg["time"], flags=api.STEP_WBC | api.STEP_TRAJ); mpc.step_collect()
    itf.synchronize(); assert itf.kernel_ms("io")[1] == 4      # MPC half + WBC half per step (csrc/kernels/k_io.h)
    streamed = counts(itf, mpc, wbc, cfg); itf.close()
    assert plain == streamed and plain["io"] == 0 and plain["lq"] > 0 and plain["wbc"] == 1 and plain["riccati"] == 1, (plain, streamed)
