"""Streamed controller tick (qmhip_tick_reset / _submit / _collect, qmhip_observe; include/qmhip.h) on the device, through the C ABI / api.QMController.

The plant is the library's own, carried by the host (qmhip_sim_step / qmhip_sim_set_command) as a stand-in for an external one; the answer is qmhip_closed_loop_sim's,
which tests/test_gpu_sim.py pins to the oracle's loop — bit for bit, the tick launches the kernels that loop launches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, block_errs

pytestmark = pytest.mark.gpu
PERIOD, NSUB, HORIZON, NMAX = 0.001, 2, 0.45, 64


def _setup(gait, B, t_start):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    return setup(gait, B, HORIZON, t_start=t_start)


def _start_states(c, B, seed=3):
    rng = np.random.default_rng(seed); q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385
    q[:, 2] += 0.002 * rng.random(B); q[:, 3:6] += 0.01 * rng.normal(size=(B, 3)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18))
    return q, 0.02 * rng.normal(size=(B, 24))


def _ctx(blobs, c, B, controller=0, feedback=False):
    from qm_control_amd import api
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=NMAX, max_ref_knots=2, max_events=c["ev"].shape[1])
    mpc = api.SqpMpc(itf); wbc = api.HierarchicalWbc(itf); sim = api.QMHWSim(itf, robust_grid=True, feedback_policy=feedback)
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); wbc.reset(); sim.set_controller(controller)
    return itf, mpc, wbc, sim


def _device_loop(blobs, c, q0, v0, t_start, controller, feedback, mpc_every, kp, kd, n_ticks):
    B = q0.shape[0]; itf, mpc, wbc, sim = _ctx(blobs, c, B, controller, feedback); sim.reset(q0, v0, t_start); ref = []
    for k in range(n_ticks):
        sim.closed_loop(1, PERIOD, HORIZON, n_substeps=NSUB, mpc_every=mpc_every, arm_kp=kp, arm_kd=kd)
        s = sim.state(); out, qps = wbc.download(B); ref.append(dict(q=s["q"], v=s["v"], out=out, qps=qps, mst=mpc.download()["status"]))
    itf.close()
    return ref


def _set_command(sim, rec):
    cmd = rec["cmd"].reshape(len(rec), 5, 18); sim.setCommand(*[np.ascontiguousarray(cmd[:, i]) for i in range(5)])


def _tick_loop(blobs, c, q0, v0, t_start, controller, feedback, mpc_every, kp, kd, n_ticks, yaw_shift=None):
    """the plant stepped by the host, the controller through api.QMController; yaw_shift [n_ticks]: multiples of 2 pi added to the measured yaw"""
    from qm_control_amd import api
    B = q0.shape[0]; itf, mpc, wbc, sim = _ctx(blobs, c, B, controller, feedback); sim.reset(q0, v0, t_start)
    ctl = api.QMController(itf, B, controller, kp, kd, mpc_every); ctl.starting()
    rbd, contact = sim.rbd(); recs = []; plant = []
    for k in range(n_ticks):
        time = sim.state()["time"]      # the plant's own time, not a host sum
        if yaw_shift is not None:
            rbd = rbd.copy(); rbd[:, 0] += 2.0 * np.pi * yaw_shift[k]
        rec = ctl.update(time, rbd, contact, horizon=HORIZON, period=PERIOD); recs.append(rec)
        _set_command(sim, rec); rbd, contact = sim.step(PERIOD, NSUB); s = sim.state(); plant.append(dict(q=s["q"], v=s["v"]))
    itf.close()
    return recs, plant


LOOP_CASES = [(64, "trot", 20.2, 0, 0, 5), (8, "trot", 5.2, 1, 1, 5), (8, "stance", 5.2, 0, 0, 1), (8, "stance", 20.2, 0, 1, 5)]


@pytest.mark.parametrize("B,gait,t_start,controller,feedback,mpc_every", LOOP_CASES)
def test_host_carried_plant_reproduces_closed_loop_sim(blobs, B, gait, t_start, controller, feedback, mpc_every):
    n = 24; kp, kd = (60.0, 2.0) if controller == 1 else (0.0, 0.5)
    c = _setup(gait, B, t_start); q0, v0 = _start_states(c, B)
    ref = _device_loop(blobs, c, q0, v0, t_start, controller, bool(feedback), mpc_every, kp, kd, n)
    recs, plant = _tick_loop(blobs, c, q0, v0, t_start, controller, bool(feedback), mpc_every, kp, kd, n)
    for k in range(n):
        r = ref[k]; rec = recs[k]
        assert (r["mst"] >= 0).all() and (r["qps"] == 0).all(), (k, r["mst"], r["qps"])
        assert plant[k]["q"].tobytes() == r["q"].tobytes() and plant[k]["v"].tobytes() == r["v"].tobytes(), (k, np.abs(plant[k]["q"] - r["q"]).max(), np.abs(plant[k]["v"] - r["v"]).max())
        assert rec["wbc_out"].tobytes() == r["out"].tobytes() and np.array_equal(rec["qp_status"], r["qps"]) and np.array_equal(rec["mpc_status"], r["mst"]), k
        assert (rec["mpc_ran"] == int(k % mpc_every == 0)).all() and (rec["tick"] == k).all() and not rec["safety"].any() and not rec["stopped"].any()
    assert not np.array_equal(ref[0]["out"][0], ref[0]["out"][1]) and not np.array_equal(ref[0]["out"], ref[-1]["out"])


def test_two_pi_shifts_of_the_measured_yaw_do_not_matter(blobs):
    B, n, t_start = 8, 24, 20.2; c = _setup("trot", B, t_start); q0, v0 = _start_states(c, B)
    shift = np.array([0, 1, 1, -1, 0, 0, 1, -1, -1, 0, 1, 0, -1, 1, 0, 0, -1, -1, 1, 1, 0, -1, 0, 1])
    base, _ = _tick_loop(blobs, c, q0, v0, t_start, 0, False, 5, 0.0, 0.5, n)
    recs, _ = _tick_loop(blobs, c, q0, v0, t_start, 0, False, 5, 0.0, 0.5, n, yaw_shift=shift)
    yaw = np.array([r["x_obs"][:, 9] for r in recs])
    assert np.abs(np.diff(yaw, axis=0)).max() < np.pi and np.abs(yaw).max() < 1.0
    worst = {}
    for k in range(n):
        assert (recs[k]["mpc_status"] >= 0).all() and (base[k]["mpc_status"] >= 0).all(), k
        for name, kind in (("x_obs", "x"), ("x_des", "x"), ("u_des", "u"), ("wbc_out", "wbc")):
            for blk, e in block_errs(recs[k][name], base[k][name], kind).items():
                worst[name + " " + blk] = max(worst.get(name + " " + blk, 0.0), e)
    print("2 pi shifts, worst per-block relative difference over %d ticks: %s" % (n, {k: "%.1e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1e-6, worst


def test_safety_stop_on_the_device(blobs):
    B, t_start, kp, kd = 3, 5.2, 60.0, 2.0; c = _setup("stance", B, t_start); q0, v0 = _start_states(c, B)
    from qm_control_amd import api
    itf, mpc, wbc, sim = _ctx(blobs, c, B, 1); sim.reset(q0, v0, t_start); rbd0, _ = sim.rbd()
    ctl = api.QMController(itf, B, 1, kp, kd, 5)

    def run(ctl, keep):
        ctl.starting(); recs = []
        for k in range(12):
            rbd = rbd0.copy(); rbd[:, 0] += 0.01 * (k + 1) * np.array([1.0, -2.0, 3.0]); rbd[1, 2] = 0.22 * k + (0.06 if k >= 7 else 0.0)
            if k == 3:
                rbd[0, 2] = np.pi / 2; rbd[2, 2] = -np.pi / 2      # exactly +-pi/2 passes: the reference's comparison is strict
            recs.append(ctl.update(t_start + 0.004 * k, rbd[keep], horizon=HORIZON, period=PERIOD))
        return recs
    recs = run(ctl, [0, 1, 2])
    for k in range(12):
        assert list(recs[k]["safety"]) == [0, int(k >= 7), 0] and list(recs[k]["stopped"]) == [0, int(k >= 8), 0] and (recs[k]["mode_meas"] == -1).all(), k
    assert recs[7]["cmd"][1].tobytes() != recs[6]["cmd"][1].tobytes()
    for k in range(8, 12):
        assert recs[k]["cmd"][1].tobytes() == recs[7]["cmd"][1].tobytes() and recs[k]["cmd"][0].tobytes() != recs[7]["cmd"][0].tobytes(), k
        assert recs[k]["x_obs"][1, 9] != recs[7]["x_obs"][1, 9]      # still observed and reported
    again = run(ctl, [0, 1, 2])      # tick_reset clears the flag: the same episode again, the same records
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, recs))
    itf.close()
    itf2, mpc2, wbc2, sim2 = _ctx(blobs, {k: (v[[0, 2]] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == B else v) for k, v in c.items()}, 2, 1)
    two = run(api.QMController(itf2, 2, 1, kp, kd, 5), [0, 2]); itf2.close()
    for k in range(12):
        assert recs[k][[0, 2]].tobytes() == two[k].tobytes(), k


def test_observe_equals_the_first_ticks_observation(blobs):
    from qm_control_amd import api
    from test_sim import centroidal_from_rbd
    B, t_start = 8, 20.2; c = _setup("stance", B, t_start); q0, v0 = _start_states(c, B)
    itf, mpc, wbc, sim = _ctx(blobs, c, B); sim.reset(q0, v0, t_start); rbd, contact = sim.rbd()
    rng = np.random.default_rng(4); rbd[:, 0] = rng.uniform(-3.1, 3.1, B); rbd[:, 24:30] = rng.normal(size=(B, 6))
    x = itf.observe(rbd)
    ctl = api.QMController(itf, B); ctl.starting(); rec = ctl.update(t_start, rbd, contact, horizon=HORIZON, period=PERIOD)
    assert rec["x_obs"].tobytes() == x.tobytes() and (rec["mpc_status"] >= 0).all()
    assert np.abs(x - np.array([centroidal_from_rbd(blobs[0], r) for r in rbd])).max() < 1e-12
    itf.close()


def test_error_returns_and_interleaving(blobs):
    from qm_control_amd import api
    B, t_start = 4, 20.2; c = _setup("stance", B, t_start); q0, v0 = _start_states(c, B)
    itf, mpc, wbc, sim = _ctx(blobs, c, B); sim.reset(q0, v0, t_start); rbd, contact = sim.rbd(); lib = itf.lib
    time = np.full(B, t_start); rec = np.zeros(B, api.TICK_RECORD); ERR_ARG, ERR_STATE = -1, -5
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def submit(h=None, B_=B, t=time, r=rbd, horizon=HORIZON, period=PERIOD):
        return lib.qmhip_tick_submit(h or itf.h, B_, dp(t), dp(r), None, C.c_double(horizon), C.c_double(period))

    def collect(B_=B, r=rec):
        return lib.qmhip_tick_collect(itf.h, B_, None if r is None else r.ctypes.data_as(C.c_void_p))

    def reset(B_=B, controller=0, every=5):
        return lib.qmhip_tick_reset(itf.h, B_, controller, C.c_double(0.0), C.c_double(0.5), every)

    def failed(rc, want):
        assert rc == want, (rc, want)
        assert len(lib.qmhip_last_error(itf.h)) > 0
    failed(submit(), ERR_STATE)                                        # a tick before tick_reset
    failed(collect(), ERR_STATE)                                       # nothing in flight
    failed(reset(every=0), ERR_ARG); failed(reset(B_=B + 1), ERR_ARG); failed(reset(controller=2), ERR_ARG)
    assert reset() == 0
    failed(submit(B_=B - 1), ERR_ARG); failed(submit(t=None), ERR_ARG); failed(submit(r=None), ERR_ARG); failed(submit(horizon=0.0), ERR_ARG); failed(submit(period=-1.0), ERR_ARG)
    assert submit() == 0
    failed(submit(), ERR_STATE)                                        # depth is one
    failed(lib.qmhip_step_submit(itf.h, B, dp(time), dp(np.ascontiguousarray(c["x0"])), None, C.c_double(HORIZON), C.c_double(PERIOD), C.c_double(t_start), C.c_uint(1)), ERR_STATE)
    xd = np.zeros((B, 30)); failed(lib.qmhip_policy_eval_feedback(itf.h, B, dp(time), dp(xd), dp(xd), dp(xd), None), ERR_STATE)
    failed(collect(B_=B - 1), ERR_ARG); failed(collect(r=None), ERR_ARG)
    assert collect() == 0 and (rec["mpc_status"] >= 0).all() and (rec["mpc_ran"] == 1).all()
    failed(collect(), ERR_STATE)
    # a streamed step is accepted after the collect, refuses a tick while it is in flight, and the ticks go on afterwards
    x0 = itf.observe(rbd)
    mpc.step_submit(time, x0, rbd, horizon=HORIZON, period=PERIOD, time=t_start, flags=api.STEP_WBC)
    failed(submit(), ERR_STATE)
    assert (mpc.step_collect()["status"] >= 0).all()
    assert submit() == 0 and collect() == 0 and (rec["tick"] == 1).all() and (rec["mpc_ran"] == 0).all() and (rec["mpc_status"] >= 0).all()
    # an upload drops the solution: a tick without an MPC call has no policy
    mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); failed(submit(), ERR_STATE)
    assert reset() == 0 and submit() == 0 and collect() == 0 and (rec["tick"] == 0).all()
    witf = itf.wbc_context(); rc = submit(h=witf.h); assert rc == ERR_STATE and len(lib.qmhip_last_error(witf.h)) > 0
    witf.close(); itf.close()
