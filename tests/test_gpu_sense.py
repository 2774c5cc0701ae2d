"""Sensor model on the MI355X through the C ABI (qmhip_sim_set_sensors / qmhip_sim_get_measured, api.QMHWSim.set_sensors / measured): the checks of tests/test_sense.py with
the same shapes and the same assertions (tests/sense_ref.py), the host-carried plant against the device loop, one full batch."""
import numpy as np
import pytest

import push_ref as pr
import sense_ref as sr

pytestmark = pytest.mark.gpu


def loop_plant(blobs):
    return lambda c: sr.DevPlant(blobs, 2, nev=c["ev"].shape[1], nmax=128, c=c)


def test_generator_through_the_plant(blobs, oracle):
    p = sr.DevPlant(blobs, 1); sr.check_generator_through_plant(p, oracle); p.close()


def test_measured_state_vs_reference(blobs, oracle):
    p = sr.DevPlant(blobs, 4); sr.check_plant_vs_reference(p, oracle, "device plant"); p.close()


def test_off_means_off(blobs):
    sr.check_off_means_off(loop_plant(blobs), "device synchronous loop")


@pytest.mark.parametrize("pipelined", [False, True])
def test_loops_pick_the_sensors_up(blobs, pipelined):
    """the levels of tests/test_sense.py::test_loops_pick_the_sensors_up, as stated in the issue"""
    sr.check_loop(loop_plant(blobs), "device %s loop" % ("pipelined" if pipelined else "synchronous"), pipelined)


def test_error_codes_leave_the_records_in_force(blobs, oracle):
    sr.check_errors(lambda B: sr.DevPlant(blobs, B), oracle)


def test_python_front(blobs, oracle):
    """api.QMHWSim.set_sensors takes [B] records or None, a refused record raises; measured() returns (rbd, samples)"""
    from qm_control_amd import api
    cases = pr.plant_cases(oracle, pr._ost())[:2]; itf = api.QMInterface(blobs=blobs, max_batch=2, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf)
    s = sr.sensors(2); sr.record(s, 1, 9, 1, sr.SIGMA); sim.set_sensors(s)
    sim.reset(pr._arr(cases, "q"), pr._arr(cases, "v"), 1.0); sim.setCommand(*[pr._arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); r0 = sim.rbd()[0]
    truth, _ = sim.step(0.001, 2); m, n = sim.measured()
    assert n.tolist() == [1, 1] and np.array_equal(m[0], truth[0]) and np.array_equal(m[1, :48], sr.corrupt(r0[1], s[1], 1)) and np.array_equal(sim.rbd()[0], truth)
    sim.set_sensors(None); truth, _ = sim.step(0.001, 2); m, n = sim.measured(); assert not n.any() and np.array_equal(m, truth)
    s["lag"][0] = api.SENSE_MAX_LAG + 1
    with pytest.raises(api.QmhipError, match="lag"):
        sim.set_sensors(s)
    itf.close()


def test_host_carried_plant_reproduces_closed_loop_sim_with_sensors(blobs):
    """after test_host_carried_plant_reproduces_closed_loop_sim_with_pushes (tests/test_gpu_push.py): QMHWSim.closed_loop against the same ticks carried by hand —
    QMController.update on sim.measured(), sim.setCommand, sim.step — with the same records set, bit for bit in q and v over 24 ticks"""
    from qm_control_amd import api
    from test_gpu_tick import _set_command
    from test_push import loop_setup, N_TICKS, EVERY, HORIZON
    c, q0, t_start = loop_setup(); B = 2; s = sr.loop_records(); v0 = np.zeros((B, 24))

    def ctx():
        d = sr.DevPlant(blobs, B, nev=c["ev"].shape[1], nmax=128, c=c); assert d.set_sensors(s) == sr.OK; d.reset(q0, v0, t_start)
        return d
    a = ctx(); ref = []
    for k in range(N_TICKS):
        st = a.closed_loop(1, sr.PERIOD, HORIZON, sr.NSUB, EVERY); assert (st["mpc_status"] >= 0).all() and (st["qp_status"] == 0).all(), k
        ref.append((st["q"], st["v"], a.measured()[1].copy()))
    a.close()
    b = ctx(); ctl = api.QMController(b.itf, B, 0, 0.0, 0.5, EVERY); ctl.starting(); contact = b.sim.rbd()[1]
    for k in range(N_TICKS):
        rec = ctl.update(b.sim.state()["time"], b.sim.measured()[0], contact, horizon=HORIZON, period=sr.PERIOD); _set_command(b.sim, rec); _, contact = b.sim.step(sr.PERIOD, sr.NSUB); st = b.sim.state()
        assert np.array_equal(st["q"], ref[k][0]) and np.array_equal(st["v"], ref[k][1]) and np.array_equal(b.sim.measured()[0], ref[k][2]), k
    assert not np.array_equal(ref[-1][2][1], b.sim.rbd()[0][1])      # instance 1 was controlled on something else than the truth
    b.close()


def test_full_batch(blobs, oracle):
    """B = 1024, random records with lags 0..8 and sigmas up to the loop tests' levels, 20 plant steps while standing (the setup of test_gpu_push.test_full_batch):
    everything finite, the measured components equal the numpy reference bit for bit, samples == 20.  Every sigma is positive, so the normalised error
    (m − x − bias) / sigma over the 20 samples is the statistical check of tests/test_sense.py::test_generator_statistics on the device's own output: 983 040 draws,
    |mean| < 5e-3, |std − 1| < 5e-3"""
    from test_sim import nominal_q, stand_height
    mb, st = blobs; B, steps = 1024, 20; rng = np.random.default_rng(3); z0 = stand_height(oracle, st)
    q = np.tile(nominal_q(st, z0 - 0.002), (B, 1)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18))
    s = sr.sensors(B); s["seed"] = rng.integers(0, 2 ** 64, B, dtype=np.uint64); s["lag"] = rng.integers(0, sr.MAX_LAG + 1, B)
    s["sigma"] = sr.SIGMA * rng.uniform(0.1, 1.0, (B, sr.NG)); s["bias_sigma"] = sr.SIGMA * rng.uniform(0.0, 1.0, (B, sr.NG)) * (rng.random((B, sr.NG)) < 0.5)
    d = sr.DevPlant(blobs, B); assert d.set_sensors(s) == sr.OK; d.reset(q, np.zeros((B, 24)), 0.0)
    kp = np.concatenate([np.full(12, 300.0), np.full(6, 20.0)]); kd = np.concatenate([np.full(12, 3.0), np.full(6, 0.5)]); d.command(q[:, 6:], 0.0, kp, kd, 0.0)
    truths = [d.sim.rbd()[0]]; sg = s["sigma"][:, sr.GROUP]; bias = s["bias_sigma"][:, sr.GROUP] * sr.nu(s["seed"][:, None], sr.BIAS_N, np.arange(48)[None, :]); errs = []
    c = np.arange(48)[None, :]; rows = np.arange(B); clean = (s["sigma"][:, sr.GROUP] == 0.0) & (s["bias_sigma"][:, sr.GROUP] == 0.0)
    for k in range(1, steps + 1):
        truth, _ = d.sim.step(sr.PERIOD, sr.NSUB); truths.append(truth); rc, m, n = d.measured(); assert rc == sr.OK and (n == k).all(), k
        src = np.stack(truths)[k - np.minimum(s["lag"], k), rows][:, :48]      # per instance the truth of sample k − min(lag, k)
        want = np.where(clean, src, (src + bias) + sg * sr.nu(s["seed"][:, None], np.uint64(k), c))
        assert np.array_equal(m[:, :48], want) and np.isfinite(m).all(), (k, np.abs(m[:, :48] - want).max())
        errs.append((m[:, :48] - src - bias) / sg)
    e = np.stack(errs); print("device, normalised error over %d draws: mean %.2e std - 1 %.2e max %.4f" % (e.size, e.mean(), e.std() - 1.0, np.abs(e).max()))
    assert e.size == 983040 and abs(e.mean()) < 5e-3 and abs(e.std() - 1.0) < 5e-3
    st_ = d.state(); assert (st_["status"] == 0).all() and np.isfinite(st_["q"]).all() and np.isfinite(st_["v"]).all() and np.isfinite(st_["rbd"]).all()
    assert len(set(s["lag"].tolist())) == sr.MAX_LAG + 1
    d.close()
