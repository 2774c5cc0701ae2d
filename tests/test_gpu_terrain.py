"""Plant terrain on the MI355X through the C ABI (qmhip_sim_set_terrain / qmhip_sim_get_ground / qmhip_terrain_eval, api.QMHWSim.set_terrain / ground / terrain_eval): the
checks of tests/test_terrain.py with the same shapes and the same assertions (tests/terrain_ref.py), the host-carried plant against the device loop with terrain, pushes and
sensors all set, the pipelined loop, the Python front, one full batch."""
import numpy as np
import pytest

import push_ref as pr
import sense_ref as sr
import terrain_ref as tr

pytestmark = pytest.mark.gpu


def test_lookup_exact_at_the_edges(blobs):
    tr.check_lookup(lambda B: tr.DevPlant(blobs, B), "device lookup")


def test_plant_on_terrain_vs_reference(blobs, oracle):
    tr.check_plant_vs_reference(lambda B: tr.DevPlant(blobs, B), oracle, "device plant")


def test_independent_properties(blobs, oracle):
    tr.check_properties(lambda B: tr.DevPlant(blobs, B), oracle)


def test_flat_isolation_and_off(blobs, oracle):
    tr.check_flat_isolation_off(lambda B: tr.DevPlant(blobs, B), oracle, "device plant")


def test_error_codes_leave_the_terrain_untouched(blobs, oracle):
    tr.check_errors(lambda B: tr.DevPlant(blobs, B), oracle)


def test_host_carried_plant_reproduces_closed_loop_sim_with_terrain_pushes_and_sensors(blobs):
    """after test_host_carried_plant_reproduces_closed_loop_sim_with_pushes (tests/test_gpu_push.py): QMHWSim.closed_loop against the same ticks carried by hand —
    QMController.update on sim.measured(), sim.setCommand, sim.step — with the same terrain, schedule and sensor records set, bit for bit in q, v and the ground records
    over 20 ticks"""
    from qm_control_amd import api
    from test_gpu_tick import _set_command
    c, q0, t_start = tr.loop_setup(); B = 2; v0 = np.zeros((B, 24)); ts = tr.loop_terrain(q0); p = tr.loop_pushes(t_start); s = sr.loop_records(); horizon = tr._horizon()

    def ctx():
        d = tr.DevPlant(blobs, B, nev=c["ev"].shape[1], nmax=128, c=c); assert d.set_terrain(ts) == tr.OK and d.set_pushes(p) == tr.OK and d.set_sensors(s) == tr.OK; d.reset(q0, v0, t_start)
        return d
    a = ctx(); ref = []
    for k in range(tr.N_TICKS):
        st = a.closed_loop(1, tr.PERIOD, horizon, tr.NSUB, tr.EVERY); assert (st["mpc_status"] >= 0).all() and (st["qp_status"] == 0).all(), k
        ref.append((st["q"], st["v"], a.ground()[1].copy(), a.push_state()[2].copy()))
    a.close()
    b = ctx(); ctl = api.QMController(b.itf, B, 0, 0.0, 0.5, tr.EVERY); ctl.starting(); contact = b.sim.rbd()[1]
    for k in range(tr.N_TICKS):
        rec = ctl.update(b.sim.state()["time"], b.sim.measured()[0], contact, horizon=horizon, period=tr.PERIOD); _set_command(b.sim, rec); _, contact = b.sim.step(tr.PERIOD, tr.NSUB); st = b.sim.state()
        assert np.array_equal(st["q"], ref[k][0]) and np.array_equal(st["v"], ref[k][1]) and np.array_equal(b.ground()[1], ref[k][2]) and np.array_equal(b.push_state()[2], ref[k][3]), k
    assert [int(r[3][1]) for r in ref] == [0] * 3 + [1] * 9 + [0] * 8 and ref[-1][2][1, :, 0].any() and not ref[-1][2][0, :, 0].any()      # the push over ticks 3-11; rough ground under robot 1 only
    b.close()


def test_pipelined_loop_picks_the_terrain_up(blobs):
    tr.check_loop(lambda c: tr.DevPlant(blobs, 2, nev=c["ev"].shape[1], nmax=128, c=c), True, "device pipelined loop")


def test_python_front(blobs, oracle):
    """api.QMHWSim.set_terrain takes [B] headers of dtype TERRAIN and [B][ny][nx] arrays of any float dtype, mu=None is the global coefficient, set_terrain(None) switches
    off, a refused grid raises; ground() is [B][4][6], terrain_eval() [B][n][4]"""
    from qm_control_amd import api
    cases = pr.plant_cases(oracle, pr._ost())[:2]; itf = api.QMInterface(blobs=blobs, max_batch=2, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf)
    hdr = np.zeros(2, api.TERRAIN); hdr["x0"] = -1.0; hdr["y0"] = -1.0; hdr["dx"] = 1.0; hdr["dy"] = 0.5
    H = np.zeros((2, 5, 3), np.float32); H[1, :, 2] = 0.25      # robot 1: a ramp of slope 0.25 beyond x = 0
    sim.set_terrain(hdr, H)
    out = sim.terrain_eval(np.array([[[0.5, 0.25]], [[0.5, 0.25]]])); assert out.shape == (2, 1, 4) and out.dtype == np.float64
    assert np.array_equal(out[0, 0], [0.0, 0.0, 0.0, 0.8]) and np.array_equal(out[1, 0], [0.125, 0.25, 0.0, 0.8])
    sim.reset(pr._arr(cases, "q"), pr._arr(cases, "v"), 1.0); sim.setCommand(*[pr._arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); g = sim.ground(); assert g.shape == (2, 4, 6) and not g.any()
    sim.step(0.001, 2, download=False); g = sim.ground(); assert (g[:, :, 4] == 0.8).all() and (g[0, :, 3] == 1.0).all() and g[:, :, 5].any()
    sim.set_terrain(hdr, H.astype(float), mu=np.full((2, 5, 3), 0.25)); sim.step(0.001, 2, download=False); assert (np.abs(sim.ground()[:, :, 4] - 0.25) <= 1e-15).all()
    sim.set_terrain(None); sim.step(0.001, 2, download=False); assert not sim.ground().any()
    with pytest.raises(api.QmhipError, match="no terrain"):
        sim.terrain_eval(np.zeros((2, 1, 2)))
    hdr["dx"][1] = 0.0
    with pytest.raises(api.QmhipError, match="dx / dy"):
        sim.set_terrain(hdr, H)
    itf.close()


def test_full_batch(blobs, oracle):
    """B = 1024, one random 16 x 16 grid of +-10 mm and friction 0.3 .. 1 each, 3 plant steps while standing (the setup of test_gpu_push.test_full_batch): status 0 and
    everything finite everywhere; 8 instances spread over the batch against the reference at the plant's tolerances, ground records included"""
    from test_sim import nominal_q, stand_height
    import pyoracle
    mb, st = blobs; B, steps = 1024, 3; rng = np.random.default_rng(4); z0 = stand_height(oracle, st); omb, ost = pyoracle.load_blobs(); ref = tr.TerrainRef(oracle, omb, ost)
    q = np.tile(nominal_q(st, z0 + 0.004), (B, 1)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18)); q[:, 0:2] += rng.uniform(-2.0, 2.0, (B, 2))
    hdr = np.zeros(B, api_terrain()); hdr["dx"] = 0.08; hdr["dy"] = 0.08; hdr["x0"] = q[:, 0] - 0.6; hdr["y0"] = q[:, 1] - 0.6
    H = 0.010 * rng.uniform(-1.0, 1.0, (B, 16, 16)); MU = rng.uniform(0.3, 1.0, (B, 16, 16))
    d = tr.DevPlant(blobs, B); assert d.set_terrain_raw(B, 16, 16, hdr, H, MU) == tr.OK; d.reset(q, np.zeros((B, 24)), 0.0)
    kp = np.concatenate([np.full(12, 300.0), np.full(6, 20.0)]); kd = np.concatenate([np.full(12, 3.0), np.full(6, 0.5)]); d.command(q[:, 6:], 0.0, kp, kd, 0.0)
    for k in range(steps):
        s = d.step_all(tr.PERIOD, tr.NSUB)
    assert (s["status"] == 0).all() and all(np.isfinite(s[n]).all() for n in ("q", "v", "rbd", "force", "ground")) and (s["contact"].sum(axis=1) > 0).mean() > 0.5
    for b in range(60, B, 128):
        case = dict(q=q[b], v=np.zeros(24), pos=q[b, 6:], vel=np.zeros(18), kp=kp, kd=kd, ff=np.zeros(18))
        r = ref.run(case, None, steps, tr.PERIOD, tr.NSUB, 0.0, tr.terrain(tuple(hdr[b]), H[b], MU[b]))[-1]
        e = dict(q=tr.rel_err(s["q"][b], r["q"]), v=tr.rel_err(s["v"][b], r["v"]), force=tr.rel_err(s["force"][b], r["force"]), rbd=tr.rel_err(s["rbd"][b], r["rbd"]), time=abs(s["time"][b] - r["time"]))
        assert all(e[n] < tr.TOL[n] for n in e) and tr.ground_err(s["ground"][b], r["ground"], 0.02) <= 1e-12 and list(s["contact"][b]) == list(r["contact"]), (b, e)
    d.close()


def api_terrain():
    from qm_control_amd import api
    return api.TERRAIN
