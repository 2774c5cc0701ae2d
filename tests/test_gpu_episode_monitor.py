"""Episode monitor on the device (qmhip_episode_*; csrc/kernels/k_episode.h): the checks of tests/test_episode_monitor.py through the C ABI.  The reference of every summary
is the numpy fold (tests/episode_ref.py) of data read back through entry points that exist without the monitor — closed_loop(1, ...) + state() / rbd() / WBC and MPC
download / the policy's mode — or of synthetic ticks.  NaN inputs reach the fold kernels only, never the plant, the MPC or the WBC."""
import os
import sys

import numpy as np
import pytest

import episode_ref as er
from conftest import ROOT
from qm_control_amd import api, layout as L

pytestmark = pytest.mark.gpu
PERIOD, NSUB, HORIZON, EVERY, T_START = 0.001, 2, 0.45, 8, 20.2
OUTPUTS = ("q", "v", "time", "wbc_out", "qp_status", "mpc_status", "x", "u")
DROP = 37


def _setup(B):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    return setup("trot", B, HORIZON, t_start=T_START)


def _start_states(c, B, seed=3):
    """B distinct start postures near the nominal stand, small velocities (a ragged batch)"""
    rng = np.random.default_rng(seed); q = np.tile(c["xbar"][6:30], (B, 1)); q[:, 2] = 0.385
    q[:, 2] += 0.002 * rng.random(B); q[:, 3:6] += 0.01 * rng.normal(size=(B, 3)); q[:, 6:] += 0.02 * rng.normal(size=(B, 18))
    v = 0.02 * rng.normal(size=(B, 24))
    if B > DROP:      # one instance starts at the low end of the heights, sinking at 0.3 m/s: within ten ticks it is millimetres below every other one — the instance the fall threshold isolates
        q[DROP, 2] = 0.385; v[DROP, 2] = -0.3
    return q, v


class Dev:
    """one device context with plant, controller and monitor"""

    def __init__(self, blobs, B, c=None, **simargs):
        self.B = B; self.c = c = _setup(B) if c is None else c
        self.itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=64, max_ref_knots=2, max_events=c["ev"].shape[1])
        self.mpc = api.SqpMpc(self.itf); self.wbc = api.HierarchicalWbc(self.itf); self.sim = api.QMHWSim(self.itf, robust_grid=True, **simargs)
        self.mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); self.wbc.reset()

    def reset(self, q0, v0):
        self.sim.reset(q0, v0, T_START)

    def loop(self, n, pipelined=False):
        self.sim.closed_loop(n, PERIOD, HORIZON, n_substeps=NSUB, mpc_every=EVERY, pipelined=pipelined)

    def readback(self, solution=True):
        """what a tick left, through entry points that exist without the monitor"""
        B = self.B; d = self.sim.state(); d["sim_status"] = d.pop("status"); d["rbd"], d["contact"] = self.sim.rbd(); d["wbc_out"], d["qp_status"] = self.wbc.download(B)
        d["mode"] = self.itf.debug_read("wbc_mode", (B,), np.int32)
        if solution:
            r = self.mpc.download(); d["mpc_status"] = r["status"]; d["x"] = r["x"]; d["u"] = r["u"]
        return d

    def close(self):
        self.itf.close()


def _taumax(blobs):
    return np.asarray(blobs[0][L.MB_TAUMAX:L.MB_TAUMAX + 18], float)


# ---------------------------------------------------------------- (1) fold on synthetic ticks
@pytest.mark.parametrize("patterns", [(0, 1, 2), (3, 4, 5), tuple(b % er.PATTERNS for b in range(65))], ids=["B3a", "B3b", "B65"])
def test_fold_on_synthetic_ticks_matches_the_numpy_fold(blobs, patterns):
    """B = 65 is one past the 64-thread block of the MPC-status kernel; the tick kernel runs one wavefront per instance"""
    taumax = _taumax(blobs); B = len(patterns); ticks, anchor = er.synthetic_ticks(patterns, taumax); ref, samples = er.fold_synthetic(ticks, anchor, taumax)
    er.check_synthetic_expectations(ref, patterns)
    itf = api.QMInterface(blobs=blobs, max_batch=B, max_nodes=8, max_ref_knots=2, max_events=2); sim = api.QMHWSim(itf); sim.B = B
    with pytest.raises(api.QmhipError):
        sim.episode_summary()      # monitor off
    sim.monitor(er.ZMIN, er.TILT, 5, 2); sim.set_anchor(anchor)
    with pytest.raises(api.QmhipError):
        sim.episode_summary()      # no episode yet
    for k, d in enumerate(ticks):
        api.episode_fold(itf, k, er.PERIOD, d["time"], d["rbd"], d["contact"], d["force"], d["mode"], d["wbc_out"], d["qp_status"], d["sim_status"], d["mpc_status"])
    got = sim.episode_summary(); er.compare_summary(got, ref.s, "device fold B=%d" % B)
    tr, count = sim.episode_trace(4); assert count == 3 and tr.shape == (2, B) and tr[0].tobytes() == samples[0].tobytes() and tr[1].tobytes() == samples[5].tobytes()
    tr, count = sim.episode_trace(); assert count == 3 and tr.shape == (2, B)
    sim.monitor(None)
    with pytest.raises(api.QmhipError):
        sim.episode_trace(1)
    itf.close()


# ---------------------------------------------------------------- (2) synchronous loop
def test_synchronous_loop_one_call_with_monitor_equals_per_tick_readback(blobs):
    """B = 65 ragged trot batch, 24 ticks, an MPC call every 8, trace_every 5 with trace_cap 3: five sampled ticks, three kept"""
    B, NT = 65, 24; taumax = _taumax(blobs)
    d = Dev(blobs, B); q0, v0 = _start_states(d.c, B); d.reset(q0, v0); rb0 = d.readback(solution=False); per = []
    for k in range(NT):
        d.loop(1); r = d.readback(solution=(k % EVERY == 0 or k == NT - 1))
        if "mpc_status" not in r:
            r["mpc_status"] = per[-1]["mpc_status"]      # no call on this tick: the solver's status words stay
        per.append(r)
    d.close()
    z = np.array([r["rbd"][:, 5] for r in per]); bf, kf, zmin = er.fall_threshold(z); print("instance %d falls at tick %d: min_base_z = %.17g" % (bf, kf, zmin))
    e = Dev(blobs, B); e.sim.monitor(zmin, 0.8, 5, 3); e.reset(q0, v0); e.loop(NT); on = e.readback()
    for name in OUTPUTS:
        assert np.array_equal(on[name], per[-1][name]), name
    ref = er.Fold(B, rb0["rbd"][:, 48:55], rb0["contact"], taumax, PERIOD, zmin, 0.8); samples = []
    for k, r in enumerate(per):
        if k % EVERY == 0:
            ref.mpc(k, r["mpc_status"])
        ref.tick(k, r); samples.append(ref.sample(k, r))
    tr, count = e.sim.episode_trace(8); assert count == 5 and tr.shape == (3, B)
    for i in range(3):
        assert tr[i].tobytes() == samples[5 * i].tobytes(), i
    got = e.sim.episode_summary()
    assert [int(t) for t in got["fall_tick"]] == [kf if b == bf else -1 for b in range(B)] and got["fall_cause"][bf] == api.FALL_HEIGHT
    assert (got["ticks"] == NT).all() and (got["joint_work"] > 0).all()
    er.compare_summary(got, ref.s, "device synchronous loop")
    e.close()


# ---------------------------------------------------------------- (3) pipelined loop
def test_pipelined_loop_with_monitor(blobs):
    """B = 65, 16 ticks: outputs bit-identical with the monitor on and off, samples at the chunk ends equal the off-run's readback, the summary the numpy fold of the trace"""
    B, NT = 65, 16; nc = NT // EVERY; taumax = _taumax(blobs)
    d = Dev(blobs, B); q0, v0 = _start_states(d.c, B); d.reset(q0, v0); rb0 = d.readback(solution=False); ends = []
    for p in range(nc):
        d.loop(EVERY, pipelined=True); ends.append(d.readback())
    d.close()
    e = Dev(blobs, B); e.sim.monitor(-1.0, 10.0, 1, NT); e.reset(q0, v0); e.loop(NT, pipelined=True)
    tr0, count = e.sim.episode_trace(NT); s0 = e.sim.episode_summary(); assert count == NT and (s0["fall_tick"] == -1).all() and (s0["mpc_calls"] == nc).all()
    bf, kf, zmin = er.fall_threshold(tr0["rbd"][:, :, 5], lo=9, hi=14); print("instance %d falls at tick %d: min_base_z = %.17g" % (bf, kf, zmin))
    e.sim.monitor(zmin, 0.8, 1, NT); e.reset(q0, v0); e.loop(NT, pipelined=True); on = e.readback()
    for name in OUTPUTS:
        assert np.array_equal(on[name], ends[-1][name]), name
    tr, count = e.sim.episode_trace(NT); assert count == NT and tr.tobytes() == tr0.tobytes()
    for p, r in enumerate(ends):      # the status a sample carries is the last call FOLDED in front of it: call p - 1 for chunk p >= 1
        k = (p + 1) * EVERY - 1; f = er.Fold(B, rb0["rbd"][:, 48:55], None, taumax, PERIOD, zmin, 0.8); f.last_status[:] = ends[max(p - 1, 0)]["mpc_status"]
        assert tr[k].tobytes() == f.sample(k, r).tobytes(), k
    status = [tr[0]["mpc_status"]] + [tr[EVERY * (p + 1)]["mpc_status"] for p in range(1, nc - 1)] + [on["mpc_status"]]
    ref = er.Fold(B, rb0["rbd"][:, 48:55], rb0["contact"], taumax, PERIOD, zmin, 0.8)
    for p in range(nc):
        if p == 0:
            ref.mpc(0, status[0])
        for k in range(p * EVERY, (p + 1) * EVERY):
            s = tr[k]; f = np.zeros((B, 4, 3)); f[:, :, 2] = s["force_z"]; cm = s["contact_mask"]; ct = np.stack([(cm >> 3) & 1, (cm >> 2) & 1, (cm >> 1) & 1, cm & 1], axis=1)
            ref.tick(k, dict(time=s["time"], rbd=s["rbd"], contact=ct, force=f.reshape(B, 12), mode=s["mode"], wbc_out=np.zeros((B, 54)), qp_status=s["qp_status"], sim_status=s["sim_status"]))
        if p >= 1:
            ref.mpc(p * EVERY, status[p])
    got = e.sim.episode_summary()
    assert [int(t) for t in got["fall_tick"]] == [kf if b == bf else -1 for b in range(B)] and (got["mpc_calls"] == nc).all() and (got["ticks"] == NT).all()
    skip = {"max_tau_ratio", "joint_work", "tau_over_ticks", "max_friction_ratio"}      # the trace carries neither the WBC output nor the tangential forces: compared on the synchronous loop
    for name in er.INTS + er.EXACT:
        if name not in skip:
            assert np.array_equal(got[name], ref.s[name]), (name, got[name], ref.s[name])
    for name in er.COMPUTED:
        if name not in skip:
            assert np.allclose(got[name], ref.s[name], rtol=er.RTOL, atol=0.0), (name, got[name], ref.s[name])
    e.close()


# ---------------------------------------------------------------- (4) on / off under the feedback policy
def test_monitor_changes_no_bit_under_the_feedback_policy(blobs):
    B, NT = 4, 16; c = _setup(B); q0, v0 = _start_states(c, B); res = {}
    for on in (False, True):
        d = Dev(blobs, B, c, feedback_policy=True)
        if on:
            d.sim.monitor(0.2, 0.8, 1, NT)
        d.reset(q0, v0); d.loop(NT); res[on] = d.readback()
        if on:
            s = d.sim.episode_summary(); assert (s["ticks"] == NT).all() and (s["mpc_calls"] == NT // EVERY).all() and (s["fall_tick"] == -1).all()
        d.close()
    for name in OUTPUTS + ("rbd", "force", "contact", "mode"):
        assert np.array_equal(res[True][name], res[False][name]), name


def test_wbc_only_context_refuses_the_monitor(blobs):
    itf = api.QMInterface(blobs=blobs, max_batch=2, max_nodes=8, max_ref_knots=2, max_events=2); w = itf.wbc_context(2); p = api._EpisodeParams(0.2, 0.8, 0, 0); out = np.zeros(2, api.EPISODE_SUMMARY)
    import ctypes as C
    assert itf.lib.qmhip_episode_monitor(w.h, C.byref(p)) == -5 and itf.lib.qmhip_episode_monitor(w.h, None) == -5 and itf.lib.qmhip_episode_summary(w.h, 2, out.ctypes.data_as(C.c_void_p)) == -5
    assert itf.lib.qmhip_episode_monitor(itf.h, C.byref(p)) == 0 and itf.lib.qmhip_episode_monitor(itf.h, None) == 0
    w.close(); itf.close()
