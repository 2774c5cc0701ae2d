"""Episode monitor (qmhip_episode_*: csrc/host/qm_episode_pipeline.h, csrc/kernels/k_episode.h) on the host emulator.

(1) the fold on synthetic ticks through the fold path against the numpy fold (tests/episode_ref.py): thresholds hit exactly, every fall cause, NaN, a fall on tick 0, MPC
    status words, f_z = 0, torque ratio exactly 1, a trace that overflows;
(2) the synchronous device loop with the monitor on in ONE call against the same loop with the monitor off, read back tick by tick: same outputs, every sample a raw copy
    of the readback, the summary the numpy fold of the readback;  (3) the pipelined loop;  (4) monitor off: the loops launch what they launch without the feature;
(5) error codes and record layout."""
import numpy as np
import pytest

import episode_ref as er
from qm_control_amd import api, layout as L
from test_emu_tick import _setup, _start_states
from test_sim import robust_grid_settings

PERIOD, NSUB, HORIZON, NMAX, EVERY, NT, B5, T_START = 0.001, 2, 0.45, 64, 8, 24, 5, 20.2
OK, ERR_ARG, ERR_STATE = 0, -1, -5


@pytest.fixture(scope="module")
def lib():
    return er.emu_lib()


def _ctx(lib, blobs, B):
    mb, st = blobs; c = _setup("trot", B, T_START); e = er.EmuEpisode(lib, mb, robust_grid_settings(st), B, c["ev"].shape[1], NMAX); e.upload(c, B)
    return e, c


# ---------------------------------------------------------------- (1) fold on synthetic ticks
@pytest.mark.parametrize("patterns", [(0, 1, 2), (3, 4, 5)])
def test_fold_on_synthetic_ticks_matches_the_numpy_fold(lib, blobs, patterns):
    mb, st = blobs; taumax = np.asarray(mb[L.MB_TAUMAX:L.MB_TAUMAX + 18], float); B = len(patterns)
    ticks, anchor = er.synthetic_ticks(patterns, taumax); ref, samples = er.fold_synthetic(ticks, anchor, taumax); er.check_synthetic_expectations(ref, patterns)
    e, _ = _ctx(lib, blobs, B)
    assert e.monitor(er.ZMIN, er.TILT, 5, 2) == OK and e.set_anchor(anchor) == OK
    for k, d in enumerate(ticks):
        assert e.fold(k, d) == OK, lib.emu_episode_why(e.h)
    rc, got = e.summary(); assert rc == OK
    er.compare_summary(got, ref.s, "synthetic %s" % (patterns,))
    # trace_every 5, trace_cap 2 over 12 ticks: ticks 0, 5, 10 are sampled, two fit; what lies behind them in the caller's array stays as it was
    rc, tr, count = e.trace(4, fill=0xAB); assert rc == OK and count == 3
    assert tr[0].tobytes() == samples[0].tobytes() and tr[1].tobytes() == samples[5].tobytes()
    assert (tr[2:].view(np.uint8) == 0xAB).all()
    rc, tr1, count = e.trace(1, fill=0xAB); assert rc == OK and count == 3 and tr1[0].tobytes() == samples[0].tobytes()
    rc, _, count = e.trace(0); assert rc == OK and count == 3
    # a second episode on the same context starts from cleared records
    assert e.monitor(er.ZMIN, er.TILT, 0, 0) == OK and e.set_anchor(anchor) == OK and e.fold(0, ticks[0]) == OK
    rc, got2 = e.summary(); assert rc == OK and (got2["ticks"] == 1).all() and e.trace(4)[2] == 0
    e.close()


# ---------------------------------------------------------------- (2), (3) the loops
@pytest.fixture(scope="module")
def off_run(lib, blobs):
    """the synchronous loop with the monitor off, 24 calls of one tick, everything read back after every tick (computed once, shared)"""
    e, c = _ctx(lib, blobs, B5); q0, v0 = _start_states(c, B5); e.reset(q0, v0, T_START); rb0 = e.readback(); per = []
    for k in range(NT):
        e.closed_loop(1, PERIOD, HORIZON, NSUB, EVERY); per.append(e.readback())
    e.close()
    for d in per:
        for a in d.values():
            a.setflags(write=False)
    return dict(c=c, q0=q0, v0=v0, reset=rb0, per=per)


def test_synchronous_loop_one_call_with_monitor_equals_per_tick_readback(lib, blobs, off_run):
    per = off_run["per"]; mb, _ = blobs; taumax = np.asarray(mb[L.MB_TAUMAX:L.MB_TAUMAX + 18], float)
    z = np.array([d["rbd"][:, 5] for d in per]); bf, kf, zmin = er.fall_threshold(z); print("instance %d falls at tick %d: min_base_z = %.17g" % (bf, kf, zmin))
    e, c = _ctx(lib, blobs, B5); assert e.monitor(zmin, 0.8, 1, NT) == OK
    e.reset(off_run["q0"], off_run["v0"], T_START); e.closed_loop(NT, PERIOD, HORIZON, NSUB, EVERY); on = e.readback()
    for name in ("q", "v", "wbc_out", "xs", "us", "mpc_status", "qp_status", "time"):
        assert np.array_equal(on[name], per[-1][name]), name
    # reference: the numpy fold of the off-run's readback, anchored at the reset state's end-effector pose, previous contact flags the reset state's
    ref = er.Fold(B5, off_run["reset"]["rbd"][:, 48:55], off_run["reset"]["contact"], taumax, PERIOD, zmin, 0.8); samples = []
    for k, d in enumerate(per):
        if k % EVERY == 0:
            ref.mpc(k, d["mpc_status"])
        ref.tick(k, d); samples.append(ref.sample(k, d))
    rc, tr, count = e.trace(NT); assert rc == OK and count == NT
    for k in range(NT):
        assert tr[k].tobytes() == samples[k].tobytes(), k
    rc, got = e.summary(); assert rc == OK
    assert [int(t) for t in got["fall_tick"]] == [kf if b == bf else -1 for b in range(B5)] and got["fall_cause"][bf] == api.FALL_HEIGHT      # it is the only one
    assert (got["ticks"] == NT).all() and (got["mpc_calls"] == [3 - int(b == bf and kf < 16) for b in range(B5)]).all() and (got["joint_work"] > 0).all() and (got["max_ee_pos_dev"] > 0).all()
    er.compare_summary(got, ref.s, "synchronous loop")
    e.close()


def test_pipelined_loop_with_monitor(lib, blobs, off_run):
    mb, _ = blobs; taumax = np.asarray(mb[L.MB_TAUMAX:L.MB_TAUMAX + 18], float); q0, v0 = off_run["q0"], off_run["v0"]
    # monitor off, in chunks of mpc_every: the readback at the chunk ends
    e, c = _ctx(lib, blobs, B5); e.reset(q0, v0, T_START); rb0 = e.readback(); ends = []
    for p in range(NT // EVERY):
        e.closed_loop(EVERY, PERIOD, HORIZON, NSUB, EVERY, pipelined=True); ends.append(e.readback())
    e.close()
    # monitor on, thresholds nobody trips: its trace (raw copies) gives the heights behind every tick the fall threshold is taken from
    e, c = _ctx(lib, blobs, B5); assert e.monitor(-1.0, 10.0, 1, NT) == OK; e.reset(q0, v0, T_START); e.closed_loop(NT, PERIOD, HORIZON, NSUB, EVERY, pipelined=True)
    rc, tr0, count = e.trace(NT); assert rc == OK and count == NT; rc, s0 = e.summary(); assert (s0["fall_tick"] == -1).all() and (s0["mpc_calls"] == 3).all()
    bf, kf, zmin = er.fall_threshold(tr0["rbd"][:, :, 5], lo=9, hi=14); print("instance %d falls at tick %d: min_base_z = %.17g" % (bf, kf, zmin))
    assert e.monitor(zmin, 0.8, 1, NT) == OK; e.reset(q0, v0, T_START); e.closed_loop(NT, PERIOD, HORIZON, NSUB, EVERY, pipelined=True); on = e.readback()
    for name in ("q", "v", "wbc_out", "xs", "us", "mpc_status", "qp_status", "time"):
        assert np.array_equal(on[name], ends[-1][name]), name
    rc, tr, count = e.trace(NT); assert rc == OK and count == NT and tr.tobytes() == tr0.tobytes()      # the trace does not depend on the thresholds
    # samples at the chunk ends against the off-run; the status they carry is the last call FOLDED in front of them: call p - 1 for chunk p >= 1 (folded behind its publication)
    for p, d in enumerate(ends):
        k = (p + 1) * EVERY - 1; f = er.Fold(B5, rb0["rbd"][:, 48:55], None, taumax, PERIOD, zmin, 0.8); f.last_status[:] = ends[max(p - 1, 0)]["mpc_status"]
        assert tr[k].tobytes() == f.sample(k, d).tobytes(), k
    # the summary is the numpy fold of the run's own trace, in the order the loop folds: call 0 in front of its ticks, call p >= 1 behind the ticks of chunk p
    # call 0 is folded in front of its ticks, call p >= 1 behind the ticks of chunk p: its status word shows in the samples of chunk p + 1, the last call's in the final readback
    nc = NT // EVERY; status = [tr[0]["mpc_status"]] + [tr[EVERY * (p + 1)]["mpc_status"] for p in range(1, nc - 1)] + [on["mpc_status"]]
    ref = er.Fold(B5, rb0["rbd"][:, 48:55], rb0["contact"], taumax, PERIOD, zmin, 0.8)
    rc, got = e.summary(); assert rc == OK
    assert [int(t) for t in got["fall_tick"]] == [kf if b == bf else -1 for b in range(B5)]
    assert (got["mpc_calls"] == [2 if b == bf else 3 for b in range(B5)]).all()
    # the summary against the numpy fold of the run's own trace (raw copies, pinned by the synchronous loop's test and by the chunk ends above), in the order the loop folds.
    # The trace carries neither the WBC output nor the tangential forces: the four fields that need them are compared on the synchronous loop, not here
    for p in range(NT // EVERY):
        if p == 0:
            ref.mpc(0, status[0])
        for k in range(p * EVERY, (p + 1) * EVERY):
            s = tr[k]; f = np.zeros((B5, 4, 3)); f[:, :, 2] = s["force_z"]
            cm = s["contact_mask"]; ct = np.stack([(cm >> 3) & 1, (cm >> 2) & 1, (cm >> 1) & 1, cm & 1], axis=1)
            ref.tick(k, dict(time=s["time"], rbd=s["rbd"], contact=ct, force=f.reshape(B5, 12), mode=s["mode"], wbc_out=np.zeros((B5, 54)), qp_status=s["qp_status"], sim_status=s["sim_status"]))
        if p >= 1:
            ref.mpc(p * EVERY, status[p])
    skip = {"max_tau_ratio", "joint_work", "tau_over_ticks", "max_friction_ratio"}
    for name in er.INTS + er.EXACT:
        if name not in skip:
            assert np.array_equal(got[name], ref.s[name]), (name, got[name], ref.s[name])
    for name in er.COMPUTED:
        if name not in skip:
            assert np.allclose(got[name], ref.s[name], rtol=er.RTOL, atol=0.0), (name, got[name], ref.s[name])
    e.close()


# ---------------------------------------------------------------- (4) monitor off
@pytest.mark.parametrize("pipelined", [False, True])
def test_monitor_off_launches_what_the_loop_launches_without_the_feature(lib, blobs, pipelined):
    counts = {}
    for kind in ("plain", "off", "on"):
        e, c = _ctx(lib, blobs, 2); q0, v0 = _start_states(c, 2)
        if kind == "on":
            assert e.monitor(0.2, 0.8, 0, 0) == OK
        e.reset(q0, v0, T_START); n0 = e.launches(); e.closed_loop(8, PERIOD, HORIZON, NSUB, 4, pipelined=pipelined, plain=(kind == "plain")); counts[kind] = e.launches() - n0; e.close()
    print(counts)
    assert counts["off"] == counts["plain"] and counts["on"] == counts["plain"] + 8 + 2      # one launch per tick, one per MPC call


# ---------------------------------------------------------------- (5) errors and layout
def test_error_codes(lib, blobs):
    mb, _ = blobs; taumax = np.asarray(mb[L.MB_TAUMAX:L.MB_TAUMAX + 18], float); ticks, anchor = er.synthetic_ticks((0, 1, 2), taumax); d = ticks[1]
    e, _ = _ctx(lib, blobs, 3)
    # monitor off
    assert e.set_anchor(anchor) == ERR_STATE and e.summary()[0] == ERR_STATE and e.trace(2)[0] == ERR_STATE and e.fold(0, d) == ERR_STATE
    for bad in ((np.nan, 0.8, 0, 0), (0.2, np.inf, 0, 0), (0.2, 0.8, -1, 0), (0.2, 0.8, 0, -1), (0.2, 0.8, 0, 4), (0.2, 0.8, 4, 0), (0.2, 0.8, -1, -1)):
        assert e.monitor(*bad) == ERR_ARG, bad
    assert e.summary()[0] == ERR_STATE      # a refused switch-on leaves it off
    assert e.monitor(0.2, 0.8, 2, 4) == OK
    assert e.summary()[0] == ERR_STATE and e.trace(2)[0] == ERR_STATE      # no episode yet
    assert e.fold(0, d) == ERR_STATE                                        # the first fold needs the anchor
    assert e.set_anchor(None) == ERR_ARG and e.set_anchor(anchor, B=0) == ERR_ARG and e.set_anchor(anchor, B=4) == ERR_ARG and e.set_anchor(anchor) == OK
    for name in ("time", "rbd", "contact", "force", "mode", "wbc_out", "qp_status"):
        dd = dict(d); dd[name] = None; assert e.fold(0, dd) == ERR_ARG, name
    assert e.fold(-1, d) == ERR_ARG and e.fold(0, d, B=0) == ERR_ARG and e.fold(0, d, B=4) == ERR_ARG
    dd = dict(d); dd["sim_status"] = None; dd["mpc_status"] = None; assert e.fold(0, dd) == OK
    d2 = {k: (None if v is None else v[:2]) for k, v in d.items()}; assert e.fold(1, d2, B=2) == ERR_ARG      # another batch than the running episode's
    assert e.summary(B=2)[0] == ERR_STATE and e.summary(B=0)[0] == ERR_ARG and e.summary(B=4)[0] == ERR_ARG and e.summary()[0] == OK
    assert e.lib.emu_episode_summary(e.h, 3, None) == ERR_ARG
    assert e.trace(2, B=2)[0] == ERR_STATE and e.trace(-1)[0] == ERR_ARG and e.lib.emu_episode_trace(e.h, 3, 2, None, None) == ERR_ARG and e.trace(2)[0] == OK
    assert e.monitor(on=False) == OK and e.summary()[0] == ERR_STATE and e.monitor(on=False) == OK
    e.close()


def test_record_layout_matches_header_and_python(lib):
    assert lib.emu_episode_bytes(0) == 256 == L.QM_EP_BYTES == api.EPISODE_SUMMARY.itemsize == 8 * L.QM_EP_WORDS
    assert lib.emu_episode_bytes(1) == 512 == L.QM_ES_BYTES == api.EPISODE_SAMPLE.itemsize == 8 * L.QM_ES_WORDS
    for fields, dt, off in ((L.EPISODE_SUMMARY_FIELDS, api.EPISODE_SUMMARY, lib.emu_episode_summary_offset), (L.EPISODE_SAMPLE_FIELDS, api.EPISODE_SAMPLE, lib.emu_episode_sample_offset)):
        assert off(len(fields)) == -1
        for k, f in enumerate(fields):
            assert off(k) == dt.fields[f[0]][1] == f[3], f[0]
    assert er.INTS + er.EXACT + er.COMPUTED and sorted(er.INTS + er.EXACT + er.COMPUTED) == sorted(f[0] for f in L.EPISODE_SUMMARY_FIELDS)
    assert (L.QM_FALL_HEIGHT, L.QM_FALL_ROLL, L.QM_FALL_PITCH, L.QM_FALL_NONFINITE) == (1, 2, 4, 8)
    assert api.EPISODE_SUMMARY["touchdowns"].shape == (4,) and api.EPISODE_SAMPLE["rbd"].shape == (55,) and api.EPISODE_SAMPLE["qp_status"].shape == (3,)
