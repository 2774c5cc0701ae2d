"""tests/episode_ref.py — TEST INFRASTRUCTURE of the episode monitor's tests (test_episode_monitor.py on the host emulator, test_gpu_episode_monitor.py on the device):

  * `Fold`: the monitor's fold restated in plain numpy, per instance and per tick, from include/qmhip.h's description — the reference of every summary comparison.  It is
    fed with per-tick data read back through entry points that exist without the monitor (or with synthetic ticks), never with the monitor's own summary;
  * `synthetic_ticks`: the synthetic tick sequences of the fold tests (thresholds hit exactly, every fall cause, NaN, MPC status words, f_z = 0, torque ratio 1);
  * `compare_summary`: integer / copied fields array_equal, computed fields rtol 1e-12 (<= ~20 FP64 operations on non-negative terms per tick, one rounding per tick in the
    sums over <= 24 ticks, a few ulp from FMA contraction and asin: 1e-12 is more than a hundred times that);
  * `EmuEpisode`: ctypes binding of tests/emu_episode."""
import ctypes as C
import os
import subprocess

import numpy as np

from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
EXACT = ["t_first", "t_last", "t_fall", "min_base_z", "max_abs_roll", "max_abs_pitch", "max_normal_force", "spare"]
COMPUTED = ["max_base_speed", "max_ee_pos_dev", "sum_sq_ee_pos_dev", "max_ee_ang_dev", "max_tau_ratio", "max_friction_ratio", "joint_work"]
INTS = ["ticks", "fall_tick", "fall_cause", "sim_bad_ticks", "mpc_calls", "mpc_fail_calls", "mpc_warn_or", "mpc_last_fail", "mpc_first_fail_tick", "reserved", "wbc_bad_ticks", "airborne_ticks",
        "contact_mismatch_ticks", "touchdowns", "tau_over_ticks", "ispare"]
RTOL = 1e-12


def contact_mask(flags):
    """[.., 4] flags LF RF LH RH -> 8 LF + 4 RF + 2 LH + RH"""
    f = (np.asarray(flags) != 0).astype(np.int64)
    return 8 * f[..., 0] + 4 * f[..., 1] + 2 * f[..., 2] + f[..., 3]


class Fold:
    """numpy restatement of the fold.  anchor [B][7]; prev_contact [B][4] flags before the first tick, or None: the first tick's own"""

    def __init__(self, B, anchor, prev_contact, taumax, period, min_base_z, max_tilt):
        self.B = B; self.anchor = np.asarray(anchor, float); self.taumax = np.asarray(taumax, float); self.period = period; self.zmin = min_base_z; self.tilt = max_tilt
        self.prev = None if prev_contact is None else [int(m) for m in contact_mask(prev_contact)]
        z = lambda n=None: np.zeros(B if n is None else (B, n)); zi = lambda n=None: np.zeros(B if n is None else (B, n), np.int32)
        self.s = dict(t_first=z(), t_last=z(), t_fall=z(), min_base_z=np.full(B, np.inf), max_abs_roll=z(), max_abs_pitch=z(), max_base_speed=z(), max_ee_pos_dev=z(), sum_sq_ee_pos_dev=z(),
                      max_ee_ang_dev=z(), max_tau_ratio=z(), max_friction_ratio=z(), max_normal_force=z(), joint_work=z(), spare=z(2),
                      ticks=zi(), fall_tick=zi() - 1, fall_cause=zi(), sim_bad_ticks=zi(), mpc_calls=zi(), mpc_fail_calls=zi(), mpc_warn_or=zi(), mpc_last_fail=zi(), mpc_first_fail_tick=zi() - 1,
                      reserved=zi(), wbc_bad_ticks=zi(3), airborne_ticks=zi(), contact_mismatch_ticks=zi(4), touchdowns=zi(4), tau_over_ticks=zi(), ispare=zi(9))
        self.last_status = np.zeros(B, np.int32)

    def mpc(self, t_obs, status):
        """one MPC call that observed at tick t_obs, folded now"""
        s = self.s
        for b in range(self.B):
            st = int(status[b]); self.last_status[b] = st
            if s["fall_tick"][b] != -1 and s["fall_tick"][b] < t_obs:
                continue
            s["mpc_calls"][b] += 1
            if st < 0:
                s["mpc_fail_calls"][b] += 1; s["mpc_last_fail"][b] = st
                if s["mpc_first_fail_tick"][b] == -1:
                    s["mpc_first_fail_tick"][b] = t_obs
            elif st > 0:
                s["mpc_warn_or"][b] |= st

    def tick(self, k, d):
        """d: time [B], rbd [B][55], contact [B][4], force [B][12], mode [B], wbc_out [B][54], qp_status [B][3], sim_status [B] or None"""
        s = self.s
        if self.prev is None:
            self.prev = [int(m) for m in contact_mask(d["contact"])]
        for b in range(self.B):
            r = d["rbd"][b]; t = d["time"][b]
            if s["ticks"][b] == 0:
                s["t_first"][b] = t
            s["ticks"][b] += 1; s["t_last"][b] = t
            if s["fall_tick"][b] != -1:
                continue
            cause = (1 if r[5] < self.zmin else 0) | (2 if abs(r[2]) > self.tilt else 0) | (4 if abs(r[1]) > self.tilt else 0) | (0 if np.isfinite(r).all() else 8)
            if cause:
                s["fall_tick"][b] = k; s["fall_cause"][b] = cause; s["t_fall"][b] = t
                continue
            s["min_base_z"][b] = min(s["min_base_z"][b], r[5]); s["max_abs_roll"][b] = max(s["max_abs_roll"][b], abs(r[2])); s["max_abs_pitch"][b] = max(s["max_abs_pitch"][b], abs(r[1]))
            s["max_base_speed"][b] = max(s["max_base_speed"][b], np.sqrt(r[27] ** 2 + r[28] ** 2 + r[29] ** 2))
            dev = r[48:51] - self.anchor[b, :3]; d2 = float(dev @ dev)
            s["max_ee_pos_dev"][b] = max(s["max_ee_pos_dev"][b], np.sqrt(d2)); s["sum_sq_ee_pos_dev"][b] += d2
            q = r[51:55]; qa = self.anchor[b, 3:]; dq = min(np.linalg.norm(q - qa), np.linalg.norm(q + qa))
            s["max_ee_ang_dev"][b] = max(s["max_ee_ang_dev"][b], 4.0 * np.arcsin(dq / 2.0))
            tau = d["wbc_out"][b, 36:54]; ratio = float((np.abs(tau) / self.taumax).max())
            s["max_tau_ratio"][b] = max(s["max_tau_ratio"][b], ratio); s["tau_over_ticks"][b] += int(ratio > 1.0)
            s["joint_work"][b] += self.period * float(np.abs(tau * r[30:48]).sum())
            f = d["force"][b].reshape(4, 3)
            for i in range(4):
                if f[i, 2] > 0.0:
                    s["max_friction_ratio"][b] = max(s["max_friction_ratio"][b], np.sqrt(f[i, 0] ** 2 + f[i, 1] ** 2) / f[i, 2])
                s["max_normal_force"][b] = max(s["max_normal_force"][b], f[i, 2])
            m = int(contact_mask(d["contact"][b])); mode = int(d["mode"][b])
            for i in range(4):
                bit = 8 >> i
                s["contact_mismatch_ticks"][b, i] += int(bool(m & bit) != bool(mode & bit)); s["touchdowns"][b, i] += int(bool(m & bit) and not (self.prev[b] & bit))
            self.prev[b] = m; s["airborne_ticks"][b] += int(m == 0)
            s["wbc_bad_ticks"][b] += (np.asarray(d["qp_status"][b]) != 0).astype(np.int32)
            if d.get("sim_status") is not None:
                s["sim_bad_ticks"][b] += int(d["sim_status"][b] != 0)

    def sample(self, k, d):
        """the raw sample of tick k as the trace holds it (the status of the last call folded so far)"""
        out = np.zeros(self.B, api.EPISODE_SAMPLE); out["time"] = d["time"]; out["rbd"] = d["rbd"]; out["force_z"] = np.asarray(d["force"]).reshape(self.B, 4, 3)[:, :, 2]
        out["tick"] = k; out["mode"] = d["mode"]; out["contact_mask"] = contact_mask(d["contact"]); out["mpc_status"] = self.last_status; out["qp_status"] = d["qp_status"]
        out["sim_status"] = 0 if d.get("sim_status") is None else d["sim_status"]
        return out


def compare_summary(got, ref, label=""):
    """got: structured array of dtype api.EPISODE_SUMMARY; ref: Fold.s.  Prints every computed field's worst relative deviation before it asserts"""
    for name in INTS + EXACT:
        assert np.array_equal(got[name], ref[name]), (label, name, got[name], ref[name])
    for name in COMPUTED:
        g = np.asarray(got[name], float); r = np.asarray(ref[name], float); assert np.isfinite(g).all() and np.isfinite(r).all(), (label, name, g, r)
        err = float((np.abs(g - r) / np.maximum(np.abs(r), 1e-300)).max()) if (r != 0).any() or (g != 0).any() else 0.0
        print("%s %-20s max rel dev %.3e" % (label, name, err))
        assert np.allclose(g, r, rtol=RTOL, atol=0.0), (label, name, g, r)


def fall_threshold(z, lo=6, hi=14):
    """z [ticks][B] base heights behind every tick of a run without a fall: (instance, tick k, midpoint of z[k - 1] and z[k]) such that exactly that instance drops below
    the midpoint, first at tick k; the pair of consecutive ticks nearest to tick 10 that has the property"""
    for k in sorted(range(lo, hi + 1), key=lambda k: abs(k - 10)):
        for b in range(z.shape[1]):
            mid = 0.5 * (z[k - 1, b] + z[k, b])
            if z[k, b] < mid < z[k - 1, b] and (z[:k, b] >= mid).all() and all((z[:, o] >= mid).all() for o in range(z.shape[1]) if o != b):
                return b, k, mid
    raise AssertionError("no instance / tick pair isolates one fall")


# ---------------------------------------------------------------- synthetic ticks
ZMIN, TILT, PERIOD, NT = 0.2, 0.8, 0.002, 12
PATTERNS = 6


def synthetic_ticks(patterns, taumax, seed=5):
    """NT ticks for len(patterns) instances; instance b follows pattern patterns[b]:
      0  touches min_base_z exactly (tick 3) and +max_tilt / -max_tilt exactly (tick 4) without falling; NaN in rbd at tick 7 (cause 8), garbage afterwards
      1  falls on tick 0 with two causes at once (height and pitch: 5)
      2  never falls: torque ratio exactly 1 at tick 6, above 1 at tick 9; a stance foot with f_z = 0; an airborne tick; warnings 1 and 2 from the MPC
      3  height alone at tick 5;  4  roll alone at tick 2;  5  pitch alone at tick 9, after two failed MPC calls (first failing tick 4, last failure -4)
    MPC calls on ticks 0, 4, 8 (None otherwise).  Returns (ticks, anchor [B][7])"""
    rng = np.random.default_rng(seed); B = len(patterns); pat = np.asarray(patterns)
    qa = rng.normal(size=(B, 4)); qa /= np.linalg.norm(qa, axis=1)[:, None]; anchor = np.concatenate([rng.normal(size=(B, 3)), qa], axis=1)
    mpc_status = {0: {p: 0 for p in range(6)}, 4: {0: -4, 1: -4, 2: 1, 3: 0, 4: 2, 5: -3}, 8: {0: 1, 1: 0, 2: 2, 3: -4, 4: -4, 5: -4}}
    ticks = []
    for k in range(NT):
        rbd = rng.normal(size=(B, 55)) * 0.3; rbd[:, 5] = 0.4 + 0.05 * rng.random(B); rbd[:, 1:3] = rng.uniform(-0.5, 0.5, (B, 2))
        rbd[:, 48:51] = anchor[:, :3] + 0.01 * rng.normal(size=(B, 3))
        q = anchor[:, 3:] + 0.02 * rng.normal(size=(B, 4)); q /= np.linalg.norm(q, axis=1)[:, None]; rbd[:, 51:55] = q * np.where(rng.random(B) < 0.5, -1.0, 1.0)[:, None]      # either sign of the quaternion
        contact = (rng.random((B, 4)) < 0.7).astype(np.int32) * (1 + k)      # any non-zero flag counts
        force = rng.normal(size=(B, 4, 3)) * 20.0; force[:, :, 2] = np.where(contact != 0, 80.0 + 40.0 * rng.random((B, 4)), 0.0)
        mode = rng.choice([15, 9, 6, 0], size=B).astype(np.int32)
        out = rng.normal(size=(B, 54)); out[:, 36:] = 0.6 * taumax * rng.uniform(-1, 1, (B, 18))
        qps = (rng.random((B, 3)) < 0.2).astype(np.int32) * rng.integers(1, 4, (B, 3)).astype(np.int32); sst = (rng.random(B) < 0.2).astype(np.int32)
        for b in range(B):
            p = pat[b]
            if p == 0:
                if k == 3: rbd[b, 5] = ZMIN
                if k == 4: rbd[b, 2] = TILT; rbd[b, 1] = -TILT
                if k == 7: rbd[b, 20] = np.nan
                if k > 7: rbd[b, 27:30] = 1e30; out[b, 36:] = 1e30; rbd[b, 40] = np.inf      # must not reach an accumulator
            if p == 1 and k == 0: rbd[b, 5] = 0.1; rbd[b, 1] = 0.9
            if p == 2:
                if k == 6: out[b, 36:] *= 0.5; out[b, 39] = -taumax[3]
                if k == 9: out[b, 44] = 1.5 * taumax[8]
                if k == 5: contact[b, 1] = 1; force[b, 1, 2] = 0.0
                if k == 2: contact[b] = 0; force[b, :, 2] = 0.0
            if p == 3 and k == 5: rbd[b, 5] = np.nextafter(ZMIN, 0.0)
            if p == 4 and k == 2: rbd[b, 2] = -np.nextafter(TILT, 1.0)
            if p == 5 and k == 9: rbd[b, 1] = 0.81
        st = None if k not in mpc_status else np.array([mpc_status[k][p] for p in pat], np.int32)
        ticks.append(dict(time=20.0 + PERIOD * (k + 1) + 1e-3 * np.arange(B), rbd=rbd, contact=contact, force=force.reshape(B, 12), mode=mode, wbc_out=out, qp_status=qps, sim_status=sst, mpc_status=st))
    return ticks, anchor


def fold_synthetic(ticks, anchor, taumax):
    """the numpy fold of synthetic_ticks in the order qmhip_episode_fold folds (the MPC call of a tick in front of the tick) and the samples of every tick"""
    B = anchor.shape[0]; f = Fold(B, anchor, None, taumax, PERIOD, ZMIN, TILT); samples = []
    for k, d in enumerate(ticks):
        if d["mpc_status"] is not None:
            f.mpc(k, d["mpc_status"])
        f.tick(k, d); samples.append(f.sample(k, d))
    return f, samples


def check_synthetic_expectations(ref, patterns):
    """what the synthetic sequences are built to produce, asserted on the REFERENCE (so the reference itself is checked against the issue's words)"""
    s = ref.s
    for b, p in enumerate(patterns):
        exp = {0: (7, 8), 1: (0, 5), 2: (-1, 0), 3: (5, 1), 4: (2, 2), 5: (9, 4)}[p]
        assert (s["fall_tick"][b], s["fall_cause"][b]) == exp, (b, p, s["fall_tick"][b], s["fall_cause"][b])
        assert s["ticks"][b] == NT and all(np.isfinite(s[n][b]).all() for n in COMPUTED + EXACT if n != "min_base_z" or p != 1)
        if p == 0:
            assert s["min_base_z"][b] == ZMIN and s["max_abs_roll"][b] == TILT and s["max_abs_pitch"][b] == TILT and s["max_base_speed"][b] < 10 and s["mpc_calls"][b] == 2 and s["mpc_fail_calls"][b] == 1
        if p == 1:
            assert s["min_base_z"][b] == np.inf and s["mpc_calls"][b] == 1 and s["max_tau_ratio"][b] == 0 and s["t_first"][b] == s["t_fall"][b]
        if p == 2:
            assert s["max_tau_ratio"][b] == 1.5 and s["tau_over_ticks"][b] == 1 and s["mpc_warn_or"][b] == 3 and s["mpc_calls"][b] == 3 and s["airborne_ticks"][b] >= 1
        if p == 5:
            assert s["mpc_calls"][b] == 3 and s["mpc_fail_calls"][b] == 2 and s["mpc_first_fail_tick"][b] == 4 and s["mpc_last_fail"][b] == -4
        if p == 3:
            assert s["mpc_calls"][b] == 2 and s["mpc_fail_calls"][b] == 0


# ---------------------------------------------------------------- host emulator binding
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_episode"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_episode", "_build", "libqm_emu_episode.so"))
    lib.emu_episode_create.restype = C.c_void_p; lib.emu_episode_why.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


class EmuEpisode:
    """one emulator context: solver, WBC, plant and the episode monitor (tests/emu_episode/emu_episode_api.cpp); the method names of api.QMHWSim where they exist"""

    def __init__(self, lib, mb, st, Bmax, nev, nmax=64):
        self.lib = lib; self.mb = np.ascontiguousarray(mb, float); self.st = np.ascontiguousarray(st, float); self.Bmax = Bmax; self.nmax = nmax; self.B = Bmax
        self.h = C.c_void_p(lib.emu_episode_create(_p(self.mb), _p(self.st), Bmax, nmax, 2, nev))

    def close(self):
        if self.h:
            self.lib.emu_episode_destroy(self.h); self.h = None

    def upload(self, c, B):
        a = lambda k, t=float: np.ascontiguousarray(c[k][:B], t)
        self.lib.emu_episode_upload(self.h, B, _p(a("t0")), _p(a("x0")), _p(a("ref_t")), _p(a("ref_x")), _p(a("ev")), _pi(a("modes", np.int32)))

    def reset(self, q, v, time):
        q = np.ascontiguousarray(q, float); self.B = B = q.shape[0]; v = np.ascontiguousarray(v, float); t = np.ascontiguousarray(np.broadcast_to(time, (B,)), float)
        self.lib.emu_episode_sim_reset(self.h, B, _p(q), _p(v), _p(t), 0)

    def closed_loop(self, n, period, horizon, nsub, mpc_every, pipelined=False, plain=False):
        fn = self.lib.emu_episode_closed_loop_plain if plain else self.lib.emu_episode_closed_loop
        fn(self.h, self.B, n, C.c_double(period), nsub, mpc_every, C.c_double(horizon), C.c_double(0.0), C.c_double(0.5), int(pipelined))

    def launches(self):
        return self.lib.emu_episode_launches(self.h)

    def readback(self):
        B = self.B; d = dict(q=np.zeros((B, 24)), v=np.zeros((B, 24)), time=np.zeros(B), rbd=np.zeros((B, 55)), contact=np.zeros((B, 4), np.int32), force=np.zeros((B, 12)), sim_status=np.zeros(B, np.int32),
                             wbc_out=np.zeros((B, 54)), qp_status=np.zeros((B, 3), np.int32), mode=np.zeros(B, np.int32), mpc_status=np.zeros(B, np.int32))
        self.lib.emu_episode_readback(self.h, B, _p(d["q"]), _p(d["v"]), _p(d["time"]), _p(d["rbd"]), _pi(d["contact"]), _p(d["force"]), _pi(d["sim_status"]), _p(d["wbc_out"]), _pi(d["qp_status"]), _pi(d["mode"]), _pi(d["mpc_status"]))
        xs = np.zeros((self.nmax, self.Bmax, 30)); us = np.zeros_like(xs); self.lib.emu_episode_solution(self.h, _p(xs), _p(us)); d["xs"] = xs; d["us"] = us
        return d

    def monitor(self, min_base_z=0.2, max_tilt=0.8, trace_every=0, trace_cap=0, on=True):
        return self.lib.emu_episode_monitor(self.h, int(on), C.c_double(min_base_z), C.c_double(max_tilt), trace_every, trace_cap)

    def set_anchor(self, ee, B=None):
        ee = None if ee is None else np.ascontiguousarray(ee, float)
        return self.lib.emu_episode_set_anchor(self.h, self.B if B is None else B, _p(ee))

    def summary(self, B=None):
        B = self.B if B is None else B; out = np.zeros(max(B, 1), api.EPISODE_SUMMARY); rc = self.lib.emu_episode_summary(self.h, B, out.ctypes.data_as(C.c_void_p))
        return rc, out

    def trace(self, cap, B=None, fill=0):
        B = self.B if B is None else B; out = np.zeros((max(cap, 1), max(B, 1)), api.EPISODE_SAMPLE); out.view(np.uint8)[...] = fill; n = np.zeros(1, np.int32)
        rc = self.lib.emu_episode_trace(self.h, B, cap, out.ctypes.data_as(C.c_void_p), _pi(n))
        return rc, out, int(n[0])

    def fold(self, k, d, B=None, period=PERIOD):
        B = self.B if B is None else B; f = lambda n: None if d.get(n) is None else np.ascontiguousarray(d[n], float)
        return self.lib.emu_episode_fold(self.h, B, k, C.c_double(period), _p(f("time")), _p(f("rbd")), _pi(_i32(d.get("contact"))), _p(f("force")), _pi(_i32(d.get("mode"))), _p(f("wbc_out")),
                                         _pi(_i32(d.get("qp_status"))), _pi(_i32(d.get("sim_status"))), _pi(_i32(d.get("mpc_status"))))
