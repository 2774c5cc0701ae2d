"""tests/sense_ref.py — TEST INFRASTRUCTURE of the sensor model between the plant and the controller (qmhip_sim_set_sensors; include/qmhip.h "sensor model").

The numpy reference of the header's semantics: the integer generator (mix / word / nu), the four individually rounded operations of the measured value, the source
sample n − min(lag, n).  numpy rounds every elementwise operation on its own, which is what the kernel is held to.

EmuPlant / DevPlant: the same few calls on the host emulator (tests/emu_sense) and on the device (api.QMHWSim), so that tests/test_sense.py and tests/test_gpu_sense.py run
the SAME checks (check_* below) with the same shapes and the same assertions."""
import ctypes as C
import os
import subprocess

import numpy as np

import push_ref as pr
from conftest import rel_err
from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double); _ip = C.POINTER(C.c_int32)
_p = pr._p; _pi = pr._pi
OK, ERR_ARG, ERR_STATE = pr.OK, pr.ERR_ARG, pr.ERR_STATE
MAX_LAG, SLOTS, NG, NC = L.QM_SENSE_MAX_LAG, L.QM_SENSE_MAX_LAG + 1, L.QM_SENSE_GROUPS, 48
GROUP = np.array([0] * 3 + [1] * 3 + [2] * 18 + [3] * 3 + [4] * 3 + [5] * 18)      # group of component c = rbd index
U = np.uint64
G = U(0x9E3779B97F4A7C15)
CNU = float.fromhex("0x1.3988e1412ed76p-17")
NU_MAX = 8 * 65535 * CNU
BIAS_N = U(0xFFFFFFFFFFFFFFFF)
# the levels of the loop tests (the issue's item 5): base zyx [rad], base position [m], joint positions [rad], base angular velocity [rad/s], base linear velocity [m/s],
# joint rates [rad/s]
SIGMA = np.array([2e-3, 2e-3, 1e-3, 2e-2, 2e-2, 5e-2])


# ---------------------------------------------------------------- the generator and the measured value
def mix(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, U); z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9); z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def word(seed, n, c, w):
    with np.errstate(over="ignore"):
        seed = np.asarray(seed, U); n = np.asarray(n, U); k = (2 * np.asarray(c, np.int64) + w + 1).astype(U)
        return mix(mix(seed + G * (n + U(1))) + G * k)


def nu(seed, n, c):
    s = np.zeros(np.broadcast(np.asarray(seed), np.asarray(n), np.asarray(c)).shape, np.int64)
    for w in (0, 1):
        x = word(seed, n, c, w)
        for k in range(4):
            s = s + ((x >> U(16 * k)) & U(0xFFFF)).astype(np.int64)
    return (2 * s - 8 * 65535).astype(np.float64) * CNU


def bias(rec):
    """[48] the constant bias of one record: bias_sigma[g] * nu(seed, 2^64 - 1, c)"""
    return rec["bias_sigma"][GROUP] * nu(rec["seed"], BIAS_N, np.arange(NC))


def corrupt(x, rec, n):
    """[48] measured components of the source truth x[0:48] under one record at sample n: (x + bias_sigma nu_bias) + sigma nu, clean groups copied"""
    c = np.arange(NC); sg = rec["sigma"][GROUP]; bs = rec["bias_sigma"][GROUP]; x = np.asarray(x, float)[:NC]
    pb = bs * nu(rec["seed"], BIAS_N, c); pn = sg * nu(rec["seed"], U(n), c); t = x + pb; m = t + pn
    return np.where((sg != 0.0) | (bs != 0.0), m, x)


def noisy(rec):
    return bool((rec["sigma"] != 0.0).any() or (rec["bias_sigma"] != 0.0).any())


def source(truths, rec, n):
    """the truth the measurement of sample n is made from: sample n − min(lag, n) of truths [n + 1][55]"""
    return truths[n - min(int(rec["lag"]), n)]


def sensors(B):
    """[B] records of dtype api.SENSOR, every one the identity (no noise, no bias, no lag)"""
    return np.zeros(B, api.SENSOR)


def record(s, b, seed, lag=0, sigma=0.0, bias_sigma=0.0):
    s["seed"][b] = seed; s["lag"][b] = lag; s["sigma"][b] = sigma; s["bias_sigma"][b] = bias_sigma


def q_of_rbd(r):
    """plant coordinates [pos, zyx, joints] of an rbd state"""
    return np.concatenate([r[3:6], r[0:3], r[6:24]])


# ---------------------------------------------------------------- the two plants
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_sense"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_sense", "_build", "libqm_emu_sense.so")); lib.emu_sense_create.restype = C.c_void_p
    lib.emu_sense_word.restype = C.c_uint64; lib.emu_sense_word.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    lib.emu_sense_nu.restype = C.c_double; lib.emu_sense_nu.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    return lib


def _rec_arg(s):
    s = np.ascontiguousarray(s, dtype=api.SENSOR); assert s.ndim == 1
    return s.shape[0], s.ctypes.data_as(C.c_void_p), s


class EmuPlant:
    """solver, WBC, plant, sensor model and episode monitor in one emulator context (tests/emu_sense/emu_sense_api.cpp); the method names of api.QMHWSim where they exist"""

    def __init__(self, lib, blobs, Bmax, nev=2, nmax=8):
        self.lib = lib; self.mb = np.ascontiguousarray(blobs[0], float); self.st = np.ascontiguousarray(blobs[1], float); self.Bmax = Bmax; self.B = Bmax
        self.h = C.c_void_p(lib.emu_sense_create(_p(self.mb), _p(self.st), Bmax, nmax, 2, nev))

    def close(self):
        if self.h:
            self.lib.emu_sense_destroy(self.h); self.h = None

    def upload(self, c, B):
        a = lambda k, t=float: np.ascontiguousarray(c[k][:B], t)
        self.lib.emu_sense_upload(self.h, B, _p(a("t0")), _p(a("x0")), _p(a("ref_t")), _p(a("ref_x")), _p(a("ev")), _pi(a("modes", np.int32)))

    def reset(self, q, v, time):
        q = np.ascontiguousarray(q, float); self.B = B = q.shape[0]; v = np.ascontiguousarray(v, float); t = np.ascontiguousarray(np.broadcast_to(time, (B,)), float)
        self.lib.emu_sense_sim_reset(self.h, B, _p(q), _p(v), _p(t))

    def command(self, pos, vel, kp, kd, ff):
        cmd = np.ascontiguousarray(np.concatenate([pr._bcast(x, self.B) for x in (pos, vel, kp, kd, ff)], axis=1)); self.lib.emu_sense_sim_command(self.h, self.B, _p(cmd))

    def state(self):
        B = self.B; d = dict(q=np.zeros((B, 24)), v=np.zeros((B, 24)), time=np.zeros(B), rbd=np.zeros((B, 55)), contact=np.zeros((B, 4), np.int32), force=np.zeros((B, 12)), status=np.zeros(B, np.int32),
                             qp_status=np.zeros((B, 3), np.int32), mpc_status=np.zeros(B, np.int32))
        self.lib.emu_sense_readback(self.h, B, _p(d["q"]), _p(d["v"]), _p(d["time"]), _p(d["rbd"]), _pi(d["contact"]), _p(d["force"]), _pi(d["status"]), _pi(d["qp_status"]), _pi(d["mpc_status"]))
        return d

    def step(self, period, nsub):
        self.lib.emu_sense_sim_step(self.h, self.B, C.c_double(period), nsub)
        return self.state()

    def closed_loop(self, n, period, horizon, nsub, mpc_every, pipelined=False):
        self.lib.emu_sense_closed_loop(self.h, self.B, n, C.c_double(period), nsub, mpc_every, C.c_double(horizon), C.c_double(0.0), C.c_double(0.5), int(pipelined))
        return self.state()

    def set_sensors(self, s):
        if s is None:
            return self.lib.emu_sense_set_sensors(self.h, 0, None)
        B, ptr, _keep = _rec_arg(s)
        return self.lib.emu_sense_set_sensors(self.h, B, ptr)

    def set_sensors_raw(self, B, s):
        return self.lib.emu_sense_set_sensors(self.h, B, s.ctypes.data_as(C.c_void_p))

    def measured(self, B=None):
        B = self.B if B is None else B; r = np.zeros((max(B, 1), 55)); n = np.full(max(B, 1), -1, np.int32)
        return self.lib.emu_sense_get_measured(self.h, B, _p(r), _pi(n)), r, n

    def set_wbc_only(self, on):
        """the context refuses the plant's calls like one of qmhip_create_wbc_context (the product's guard itself runs in tests/test_gpu_sense.py)"""
        self.lib.emu_sense_set_wbc_only(self.h, int(on))

    def launches(self):
        """(qm_sim_kernel, qm_sim_push_kernel, qm_sense_kernel) launches so far"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0); self.lib.emu_sense_counts(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def monitor(self, trace_cap):
        assert self.lib.emu_sense_monitor(self.h, C.c_double(0.2), C.c_double(0.8), 1, trace_cap) == OK

    def episode(self, cap):
        out = np.zeros(self.B, api.EPISODE_SUMMARY); assert self.lib.emu_sense_episode_summary(self.h, self.B, out.ctypes.data_as(C.c_void_p)) == OK
        tr = np.zeros((cap, self.B), api.EPISODE_SAMPLE); n = C.c_int(0); assert self.lib.emu_sense_episode_trace(self.h, self.B, cap, tr.ctypes.data_as(C.c_void_p), C.byref(n)) == OK and n.value == cap
        return out, tr


class DevPlant(pr.DevPlant):
    """the same calls through the C ABI on the device"""

    def set_sensors(self, s):
        if s is None:
            return self.itf.lib.qmhip_sim_set_sensors(self._h(), 0, None)
        B, ptr, _keep = _rec_arg(s)
        return self.itf.lib.qmhip_sim_set_sensors(self._h(), B, ptr)

    def set_sensors_raw(self, B, s):
        return self.itf.lib.qmhip_sim_set_sensors(self._h(), B, s.ctypes.data_as(C.c_void_p))

    def measured(self, B=None):
        B = self.B if B is None else B; r = np.zeros((max(B, 1), 55)); n = np.full(max(B, 1), -1, np.int32)
        return self.itf.lib.qmhip_sim_get_measured(self._h(), B, _p(r), _pi(n)), r, n

    def monitor(self, trace_cap):
        self.sim.monitor(0.2, 0.8, trace_every=1, trace_cap=trace_cap)

    def episode(self, cap):
        tr, n = self.sim.episode_trace(); assert n == cap
        return self.sim.episode_summary(), tr


# ---------------------------------------------------------------- shared cases and checks
STEPS, PERIOD, NSUB, T0 = 12, pr.PERIOD, pr.NSUB, pr.T0


def plant_records():
    """item 2: identity;  noise on all groups, lag 0;  lag 3 only;  noise + bias + the largest lag"""
    s = sensors(4)
    record(s, 1, 11, 0, SIGMA); record(s, 2, 12, 3); record(s, 3, 0xFEDCBA9876543210, MAX_LAG, SIGMA, 0.5 * SIGMA)
    return s


def check_measurement(m, n_dev, truths, s, n, oracle=None, worst=None):
    """one sample of a batch: rbd_meas [B][55] against the reference applied to the recorded truths [n + 1][B][55]; with an oracle, the end-effector pose too"""
    for b in range(len(s)):
        src = source([t[b] for t in truths], s[b], n)
        assert n_dev[b] == n, (b, n, n_dev[b])
        assert np.array_equal(m[b, :NC], corrupt(src, s[b], n)), (b, n, np.abs(m[b, :NC] - corrupt(src, s[b], n)).max())
        if not noisy(s[b]):
            assert np.array_equal(m[b], src), (b, n)      # all 55 entries: delayed truth, bit for bit
        elif oracle is not None:
            q = q_of_rbd(m[b]); E = np.stack([oracle.rbd_from_q(q, np.eye(24)[3 + k])[24:27] for k in range(3)], axis=1)
            v = np.concatenate([m[b, 27:30], np.linalg.solve(E, m[b, 24:27]), m[b, 30:48]])
            want = oracle.rbd_from_q(q, v)[48:55]; e, moved = rel_err(m[b, 48:55], want), rel_err(m[b, 48:55], truths[n][b][48:55])
            assert e < 1e-7 and moved > 1e-4, (b, n, e, moved)      # the plant's own tolerance on rbd (tests/test_gpu_sim.py); recomputed, not copied
            if worst is not None:
                worst[0] = max(worst[0], e); worst[1] = min(worst[1], moved)


def check_plant_vs_reference(plant, oracle, what):
    """items 2 and 3: B = 4, 12 steps"""
    cases = pr.plant_cases(oracle, pr._ost())[:4]; s = plant_records(); worst = [0.0, np.inf]
    assert plant.set_sensors(s) == OK      # before the first reset
    pr._start(plant, cases); truths = [plant.state()["rbd"].copy()]
    rc, m, n = plant.measured(); assert rc == OK; check_measurement(m, n, truths, s, 0, oracle, worst)
    for k in range(1, STEPS + 1):
        st = plant.step(PERIOD, NSUB); assert (st["status"] == 0).all(); truths.append(st["rbd"].copy())
        rc, m, n = plant.measured(); assert rc == OK; check_measurement(m, n, truths, s, k, oracle, worst)
        assert np.array_equal(m[0], truths[k][0]) and np.array_equal(m[2], truths[max(k - 3, 0)][2]), k
    assert not np.array_equal(truths[STEPS][2], truths[STEPS - 3][2])      # (the plant moves: a lag that was ignored would not pass)
    print("%s: end-effector pose of the measured configuration vs the oracle, worst of 2 instances x %d samples: %.1e; least distance from the truth's pose: %.1e" % (what, STEPS + 1, *worst))


def check_generator_through_plant(plant, oracle):
    """item 1, one instance: with x = +0.0 the measured value IS the draw — the yaw rbd[0] of a reset at zero yaw under sigma = 1, the last joint rate rbd[47] of a reset at
    rest under bias_sigma = 1"""
    case = dict(pr.plant_cases(oracle, pr._ost())[0]); q = np.array(case["q"], float); q[3] = 0.0; v = np.zeros(24)
    s = sensors(1); sg = np.zeros(NG); sg[0] = 1.0; bs = np.zeros(NG); bs[5] = 1.0; record(s, 0, 1, 0, sg, bs)
    assert plant.set_sensors(s) == OK; plant.reset(q[None], v[None], T0); rc, m, n = plant.measured(); assert rc == OK and n[0] == 0
    assert plant.state()["rbd"][0, 0] == 0.0 and plant.state()["rbd"][0, 47] == 0.0
    assert m[0, 0] == 0.518857065021891 and m[0, 47] == 1.6007686074982033, (m[0, 0], m[0, 47])


_LOOPS = {}


def loop_records():
    """item 5: instance 0 the identity, instance 1 noise SIGMA, bias SIGMA / 2, lag 2"""
    s = sensors(2); record(s, 1, 5, 2, SIGMA, 0.5 * SIGMA)
    return s


def loop_run(make, what, pipelined, mode):
    """24 ticks of a device loop (the setup of test_push.loop_setup), the status words checked behind every call.  mode "never": a context that never heard of sensors;
    "off": records set, then switched off again; "on": loop_records() with the episode monitor tracing every tick.  One run per (plant, loop, mode) and session"""
    from test_push import loop_setup, N_TICKS, EVERY, HORIZON
    key = (what, pipelined, mode)
    if key in _LOOPS:
        return _LOOPS[key]
    c, q0, t_start = loop_setup(); plant = make(c); r = dict(ends=[], meas=[])
    if mode == "on":
        plant.monitor(N_TICKS); assert plant.set_sensors(loop_records()) == OK
    if mode == "off":
        assert plant.set_sensors(loop_records()) == OK and plant.set_sensors(None) == OK
        if hasattr(plant, "launches"):
            assert plant.launches() == (0, 0, 0)
    plant.reset(q0, np.zeros((2, 24)), t_start); r["rbd0"] = plant.state()["rbd"].copy(); rc, m, n = plant.measured(); assert rc == OK; r["meas0"] = (m.copy(), n.copy())
    chunk = EVERY if pipelined else 1
    for _ in range(N_TICKS // chunk):
        s = plant.closed_loop(chunk, PERIOD, HORIZON, NSUB, EVERY, pipelined=pipelined)
        assert (np.asarray(s["mpc_status"]) == 0).all() and (np.asarray(s["qp_status"]) == 0).all() and (s["status"] == 0).all(), (s["mpc_status"], s["qp_status"], s["status"])
        rc, m, n = plant.measured(); assert rc == OK; r["ends"].append(s["rbd"].copy()); r["meas"].append((m.copy(), n.copy()))
    r["state"] = s; r["launches"] = plant.launches() if hasattr(plant, "launches") else None
    if mode == "on":
        r["summary"], r["trace"] = plant.episode(N_TICKS)
    plant.close(); _LOOPS[key] = r
    return r


def _same(a, b, i):
    return all(np.array_equal(a[n][i], b[n][i]) for n in ("q", "v", "rbd", "force"))


def check_off_means_off(make, what):
    """item 4, on the synchronous loop"""
    from test_push import N_TICKS
    never, off, on = (loop_run(make, what, False, m) for m in ("never", "off", "on"))
    for r in (never, off):
        m, n = r["meas0"]; assert np.array_equal(m, r["rbd0"]) and not n.any()      # measured() is the truth, samples 0
        m, n = r["meas"][-1]; assert np.array_equal(m, r["state"]["rbd"]) and not n.any()
    if off["launches"] is not None:
        assert never["launches"] == (N_TICKS + 1, 0, 0) and off["launches"] == (N_TICKS + 1, 0, 0) and on["launches"] == (N_TICKS + 1, 0, N_TICKS + 1), (never["launches"], off["launches"], on["launches"])
    assert _same(off["state"], never["state"], slice(None))      # off: the bits of a context that never heard of sensors
    assert _same(on["state"], never["state"], 0)                  # isolation: the identity instance beside a noisy one
    d = np.abs(on["state"]["q"][1] - never["state"]["q"][1]).max(); print("%s: q of the noisy instance against its run without sensors after %d ticks: %.2e" % (what, N_TICKS, d))
    assert d > 1e-6, d


def check_loop(make, what, pipelined):
    """item 5: the loop consumes the measured state (samples count the ticks, the measured state is the reference's), the episode monitor reports from the truth"""
    from test_push import N_TICKS, EVERY
    r = loop_run(make, what, pipelined, "on"); s = loop_records(); chunk = EVERY if pipelined else 1; tr = r["trace"]; sm = r["summary"]
    assert tr.shape[0] == N_TICKS and (tr["tick"] == np.arange(N_TICKS)[:, None]).all()
    truths = [r["rbd0"]] + [tr["rbd"][k] for k in range(N_TICKS)]      # sample n: the reset state, then the state behind tick n - 1
    m, n = r["meas0"]; check_measurement(m, n, truths, s, 0)
    for i, (m, n) in enumerate(r["meas"]):
        k = (i + 1) * chunk
        assert np.array_equal(tr["rbd"][k - 1], r["ends"][i]), k      # the monitor's samples are the plant's state ...
        check_measurement(m, n, truths, s, k)                         # ... and the measured state is the reference's corruption of them
        assert not np.array_equal(m[1], r["ends"][i][1])
    dev = np.linalg.norm(tr["rbd"][:, :, 48:51] - r["rbd0"][None, :, 48:51], axis=2).max(axis=0)      # anchored at the reset state's TRUE end-effector position
    assert (sm["ticks"] == N_TICKS).all() and (sm["fall_tick"] < 0).all()
    assert np.array_equal(sm["min_base_z"], tr["rbd"][:, :, 5].min(axis=0)) and np.allclose(sm["max_ee_pos_dev"], dev, rtol=1e-12, atol=0.0), (sm["max_ee_pos_dev"], dev)
    assert (dev > 0).all()


def check_errors(make, oracle):
    """item 7: every refused call returns its code and leaves the records in force — the next sample equals the sample of a twin context bit for bit"""
    cases = pr.plant_cases(oracle, pr._ost())[:2]; B = 2; good = sensors(B); record(good, 0, 21, 1, SIGMA); record(good, 1, 22, 2, 0.0, SIGMA)
    a = make(B); twin = make(B)
    assert a.set_sensors(good) == OK and twin.set_sensors(good) == OK      # before the first reset: allocated on demand
    pr._start(a, cases); pr._start(twin, cases)
    for _ in range(2):
        a.step(PERIOD, NSUB); twin.step(PERIOD, NSUB)
    other = sensors(B); record(other, 0, 31, 0, 10.0 * SIGMA); record(other, 1, 32, 4, SIGMA, SIGMA); bad = [(0, other), (-1, other), (B + 1, sensors(B + 1))]
    for field, val in (("lag", -1), ("lag", MAX_LAG + 1), ("sigma", -1e-3), ("sigma", np.nan), ("sigma", np.inf), ("bias_sigma", -1e-3), ("bias_sigma", np.nan), ("bias_sigma", -np.inf)):
        s = other.copy()
        if field == "lag":
            s["lag"][1] = val
        else:
            s[field][1, 4] = val
        bad.append((B, s))
    for k, (nb, s) in enumerate(bad):
        assert a.set_sensors_raw(nb, s) == ERR_ARG, k
    assert a.measured(0)[0] == ERR_ARG and a.measured(B + 1)[0] == ERR_ARG
    a.set_wbc_only(True)
    assert a.set_sensors_raw(B, other) == ERR_STATE and a.set_sensors(None) == ERR_STATE and a.measured()[0] == ERR_STATE
    a.set_wbc_only(False)
    for k in range(3, 6):
        sa = a.step(PERIOD, NSUB); st = twin.step(PERIOD, NSUB); ma, mt = a.measured(), twin.measured()
        assert ma[0] == OK and np.array_equal(ma[1], mt[1]) and np.array_equal(ma[2], mt[2]) and (ma[2] == k).all() and np.array_equal(sa["rbd"], st["rbd"]), k
    # new records in the middle of an episode: the count starts over, sample 0 is taken from the current truth at once, the plant is not launched
    before = a.launches() if hasattr(a, "launches") else None
    assert a.set_sensors(other) == OK; rc, m, n = a.measured(); truth = a.state()["rbd"]
    assert rc == OK and not n.any() and np.array_equal(truth, sa["rbd"])
    for b in range(B):
        assert np.array_equal(m[b, :NC], corrupt(truth[b], other[b], 0)), b
    if before is not None:
        assert a.launches() == (before[0], before[1], before[2] + 1)
    a.step(PERIOD, NSUB); rc, m, n = a.measured(); assert (n == 1).all() and np.array_equal(m[1, :NC], corrupt(truth[1], other[1], 1))      # lag 4 at sample 1: still the oldest sample
    a.close(); twin.close()
