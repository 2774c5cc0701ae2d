"""tests/push_ref.py — TEST INFRASTRUCTURE of the plant's scheduled external wrenches (qmhip_sim_set_pushes; include/qmhip.h "plant disturbances").

PushRef: the checker.  The oracle's plant (oracle/src/sim.h) knows no external force, so the reference is a numpy sub-step assembled from oracle quantities: M, nle and the
12 x 24 foot Jacobian from Oracle.wbc(..., debug=True) on Oracle.rbd_from_q(q, v), foot positions from Oracle.frame_pose, E column by column from
Oracle.rbd_from_q(q, e_{3+k})[24:27], J_ee from central differences (step 1e-6) of Oracle.frame_pose(q, 4); the command law with effort saturation, the penalty contact,
the semi-implicit Euler step and the time accumulation are restated from sim.h.  The held command is constant over a run (set once behind the reset), so every entry of the
delay buffer is that command and the buffer needs no restatement.

EmuPlant / DevPlant: the same few calls on the host emulator (tests/emu_push) and on the device (api.QMHWSim), so that tests/test_push.py and tests/test_gpu_push.py run the
SAME checks (check_* below) with the same shapes and the same assertions."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from conftest import rel_err
from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double); _ip = C.POINTER(C.c_int32)
_p = lambda a: None if a is None else a.ctypes.data_as(_dp)
_pi = lambda a: None if a is None else a.ctypes.data_as(_ip)
OK, ERR_ARG, ERR_STATE = 0, -1, -5
KMAX = L.QM_SIM_MAX_PUSH
INF = float("inf")
# tolerances of test_plant_vs_oracle (tests/test_gpu_sim.py), the project's own for this kernel
TOL = dict(q=1e-9, v=1e-7, force=1e-6, rbd=1e-7, time=1e-12)


def pushes(B, K):
    """[B][K] records of dtype api.PUSH, every slot inactive (t_on == t_off is never active)"""
    return np.zeros((B, K), api.PUSH)


def slot(p, b, k, t_on, t_off, base_force=(0, 0, 0), base_torque=(0, 0, 0), ee_force=(0, 0, 0)):
    p["t_on"][b, k] = t_on; p["t_off"][b, k] = t_off; p["base_force"][b, k] = base_force; p["base_torque"][b, k] = base_torque; p["ee_force"][b, k] = ee_force


def applied(p_b, t_s):
    """(wrench [9], mask) of one instance's slots at sub-step start time t_s: the sum over the active slots in ascending order, from +0.0"""
    w = np.zeros(9); mask = 0
    for k in range(len(p_b)):
        if p_b[k]["t_on"] <= t_s < p_b[k]["t_off"]:
            mask |= 1 << k; w = w + np.concatenate([p_b[k]["base_force"], p_b[k]["base_torque"], p_b[k]["ee_force"]])
    return w, mask


def substep_times(t0, period, nsub, steps):
    """start times of all sub-steps [steps][nsub] and the time behind every step [steps], accumulated as the kernel accumulates them: one `time += h` per sub-step"""
    h = np.float64(period) / nsub; t = np.float64(t0); ts = np.zeros((steps, nsub)); te = np.zeros(steps)
    for k in range(steps):
        for s in range(nsub):
            ts[k, s] = t; t = t + h
        te[k] = t
    return ts, te


class PushRef:
    def __init__(self, oracle, omb, ost, k_n=4.0e4, d_n=200.0, mu=0.8, v_eps=1.0e-2, foot_radius=0.02):
        self.o = oracle; self.taumax = np.array(omb[L.MB_TAUMAX:L.MB_TAUMAX + 18], float); self.xinit = np.array(ost[L.ST_XINIT:L.ST_XINIT + 30], float)
        self.k_n, self.d_n, self.mu, self.v_eps, self.r = k_n, d_n, mu, v_eps, foot_radius

    def ee_jacobian(self, q, eps=1e-6):
        J = np.zeros((3, 24))
        for i in range(24):
            qp = q.copy(); qm = q.copy(); qp[i] += eps; qm[i] -= eps
            J[:, i] = (self.o.frame_pose(qp, 4)[0] - self.o.frame_pose(qm, 4)[0]) / (2.0 * eps)
        return J

    def euler_E(self, q):
        return np.stack([self.o.rbd_from_q(q, np.eye(24)[3 + k])[24:27] for k in range(3)], axis=1)      # column k: the angular velocity of a unit rate k

    def substep(self, q, v, h, cmd, wrench):
        o = self.o; d = o.wbc(self.xinit, np.zeros(30), o.rbd_from_q(q, v), 15, 0.002, 20.0, debug=True)[2]; M, nle, J = d["M"], d["nle"], d["J"]
        tau = cmd["kp"] * (cmd["pos"] - q[6:]) + cmd["kd"] * (cmd["vel"] - v[6:]) + cmd["ff"]; tau = np.minimum(self.taumax, np.maximum(-self.taumax, tau))
        force = np.zeros(12)
        for f in range(4):
            vf = J[3 * f:3 * f + 3] @ v; pen = self.r - o.frame_pose(q, f)[0][2]
            if pen > 0.0:
                fz = max(0.0, self.k_n * pen - self.d_n * vf[2]); sc = -self.mu * fz / np.sqrt(vf[0] * vf[0] + vf[1] * vf[1] + self.v_eps * self.v_eps)
                force[3 * f:3 * f + 3] = (sc * vf[0], sc * vf[1], fz)
        rhs = np.concatenate([np.zeros(6), tau]) - nle + J.T @ force
        if wrench is not None:
            rhs[0:3] += wrench[0:3]
            if np.any(wrench[3:6] != 0.0):
                rhs[3:6] += self.euler_E(q).T @ wrench[3:6]
            if np.any(wrench[6:9] != 0.0):
                rhs += self.ee_jacobian(q).T @ wrench[6:9]
        a = np.linalg.solve(M, rhs)
        v = v + h * a; q = q + h * v
        return q, v, force

    def run(self, case, p_b, steps, period, nsub, t0):
        """one instance: `steps` steps from (case q, v) at time t0 under the constant command of `case` and the slots p_b ([K] of api.PUSH, or None)"""
        q = np.array(case["q"], float); v = np.array(case["v"], float); ts, te = substep_times(t0, period, nsub, steps); h = np.float64(period) / nsub; out = []
        for k in range(steps):
            for s in range(nsub):
                w, mask = applied(p_b, ts[k, s]) if p_b is not None else (None, 0)
                q, v, force = self.substep(q, v, h, case, w)
            contact = np.array([1 if self.r - self.o.frame_pose(q, f)[0][2] > 0.0 else 0 for f in range(4)], np.int32)
            out.append(dict(q=q.copy(), v=v.copy(), time=te[k], force=force, contact=contact, rbd=self.o.rbd_from_q(q, v), wrench=np.zeros(9) if w is None else w, mask=mask))
        return out


# ---------------------------------------------------------------- the two plants
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_push"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_push", "_build", "libqm_emu_push.so")); lib.emu_push_create.restype = C.c_void_p
    return lib


def _bcast(x, B):
    return np.ascontiguousarray(np.broadcast_to(x, (B, 18)), float)


def _push_arg(p):
    """(B, K, pointer, keep-alive) of a [B][K] / [B] array of api.PUSH"""
    p = np.ascontiguousarray(p, dtype=api.PUSH)
    if p.ndim == 1:
        p = p[:, None]
    return p.shape[0], p.shape[1], p.ctypes.data_as(C.c_void_p), p


class EmuPlant:
    """solver, WBC and plant in one emulator context (tests/emu_push/emu_push_api.cpp); the method names of api.QMHWSim where they exist"""

    def __init__(self, lib, blobs, Bmax, nev=2, nmax=8):
        self.lib = lib; self.mb = np.ascontiguousarray(blobs[0], float); self.st = np.ascontiguousarray(blobs[1], float); self.Bmax = Bmax; self.B = Bmax
        self.h = C.c_void_p(lib.emu_push_create(_p(self.mb), _p(self.st), Bmax, nmax, 2, nev))

    def close(self):
        if self.h:
            self.lib.emu_push_destroy(self.h); self.h = None

    def upload(self, c, B):
        a = lambda k, t=float: np.ascontiguousarray(c[k][:B], t)
        self.lib.emu_push_upload(self.h, B, _p(a("t0")), _p(a("x0")), _p(a("ref_t")), _p(a("ref_x")), _p(a("ev")), _pi(a("modes", np.int32)))

    def reset(self, q, v, time):
        q = np.ascontiguousarray(q, float); self.B = B = q.shape[0]; v = np.ascontiguousarray(v, float); t = np.ascontiguousarray(np.broadcast_to(time, (B,)), float)
        self.lib.emu_push_sim_reset(self.h, B, _p(q), _p(v), _p(t))

    def command(self, pos, vel, kp, kd, ff):
        cmd = np.ascontiguousarray(np.concatenate([_bcast(x, self.B) for x in (pos, vel, kp, kd, ff)], axis=1)); self.lib.emu_push_sim_command(self.h, self.B, _p(cmd))

    def state(self):
        B = self.B; d = dict(q=np.zeros((B, 24)), v=np.zeros((B, 24)), time=np.zeros(B), rbd=np.zeros((B, 55)), contact=np.zeros((B, 4), np.int32), force=np.zeros((B, 12)), status=np.zeros(B, np.int32),
                             qp_status=np.zeros((B, 3), np.int32), mpc_status=np.zeros(B, np.int32))
        self.lib.emu_push_readback(self.h, B, _p(d["q"]), _p(d["v"]), _p(d["time"]), _p(d["rbd"]), _pi(d["contact"]), _p(d["force"]), _pi(d["status"]), _pi(d["qp_status"]), _pi(d["mpc_status"]))
        return d

    def step(self, period, nsub):
        self.lib.emu_push_sim_step(self.h, self.B, C.c_double(period), nsub)
        return self.state()

    def closed_loop(self, n, period, horizon, nsub, mpc_every, pipelined=False):
        self.lib.emu_push_closed_loop(self.h, self.B, n, C.c_double(period), nsub, mpc_every, C.c_double(horizon), C.c_double(0.0), C.c_double(0.5), int(pipelined))
        return self.state()

    def set_pushes(self, p):
        if p is None:
            return self.lib.emu_push_set_pushes(self.h, 0, 0, None)
        B, K, ptr, _keep = _push_arg(p)
        return self.lib.emu_push_set_pushes(self.h, B, K, ptr)

    def set_pushes_raw(self, B, K, p):
        return self.lib.emu_push_set_pushes(self.h, B, K, None if p is None else p.ctypes.data_as(C.c_void_p))

    def push_state(self, B=None):
        B = self.B if B is None else B; w = np.zeros((max(B, 1), 9)); m = np.zeros(max(B, 1), np.int32)
        return self.lib.emu_push_get_push(self.h, B, _p(w), _pi(m)), w, m

    def set_wbc_only(self, on):
        """the context refuses the plant's calls like one of qmhip_create_wbc_context (the product's guard itself runs in tests/test_gpu_push.py)"""
        self.lib.emu_push_set_wbc_only(self.h, int(on))

    def launches(self):
        a = C.c_int(0); b = C.c_int(0); self.lib.emu_push_counts(self.h, C.byref(a), C.byref(b))
        return a.value, b.value


class DevPlant:
    """the same calls through the C ABI on the device"""

    def __init__(self, blobs, Bmax, nev=2, nmax=8, c=None):
        self.itf = api.QMInterface(blobs=blobs, max_batch=Bmax, max_nodes=nmax, max_ref_knots=2, max_events=nev); self.sim = api.QMHWSim(self.itf, robust_grid=c is not None)
        self.mpc = api.SqpMpc(self.itf); self.wbc = api.HierarchicalWbc(self.itf); self.Bmax = Bmax; self.B = Bmax; self.other = None
        if c is not None:
            self.mpc.set_problem(c["t0"], c["x0"], c["ref_t"], c["ref_x"], c["ev"], c["modes"]); self.wbc.reset()

    def close(self):
        if self.other is not None:
            self.other.close(); self.other = None
        self.itf.close()

    def reset(self, q, v, time):
        self.sim.reset(q, v, time); self.B = self.sim.B

    def command(self, pos, vel, kp, kd, ff):
        self.sim.setCommand(pos, vel, kp, kd, ff)

    def state(self):
        s = self.sim.state(); s["rbd"], s["contact"] = self.sim.rbd()
        return s

    def step(self, period, nsub):
        self.sim.step(period, nsub, download=False)
        return self.state()

    def closed_loop(self, n, period, horizon, nsub, mpc_every, pipelined=False):
        self.sim.closed_loop(n, period, horizon, n_substeps=nsub, mpc_every=mpc_every, pipelined=pipelined); s = self.state()
        s["qp_status"] = self.wbc.download(self.B)[1]; s["mpc_status"] = self.mpc.download()["status"]
        return s

    def _h(self):
        return self.itf.h if self.other is None else self.other.h

    def set_pushes(self, p):
        if p is None:
            return self.itf.lib.qmhip_sim_set_pushes(self._h(), 0, 0, None)
        B, K, ptr, _keep = _push_arg(p)
        return self.itf.lib.qmhip_sim_set_pushes(self._h(), B, K, ptr)

    def set_pushes_raw(self, B, K, p):
        return self.itf.lib.qmhip_sim_set_pushes(self._h(), B, K, None if p is None else p.ctypes.data_as(C.c_void_p))

    def push_state(self, B=None):
        B = self.B if B is None else B; w = np.zeros((max(B, 1), 9)); m = np.zeros(max(B, 1), np.int32)
        return self.itf.lib.qmhip_sim_get_push(self._h(), B, _p(w), _pi(m)), w, m

    def set_wbc_only(self, on):
        """the push calls go to a WBC-only context made from this one (qmhip_create_wbc_context)"""
        if on and self.other is None:
            self.other = self.itf.wbc_context()
        if not on and self.other is not None:
            self.other.close(); self.other = None


# ---------------------------------------------------------------- shared cases and checks
STEPS, PERIOD, NSUB, T0 = 12, 0.001, 2, 1.0
FORCE, TORQUE, EE = (80.0, -40.0, 30.0), (10.0, 20.0, -15.0), (20.0, 30.0, -25.0)


def plant_cases(oracle, ost):
    from test_sim import random_cases
    return random_cases(oracle, ost, 6, 11)


def plant_schedule():
    """test 1: B = 6, K = 3 — one component each, all three in one slot, overlapping windows with one that opens and closes inside the run, a permanent end-effector load"""
    p = pushes(6, 3)
    slot(p, 0, 1, T0, 2.0, base_force=FORCE)
    slot(p, 1, 0, T0, 2.0, base_torque=TORQUE)
    slot(p, 2, 2, T0, 2.0, ee_force=EE)
    slot(p, 3, 0, 0.0, 2.0, FORCE, TORQUE, EE)
    slot(p, 4, 0, T0, T0 + 0.008, base_force=(50.0, 10.0, 0.0)); slot(p, 4, 1, T0 + 0.003, 2.0, ee_force=(0.0, -20.0, 10.0)); slot(p, 4, 2, T0 + 0.0045, T0 + 0.0075, base_force=(-30.0, 0.0, 20.0), base_torque=(0.0, 8.0, 0.0))
    slot(p, 5, 0, -INF, INF, ee_force=(0.0, 0.0, -15.0))
    return p


@functools.lru_cache(maxsize=None)
def _reference_runs_cached(oracle):
    import pyoracle
    omb, ost = pyoracle.load_blobs(); ref = PushRef(oracle, omb, ost); cases = plant_cases(oracle, ost); p = plant_schedule()
    pushed = [ref.run(c, p[b], STEPS, PERIOD, NSUB, T0) for b, c in enumerate(cases)]
    plain = [ref.run(cases[b], None, STEPS, PERIOD, NSUB, T0) for b in range(3)]      # the single-component instances without their push
    return cases, p, pushed, plain


def reference_runs(oracle):
    """(cases, schedule, pushed reference runs [6][STEPS], unpushed reference runs of instances 0-2) — computed once per session, shared by the CPU and the GPU test"""
    return _reference_runs_cached(oracle)


def _arr(cases, k):
    return np.array([c[k] for c in cases])


def _start(plant, cases, t0=T0):
    plant.reset(_arr(cases, "q"), _arr(cases, "v"), t0); plant.command(*[_arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")])


def check_plant_vs_reference(plant, oracle, what):
    """test 1"""
    cases, p, pushed, plain = reference_runs(oracle)
    # a push the plant ignored must not pass: every single component moves the reference itself by five decades more than the tolerances
    for b in range(3):
        eq, ev = rel_err(pushed[b][-1]["q"], plain[b][-1]["q"]), rel_err(pushed[b][-1]["v"], plain[b][-1]["v"]); print("%s: reference pushed vs unpushed, instance %d: q %.2e v %.2e" % (what, b, eq, ev))
        assert eq >= 1e-4 and ev >= 1e-2, (b, eq, ev)
    assert plant.set_pushes(p) == OK; _start(plant, cases); worst = dict(q=0.0, v=0.0, force=0.0, rbd=0.0, time=0.0)
    for k in range(STEPS):
        s = plant.step(PERIOD, NSUB); rc, w, m = plant.push_state(); assert rc == OK
        for b in range(6):
            r = pushed[b][k]; e = dict(q=rel_err(s["q"][b], r["q"]), v=rel_err(s["v"][b], r["v"]), force=rel_err(s["force"][b], r["force"]), rbd=rel_err(s["rbd"][b], r["rbd"]), time=abs(s["time"][b] - r["time"]))
            worst = {n: max(worst[n], e[n]) for n in e}
            assert s["status"][b] == 0 and all(e[n] < TOL[n] for n in e), (b, k, e)
            assert list(s["contact"][b]) == list(r["contact"]), (b, k)
            assert m[b] == r["mask"] and np.array_equal(w[b], r["wrench"]), (b, k, m[b], r["mask"], w[b], r["wrench"])
    print("%s vs push_ref, worst over 6 instances x %d steps: %s" % (what, STEPS, {n: "%.1e" % x for n, x in worst.items()}))


def check_window_edges(plant, oracle, j=4, steps=8):
    """test 2: nsub = 1, four copies of one state; t* = start time of sub-step j, accumulated by the same repeated += h"""
    cases = [plant_cases(oracle, _ost())[0]] * 4; ts, _ = substep_times(T0, PERIOD, 1, steps); t = ts[j, 0]; F = np.array([12.0, -7.0, 3.0])
    p = pushes(4, 1)
    slot(p, 0, 0, t, INF, base_force=F); slot(p, 1, 0, np.nextafter(t, INF), INF, base_force=F); slot(p, 2, 0, -INF, t, base_force=F); slot(p, 3, 0, t, t, base_force=F)
    assert plant.set_pushes(p) == OK; _start(plant, cases)
    rc, w, m = plant.push_state(); assert rc == OK and not m.any() and not w.any()      # the hand-over launch of the reset applies nothing
    for k in range(steps):
        plant.step(PERIOD, 1); rc, w, m = plant.push_state(); assert rc == OK
        want = np.array([k >= j, k >= j + 1, k <= j - 1, False]); ww = np.zeros((4, 9)); ww[want, 0:3] = F
        assert np.array_equal(m, want.astype(np.int32)) and np.array_equal(w, ww), (k, m, w)


def _ost():
    import pyoracle
    return pyoracle.load_blobs()[1]


def _run(plant, cases, p, steps, nsub=NSUB):
    assert plant.set_pushes(p) == OK; _start(plant, cases)
    for _ in range(steps):
        s = plant.step(PERIOD, nsub)
    return s


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(a[n][rows], b[n][rows]) for n in ("q", "v", "rbd", "force"))


def check_slot_sum(make, oracle):
    """test 3: two slots active together equal one slot holding the float sums, K = 1 against K = QM_SIM_MAX_PUSH with the unused slots inactive; B = 1"""
    cases = [plant_cases(oracle, _ost())[1]]; a = dict(base_force=np.array(FORCE), base_torque=np.array(TORQUE), ee_force=np.array(EE))
    b = dict(base_force=np.array([-13.7, 0.3, 51.0]), base_torque=np.array([0.1, -9.9, 4.4]), ee_force=np.array([7.7, -0.9, 13.1]))
    one = pushes(1, 1); slot(one, 0, 0, T0, 2.0, **{n: a[n] + b[n] for n in a})
    two = pushes(1, KMAX); slot(two, 0, 2, T0, 2.0, **a); slot(two, 0, KMAX - 1, -INF, INF, **b); slot(two, 0, 0, 2.0, 3.0, **b); slot(two, 0, 4, 0.0, T0, **a)      # (two more that are never active in the run)
    p1 = make(1); s1 = _run(p1, cases, one, 6); rc, w1, m1 = p1.push_state(); p1.close()
    p2 = make(1); s2 = _run(p2, cases, two, 6); rc, w2, m2 = p2.push_state(); p2.close()
    assert m1[0] == 1 and m2[0] == (1 << 2 | 1 << (KMAX - 1)) and np.array_equal(w1, w2)
    assert _same(s1, s2) and s1["status"][0] == 0


def check_isolation_and_off(make, oracle, what):
    """test 4"""
    cases = plant_cases(oracle, _ost())[:3]; B = 3
    pushed = pushes(B, 2); slot(pushed, 0, 0, T0, 2.0, FORCE, TORQUE, EE); slot(pushed, 2, 1, T0 + 0.002, 2.0, ee_force=EE); slot(pushed, 1, 0, 5.0, 6.0, base_force=FORCE)      # instance 1: a slot that never opens in the run
    nobody = pushes(B, 2); slot(nobody, 1, 0, 5.0, 6.0, base_force=FORCE); slot(nobody, 0, 1, 5.0, 6.0, base_force=FORCE)
    a = make(B); sa = _run(a, cases, pushed, 6); b = make(B); sb = _run(b, cases, nobody, 6)
    assert _same(sa, sb, 1) and not _same(sa, sb, 0) and not _same(sa, sb, 2)      # both through the push kernel: bit for bit
    if hasattr(b, "launches"):
        assert a.launches() == (0, 7) and b.launches() == (0, 7)      # (plain, push) kernel launches: the reset's hand-over and six steps
    # a schedule that covers fewer instances than the step: the instances behind it have none
    c = make(B); sc = _run(c, cases, pushed[:1], 6); rc, w, m = c.push_state(); assert rc == OK and m[0] == 1 and not m[1:].any() and not w[1:].any()
    assert _same(sc, sa, 0) and _same(sc, sb, 1) and _same(sc, sb, 2)
    # pushes off again: equal to a context that never had a schedule, bit for bit (both run the plain kernel)
    assert c.set_pushes(None) == OK; _start(c, cases)
    for _ in range(6):
        s_off = c.step(PERIOD, NSUB)
    rc, w, m = c.push_state(); assert rc == OK and not m.any() and not w.any()
    d = make(B); _start(d, cases)
    for _ in range(6):
        s_never = d.step(PERIOD, NSUB)
    assert _same(s_off, s_never) and np.array_equal(s_off["time"], s_never["time"])
    if hasattr(d, "launches"):
        assert d.launches() == (7, 0) and c.launches() == (7, 7)
    # against the plain kernel the all-inactive instances agree within the plant's tolerances (two compilations of one body: not asserted bit for bit)
    e = {n: max(rel_err(sb[n][i], s_never[n][i]) for i in range(B)) for n in ("q", "v", "force", "rbd")}
    print("%s: push kernel with inactive slots vs plain kernel, largest relative difference after 6 steps: %s" % (what, {n: "%.1e" % x for n, x in e.items()}))
    assert all(e[n] < TOL[n] for n in e) and np.array_equal(sb["contact"], s_never["contact"]), e
    for x in (a, b, c, d):
        x.close()


def check_errors(make, oracle):
    """test 6: every refused call returns its code and leaves the schedule untouched — the next step equals the step of an identical context bit for bit"""
    cases = plant_cases(oracle, _ost())[:2]; B = 2; good = pushes(B, 2); slot(good, 0, 0, T0, 2.0, FORCE, TORQUE, EE); slot(good, 1, 1, T0, 2.0, ee_force=EE)
    a = make(B); twin = make(B)
    assert a.set_pushes(good) == OK and twin.set_pushes(good) == OK      # before the first reset: allocated on demand
    _start(a, cases); _start(twin, cases)
    rc, w, m = a.push_state(); assert rc == OK and not w.any() and not m.any()      # zeros after a reset
    bad = []
    for field, idx, val in (("t_on", None, np.nan), ("t_off", None, np.nan), ("base_force", 1, INF), ("base_torque", 0, np.nan), ("ee_force", 2, -INF)):
        p = good.copy()
        if idx is None:
            p[field][1, 0] = val
        else:
            p[field][1, 0, idx] = val
        bad.append((B, 2, p))
    other = pushes(B, 2); slot(other, 0, 0, -INF, INF, base_force=(500.0, 0.0, 0.0)); big = pushes(B, KMAX + 1)
    bad += [(0, 2, other), (-1, 2, other), (B + 1, 2, pushes(B + 1, 2)), (B, -1, other), (B, KMAX + 1, big)]
    for k, (nb, nk, p) in enumerate(bad):
        assert a.set_pushes_raw(nb, nk, p) == ERR_ARG, k
    assert a.push_state(0)[0] == ERR_ARG and a.push_state(B + 1)[0] == ERR_ARG
    a.set_wbc_only(True)
    assert a.set_pushes_raw(B, 2, other) == ERR_STATE and a.set_pushes_raw(0, 0, None) == ERR_STATE and a.push_state()[0] == ERR_STATE
    a.set_wbc_only(False)
    for _ in range(3):
        sa = a.step(PERIOD, NSUB); st = twin.step(PERIOD, NSUB)
        assert _same(sa, st) and np.array_equal(a.push_state()[1], twin.push_state()[1]) and np.array_equal(a.push_state()[2], twin.push_state()[2])
    assert a.push_state()[2].tolist() == [1, 2]
    # t_off = +inf, t_on = -inf and infinite windows are arguments like any other
    ok = good.copy(); ok[0, 1]["t_on"] = -INF; ok[0, 1]["t_off"] = INF; assert a.set_pushes(ok) == OK
    a.reset(_arr(cases, "q"), _arr(cases, "v"), T0); rc, w, m = a.push_state(); assert rc == OK and not w.any() and not m.any()      # zeros after a reset, the schedule stays
    a.command(*[_arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); a.step(PERIOD, NSUB); assert a.push_state()[2].tolist() == [3, 2]
    a.close(); twin.close()
