"""tests/published_ref.py — TEST INFRASTRUCTURE of the published feedback policy (include/qmhip.h "published feedback policy"), shared by tests/test_published_policy.py (host
emulator) and tests/test_gpu_published_policy.py (device): the ctypes binding of tests/emu_pub, the numpy coverage predicate, and the pipelined loop built from the oracle's
pieces with the linear controller in the tick."""
import ctypes as C
import os
import subprocess

import numpy as np

import feedback_ref as fr
import interp_cases as ic

_HERE = os.path.dirname(os.path.abspath(__file__))
SIM_PARAMS = np.array([4.0e4, 200.0, 0.8, 1.0e-2, 0.02, 0.009, 1.0])      # the defaults of api.QMHWSim / emu_harness.Emu.sim_params


def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_pub"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_pub", "_build", "libqm_emu_pub.so"))
    lib.emu_pub_create.restype = C.c_void_p; lib.emu_pub_publish_eval.restype = C.c_long
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def covered_ref(res, W, t):
    """the predicate of qm_policy_fb_pub_kernel: both nodes bracketing t (the feed-forward policy's segment on the nudged node times) lie inside min(W, n)"""
    ta = res["t"] + np.where(res["ev"] == 2, ic.LIMIT_EPS, np.where(res["ev"] == 1, -ic.LIMIT_EPS, 0.0)); n = len(ta)
    i, _ = ic.time_segment(ta, t); j = i + 1 if n > 1 else i; wn = min(W, n)
    return int(i < wn and j < wn)


class EmuLoop:
    """the pipelined loop around the plant on the host emulator (tests/emu_pub): one context, a publish window, the loop with or without the publisher"""

    def __init__(self, lib, mb, st, Bmax, nmax, nref, nev):
        self.lib = lib; self.mb = np.ascontiguousarray(mb, float); self.st = np.ascontiguousarray(st, float)
        self.h = C.c_void_p(lib.emu_pub_create(ptr(self.mb), ptr(self.st), Bmax, nmax, nref, nev)); self.B = 0

    def close(self):
        if self.h: self.lib.emu_pub_destroy(self.h); self.h = None

    def set_window(self, W): self.lib.emu_pub_set_window(self.h, C.c_int(W))

    def start(self, cfg, B, q0, time0):
        a = lambda k, t=float: np.ascontiguousarray(cfg[k][:B], t)
        self.lib.emu_pub_upload_grid(self.h, C.c_int(B), ptr(a("t0")), ptr(a("x0")), ptr(a("ref_t")), ptr(a("ref_x")), ptr(a("ev")), ptr(a("modes", np.int32)), C.c_double(cfg["horizon"]))
        q = np.ascontiguousarray(np.tile(q0, (B, 1)), float); v = np.zeros((B, 24)); t = np.full(B, float(time0))
        self.lib.emu_pub_sim_start(self.h, C.c_int(B), ptr(SIM_PARAMS), ptr(q), ptr(v), ptr(t)); self.B = B

    def loop(self, n_ticks, period, horizon, nsub, mpc_every, feedback, arm_kp=0.0, arm_kd=0.5):
        self.lib.emu_pub_loop(self.h, C.c_int(self.B), C.c_int(n_ticks), C.c_double(period), C.c_int(nsub), C.c_int(mpc_every), C.c_double(horizon), C.c_double(arm_kp), C.c_double(arm_kd), C.c_int(int(feedback)))

    def state(self):
        B = self.B; q = np.zeros((B, 24)); v = np.zeros((B, 24)); out = np.zeros((B, 54)); qp = np.zeros((B, 3), np.int32); ms = np.zeros(B, np.int32); ud = np.zeros((B, 30)); unc = np.zeros(B, np.int32); seq = C.c_long(0)
        self.lib.emu_pub_state(self.h, C.c_int(B), ptr(q), ptr(v), ptr(out), ptr(qp), ptr(ms), ptr(ud), ptr(unc), C.byref(seq))
        return dict(q=q, v=v, out=out, tau=out[:, 36:].copy(), wbc_status=qp, mpc_status=ms, u_des=ud, uncovered=unc, seq=seq.value)

    def counts(self):
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0); self.lib.emu_pub_counts(self.h, C.byref(a), C.byref(b), C.byref(c)); return a.value, b.value, c.value


def oracle_pipelined_feedback_loop(oracle, mb, cfg, q0, n_ticks, period, nsub, mpc_every, horizon, arm_kp, arm_kd, time0):
    """tests/test_sim.py::_oracle_closed_loop(pipelined=True) — the MPC triggered at a period's first tick observes the plant there, its solution is used from the next period
    on, the first one synchronously — with the LINEAR controller in the tick: the gains are taken at solve time, while the oracle still holds that solve
    (feedback_ref.oracle_gains), and used one period later with feedback_ref.linear_policy at the tick's centroidal_from_rbd estimate.  x_des and mode come from the solve the
    gains belong to (ic.policy_reference / the schedule).  Runs on the robust time grid like test_sim.oracle_closed_loop"""
    from qm_control_amd import layout as L
    from test_sim import centroidal_from_rbd
    assert n_ticks % mpc_every == 0
    old = oracle.set_setting(L.ST_GRID_DT_MIN, L.QM_GRID_DT_MIN_ROBUST)
    try:
        oracle.set_schedule(cfg["ev"][0], cfg["modes"][0]); oracle.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
        oracle.wbc_reset(); oracle.sim_params(); oracle.sim_reset(q0, np.zeros(24), time0); oracle.sim_command(0, 0, 0, 0, 0)
        st = dict(rbd=oracle.rbd_from_q(q0, np.zeros(24)), time=time0, k=0); log = []
        pos = np.zeros(18); vel = np.zeros(18); kp = np.zeros(18); kd = np.zeros(18); ff = np.zeros(18)
        ev_t = np.asarray(cfg["ev"][0], float); ev_m = np.asarray(cfg["modes"][0])

        def solve(t_obs, x_obs, warm):
            r = oracle.mpc_step(t_obs, t_obs + horizon, x_obs, warm=warm); assert r["warn"] == 0
            K, _, src = fr.oracle_gains(oracle, r); return dict(r=r, K=K, src=src)

        def tick(pol):
            time, rbd = st["time"], st["rbd"]; r = pol["r"]; x_est = centroidal_from_rbd(mb, rbd)
            xd, uff = ic.policy_reference(r["t"], r["ev"], r["x"], r["u"], time); ud = fr.linear_policy(r, pol["K"], pol["src"], time, x_est)
            mode = int(ev_m[int(np.searchsorted(ev_t, time, side="left"))])      # ModeSchedule::modeAtTime (grid_find_index: lower bound)
            if st["k"] == 0: oracle.wbc_set_input_last(ud)
            out, wst = oracle.wbc(xd, ud, rbd, mode, period, time)
            if time > 10.0: pos[:12] = xd[12:24]; vel[:12] = ud[12:24]; kp[:12] = 0.0; kd[:12] = 3.0; ff[:12] = out[36:48]
            pos[12:] = xd[24:30]; vel[12:] = 0.0; kp[12:] = arm_kp; kd[12:] = arm_kd; ff[12:] = out[48:54]
            oracle.sim_command(pos, vel, kp, kd, ff); s = oracle.sim_step(period, nsub); st["rbd"] = s["rbd"]; st["time"] = s["time"]; st["k"] += 1
            log.append(dict(q=s["q"].copy(), v=s["v"].copy(), tau=out[36:].copy(), wbc_status=list(wst), du=float(np.abs(ud - uff).max()), covered=covered_ref(r, 1 << 30, time), node=_node_of(r, time)))

        pol = None
        for p in range(n_ticks // mpc_every):
            t_obs, x_obs = st["time"], centroidal_from_rbd(mb, st["rbd"])
            if p == 0: pol = solve(t_obs, x_obs, False)
            for _ in range(mpc_every): tick(pol)
            if p > 0: pol = solve(t_obs, x_obs, True)
        return log
    finally:
        oracle.set_setting(L.ST_GRID_DT_MIN, old)


def _node_of(r, t):
    ta = r["t"] + np.where(r["ev"] == 2, ic.LIMIT_EPS, np.where(r["ev"] == 1, -ic.LIMIT_EPS, 0.0)); i, _ = ic.time_segment(ta, t); return i + 1
