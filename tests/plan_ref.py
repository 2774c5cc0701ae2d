"""tests/plan_ref.py — TEST INFRASTRUCTURE: the reference for the task-space plan records (include/qmhip.h "planned task-space trajectories") built from what
pyoracle.Oracle offers — foot_pos_vel, frame_pose + front.mat_to_quat_xyzw, ee_pose_error against desired_state(t) — with masks, centre of pressure and the
foothold bracketing in numpy; the comparison with the bounds of the issue; the emulator binding (tests/emu_plan)."""
import ctypes as C
import os
import subprocess

import numpy as np

import front
from qm_control_amd import api, scenarios

_HERE = os.path.dirname(os.path.abspath(__file__))
ATOL_POS, ATOL_VEL = 1e-12, 1e-9      # DESIGN.md section 1 (front-end targets: pure kinematics) / section 4 (analytic Jacobians): positions, quaternion, CoP / foot_vel, ee_err


def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_plan"), "-s"])
    return C.CDLL(os.path.join(_HERE, "emu_plan", "_build", "libqm_emu_plan.so"))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def contact_mask(mode):
    """bit i = foot i (LF RF LH RH) in stance: modeNumber2StanceLeg of the mode id 8 LF + 4 RF + 2 LH + RH"""
    return sum(((int(mode) >> (3 - i)) & 1) << i for i in range(4))


def record(oracle, x, u, mode, ee=None, time=0.0):
    """one record of dtype api.PLAN_RECORD from the oracle's kinematics; ee = (pos, quat xyzw) or None"""
    r = np.zeros((), api.PLAN_RECORD); x = np.asarray(x, float); u = np.zeros(30) if u is None else np.asarray(u, float)
    r["time"] = time; r["mode"] = mode; m = contact_mask(mode); r["contact_mask"] = m; r["base_pos"] = x[6:9]; r["base_zyx"] = x[9:12]
    sx = sy = sz = 0.0
    for i in range(4):
        p, v = oracle.foot_pos_vel(x, u, i); r["foot_pos"][i] = p; r["foot_vel"][i] = v; r["foot_force"][i] = u[3 * i:3 * i + 3]
        if (m >> i) & 1:
            sx += u[3 * i + 2] * p[0]; sy += u[3 * i + 2] * p[1]; sz += u[3 * i + 2]
    p, R = oracle.frame_pose(x[6:30], 4); r["ee_pos"] = p; r["ee_quat"] = front.mat_to_quat_xyzw(R)
    if ee is not None:
        r["ee_err"] = oracle.ee_pose_error(x, ee[0], ee[1])
    r["cop"] = (sx / sz, sy / sz, sz) if sz > 0.0 else (0.0, 0.0, sz)
    return r


def plan(oracle, ref_t, ref_x, t, x, u, mode):
    """records of the n nodes (t, x, u, mode) of one instance; the end-effector reference of a node is the target trajectory (ref_t, ref_x) at the node's time"""
    oracle.set_target(ref_t, ref_x); n = len(t); out = np.zeros(n, api.PLAN_RECORD)
    for i in range(n):
        out[i] = record(oracle, x[i], u[i], mode[i], oracle.desired_state(t[i])[1:], t[i])
    return out


def footholds(oracle, t, x, ev, modes):
    """[(time, leg, event, pos)] ordered by (event, foot): events strictly inside (t[0], t[-1]), the state interpolated linearly in the bracket np.searchsorted(t, te, "left")
    finds, every foot that is off in modes[e] and on in modes[e + 1]"""
    out = []
    for e, te in enumerate(ev):
        if not (t[0] < te < t[-1]):
            continue
        land = ~contact_mask(modes[e]) & contact_mask(modes[e + 1]) & 15
        if not land:
            continue
        i = int(np.searchsorted(t, te, "left")); al = (t[i] - te) / (t[i] - t[i - 1]); xe = al * x[i - 1] + (1.0 - al) * x[i]
        for k in range(4):
            if (land >> k) & 1:
                out.append((te, k, e, oracle.foot_pos_vel(xe, np.zeros(30), k)[0]))
    return out


COPIED = ("time", "base_pos", "base_zyx", "foot_force")


def compare(got, ref, what=""):
    """asserts got == ref field by field with the bounds of the issue; returns the measured maxima {field: max abs difference}"""
    got = np.atleast_1d(got); ref = np.atleast_1d(ref); assert got.shape == ref.shape, (got.shape, ref.shape)
    for f in ("mode", "contact_mask"):
        assert np.array_equal(got[f], ref[f]), (what, f)
    for f in COPIED:
        assert np.array_equal(got[f], ref[f]), (what, f, np.abs(got[f] - ref[f]).max())
    assert not got["spare"].any(), what
    mx = {}
    for f, tol in (("foot_pos", ATOL_POS), ("ee_pos", ATOL_POS), ("ee_quat", ATOL_POS), ("foot_vel", ATOL_VEL), ("ee_err", ATOL_VEL)):
        mx[f] = float(np.abs(got[f] - ref[f]).max()); assert mx[f] <= tol, (what, f, mx[f])
    mx["cop_fz"] = float(np.abs(got["cop"][..., 2] - ref["cop"][..., 2]).max()); assert mx["cop_fz"] <= ATOL_POS, (what, mx)
    heavy = ref["cop"][..., 2] > 1.0; none = ref["cop"][..., 2] <= 0.0
    mx["cop_xy"] = float(np.abs(got["cop"][heavy][:, :2] - ref["cop"][heavy][:, :2]).max()) if heavy.any() else 0.0; assert mx["cop_xy"] <= ATOL_POS, (what, mx)
    assert not got["cop"][none][:, :2].any(), what
    return mx


def compare_footholds(fh, count, ref, cap, what=""):
    """fh [cap] of dtype api.FOOTHOLD and count of ONE instance against footholds(): count, leg, event, time equal; positions within ATOL_POS; slots behind the list untouched (zero)"""
    assert count == len(ref), (what, count, len(ref)); n = min(cap, len(ref)); mx = 0.0
    for s in range(n):
        te, k, e, p = ref[s]
        assert fh["leg"][s] == k and fh["event"][s] == e and fh["time"][s] == te, (what, s, fh[s], ref[s])
        mx = max(mx, float(np.abs(fh["pos"][s] - p).max()))
    assert mx <= ATOL_POS, (what, mx)
    assert not fh[n:].tobytes().strip(b"\0"), what
    return mx


def merge(a, b):
    return {k: max(a.get(k, 0.0), b.get(k, 0.0)) for k in set(a) | set(b)}


def random_states(blobs, R, seed):
    """R states sampled like scenarios.make_config("C5"): the initial state plus uniform offsets, the arm clipped inside its joint limits — and a random base attitude
    (roll, pitch, yaw all non-zero), random inputs, random modes (every one of the 16), random end-effector references"""
    mb, st = blobs; rng = np.random.default_rng(seed)
    x = np.tile(st[scenarios.ST_XINIT:scenarios.ST_XINIT + 30], (R, 1))
    x[:, 0:6] += rng.uniform(-0.1, 0.1, (R, 6)); x[:, 6:9] += rng.uniform(-0.5, 0.5, (R, 3)); x[:, 9] += rng.uniform(-3.0, 3.0, R); x[:, 10:12] += rng.uniform(-0.4, 0.4, (R, 2))
    x[:, 12:24] += rng.uniform(-0.1, 0.1, (R, 12)); x[:, 24:30] += rng.uniform(-0.2, 0.2, (R, 6))
    x[:, 24:30] = np.clip(x[:, 24:30], mb[scenarios.MB_QLO + 12:scenarios.MB_QLO + 18] + 0.05, mb[scenarios.MB_QHI + 12:scenarios.MB_QHI + 18] - 0.05)
    u = np.zeros((R, 30)); u[:, 0:12] = rng.uniform(-30.0, 120.0, (R, 12)); u[:, 12:30] = rng.uniform(-1.0, 1.0, (R, 18))
    mode = rng.integers(0, 16, R).astype(np.int32); mode[:16] = np.arange(16)
    ee = np.zeros((R, 7)); ee[:, :3] = scenarios.EE_NOMINAL_POS + rng.uniform(-0.3, 0.3, (R, 3)); q = rng.normal(size=(R, 4)); ee[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return x, u, mode, ee
