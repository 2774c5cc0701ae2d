"""tests/terrain_ref.py — TEST INFRASTRUCTURE of the plant's per-robot terrain (qmhip_sim_set_terrain / _get_ground / qmhip_terrain_eval; include/qmhip.h "plant terrain").

lookup(): the grid lookup restated in numpy, operation for operation.  TerrainRef: PushRef (tests/push_ref.py) with the contact block of its sub-step restated against the
tangent plane under every foot; M, nle, the foot Jacobian and the foot positions stay the oracle quantities PushRef.substep is built on.

EmuPlant / DevPlant: the same few calls on the host emulator (tests/emu_terrain) and on the device (api.QMHWSim), so that tests/test_terrain.py and tests/test_gpu_terrain.py
run the SAME checks (check_* below) with the same shapes and the same assertions."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import push_ref as pr
import sense_ref as sr
from conftest import rel_err
from push_ref import OK, ERR_ARG, ERR_STATE, TOL, STEPS, PERIOD, NSUB, T0, _p, _pi, _arr, _start, _ost
from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
NMAX = L.QM_TERRAIN_MAX
INF = float("inf")


# ---------------------------------------------------------------- the model in numpy
def _axis(x, x0, dx, n):
    s = (x - x0) / dx; c = bool(s < 0.0 or s > n - 1); s = min(max(s, 0.0), float(n - 1)); i = min(int(np.floor(s)), n - 2)
    return i, s - i, c


def lookup(t, x, y, mu_default):
    """(h, gx, gy, mu) of the terrain t = dict(hdr=(x0, y0, dx, dy), H=[ny][nx], MU=[ny][nx] or None) at (x, y) — qmhip.h, LOOKUP; t None: the plane"""
    if t is None:
        return 0.0, 0.0, 0.0, mu_default
    x0, y0, dx, dy = [np.float64(a) for a in t["hdr"]]; H = t["H"]; ny, nx = H.shape; i, u, cx = _axis(np.float64(x), x0, dx, nx); j, w, cy = _axis(np.float64(y), y0, dy, ny)
    bl = lambda A: (1.0 - w) * ((1.0 - u) * A[j, i] + u * A[j, i + 1]) + w * ((1.0 - u) * A[j + 1, i] + u * A[j + 1, i + 1])
    h00, h10, h01, h11 = H[j, i], H[j, i + 1], H[j + 1, i], H[j + 1, i + 1]
    gx = 0.0 if cx else ((1.0 - w) * (h10 - h00) + w * (h11 - h01)) / dx
    gy = 0.0 if cy else ((1.0 - u) * (h01 - h00) + u * (h11 - h10)) / dy
    return bl(H), gx, gy, (mu_default if t.get("MU") is None else bl(t["MU"]))


def plane_of(g, r, pz):
    """(n, pen) of the tangent plane g = (h, gx, gy, mu) against a sphere of radius r centred at height pz"""
    n = np.array([-g[1], -g[2], 1.0]) / np.sqrt(1.0 + g[1] * g[1] + g[2] * g[2])
    return n, r - (pz - g[0]) * n[2]


class TerrainRef(pr.PushRef):
    def feet(self, q):
        return [self.o.frame_pose(q, f)[0] for f in range(4)]

    def contact(self, q, t):
        return np.array([1 if plane_of(lookup(t, p[0], p[1], self.mu), self.r, p[2])[1] > 0.0 else 0 for p in self.feet(q)], np.int32)

    def substep(self, q, v, h, cmd, wrench, t=None):
        """PushRef.substep with the contact block of qmhip.h "plant terrain" (CONTACT); also returns the ground records [4][6]"""
        o = self.o; d = o.wbc(self.xinit, np.zeros(30), o.rbd_from_q(q, v), 15, 0.002, 20.0, debug=True)[2]; M, nle, J = d["M"], d["nle"], d["J"]
        tau = cmd["kp"] * (cmd["pos"] - q[6:]) + cmd["kd"] * (cmd["vel"] - v[6:]) + cmd["ff"]; tau = np.minimum(self.taumax, np.maximum(-self.taumax, tau))
        force = np.zeros(12); ground = np.zeros((4, 6))
        for f, p in enumerate(self.feet(q)):
            vf = J[3 * f:3 * f + 3] @ v; g = lookup(t, p[0], p[1], self.mu); n, pen = plane_of(g, self.r, p[2]); ground[f] = (g[0], n[0], n[1], n[2], g[3], pen)
            if pen > 0.0:
                vn = vf @ n; fn = max(0.0, self.k_n * pen - self.d_n * vn); vt = vf - vn * n
                force[3 * f:3 * f + 3] = fn * n - g[3] * fn * vt / np.sqrt(vt @ vt + self.v_eps * self.v_eps)
        rhs = np.concatenate([np.zeros(6), tau]) - nle + J.T @ force
        if wrench is not None:
            rhs[0:3] += wrench[0:3]
            if np.any(wrench[3:6] != 0.0):
                rhs[3:6] += self.euler_E(q).T @ wrench[3:6]
            if np.any(wrench[6:9] != 0.0):
                rhs += self.ee_jacobian(q).T @ wrench[6:9]
        a = np.linalg.solve(M, rhs)
        v = v + h * a; q = q + h * v
        return q, v, force, ground

    def run(self, case, p_b, steps, period, nsub, t0, t=None):
        q = np.array(case["q"], float); v = np.array(case["v"], float); ts, te = pr.substep_times(t0, period, nsub, steps); h = np.float64(period) / nsub; out = []
        for k in range(steps):
            for s in range(nsub):
                w, mask = pr.applied(p_b, ts[k, s]) if p_b is not None else (None, 0)
                q, v, force, ground = self.substep(q, v, h, case, w, t)
            out.append(dict(q=q.copy(), v=v.copy(), time=te[k], force=force, ground=ground, contact=self.contact(q, t), rbd=self.o.rbd_from_q(q, v)))
        return out


# ---------------------------------------------------------------- terrains
def terrain(hdr, H, MU=None):
    return dict(hdr=tuple(float(a) for a in hdr), H=np.array(H, float), MU=None if MU is None else np.array(MU, float))


def plane(xc, yc, half, sx, sy, MU=None):
    """2 x 2 grid of half-width `half` around (xc, yc): the plane of slopes (sx, sy) through height 0 at the centre"""
    H = np.array([[-sx - sy, sx - sy], [-sx + sy, sx + sy]]) * half
    return terrain((xc - half, yc - half, 2 * half, 2 * half), H, MU)


def saddle(xc, yc, half):
    return terrain((xc - half, yc - half, 2 * half, 2 * half), [[0.0, 0.1], [0.1, 0.0]])


def rough(xc, yc, nx, ny, dx, dy, amp, seed):
    rng = np.random.default_rng(seed)
    return terrain((xc - 0.5 * (nx - 1) * dx, yc - 0.5 * (ny - 1) * dy, dx, dy), amp * rng.uniform(-1.0, 1.0, (ny, nx)))


def pack(ts):
    """(hdr [B] of api.TERRAIN, height [B][ny][nx], mu or None) of terrains of one shape; an instance without MU among others with one carries the default 0.8"""
    hdr = np.zeros(len(ts), api.TERRAIN)
    for b, t in enumerate(ts):
        hdr["x0"][b], hdr["y0"][b], hdr["dx"][b], hdr["dy"][b] = t["hdr"]
    H = np.ascontiguousarray(np.stack([t["H"] for t in ts])); any_mu = any(t["MU"] is not None for t in ts)
    MU = np.ascontiguousarray(np.stack([t["MU"] if t["MU"] is not None else np.full(t["H"].shape, 0.8) for t in ts])) if any_mu else None
    return hdr, H, MU


# ---------------------------------------------------------------- the two plants
def emu_lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_terrain"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_terrain", "_build", "libqm_emu_terrain.so")); lib.emu_terrain_create.restype = C.c_void_p
    return lib


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _TerrainCalls:
    """what both plants share: the terrain calls in terms of _set_terrain / _get_ground / _eval"""

    def set_terrain(self, ts):
        if ts is None:
            return self._set_terrain(0, 0, 0, None, None, None)
        hdr, H, MU = pack(ts)
        return self._set_terrain(len(ts), H.shape[2], H.shape[1], hdr, H, MU)

    def set_terrain_raw(self, B, nx, ny, hdr, H, MU):
        return self._set_terrain(B, nx, ny, hdr, H, MU)

    def ground(self, B=None):
        B = self.B if B is None else B; g = np.full((max(B, 1), 4, 6), -1.0)
        return self._get_ground(B, g), g

    def terrain_eval(self, xy, B=None, n=None):
        xy = np.ascontiguousarray(xy, float); out = np.full(xy.shape[:2] + (4,), -1.0)
        return self._eval(xy.shape[0] if B is None else B, xy.shape[1] if n is None else n, xy, out), out

    def step_all(self, period, nsub):
        s = self.step(period, nsub); rc, g = self.ground(); assert rc == OK; s["ground"] = g
        return s


class EmuPlant(_TerrainCalls):
    """solver, WBC and plant in one emulator context (tests/emu_terrain/emu_terrain_api.cpp); the method names of api.QMHWSim where they exist"""

    def __init__(self, lib, blobs, Bmax, nev=2, nmax=8):
        self.lib = lib; self.mb = np.ascontiguousarray(blobs[0], float); self.st = np.ascontiguousarray(blobs[1], float); self.Bmax = Bmax; self.B = Bmax
        self.h = C.c_void_p(lib.emu_terrain_create(_p(self.mb), _p(self.st), Bmax, nmax, 2, nev))

    def close(self):
        if self.h:
            self.lib.emu_terrain_destroy(self.h); self.h = None

    def upload(self, c, B):
        a = lambda k, t=float: np.ascontiguousarray(c[k][:B], t)
        self.lib.emu_terrain_upload(self.h, B, _p(a("t0")), _p(a("x0")), _p(a("ref_t")), _p(a("ref_x")), _p(a("ev")), _pi(a("modes", np.int32)))

    def reset(self, q, v, time):
        q = np.ascontiguousarray(q, float); self.B = B = q.shape[0]; v = np.ascontiguousarray(v, float); t = np.ascontiguousarray(np.broadcast_to(time, (B,)), float)
        self.lib.emu_terrain_sim_reset(self.h, B, _p(q), _p(v), _p(t))

    def command(self, pos, vel, kp, kd, ff):
        cmd = np.ascontiguousarray(np.concatenate([pr._bcast(x, self.B) for x in (pos, vel, kp, kd, ff)], axis=1)); self.lib.emu_terrain_sim_command(self.h, self.B, _p(cmd))

    def state(self):
        B = self.B; d = dict(q=np.zeros((B, 24)), v=np.zeros((B, 24)), time=np.zeros(B), rbd=np.zeros((B, 55)), contact=np.zeros((B, 4), np.int32), force=np.zeros((B, 12)), status=np.zeros(B, np.int32),
                             qp_status=np.zeros((B, 3), np.int32), mpc_status=np.zeros(B, np.int32))
        self.lib.emu_terrain_readback(self.h, B, _p(d["q"]), _p(d["v"]), _p(d["time"]), _p(d["rbd"]), _pi(d["contact"]), _p(d["force"]), _pi(d["status"]), _pi(d["qp_status"]), _pi(d["mpc_status"]))
        return d

    def step(self, period, nsub):
        self.lib.emu_terrain_sim_step(self.h, self.B, C.c_double(period), nsub)
        return self.state()

    def closed_loop(self, n, period, horizon, nsub, mpc_every, pipelined=False):
        self.lib.emu_terrain_closed_loop(self.h, self.B, n, C.c_double(period), nsub, mpc_every, C.c_double(horizon), C.c_double(0.0), C.c_double(0.5), int(pipelined))
        return self.state()

    def set_pushes(self, p):
        if p is None:
            return self.lib.emu_terrain_set_pushes(self.h, 0, 0, None)
        B, K, ptr, _keep = pr._push_arg(p)
        return self.lib.emu_terrain_set_pushes(self.h, B, K, ptr)

    def set_sensors(self, s):
        if s is None:
            return self.lib.emu_terrain_set_sensors(self.h, 0, None)
        B, ptr, _keep = sr._rec_arg(s)
        return self.lib.emu_terrain_set_sensors(self.h, B, ptr)

    def _set_terrain(self, B, nx, ny, hdr, H, MU):
        return self.lib.emu_terrain_set_terrain(self.h, B, nx, ny, _vp(hdr), _p(H), _p(MU))

    def _get_ground(self, B, g):
        return self.lib.emu_terrain_get_ground(self.h, B, _p(g))

    def _eval(self, B, n, xy, out):
        return self.lib.emu_terrain_eval(self.h, B, n, _p(xy), _p(out))

    def set_wbc_only(self, on):
        self.lib.emu_terrain_set_wbc_only(self.h, int(on))

    def launches(self):
        """(plain, push, terrain, terrain + push) launches of the plant kernel's four instances"""
        n = (C.c_int * 5)(); self.lib.emu_terrain_counts(self.h, n)
        return tuple(n[:4])

    def allocated(self):
        return bool(self.lib.emu_terrain_allocated(self.h))


class DevPlant(sr.DevPlant, _TerrainCalls):
    """the same calls through the C ABI on the device"""

    def _set_terrain(self, B, nx, ny, hdr, H, MU):
        return self.itf.lib.qmhip_sim_set_terrain(self._h(), B, nx, ny, _vp(hdr), _p(H), _p(MU))

    def _get_ground(self, B, g):
        return self.itf.lib.qmhip_sim_get_ground(self._h(), B, _p(g))

    def _eval(self, B, n, xy, out):
        return self.itf.lib.qmhip_terrain_eval(self._h(), B, n, _p(xy), _p(out))


# ---------------------------------------------------------------- (1) lookup, exact at the edges
def lookup_grids():
    """two calls of B = 2: the 2 x 2 saddle beside a 2 x 2 grid off the binary raster, and two 3 x 16 grids (ny = 3, nx = 16) whose neighbouring cells differ in slope by
    more than 0.1 in both directions and whose edge cells slope by more than 0.1 — a neighbouring cell picked or a clamp missed moves gx / gy by at least 0.1"""
    rng = np.random.default_rng(5)
    sad = saddle(0.125, -0.25, 0.125); sad["MU"] = np.array([[0.3, 0.9], [0.6, 0.4]])
    odd = terrain((-0.77, 0.31, 0.3, 0.7), [[1.0, 1.2], [0.7, 1.3]], [[0.5, 0.2], [1.0, 0.8]])
    out = [[sad, odd]]; wide = []
    for hdr in ((-0.75, -0.125, 0.125, 0.125), (0.13, -1.7, 0.1, 0.3)):
        nx, ny = 16, 3; dx, dy = hdr[2], hdr[3]; i = np.arange(nx - 1); sx = np.array([(-1.0) ** i * (0.3 + 0.05 * i + 0.2 * j) for j in range(ny)])      # [ny][nx - 1] slopes along x
        c = 1.0 + np.array([0.0, 0.48, 0.08]) * dy; H = c[:, None] + np.concatenate([np.zeros((ny, 1)), np.cumsum(sx * dx, axis=1)], axis=1)
        wide.append(terrain(hdr, H, rng.uniform(0.2, 1.0, (ny, nx))))
    out.append(wide)
    for group in out:
        for t in group:
            H = t["H"]; gx = np.diff(H, axis=1) / t["hdr"][2]; gy = np.diff(H, axis=0) / t["hdr"][3]
            assert np.abs(gx[:, [0, -1]]).min() >= 0.1 and np.abs(gy[[0, -1]]).min() >= 0.1
            assert gx.shape[1] == 1 or np.abs(np.diff(gx, axis=1)).min() >= 0.1
            assert gy.shape[0] == 1 or np.abs(np.diff(gy, axis=0)).min() >= 0.1
    return out


def lookup_points(t):
    """24 points in grid coordinates turned into world coordinates: vertices, points on grid lines, both neighbours of a line, the last vertex and its neighbour beyond,
    points outside on each side and at a corner"""
    x0, y0, dx, dy = t["hdr"]; ny, nx = t["H"].shape; X = lambda s: x0 + s * dx; Y = lambda s: y0 + s * dy; m = min(7, nx - 1); my = min(1, ny - 1); up = np.nextafter
    return np.array([
        (X(0), Y(0)), (X(nx - 1), Y(ny - 1)), (X(m), Y(my)), (X(0), Y(ny - 1)),                                                  # vertices
        (X(m), Y(0.3)), (X(0.4), Y(my)), (X(m - 0.6), Y(my)),                                                                   # on grid lines
        (up(X(m), -INF), Y(0.3)), (up(X(m), INF), Y(0.3)), (X(0.7), up(Y(my), -INF)), (X(0.7), up(Y(my), INF)),                  # both sides of a line
        (X(nx - 1), Y(0.25)), (up(X(nx - 1), INF), Y(0.25)), (X(0.25), Y(ny - 1)), (X(0.25), up(Y(ny - 1), INF)),                # s == nx - 1 and beyond
        (up(X(0), -INF), Y(0.8)), (X(0.2), up(Y(0), -INF)),                                                                     # just outside the first line
        (X(-1.5), Y(0.2)), (X(nx + 0.5), Y(ny - 1.2)), (X(0.8), Y(-2.0)), (X(nx - 1.8), Y(ny + 3.0)),                            # outside on each side
        (X(-0.5), Y(ny + 0.5)), (X(nx + 2.0), Y(-0.1)),                                                                         # outside at two corners
        (X(0.37), Y(0.81))])                                                                                                    # inside a cell


def check_lookup(make, what):
    for group in lookup_grids():
        p = make(2); assert p.set_terrain(group) == OK
        xy = np.stack([lookup_points(t) for t in group]); assert xy.shape == (2, 24, 2)
        rc, out = p.terrain_eval(xy); assert rc == OK
        want = np.array([[lookup(t, x, y, 0.8) for x, y in xy[b]] for b, t in enumerate(group)])
        err = np.abs(out - want); assert (err <= 1e-14 * np.abs(want)).all(), (what, np.argwhere(err > 1e-14 * np.abs(want)), out[err > 1e-14 * np.abs(want)], want[err > 1e-14 * np.abs(want)])
        assert (want[:, 17:21, 1:3] == 0.0).any(axis=2).all() and (want[:, 21:23, 1:3] == 0.0).all()      # the clamps were exercised
        # mu = NULL: the global coefficient; an instance beyond the terrain's B: the plane
        assert p.set_terrain_raw(1, *group[0]["H"].shape[::-1], *pack(group[:1])[:2], None) == OK
        rc, bare = p.terrain_eval(xy); assert rc == OK and (bare[0, :, 3] == 0.8).all() and np.array_equal(bare[0, :, :3], out[0, :, :3]) and np.array_equal(bare[1], np.tile([0.0, 0.0, 0.0, 0.8], (24, 1)))
        p.close()


# ---------------------------------------------------------------- (2) plant vs reference
# the grids are raised until the deepest foot of the start state stands PEN0 in the ground (the cases' own clearances are -6 .. +4 mm on the plane)
PEN0 = 0.006
GROUPS = ((0, 1, 3), (2, 4), (5,))      # instances of one grid shape share a call: 2 x 2, 8 x 8, 3 x 16


def settle(ref, case, t, pen0=PEN0):
    deepest = -INF
    for p in ref.feet(np.array(case["q"], float)):
        n, pen = plane_of(lookup(t, p[0], p[1], ref.mu), ref.r, p[2]); deepest = max(deepest, pen / n[2])      # (a vertical shift by d moves pen by d n_z)
    t["H"] = t["H"] + (pen0 - deepest)
    return t


def plant_terrains(ref, cases):
    """slope 0.2 in x; slope 0.2 in y with mu = 0.2; a random rough 8 x 8 grid (+-15 mm, 0.15 m cells); the 2 x 2 saddle; an 8 x 8 grid that ends between the front and
    the hind feet (the hind feet stand outside it, on its clamped edge); a 3 x 16 grid (ny = 3, nx = 16) of +-10 mm"""
    xy = [np.array(c["q"][:2], float) for c in cases]; fx = [np.array([p[0] for p in ref.feet(np.array(c["q"], float))]) for c in cases]
    ts = [plane(xy[0][0], xy[0][1], 1.0, 0.2, 0.0), plane(xy[1][0], xy[1][1], 1.0, 0.0, 0.2, np.full((2, 2), 0.2)), rough(xy[2][0], xy[2][1], 8, 8, 0.15, 0.15, 0.015, 21),
          saddle(xy[3][0], xy[3][1], 0.5), None, None]
    x_edge = 0.5 * (np.sort(fx[4])[1] + np.sort(fx[4])[2]); rng = np.random.default_rng(22); i = np.arange(8)
    ts[4] = terrain((x_edge, xy[4][1] - 0.525, 0.1, 0.15), -0.02 * 0.1 * i[None, :] + 0.015 * (i[None, :] == 0) + 0.004 * rng.uniform(-1.0, 1.0, (8, 8)))      # (a kerb of 15 mm at the edge: this case carries its hind feet high)
    ts[5] = rough(xy[5][0], xy[5][1], 16, 3, 0.08, 0.4, 0.010, 23)
    assert (fx[4] < x_edge).sum() == 2
    return [settle(ref, c, t) for c, t in zip(cases, ts)]


def plant_pushes():
    """a base force over steps 2-8 and a permanent base torque (no end-effector force: its Jacobian in PushRef is a finite difference, whose 1e-10 would be the largest
    error of this comparison)"""
    p = pr.pushes(1, 2); pr.slot(p, 0, 0, T0 + 0.002, T0 + 0.009, base_force=(40.0, -30.0, 10.0)); pr.slot(p, 0, 1, -INF, INF, base_torque=(4.0, -6.0, 3.0))
    return p


@functools.lru_cache(maxsize=None)
def _reference_runs_cached(oracle):
    import pyoracle
    omb, ost = pyoracle.load_blobs(); ref = TerrainRef(oracle, omb, ost); cases = pr.plant_cases(oracle, ost); ts = plant_terrains(ref, cases); p = plant_pushes()
    on = [ref.run(c, p[0] if b == 5 else None, STEPS, PERIOD, NSUB, T0, ts[b]) for b, c in enumerate(cases)]
    flat = [ref.run(c, p[0] if b == 5 else None, STEPS, PERIOD, NSUB, T0, None) for b, c in enumerate(cases)]
    return cases, ts, p, on, flat


def reference_runs(oracle):
    """(cases, terrains, the push schedule of instance 5, reference runs on the terrain [6][STEPS], on the plane) — computed once per session"""
    return _reference_runs_cached(oracle)


def ground_err(got, want, r):
    """largest relative difference of ground records [4][6].  h, n and mu as they stand; pen = r - (p_z - h) n_z is a difference of two numbers of the size of the foot
    radius that passes through zero at every touchdown, so it is compared in the form without the cancellation, (p_z - h) n_z = r - pen: the same number, relative to the
    operands it was rounded at"""
    got = np.array(got, float); want = np.array(want, float); got[:, 5] = r - got[:, 5]; want[:, 5] = r - want[:, 5]
    e = np.abs(got - want) / np.maximum(np.abs(want), 1e-300); e[got == want] = 0.0
    return e.max()


def check_plant_vs_reference(make, oracle, what):
    cases, ts, p, on, flat = reference_runs(oracle); ref_radius = 0.02      # (QmSimParams::foot_radius, PushRef's default)
    for b in range(6):      # the conditions, on the CPU: somebody stands on the ground on every step, and the ground matters three decades above the tolerances
        assert all(r["contact"].any() for r in on[b]), b
        eq, ev = rel_err(on[b][-1]["q"], flat[b][-1]["q"]), rel_err(on[b][-1]["v"], flat[b][-1]["v"]); print("%s: reference on its terrain vs on the plane, instance %d: q %.2e v %.2e" % (what, b, eq, ev))
        assert eq >= 1e3 * TOL["q"] and ev >= 1e3 * TOL["v"], (b, eq, ev)
    worst = dict(q=0.0, v=0.0, force=0.0, rbd=0.0, time=0.0, ground=0.0)
    for group in GROUPS:
        plant = make(len(group)); sub = [cases[b] for b in group]
        assert plant.set_terrain([ts[b] for b in group]) == OK and plant.set_pushes(p if group == (5,) else None) == OK; _start(plant, sub)
        rc, g = plant.ground(); assert rc == OK and not g.any()      # zeros after a reset
        for k in range(STEPS):
            s = plant.step_all(PERIOD, NSUB)
            for i, b in enumerate(group):
                r = on[b][k]; e = dict(q=rel_err(s["q"][i], r["q"]), v=rel_err(s["v"][i], r["v"]), force=rel_err(s["force"][i], r["force"]), rbd=rel_err(s["rbd"][i], r["rbd"]), time=abs(s["time"][i] - r["time"]))
                e["ground"] = ground_err(s["ground"][i], r["ground"], ref_radius)
                worst = {n: max(worst[n], e[n]) for n in e}
                assert s["status"][i] == 0 and all(e[n] < TOL[n] for n in TOL) and e["ground"] <= 1e-12, (b, k, e)
                assert list(s["contact"][i]) == list(r["contact"]), (b, k)
        if hasattr(plant, "launches"):
            assert plant.launches() == ((0, 0, 0, STEPS + 1) if group == (5,) else (0, 0, STEPS + 1, 0))
        plant.close()
    print("%s vs terrain_ref, worst over 6 instances x %d steps: %s" % (what, STEPS, {n: "%.1e" % x for n, x in worst.items()}))


# ---------------------------------------------------------------- (3) independent properties, from the plant's own output
def _run(plant, cases, ts, steps=6, shift=None, keep=False):
    assert plant.set_terrain(ts) == OK; q = _arr(cases, "q").copy()
    if shift is not None:
        q[:, :3] += shift
    plant.reset(q, _arr(cases, "v"), T0); plant.command(*[_arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); out = []
    for _ in range(steps):
        s = plant.step_all(PERIOD, NSUB); out.append(s)
    return out if keep else s


def _close(a, b, shift, what):
    """b reproduces a moved by `shift`: q, v and force within the plant's tolerances"""
    for i in range(len(a["q"])):
        qa = a["q"][i].copy(); qa[:3] += shift
        e = dict(q=rel_err(b["q"][i], qa), v=rel_err(b["v"][i], a["v"][i]), force=rel_err(b["force"][i], a["force"][i]))
        assert all(e[n] < TOL[n] for n in e) and list(a["contact"][i]) == list(b["contact"][i]), (what, i, e)


def check_properties(make, oracle):
    import pyoracle
    omb, ost = pyoracle.load_blobs(); ref = TerrainRef(oracle, omb, ost); cases = pr.plant_cases(oracle, ost)[:2]; xy = [np.array(c["q"][:2], float) for c in cases]
    # a constant height c under a pose lifted by c is the plane
    c = 0.37; p = make(2); flat = _run(p, cases, None); p.close()
    p = make(2); up = _run(p, cases, [terrain((xy[b][0] - 1.0, xy[b][1] - 1.0, 0.5, 0.5), np.full((5, 5), c)) for b in range(2)], shift=np.array([0.0, 0.0, c])); p.close()
    assert flat["force"].any(); _close(flat, up, np.array([0.0, 0.0, c]), "lifted")
    # grid and robot moved together in x, y
    ts = [settle(ref, cases[b], rough(xy[b][0], xy[b][1], 8, 8, 0.15, 0.15, 0.015, 31 + b)) for b in range(2)]; d = np.array([1.3, -0.7, 0.0])
    moved = [terrain((t["hdr"][0] + d[0], t["hdr"][1] + d[1], t["hdr"][2], t["hdr"][3]), t["H"]) for t in ts]
    p = make(2); here = _run(p, cases, ts); p.close(); p = make(2); there = _run(p, cases, moved, shift=d); p.close()
    assert here["force"].any() and rel_err(here["q"], flat["q"]) > 1e3 * TOL["q"]; _close(here, there, d, "moved")
    # without friction every contact force is along the ground's normal; with it, inside the cone
    slopes = [settle(ref, cases[0], plane(xy[0][0], xy[0][1], 1.0, 0.2, -0.1)), settle(ref, cases[1], saddle(xy[1][0], xy[1][1], 0.5))]; seen = [0, 0]
    for k, mu in enumerate((0.0, 0.6)):
        for t in slopes:
            t["MU"] = np.full(t["H"].shape, mu)
        p = make(2)
        for s in _run(p, cases, slopes, keep=True):
            for b in range(2):
                for f in range(4):
                    fo = s["force"][b, 3 * f:3 * f + 3]; g = s["ground"][b, f]; n = g[1:4]
                    if not fo.any():
                        continue
                    seen[k] += 1; fn = fo @ n; ft = fo - fn * n; assert g[5] > 0.0 and abs(g[4] - mu) <= 1e-15 and abs(n @ n - 1.0) < 1e-14 and (b == 1 or abs(n[0]) > 0.15)      # (instance 0 stands on a slope of 0.2)
                    if mu == 0.0:
                        assert np.linalg.norm(np.cross(fo, n)) <= 1e-12 * np.linalg.norm(fo), (b, f, fo, n)
                    else:
                        assert np.linalg.norm(ft) < g[4] * fn, (b, f, fo, n)
        p.close()
    assert min(seen) >= 12, seen


# ---------------------------------------------------------------- (4) flat, isolation, off
def _same(a, b, rows=slice(None)):
    return all(np.array_equal(a[n][rows], b[n][rows]) for n in ("q", "v", "rbd", "force", "contact"))


def check_flat_isolation_off(make, oracle, what):
    import pyoracle
    omb, ost = pyoracle.load_blobs(); ref = TerrainRef(oracle, omb, ost); cases = pr.plant_cases(oracle, ost)[:3]; B = 3; xy = [np.array(c["q"][:2], float) for c in cases]
    zero = lambda b: terrain((xy[b][0] - 1.0, xy[b][1] - 1.0, 0.25, 0.25), np.zeros((8, 8)))
    bump = lambda b, seed: settle(ref, cases[b], rough(xy[b][0], xy[b][1], 8, 8, 0.15, 0.15, 0.015, seed))
    # a flat grid without a friction grid against the plain kernel: two compilations of one body, within the plant's tolerances and with equal contact flags
    never = make(B); s_never = _run(never, cases, None); fl = make(B); s_flat = _run(fl, cases, [zero(b) for b in range(B)])
    e = {n: max(rel_err(s_flat[n][i], s_never[n][i]) for i in range(B)) for n in ("q", "v", "force", "rbd")}
    print("%s: terrain kernel on a flat grid vs plain kernel, largest relative difference after 6 steps: %s" % (what, {n: "%.1e" % x for n, x in e.items()}))
    assert all(e[n] < TOL[n] for n in e) and np.array_equal(s_flat["contact"], s_never["contact"]) and s_never["force"].any(), e
    assert np.array_equal(s_flat["ground"][:, :, :5], np.tile([0.0, 0.0, 0.0, 1.0, 0.8], (B, 4, 1))) and not s_never["ground"].any()
    # robot 0's grid changes: robot 1 and 2 keep their bits
    a = make(B); sa = _run(a, cases, [bump(0, 41), bump(1, 42), zero(2)]); b = make(B); sb = _run(b, cases, [bump(0, 43), bump(1, 42), zero(2)])
    assert _same(sa, sb, slice(1, 3)) and not _same(sa, sb, 0) and np.array_equal(sa["ground"][1:], sb["ground"][1:])
    # a terrain that covers fewer robots than the step: the rest stand like robots on a flat grid, bit for bit
    c = make(B); sc = _run(c, cases, [bump(0, 41)]); assert _same(sc, sa, 0) and _same(sc, s_flat, slice(1, 3)) and np.array_equal(sc["ground"][1:], s_flat["ground"][1:])
    # with a schedule of pushes the fourth instance runs; without an active slot it agrees with the third within the tolerances
    assert c.set_pushes(pr.pushes(B, 1)) == OK; sp = _run(c, cases, [bump(0, 41)]); assert c.set_pushes(None) == OK
    assert all(rel_err(sp[n], sc[n]) < TOL[n] for n in ("q", "v", "force", "rbd")) and np.array_equal(sp["contact"], sc["contact"])
    # terrain off again: equal to a context that never had one, bit for bit (both run the plain kernel), the ground records zero
    s_off = _run(c, cases, None); assert _same(s_off, s_never) and np.array_equal(s_off["time"], s_never["time"]) and not s_off["ground"].any()
    assert c.terrain_eval(np.zeros((B, 1, 2)))[0] == ERR_STATE
    if hasattr(c, "launches"):      # (plain, push, terrain, terrain + push): the reset's hand-over and six steps each
        assert never.launches() == (7, 0, 0, 0) and fl.launches() == (0, 0, 7, 0) and a.launches() == (0, 0, 7, 0) and c.launches() == (7, 0, 7, 7), (never.launches(), fl.launches(), c.launches())
        assert not never.allocated() and fl.allocated()      # the grids are allocated by the first set_terrain, not with the plant
    for x in (never, fl, a, b, c):
        x.close()


# ---------------------------------------------------------------- (5) error codes
def check_errors(make, oracle):
    """every refused call returns its code and leaves the terrain untouched — the next steps equal the steps of an identical context bit for bit"""
    import pyoracle
    omb, ost = pyoracle.load_blobs(); ref = TerrainRef(oracle, omb, ost); cases = pr.plant_cases(oracle, ost)[:2]; B = 2; xy = [np.array(c["q"][:2], float) for c in cases]
    good = [settle(ref, cases[b], rough(xy[b][0], xy[b][1], 4, 3, 0.3, 0.4, 0.01, 51 + b)) for b in range(B)]
    for t in good:
        t["MU"] = np.full(t["H"].shape, 0.5)
    a = make(B); twin = make(B)
    assert a.terrain_eval(np.zeros((B, 1, 2)))[0] == ERR_STATE      # no terrain yet
    assert a.set_terrain(good) == OK and twin.set_terrain(good) == OK      # before the first reset: allocated on demand
    _start(a, cases); _start(twin, cases)
    hdr, H, MU = pack(good); other = np.full_like(H, 0.05); bad = []
    for field, val in (("x0", np.nan), ("y0", INF), ("dx", 0.0), ("dx", -0.1), ("dy", 0.0), ("dy", np.nan), ("dx", INF)):
        h2 = hdr.copy(); h2[field][1] = val; bad.append((B, 4, 3, h2, other, MU))
    for val in (np.nan, INF, -INF):
        H2 = other.copy(); H2[1, 2, 3] = val; bad.append((B, 4, 3, hdr, H2, MU))
    for val in (np.nan, INF, -0.1):
        M2 = MU.copy(); M2[1, 0, 1] = val; bad.append((B, 4, 3, hdr, other, M2))
    big = np.zeros((B, NMAX + 1, NMAX + 1))
    bad += [(0, 4, 3, hdr, other, MU), (-1, 4, 3, hdr, other, MU), (B + 1, 4, 3, np.zeros(B + 1, api.TERRAIN), np.zeros((B + 1, 3, 4)), None), (B, 1, 3, hdr, other, MU), (B, 4, 1, hdr, other, MU),
            (B, NMAX + 1, 3, hdr, big, None), (B, 4, NMAX + 1, hdr, big, None), (B, 0, 0, hdr, other, MU)]
    for k, args in enumerate(bad):
        assert a.set_terrain_raw(*args) == ERR_ARG, k
    assert a.ground(0)[0] == ERR_ARG and a.ground(B + 1)[0] == ERR_ARG and a.terrain_eval(np.zeros((B, 1, 2)), B=B + 1)[0] == ERR_ARG and a.terrain_eval(np.zeros((B, 1, 2)), n=0)[0] == ERR_ARG
    a.set_wbc_only(True)
    assert a.set_terrain_raw(B, 4, 3, hdr, other, MU) == ERR_STATE and a.set_terrain(None) == ERR_STATE and a.ground()[0] == ERR_STATE and a.terrain_eval(np.zeros((B, 1, 2)))[0] == ERR_STATE
    a.set_wbc_only(False)
    for _ in range(3):
        sa = a.step_all(PERIOD, NSUB); st = twin.step_all(PERIOD, NSUB)
        assert _same(sa, st) and np.array_equal(sa["ground"], st["ground"]) and sa["force"].any()
    assert (np.abs(sa["ground"][:, :, 4] - 0.5) <= 1e-15).all()      # (a blend of four equal values may round in the last place)
    # the terrain persists across a reset, the ground records start over
    a.reset(_arr(cases, "q"), _arr(cases, "v"), T0); rc, g = a.ground(); assert rc == OK and not g.any()
    a.command(*[_arr(cases, k) for k in ("pos", "vel", "kp", "kd", "ff")]); s = a.step_all(PERIOD, NSUB); assert (np.abs(s["ground"][:, :, 4] - 0.5) <= 1e-15).all()
    a.close(); twin.close()


# ---------------------------------------------------------------- (6) the loops: B = 2, 20 ticks, an MPC call every 5
N_TICKS, EVERY = 20, 5


def loop_setup():
    from test_push import loop_setup as setup
    return setup()


def loop_terrain(q0, flat=False):
    """robot 0 on a flat grid, friction 0.8; robot 1 on a rough 8 x 8 grid of +-8 mm with zero mean, 0.15 m cells, friction 0.6 (flat: the same friction on flat grids)"""
    ts = [terrain((q0[b][0] - 1.0, q0[b][1] - 1.0, 2.0, 2.0), np.zeros((8, 8)), np.full((8, 8), (0.8, 0.6)[b])) for b in range(2)]
    if not flat:
        t = rough(q0[1][0], q0[1][1], 8, 8, 0.15, 0.15, 0.008, 61); t["H"] -= t["H"].mean(); t["MU"] = ts[1]["MU"]; ts[1] = t
    return ts


def loop_pushes(t_start):
    ts, _ = pr.substep_times(t_start, PERIOD, NSUB, N_TICKS); p = pr.pushes(2, 1); pr.slot(p, 1, 0, ts[3, 0], ts[12, 0], base_force=(0.0, 30.0, 0.0))
    return p


def run_loop(plant, q0, t_start, ts, pipelined, pushes=None, sensors=None):
    """20 ticks, the status words checked behind every call (one tick each; the pipelined loop in chunks of mpc_every)"""
    assert plant.set_terrain(ts) == OK and plant.set_pushes(pushes) == OK and plant.set_sensors(sensors) == OK; plant.reset(q0, np.zeros((2, 24)), t_start); chunk = EVERY if pipelined else 1
    for _ in range(N_TICKS // chunk):
        s = plant.closed_loop(chunk, PERIOD, _horizon(), NSUB, EVERY, pipelined=pipelined)
        assert (np.asarray(s["mpc_status"]) == 0).all() and (np.asarray(s["qp_status"]) == 0).all() and (s["status"] == 0).all(), (s["mpc_status"], s["qp_status"])
    rc, g = plant.ground(); assert rc == OK; s["ground"] = g
    return s


def _horizon():
    from test_push import HORIZON
    return HORIZON


def check_loop(make, pipelined, what):
    c, q0, t_start = loop_setup()
    a = make(c); sa = run_loop(a, q0, t_start, loop_terrain(q0), pipelined, loop_pushes(t_start)); a.close()
    b = make(c); sb = run_loop(b, q0, t_start, loop_terrain(q0, flat=True), pipelined, loop_pushes(t_start)); b.close()
    assert all(np.array_equal(sa[n][0], sb[n][0]) for n in ("q", "v", "rbd", "force"))      # the neighbour's ground does not reach instance 0
    e = rel_err(sa["q"][1], sb["q"][1]); print("%s: rough vs flat ground, q after %d ticks: %.2e" % (what, N_TICKS, e)); assert e > 1e-4
    assert (np.abs(sa["ground"][1, :, 4] - 0.6) <= 1e-15).all() and sa["ground"][1, :, 0].any() and not sb["ground"][:, :, 0].any()
