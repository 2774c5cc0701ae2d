"""tests/offnominal_cases.py — TEST INFRASTRUCTURE: problems away from the nominal pose, shared by the CPU and GPU tests (test_offnominal.py, test_gpu_offnominal.py).

Every other comparison with the oracle starts within +-0.02 m of the origin and about +-0.1 rad of zero attitude, where the rotation matrices are near identity, the
Euler-rate map loses most of its terms and world- and base-frame quantities almost coincide.  The movers here take a problem the suite already uses and put it somewhere
else: a rotation by psi about the world's z axis plus a translation d in the ground plane (a symmetry of the model: momenta, positions and contact forces turn with
Rz(psi), the yaw angle gets + psi) and, on top of that, a pitch and a roll added to the base attitude (no symmetry: a different problem).  With psi = 0, d = 0,
pitch = roll = 0 they return the inputs they were given, bit for bit (test_offnominal.py asserts it once)."""
import copy
import numpy as np

# (yaw, pitch, roll) of the base; the base stands at BASE_XY.  Headings in all four quadrants, one almost exactly pi, one beyond a full turn.
POSES = [(2.5, 0.3, -0.25), (-3.1, -0.4, 0.3), (3.14159, 0.5, 0.5), (7.0, 0.3, 0.2), (-1.6, 0.45, -0.4), (0.8, -0.5, 0.1), (4.0, 0.2, 0.2), (-2.0, 0.1, -0.5)]
BASE_XY = (40.0, -25.0)

# all 16 contact modes in one schedule: stance, then one foot after the other leaves and comes back (Gray-code-like steps through 3-, 2-, 1- and 0-leg support)
ALL_MODES = [15, 7, 3, 1, 0, 8, 12, 14, 6, 2, 10, 11, 9, 13, 5, 4, 15]

WBC_MODES = (15, 9, 6, 7, 14, 3, 12, 15)      # stance, the trot phases, three- and two-leg support on either side
WBC_SEED, WBC_HARD_SEED, PLANT_SEED = 61, 161, 7      # (+ variant for the WBC; the oracle alone ends every one of these cases with status [0, 0, 0])


def Rz(psi):
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def Gx(psi):
    """how the centroidal state (30) turns: linear and angular momentum and the base position with Rz; Euler angles and joints stay (yaw is shifted, not turned)"""
    G = np.eye(30)
    for k in (0, 3, 6):
        G[k:k + 3, k:k + 3] = Rz(psi)
    return G


def Gu(psi):
    """how the input (30) turns: the four contact forces with Rz; joint velocities stay"""
    G = np.eye(30)
    for k in (0, 3, 6, 9):
        G[k:k + 3, k:k + 3] = Rz(psi)
    return G


def Gc(mode, psi):
    """how the equality rows of a contact mode turn (rows per foot LF, RF, LH, RH: stance = zero velocity (3); swing = zero force (3) + normal velocity (1)):
    every three-row group with Rz, a swing leg's single normal-velocity row stays"""
    blocks = []
    for i in range(4):
        blocks.append(Rz(psi))
        if not (mode >> (3 - i)) & 1:
            blocks.append(np.eye(1))
    n = sum(b.shape[0] for b in blocks); G = np.zeros((n, n)); o = 0
    for b in blocks:
        G[o:o + b.shape[0], o:o + b.shape[0]] = b; o += b.shape[0]
    return G


def _shift3(d):
    return np.array([d[0], d[1], 0.0])


def move_state(x, psi, d, pitch, roll):
    """centroidal state (30) or target knot (37: + end-effector position and quaternion, the position moved with the base)"""
    x = np.array(x, float); R = Rz(psi)
    x[0:3] = R @ x[0:3]; x[3:6] = R @ x[3:6]; x[6:9] = R @ x[6:9] + _shift3(d)
    x[9] += psi; x[10] += pitch; x[11] += roll
    if x.shape[0] == 37:
        x[30:33] = R @ x[30:33] + _shift3(d)
    return x


def move_input(u, psi):
    u = np.array(u, float); R = Rz(psi)
    for k in (0, 3, 6, 9):
        u[k:k + 3] = R @ u[k:k + 3]
    return u


def move_problem(cfg, b, psi, d=(0.0, 0.0), pitch=0.0, roll=0.0):
    """instance b of a scenarios config, in place: x0 and both target knots"""
    cfg["x0"][b] = move_state(cfg["x0"][b], psi, d, pitch, roll)
    for k in range(cfg["ref_x"].shape[1]):
        cfg["ref_x"][b, k] = move_state(cfg["ref_x"][b, k], psi, d, pitch, roll)
    return cfg


def move_plant_state(q, v, psi, d=(0.0, 0.0), pitch=0.0, roll=0.0):
    """generalised coordinates of the plant and of the WBC's measured state: q = [base position, Euler zyx, joints], v = dq/dt (Euler RATES: they do not turn)"""
    q = np.array(q, float); v = np.array(v, float); R = Rz(psi)
    q[0:3] = R @ q[0:3] + _shift3(d); q[3] += psi; q[4] += pitch; q[5] += roll
    v[0:3] = R @ v[0:3]
    return q, v


def move_plant_case(c, psi, d=(0.0, 0.0), pitch=0.0, roll=0.0):
    c = copy.deepcopy(c)
    c["q"], c["v"] = move_plant_state(c["q"], c["v"], psi, d, pitch, roll)
    return c


def move_wbc_case(oracle, c, psi, d=(0.0, 0.0), pitch=0.0, roll=0.0):
    """a case of wbc_base_cases: the measured state from the moved (q, v) it was built from (so the end-effector pose in the rbd vector moves with it),
    the planned state, the planned input and the previous input"""
    c = copy.deepcopy(c)
    c["q"], c["v"] = move_plant_state(c["q"], c["v"], psi, d, pitch, roll)
    c["rbd"] = oracle.rbd_from_q(c["q"], c["v"])
    c["xd"] = move_state(c["xd"], psi, d, pitch, roll); c["ud"] = move_input(c["ud"], psi); c["il"] = move_input(c["il"], psi)
    return c


def all_modes_schedule(t0, dur, order=ALL_MODES):
    """every mode of `order` held for `dur`, the first event at t0 + 0.01: (event times [16], modes [17])"""
    ev = np.array([t0 + 0.01 + k * dur for k in range(len(order) - 1)])
    return ev, np.array(order, dtype=np.int32)


def all_modes_config(dur=0.03, order=ALL_MODES, n_intervals=34):
    """C3 instance 0 walking the all-modes schedule"""
    from qm_control_amd import scenarios
    cfg = scenarios.make_config("C3", batch=1, n_intervals=n_intervals)
    ev, modes = all_modes_schedule(float(cfg["t0"][0]), dur, order)
    cfg["ev"] = ev[None].copy(); cfg["modes"] = modes[None].copy()
    return cfg


def stack_configs(cfgs):
    """one batch from single-instance configs of the same horizon (schedules padded as scenarios does it: further events far in the future, stance)"""
    from qm_control_amd import scenarios
    assert all(c["horizon"] == cfgs[0]["horizon"] and c["ref_t"].shape[1] == cfgs[0]["ref_t"].shape[1] for c in cfgs)
    ev, modes = scenarios._pad_schedules([c["ev"][0] for c in cfgs], [c["modes"][0] for c in cfgs])
    out = dict(cfgs[0]); out["B"] = len(cfgs); out["ev"] = ev; out["modes"] = modes
    for k in ("t0", "x0", "ref_t", "ref_x"):
        out[k] = np.concatenate([c[k][:1] for c in cfgs])
    return out


def lq_instances():
    """the batch of the entrywise LQ test: (name, single-instance config) — all modes at the nominal pose, all modes at POSES[0], all modes reversed and held longer at
    POSES[1], stance (C1) at POSES[2], and for each moved instance its twin: same schedule, pitch and roll, but psi = 0 and no translation (device equivariance)"""
    from qm_control_amd import scenarios
    out = [("all modes, nominal", all_modes_config(), None)]
    for name, make, pose in (("all modes", all_modes_config, POSES[0]), ("all modes reversed, 0.045 s", lambda: all_modes_config(0.045, ALL_MODES[::-1]), POSES[1]),
                             ("stance", lambda: scenarios.make_config("C1", batch=1, n_intervals=34), POSES[2])):
        out.append((name + " at %s" % (pose,), move_problem(make(), 0, pose[0], BASE_XY, pose[1], pose[2]), None))
        out.append((name + " twin", move_problem(make(), 0, 0.0, (0.0, 0.0), pose[1], pose[2]), (len(out) - 1, pose[0])))
    return out


def oracle_solve(oracle, cfg, b=0):
    oracle.set_schedule(cfg["ev"][b], cfg["modes"][b]); oracle.set_target(cfg["ref_t"][b], cfg["ref_x"][b])
    return oracle.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b])


def check_records(stage, dbg, oracle, r, after_riccati):
    """every non-event interval of the solve the oracle ran last (r = its result) through lq_record_check.check_interval; stage / dbg: [node][...] of that instance.
    Returns ({block: worst relative error}, [m of every checked interval])"""
    import lq_record_check as LC
    worst = {}; ms = []
    for i in range(len(r["t"]) - 1):
        if r["ev"][i] == 1:
            continue
        pr = oracle.node_proj(i); ms.append(pr["m"])
        for k, v in LC.check_interval(stage[i], dbg[i], oracle.node_lq(i), pr, after_riccati=after_riccati).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst, ms


def lq_blocks(dbg):
    """the unprojected model of one interval from a device debug record, keyed like oracle.node_lq"""
    import lq_record_check as LC
    D = LC.DBG; g = lambda off, *shape: np.asarray(dbg[off:off + int(np.prod(shape))]).reshape(shape)
    return dict(A=g(D["LQ_DBG_A"], 30, 30), B=g(D["LQ_DBG_B"], 30, 30), b=g(D["LQ_DBG_b"], 30), C=g(D["LQ_DBG_C"], 16, 30), D=g(D["LQ_DBG_D"], 16, 30), e=g(D["LQ_DBG_e"], 16), nc=int(dbg[D["LQ_DBG_nc"]]))


def equivariance_errs(twin, moved, mode, psi):
    """{block: max |moved - G twin G'| / max(max |G twin G'|, 1e-3)} of one interval (dicts as oracle.node_lq gives them), the metric of lq_record_check"""
    nc = twin["nc"]; assert moved["nc"] == nc
    gx, gu, gc = Gx(psi), Gu(psi), Gc(mode, psi); assert gc.shape[0] == nc
    out = {}
    for k, got, exp in (("A", moved["A"], gx @ twin["A"] @ gx.T), ("B", moved["B"], gx @ twin["B"] @ gu.T), ("b", moved["b"], gx @ twin["b"]),
                        ("C", moved["C"][:nc], gc @ twin["C"][:nc] @ gx.T), ("D", moved["D"][:nc], gc @ twin["D"][:nc] @ gu.T), ("e", moved["e"][:nc], gc @ twin["e"][:nc])):
        out[k] = float(np.abs(got - exp).max() / max(float(np.abs(exp).max()), 1e-3))
    return out


# the ORACLE's own equivariance residual of every moved instance of lq_instances() against its twin, worst interval, in equivariance_errs' metric (measured by
# test_offnominal.test_oracle_lq_model_is_equivariant, which holds the oracle to 100 x these).  The device is held to 100 x these too, and to 1e-10 at most.
ORACLE_EQUIVARIANCE = {
    1: dict(A=2.2e-16, B=2.6e-16, b=3.8e-13, C=1.5e-14, D=1.6e-14, e=1.1e-14),
    3: dict(A=2.6e-16, B=3.2e-16, b=2.0e-13, C=2.7e-14, D=1.5e-14, e=2.1e-14),
    5: dict(A=4.4e-16, B=3.7e-16, b=2.5e-14, C=7.4e-15, D=9.1e-15, e=0.0),      # (stance from rest: every foot velocity is exactly zero on both sides)
}


def equivariance_bound(inst, block):
    return min(100.0 * ORACLE_EQUIVARIANCE[inst][block], 1e-10)


def oracle_wbc(oracle, c, variant):
    oracle.wbc_reset(); oracle.wbc(c["xd"], c["il"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant))
    return oracle.wbc(c["xd"], c["ud"], c["rbd"], c["mode"], 0.002, c["time"], mpc_variant=bool(variant))


def torque_err(a, b):
    """the torque block of two WBC outputs on the scale tests/blocks.py gives it"""
    return float(np.abs(a[..., 36:] - b[..., 36:]).max() / max(float(np.abs(b[..., 36:]).max()), 0.1))


class _RecordingOracle:
    """hands rbd_from_q through to the oracle and keeps the (q, v) it was called with: wbc_cases builds each case's measured state from them and does not return them"""

    def __init__(self, oracle):
        self.oracle = oracle; self.calls = []

    def rbd_from_q(self, q, v=None):
        self.calls.append((np.array(q, float), np.array(v, float)))
        return self.oracle.rbd_from_q(q, v)


def wbc_base_cases(oracle, blobs, n, seed, hard=False, modes=None):
    """wbc_cases.random_wbc_inputs (vel_scale 0.05) or hard_wbc_inputs, unchanged, each case with the generalised coordinates q, v its rbd vector was built from"""
    from wbc_cases import random_wbc_inputs, hard_wbc_inputs
    rec = _RecordingOracle(oracle); modes = WBC_MODES if modes is None else modes
    cases = hard_wbc_inputs(rec, blobs, n, seed, modes) if hard else random_wbc_inputs(rec, blobs, n, seed, 0.05, modes)
    assert len(rec.calls) == len(cases)
    for c, (q, v) in zip(cases, rec.calls):
        c["q"], c["v"] = q, v
    return cases


def wbc_offnominal_cases(oracle, blobs, seed, hard_seed):
    """16 cases: random_wbc_inputs at the eight poses, then hard_wbc_inputs at the eight poses"""
    base = wbc_base_cases(oracle, blobs, 8, seed) + wbc_base_cases(oracle, blobs, 8, hard_seed, hard=True)
    return [move_wbc_case(oracle, c, POSES[k % 8][0], BASE_XY, POSES[k % 8][1], POSES[k % 8][2]) for k, c in enumerate(base)]


def plant_offnominal_cases(oracle, st, seed):
    """8 cases of test_sim.random_cases at the eight yaws and BASE_XY; pitch and roll scaled by 0.3 so that the feet stay near the ground"""
    from test_sim import random_cases
    return [move_plant_case(c, POSES[k][0], BASE_XY, 0.3 * POSES[k][1], 0.3 * POSES[k][2]) for k, c in enumerate(random_cases(oracle, st, 8, seed))]
