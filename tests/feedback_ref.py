"""tests/feedback_ref.py — TEST INFRASTRUCTURE: numpy references of the SQP's linear controller (sqp.useFeedbackPolicy; include/qmhip.h "feedback policy"), shared by
tests/test_feedback_policy.py (host emulator) and tests/test_gpu_feedback_policy.py (device).

Two independent routes to the gain of a node with an input of its own:
  kkt_gains     backward recursion of the EQUALITY-CONSTRAINED LQR on the oracle's unprojected node data (one dense KKT solve per stage with the rows C dx + D du + e = 0):
                no Px / Pu, no Cholesky of a reduced Hessian
  oracle_gains  Px + Pu K from the oracle's projection and Riccati sweep (node_proj)
"""
import numpy as np
import interp_cases as ic

GAIN_BLOCKS = [(rn, rs, cn, cs) for rn, rs in (("forces", slice(0, 12)), ("joint velocities", slice(12, 30)))
               for cn, cs in (("momentum", slice(0, 6)), ("base pose", slice(6, 12)), ("joints", slice(12, 30)))]
# |K_a - K_b| <= GAIN_TOL * max|K_b| per block (rows: forces / joint velocities; columns: momentum / base pose / joints).  Measured: the two CPU references above agree to
# 5.53e-13 in the worst block (forces / joints, C1) over stance (C1, 6 intervals), trot across a gait event (C2, 30 and 40 intervals) and the C5 instance near the arm's joint
# limits (56 intervals, three events), none with a warning bit.  The bound is ten times that (room for another compiler's contraction); it is far inside
# the ceiling of 1e-6 of the block's largest entry
GAIN_TOL = 5.6e-12


def gain_block_errs(K, Kref):
    return {"%s / %s" % (rn, cn): float(np.abs(K[rs, cs] - Kref[rs, cs]).max() / max(float(np.abs(Kref[rs, cs]).max()), 1e-300)) for rn, rs, cn, cs in GAIN_BLOCKS}


def assert_gain(K, Kref, what, tol=GAIN_TOL):
    errs = gain_block_errs(K, Kref); bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, "%s: gain blocks above %.1e: %s (all: %s)" % (what, tol, bad, errs)
    return errs


def kkt_gains(oracle, n):
    """K_ref,i of every node i < n - 1 with an input of its own (None at event nodes): equality-constrained LQR, conventions of tests/test_oracle.py::_dense_kkt_step
    (P is [u][x]; event nodes are identity jumps without input)"""
    S, _, _ = oracle.terminal(); out = [None] * (n - 1)
    for i in reversed(range(n - 1)):
        q = oracle.node_lq(i)
        if q["event"]:
            assert np.array_equal(q["A"], np.eye(30)); continue            # S_i = S_{i+1}
        nc = q["nc"]; A, B, C, D = q["A"], q["B"], q["C"][:nc], q["D"][:nc]
        Huu = q["R"] + B.T @ S @ B; Hux = q["P"] + B.T @ S @ A; Hxx = q["Q"] + A.T @ S @ A
        kkt = np.block([[Huu, D.T], [D, np.zeros((nc, nc))]])
        K = np.linalg.solve(kkt, -np.vstack([Hux, C]))[:30]
        S = Hxx + Hux.T @ K + K.T @ Hux + K.T @ Huu @ K; S = 0.5 * (S + S.T)
        out[i] = K
    return out


def source_node(ev, i):
    """the node whose input node i of the grid carries (qm_ls_apply_kernel, k_ls.h): itself, or the closest earlier node with an input of its own; None: there is none"""
    n = len(ev); j = n - 2 if i == n - 1 else i
    if j < 0: return None
    while j > 0 and ev[j] == 1: j -= 1
    return None if ev[j] == 1 else j


def oracle_gains(oracle, res):
    """per node of the oracle's last solve `res`: (K_full [n][30][30], uff [n][30], src [n]) with K_full = Px + Pu K of the node the input was copied from, uff = u* - K_full x*_src"""
    n = len(res["t"]); own = {}
    for i in range(n - 1):
        if res["ev"][i] != 1:
            p = oracle.node_proj(i); m = p["m"]; own[i] = p["Px"] + p["Pu"][:, :m] @ p["K"][:m]
    K = np.zeros((n, 30, 30)); uff = np.zeros((n, 30)); src = np.full(n, -1)
    for i in range(n):
        j = source_node(res["ev"], i)
        if j is None: continue
        K[i] = own[j]; uff[i] = res["u"][i] - own[j] @ res["x"][j]; src[i] = j
    return K, uff, src


def linear_policy(res, K, src, t, x):
    """u(t, x) of the linear controller: segment and weight as the feed-forward policy (interp_cases.time_segment on the nudged node times), each bracketing node's term
    u*_i + K_i (x - x*_src(i))"""
    ta = res["t"] + np.where(res["ev"] == 2, ic.LIMIT_EPS, np.where(res["ev"] == 1, -ic.LIMIT_EPS, 0.0))
    i, al = ic.time_segment(ta, t); j = i + 1 if len(ta) > 1 else i
    term = lambda k: res["u"][k] + (K[k] @ (x - res["x"][src[k]]) if src[k] >= 0 else 0.0)
    return al * term(i) + (1.0 - al) * term(j)


# ---- the oracle's gains as the stage records the device kernels read (host emulator fixtures) ----
def _chain(c): return {0: 0, 1: 2, 2: 1, 3: 3}[c]          # contact (LF RF LH RH) -> leg chain (LF LH RF RH)


def device_pu(mode, D):
    """the null-space basis in the product's form (k_riccati.h forward rollout): unit columns for the stance feet's force components, one 3 x 2 block per swing leg on its
    joint velocities (ANY basis of the null space of the leg's swing-height row of D), unit columns for the arm.  Returns (Pu [30][m], swing blocks [4][3][2])"""
    flag = lambda c: (mode >> (3 - c)) & 1
    cols = []; swg = np.zeros((4, 3, 2))
    for c in range(4):
        if flag(c):
            for k in range(3): e = np.zeros(30); e[3 * c + k] = 1.0; cols.append(e)
    for c in range(4):
        if not flag(c):
            js = slice(12 + 3 * _chain(c), 15 + 3 * _chain(c))
            rows = [r for r in D if np.abs(r[js]).max() > 0.0]
            assert len(rows) == 1 and np.abs(np.delete(rows[0], np.r_[js])).max() == 0.0, "a swing leg has one row of D, on its own joint velocities"
            N = np.linalg.svd(rows[0][js][None, :])[2][1:].T; swg[c] = N
            for k in range(2): e = np.zeros(30); e[js] = N[:, k]; cols.append(e)
    for k in range(6): e = np.zeros(30); e[24 + k] = 1.0; cols.append(e)
    return np.stack(cols, axis=1), swg


def device_records(oracle, res, layout, nmax):
    """stage records [nmax][SR_SIZE] holding what the feedback kernels read (K, the twelve rows of Px, swing blocks, mode, m), built from the oracle's projection and gains
    re-expressed in the product's null-space basis; everything else NaN (a read outside those fields shows)"""
    SR, PP, PX, SWG, MODEF, SCAL = layout
    n = len(res["t"]); rec = np.full((nmax, SR), np.nan)
    for i in range(n - 1):
        if res["ev"][i] == 1: continue
        p = oracle.node_proj(i); q = oracle.node_lq(i); m = p["m"]; mode = int(res["mode"][i])
        Pu, swg = device_pu(mode, q["D"][:q["nc"]]); assert Pu.shape[1] == m
        PuK = p["Pu"][:, :m] @ p["K"][:m]
        Kd = np.linalg.lstsq(Pu, PuK, rcond=None)[0]
        assert np.abs(Pu @ Kd - PuK).max() <= 1e-10 * max(1.0, np.abs(PuK).max()), "the product's basis spans the oracle's null space"
        assert max(np.abs(p["Px"][:12]).max(), np.abs(p["Px"][24:]).max()) <= 1e-13 * np.abs(p["Px"]).max(), "Px has the leg joint-velocity rows only (up to the rounding of the oracle's pseudo-inverse)"
        r = rec[i]; r[PP:PP + 540] = 0.0; r[PP:PP + 30 * m] = Kd.ravel(); r[PX + 360:PX + 720] = p["Px"][12:24].ravel()
        for c in range(4): r[SWG + 6 * c:SWG + 6 * c + 6] = swg[c].T.ravel()      # column-major 3 x 2
        r[MODEF] = float(mode); r[SCAL] = float(m)
    return rec
