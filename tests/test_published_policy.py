"""Published feedback policy (include/qmhip.h "published feedback policy") without a GPU: the two kernels of csrc/kernels/k_publish.h on the host emulator (tests/emu_pub)
against numpy on records built from the oracle's gains, and the pipelined loop with the published linear controller against the loop built from the oracle's pieces."""
import ctypes as C

import numpy as np
import pytest

import feedback_ref as fr
import interp_cases as ic
import published_ref as pr
from conftest import assert_blocks, rel_err
from qm_control_amd import layout as L, scenarios

CASES = [("C1", 6, "stance"), ("C2", 30, "trot across a gait event"), ("C5", 56, "trot -> stance, arm near its joint limits")]
NMAX = 66


@pytest.fixture(scope="module")
def lib():
    return pr.emu_lib()


def _solve(oracle, blobs_o, name, N):
    cfg = scenarios.make_config(name, batch=8 if name == "C5" else 1, n_intervals=N); b = 0
    if name == "C5":                                          # the instance whose arm starts within 0.1 rad of the joint-2/3 lower limits (tests/test_oracle.py)
        lo = blobs_o[0][288 + 12:288 + 18]
        b = [k for k in range(8) if cfg["x0"][k, 25] - lo[1] < 0.1001 and cfg["x0"][k, 26] - lo[2] < 0.1001][0]
    oracle.set_schedule(cfg["ev"][b], cfg["modes"][b]); oracle.set_target(cfg["ref_t"][b], cfg["ref_x"][b])
    res = oracle.mpc_step(cfg["t0"][b], cfg["t0"][b] + cfg["horizon"], cfg["x0"][b])
    assert res["warn"] == 0
    return dict(cfg=cfg, b=b, res=res)


class Batch:
    """solver buffers of a ragged batch in the device's layout (node-major [nmax][B][k], stage records [B][nmax][SR_SIZE], NaN outside the fields the feedback kernels
    read — feedback_ref.device_records) holding the oracle's solves, instance b = solve b % 3.  Computed once, never modified"""

    def __init__(self, lib, oracle, oblobs, B):
        lay = [lib.emu_pub_layout(i) for i in range(12)]; self.SR = lay[:6]; self.PR = lay[6:]; self.B = B; self.nmax = NMAX; self.solves = []
        for name, N, _ in CASES:      # (the oracle holds the node data of its LAST solve: gains and records are taken before the next one)
            s = _solve(oracle, oblobs, name, N); s["K"], s["uff"], s["src"] = fr.oracle_gains(oracle, s["res"]); s["rec"] = fr.device_records(oracle, s["res"], self.SR, NMAX); self.solves.append(s)
        self.nev = max(s["cfg"]["ev"].shape[1] for s in self.solves); nm, ne = NMAX, self.nev
        self.n_nodes = np.zeros(B, np.int32); self.node_t = np.zeros((nm, B)); self.node_ev = np.zeros((nm, B), np.int32); self.xs = np.full((nm, B, 30), np.nan); self.us = np.full((nm, B, 30), np.nan)
        self.ev = np.full((B, ne), 1e9); self.modes = np.full((B, ne + 1), 15, np.int32)
        raw = np.zeros(B * nm * self.SR[0] + 8); off = (-raw.ctypes.data // 8) % 8; self.stage = raw[off:off + B * nm * self.SR[0]].reshape(B, nm, self.SR[0])      # 64-byte aligned: the kernel moves 16-byte pieces
        for b in range(B):
            s = self.of(b); r = s["res"]; n = len(r["t"]); e = s["cfg"]["ev"][s["b"]]; m = s["cfg"]["modes"][s["b"]]; assert n + 3 <= nm
            self.n_nodes[b] = n; self.node_t[:n, b] = r["t"]; self.node_ev[:n, b] = r["ev"]; self.xs[:n, b] = r["x"]; self.us[:n, b] = r["u"]; self.stage[b] = s["rec"]
            self.ev[b, :len(e)] = e; self.modes[b, :len(m)] = m; self.modes[b, len(m):] = m[-1]

    def of(self, b): return self.solves[b % len(self.solves)]

    def published(self, lib, W, t, x, n_pub=1, want_pub=False):
        B = self.B; t = np.ascontiguousarray(t, float); x = None if x is None else np.ascontiguousarray(x, float)
        xd = np.full((B, 30), np.nan); ud = np.full((B, 30), np.nan); mode = np.full(B, -7, np.int32); cov = np.full(B, -7, np.int32); pub = np.zeros((B + 1, W, self.PR[0])) if want_pub else None
        seq = lib.emu_pub_publish_eval(B, self.nmax, self.nev, W, n_pub, pr.ptr(self.n_nodes), pr.ptr(self.node_t), pr.ptr(self.node_ev), pr.ptr(self.xs), pr.ptr(self.us), pr.ptr(self.ev), pr.ptr(self.modes),
                                       pr.ptr(self.stage), pr.ptr(t), pr.ptr(x), pr.ptr(xd), pr.ptr(ud), pr.ptr(mode), pr.ptr(cov), pr.ptr(pub))
        return xd, ud, mode, cov, seq, pub


@pytest.fixture(scope="module")
def batch(lib, oracle, oblobs):
    return Batch(lib, oracle, oblobs, 9)      # three instances per case; ragged n_nodes (7, 33, 62 nodes)


@pytest.fixture(scope="module")
def live(batch):
    """qm_policy_fb_kernel on the same data through tests/emu_fb (the live-record path): (t, x) -> (x_des, u_des, mode)"""
    import os, subprocess
    here = os.path.dirname(os.path.abspath(__file__)); subprocess.check_call(["make", "-C", os.path.join(here, "emu_fb"), "-s"])
    fb = C.CDLL(os.path.join(here, "emu_fb", "_build", "libqm_emu_fb.so"))

    def run(t, x):
        B = batch.B; t = np.ascontiguousarray(t, float); x = np.ascontiguousarray(x, float); xd = np.zeros((B, 30)); ud = np.zeros((B, 30)); mode = np.zeros(B, np.int32)
        assert fb.emu_fb_policy(B, batch.nmax, batch.nev, pr.ptr(batch.n_nodes), pr.ptr(batch.node_t), pr.ptr(batch.node_ev), pr.ptr(batch.xs), pr.ptr(batch.us), pr.ptr(batch.ev), pr.ptr(batch.modes),
                                pr.ptr(batch.stage), pr.ptr(t), pr.ptr(x), pr.ptr(xd), pr.ptr(ud), pr.ptr(mode)) == 1
        return xd, ud, mode
    return run


def _perturbation(rng, B):
    dx = rng.normal(size=(B, 30))
    for sl in (slice(0, 6), slice(6, 12), slice(12, 30)): dx[:, sl] *= 10.0 ** rng.uniform(-3, -1, size=(B, 1))
    return dx


def test_publish_kernel_copies_the_read_fields_only(lib, batch):
    """qm_policy_publish_kernel: node i < W of instance b holds exactly K, the twelve rows of Px, the swing blocks, the mode and m of its stage record at the PR_* offsets —
    the NaNs around those fields in the stage record do not travel —, zeros where the node has no record of its own, and nothing is written behind the batch (the slot's
    tail keeps the NaNs a fresh buffer holds)"""
    SRn, PP, PX, SWG, MODEF, SCAL = batch.SR; PRn, pPP, pPX, pSWG, pMODEF, pSCAL = batch.PR
    assert PRn % 2 == 0 and PRn <= 1024 and PRn == L.PR_SIZE and (pPP, pPX, pSWG, pMODEF, pSCAL) == (L.PR_PP, L.PR_PX, L.PR_SWG, L.PR_MODEF, L.PR_SCAL)
    for W in (2, 5, 62):
        *_, seq, pub = batch.published(lib, W, np.zeros(batch.B), None, want_pub=True); assert seq == 1
        assert np.isnan(pub[batch.B]).all()
        for b in range(batch.B):
            r = batch.of(b)["res"]; n = len(r["t"])
            for i in range(W):
                rec = batch.stage[b, i]; got = pub[b, i]
                if i < n - 1 and r["ev"][i] != 1:
                    want = np.zeros(PRn); want[pPP:pPP + 540] = rec[PP:PP + 540]; want[pPX + 360:pPX + 720] = rec[PX + 360:PX + 720]; want[pSWG:pSWG + 24] = rec[SWG:SWG + 24]; want[pMODEF] = rec[MODEF]; want[pSCAL] = rec[SCAL]
                    assert np.array_equal(got, want), (W, b, i)
                else: assert not got.any(), (W, b, i)


@pytest.mark.parametrize("W", [2, 5, 7, 33, 62])
def test_emulated_published_policy_vs_numpy(lib, batch, live, W):
    """qm_policy_fb_pub_kernel after qm_policy_publish_kernel with windows of 2, 5 and n nodes (n = 7, 33, 62 for the three cases), at the times of
    interp_cases.policy_times (node times and their neighbours, both sides of every event, outside the grid) and between nodes, at states 1e-3 ... 1e-1 off the plan:
    `covered` is the numpy predicate; an instance that is not covered — and every instance with x == NULL — gets interp_cases.policy_reference bit for bit; a covered one is
    within 1e-12 per block of feedback_ref.linear_policy and array_equal to qm_policy_fb_kernel on the live records.  The window's far end is read, nothing behind it:
    the records behind the window and the slot's tail hold NaN"""
    rng = np.random.default_rng(11 + W); B = batch.B; per = B // len(batch.solves); sweeps = []
    for s in batch.solves:
        r = s["res"]; w = ic.policy_times(r["t"], r["ev"], s["cfg"]["ev"][s["b"]], r["t"][0], r["t"][-1])
        n = len(r["t"]); mid = 0.5 * (r["t"][:-1] + r["t"][1:])      # every query around the grid's start and around the window's end, a thinned sweep of the rest
        dense = (w <= r["t"][min(n, 3) - 1] + 1e-5) | ((w >= r["t"][min(max(W - 2, 0), n - 1)] - 1e-5) & (w <= r["t"][min(W + 1, n - 1)] + 1e-5))
        sweeps.append(np.concatenate([w[dense], w[~dense][::9], mid[max(W - 3, 0):W + 2], mid[::7], w[-4:]]))
    rounds = max(len(w) for w in sweeps) // per + 1; n_cov = n_unc = 0; n_pub = 1
    for k in range(rounds):
        t = np.zeros(B)
        for b in range(B):
            w = sweeps[b % len(sweeps)]; j = k * per + b // len(sweeps); t[b] = w[j] if j < len(w) else rng.uniform(w[0], w[-3])
        xm = np.zeros((B, 30)); dx = _perturbation(rng, B); ref = np.zeros((B, 30)); ffx = np.zeros((B, 30)); ffu = np.zeros((B, 30)); cref = np.zeros(B, np.int32)
        for b in range(B):
            s = batch.of(b); r = s["res"]; ffx[b], ffu[b] = ic.policy_reference(r["t"], r["ev"], r["x"], r["u"], t[b]); xm[b] = ffx[b] + dx[b]
            ref[b] = fr.linear_policy(r, s["K"], s["src"], t[b], xm[b]); cref[b] = pr.covered_ref(r, W, t[b])
        n_pub = 1 + k % 3      # (one, two or three publications: the slots alternate, the last one is evaluated)
        xd, ud, mode, cov, seq, _ = batch.published(lib, W, t, xm, n_pub=n_pub); assert seq == n_pub
        xf, uf, mf, covf, _, _ = batch.published(lib, W, t, None)
        xl, ul, ml = live(t, xm)
        assert np.array_equal(cov, cref) and np.array_equal(covf, cref), (W, k)
        assert np.array_equal(xd, ffx) and np.array_equal(xf, ffx) and np.array_equal(uf, ffu) and np.array_equal(mode, ml) and np.array_equal(mf, ml), (W, k)
        c = cref == 1; n_cov += int(c.sum()); n_unc += int((~c).sum())
        assert np.array_equal(ud[~c], ffu[~c]), (W, k)
        assert np.array_equal(ud[c], ul[c]), (W, k)
        if c.any(): assert_blocks(ud[c], ref[c], "u", 1e-12, "W %d round %d" % (W, k))
    assert n_cov > 20 and (n_unc > 20 or W == 62)


def _loop_setup(blobs):
    import os, sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    from test_sim import robust_grid_settings
    mb, st = blobs; horizon = 0.45; c = setup("trot", 1, horizon, t_start=20.2); c["horizon"] = horizon; c["B"] = 1
    q0 = c["xbar"][6:30].copy(); q0[2] = 0.385
    return mb, robust_grid_settings(st), c, q0, horizon


def test_emulated_pipelined_feedback_loop_vs_oracle(lib, blobs, oracle):
    """qm_closed_loop_sim_pipelined with a publisher (window 8): 3 periods of 4 ticks on the host emulator against the oracle-built loop with the same latency and the numpy
    linear controller on the gains taken at solve time (published_ref.oracle_pipelined_feedback_loop); the bounds of test_sim.py::test_emulated_pipelined_loop_vs_oracle
    (tau 1e-6, q 1e-9, v 1e-7).  Every tick is covered and the feedback term is there"""
    mb, st, c, q0, horizon = _loop_setup(blobs)
    e = pr.EmuLoop(lib, mb, st, 1, 64, 2, c["ev"].shape[1]); e.set_window(8); e.start(c, 1, q0, 20.2); dev = []
    for p in range(3):
        e.loop(4, 0.001, horizon, 2, 4, True); dev.append(e.state())
    launches, waits, records = e.counts(); e.close()
    log = pr.oracle_pipelined_feedback_loop(oracle, mb, c, q0, 12, 0.001, 2, 4, horizon, 0.0, 0.5, 20.2)
    worst = dict(tau=0.0, q=0.0, v=0.0)
    for p in range(3):
        k = 4 * p + 3
        assert dev[p]["mpc_status"][0] == 0 and list(dev[p]["wbc_status"][0]) == [0, 0, 0] and log[k]["wbc_status"] == [0, 0, 0], p
        assert dev[p]["seq"] == p + 1 and dev[p]["uncovered"][0] == 0, (p, dev[p]["seq"], dev[p]["uncovered"])
        for key in worst: worst[key] = max(worst[key], rel_err(dev[p][key][0], log[k][key]))
    print("emulated pipelined feedback loop: worst errors vs the oracle loop %s, largest feedback term %.3e, furthest node read %d" % ({k: "%.2e" % v for k, v in worst.items()}, max(l["du"] for l in log), max(l["node"] for l in log)))
    assert worst["tau"] < 1e-6 and worst["q"] < 1e-9 and worst["v"] < 1e-7, worst
    assert max(l["du"] for l in log) > 1e-3 and max(l["node"] for l in log) < 8
    assert records == 3 and waits == 0      # one publication event per publication; no evaluation from outside the loop to wait for


def test_emulated_pipelined_loop_ignores_the_window_without_feedback(lib, blobs):
    """window on, ST_FEEDBACK_POLICY = 0: the loop is the feed-forward one — array_equal to the loop on a context without a window, tick for tick"""
    mb, st, c, q0, horizon = _loop_setup(blobs); runs = []
    for W in (0, 8):
        e = pr.EmuLoop(lib, mb, st, 1, 64, 2, c["ev"].shape[1])
        if W: e.set_window(W)
        e.start(c, 1, q0, 20.2); out = []
        for p in range(2):
            e.loop(4, 0.001, horizon, 2, 4, False); out.append(e.state())
        assert out[-1]["seq"] == 0; runs.append(out); e.close()
    for a, b in zip(*runs):
        for key in ("q", "v", "out", "u_des", "wbc_status", "mpc_status"): assert np.array_equal(a[key], b[key]), key
