"""Planned task-space trajectories (include/qmhip.h "planned task-space trajectories") without a GPU: the three kernels of csrc/kernels/k_plan.h on the host emulator
(tests/emu_plan), launched through the product's pipeline calls, against the oracle-built reference of tests/plan_ref.py on a ragged batch of oracle solves."""
import ctypes as C

import numpy as np
import pytest

import plan_ref as pf
from qm_control_amd import api, layout as L, scenarios

B = 65                      # one full wave of instances plus one row in the next: every node's rows cross the cooperative tile's edge with a nearly empty wave
GAITS = [("trot", 20, 7), ("stance", 12, 8), ("flying_trot", 20, 9), ("trot", 17, 10), ("standing_trot", 20, 11)]      # (template, intervals, seed): different node counts, a flight phase, all-stance phases


@pytest.fixture(scope="module")
def lib():
    return pf.emu_lib()


class Batch:
    """solver buffers of a ragged batch in the device's layout (node-major [nmax][B][k]) holding the oracle's solves, instance b = solve b % len(GAITS); NaN (ints: -1)
    wherever the solver would hold stale data.  Computed once, never modified"""

    def __init__(self, oracle):
        self.solves = []
        for gait, N, seed in GAITS:
            cfg = scenarios.gait_config(gait, batch=1, n_intervals=N, seed=seed)
            oracle.set_schedule(cfg["ev"][0], cfg["modes"][0]); oracle.set_target(cfg["ref_t"][0], cfg["ref_x"][0])
            r = oracle.mpc_step(cfg["t0"][0], cfg["t0"][0] + cfg["horizon"], cfg["x0"][0]); n = len(r["t"])
            ee = np.array([np.concatenate(oracle.desired_state(t)[1:]) for t in r["t"]])
            self.solves.append(dict(cfg=cfg, res=r, n=n, ee=ee, ref=pf.plan(oracle, cfg["ref_t"][0], cfg["ref_x"][0], r["t"], r["x"], r["u"], r["mode"]),
                                    fh=pf.footholds(oracle, r["t"], r["x"], cfg["ev"][0], cfg["modes"][0])))
        self.nmax = nm = max(s["n"] for s in self.solves) + 3; self.nev = ne = max(s["cfg"]["ev"].shape[1] for s in self.solves)
        self.n_nodes = np.zeros(B, np.int32); self.node_t = np.full((nm, B), np.nan); self.node_ev = np.full((nm, B), -1, np.int32); self.node_mode = np.full((nm, B), -1, np.int32)
        self.xs = np.full((nm, B, 30), np.nan); self.us = np.full((nm, B, 30), np.nan); self.eeref = np.full((nm, B, 7), np.nan)
        self.ev = np.zeros((B, ne)); self.modes = np.full((B, ne + 1), 15, np.int32)
        for b in range(B):
            s = self.of(b); r = s["res"]; n = s["n"]; e = s["cfg"]["ev"][0]; m = s["cfg"]["modes"][0]
            self.n_nodes[b] = n; self.node_t[:n, b] = r["t"]; self.node_ev[:n, b] = r["ev"]; self.node_mode[:n, b] = r["mode"]; self.xs[:n, b] = r["x"]; self.us[:n, b] = r["u"]; self.eeref[:n, b] = s["ee"]
            self.ev[b, :len(e)] = e; self.ev[b, len(e):] = e[-1] + 1e3 * np.arange(1, ne - len(e) + 1); self.modes[b, :len(m)] = m; self.modes[b, len(m):] = m[-1]
        self.mb = np.ascontiguousarray(scenarios.load_blobs()[0])

    def of(self, b): return self.solves[b % len(self.solves)]

    def run(self, lib, cap, records=True):
        rec = np.full((B, self.nmax), 0, api.PLAN_RECORD); rec.view(np.uint8)[:] = 0xff; nn = np.full(B, -7, np.int32)
        fh = np.zeros((B, max(cap, 1)), api.FOOTHOLD); cnt = np.full(B, -7, np.int32)
        code = lib.emu_plan_solution(pf.ptr(self.mb), B, self.nmax, self.nev, pf.ptr(self.n_nodes), pf.ptr(self.node_t), pf.ptr(self.node_ev), pf.ptr(self.node_mode), pf.ptr(self.xs), pf.ptr(self.us), pf.ptr(self.eeref),
                                     pf.ptr(self.ev), pf.ptr(self.modes), pf.ptr(rec) if records else None, pf.ptr(nn), cap, pf.ptr(fh), pf.ptr(cnt))
        return rec, nn, fh, cnt, code


@pytest.fixture(scope="module")
def batch(oracle):
    return Batch(oracle)


def test_record_layout(lib):
    """struct qmhip_plan_record / qmhip_foothold as the compiler lays them out, the PT_* word offsets, layout.py and the numpy mirrors agree"""
    v = [lib.emu_plan_layout(i) for i in range(18)]
    assert v[:3] == [512, 64, 40] and v[16:] == [512, 40] and v[15] <= 24 * 1024
    names = ["PT_TIME", "PT_MODE", "PT_BASE_POS", "PT_BASE_ZYX", "PT_FOOT_POS", "PT_FOOT_VEL", "PT_FOOT_FORCE", "PT_EE_POS", "PT_EE_QUAT", "PT_EE_ERR", "PT_COP", "PT_SPARE"]
    assert v[3:15] == [getattr(L, n) for n in names] == [0, 1, 2, 5, 8, 20, 32, 44, 47, 51, 57, 60]
    d = api.PLAN_RECORD; assert d.itemsize == L.QM_PLAN_BYTES == 512
    for f, n in zip(("time", "mode", "base_pos", "base_zyx", "foot_pos", "foot_vel", "foot_force", "ee_pos", "ee_quat", "ee_err", "cop", "spare"), names):
        assert d.fields[f][1] == 8 * getattr(L, n), f
    assert d.fields["contact_mask"][1] == 8 * L.PT_MODE + 4 and d["foot_pos"].shape == (4, 3) and d["spare"].shape == (4,)
    assert api.FOOTHOLD.itemsize == L.QM_FOOTHOLD_BYTES == 40 and [api.FOOTHOLD.fields[f][1] for f in ("time", "leg", "event", "pos")] == [0, 8, 12, 16]
    assert [pf.contact_mask(m) for m in (15, 9, 6, 0, 8)] == [15, 9, 6, 0, 1]      # 9 = LF + RH: bits 0 and 3; 8 = LF alone: bit 0


def test_node_records_of_a_ragged_batch(lib, batch):
    """every record of every instance against the oracle-built reference; rows at or behind num_nodes[b] are zero; instances holding the same solve get the same bits
    (whatever wave and lane they sit in); both CoP branches and the all-stance mask occur.  One node kernel launch, one gather, one host wait"""
    rec, nn, _, _, code = batch.run(lib, 0); assert np.array_equal(nn, batch.n_nodes); mx = {}
    for b in range(B):
        s = batch.of(b); n = s["n"]
        assert not rec[b, n:].tobytes().strip(b"\0"), b
        if b < len(GAITS): mx = pf.merge(mx, pf.compare(rec[b, :n], s["ref"], "instance %d" % b))
        else: assert rec[b, :n].tobytes() == rec[b % len(GAITS), :n].tobytes(), b
    live = np.concatenate([rec[b, :batch.of(b)["n"]] for b in range(len(GAITS))])
    assert (live["contact_mask"] == 0).any() and (live["contact_mask"] == 15).any() and (live["cop"][:, 2] > 1.0).any()
    print("emulator, node records: max abs differences", {k: "%.1e" % v for k, v in sorted(mx.items())})
    for k, v in mx.items(): assert v <= 0.1 * (pf.ATOL_VEL if k in ("foot_vel", "ee_err") else pf.ATOL_POS), (k, v)      # a tenth of the bound: the margin the issue asks to look into
    assert code // 100 == 3 and code % 100 == 2      # nodes + gather + footholds; one wait per call


def test_footholds_of_a_ragged_batch(lib, batch):
    """count, leg, event, time equal the reference's, positions within the position bound, ordered by (event, foot); cap = 1 leaves count as it is and writes slot 0 only"""
    cap = 16; _, _, fh, cnt, _ = batch.run(lib, cap, records=False); mx = 0.0
    for b in range(B): mx = max(mx, pf.compare_footholds(fh[b], cnt[b], batch.of(b)["fh"], cap, "instance %d" % b))
    assert cnt.sum() > 0 and len(set(cnt.tolist())) > 1 and cnt.max() <= cap, cnt
    _, _, fh1, cnt1, _ = batch.run(lib, 1, records=False); assert np.array_equal(cnt1, cnt)
    for b in range(B): pf.compare_footholds(fh1[b], cnt1[b], batch.of(b)["fh"], 1, "cap 1, instance %d" % b)
    _, _, _, cnt0, _ = batch.run(lib, 0, records=False); assert np.array_equal(cnt0, cnt)
    print("emulator, footholds: %d landings, per instance %s, max abs position difference %.1e" % (cnt.sum(), sorted(set(cnt.tolist())), mx)); assert mx <= 0.1 * pf.ATOL_POS


def test_states_rows(lib, batch, oracle, blobs):
    """R = 130 random states (joints inside their limits, random base attitude, every mode) through qm_plan_states_kernel: with inputs and references, without inputs,
    without references; a node of the plan evaluated as a row gives the node record's bits"""
    R = 130; x, u, mode, ee = pf.random_states(blobs, R, 3); mb = batch.mb; mx = {}
    def run(xx, uu, mm, ee_):
        rec = np.zeros(len(xx), api.PLAN_RECORD); rec.view(np.uint8)[:] = 0xff
        lib.emu_plan_eval(pf.ptr(mb), len(xx), pf.ptr(np.ascontiguousarray(xx)), pf.ptr(uu), pf.ptr(np.ascontiguousarray(mm, np.int32)), pf.ptr(ee_), pf.ptr(rec)); return rec
    for uu, ee_, what in ((u, ee, "u, ee"), (None, ee, "no u"), (u, None, "no ee"), (None, None, "neither")):
        ref = np.array([pf.record(oracle, x[r], None if uu is None else uu[r], mode[r], None if ee_ is None else (ee_[r, :3], ee_[r, 3:])) for r in range(R)])
        got = run(x, uu, mode, ee_); mx = pf.merge(mx, pf.compare(got, ref, what))
        if ee_ is None: assert not got["ee_err"].any()
        if uu is None: assert not got["foot_force"].any() and not got["cop"].any()
    print("emulator, state rows: max abs differences", {k: "%.1e" % v for k, v in sorted(mx.items())})
    for k, v in mx.items(): assert v <= 0.1 * (pf.ATOL_VEL if k in ("foot_vel", "ee_err") else pf.ATOL_POS), (k, v)
    rec, _, _, _, _ = batch.run(lib, 0); s = batch.of(0); r = s["res"]; n = s["n"]
    row = run(r["x"], np.ascontiguousarray(r["u"]), r["mode"], np.ascontiguousarray(s["ee"])); row["time"] = r["t"]
    assert row.tobytes() == rec[0, :n].tobytes()
