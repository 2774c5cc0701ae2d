"""Step-I/O pack kernel (csrc/kernels/k_io.h) and its host pipeline (csrc/host/qm_io_pipeline.h) on the host emulator, against a numpy gather — exactly: the kernel moves
bits.  Also: the record's layout (include/qmhip_layout.h <-> qm_control_amd/layout.py) and qm_mpc_status, device instance against host instance, on the table of its comment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from qm_control_amd import api, layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
MPC, WBC, NOWBC, TRAJ = 1, 2, 4, 8      # QM_PACK_* (k_io.h)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_io"), "-s"])
    lib = C.CDLL(os.path.join(_HERE, "emu_io", "_build", "libqm_emu_io.so"))
    lib.emu_io_slot_bytes.restype = C.c_long
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _buffers(rng, B, nmax, n_nodes):
    """node-major solver buffers [nmax][B][k] and per-instance ones, every word distinct enough that a wrong index shows"""
    d = dict(x_des=rng.normal(size=(B, 30)), u_des=rng.normal(size=(B, 30)), mode=rng.integers(0, 16, B).astype(np.int32), wbc_out=rng.normal(size=(B, 54)),
             qp_status=rng.integers(0, 3, (B, 3)).astype(np.int32), out_perf=rng.normal(size=(B, 10)), status=np.zeros(B, np.int32), step_info=np.abs(rng.normal(size=(B, 4))),
             n_nodes=np.asarray(n_nodes, np.int32), node_t=rng.normal(size=(nmax, B)), node_ev=rng.integers(0, 3, (nmax, B)).astype(np.int32),
             node_mode=rng.integers(0, 16, (nmax, B)).astype(np.int32), xs=rng.normal(size=(nmax, B, 30)), us=rng.normal(size=(nmax, B, 30)))
    d["step_info"][:, 3] = 0.0
    return d


ORDER = ("x_des", "u_des", "mode", "wbc_out", "qp_status", "out_perf", "status", "step_info", "n_nodes", "node_t", "node_ev", "node_mode", "xs", "us")


def _expected(d, B, ncap, with_wbc, traj):
    rec = np.zeros(B, api.STEP_RECORD)
    rec["x_des"] = d["x_des"]; rec["u_des"] = d["u_des"]; rec["perf"] = d["out_perf"]; rec["mode"] = d["mode"]; rec["mpc_status"] = d["status"]; rec["n_nodes"] = d["n_nodes"]
    if with_wbc:
        rec["wbc_out"] = d["wbc_out"]; rec["qp_status"] = d["qp_status"]
    out = [rec.tobytes()]
    if traj:
        keep = (np.arange(ncap)[None, :] < d["n_nodes"][:, None])                      # [B][ncap]
        g = lambda a: np.where(keep.reshape(keep.shape + (1,) * (a.ndim - 2)), np.moveaxis(a[:ncap], 0, 1), 0).astype(a.dtype)
        pad = lambda a: a.tobytes() + b"\0" * (-a.nbytes % 8)
        out += [g(d["node_t"]).tobytes(), g(d["xs"]).tobytes(), g(d["us"]).tobytes(), pad(g(d["node_ev"])), pad(g(d["node_mode"]))]
    return b"".join(out)


CASES = [  # (B, nmax, ncap, n_nodes)
    (1, 8, 5, [5]),                                              # B = 1, n_nodes == ncap
    (1, 8, 3, [3]),
    (5, 12, 9, [9, 3, 7, 3, 8]),                                 # ragged, odd B * ncap (the int sections end in half a word)
    (67, 20, 17, None),                                          # B not a multiple of the block size, records spread over several blocks
    (300, 16, 16, None),                                         # ncap == nmax
]


@pytest.mark.parametrize("B,nmax,ncap,n_nodes", CASES)
@pytest.mark.parametrize("with_wbc", [True, False])
def test_pack_kernel_equals_a_numpy_gather(lib, B, nmax, ncap, n_nodes, with_wbc):
    rng = np.random.default_rng(B * 131 + ncap)
    if n_nodes is None:
        n_nodes = rng.integers(3, ncap + 1, B); n_nodes[0] = ncap; n_nodes[-1] = 3
    d = _buffers(rng, B, nmax, n_nodes)
    nbytes = lib.emu_io_slot_bytes(B, ncap, 1)
    assert nbytes == B * L.QM_STEP_BYTES + 8 * (B * ncap * 61 + 2 * ((B * ncap + 1) // 2))
    slot = np.full(nbytes, 0xA5, np.uint8)
    lib.emu_io_pack(B, nmax, ncap, MPC | TRAJ | (0 if with_wbc else NOWBC), 0, *[_ptr(d[k]) for k in ORDER], _ptr(slot))
    if with_wbc:      # the MPC half leaves the WBC fields alone (another launch, on another stream, writes them) ...
        half = np.frombuffer(slot.tobytes()[:B * L.QM_STEP_BYTES], api.STEP_RECORD)
        assert (half["wbc_out"].view(np.uint8) == 0xA5).all() and (half["qp_status"].view(np.uint8) == 0xA5).all() and np.array_equal(half["n_nodes"], d["n_nodes"])
        before = slot.copy(); lib.emu_io_pack(B, nmax, ncap, WBC, 0, *[_ptr(d[k]) for k in ORDER], _ptr(slot))
        diff = np.flatnonzero(before != slot)      # ... and the WBC half writes nothing else
        assert diff.size and diff.max() < B * L.QM_STEP_BYTES and ((diff % L.QM_STEP_BYTES >= 8 * L.QM_STEP_WBC) & (diff % L.QM_STEP_BYTES < 8 * L.QM_STEP_DOUBLES + 4 * (L.QM_STEP_I_QP + 3))).all()
    assert slot.tobytes() == _expected(d, B, ncap, with_wbc, True)
    # without the trajectory part only the records are touched
    slot2 = np.full(nbytes, 0xA5, np.uint8)
    lib.emu_io_pack(B, nmax, ncap, MPC | WBC if with_wbc else MPC | NOWBC, 0, *[_ptr(d[k]) for k in ORDER], _ptr(slot2))
    assert slot2.tobytes()[:B * L.QM_STEP_BYTES] == _expected(d, B, ncap, with_wbc, False) and (slot2[B * L.QM_STEP_BYTES:] == 0xA5).all()


@pytest.mark.parametrize("B,nmax,ncap,n_nodes", CASES[2:4])
@pytest.mark.parametrize("with_wbc,traj", [(True, True), (False, True), (True, False)])
def test_pipeline_roundtrip_hands_over_the_first_n_nodes_only(lib, B, nmax, ncap, n_nodes, with_wbc, traj):
    """pack -> slot -> mirror -> collect over both slots: records as packed; the caller's trajectory arrays [B][max_nodes][k] get nodes 0 .. n_nodes[b] - 1 and keep the rest"""
    rng = np.random.default_rng(B + 7)
    if n_nodes is None:
        n_nodes = rng.integers(3, ncap + 1, B); n_nodes[0] = ncap; n_nodes[-1] = 3
    d = _buffers(rng, B, nmax, n_nodes); nm = nmax + 2
    rec = np.zeros(B, api.STEP_RECORD)
    o = dict(t=np.full((B, nm), -9.5), ev=np.full((B, nm), -77, np.int32), mode=np.full((B, nm), -77, np.int32), x=np.full((B, nm, 30), -9.5), u=np.full((B, nm, 30), -9.5))
    outs = [_ptr(o[k]) if traj else None for k in ("t", "ev", "mode", "x", "u")]
    rc = lib.emu_io_roundtrip(B + 3, B, nmax, ncap, int(with_wbc), int(traj), 0, *[_ptr(d[k]) for k in ORDER], _ptr(rec), nm, *outs)
    assert rc == 3 * (2 if with_wbc else 1)      # nothing left in flight; launches per step: MPC half (+ WBC half)
    assert rec.tobytes() == _expected(d, B, ncap, with_wbc, False)
    for b, n in enumerate(d["n_nodes"]):
        for k, src in (("t", "node_t"), ("ev", "node_ev"), ("mode", "node_mode"), ("x", "xs"), ("u", "us")):
            if traj:
                assert np.array_equal(o[k][b, :n], d[src][:n, b]), (k, b)
            assert (o[k][b, n if traj else 0:] == (-9.5 if o[k].dtype == np.float64 else -77)).all(), (k, b)


def test_record_layout_matches_header_and_python(lib):
    assert lib.emu_io_record_bytes() == 1024 == L.QM_STEP_BYTES == api.STEP_RECORD.itemsize == 8 * L.QM_STEP_DOUBLES + 4 * L.QM_STEP_INTS
    names = ["x_des", "u_des", "wbc_out", "perf", "mode", "mpc_status", "n_nodes", "qp_status", "reserved"]
    assert [f[0] for f in L.STEP_RECORD_FIELDS] == names
    for k, name in enumerate(names):
        assert lib.emu_io_record_offset(k) == api.STEP_RECORD.fields[name][1] == L.STEP_RECORD_FIELDS[k][3], name
    assert (L.QM_STEP_XDES, L.QM_STEP_UDES, L.QM_STEP_WBC, L.QM_STEP_PERF, L.QM_STEP_DOUBLES) == (0, 30, 60, 114, 124)
    assert api.STEP_RECORD["wbc_out"].shape == (54,) and api.STEP_RECORD["qp_status"].shape == (3,)


NAN = float("nan")
STATUS_TABLE = [  # (K0 status, step_info[4], strict, expected) — the cases of qm_mpc_status' comment (csrc/host/qm_pipeline.h)
    (0, [0.5, 1.0, 2.0, 0.0], 0, 0), (0, [0.5, 1.0, 2.0, 0.0], 1, 0),                        # ok
    (-1, [0.5, 1.0, 2.0, 0.0], 0, -1), (-2, [NAN, 1.0, 2.0, 3.0], 0, -2), (-3, [0.5, 1.0, 2.0, 1.0], 1, -3),      # K0's codes pass through
    (0, [0.5, 1.0, 2.0, 1.0], 0, L.QM_MPC_WARN_PIVOT), (0, [0.5, 1.0, 2.0, 1.0], 1, -4),    # pivot bit 0: warning, failure with ST_RICCATI_STRICT
    (0, [0.5, 1.0, 2.0, 2.0], 0, -4), (0, [0.5, 1.0, 2.0, 3.0], 0, -4),                      # pivot bit 1
    (0, [0.5, 1.0, 2.0, NAN], 0, -4),                                                        # a pivot that is not a number
    (0, [NAN, 1.0, 2.0, 0.0], 0, -4), (0, [0.5, float("inf"), 2.0, 0.0], 0, -4), (0, [0.5, 1.0, NAN, 1.0], 0, -4),      # NaN / infinite step
]


def test_mpc_status_device_and_host_agree(lib):
    B = len(STATUS_TABLE); rng = np.random.default_rng(5)
    for strict in (0, 1):
        rows = [r for r in STATUS_TABLE if r[2] == strict]; B = len(rows)
        d = _buffers(rng, B, 4, [3] * B)
        d["status"] = np.array([r[0] for r in rows], np.int32); d["step_info"] = np.array([r[1] for r in rows], float)
        slot = np.zeros(lib.emu_io_slot_bytes(B, 3, 0), np.uint8)
        lib.emu_io_pack(B, 4, 3, MPC | NOWBC, strict, *[_ptr(d[k]) for k in ORDER], _ptr(slot))
        dev = np.frombuffer(slot.tobytes(), api.STEP_RECORD)["mpc_status"]
        host = [lib.emu_io_status_host(int(r[0]), _ptr(np.array(r[1], float)), strict) for r in rows]
        assert list(dev) == host == [r[3] for r in rows], (strict, list(dev), host)
