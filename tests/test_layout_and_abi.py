"""Layout constants, C-ABI exports and host-only behaviour of libqmhip.so (no GPU needed)."""
import ctypes as C
import os
import re
import numpy as np
from qm_control_amd import layout as L
import pytest
from conftest import ROOT


def _defines(path):
    d = {}
    for line in open(path):
        m = re.match(r"#define\s+(\w+)\s+(\d+)\b", line)
        if m:
            d[m.group(1)] = int(m.group(2))
    return d


def test_front_layout_matches_header():
    import front
    d = _defines(os.path.join(ROOT, "include", "qmhip_layout.h"))
    for k, v in front.MB.items():
        assert d["MB_" + k] == v, k
    for k, v in front.ST.items():
        assert d["ST_" + k] == v, k
    assert d["QM_NX"] == 30 and d["QM_NU"] == 30 and d["QM_NREF"] == 37 and d["QM_NRBD"] == 55


def test_library_exports_every_declared_symbol():
    from qm_control_amd import api
    hdr = open(os.path.join(ROOT, "include", "qmhip.h")).read()
    declared = sorted(set(re.findall(r"\b(qmhip_\w+)\s*\(", hdr)))
    assert len(declared) >= 20
    lib = api.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(api.EXPORTS) == [n for n in declared if n in api.EXPORTS]
    assert set(api.EXPORTS) == set(declared)


def test_no_cpu_fallback_without_device(blobs):
    """the product path must fail loudly when no HIP device is present"""
    import os, torch
    if torch.cuda.is_available() or os.path.exists("/dev/kfd"):       # (torch can be blind to a device this process has hidden from it; the kernel driver node is not)
        pytest.skip("a GPU is present")
    from qm_control_amd import api
    with pytest.raises(api.QmhipError):
        api.QMInterface(blobs=blobs, max_batch=1, max_nodes=16)


def test_missing_files_raise_like_the_reference():
    from qm_control_amd import api
    with pytest.raises(ValueError, match="Task file not found"):
        api.parse_model("/nonexistent/robot.urdf", "/nonexistent/task.info", "/nonexistent/reference.info")


DATA = os.path.join(ROOT, "tests", "data")
INPUTS = [os.path.join(DATA, f) for f in ("robot.urdf", "task.info", "reference.info")]


def test_product_blobs_come_from_the_product_parser(blobs):
    """the blobs the product runs on (qm_control_amd/data) are bit-equal to what its own C++ ingestion (qmhip_parse_model) makes of the shipped input files"""
    from qm_control_amd import api
    mb, st = api.parse_model(*INPUTS)
    assert np.array_equal(mb, blobs[0]) and np.array_equal(st, blobs[1])
    assert abs(mb[L.MB_ROBOTMASS] - 27.371574) < 1e-9                         # total mass
    with pytest.raises(ValueError, match="URDF file not found"):
        api.parse_model("/nonexistent/robot.urdf", INPUTS[1], INPUTS[2])


def test_oracle_blobs_come_from_the_numpy_front_end_and_check_the_product(blobs, oblobs):
    """the oracle's blobs (oracle/data) are bit-equal to a fresh run of the independent numpy front-end, and the two ingestions agree to round-off"""
    import front
    mb, _ = front.build_model(INPUTS[0], INPUTS[2])
    st = front.build_settings(INPUTS[1], mb)
    assert np.array_equal(mb, oblobs[0]) and np.array_equal(st, oblobs[1])
    assert np.abs(blobs[0] - oblobs[0]).max() <= 1e-13 and np.abs(blobs[1] - oblobs[1]).max() <= 1e-13
    # everything the integer / event-time path reads from the settings is the same f64 in both
    for k in ("SQP_DT", "PHASE_TRANS_STANCE", "TIME_HORIZON", "SWING_TIME_SCALE"):
        assert blobs[1][front.ST[k]] == oblobs[1][front.ST[k]], k


GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_shipped_inputs_and_gaits_are_the_reference_files():
    """tests/data holds the reference's input files byte for byte (their sha256, recorded from the reference tree in tests/golden/reference_inputs.json), and the
    shipped trot template is the one of the reference's gait.info (a copy: tests/golden/reference_gait.info)"""
    import hashlib, json, front
    from qm_control_amd import scenarios
    rec = json.load(open(os.path.join(GOLDEN, "reference_inputs.json")))["files"]
    for a in INPUTS:
        assert hashlib.sha256(open(a, "rb").read()).hexdigest() == rec[os.path.basename(a)]["sha256"], a
    times, modes = front.load_gait(os.path.join(GOLDEN, "reference_gait.info"), "trot")
    g = scenarios.load_gaits()["trot"]
    assert times == g["switchingTimes"] and modes == g["modeSequence"]


def test_create_rejects_bad_sizes(blobs):
    """argument validation happens before any device work (qmhip.h: 3 <= max_nodes <= 512)"""
    from qm_control_amd import api
    for bad in (2, 513):
        with pytest.raises(api.QmhipError, match="bad argument"):
            api.QMInterface(blobs=blobs, max_batch=1, max_nodes=bad)


def test_wbc_gain_names_of_the_reconfigure_server():
    """qmhip_wbc_gain_index: every field WbcBase::dynamicCallback reads (qm_wbc/src/WbcBase.cpp:69-116; declared in qm_wbc/cfg/wbcWigeht.cfg:7-47) maps to its settings
    slot, the six fields it does not read (d_ee_*, da_ee_*) and unknown names map to -1.  Host-only entry point: no GPU needed."""
    import ctypes as C
    from qm_control_amd import api, layout as L
    lib = api.load_library(); f = lib.qmhip_wbc_gain_index; f.restype = C.c_int; f.argtypes = [C.c_char_p]
    want = {"kp_swing": L.ST_KP_SWING, "kd_swing": L.ST_KD_SWING, "baseHeightKp": L.ST_KP_BASE_H, "baseHeightKd": L.ST_KD_BASE_H, "kp_base_linear": L.ST_KP_BASE_LIN,
            "kd_base_linear": L.ST_KD_BASE_LIN, "kp_base_angular": L.ST_KP_BASE_ANG, "kd_base_angular": L.ST_KD_BASE_ANG}
    for j in range(6):
        want["kp_arm_joint_%d" % (j + 1)] = L.ST_KP_ARM_J + j; want["kd_arm_joint_%d" % (j + 1)] = L.ST_KD_ARM_J + j
    for a, ax in enumerate("xyz"):
        want["kp_ee_linear_" + ax] = L.ST_KP_EE_LIN + a; want["kd_ee_linear_" + ax] = L.ST_KD_EE_LIN + a
        want["kp_ee_angular_" + ax] = L.ST_KP_EE_ANG + a; want["kd_ee_angular_" + ax] = L.ST_KD_EE_ANG + a
    assert len(want) == 32 and len(set(want.values())) == 32
    for name, idx in want.items():
        assert f(name.encode()) == idx, name
    for name in ("d_ee_x", "d_ee_y", "d_ee_z", "da_ee_z", "da_ee_y", "da_ee_x", "kp_arm_joint_7", "kp_arm_joint_0", "kp_ee_linear_w", "kp_swing_", "", "kp_arm_joint_11"):
        assert f(name.encode()) == -1, name
    assert f(None) == -1
    # the reference's cfg file declares exactly these names + the six unread ones, with the blob's defaults (its declarations, recorded in tests/golden/reference_wbc_gains.json)
    import json
    from qm_control_amd import scenarios
    st = scenarios.load_blobs()[1]
    decl = dict((p["name"], float(p["default"])) for p in json.load(open(os.path.join(ROOT, "tests", "golden", "reference_wbc_gains.json")))["parameters"])
    assert set(want) <= set(decl) and len(decl) == 38
    for name, idx in want.items():
        assert st[idx] == decl[name], name
