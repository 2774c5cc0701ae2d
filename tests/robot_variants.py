"""tests/robot_variants.py — TEST INFRASTRUCTURE: perturbed copies of the shipped robot and their blobs, shared by tests/test_robot_variants.py (host emulator) and
tests/test_gpu_robot_variants.py (device).

Every other test runs on what the two ingestions make of tests/data/robot.urdf, and that robot is special: JR = I on all twelve leg joints, every joint axis a coordinate
axis, FR = I and FP = (0, 0, -0.25) on the four feet, diagonal arm inertias, mirror-image legs, exact zeros in JP and COM.  The device code reads MB_JR, MB_AXIS, MB_FP and
MB_FR as if they were general.  write_variant() rewrites the URDF so that none of that structure is left (each item is one block of _perturb below); names, tree, joint
limits, task.info and reference.info stay as they are, so every problem of qm_control_amd.scenarios is a problem of the variant too.

    a = angle scale [rad], l = length scale [m], U = uniform(-1, 1), drawn from numpy.random.default_rng(seed of the variant) in document order:
      <origin> of every revolute joint, of the four *_foot_fixed joints and of the end effector's fixed joint:  rpy += a U^3, xyz += l U^3    (JR, JP, FR, FP: general)
      <axis>   of every revolute joint:                                 xyz += a U^3, then normalised to unit length                          (no coordinate axis)
      <mass>   of every link:                                           value *= uniform(0.7, 1.4), independently per link                     (no left / right symmetry)
      <inertia> of every link:                                          ixy, ixz, iyz += 0.2 min(ixx, iyy, izz) U each                         (no diagonal tensor)
    The added products of inertia are small against the diagonal (0.2 of its smallest entry), so the tensors stay positive definite; test_robot_variants.py asserts
    that for every body of every variant.

The committed URDF is not touched (its sha256 is pinned); the variants are written to a temporary directory of the process."""
import atexit
import functools
import os
import shutil
import tempfile
import xml.etree.ElementTree as ET

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(_HERE, "data")
URDF, TASK, REFI = (os.path.join(DATA, f) for f in ("robot.urdf", "task.info", "reference.info"))

# name -> (angle scale a [rad], length scale l [m], seed).  A seed is replaced, never a bound, when the ORACLE alone does not solve the configurations of the tests cleanly
# on the variant (test_robot_variants.test_oracle_solves_every_configuration_cleanly) or a line-search decision is a near tie
VARIANTS = {"mild": (0.05, 0.005, 101), "skew": (0.15, 0.02, 102), "strong": (0.4, 0.03, 103)}
EE_JOINT = "j2n6s300_joint_end_effector"
FOOT_JOINTS = ("LF_foot_fixed", "RF_foot_fixed", "LH_foot_fixed", "RH_foot_fixed")


def _vec(s):
    return np.array([float(v) for v in s.split()])


def _fmt(v):
    return " ".join(repr(float(x)) for x in v)


def _perturb(root, a, l, rng):
    U = lambda n=None: rng.uniform(-1.0, 1.0, n)
    for j in root.findall("joint"):
        revolute = j.get("type") in ("revolute", "continuous")
        if revolute or j.get("name") in FOOT_JOINTS or j.get("name") == EE_JOINT:
            o = j.find("origin")
            if o is None:
                o = ET.SubElement(j, "origin", {"rpy": "0 0 0", "xyz": "0 0 0"})
            o.set("rpy", _fmt(_vec(o.get("rpy", "0 0 0")) + a * U(3))); o.set("xyz", _fmt(_vec(o.get("xyz", "0 0 0")) + l * U(3)))
        if revolute:
            ax = j.find("axis"); v = _vec(ax.get("xyz")) + a * U(3); ax.set("xyz", _fmt(v / np.linalg.norm(v)))
    for k in root.findall("link"):
        ine = k.find("inertial")
        if ine is None:
            continue
        m = ine.find("mass"); m.set("value", repr(float(m.get("value")) * rng.uniform(0.7, 1.4)))
        i = ine.find("inertia"); d = min(float(i.get(n)) for n in ("ixx", "iyy", "izz"))
        for n in ("ixy", "ixz", "iyz"):
            i.set(n, repr(float(i.get(n)) + 0.2 * d * U()))


def write_variant(name, out_dir):
    """the URDF of variant `name` in out_dir; the same bytes on every call"""
    a, l, seed = VARIANTS[name]
    tree = ET.parse(URDF)
    _perturb(tree.getroot(), a, l, np.random.default_rng(seed))
    path = os.path.join(out_dir, "robot_%s.urdf" % name)
    tree.write(path)
    return path


_dir = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="qm_robot_variants_"); atexit.register(shutil.rmtree, _dir, True)
    return _dir


@functools.lru_cache(maxsize=None)
def urdf(name):
    return write_variant(name, _tmp())


@functools.lru_cache(maxsize=None)
def blobs(name):
    """(model, settings) of the variant from the PRODUCT's ingestion (qmhip_parse_model: host code of libqmhip.so, no GPU needed)"""
    from qm_control_amd import api
    return api.parse_model(urdf(name), TASK, REFI)


@functools.lru_cache(maxsize=None)
def oracle_blobs(name):
    """(model, settings) of the variant from the numpy front-end (oracle/front.py): what the oracle runs on — no common-mode model input, as with the session fixtures
    `blobs` and `oblobs`"""
    import front
    mb, _ = front.build_model(urdf(name), REFI)
    return mb, front.build_settings(TASK, mb)


@functools.lru_cache(maxsize=None)
def oracle(name):
    import pyoracle
    return pyoracle.Oracle(*oracle_blobs(name))
