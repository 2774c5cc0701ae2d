"""tests/devprim_harness.py — TEST INFRASTRUCTURE: builds and binds the device-primitive test kernels (tests/devprim): the gfx950 library tests/_build/libqm_devprim.so
(hipcc with exactly qm_control_amd/build_flags.HIPCC_FLAGS — the vectorizer switch and the contraction default are part of what is tested) and the two host-emulator
libraries of tests/emu_prim (exact estimates / estimates wrong by 2^-EST_BITS).  All three export the same entry points (tests/devprim/devprim.hip)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEVICE_LIB = os.path.join(_HERE, "_build", "libqm_devprim.so")
_SOURCES = ["tests/devprim/devprim.hip", "tests/devprim/devprim_kernels.h", "qm_control_amd/csrc/kernels/qm_dev_common.h", "include/qmhip_layout.h"]

SCALAR_OPS = ["rcp", "rsq", "frcp", "log", "sincos", "recip", "rsqrt", "rsqrt_n2", "givens", "house", "barrier_val", "barrier_d12", "rot_zyx_fast", "rot_zyx_lib",
              "euler_E_fast", "rot_axis_fast"]      # order of the enum in devprim_kernels.h
SCALAR_NOUT = dict(rcp=1, rsq=1, frcp=1, log=1, sincos=2, recip=1, rsqrt=1, rsqrt_n2=1, givens=2, house=4, barrier_val=1, barrier_d12=2, rot_zyx_fast=9, rot_zyx_lib=9,
                   euler_E_fast=9, rot_axis_fast=9)
WAVE_OPS = ["wave_sum", "wave_max", "bcast", "dpp0_111", "dpp0_112", "dpp0_114", "dpp0_118", "dpp_142_a", "dpp_143_c", "dpp_111_f", "dpp_112_f", "dpp_114_f", "dpp_118_f"]

_dp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)


def _stamp():
    from qm_control_amd.build_flags import HIPCC_FLAGS
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for s in _SOURCES:
        h.update(open(os.path.join(ROOT, s), "rb").read())
    return h.hexdigest()


def device_lib_stale():
    """the library is current when its stamp file holds the hash of its sources and flags (a hash, not a time: copying the tree must not make it stale)"""
    try:
        return not os.path.exists(DEVICE_LIB) or open(DEVICE_LIB + ".stamp").read() != _stamp()
    except OSError:
        return True


def build_device_lib(force=False):
    """tests/_build/libqm_devprim.so for gfx950 (cross-compiles without a GPU); raises when it is stale and cannot be built"""
    if not force and not device_lib_stale():
        return DEVICE_LIB
    from qm_control_amd.build_flags import HIPCC_FLAGS
    if not os.path.exists(HIPCC):
        raise RuntimeError("tests/_build/libqm_devprim.so is missing or stale and there is no hipcc to build it")
    os.makedirs(os.path.dirname(DEVICE_LIB), exist_ok=True)
    subprocess.check_call([HIPCC] + HIPCC_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "devprim", "devprim.hip"), "-o", DEVICE_LIB], cwd=ROOT)
    with open(DEVICE_LIB + ".stamp", "w") as f:
        f.write(_stamp())
    return DEVICE_LIB


def build_emu_libs(est_bits):
    d = os.path.join(_HERE, "emu_prim")
    subprocess.check_call(["make", "-C", d, "-s", "EST_BITS=%d" % est_bits])
    return os.path.join(d, "_build", "libqm_emu_prim.so"), os.path.join(d, "_build", "libqm_emu_prim_est%d.so" % est_bits)


def _f(a):
    return np.ascontiguousarray(a, np.float64)


class Prim:
    """one of the three libraries.  kind: "gpu", "emu" (exact estimates) or "emu_est" (estimates wrong by 2^-est_bits, sign mode est_sign: 0 alternating, +1, -1)"""

    def __init__(self, path, kind, est_sign=0):
        self.lib = C.CDLL(path); self.kind = kind; self.est_sign = est_sign; self.path = path
        if kind == "emu_est":
            self.lib.emu_prim_est_sign(C.c_int(est_sign))
        self.label = kind + ("" if kind != "emu_est" else {0: "_alt", 1: "_plus", -1: "_minus"}[est_sign])

    def _select(self):
        if self.kind == "emu_est":      # (the sign mode is a global of the library: instances with different modes share it)
            self.lib.emu_prim_est_sign(C.c_int(self.est_sign))

    @staticmethod
    def _ok(rc, what):
        assert rc == 0, "%s: error %d from the runtime / argument check" % (what, rc)

    def device_name(self):
        b = C.create_string_buffer(256); self._ok(self.lib.dp_device_name(b, 256), "dp_device_name"); return b.value.decode()

    def scalar(self, op, *ins):
        """op(ins[0][i], ins[1][i], ...) for every i -> list of output arrays"""
        self._select(); x = _f(np.stack([_f(a) for a in ins])); n = x.shape[1]; nout = SCALAR_NOUT[op]; out = np.full((nout, n), np.nan)
        self._ok(self.lib.dp_scalar(SCALAR_OPS.index(op), n, len(ins), nout, x.ctypes.data_as(_dp), out.ctypes.data_as(_dp)), op)
        return list(out)

    def wave(self, op, v, old=None, src=0):
        """v, old: [nwaves][64] float64 (bit patterns travel untouched), nwaves a multiple of 4 -> every lane's result, same shape"""
        v = _f(v); old = _f(np.zeros_like(v) if old is None else old); assert v.shape[1] == 64 and v.shape[0] % 4 == 0 and old.shape == v.shape
        out = np.zeros_like(v)
        self._ok(self.lib.dp_wave(WAVE_OPS.index(op), src, v.shape[0] // 4, old.ctypes.data_as(_dp), v.ctypes.data_as(_dp), out.ctypes.data_as(_dp)), op)
        return out

    def rows(self, W, nrows, nblocks, stride, src, vals, dst, dst_off, mask):
        lanes = np.full((64 * nblocks, W), np.nan); src = _f(src); vals = _f(vals); mask = np.ascontiguousarray(mask, np.uint64); assert dst.dtype == np.float64 and dst.flags.c_contiguous
        assert src.size == max(nrows, 1) * W and vals.shape == lanes.shape and mask.size == nblocks
        self._ok(self.lib.dp_rows(W, C.c_long(nrows), nblocks, C.c_long(stride), src.ctypes.data_as(_dp), lanes.ctypes.data_as(_dp), vals.ctypes.data_as(_dp), dst.ctypes.data_as(_dp),
                                  C.c_long(dst.size), C.c_long(dst_off), mask.ctypes.data_as(_up)), "rows")
        return lanes

    def wg_gemm(self, ta, tb, block, A, B, mt, nt, ks0, ks1, C0):
        A = _f(A); B = _f(B); Cc = _f(C0).copy(); calls = np.zeros((32, 32), np.int32); assert A.shape == (32, 34) and B.shape == (32, 34) and Cc.shape == (32, 32)
        self._ok(self.lib.dp_wg_gemm(int(ta), int(tb), block, A.ctypes.data_as(_dp), B.ctypes.data_as(_dp), mt, nt, ks0, ks1, Cc.ctypes.data_as(_dp), calls.ctypes.data_as(_ip)), "wg_gemm")
        return Cc, calls

    def frag(self, tr, stream, tile, src, ld, rows, cols, dst, dst_off, ldd):
        src = _f(src).ravel(); regs = np.full((16, 64), np.nan); assert dst.dtype == np.float64 and dst.flags.c_contiguous
        self._ok(self.lib.dp_frag(int(tr), int(stream), int(tile), src.ctypes.data_as(_dp), C.c_long(src.size), ld, rows, cols, regs.ctypes.data_as(_dp), dst.ctypes.data_as(_dp),
                                  C.c_long(dst.size), C.c_long(dst_off), ldd), "frag")
        return regs

    def gemm_tn(self, shape, Z, Y, P, k0, k1, neg):
        kt, it, jt = shape; Z = _f(Z); Y = _f(Y); P = _f(P).copy(); assert Z.shape == (16 * kt, 16 * it) and Y.shape == (16 * kt, 16 * jt) and P.shape == (16 * it, 16 * jt)
        self._ok(self.lib.dp_gemm_tn(kt, it, jt, Z.ctypes.data_as(_dp), Y.ctypes.data_as(_dp), P.ctypes.data_as(_dp), k0, k1, int(neg)), "gemm_tn")
        return P

    def dma(self, mode, g, g_off, lds_at, fill):
        g = _f(g); out = np.zeros(1024)
        self._ok(self.lib.dp_dma(mode, g.ctypes.data_as(_dp), C.c_long(g.size), C.c_long(g_off), lds_at, C.c_double(fill), out.ctypes.data_as(_dp)), "dma")
        return out

    def dense(self, block, src, rows, cols, dld, x, fill, dst, dst_off, m3):
        src = _f(src); x = _f(x); m3 = _f(m3); tile = np.zeros((32, 34)); rd = np.full(32, np.nan); cd = np.full(32, np.nan); m3out = np.full(24, np.nan)
        assert src.shape[0] == rows and x.size == 32 and m3.size == 24 and dst.dtype == np.float64
        self._ok(self.lib.dp_dense(block, src.ctypes.data_as(_dp), rows, cols, src.shape[1], dld, x.ctypes.data_as(_dp), C.c_double(fill), tile.ctypes.data_as(_dp), dst.ctypes.data_as(_dp),
                                   C.c_long(dst.size), C.c_long(dst_off), rd.ctypes.data_as(_dp), cd.ctypes.data_as(_dp), m3.ctypes.data_as(_dp), m3out.ctypes.data_as(_dp)), "dense")
        return tile, rd, cd, m3out


def emu_libs(est_bits):
    """the emulator libraries: exact estimates, and the degraded ones with alternating / fixed + / fixed - error"""
    exact, est = build_emu_libs(est_bits)
    return [Prim(exact, "emu"), Prim(est, "emu_est", 0), Prim(est, "emu_est", 1), Prim(est, "emu_est", -1)]


def device_lib():
    """the gfx950 library; a missing or stale one is rebuilt, and a failure to do so is an error (never a skip)"""
    return Prim(build_device_lib(), "gpu")
