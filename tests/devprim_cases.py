"""tests/devprim_cases.py — inputs, references and checks of the device-primitive tests, shared by tests/test_emu_devprim.py (host emulator, exact and degraded
estimates) and tests/test_gpu_devprim.py (gfx950).  Every check takes a devprim_harness.Prim and asserts; CHECKS lists them.

References: numpy long double (x87: 64-bit significand) for everything rounded, exact integer arithmetic or a numpy restatement of the documented operation order
for everything that must be bit-equal.  No bound here was fitted to what a kernel returned: each is the one the project already stated (tests/test_device_math.py)
or is derived in the docstring of its check from the roundings of the operation sequence in qm_dev_common.h."""
import math
import os
import re
import numpy as np

EST_BITS = 24      # claimed accuracy of v_rcp_f64 / v_rsq_f64 on gfx950: relative error <= 2^-EST_BITS.  The degraded emulator library is wrong by exactly this much
                   # and the GPU test asserts the hardware is no worse and writes what it measured to tests/_build/devprim_estimates.json
U = 2.0 ** -53     # one rounding
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRCP_BOUND, LOG_BOUND = 4.5e-16, 1e-15      # the bounds tests/test_device_math.py states for qm_frcp and qm_log

ESTIMATES = {}      # filled by check_raw_estimates: {"rcp": {...}, "rsq": {...}} (the GPU test writes it to tests/_build/devprim_estimates.json)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_u64(a), _u64(b))


# ---------------------------------------------------------------- (a) scalar maps ----------------------------------------------------------------
def positive_args():
    rng = np.random.default_rng(11); k = np.arange(-400, 401); p2 = np.ldexp(1.0, k)
    return np.concatenate([np.exp2(rng.uniform(-400, 400, 120000)), rng.uniform(0.5, 2.0, 60000), p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf), 10.0 ** rng.uniform(-12, 12, 20000)])


def sincos_args():
    """the two input sets of tests/test_device_math.py"""
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(-s, s, 200000) for s in (1.0, 7.0, 100.0, 9.0e4)] + [np.arange(-40, 41) * (np.pi / 2), np.arange(-40, 41) * (np.pi / 4), [0.0, -0.0, 1e-300, 5e-324]])
    rng = np.random.default_rng(5)
    b = np.concatenate([rng.uniform(-s, s, 100000) for s in (1.0e5, 1.0e7, 2.0e9)] + [[1.0e5, -3.0e7, 2147483647.0, -2147483647.5], np.arange(1, 1300) * 1.0e6 * (np.pi / 2)])
    return a, b


def check_raw_estimates(p):
    """v_rcp_f64 / v_rsq_f64 alone: the maximum relative error is recorded; on the GPU it must not exceed 2^-EST_BITS — the error the degraded emulator library models,
    so that what test_emu_devprim proves about the correction steps covers the hardware.  0, ±inf and the extreme normal numbers are recorded, not asserted."""
    x = positive_args(); xl = x.astype(LD); special = np.array([0.0, -0.0, np.inf, -np.inf, 2.2250738585072014e-308, 1.7976931348623157e308])
    for op, ref in (("rcp", 1 / xl), ("rsq", 1 / np.sqrt(xl))):
        (r,) = p.scalar(op, x); err = np.abs(r / ref - 1); i = int(np.argmax(err)); (s,) = p.scalar(op, special)
        ESTIMATES[op] = {"max_rel_err": float(err[i]), "max_rel_err_log2": float(np.log2(max(float(err[i]), 1e-300))), "at": float(x[i]), "at_hex": float(x[i]).hex(), "n": int(x.size),
                         "special": {repr(float(a)): repr(float(b)) for a, b in zip(special, s)}, "device": p.device_name()}
        print("%s %s: max rel err %.3e = 2^%.2f at %s" % (p.label, op, err[i], ESTIMATES[op]["max_rel_err_log2"], float(x[i]).hex()))
        if p.kind == "gpu":
            assert err[i] <= 2.0 ** -EST_BITS, (op, err[i], x[i])
        elif p.kind == "emu_est":
            assert 2.0 ** -(EST_BITS + 1) < err[i] < 2.0 ** -(EST_BITS - 1), (op, err[i])      # the model is in force


def check_frcp_log_existing_bounds(p):
    """the bounds of tests/test_device_math.py, unchanged: |x qm_frcp(x) - 1| < 4.5e-16, |qm_log - log| <= 1e-15 max(1, |log|)"""
    x = positive_args(); xl = x.astype(LD)
    (r,) = p.scalar("frcp", x); e = np.abs(r * xl - 1).max(); print(p.label, "frcp", float(e)); assert e < FRCP_BOUND, e
    (lg,) = p.scalar("log", x); ref = np.log(xl); e = (np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max(); print(p.label, "log", float(e)); assert e <= LOG_BOUND, e


def check_sincos_existing_bounds(p):
    """the bounds of tests/test_device_math.py, unchanged: 2.5e-16 / 3e-16 absolute on its two input sets, s² + c² - 1 < 5e-16, NaN from 2^31 on"""
    for x, tol in zip(sincos_args(), (2.5e-16, 3e-16)):
        s, c = p.scalar("sincos", x); xl = x.astype(LD); es, ec = np.abs(s - np.sin(xl)).max(), np.abs(c - np.cos(xl)).max(); print(p.label, "sincos", float(es), float(ec))
        assert es < tol and ec < tol, (es, ec, tol)
        if tol == 2.5e-16:
            assert np.abs(s * s + c * c - 1.0).max() < 5e-16
    s, c = p.scalar("sincos", np.array([2147483648.0, -2147483648.0, 1.0e10, -1.0e300, np.inf, -np.inf, np.nan]))
    assert np.isnan(s).all() and np.isnan(c).all()


def check_recip_rsqrt_to_one_ulp(p):
    """qm_recip, qm_rsqrt, qm_rsqrt_n2: relative error <= 2^-52 = one final fma rounding (2^-53) + the residual of the correction (order e³ ≈ 2^-70 for an estimate
    with e <= 2^-23; for the Newton forms the rounding of x·y0 resp. d·inv enters the residual once, halved: 2^-54), with a factor < 2 of margin"""
    x = positive_args(); xl = x.astype(LD)
    for op, ref in (("recip", 1 / xl), ("rsqrt", 1 / np.sqrt(xl)), ("rsqrt_n2", 1 / np.sqrt(xl))):
        (r,) = p.scalar(op, x); e = np.abs(r / ref - 1).max(); print(p.label, op, float(e), "= %.3f x 2^-52" % float(e * 2.0 ** 52)); assert e <= 2.0 ** -52, (op, e)


def givens_args():
    rng = np.random.default_rng(12); n = 200000
    b = np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n); a = np.abs(b) * np.exp2(rng.uniform(-60, 60, n)) * rng.choice([-1.0, 1.0], n)
    z = np.exp2(rng.uniform(-30, 30, 200)) * rng.choice([-1.0, 1.0], 200)
    return np.concatenate([a, z, np.zeros(200), [0.0, -0.0, 3.0, 1.0]]), np.concatenate([b, np.zeros(200), z, [0.0, 0.0, 4.0, 1.0]])


def check_givens(p):
    """c = a r, s = b r with r = qm_rsqrt(fma(a, a, b b)): four roundings (b·b, the fma, the rsqrt's own 1.5 x 2^-53 — halved for the first two — and the product):
    relative error of c and s <= 2^-51; hence |c² + s² - 1| <= 2^-50 and |-s a + c b| <= 2^-50 hypot(a, b).  The null pair gives exactly (1, 0)."""
    a, b = givens_args(); c, s = p.scalar("givens", a, b); al, bl = a.astype(LD), b.astype(LD); h = np.sqrt(al * al + bl * bl); nz = h > 0
    cr, sr = al[nz] / h[nz], bl[nz] / h[nz]; cl, sl = c.astype(LD)[nz], s.astype(LD)[nz]
    ec, es = (np.abs(cl - cr) - 2.0 ** -51 * np.abs(cr)).max(), (np.abs(sl - sr) - 2.0 ** -51 * np.abs(sr)).max(); print(p.label, "givens", float(ec), float(es))
    assert ec <= 0 and es <= 0, (ec, es)
    assert np.abs(cl * cl + sl * sl - 1).max() <= 2.0 ** -50
    assert (np.abs(-sl * al[nz] + cl * bl[nz]) <= 2.0 ** -50 * h[nz]).all()
    assert (c[~nz] == 1.0).all() and (s[~nz] == 0.0).all() and (~nz).sum() == 2


def house_args():
    rng = np.random.default_rng(13); n = 200000
    g = np.exp2(rng.uniform(-10, 10, n)) * rng.choice([-1.0, 1.0], n); t = g * g * np.exp2(rng.uniform(-20, 20, n)); t[::7] = 0.0      # t / g² over 40 binades, and t = 0
    g0 = np.zeros(100); t0 = np.exp2(rng.uniform(-20, 20, 100))                                                                       # g = 0 (positive branch)
    return np.concatenate([g * g + t, t0, [0.0, 0.0]]), np.concatenate([g, g0, [0.0, 1.5]])


def check_house_scalars(p):
    """qm_house_scalars(nrm2, g): |alpha| = sqrt(nrm2) to 2^-52 (rounding of h = x y0 enters halved, 2^-54, + the final fma, 2^-53); sign(alpha) = -sign(g) with g = 0
    positive; vk = g - alpha is one rounding of the returned alpha; b2 (2 |x| (|x| + |g|)) = 2 to a relative 2^-50 (r and q to ≈ 1.5 x 2^-53 each, den = nrm + |g| one
    rounding on top of nrm's 2^-52, the product r q one more: < 7 x 2^-53); a null column returns ok = false and b2 = 0"""
    n2, g = house_args(); al, vk, b2, ok = p.scalar("house", n2, g); pos = n2 > 0; rt = np.sqrt(n2.astype(LD))
    assert (ok[pos] == 1.0).all() and (ok[~pos] == 0.0).all() and (b2[~pos] == 0.0).all() and (~pos).sum() == 2
    e = (np.abs(np.abs(al.astype(LD)) / np.where(pos, rt, 1) - 1))[pos].max(); print(p.label, "house |alpha|", float(e)); assert e <= 2.0 ** -52, e
    assert (np.sign(al[pos]) == np.where(g[pos] > 0, -1.0, 1.0)).all()
    assert _same_bits(vk[pos], g[pos] - al[pos])
    e = (np.abs(b2.astype(LD) * (2 * rt * (rt + np.abs(g.astype(LD)))) - 2) / 2)[pos].max(); print(p.label, "house b2", float(e)); assert e <= 2.0 ** -50, e


def barrier_args():
    """mu and delta of tests/data/task.info (the three relaxed-barrier blocks: mu 0.1 with delta 5.0, 1e-3, 1e-3); h on both sides of delta, at it, its neighbours, negative"""
    txt = open(os.path.join(ROOT, "tests", "data", "task.info")).read()
    mus = sorted({float(v) for v in re.findall(r"^\s*mu\s+(\S+)", txt, re.M)}); deltas = sorted({float(v) for v in re.findall(r"^\s*delta\s+(\S+)", txt, re.M)})
    assert mus == [0.1] and deltas == [1e-3, 5.0], (mus, deltas)
    rng = np.random.default_rng(14); out = []
    for mu in mus:
        for d in deltas:
            h = np.concatenate([d * np.exp2(rng.uniform(-20, 20, 50000)), d * rng.uniform(0.5, 2.0, 40000), -d * np.exp2(rng.uniform(-20, 12, 10000)),
                                [d, np.nextafter(d, 0.0), np.nextafter(d, np.inf), 0.0, -d]])
            out.append((np.full(h.size, mu), np.full(h.size, d), h))
    return [np.concatenate(c) for c in zip(*out)]


def check_barrier(p):
    """barrier_val / barrier_d12 against the closed form.  Operation counts (roundings of 2^-53 each, relative to the magnitude of the terms they act on):
      value, h > delta:  -mu L                                   the logarithm's bound + 1
      value, h <= delta: mu (-L + t²/2 - 1/2), t = (h - 2 delta)(1/delta):  the logarithm's bound + 10 (t: 3; t²/2: 2 x 3 + 1; the two sums and the product: 3), on |L| + t²/2 + 1/2
      d1, h > delta:     -mu inv                                 qm_frcp's bound + 1
      d1, h <= delta:    mu (h - 2 delta) (inv inv)              2 x qm_frcp's bound + 4
      d2:                mu (inv inv)                            2 x qm_frcp's bound + 2"""
    mu, d, h = barrier_args(); ml, dl, hl = mu.astype(LD), d.astype(LD), h.astype(LD); inn = h > d
    L = np.log(np.where(inn, hl, dl)); t = (hl - 2 * dl) / dl
    (v,) = p.scalar("barrier_val", mu, d, h); ref = np.where(inn, -ml * L, ml * (-L + 0.5 * t * t - 0.5))
    bound = ml * (LOG_BOUND * np.maximum(1, np.abs(L)) + np.where(inn, 1 * U * np.abs(L), 10 * U * (np.abs(L) + 0.5 * t * t + 0.5)))
    print(p.label, "barrier_val", float((np.abs(v - ref) / bound).max())); assert (np.abs(v - ref) <= bound).all()
    d1, d2 = p.scalar("barrier_d12", mu, d, h); inv = 1 / np.where(inn, hl, dl)
    r1 = np.where(inn, -ml * inv, ml * (hl - 2 * dl) * inv * inv); r2 = ml * inv * inv
    b1 = np.abs(r1) * np.where(inn, FRCP_BOUND + U, 2 * FRCP_BOUND + 4 * U); b2 = np.abs(r2) * (2 * FRCP_BOUND + 2 * U)
    print(p.label, "barrier_d12", float((np.abs(d1 - r1) / np.maximum(b1, 1e-300)).max()), float((np.abs(d2 - r2) / b2).max()))
    assert (np.abs(d1 - r1) <= b1).all() and (np.abs(d2 - r2) <= b2).all()


def _rot_refs(z, y, x):
    sz, cz, sy, cy, sx, cx = np.sin(z), np.cos(z), np.sin(y), np.cos(y), np.sin(x), np.cos(x)
    return np.array([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx])


def _orth_err(R):
    M = np.moveaxis(R.astype(LD).reshape(3, 3, -1), 2, 0); return np.abs(M @ np.swapaxes(M, 1, 2) - np.eye(3, dtype=LD)).max()


def check_rotations(p):
    """rot_zyx<true / false>, euler_E<true>, rot_axis_angle<true>: entries within 4 x 2^-52 absolute of long double, R Rᵀ - I within 8 x 2^-52 — the one place where the
    library sin / cos path and qm_sincos are evaluated side by side on the device"""
    rng = np.random.default_rng(15); n = 200000; z, y, x = (np.concatenate([rng.uniform(-7, 7, n // 2), rng.uniform(-100, 100, n // 2)]) for _ in range(3)); zl, yl, xl = (a.astype(LD) for a in (z, y, x))
    ref = _rot_refs(zl, yl, xl)
    for op in ("rot_zyx_fast", "rot_zyx_lib"):
        R = np.array(p.scalar(op, z, y, x)); e, o = np.abs(R - ref).max(), _orth_err(R); print(p.label, op, float(e) * 2 ** 52, float(o) * 2 ** 52); assert e <= 4 * 2.0 ** -52 and o <= 8 * 2.0 ** -52, (op, e, o)
    E = np.array(p.scalar("euler_E_fast", z, y)); sz, cz, sy, cy = np.sin(zl), np.cos(zl), np.sin(yl), np.cos(yl); o_, l_ = np.zeros(n, LD), np.ones(n, LD)
    e = np.abs(E - np.array([o_, -sz, cy * cz, o_, cz, cy * sz, l_, o_, -sy])).max(); print(p.label, "euler_E", float(e) * 2 ** 52); assert e <= 4 * 2.0 ** -52, e
    # axes: the first half signed coordinate axes (|a| = 1 exactly: what the joint axes of the model are), the rest normalised random vectors (|a|² = 1 + O(2^-52): the
    # long-double Rodrigues matrix of such an axis is itself off orthogonality by a few 2^-52, so R Rᵀ - I is asserted on the exactly-unit half only; the entries on all)
    ax = rng.normal(size=(3, n)); ax /= np.linalg.norm(ax, axis=0); ax[:, :n // 2] = np.eye(3)[rng.integers(0, 3, n // 2)].T * rng.choice([-1.0, 1.0], n // 2); q = z; a = ax.astype(LD); s, c = np.sin(zl), np.cos(zl); oc = 1 - c
    ref = np.array([c + oc * a[0] * a[0], oc * a[0] * a[1] - s * a[2], oc * a[0] * a[2] + s * a[1], oc * a[1] * a[0] + s * a[2], c + oc * a[1] * a[1], oc * a[1] * a[2] - s * a[0],
                    oc * a[2] * a[0] - s * a[1], oc * a[2] * a[1] + s * a[0], c + oc * a[2] * a[2]])
    R = np.array(p.scalar("rot_axis_fast", ax[0], ax[1], ax[2], q)); e, o = np.abs(R - ref).max(), _orth_err(R[:, :n // 2]); print(p.label, "rot_axis", float(e) * 2 ** 52, float(o) * 2 ** 52)
    assert e <= 4 * 2.0 ** -52 and o <= 8 * 2.0 ** -52, (e, o)


# ---------------------------------------------------------------- (b) wave reductions, broadcasts, DPP steps ----------------------------------------------------------------
# All of these run under a FULL exec mask (whole 256-thread blocks, no lane leaves before the call), as in the kernels.  256 waves = 64 blocks x 4: waves 1-3 of a block too.
NW = 256
_POS = np.arange(64) & 15


def _shr(v, n, fill):
    """row_shr:n inside the 16-lane rows; lanes shifted in from outside the row take `fill` (an array: per lane)"""
    out = np.array(fill, copy=True); m = _POS >= n; out[:, m] = v[:, np.arange(64)[m] - n]; return out


def _bcast15(v, old):      # row_bcast:15, row mask 0xa: rows 1 and 3 take lane 15 of the row before
    out = np.array(old, copy=True); out[:, 16:32] = v[:, 15:16]; out[:, 48:64] = v[:, 47:48]; return out


def _bcast31(v, old):      # row_bcast:31, row mask 0xc: rows 2 and 3 take lane 31
    out = np.array(old, copy=True); out[:, 32:64] = v[:, 31:32]; return out


def wave_sum_tree(v):
    """the documented order of qm_wave_sum in float64: prefix sums inside the rows by shifts 1, 2, 4, 8 (zeros shifted in), rows 1 and 3 add lane 15 of the row before,
    rows 2 and 3 add lane 31, lane 63 is read"""
    v = np.array(v, np.float64); z = np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in (1, 2, 4, 8):
            v = v + _shr(v, n, z)
        v = v + _bcast15(v, z); v = v + _bcast31(v, z)
    return v[:, 63]


def wave_sum_inputs():
    rng = np.random.default_rng(21); v = rng.normal(size=(NW, 64)) * np.exp2(rng.integers(-30, 30, (NW, 64)))
    v[:64] = 0.0; v[np.arange(64), np.arange(64)] = rng.uniform(1, 2, 64)                       # one non-zero lane, at each position
    v[64:72] = np.where(np.arange(64) % 2 == 0, 1e16, -1e16) + rng.uniform(-1, 1, (8, 64))      # alternating ±1e16 with small terms
    v[72:76] = -0.0
    nan_waves = np.arange(76, 92); v[nan_waves, rng.integers(0, 64, 16)] = np.nan; v[76, 0] = np.nan; v[77, 63] = np.nan
    return v, nan_waves


def check_wave_sum(p):
    """every lane holds the same bits; the value is bit-equal to the float64 restatement of the documented tree and within 64 x 2^-53 x sum|v| of math.fsum; one NaN lane
    makes every lane NaN (NaN payloads are not compared)"""
    v, nan_waves = wave_sum_inputs(); r = p.wave("wave_sum", v); fin = np.ones(NW, bool); fin[nan_waves] = False
    assert (_u64(r) == _u64(r)[:, :1]).all(), "lanes of a wave disagree"
    assert np.isnan(r[nan_waves]).all()
    assert _same_bits(r[fin, 0], wave_sum_tree(v)[fin]), np.flatnonzero(_u64(r[:, 0]) != _u64(wave_sum_tree(v)))
    assert np.signbit(r[72:76]).all()      # -0.0 everywhere stays -0.0 in lane 63's chain
    for w in np.flatnonzero(fin):
        assert abs(r[w, 0] - math.fsum(v[w])) <= 64 * U * math.fsum(np.abs(v[w])), w


def check_wave_max(p):
    """bit-equal to the maximum; all-negative waves catch a zero shifted in; the maximum sits at each of the 64 lanes; a NaN lane is ignored (fmax)"""
    rng = np.random.default_rng(22); v = rng.normal(size=(NW, 64)) * np.exp2(rng.integers(-30, 30, (NW, 64)))
    v[:64] = -np.abs(v[:64]) - 1.0; v[np.arange(64), np.arange(64)] = -rng.uniform(0.1, 0.9, 64)      # all negative, the maximum at lane w
    v[64:128] = rng.uniform(-5, 5, (64, 64)); v[64 + np.arange(64), np.arange(64)] = 7.0 + np.arange(64)
    nanw = np.arange(128, 144); v[nanw, rng.integers(0, 64, 16)] = np.nan; v[128, 63] = np.nan; v[129, 0] = np.nan; v[130:132] = -np.abs(v[130:132]); v[130, 15] = np.nan; v[131, 31] = np.nan
    r = p.wave("wave_max", v)
    assert (_u64(r) == _u64(r)[:, :1]).all(), "lanes of a wave disagree"
    assert _same_bits(r[:, 0], np.fmax.reduce(v, axis=1)), np.flatnonzero(r[:, 0] != np.fmax.reduce(v, axis=1))


def bit_patterns():
    """64-bit patterns whose two words differ, with NaN payloads (quiet and signalling), subnormals, infinities and both zeros among them"""
    rng = np.random.default_rng(23); b = rng.integers(0, 2 ** 63, (NW, 64), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (NW, 64), dtype=np.uint64)
    sp = np.array([0x7ff8deadbeef0001, 0xfff0000000000001, 0x7ff4000012345678, 0x0000000000000001, 0x000fffffffffffff, 0x800abcde00000001, 0x8000000000000000, 0x7ff0000000000000,
                   0x00000000ffffffff, 0xffffffff00000000], np.uint64)
    b[:, ::7] = sp[(np.arange(NW)[:, None] + np.arange(10)[None, :]) % 10]
    assert ((b >> np.uint64(32)) != (b & np.uint64(0xffffffff))).mean() > 0.9
    return b


def check_bcast(p):
    """qm_bcast(v, src) for every src: all 64 lanes hold lane src's 64 bits"""
    b = bit_patterns(); v = b.view(np.float64)
    for src in range(64):
        r = _u64(p.wave("bcast", v, src=src)); assert (r == b[:, src:src + 1]).all(), src


# every qm_dpp<ctrl, row mask> / qm_dpp0<ctrl> the library instantiates (qm_wave_sum, qm_wave_max, K1b's row sums)
DPP_STEPS = {"dpp0_111": lambda v, o: _shr(v, 1, np.zeros_like(v)), "dpp0_112": lambda v, o: _shr(v, 2, np.zeros_like(v)), "dpp0_114": lambda v, o: _shr(v, 4, np.zeros_like(v)),
             "dpp0_118": lambda v, o: _shr(v, 8, np.zeros_like(v)), "dpp_142_a": _bcast15, "dpp_143_c": _bcast31,
             "dpp_111_f": lambda v, o: _shr(v, 1, o), "dpp_112_f": lambda v, o: _shr(v, 2, o), "dpp_114_f": lambda v, o: _shr(v, 4, o), "dpp_118_f": lambda v, o: _shr(v, 8, o)}


def dpp_instantiations():
    """(ctrl, mask) of every qm_dpp / qm_dpp0 use in the kernel sources, by search"""
    found = set()
    d = os.path.join(ROOT, "qm_control_amd", "csrc", "kernels")
    for f in os.listdir(d):
        txt = open(os.path.join(d, f)).read()
        found |= {"dpp0_%s" % a[2:] for a in re.findall(r"qm_dpp0<(0x[0-9a-f]+)>", txt)} | {"dpp_%s_%s" % (a[2:], b[2:]) for a, b in re.findall(r"qm_dpp<(0x[0-9a-f]+),\s*(0x[0-9a-f]+)>", txt)}
    return found


def check_dpp_steps(p):
    """each DPP step alone against its numpy restatement, on bit patterns (compared as uint64)"""
    assert dpp_instantiations() == set(DPP_STEPS), (dpp_instantiations(), set(DPP_STEPS))
    b = bit_patterns(); v = b.view(np.float64); o = b[::-1, ::-1].copy().view(np.float64)
    for op, ref in DPP_STEPS.items():
        r = p.wave(op, v, old=o); want = ref(b, _u64(o)); assert np.array_equal(_u64(r), want), (op, np.argwhere(_u64(r) != want)[:4])


# ---------------------------------------------------------------- (c) qm_rows_gather / qm_rows_scatter ----------------------------------------------------------------
# A search of the kernel sources (rows_instantiations) finds NO instantiation today: the pair is shared infrastructure without a caller.  The widths below are chosen to
# take every path of the index arithmetic e = 64 t + l -> (e / W, e % W): W = 1 (one pass, r = l), 3 and 30 (W does not divide 64: a pass straddles rows; W + 1 even / odd
# LDS row pitch), 8 (W divides 64).  A width the library starts to use must be added here: check_rows asserts the search result is covered.
ROWS_WIDTHS = [1, 3, 8, 30]


def rows_instantiations():
    d = os.path.join(ROOT, "qm_control_amd", "csrc", "kernels"); found = set()
    for f in os.listdir(d):
        found |= {int(w) for w in re.findall(r"qm_rows_(?:gather|scatter)<\s*(\d+)", open(os.path.join(d, f)).read())}
    return found


def _canary(n, tag):
    return (np.uint64(0x7ff8000000000000) + np.uint64(tag << 32) + np.arange(n, dtype=np.uint64)).view(np.float64)


def check_rows(p):
    """gathered per-lane arrays equal the numpy gather exactly, rows beyond nrows read as zero; the scatter writes exactly the masked rows into a strided destination
    whose every other double (256 on both sides, stride - W between rows, the unmasked rows) is a NaN-pattern canary that must keep its bits"""
    assert ROWS_WIDTHS and rows_instantiations() <= set(ROWS_WIDTHS), rows_instantiations()
    rng = np.random.default_rng(31); nb = 3; masks = [0xffffffffffffffff, 0xaaaaaaaaaaaaaaaa, 1 << 37, 0]
    for W in ROWS_WIDTHS:
        stride = W + 5
        for k, nrows in enumerate((1, 63, 64, 65, 130)):
            src = rng.integers(-1000, 1000, (nrows, W)).astype(float) + 0.25; vals = rng.integers(-1000, 1000, (64 * nb, W)).astype(float) + 0.5
            want = np.zeros((64 * nb, W)); m = min(nrows, 64 * nb); want[:m] = src[:m]
            mask = np.array([masks[(k + b) % 4] for b in range(nb)], np.uint64)
            valid = np.array([sum(1 << r for r in range(64) if 64 * b + r < nrows) for b in range(nb)], np.uint64); mask &= valid      # the caller masks the rows that do not exist
            dst = _canary(512 + 64 * nb * stride, W); before = dst.copy()
            lanes = p.rows(W, nrows, nb, stride, src, vals, dst, 256, mask)
            assert _same_bits(lanes, want), (W, nrows)
            exp = before.copy(); body = exp[256:256 + 64 * nb * stride].reshape(64 * nb, stride)
            for r in range(64 * nb):
                if (int(mask[r // 64]) >> (r % 64)) & 1: body[r, :W] = vals[r]
            assert _same_bits(dst, exp), (W, nrows, np.flatnonzero(_u64(dst) != _u64(exp))[:8])


# ---------------------------------------------------------------- (d) wg_gemm ----------------------------------------------------------------
K_RANGES = [(0, 8), (0, 5), (3, 8), (2, 3), (4, 4)]      # full, head, tail, one slab, empty


def _tile_image(M, transposed, rows, k0, k1):
    """32 x QM_LD image holding op(X)[:rows, k0:k1] (or its transpose) and a NaN sentinel everywhere else: padding columns 32, 33, unused rows, slabs outside the range"""
    T = np.full((32, 34), np.nan)
    if transposed: T[k0:k1, :rows] = M[:rows, k0:k1].T
    else: T[:rows, k0:k1] = M[:rows, k0:k1]
    return T


def check_wg_gemm(p):
    """integer inputs in [-8, 8]: every product and partial sum is exact, the result is bit-equal to the integer product — a wrong fragment map, tile index or slab bound
    is a wrong integer (or the NaN sentinel).  Random reals: within K x 2^-53 x (|A| |B|) of long double, K = 4 (ks1 - ks0) terms.  The epilogue runs exactly once per
    output element and nowhere else; C outside the 16 mt x 16 nt block keeps its canary."""
    rng = np.random.default_rng(41); Ai = rng.integers(-8, 9, (32, 32)).astype(float); Bi = rng.integers(-8, 9, (32, 32)).astype(float); Ar = rng.normal(size=(32, 32)); Br = rng.normal(size=(32, 32))
    C0 = _canary(1024, 0xd).reshape(32, 32)
    for ta in (False, True):
        for tb in (False, True):
            for mt in (1, 2):
                for nt in (1, 2):
                    for ks0, ks1 in K_RANGES:
                        for block in (64, 128, 256):
                            M, N, k0, k1 = 16 * mt, 16 * nt, 4 * ks0, 4 * ks1; case = (ta, tb, mt, nt, ks0, ks1, block)
                            for A, B, exact in ((Ai, Bi, True), (Ar, Br, False)):
                                # op(A) = A[:M, :] (M x 32), op(B) = B.T[:, :N] i.e. B holds op(B)ᵀ as an N x 32 matrix: both are "rows x k" here
                                Cg, calls = p.wg_gemm(ta, tb, block, _tile_image(A, ta, M, k0, k1), _tile_image(B, not tb, N, k0, k1), mt, nt, ks0, ks1, C0)
                                want_calls = np.zeros((32, 32), np.int32); want_calls[:M, :N] = 1
                                assert np.array_equal(calls, want_calls), case
                                ref = A[:M, k0:k1].astype(LD) @ B[:N, k0:k1].astype(LD).T
                                if exact:
                                    exp = C0.copy(); exp[:M, :N] = ref.astype(float); assert _same_bits(Cg, exp), (case, np.argwhere(_u64(Cg) != _u64(exp))[:4])
                                else:
                                    assert _same_bits(np.where(want_calls == 1, 0.0, Cg), np.where(want_calls == 1, 0.0, C0)), case
                                    bound = (k1 - k0) * U * (np.abs(A[:M, k0:k1]) @ np.abs(B[:N, k0:k1]).T); assert (np.abs(Cg[:M, :N] - ref) <= bound).all(), case


# ---------------------------------------------------------------- (e) register fragments ----------------------------------------------------------------
FRAG_SIZES = [(30, 30), (18, 30), (30, 18), (16, 16), (17, 31), (1, 1)]
# every <KT, IT, JT> of qm_gemm_tn the library instantiates: K1b (k_lq.h), K3 (k_riccati.h: rw_gemm_tn with MT = 1, 2 and its split form), the WBC (k_wbc.h)
GEMM_TN_SHAPES = [(2, 2, 2), (2, 2, 1), (2, 1, 2), (2, 1, 1), (1, 1, 2), (1, 1, 1), (1, 2, 2), (3, 2, 2)]


def gemm_tn_instantiations():
    """literal <KT, IT, JT> of every qm_gemm_tn / rw_gemm_tn call in the kernel sources (MT and KT expanded to 1 and 2, the values the Riccati kernel is instantiated with)"""
    d = os.path.join(ROOT, "qm_control_amd", "csrc", "kernels"); found = set()
    for f in os.listdir(d):
        for m in re.findall(r"(?:qm|rw)_gemm_tn<\s*(\w+),\s*(\w+),\s*(\w+)>\(", open(os.path.join(d, f)).read()):
            if m == ("KT", "IT", "JT"): continue      # rw_gemm_tn's forwarding call
            for mt in (1, 2):
                for kt in (1, 2):      # rw_gemm_tn_upper<KT> is called with 2 and with MT
                    found.add(tuple({"MT": mt, "KT": kt}.get(t, None) or int(t) for t in m))
    return found


def _frag_regs(M):
    """D-layout of a 32 x 32 matrix: register (2 I + J) 4 + r of lane l <-> M[16 I + (l >> 4) + 4 r][16 J + (l & 15)]"""
    l = np.arange(64); out = np.zeros((16, 64))
    for I in range(2):
        for J in range(2):
            for r in range(4): out[(2 * I + J) * 4 + r] = M[16 * I + (l >> 4) + 4 * r, 16 * J + (l & 15)]
    return out


def check_frag_round_trips(p):
    """qm_frag_load<2, 2, TR> / qm_frag_load_tile -> the registers as they are -> qm_frag_store<2, 2, STREAM>: the registers hold the D-layout of the rows x cols window and
    exact zeros outside it (whole tile for the unbounded load), the stored matrix equals the source on the window and the canaries around and between its rows keep their
    bits.  ld = 30 is used where a row of the source fits it (the stored window needs cols <= ld)."""
    rng = np.random.default_rng(51); n = 0
    for rows, cols in FRAG_SIZES:
        for ld in (30, 34):
            for tr in (False, True):
                for stream in (False, True):
                    for tile in (False, True):
                        if tile and ld != 34: continue                                  # the unbounded load reads a whole 32 x ld tile
                        if (rows if tr else cols) > ld or cols > ld: continue           # a source / destination row must fit its leading dimension
                        M = np.zeros((32, 32)); M[:rows, :cols] = rng.integers(1, 1000, (rows, cols)) + 0.5
                        if tile: M = rng.integers(1, 1000, (32, 32)) + 0.5               # fully populated: the load has no bounds, the store has
                        S = M.T if tr else M; src = np.full((32, ld), -7.0); src[:, :min(32, ld)] = S[:, :min(32, ld)]
                        if not tile: src = src.ravel()[:((cols - 1) * ld + rows) if tr else ((rows - 1) * ld + cols)]      # exactly what the bounded load may touch
                        dst = _canary(512 + 32 * ld, 0xe); exp = dst.copy()
                        regs = p.frag(tr, stream, tile, src, ld, rows, cols, dst, 256, ld)
                        assert _same_bits(regs, _frag_regs(M)), (rows, cols, ld, tr, stream, tile)
                        for r in range(rows): exp[256 + r * ld:256 + r * ld + cols] = M[r, :cols]
                        assert _same_bits(dst, exp), (rows, cols, ld, tr, stream, tile); n += 1
    assert n >= 60


def check_gemm_tn(p):
    """P ± Zᵀ Y over k-steps [k0, k1) (rows 4 k0 .. 4 k1 - 1 of Z and Y) onto a non-zero P, for every shape the library instantiates: integers bit-exact, random reals within
    (K + 1) x 2^-53 x (|P| + |Z|ᵀ |Y|) of long double, K = 4 (k1 - k0) terms"""
    assert GEMM_TN_SHAPES and gemm_tn_instantiations() == set(GEMM_TN_SHAPES), gemm_tn_instantiations()
    rng = np.random.default_rng(52)
    for kt, it, jt in GEMM_TN_SHAPES:
        for k0, k1 in ((0, 4 * kt), (1, 4 * kt - 1), (3, min(6, 4 * kt)), (2, 2)):
            for neg in (False, True):
                for exact in (True, False):
                    gen = (lambda s: rng.integers(-8, 9, s).astype(float)) if exact else (lambda s: rng.normal(size=s))
                    Z, Y, P = gen((16 * kt, 16 * it)), gen((16 * kt, 16 * jt)), gen((16 * it, 16 * jt)); sl = slice(4 * k0, 4 * k1); sg = -1 if neg else 1
                    ref = P.astype(LD) + sg * (Z[sl].astype(LD).T @ Y[sl].astype(LD)); got = p.gemm_tn((kt, it, jt), Z, Y, P, k0, k1, neg); case = (kt, it, jt, k0, k1, neg)
                    if exact: assert _same_bits(got, ref.astype(float) + 0.0), (case, np.argwhere(got != ref.astype(float))[:4])
                    else: assert (np.abs(got - ref) <= (4 * (k1 - k0) + 1) * U * (np.abs(P) + np.abs(Z[sl]).T @ np.abs(Y[sl]))).all(), case


# ---------------------------------------------------------------- (f) global -> LDS copy ----------------------------------------------------------------
def check_dma(p):
    """a lone wave copies a 4 KB segment with qm_dma16_at<0 / 1024 / 2048 / 3072> (one global base, one LDS base), waits, and returns its whole 8 KB LDS image: the segment
    as uint64, the pre-filled LDS before and behind it untouched; then single 1 KB chunks with qm_dma16 to arbitrary 16-byte-aligned LDS places.  The global sources are
    16-byte aligned and not 1 KB aligned (an allocation is at least 256-byte aligned: offsets of 2, 34, 250 doubles)."""
    g = bit_patterns().ravel()[:2048].view(np.float64); fill = _canary(1, 0xf)[0]; fb = _u64(np.array([fill]))[0]
    for off in (2, 34, 250):
        img = _u64(p.dma(0, g, off, 0, fill)); exp = np.full(1024, fb, np.uint64); exp[128:640] = _u64(g)[off:off + 512]; assert np.array_equal(img, exp), (off, np.flatnonzero(img != exp)[:8])
    for off, at in ((2, 0), (10, 6), (34, 130), (250, 896), (1918, 510)):
        img = _u64(p.dma(1, g, off, at, fill)); exp = np.full(1024, fb, np.uint64); exp[at:at + 128] = _u64(g)[off:off + 128]; assert np.array_equal(img, exp), (off, at, np.flatnonzero(img != exp)[:8])


# ---------------------------------------------------------------- (g) small dense helpers ----------------------------------------------------------------
def _unimodular(rng):
    """integer 3 x 3 matrix with determinant ±1: a product of elementary shears and a signed permutation"""
    A = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)[:, None]
    for _ in range(4):
        i, j = rng.choice(3, 2, replace=False); E = np.eye(3); E[i, j] = rng.integers(-2, 3); A = E @ A
    return A


def check_dense_helpers(p):
    """tile_load / tile_store / tile_row_dot / tile_col_dot and the 3 x 3 helpers on integer inputs: bit-exact.  The tile image outside the loaded window and the
    destination outside the stored window keep their NaN-pattern fill; m3_inv takes matrices of determinant ±1 (its integer cofactors times 1 / ±1)."""
    rng = np.random.default_rng(61); fill = _canary(1, 0xa)[0]; fb = _u64(np.array([fill]))[0]
    for (rows, cols), block in zip([(30, 30), (18, 30), (17, 31), (1, 1), (32, 32), (31, 5)], (256, 64, 128, 64, 256, 64)):
        sld, dld = cols + 3, cols + 2; src = rng.integers(-9, 10, (rows, sld)).astype(float); x = rng.integers(-9, 10, 32).astype(float); M = src[:, :cols]
        A = _unimodular(rng); Bm = rng.integers(-9, 10, (3, 3)).astype(float); v, w = rng.integers(-9, 10, 3).astype(float), rng.integers(-9, 10, 3).astype(float)
        assert abs(round(np.linalg.det(A))) == 1
        dst = _canary(512 + rows * dld, 0xb); exp = dst.copy()
        tile, rd, cd, m3 = p.dense(block, src, rows, cols, dld, x, fill, dst, 256, np.concatenate([A.ravel(), Bm.ravel(), v, w]))
        timg = np.full((32, 34), fb, np.uint64); timg[:rows, :cols] = _u64(M); assert np.array_equal(_u64(tile), timg), (rows, cols)
        for r in range(rows): exp[256 + r * dld:256 + r * dld + cols] = M[r]
        assert _same_bits(dst, exp), (rows, cols)
        assert _same_bits(rd[:rows], M @ x[:cols] + 0.0) and _same_bits(cd[:cols], M.T @ x[:rows] + 0.0), (rows, cols)
        inv = np.round(np.linalg.inv(A)); assert np.array_equal(inv @ A, np.eye(3))
        assert np.array_equal(m3[:9], (A @ Bm).ravel()) and np.array_equal(m3[9:12], A @ v) and np.array_equal(m3[12:21], inv.ravel()) and np.array_equal(m3[21:24], np.cross(v, w)), (rows, cols)


SCALAR_CHECKS = {"raw_estimates": check_raw_estimates, "frcp_log_existing_bounds": check_frcp_log_existing_bounds, "sincos_existing_bounds": check_sincos_existing_bounds,
                 "recip_rsqrt_to_one_ulp": check_recip_rsqrt_to_one_ulp, "givens": check_givens, "house_scalars": check_house_scalars, "barrier": check_barrier, "rotations": check_rotations}
STRUCT_CHECKS = {"wave_sum": check_wave_sum, "wave_max": check_wave_max, "bcast": check_bcast, "dpp_steps": check_dpp_steps, "rows": check_rows, "wg_gemm": check_wg_gemm,
                 "frag_round_trips": check_frag_round_trips, "gemm_tn": check_gemm_tn, "dma": check_dma, "dense_helpers": check_dense_helpers}
