"""Sensor model between the plant and the controller (qmhip_sim_set_sensors / qmhip_sim_get_measured: csrc/kernels/k_sense.h qm_sense_kernel, csrc/host/qm_sim_pipeline.h)
on the host emulator.

(1) the generator;  (2) the measured state against the numpy reference (tests/sense_ref.py), bit for bit, and (3) the end-effector pose of the measured configuration;
(4) off means off;  (5) the two device loops;  (7) error codes;  (8) the record's layout.  (2)-(5) and (7) are the checks tests/test_gpu_sense.py runs on the device."""
import numpy as np
import pytest

import sense_ref as sr
from test_sim import robust_grid_settings


@pytest.fixture(scope="module")
def lib():
    return sr.emu_lib()


def loop_plant(lib, blobs):
    mb, st = blobs

    def make(c):
        p = sr.EmuPlant(lib, (mb, robust_grid_settings(st)), 2, nev=c["ev"].shape[1], nmax=128); p.upload(c, 2)
        return p
    return make


# ---------------------------------------------------------------- (1) the generator
def test_generator_values(lib):
    """the three values of the header's semantics from numpy and from the kernel's own routines on the host"""
    assert int(sr.word(1, 0, 0, 0)) == 0x5e41ab087439611e == lib.emu_sense_word(1, 0, 0, 0)
    assert float(sr.nu(1, 0, 0)) == 0.518857065021891 == lib.emu_sense_nu(1, 0, 0)
    assert float(sr.nu(1, sr.BIAS_N, 47)) == 1.6007686074982033 == lib.emu_sense_nu(1, 0xFFFFFFFFFFFFFFFF, 47)
    assert sr.CNU == 9.344061825059267e-06 and sr.NU_MAX <= 4.8990
    rng = np.random.default_rng(1); seeds = rng.integers(0, 2 ** 64, 64, dtype=np.uint64); ns = rng.integers(0, 2 ** 64, 64, dtype=np.uint64)      # any seed, any sample index
    for sd, n in zip(seeds.tolist(), ns.tolist()):
        c = int(n % 48); assert lib.emu_sense_nu(sd, n, c) == float(sr.nu(sd, n, c)) and lib.emu_sense_word(sd, n, c, 1) == int(sr.word(sd, n, c, 1))


def test_generator_through_the_plant(lib, blobs, oracle):
    p = sr.EmuPlant(lib, blobs, 1); sr.check_generator_through_plant(p, oracle); p.close()


def test_generator_statistics():
    """B = 1024 random seeds x 48 components x 20 samples = 983 040 draws of unit variance: |mean| < 5e-3 and |std - 1| < 5e-3 are 5 standard errors of the mean
    (1 / sqrt(N) = 1.0e-3) and 7 of the standard deviation; every draw within the Irwin-Hall bound.  The normalised error (m − x − bias) / sigma of the measured value is this
    draw up to the rounding of the four operations; tests/test_gpu_sense.py::test_full_batch takes it from the device's measured states"""
    rng = np.random.default_rng(7); seeds = rng.integers(0, 2 ** 64, 1024, dtype=np.uint64)
    d = sr.nu(seeds[:, None, None], np.arange(1, 21, dtype=np.uint64)[None, :, None], np.arange(48)[None, None, :])
    print("nu over %d draws: mean %.2e std - 1 %.2e max |nu| %.4f" % (d.size, d.mean(), d.std() - 1.0, np.abs(d).max()))
    assert d.size == 983040 and abs(d.mean()) < 5e-3 and abs(d.std() - 1.0) < 5e-3 and np.abs(d).max() <= 4.8990
    b = sr.nu(seeds[:, None], sr.BIAS_N, np.arange(48)[None, :]); assert np.abs(b).max() <= 4.8990 and abs(b.mean()) < 5.0 / np.sqrt(b.size)


# ---------------------------------------------------------------- (2), (3) the plant
def test_measured_state_vs_reference(lib, blobs, oracle):
    p = sr.EmuPlant(lib, blobs, 4); sr.check_plant_vs_reference(p, oracle, "emulated plant"); p.close()


# ---------------------------------------------------------------- (4), (5) the loops
def test_off_means_off(lib, blobs):
    sr.check_off_means_off(loop_plant(lib, blobs), "emulated synchronous loop")


@pytest.mark.parametrize("pipelined", [False, True])
def test_loops_pick_the_sensors_up(lib, blobs, pipelined):
    """sigma = (2e-3, 2e-3, 1e-3, 2e-2, 2e-2, 5e-2), bias_sigma = sigma / 2, lag 2 on instance 1: these levels keep every MPC, QP and plant status word at 0 over the
    24 ticks on the emulator (confirmed by this test: loop_run asserts them behind every call), so they are used as stated"""
    sr.check_loop(loop_plant(lib, blobs), "emulated %s loop" % ("pipelined" if pipelined else "synchronous"), pipelined)


# ---------------------------------------------------------------- (7), (8)
def test_error_codes_leave_the_records_in_force(lib, blobs, oracle):
    sr.check_errors(lambda B: sr.EmuPlant(lib, blobs, B), oracle)


def test_record_layout_matches_header_and_python(lib):
    from qm_control_amd import api, layout as L
    assert lib.emu_sense_bytes() == api.SENSOR.itemsize == L.QM_SENSE_BYTES == 128 and L.QM_SENSE_MAX_LAG == lib.emu_sense_max_lag() == 8 and L.QM_SENSE_GROUPS == 6
    want = dict(seed=0, lag=8, spare0=12, sigma=16, bias_sigma=64, spare=112)
    for k, (name, _, _, off) in enumerate(L.SENSOR_FIELDS):
        assert lib.emu_sense_offset(k) == off == api.SENSOR.fields[name][1] == want[name], name
    assert lib.emu_sense_offset(len(L.SENSOR_FIELDS)) == -1 and len(L.SENSOR_FIELDS) == len(want)
    assert api.SENSOR["sigma"].shape == (6,) and api.SENSOR["bias_sigma"].shape == (6,) and api.SENSOR["seed"] == np.dtype("<u8") and api.SENSOR["lag"] == np.dtype("<i4")
