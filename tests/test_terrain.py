"""Plant terrain (qmhip_sim_set_terrain / qmhip_sim_get_ground / qmhip_terrain_eval: csrc/kernels/k_sim.h qm_sim_terrain_kernel, qm_sim_terrain_push_kernel,
qm_terrain_eval_kernel; csrc/host/qm_sim_pipeline.h) on the host emulator.

(0) the reference (tests/terrain_ref.py) on the plane is PushRef;  (1) the lookup, exact at the edges;  (2) the plant against the reference;  (3) independent properties;
(4) flat, isolation, off;  (5) error codes;  (6) the pipelined loop.  (1)-(5) are the checks tests/test_gpu_terrain.py runs on the device."""
import numpy as np
import pytest

import push_ref as pr
import terrain_ref as tr
from test_sim import robust_grid_settings


@pytest.fixture(scope="module")
def lib():
    return tr.emu_lib()


def test_reference_on_the_plane_is_the_push_reference(oracle, oblobs):
    """the contact block restated against a tangent plane, on the plane z = 0, is PushRef's: 1e-13 relative in q, v and force over 12 steps — rounding of n = (0, 0, 1)
    products only, eight decades below the tolerances the reference is used at"""
    omb, ost = oblobs; mine = tr.TerrainRef(oracle, omb, ost); theirs = pr.PushRef(oracle, omb, ost)
    for c in pr.plant_cases(oracle, ost)[:3]:
        a = mine.run(c, None, 12, tr.PERIOD, tr.NSUB, tr.T0, None); b = theirs.run(c, None, 12, tr.PERIOD, tr.NSUB, tr.T0)
        for k in range(12):
            assert all(tr.rel_err(a[k][n], b[k][n]) < 1e-13 for n in ("q", "v", "force")) and list(a[k]["contact"]) == list(b[k]["contact"]), k
        assert any(r["force"].any() for r in b)


def test_lookup_exact_at_the_edges(lib, blobs):
    tr.check_lookup(lambda B: tr.EmuPlant(lib, blobs, B), "emulated lookup")


def test_plant_on_terrain_vs_reference(lib, blobs, oracle):
    tr.check_plant_vs_reference(lambda B: tr.EmuPlant(lib, blobs, B), oracle, "emulated plant")


def test_independent_properties(lib, blobs, oracle):
    tr.check_properties(lambda B: tr.EmuPlant(lib, blobs, B), oracle)


def test_flat_isolation_and_off(lib, blobs, oracle):
    tr.check_flat_isolation_off(lambda B: tr.EmuPlant(lib, blobs, B), oracle, "emulated plant")


def test_error_codes_leave_the_terrain_untouched(lib, blobs, oracle):
    tr.check_errors(lambda B: tr.EmuPlant(lib, blobs, B), oracle)


def test_record_layout_matches_header_and_python(lib):
    from qm_control_amd import api, layout as L
    assert lib.emu_terrain_bytes() == api.TERRAIN.itemsize == L.QM_TERRAIN_BYTES == 32 and lib.emu_terrain_max() == L.QM_TERRAIN_MAX == api.TERRAIN_MAX == 16
    for k, (name, _, _, off) in enumerate(L.TERRAIN_FIELDS):
        assert lib.emu_terrain_offset(k) == off == api.TERRAIN.fields[name][1], name
    assert lib.emu_terrain_offset(len(L.TERRAIN_FIELDS)) == -1


def test_pipelined_loop_picks_the_terrain_up(lib, blobs):
    mb, st = blobs

    def make(c):
        p = tr.EmuPlant(lib, (mb, robust_grid_settings(st)), 2, nev=c["ev"].shape[1], nmax=128); p.upload(c, 2)
        return p
    tr.check_loop(make, True, "emulated pipelined loop")
