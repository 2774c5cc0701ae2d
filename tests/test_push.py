"""Plant disturbances (qmhip_sim_set_pushes / qmhip_sim_get_push: csrc/kernels/k_sim.h qm_sim_push_kernel, csrc/host/qm_sim_pipeline.h) on the host emulator.

(0) the reference (tests/push_ref.py) without pushes is the oracle's plant;  (1) the pushed plant against it;  (2) window edges, exact;  (3) slot sum;  (4) isolation and off;
(5) the two device loops;  (6) error codes.  (1)-(4) and (6) are the checks tests/test_gpu_push.py runs on the device."""
import numpy as np
import pytest

import push_ref as pr
from conftest import rel_err
from test_sim import random_cases, robust_grid_settings


@pytest.fixture(scope="module")
def lib():
    return pr.emu_lib()


@pytest.mark.parametrize("nsub", [1, 2])
def test_reference_without_pushes_is_the_oracles_plant(oracle, oblobs, nsub):
    """1e-11 relative in q and v over 12 steps on twelve random cases: three decades above what the construction was observed at (1e-14 in v), four below the tolerances it is
    used at"""
    omb, ost = oblobs; ref = pr.PushRef(oracle, omb, ost); worst = [0.0, 0.0]
    for c in random_cases(oracle, ost, 12, 7):
        mine = ref.run(c, None, 12, 0.001, nsub, 1.0)
        oracle.sim_params(); oracle.sim_reset(c["q"], c["v"], 1.0); oracle.sim_command(c["pos"], c["vel"], c["kp"], c["kd"], c["ff"])
        for k in range(12):
            r = oracle.sim_step(0.001, nsub); eq, ev = rel_err(mine[k]["q"], r["q"]), rel_err(mine[k]["v"], r["v"]); worst = [max(worst[0], eq), max(worst[1], ev)]
            assert r["status"] == 0 and eq < 1e-11 and ev < 1e-11, (k, eq, ev)
            assert mine[k]["time"] == r["time"] and list(mine[k]["contact"]) == list(r["contact"]) and rel_err(mine[k]["force"], r["force"]) < 1e-9, k
    print("push_ref vs Oracle.sim_step, nsub %d: q %.1e v %.1e" % (nsub, *worst))


def test_pushed_plant_vs_reference(lib, blobs, oracle):
    p = pr.EmuPlant(lib, blobs, 6); pr.check_plant_vs_reference(p, oracle, "emulated plant"); p.close()


def test_window_edges_exact(lib, blobs, oracle):
    p = pr.EmuPlant(lib, blobs, 4); pr.check_window_edges(p, oracle); p.close()


def test_slot_sum(lib, blobs, oracle):
    pr.check_slot_sum(lambda B: pr.EmuPlant(lib, blobs, B), oracle)


def test_isolation_and_off(lib, blobs, oracle):
    pr.check_isolation_and_off(lambda B: pr.EmuPlant(lib, blobs, B), oracle, "emulated plant")


def test_error_codes_leave_the_schedule_untouched(lib, blobs, oracle):
    pr.check_errors(lambda B: pr.EmuPlant(lib, blobs, B), oracle)


def test_record_layout_matches_header_and_python(lib):
    from qm_control_amd import api, layout as L
    assert lib.emu_push_bytes() == api.PUSH.itemsize == L.QM_PUSH_BYTES == 96 and L.QM_SIM_MAX_PUSH == 8
    for k, (name, _, _, off) in enumerate(L.PUSH_FIELDS):
        assert lib.emu_push_offset(k) == off == api.PUSH.fields[name][1], name
    assert lib.emu_push_offset(len(L.PUSH_FIELDS)) == -1


# ---------------------------------------------------------------- (5) the loops
N_TICKS, EVERY, HORIZON, T_START = 24, 8, 0.6, 20.3


def loop_setup():
    """B = 2 as in test_closed_loop_around_the_plant_vs_oracle (tests/test_gpu_sim.py): trot, t_start = 20.3"""
    import os, sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sim_closed_loop_demo import setup
    c = setup("trot", 2, HORIZON, t_start=T_START); q0 = c["xbar"][6:30].copy(); q0[2] = 0.385
    return c, np.tile(q0, (2, 1)), float(c["t0"][0])


def loop_schedule(t_start, inactive=False):
    """instance 1: 60 N lateral base force over ticks 4-14, 15 N downward on the end effector throughout; instance 0 nothing.  inactive: instance 1's slots closed too"""
    ts, _ = pr.substep_times(t_start, pr.PERIOD, pr.NSUB, N_TICKS); p = pr.pushes(2, 2)
    if not inactive:
        pr.slot(p, 1, 0, ts[4, 0], ts[15, 0], base_force=(0.0, 60.0, 0.0)); pr.slot(p, 1, 1, -pr.INF, pr.INF, ee_force=(0.0, 0.0, -15.0))
    return p


def run_loop(plant, q0, t_start, p, pipelined):
    """24 ticks, the status words checked behind every call (one tick each; the pipelined loop in chunks of mpc_every)"""
    assert plant.set_pushes(p) == pr.OK; plant.reset(q0, np.zeros((2, 24)), t_start); chunk = EVERY if pipelined else 1
    for _ in range(N_TICKS // chunk):
        s = plant.closed_loop(chunk, pr.PERIOD, HORIZON, pr.NSUB, EVERY, pipelined=pipelined)
        assert (np.asarray(s["mpc_status"]) == 0).all() and (np.asarray(s["qp_status"]) == 0).all() and (s["status"] == 0).all(), (s["mpc_status"], s["qp_status"])
    rc, w, m = plant.push_state(); assert rc == pr.OK
    return s, w, m


def check_loop(make, pipelined, what):
    c, q0, t_start = loop_setup()
    a = make(c); sa, wa, ma = run_loop(a, q0, t_start, loop_schedule(t_start), pipelined); a.close()
    b = make(c); sb, wb, mb_ = run_loop(b, q0, t_start, loop_schedule(t_start, inactive=True), pipelined); b.close()
    assert all(np.array_equal(sa[n][0], sb[n][0]) for n in ("q", "v", "rbd", "force"))      # the neighbour's pushes do not reach instance 0
    e = rel_err(sa["q"][1], sb["q"][1]); print("%s: pushed vs unpushed instance, q after %d ticks: %.2e" % (what, N_TICKS, e)); assert e > 1e-4
    assert ma.tolist() == [0, 2] and np.array_equal(wa, [[0.0] * 9, [0.0] * 8 + [-15.0]]) and not mb_.any() and not wb.any()      # at the end only the permanent load is on


@pytest.mark.parametrize("pipelined", [False, True])
def test_loops_pick_the_schedule_up(lib, blobs, pipelined):
    mb, st = blobs

    def make(c):
        p = pr.EmuPlant(lib, (mb, robust_grid_settings(st)), 2, nev=c["ev"].shape[1], nmax=128); p.upload(c, 2)
        return p
    check_loop(make, pipelined, "emulated %s loop" % ("pipelined" if pipelined else "synchronous"))
