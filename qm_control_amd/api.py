"""Host-side mirror of the reference's interfaces for the hot path, over the C ABI of libqmhip.so.

    QMInterface   <- qm::QMInterface            (qm_interface/include/qm_interface/QMInterface.h:31-54)
    SqpMpc        <- ocs2::MPC_BASE / SqpMpc    (qm_controllers/src/QMController.cpp:287-288; run(), policy)
    HierarchicalWbc <- qm::HierarchicalWbc      (qm_wbc/src/HierarchicalWbc.cpp:18-44; update(), loadTasksSetting)

There is NO CPU fallback: if libqmhip.so is missing, or no HIP device is present, construction raises.
Arrays are numpy f64, instance-major (batch first).  torch is not needed by this module.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqmhip.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
from . import layout as L
MB_SIZE, ST_SIZE = L.MB_SIZE, L.ST_SIZE

EXPORTS = ["qmhip_create", "qmhip_create_from_blobs", "qmhip_create_wbc_context", "qmhip_destroy", "qmhip_last_error", "qmhip_parse_model", "qmhip_export_blobs",
           "qmhip_set_setting", "qmhip_wbc_gain_index", "qmhip_mpc_step", "qmhip_mpc_upload", "qmhip_mpc_solve_resident", "qmhip_mpc_set_initial", "qmhip_mpc_update_references", "qmhip_mpc_solve_resident_warm",
           "qmhip_mpc_advance_resident", "qmhip_closed_loop_resident", "qmhip_mpc_download", "qmhip_policy_eval", "qmhip_policy_eval_feedback", "qmhip_mpc_download_feedback",
           "qmhip_policy_set_publish_window", "qmhip_policy_publish", "qmhip_policy_eval_published", "qmhip_policy_published_info",
           "qmhip_wbc_step", "qmhip_wbc_reset", "qmhip_hoqp_solve", "qmhip_control_step_resident", "qmhip_wbc_download", "qmhip_set_profiling",
           "qmhip_get_kernel_ms", "qmhip_reset_kernel_ms", "qmhip_synchronize", "qmhip_last_ls_trials", "qmhip_debug_read", "qmhip_debug_set", "qmhip_debug_get", "qmhip_microbench_fp64",
           "qmhip_gait_set_templates", "qmhip_gait_reset", "qmhip_gait_insert_template", "qmhip_gait_update_resident", "qmhip_gait_download", "qmhip_schedule_download",
           "qmhip_target_reset", "qmhip_target_from_command", "qmhip_target_download",
           "qmhip_step_submit", "qmhip_step_collect", "qmhip_step_in_flight",
           "qmhip_plan_task_space", "qmhip_plan_footholds", "qmhip_task_space_eval", "qmhip_policy_rollout",
           "qmhip_episode_monitor", "qmhip_episode_set_anchor", "qmhip_episode_summary", "qmhip_episode_trace", "qmhip_episode_fold",
           "qmhip_tick_reset", "qmhip_tick_submit", "qmhip_tick_collect", "qmhip_observe", "qmhip_sim_get_rbd", "qmhip_sim_set_pushes", "qmhip_sim_get_push", "qmhip_sim_set_sensors", "qmhip_sim_get_measured",
           "qmhip_sim_set_terrain", "qmhip_sim_get_ground", "qmhip_terrain_eval",
           "qmhip_sim_set_params", "qmhip_sim_set_controller", "qmhip_sim_reset", "qmhip_sim_set_command", "qmhip_sim_step", "qmhip_sim_get_state", "qmhip_closed_loop_sim", "qmhip_closed_loop_sim_pipelined"]

# struct qmhip_step_record (include/qmhip_layout.h) as a numpy structured dtype: one 1024-byte record per instance and control step
STEP_WBC, STEP_TRAJ = 1, 2
STEP_RECORD = np.dtype({"names": [f[0] for f in L.STEP_RECORD_FIELDS], "formats": [f[1] if f[2] == 1 else (f[1], (f[2],)) for f in L.STEP_RECORD_FIELDS],
                        "offsets": [f[3] for f in L.STEP_RECORD_FIELDS], "itemsize": L.QM_STEP_BYTES})
# struct qmhip_tick_record: one 2048-byte record per instance and controller tick (QMController below)
TICK_RECORD = np.dtype({"names": [f[0] for f in L.TICK_RECORD_FIELDS], "formats": [f[1] if f[2] == 1 else (f[1], (f[2],)) for f in L.TICK_RECORD_FIELDS],
                        "offsets": [f[3] for f in L.TICK_RECORD_FIELDS], "itemsize": L.QM_TICK_BYTES})

# struct qmhip_plan_record: one 512-byte record per node of a plan in task space (SqpMpc.plan_task_space, QMInterface.task_space); struct qmhip_foothold: one landing
_rec_dtype = lambda fields, size: np.dtype({"names": [f[0] for f in fields], "formats": [f[1] if f[2] == 1 else (f[1], f[2] if isinstance(f[2], tuple) else (f[2],)) for f in fields],
                                            "offsets": [f[3] for f in fields], "itemsize": size})
PLAN_RECORD = _rec_dtype(L.PLAN_RECORD_FIELDS, L.QM_PLAN_BYTES)
FOOTHOLD = _rec_dtype(L.FOOTHOLD_FIELDS, L.QM_FOOTHOLD_BYTES)
# struct qmhip_episode_summary: one 256-byte record per instance of a monitored episode; struct qmhip_episode_sample: one 512-byte raw sample (QMHWSim.monitor)
EPISODE_SUMMARY = _rec_dtype(L.EPISODE_SUMMARY_FIELDS, L.QM_EP_BYTES)
EPISODE_SAMPLE = _rec_dtype(L.EPISODE_SAMPLE_FIELDS, L.QM_ES_BYTES)
# struct qmhip_push: one scheduled external wrench on the plant, 96 bytes (QMHWSim.set_pushes)
PUSH = _rec_dtype(L.PUSH_FIELDS, L.QM_PUSH_BYTES)
SIM_MAX_PUSH = L.QM_SIM_MAX_PUSH
# struct qmhip_terrain: origin and spacing of one instance's ground grid, 32 bytes (QMHWSim.set_terrain)
TERRAIN = _rec_dtype(L.TERRAIN_FIELDS, L.QM_TERRAIN_BYTES)
TERRAIN_MAX = L.QM_TERRAIN_MAX
# struct qmhip_sensor: the sensor model of one instance of the plant, 128 bytes (QMHWSim.set_sensors)
SENSOR = _rec_dtype(L.SENSOR_FIELDS, L.QM_SENSE_BYTES)
SENSE_MAX_LAG, SENSE_GROUPS = L.QM_SENSE_MAX_LAG, L.QM_SENSE_GROUPS
# struct qmhip_rollout_summary: one 128-byte record per row of a policy rollout; qmhip_rollout_sample: one 512-byte trace sample per evaluation point (SqpMpc.rollout_policy)
ROLLOUT_SUMMARY = _rec_dtype(L.ROLLOUT_SUMMARY_FIELDS, L.QM_RS_BYTES)
ROLLOUT_SAMPLE = _rec_dtype(L.ROLLOUT_SAMPLE_FIELDS, L.QM_RT_BYTES)
ROLLOUT_MAX_STEPS, ROLLOUT_NONFINITE, ROLLOUT_OUTSIDE = L.QM_ROLLOUT_MAX_STEPS, L.QM_ROLLOUT_NONFINITE, L.QM_ROLLOUT_OUTSIDE
FALL_HEIGHT, FALL_ROLL, FALL_PITCH, FALL_NONFINITE = L.QM_FALL_HEIGHT, L.QM_FALL_ROLL, L.QM_FALL_PITCH, L.QM_FALL_NONFINITE


class _RolloutParams(C.Structure):
    _fields_ = [("max_step", C.c_double), ("max_steps", C.c_int32), ("source", C.c_int32), ("feedback", C.c_int32), ("trace_cap", C.c_int32)]


class _EpisodeParams(C.Structure):
    _fields_ = [("min_base_z", C.c_double), ("max_tilt", C.c_double), ("trace_every", C.c_int32), ("trace_cap", C.c_int32)]


def episode_fold(interface, tick, period, time, rbd, contact, force, mode, wbc_out, qp_status, sim_status=None, mpc_status=None):
    """qmhip_episode_fold: one tick of a plant the caller owns into the episode monitor (the companion of QMController.update): the state BEHIND the tick (time [B], rbd
    [B][55], contact [B][4], force [B][12]), what the tick's policy / WBC returned (mode [B], wbc_out [B][54], qp_status [B][3]), optionally the plant's status [B] and, on
    a tick with an MPC call, the call's status word [B].  The first fold after QMHWSim.monitor() starts the episode (set_anchor first)."""
    rbd = _f(rbd); B = rbd.shape[0]; i32 = lambda a, shape: None if a is None else np.ascontiguousarray(np.broadcast_to(a, shape), dtype=np.int32)
    t = _f(np.broadcast_to(time, (B,))); ct = i32(contact, (B, 4)); fo = _f(force, (B, 12)); mo = i32(mode, (B,)); wo = _f(wbc_out, (B, 54)); qp = i32(qp_status, (B, 3)); ss = i32(sim_status, (B,)); ms = i32(mpc_status, (B,))
    assert rbd.shape == (B, 55)
    interface._check(interface.lib.qmhip_episode_fold(interface.h, B, int(tick), C.c_double(period), _p(t), _p(rbd), _pi(ct), _p(fo), _pi(mo), _p(wo), _pi(qp), _pi(ss), _pi(ms)), "qmhip_episode_fold")


class QmhipError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen libqmhip.so (built by __graft_entry__.build()); raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QmhipError("libqmhip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.qmhip_last_error.restype = C.c_char_p
        _lib.qmhip_last_error.argtypes = [C.c_void_p]
        _lib.qmhip_destroy.argtypes = [C.c_void_p]
        _lib.qmhip_destroy.restype = None
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _f(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def parse_model(urdf_file, task_file, reference_file):
    """host-only parse (no GPU needed): returns (model_blob, settings_blob); raises ValueError for missing files
    like the reference constructor's std::invalid_argument (QMInterface.cpp:45,53,61)."""
    lib = load_library()
    mb = np.zeros(MB_SIZE); st = np.zeros(ST_SIZE)
    rc = lib.qmhip_parse_model(urdf_file.encode(), task_file.encode(), reference_file.encode(), _p(mb), _p(st))
    if rc != 0:
        msg = lib.qmhip_last_error(None).decode()
        raise (ValueError if rc == -2 else QmhipError)(msg)
    return mb, st


class QMInterface:
    """Owns the device context (model + settings + all HBM buffers) — qm::QMInterface's role."""

    def __init__(self, task_file=None, urdf_file=None, reference_file=None, *, blobs=None, device=0, max_batch=1, max_nodes=128, max_ref_knots=2, max_events=8):
        self.lib = load_library()
        h = C.c_void_p()
        if blobs is not None:
            mb, st = _f(blobs[0], (MB_SIZE,)), _f(blobs[1], (ST_SIZE,))
            rc = self.lib.qmhip_create_from_blobs(_p(mb), _p(st), device, max_batch, max_nodes, max_ref_knots, max_events, C.byref(h))
        else:
            rc = self.lib.qmhip_create(urdf_file.encode(), task_file.encode(), reference_file.encode(), device, max_batch, max_nodes, max_ref_knots, max_events, C.byref(h))
        if rc != 0:
            msg = self.lib.qmhip_last_error(None).decode()
            raise (ValueError if rc == -2 else QmhipError)("qmhip_create failed (%d): %s" % (rc, msg))
        self.h = h
        self.max_batch, self.max_nodes, self.max_ref_knots, self.max_events = max_batch, max_nodes, max_ref_knots, max_events
        self.model_blob = np.zeros(MB_SIZE); self.settings_blob = np.zeros(ST_SIZE)
        self.lib.qmhip_export_blobs(self.h, _p(self.model_blob), _p(self.settings_blob))

    def wbc_context(self, max_batch=None):
        """WBC-only context for the control thread (include/qmhip.h "Threads"): an interface object whose handle serves HierarchicalWbc only"""
        h = C.c_void_p()
        mbatch = self.max_batch if max_batch is None else int(max_batch)
        rc = self.lib.qmhip_create_wbc_context(self.h, mbatch, C.byref(h))
        if rc != 0:
            raise QmhipError("qmhip_create_wbc_context failed (%d): %s" % (rc, self.lib.qmhip_last_error(None).decode()))
        o = object.__new__(QMInterface)
        o.lib = self.lib; o.h = h; o.max_batch = mbatch; o.max_nodes, o.max_ref_knots, o.max_events = 3, 1, 1
        o.model_blob = self.model_blob.copy(); o.settings_blob = self.settings_blob.copy()
        return o

    def close(self):
        if getattr(self, "h", None):
            self.lib.qmhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise QmhipError("%s failed (%d): %s" % (what, rc, self.lib.qmhip_last_error(self.h).decode()))

    # getters named after the reference's
    def getInitialState(self):
        return self.settings_blob[L.ST_XINIT:L.ST_XINIT + 30].copy()

    def getCentroidalModelInfo(self):
        mb = self.model_blob
        return dict(robotMass=mb[L.MB_ROBOTMASS], centroidalInertiaNominal=mb[L.MB_INOM:L.MB_INOM + 9].reshape(3, 3).copy(), comToBasePositionNominal=mb[L.MB_RNOM:L.MB_RNOM + 3].copy(),
                    qPinocchioNominal=np.concatenate([np.zeros(6), mb[L.MB_QNOM:L.MB_QNOM + 18]]), stateDim=30, inputDim=30, generalizedCoordinatesNum=24, actuatedDofNum=18, numThreeDofContacts=4)

    def observe(self, rbd):
        """computeCentroidalStateFromRbdModel of measured rbd states [B][55] -> centroidal states [B][30] (qmhip_observe; stateless: the yaw is not unwrapped)"""
        rbd = _f(rbd); B = rbd.shape[0]; assert rbd.shape == (B, 55)
        x = np.zeros((B, 30))
        self._check(self.lib.qmhip_observe(self.h, B, _p(rbd), _p(x)), "qmhip_observe")
        return x

    def task_space(self, x, u=None, mode=15, ee_ref=None):
        """task-space records of caller-supplied states (qmhip_task_space_eval; QmVisualizer::publishDesiredTrajectory for target knots, publishObservation for an
        observation): x [R][30] (or [30]), u [R][30] or None (zero inputs), mode [R] (or one for all rows), ee_ref [R][7] = pos + quat xyzw or None (ee_err = 0).
        Returns [R] of dtype PLAN_RECORD (time = 0)"""
        x = np.atleast_2d(_f(x)); R = x.shape[0]; assert x.shape == (R, 30)
        u = None if u is None else _f(np.atleast_2d(u), (R, 30)); ee = None if ee_ref is None else _f(np.broadcast_to(np.asarray(ee_ref, float), (R, 7)))
        md = np.ascontiguousarray(np.broadcast_to(np.asarray(mode, np.int32), (R,)), dtype=np.int32)
        rec = np.zeros(R, PLAN_RECORD)
        self._check(self.lib.qmhip_task_space_eval(self.h, R, _p(x), _p(u), _pi(md), _p(ee), rec.ctypes.data_as(C.c_void_p)), "qmhip_task_space_eval")
        return rec

    def set_gain(self, name, value):
        """one field of the reference's dynamic_reconfigure config qm_wbc::WbcWeightConfig by NAME (WbcBase::dynamicCallback, WbcBase.cpp:69-116); False for a field
        the callback does not read (d_ee_x ...)"""
        idx = self.lib.qmhip_wbc_gain_index(name.encode())
        if idx < 0:
            return False
        self.set_setting(idx, value)
        return True

    def set_setting(self, index, value):
        self._check(self.lib.qmhip_set_setting(self.h, C.c_int(index), C.c_double(value)), "qmhip_set_setting")
        self.settings_blob[index] = value

    def set_publish_window(self, nodes):
        """qmhip_policy_set_publish_window: 0 = off (nothing allocated); 2 ... max_nodes = two slots holding the first `nodes` nodes' gain data per instance"""
        self._check(self.lib.qmhip_policy_set_publish_window(self.h, int(nodes)), "qmhip_policy_set_publish_window")

    def published_info(self, B=0):
        """(seq, window, uncovered [B]) of qmhip_policy_published_info; B: batch of the active publication (0: no counters)"""
        seq = C.c_int64(0); w = C.c_int32(0); unc = np.zeros(max(int(B), 1), np.int32)
        self._check(self.lib.qmhip_policy_published_info(self.h, C.byref(seq), C.byref(w), _pi(unc) if B else None), "qmhip_policy_published_info")
        return seq.value, w.value, unc[:int(B)]

    # instrumentation
    def set_profiling(self, on):
        """False / True: spans around no / every launch; 2: only around the modelled kernels (lq, riccati, wbc)"""
        self.lib.qmhip_set_profiling(self.h, int(on))

    def kernel_ms(self, name):
        ms = C.c_double(0); n = C.c_int(0)
        self.lib.qmhip_get_kernel_ms(self.h, name.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def reset_kernel_ms(self):
        self.lib.qmhip_reset_kernel_ms(self.h)

    def synchronize(self):
        self._check(self.lib.qmhip_synchronize(self.h), "qmhip_synchronize")

    def microbench_fp64(self, use_mfma):
        v = C.c_double(0)
        self._check(self.lib.qmhip_microbench_fp64(self.h, int(use_mfma), C.byref(v)), "qmhip_microbench_fp64")
        return v.value

    def debug_set(self, key, value):
        self._check(self.lib.qmhip_debug_set(self.h, key.encode(), C.c_int(value)), "qmhip_debug_set")

    def debug_get(self, key):
        v = C.c_int(0)
        self._check(self.lib.qmhip_debug_get(self.h, key.encode(), C.byref(v)), "qmhip_debug_get")
        return v.value

    def debug_read(self, name, shape, dtype=np.float64):
        out = np.zeros(shape, dtype=dtype)
        self._check(self.lib.qmhip_debug_read(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)), "qmhip_debug_read")
        return out


class SqpMpc:
    """ocs2::MPC_BASE-shaped front: run() = one multiple-shooting SQP iteration per instance (cold start)."""

    def __init__(self, interface):
        self.itf = interface
        self.lib = interface.lib
        self.B = 0

    def set_problem(self, t0, x0, ref_t, ref_x, event_times, modes):
        B = len(t0)
        t0 = _f(t0, (B,)); x0 = _f(x0, (B, 30)); ref_t = _f(ref_t); ref_x = _f(ref_x); ev = _f(event_times)
        modes = np.ascontiguousarray(modes, dtype=np.int32)
        assert ref_x.shape == (B, ref_t.shape[1], 37) and modes.shape == (B, ev.shape[1] + 1)
        self.itf._check(self.lib.qmhip_mpc_upload(self.itf.h, B, _p(t0), _p(x0), ref_t.shape[1], _p(ref_t), _p(ref_x), ev.shape[1], _p(ev), _pi(modes)), "qmhip_mpc_upload")
        self.B = B

    def solve_resident(self, horizon, warm=False):
        """one SQP iteration; warm=True starts from the previous primal solution (what MPC_BASE::run does on every call after the first)"""
        if warm:
            self.itf._check(self.lib.qmhip_mpc_solve_resident_warm(self.itf.h, self.B, C.c_double(horizon)), "qmhip_mpc_solve_resident_warm")
        else:
            self.itf._check(self.lib.qmhip_mpc_solve_resident(self.itf.h, self.B, C.c_double(horizon)), "qmhip_mpc_solve_resident")

    def set_initial(self, t0, x0):
        """new observation (MPC_MRT_Interface::setCurrentObservation); references, schedule and the previous solution stay resident"""
        t0 = _f(t0, (self.B,)); x0 = _f(x0, (self.B, 30))
        self.itf._check(self.lib.qmhip_mpc_set_initial(self.itf.h, self.B, _p(t0), _p(x0)), "qmhip_mpc_set_initial")

    def update_references(self, ref_t=None, ref_x=None, event_times=None, modes=None):
        """new targets and / or mode schedule for the next call; the previous primal solution stays (warm start) — ReferenceManager::preSolverRun"""
        B = self.B
        rt = rx = ev = mo = None; n_ref = self.itf.max_ref_knots; n_ev = self.itf.max_events
        if ref_t is not None:
            rt = _f(ref_t, (B, n_ref)); rx = _f(ref_x, (B, n_ref, 37))
        if event_times is not None:
            ev = _f(event_times, (B, n_ev)); mo = np.ascontiguousarray(modes, dtype=np.int32); assert mo.shape == (B, n_ev + 1)
        self.itf._check(self.lib.qmhip_mpc_update_references(self.itf.h, B, n_ref, _p(rt), _p(rx), n_ev, _p(ev), _pi(mo)), "qmhip_mpc_update_references")

    def advance(self, dt):
        """perfect-tracking plant on the device: t0 += dt, x0 <- policy state at the new t0"""
        self.itf._check(self.lib.qmhip_mpc_advance_resident(self.itf.h, self.B, C.c_double(dt)), "qmhip_mpc_advance_resident")

    def closed_loop_resident(self, n_steps, mpc_dt, horizon, period, time0):
        self.itf._check(self.lib.qmhip_closed_loop_resident(self.itf.h, self.B, int(n_steps), C.c_double(mpc_dt), C.c_double(horizon), C.c_double(period), C.c_double(time0)), "qmhip_closed_loop_resident")

    def control_step_resident(self, horizon, period, time):
        self.itf._check(self.lib.qmhip_control_step_resident(self.itf.h, self.B, C.c_double(horizon), C.c_double(period), C.c_double(time)), "qmhip_control_step_resident")

    def step_submit(self, t0, x0, rbd_meas=None, *, horizon, period, time, flags=STEP_WBC):
        """streamed control step (qmhip_step_submit): new observation + one warm-started control step, enqueued and not waited for; at most two in flight.
        rbd_meas [B][55]: the measured state the WBC runs on (None: built from x0 as control_step_resident does); flags: STEP_WBC | STEP_TRAJ"""
        B = self.B; t0 = _f(t0, (B,)); x0 = _f(x0, (B, 30)); rbd = None if rbd_meas is None else _f(rbd_meas, (B, 55))
        self.itf._check(self.lib.qmhip_step_submit(self.itf.h, B, _p(t0), _p(x0), _p(rbd), C.c_double(horizon), C.c_double(period), C.c_double(time), C.c_uint(flags)), "qmhip_step_submit")
        self._step_flags = getattr(self, "_step_flags", []) + [int(flags)]

    def step_collect(self, out=None):
        """the oldest step in flight (qmhip_step_collect): the keys and shapes of download() + HierarchicalWbc.download() — num_nodes, perf, status, wbc_out, qp_status, plus
        the policy at t0 (x_des, u_des, mode_t0) and the raw records (`record`, dtype STEP_RECORD); with STEP_TRAJ also t, event, mode, x, u [B][max_nodes][...], of which only
        the first num_nodes[b] nodes are written (`out`: a dict of arrays to write into instead of fresh zeros)"""
        B, nm = self.B, self.itf.max_nodes
        flags = self._step_flags[0] if getattr(self, "_step_flags", None) else 0
        rec = np.zeros(B, STEP_RECORD); res = {}
        if flags & STEP_TRAJ:
            out = out or {}
            res = dict(t=out.get("t", np.zeros((B, nm))), event=out.get("event", np.zeros((B, nm), np.int32)), mode=out.get("mode", np.zeros((B, nm), np.int32)),
                       x=out.get("x", np.zeros((B, nm, 30))), u=out.get("u", np.zeros((B, nm, 30))))
        self.itf._check(self.lib.qmhip_step_collect(self.itf.h, B, rec.ctypes.data_as(C.c_void_p), _p(res.get("t")), _pi(res.get("event")), _pi(res.get("mode")), _p(res.get("x")), _p(res.get("u"))), "qmhip_step_collect")
        self._step_flags.pop(0)
        res.update(num_nodes=rec["n_nodes"].copy(), perf=rec["perf"].copy(), status=rec["mpc_status"].copy(), wbc_out=rec["wbc_out"].copy(), qp_status=rec["qp_status"].copy(),
                   x_des=rec["x_des"].copy(), u_des=rec["u_des"].copy(), mode_t0=rec["mode"].copy(), record=rec)
        return res

    def steps_in_flight(self):
        return int(self.lib.qmhip_step_in_flight(self.itf.h))

    def download(self):
        B, nm = self.B, self.itf.max_nodes
        nn = np.zeros(B, np.int32); t = np.zeros((B, nm)); ev = np.zeros((B, nm), np.int32); mode = np.zeros((B, nm), np.int32)
        x = np.zeros((B, nm, 30)); u = np.zeros((B, nm, 30)); perf = np.zeros((B, 10)); status = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_mpc_download(self.itf.h, B, _pi(nn), _p(t), _pi(ev), _pi(mode), _p(x), _p(u), _p(perf), _pi(status)), "qmhip_mpc_download")
        return dict(num_nodes=nn, t=t, event=ev, mode=mode, x=x, u=u, perf=perf, status=status, ls_trials=self.lib.qmhip_last_ls_trials(self.itf.h))

    def run(self, t0, x0, ref_t, ref_x, event_times, modes, horizon):
        self.set_problem(t0, x0, ref_t, ref_x, event_times, modes)
        self.solve_resident(horizon)
        return self.download()

    def evaluatePolicy(self, t):
        t = _f(t, (self.B,))
        x = np.zeros((self.B, 30)); u = np.zeros((self.B, 30)); mode = np.zeros(self.B, np.int32)
        self.itf._check(self.lib.qmhip_policy_eval(self.itf.h, self.B, _p(t), _p(x), _p(u), _pi(mode)), "qmhip_policy_eval")
        return x, u, mode

    def evaluate_policy(self, t, x=None):
        """MPC_MRT_Interface::evaluatePolicy(t, x): with a measured state x [B][30] the SQP's linear controller u = uff(t) + K(t) x (qmhip_policy_eval_feedback: the policy
        of `sqp.useFeedbackPolicy true`, applied whatever the settings slot says); x=None: the feed-forward policy, exactly evaluatePolicy(t).  Returns (x_des, u_des, mode)"""
        if x is None:
            return self.evaluatePolicy(t)
        t = _f(t, (self.B,)); xm = _f(x, (self.B, 30))
        xd = np.zeros((self.B, 30)); u = np.zeros((self.B, 30)); mode = np.zeros(self.B, np.int32)
        self.itf._check(self.lib.qmhip_policy_eval_feedback(self.itf.h, self.B, _p(t), _p(xm), _p(xd), _p(u), _pi(mode)), "qmhip_policy_eval_feedback")
        return xd, u, mode

    def publish_policy(self):
        """MPC_MRT_Interface's policy hand-over (qmhip_policy_publish): snapshot of the last solve into the inactive publication slot, which becomes the active one; needs
        QMInterface.set_publish_window"""
        self.itf._check(self.lib.qmhip_policy_publish(self.itf.h, self.B), "qmhip_policy_publish")

    def evaluate_published(self, t, x=None):
        """updatePolicy + evaluatePolicy(t, x) on the ACTIVE publication (qmhip_policy_eval_published): safe beside a running solve, from another thread too.
        Returns (x_des, u_des, mode, covered, seq); an instance with covered == 0 got the feed-forward input"""
        B = self.B; t = _f(t, (B,)); xm = None if x is None else _f(x, (B, 30))
        xd = np.zeros((B, 30)); u = np.zeros((B, 30)); mode = np.zeros(B, np.int32); cov = np.zeros(B, np.int32); seq = C.c_int64(0)
        self.itf._check(self.lib.qmhip_policy_eval_published(self.itf.h, B, _p(t), _p(xm), _p(xd), _p(u), _pi(mode), _pi(cov), C.byref(seq)), "qmhip_policy_eval_published")
        return xd, u, mode, cov, seq.value

    def plan_task_space(self):
        """the last solve's plan in task space (qmhip_plan_task_space; QmVisualizer::publishOptimizedStateTrajectory): (records [B][max_nodes] of dtype PLAN_RECORD,
        num_nodes [B]); records at or behind num_nodes[b] are zero"""
        B, nm = self.B, self.itf.max_nodes
        rec = np.zeros((B, nm), PLAN_RECORD); nn = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_plan_task_space(self.itf.h, B, rec.ctypes.data_as(C.c_void_p), _pi(nn)), "qmhip_plan_task_space")
        return rec, nn

    def plan_footholds(self, cap=16):
        """where the feet land inside the planned horizon (qmhip_plan_footholds): (footholds [B][cap] of dtype FOOTHOLD ordered by (event, foot), count [B]); count[b]
        is the full number of landings, of which the first min(count[b], cap) are written"""
        B = self.B; fh = np.zeros((B, int(cap)), FOOTHOLD); cnt = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_plan_footholds(self.itf.h, B, int(cap), fh.ctypes.data_as(C.c_void_p) if cap else None, _pi(cnt)), "qmhip_plan_footholds")
        return fh, cnt

    def rollout_policy(self, t, x, t_end, inst=None, *, max_step=None, max_steps=4096, feedback=True, source="solve", trace=0):
        """MPC_MRT_Interface::rolloutPolicy, batched (qmhip_policy_rollout): R rows — start times t [R], start states x [R][30], absolute final times t_end [R] (or one for
        all rows), inst [R] the instance of the last solve / the active publication a row rolls out (None: row r = instance r) — integrated with the transcription's Heun
        rule at steps of at most max_step (None: sqp.dt, the step the gains belong to) that also end on the schedule's events, the input held over a step.  feedback:
        the SQP's linear controller at the rolled state (True) or the feed-forward policy; source "solve": the last solve (the validity window of evaluate_policy(t, x)),
        "published": the active publication, safe beside a running solve.  trace: samples to keep per row.
        Returns dict(x, u, mode = the end point's state, input, mode; summary [R] of dtype ROLLOUT_SUMMARY), with a trace also trace [R][trace] of dtype ROLLOUT_SAMPLE
        and count [R] (evaluation points; the first min(count, trace) samples of a row are written), for "published" also seq"""
        t = np.atleast_1d(_f(t)); R = t.shape[0]; xs = _f(np.atleast_2d(x), (R, 30)); te = _f(np.broadcast_to(np.asarray(t_end, float), (R,)))
        ins = None if inst is None else np.ascontiguousarray(np.broadcast_to(np.asarray(inst, np.int32), (R,)), dtype=np.int32)
        if source not in ("solve", "published"):
            raise ValueError("source is 'solve' or 'published'")
        step = self.itf.settings_blob[L.ST_IPM_DT if self.itf.settings_blob[L.ST_SOLVER] >= 2.0 else L.ST_SQP_DT] if max_step is None else max_step
        p = _RolloutParams(float(step), int(max_steps), 1 if source == "published" else 0, int(bool(feedback)), int(trace))
        xe = np.zeros((R, 30)); ue = np.zeros((R, 30)); mode = np.zeros(R, np.int32); sm = np.zeros(R, ROLLOUT_SUMMARY); cnt = np.zeros(R, np.int32); seq = C.c_int64(0)
        tr = np.zeros((R, int(trace)), ROLLOUT_SAMPLE) if trace else None
        self.itf._check(self.lib.qmhip_policy_rollout(self.itf.h, R, _pi(ins), _p(t), _p(xs), _p(te), C.byref(p), _p(xe), _p(ue), _pi(mode), sm.ctypes.data_as(C.c_void_p),
                                                      tr.ctypes.data_as(C.c_void_p) if trace else None, _pi(cnt), C.byref(seq)), "qmhip_policy_rollout")
        out = dict(x=xe, u=ue, mode=mode, summary=sm)
        if trace: out.update(trace=tr, count=cnt)
        if source == "published": out["seq"] = seq.value
        return out

    def rolloutPolicy(self, currentTime, currentState, timeStep):
        """MPC_MRT_Interface::rolloutPolicy(currentTime, currentState, timeStep, mpcState, mpcInput, mode) for the batch of the last solve: instance b rolled from
        (currentTime[b], currentState[b]) over timeStep under the policy ST_FEEDBACK_POLICY selects.  Returns (mpcState, mpcInput, mode)"""
        t = _f(np.broadcast_to(np.asarray(currentTime, float), (self.B,)))
        r = self.rollout_policy(t, _f(currentState, (self.B, 30)), t + float(timeStep), feedback=self.itf.settings_blob[L.ST_FEEDBACK_POLICY] != 0.0)
        return r["x"], r["u"], r["mode"]

    def feedback(self):
        """the linear controller of the last solve as ocs2::LinearController holds it (qmhip_mpc_download_feedback): (gain [B][max_nodes][30][30], uff [B][max_nodes][30]) on the
        time stamps of download()["t"]; nodes behind an instance's grid hold zeros"""
        B, nm = self.B, self.itf.max_nodes
        gain = np.zeros((B, nm, 30, 30)); uff = np.zeros((B, nm, 30))
        self.itf._check(self.lib.qmhip_mpc_download_feedback(self.itf.h, B, _p(gain), _p(uff)), "qmhip_mpc_download_feedback")
        return gain, uff


class HierarchicalWbc:
    """qm::HierarchicalWbc-shaped front: update(stateDesired, inputDesired, rbdStateMeasured, mode, period, time) -> [x(36); tau(18)]."""

    def __init__(self, interface, mpc_variant=False):
        self.itf = interface
        self.lib = interface.lib
        self.variant = 1 if mpc_variant else 0

    def reset(self):
        self.itf._check(self.lib.qmhip_wbc_reset(self.itf.h), "qmhip_wbc_reset")

    def update(self, stateDesired, inputDesired, rbdStateMeasured, mode, period, time):
        xd = _f(stateDesired); B = xd.shape[0]
        ud = _f(inputDesired, (B, 30)); rbd = _f(rbdStateMeasured, (B, 55)); mode = np.ascontiguousarray(mode, np.int32); time = _f(np.broadcast_to(time, (B,)))
        out = np.zeros((B, 54)); st = np.zeros((B, 3), np.int32)
        self.itf._check(self.lib.qmhip_wbc_step(self.itf.h, B, _p(xd), _p(ud), _p(rbd), _pi(mode), C.c_double(period), _p(time), self.variant, _p(out), _pi(st)), "qmhip_wbc_step")
        return out, st

    def download(self, B):
        out = np.zeros((B, 54)); st = np.zeros((B, 3), np.int32)
        self.itf._check(self.lib.qmhip_wbc_download(self.itf.h, B, _p(out), _pi(st)), "qmhip_wbc_download")
        return out, st


class HoQp:
    """qm::HoQp-shaped front of the general cascade (qm_wbc/include/qm_wbc/HoQp.h:17-36): tasks from the highest priority down, every task dict(A, b, D, f) with
    arrays [B][rows][n] / [B][rows] (or without the batch axis for one problem); getSolutions() of the last level and the per-level status"""

    def __init__(self, interface):
        self.itf = interface; self.lib = interface.lib

    def solve(self, tasks):
        first = np.asarray(tasks[0]["A"] if np.asarray(tasks[0]["A"]).size else tasks[0]["D"], float)
        single = first.ndim == 2
        n = first.shape[-1]
        arr = lambda t, k, w: np.asarray(t[k], float).reshape((1, -1, n) if w else (1, -1)) if single else np.asarray(t[k], float).reshape((len(np.asarray(t[k])), -1, n) if w else (len(np.asarray(t[k])), -1))
        As = [arr(t, "A", True) for t in tasks]; bs = [arr(t, "b", False) for t in tasks]; Ds = [arr(t, "D", True) for t in tasks]; fs = [arr(t, "f", False) for t in tasks]
        B = max(a.shape[0] for a in As + Ds)
        ma = np.array([a.shape[1] for a in As], np.int32); md = np.array([d.shape[1] for d in Ds], np.int32)
        A = _f(np.concatenate(As, axis=1)) if ma.sum() else np.zeros(1); b = _f(np.concatenate(bs, axis=1)) if ma.sum() else np.zeros(1)
        D = _f(np.concatenate(Ds, axis=1)) if md.sum() else np.zeros(1); f = _f(np.concatenate(fs, axis=1)) if md.sum() else np.zeros(1)
        x = np.zeros((B, n)); st = np.zeros((B, len(tasks)), np.int32)
        self.itf._check(self.lib.qmhip_hoqp_solve(self.itf.h, B, len(tasks), n, _pi(ma), _pi(md), _p(A), _p(b), _p(D), _p(f), _p(x), _pi(st)), "qmhip_hoqp_solve")
        return (x[0], st[0]) if single else (x, st)


class QMHWSim:
    """qm_gazebo::QMHWSim-shaped front of the batched rigid-body plant (qm_gazebo/src/QMHWSim.cpp:60-116): `setCommand` is what
    QMController::updateControlLaw issues through the hybrid joint handles, `step(period)` = writeSim (delay buffer + joint PD law) + the physics step +
    readSim (rbd state in the estimator's layout, contact flags)."""
    PARAMS = ("contact_stiffness", "contact_damping", "friction", "friction_speed_eps", "foot_radius", "delay", "saturate_effort")

    def __init__(self, interface, robust_grid=False, feedback_policy=False, publish_window=None, **params):
        """robust_grid: opt into the SQP time grid's robust minimum step (ST_GRID_DT_MIN = QM_GRID_DT_MIN_ROBUST, include/qmhip_layout.h) — for long fixed-rate loops whose
        1 ms observation raster can land within weakEpsilon of a gait event; the default keeps [upstream]'s 10 * limitEpsilon.
        feedback_policy: ST_FEEDBACK_POLICY = 1 (`sqp.useFeedbackPolicy true`): the ticks of closed_loop() evaluate the SQP's linear controller at the estimated state; False
        leaves the context's setting as its task file / blob has it.
        publish_window: nodes of the published gain window (QMInterface.set_publish_window) — with it closed_loop(pipelined=True) runs the feedback policy too; None leaves
        the context's window as it is"""
        self.itf = interface
        self.lib = interface.lib
        self.B = 0
        if robust_grid:
            interface.set_setting(L.ST_GRID_DT_MIN, L.QM_GRID_DT_MIN_ROBUST)
        if feedback_policy:
            interface.set_setting(L.ST_FEEDBACK_POLICY, 1.0)
        if publish_window is not None:
            interface.set_publish_window(publish_window)
        if params:
            self.set_params(**params)

    def set_params(self, **params):
        cur = dict(contact_stiffness=4.0e4, contact_damping=200.0, friction=0.8, friction_speed_eps=1.0e-2, foot_radius=0.02, delay=0.009, saturate_effort=1.0)
        cur.update(getattr(self, "params", {}))
        for k in params:
            if k not in cur:
                raise KeyError(k)
        cur.update(params); self.params = cur
        v = _f([float(cur[k]) for k in self.PARAMS])
        self.itf._check(self.lib.qmhip_sim_set_params(self.itf.h, _p(v), 7), "qmhip_sim_set_params")

    def reset(self, q, v, time=0.0):
        q = _f(q); B = q.shape[0]; v = _f(v, (B, 24)); t = _f(np.broadcast_to(time, (B,)))
        assert q.shape == (B, 24)
        self.itf._check(self.lib.qmhip_sim_reset(self.itf.h, B, _p(q), _p(v), _p(t)), "qmhip_sim_reset")
        self.B = B

    def setCommand(self, posDes, velDes, kp, kd, ff):
        B = self.B; a = [_f(np.broadcast_to(x, (B, 18))) for x in (posDes, velDes, kp, kd, ff)]
        self.itf._check(self.lib.qmhip_sim_set_command(self.itf.h, B, *[_p(x) for x in a]), "qmhip_sim_set_command")

    def step(self, period, n_substeps=2, download=True):
        B = self.B; rbd = np.zeros((B, 55)) if download else None; contact = np.zeros((B, 4), np.int32) if download else None
        self.itf._check(self.lib.qmhip_sim_step(self.itf.h, B, C.c_double(period), int(n_substeps), _p(rbd), _pi(contact)), "qmhip_sim_step")
        return rbd, contact

    def set_pushes(self, p):
        """schedule of external wrenches (qmhip_sim_set_pushes): p is [B][K] or [B] of dtype PUSH (K <= SIM_MAX_PUSH) — per slot a window t_on <= t < t_off of absolute
        plant time (t_off = inf: a permanent load) and, in the world frame, base_force at the base origin, base_torque on the base body, ee_force at the arm's tip.
        None switches pushes off.  The schedule persists across reset()"""
        if p is None:
            self.itf._check(self.lib.qmhip_sim_set_pushes(self.itf.h, 0, 0, None), "qmhip_sim_set_pushes"); return
        p = np.ascontiguousarray(p, dtype=PUSH)
        if p.ndim == 1:
            p = p[:, None]
        assert p.ndim == 2
        self.itf._check(self.lib.qmhip_sim_set_pushes(self.itf.h, p.shape[0], p.shape[1], p.ctypes.data_as(C.c_void_p)), "qmhip_sim_set_pushes")

    def push_state(self, B=None):
        """(wrench [B][9], mask [B]): base force, base torque and end-effector force the last sub-step of the last step applied; bit k of mask: slot k was active"""
        B = self.B if B is None else int(B); w = np.zeros((B, 9)); m = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_sim_get_push(self.itf.h, B, _p(w), _pi(m)), "qmhip_sim_get_push")
        return w, m

    def set_terrain(self, hdr, height=None, mu=None):
        """ground under the feet (qmhip_sim_set_terrain): hdr is [B] of dtype TERRAIN (x0, y0, dx, dy of each instance's grid in the world frame), height [B][ny][nx] and
        mu (same shape, or None: the `friction` of set_params everywhere) with 2 <= nx, ny <= TERRAIN_MAX.  Bilinear between the vertices, continued at the edge's height
        outside; every foot meets the tangent plane under it.  set_terrain(None) puts the plant back on the plane z = 0.  The terrain persists across reset()"""
        if hdr is None:
            self.itf._check(self.lib.qmhip_sim_set_terrain(self.itf.h, 0, 0, 0, None, None, None), "qmhip_sim_set_terrain"); return
        hdr = np.ascontiguousarray(hdr, dtype=TERRAIN); height = _f(height); mu = None if mu is None else _f(mu)
        assert hdr.ndim == 1 and height.ndim == 3 and height.shape[0] == hdr.shape[0] and (mu is None or mu.shape == height.shape)
        self.itf._check(self.lib.qmhip_sim_set_terrain(self.itf.h, hdr.shape[0], height.shape[2], height.shape[1], hdr.ctypes.data_as(C.c_void_p), _p(height), _p(mu)), "qmhip_sim_set_terrain")

    def ground(self, B=None):
        """[B][4][6]: per foot (LF RF LH RH) h, n_x, n_y, n_z, mu, pen of the last sub-step of the last step — zeros after reset() and without a terrain"""
        B = self.B if B is None else int(B); g = np.zeros((B, 4, 6))
        self.itf._check(self.lib.qmhip_sim_get_ground(self.itf.h, B, _p(g)), "qmhip_sim_get_ground")
        return g

    def terrain_eval(self, xy):
        """the plant's lookup at xy [B][n][2] (world frame): [B][n][4] = h, gx, gy, mu"""
        xy = _f(xy); assert xy.ndim == 3 and xy.shape[2] == 2
        out = np.zeros(xy.shape[:2] + (4,))
        self.itf._check(self.lib.qmhip_terrain_eval(self.itf.h, xy.shape[0], xy.shape[1], _p(xy), _p(out)), "qmhip_terrain_eval")
        return out

    def set_sensors(self, s):
        """sensor model between the plant and the controller (qmhip_sim_set_sensors): s is [B] of dtype SENSOR — per instance a seed, a latency `lag` of whole samples
        (<= SENSE_MAX_LAG) and, per group of the rbd state (base zyx, base position, joint positions, base angular velocity, base linear velocity, joint rates), the standard
        deviations sigma of white noise and bias_sigma of a constant bias.  None switches the model off.  closed_loop() then controls on the measured state; step(), rbd(),
        state() and the episode monitor keep the truth.  The records persist across reset(); the sample count starts over"""
        if s is None:
            self.itf._check(self.lib.qmhip_sim_set_sensors(self.itf.h, 0, None), "qmhip_sim_set_sensors"); return
        s = np.ascontiguousarray(s, dtype=SENSOR)
        assert s.ndim == 1
        self.itf._check(self.lib.qmhip_sim_set_sensors(self.itf.h, s.shape[0], s.ctypes.data_as(C.c_void_p)), "qmhip_sim_set_sensors")

    def measured(self, B=None):
        """(rbd [B][55], samples [B]): the state the loops consume and the index of the last sample — the truth and zeros while the sensor model is off"""
        B = self.B if B is None else int(B); rbd = np.zeros((B, 55)); n = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_sim_get_measured(self.itf.h, B, _p(rbd), _pi(n)), "qmhip_sim_get_measured")
        return rbd, n

    def set_controller(self, kind):
        """0: qm::QMController, 1: qm::QMMpcController (HierarchicalMpcWbc + arm position commands at 100 Hz); call before reset()"""
        self.itf._check(self.lib.qmhip_sim_set_controller(self.itf.h, int(kind)), "qmhip_sim_set_controller")

    def closed_loop(self, n_ticks, period, horizon, n_substeps=2, mpc_every=10, arm_kp=0.0, arm_kd=0.5, pipelined=False):
        """n_ticks of [state estimate -> MPC every mpc_every ticks -> policy -> WBC -> updateControlLaw -> simulation step] on the device (QMController::update);
        arm gains default to the reference's dynamic-reconfigure defaults (qm_controllers/cfg/weight.cfg:7-8)"""
        fn = self.lib.qmhip_closed_loop_sim_pipelined if pipelined else self.lib.qmhip_closed_loop_sim     # pipelined: the MPC beside the ticks, one period of latency
        self.itf._check(fn(self.itf.h, self.B, int(n_ticks), C.c_double(period), int(n_substeps), int(mpc_every), C.c_double(horizon), C.c_double(arm_kp), C.c_double(arm_kd)), "qmhip_closed_loop_sim")

    def monitor(self, min_base_z=0.2, max_tilt=0.8, trace_every=0, trace_cap=0):
        """episode monitor (qmhip_episode_monitor): per-instance statistics of every tick of closed_loop() folded on the device, a fall when the base height drops below
        min_base_z or |roll| / |pitch| exceed max_tilt, optionally a trace of up to trace_cap raw samples, one every trace_every ticks.  monitor(None) switches it off.
        The next reset() starts the episode; read it with episode_summary() / episode_trace()"""
        if min_base_z is None:
            self.itf._check(self.lib.qmhip_episode_monitor(self.itf.h, None), "qmhip_episode_monitor"); self._trace_cap = 0; return
        p = _EpisodeParams(float(min_base_z), float(max_tilt), int(trace_every), int(trace_cap))
        self.itf._check(self.lib.qmhip_episode_monitor(self.itf.h, C.byref(p)), "qmhip_episode_monitor")
        self._trace_cap = int(trace_cap)

    def set_anchor(self, ee_pose):
        """end-effector anchor [B][7] (position + quaternion xyzw) of the deviation statistics; without it the anchor is the reset state's end-effector pose"""
        ee = _f(ee_pose); assert ee.ndim == 2 and ee.shape[1] == 7
        self.itf._check(self.lib.qmhip_episode_set_anchor(self.itf.h, ee.shape[0], _p(ee)), "qmhip_episode_set_anchor")

    def episode_summary(self, B=None):
        """records [B] of dtype EPISODE_SUMMARY of the running episode"""
        B = self.B if B is None else int(B); out = np.zeros(B, EPISODE_SUMMARY)
        self.itf._check(self.lib.qmhip_episode_summary(self.itf.h, B, out.ctypes.data_as(C.c_void_p)), "qmhip_episode_summary")
        return out

    def episode_trace(self, cap=None, B=None):
        """(samples [n][B] of dtype EPISODE_SAMPLE, count): n = min(count, cap) samples the trace holds, count the number of sampled ticks (it keeps counting behind trace_cap)"""
        B = self.B if B is None else int(B); n = np.zeros(1, np.int32)
        if cap is None:
            self.itf._check(self.lib.qmhip_episode_trace(self.itf.h, B, 0, None, _pi(n)), "qmhip_episode_trace"); cap = int(n[0])
        out = np.zeros((int(cap), B), EPISODE_SAMPLE)
        self.itf._check(self.lib.qmhip_episode_trace(self.itf.h, B, int(cap), out.ctypes.data_as(C.c_void_p) if cap else None, _pi(n)), "qmhip_episode_trace")
        return out[:min(int(n[0]), int(cap), getattr(self, "_trace_cap", 0))], int(n[0])

    def rbd(self):
        """(rbd [B][55], contact [B][4]) of the plant's current state, without stepping (qmhip_sim_get_rbd)"""
        B = self.B; rbd = np.zeros((B, 55)); contact = np.zeros((B, 4), np.int32)
        self.itf._check(self.lib.qmhip_sim_get_rbd(self.itf.h, B, _p(rbd), _pi(contact)), "qmhip_sim_get_rbd")
        return rbd, contact

    def state(self):
        B = self.B; q = np.zeros((B, 24)); v = np.zeros((B, 24)); t = np.zeros(B); f = np.zeros((B, 12)); st = np.zeros(B, np.int32)
        self.itf._check(self.lib.qmhip_sim_get_state(self.itf.h, B, _p(q), _p(v), _p(t), _p(f), _pi(st)), "qmhip_sim_get_state")
        return dict(q=q, v=v, time=t, force=f, status=st)


class QMController:
    """qm::QMController::update as a service for a plant on the host (qmhip_tick_reset / _submit / _collect): measured rbd states in, hybrid joint commands out, once
    per tick, the MPC on every mpc_every-th tick, the controller's state on the device in between.  controller: 0 qm::QMController, 1 qm::QMMpcController; arm gains
    default to the reference's dynamic-reconfigure defaults.  References and schedule: SqpMpc.set_problem / update_references or the device GaitSchedule, before starting()."""

    def __init__(self, interface, batch, controller=0, arm_kp=0.0, arm_kd=0.5, mpc_every=5):
        self.itf = interface; self.lib = interface.lib
        self.B = int(batch); self.controller = int(controller); self.arm_kp = float(arm_kp); self.arm_kd = float(arm_kd); self.mpc_every = int(mpc_every)

    def starting(self):
        """QMController::starting: zeroed observation, nothing commanded, stop flags cleared, the next tick is tick 0 and solves cold"""
        self.itf._check(self.lib.qmhip_tick_reset(self.itf.h, self.B, self.controller, C.c_double(self.arm_kp), C.c_double(self.arm_kd), self.mpc_every), "qmhip_tick_reset")

    def update_submit(self, time, rbd, contact=None, *, horizon, period):
        """one tick, enqueued and not waited for; time [B] (or a scalar), rbd [B][55], contact [B][4] (LF RF LH RH) or None"""
        B = self.B; t = _f(np.broadcast_to(time, (B,))); rbd = _f(rbd, (B, 55))
        ct = None if contact is None else np.ascontiguousarray(contact, dtype=np.int32)
        assert ct is None or ct.shape == (B, 4)
        self.itf._check(self.lib.qmhip_tick_submit(self.itf.h, B, _p(t), _p(rbd), _pi(ct), C.c_double(horizon), C.c_double(period)), "qmhip_tick_submit")

    def update_collect(self):
        """the tick in flight: records [B] of dtype TICK_RECORD (cmd = posDes, velDes, kp, kd, ff x 18, the order QMHWSim.setCommand takes)"""
        rec = np.zeros(self.B, TICK_RECORD)
        self.itf._check(self.lib.qmhip_tick_collect(self.itf.h, self.B, rec.ctypes.data_as(C.c_void_p)), "qmhip_tick_collect")
        return rec

    def update(self, time, rbd, contact=None, *, horizon, period):
        self.update_submit(time, rbd, contact, horizon=horizon, period=period)
        return self.update_collect()

    def fold(self, tick, period, time, rbd, contact, force, mode, wbc_out, qp_status, sim_status=None, mpc_status=None):
        """episode_fold() on this controller's interface: the tick just collected and the plant state behind it into the episode monitor"""
        episode_fold(self.itf, tick, period, time, rbd, contact, force, mode, wbc_out, qp_status, sim_status, mpc_status)


GAIT_MAX_PHASES, GAIT_EVENT_SLOTS = 16, 256
CMD_NONE, CMD_VEL, CMD_EE_VEL, CMD_EE_GOAL = 0, 1, 2, 3


class _TargetParams(C.Structure):
    _fields_ = [("time_to_target", C.c_double), ("target_displacement_velocity", C.c_double), ("target_rotation_velocity", C.c_double), ("com_height", C.c_double)]


class GaitSchedule:
    """B device-resident copies of the reference's GaitSchedule ([upstream ocs2_legged_robot]; built at QMInterface.cpp:455-480) plus the
    template table GaitJoyPublisher loads from gait.info (GaitJoyPublisher.cpp:17-33).  Method names follow the upstream class."""

    def __init__(self, interface, gaits, batch, initial_event_times=(0.5,), initial_mode_sequence=(15, 15), default_gait="stance"):
        """gaits: {name: {"modeSequence": [...], "switchingTimes": [...]}} (scenarios.load_gaits()); initial schedule = reference.info:28-39."""
        self.itf = interface; self.lib = interface.lib; self.B = batch
        self.names = list(gaits.keys())
        G = len(self.names)
        n_ph = np.zeros(G, dtype=np.int32); times = np.zeros((G, GAIT_MAX_PHASES + 1)); modes = np.zeros((G, GAIT_MAX_PHASES), dtype=np.int32)
        for g, name in enumerate(self.names):
            seq, sw = gaits[name]["modeSequence"], gaits[name]["switchingTimes"]
            if len(seq) > GAIT_MAX_PHASES or len(sw) != len(seq) + 1:
                raise ValueError("gait template %r: at most %d phases, switchingTimes one longer than modeSequence" % (name, GAIT_MAX_PHASES))
            n_ph[g] = len(seq); times[g, :len(sw)] = sw; modes[g, :len(seq)] = seq
        self.itf._check(self.lib.qmhip_gait_set_templates(self.itf.h, G, _pi(n_ph), _p(times), _pi(modes)), "qmhip_gait_set_templates")
        ev = _f(initial_event_times); mo = np.ascontiguousarray(initial_mode_sequence, dtype=np.int32)
        self.itf._check(self.lib.qmhip_gait_reset(self.itf.h, batch, len(ev), _p(ev), _pi(mo), self.names.index(default_gait)), "qmhip_gait_reset")

    def insertModeSequenceTemplate(self, gait, start_time, final_time):
        """gait: one name for every instance, or a list of names / None per instance."""
        B = self.B
        req = [gait] * B if (gait is None or isinstance(gait, str)) else list(gait)
        ids = np.array([-1 if g is None else self.names.index(g) for g in req], dtype=np.int32)
        st = _f(np.broadcast_to(np.asarray(start_time, dtype=float), (B,)).copy()); fi = _f(np.broadcast_to(np.asarray(final_time, dtype=float), (B,)).copy())
        self.itf._check(self.lib.qmhip_gait_insert_template(self.itf.h, B, _pi(ids), _p(st), _p(fi)), "qmhip_gait_insert_template")

    def preSolverRun(self, gait, init_time, horizon):
        """GaitReceiver::preSolverRun [upstream]: a received template is inserted at the end of the current horizon; the upstream call passes the
        horizon LENGTH as the tiling bound (insertModeSequenceTemplate(template, finalTime, finalTime − initTime))."""
        init_time = np.broadcast_to(np.asarray(init_time, dtype=float), (self.B,))
        final = init_time + horizon
        self.insertModeSequenceTemplate(gait, final, final - init_time)

    def updateSolverSchedule(self, horizon):
        """SwitchedModelReferenceManager::modifyReferences [upstream]: getModeSchedule(t0 − T, t0 + 2T) for the resident observation times;
        the result becomes the mode schedule of the next MPC iteration."""
        self.itf._check(self.lib.qmhip_gait_update_resident(self.itf.h, self.B, C.c_double(horizon)), "qmhip_gait_update_resident")

    def download(self):
        B = self.B
        n = np.zeros(B, dtype=np.int32); ev = np.zeros((B, GAIT_EVENT_SLOTS)); mo = np.zeros((B, GAIT_EVENT_SLOTS + 1), dtype=np.int32); tp = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        self.itf._check(self.lib.qmhip_gait_download(self.itf.h, B, _pi(n), _p(ev), _pi(mo), _pi(tp), _pi(st)), "qmhip_gait_download")
        return dict(n=n, event_times=ev, mode_sequence=mo, template=tp, status=st)

    def solver_schedule(self):
        B, ne = self.B, self.itf.max_events
        ev = np.zeros((B, ne)); mo = np.zeros((B, ne + 1), dtype=np.int32)
        self.itf._check(self.lib.qmhip_schedule_download(self.itf.h, B, _p(ev), _pi(mo)), "qmhip_schedule_download")
        return ev, mo


class TargetTrajectoriesPublisher:
    """The command callbacks of QmTargetTrajectoriesInteractiveMarker for B robots (QmTargetTrajectoriesPublisher.h:75-112,
    QmTargetTrajectoriesPublisher_node.cpp:44-208): commands in, the solver's resident 2-knot TargetTrajectories out."""

    def __init__(self, interface, batch, time_to_target=None, target_displacement_velocity=0.3, target_rotation_velocity=0.1, com_height=0.4,
                 last_ee_target=(0.52, 0.09, 0.44, 0.5, -0.5, 0.5, -0.5)):
        self.itf = interface; self.lib = interface.lib; self.B = batch
        T = interface.settings_blob[996] if time_to_target is None else time_to_target       # mpc.timeHorizon
        self.params = _TargetParams(T, target_displacement_velocity, target_rotation_velocity, com_height)
        self.itf._check(self.lib.qmhip_target_reset(self.itf.h, batch, _p(_f(last_ee_target, (7,)))), "qmhip_target_reset")

    def publish(self, kind, cmd, ee_state=None, ee_through_float=False):
        """kind[B] in {CMD_NONE, CMD_VEL, CMD_EE_VEL, CMD_EE_GOAL}; cmd[B][7]; ee_state[B][7] (None: forward kinematics of the resident x0)."""
        B = self.B
        kd = np.ascontiguousarray(np.broadcast_to(np.asarray(kind, dtype=np.int32), (B,)), dtype=np.int32)
        cm = _f(cmd, (B, 7)); ee = None if ee_state is None else _f(ee_state, (B, 7))
        self.itf._check(self.lib.qmhip_target_from_command(self.itf.h, B, _pi(kd), _p(cm), _p(ee), int(bool(ee_through_float)), C.byref(self.params)), "qmhip_target_from_command")

    def download(self):
        B, nr = self.B, self.itf.max_ref_knots
        rt = np.zeros((B, nr)); rx = np.zeros((B, nr, 37)); le = np.zeros((B, 7))
        self.itf._check(self.lib.qmhip_target_download(self.itf.h, B, _p(rt), _p(rx), _p(le)), "qmhip_target_download")
        return rt, rx, le
