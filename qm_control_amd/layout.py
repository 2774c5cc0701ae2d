"""Named offsets of the MODEL / SETTINGS blobs: the #defines of include/qmhip_layout.h, read from the header itself
(one source of truth; e.g. layout.ST_SQP_ITER, layout.MB_ROBOTMASS, layout.QM_NX)."""
import os
import re

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qmhip_layout.h")
DEFINES = {}
with open(_HDR) as _fh:
    for _line in _fh:
        _m = re.match(r"#define\s+((?:MB|ST|QM|PR|PT|EP|ES)_\w+)\s+(\d+)\s", _line)
        if _m:
            DEFINES[_m.group(1)] = int(_m.group(2))
            continue
        _m = re.match(r"#define\s+(QM_\w+)\s+(\d+\.\d*(?:[eE][-+]?\d+)?)\s", _line)      # floating-point constants (QM_GRID_DT_MIN_*)
        if _m:
            DEFINES[_m.group(1)] = float(_m.group(2))
globals().update(DEFINES)

# struct qmhip_step_record (include/qmhip_layout.h): (field, numpy type, count, byte offset) — the offsets follow from the QM_STEP_* defines above
STEP_RECORD_FIELDS = [("x_des", "<f8", 30, 8 * QM_STEP_XDES), ("u_des", "<f8", 30, 8 * QM_STEP_UDES), ("wbc_out", "<f8", 54, 8 * QM_STEP_WBC), ("perf", "<f8", 10, 8 * QM_STEP_PERF),
                      ("mode", "<i4", 1, 8 * QM_STEP_DOUBLES + 4 * QM_STEP_I_MODE), ("mpc_status", "<i4", 1, 8 * QM_STEP_DOUBLES + 4 * QM_STEP_I_STATUS),
                      ("n_nodes", "<i4", 1, 8 * QM_STEP_DOUBLES + 4 * QM_STEP_I_NODES), ("qp_status", "<i4", 3, 8 * QM_STEP_DOUBLES + 4 * QM_STEP_I_QP),
                      ("reserved", "<i4", 2, 8 * QM_STEP_DOUBLES + 4 * (QM_STEP_I_QP + 3))]

# struct qmhip_tick_record (include/qmhip_layout.h), same form, from the QM_TICK_* defines
_TI = 8 * QM_TICK_DOUBLES
TICK_RECORD_FIELDS = [("cmd", "<f8", 90, 8 * QM_TICK_CMD), ("x_obs", "<f8", 30, 8 * QM_TICK_XOBS), ("x_des", "<f8", 30, 8 * QM_TICK_XDES), ("u_des", "<f8", 30, 8 * QM_TICK_UDES),
                      ("wbc_out", "<f8", 54, 8 * QM_TICK_WBC), ("perf", "<f8", 10, 8 * QM_TICK_PERF),
                      ("mode", "<i4", 1, _TI + 4 * QM_TICK_I_MODE), ("mode_meas", "<i4", 1, _TI + 4 * QM_TICK_I_MEAS), ("mpc_status", "<i4", 1, _TI + 4 * QM_TICK_I_STATUS),
                      ("n_nodes", "<i4", 1, _TI + 4 * QM_TICK_I_NODES), ("qp_status", "<i4", 3, _TI + 4 * QM_TICK_I_QP), ("safety", "<i4", 1, _TI + 4 * QM_TICK_I_SAFETY),
                      ("stopped", "<i4", 1, _TI + 4 * QM_TICK_I_STOPPED), ("mpc_ran", "<i4", 1, _TI + 4 * QM_TICK_I_MPCRAN), ("tick", "<i4", 1, _TI + 4 * QM_TICK_I_TICK),
                      ("reserved", "<i4", 13, _TI + 4 * (QM_TICK_I_TICK + 1))]

# struct qmhip_plan_record (include/qmhip_layout.h), same form, from the PT_* word offsets; struct qmhip_foothold
PLAN_RECORD_FIELDS = [("time", "<f8", 1, 8 * PT_TIME), ("mode", "<i4", 1, 8 * PT_MODE), ("contact_mask", "<i4", 1, 8 * PT_MODE + 4), ("base_pos", "<f8", 3, 8 * PT_BASE_POS), ("base_zyx", "<f8", 3, 8 * PT_BASE_ZYX),
                      ("foot_pos", "<f8", (4, 3), 8 * PT_FOOT_POS), ("foot_vel", "<f8", (4, 3), 8 * PT_FOOT_VEL), ("foot_force", "<f8", (4, 3), 8 * PT_FOOT_FORCE),
                      ("ee_pos", "<f8", 3, 8 * PT_EE_POS), ("ee_quat", "<f8", 4, 8 * PT_EE_QUAT), ("ee_err", "<f8", 6, 8 * PT_EE_ERR), ("cop", "<f8", 3, 8 * PT_COP), ("spare", "<f8", 4, 8 * PT_SPARE)]
FOOTHOLD_FIELDS = [("time", "<f8", 1, 0), ("leg", "<i4", 1, 8), ("event", "<i4", 1, 12), ("pos", "<f8", 3, 16)]
# struct qmhip_push (include/qmhip_layout.h): one scheduled external wrench on the plant
PUSH_FIELDS = [("t_on", "<f8", 1, 0), ("t_off", "<f8", 1, 8), ("base_force", "<f8", 3, 16), ("base_torque", "<f8", 3, 40), ("ee_force", "<f8", 3, 64), ("spare", "<f8", 1, 88)]
# struct qmhip_terrain (include/qmhip_layout.h): origin and spacing of one instance's ground grid (QM_TERRAIN_MAX, QM_TERRAIN_BYTES come from the header above)
TERRAIN_FIELDS = [("x0", "<f8", 1, 0), ("y0", "<f8", 1, 8), ("dx", "<f8", 1, 16), ("dy", "<f8", 1, 24)]
# struct qmhip_sensor (include/qmhip_layout.h): the sensor model of one instance of the plant
SENSOR_FIELDS = [("seed", "<u8", 1, 0), ("lag", "<i4", 1, 8), ("spare0", "<i4", 1, 12), ("sigma", "<f8", 6, 16), ("bias_sigma", "<f8", 6, 64), ("spare", "<f8", 2, 112)]

# struct qmhip_episode_summary / qmhip_episode_sample (include/qmhip_layout.h, the episode monitor), same form, from the EP_* / ES_* word offsets
_EI = 8 * EP_INTS
EPISODE_SUMMARY_FIELDS = [("t_first", "<f8", 1, 8 * EP_T_FIRST), ("t_last", "<f8", 1, 8 * EP_T_LAST), ("t_fall", "<f8", 1, 8 * EP_T_FALL), ("min_base_z", "<f8", 1, 8 * EP_MIN_BASE_Z),
                          ("max_abs_roll", "<f8", 1, 8 * EP_MAX_ROLL), ("max_abs_pitch", "<f8", 1, 8 * EP_MAX_PITCH), ("max_base_speed", "<f8", 1, 8 * EP_MAX_SPEED),
                          ("max_ee_pos_dev", "<f8", 1, 8 * EP_MAX_EE_POS), ("sum_sq_ee_pos_dev", "<f8", 1, 8 * EP_SUMSQ_EE_POS), ("max_ee_ang_dev", "<f8", 1, 8 * EP_MAX_EE_ANG),
                          ("max_tau_ratio", "<f8", 1, 8 * EP_MAX_TAU_RATIO), ("max_friction_ratio", "<f8", 1, 8 * EP_MAX_FRICTION), ("max_normal_force", "<f8", 1, 8 * EP_MAX_NORMAL),
                          ("joint_work", "<f8", 1, 8 * EP_JOINT_WORK), ("spare", "<f8", 2, 8 * EP_SPARE),
                          ("ticks", "<i4", 1, _EI + 4 * EP_I_TICKS), ("fall_tick", "<i4", 1, _EI + 4 * EP_I_FALL_TICK), ("fall_cause", "<i4", 1, _EI + 4 * EP_I_FALL_CAUSE),
                          ("sim_bad_ticks", "<i4", 1, _EI + 4 * EP_I_SIM_BAD), ("mpc_calls", "<i4", 1, _EI + 4 * EP_I_MPC_CALLS), ("mpc_fail_calls", "<i4", 1, _EI + 4 * EP_I_MPC_FAILS),
                          ("mpc_warn_or", "<i4", 1, _EI + 4 * EP_I_MPC_WARN_OR), ("mpc_last_fail", "<i4", 1, _EI + 4 * EP_I_MPC_LAST_FAIL),
                          ("mpc_first_fail_tick", "<i4", 1, _EI + 4 * EP_I_MPC_FIRST_FAIL), ("reserved", "<i4", 1, _EI + 4 * EP_I_RESERVED), ("wbc_bad_ticks", "<i4", 3, _EI + 4 * EP_I_WBC_BAD),
                          ("airborne_ticks", "<i4", 1, _EI + 4 * EP_I_AIRBORNE), ("contact_mismatch_ticks", "<i4", 4, _EI + 4 * EP_I_MISMATCH), ("touchdowns", "<i4", 4, _EI + 4 * EP_I_TOUCHDOWN),
                          ("tau_over_ticks", "<i4", 1, _EI + 4 * EP_I_TAU_OVER), ("ispare", "<i4", 9, _EI + 4 * EP_I_SPARE)]
_SI = 8 * ES_INTS
EPISODE_SAMPLE_FIELDS = [("time", "<f8", 1, 8 * ES_TIME), ("rbd", "<f8", 55, 8 * ES_RBD), ("force_z", "<f8", 4, 8 * ES_FORCE_Z), ("tick", "<i4", 1, _SI), ("mode", "<i4", 1, _SI + 4),
                         ("contact_mask", "<i4", 1, _SI + 8), ("mpc_status", "<i4", 1, _SI + 12), ("qp_status", "<i4", 3, _SI + 16), ("sim_status", "<i4", 1, _SI + 28)]

# struct qmhip_rollout_summary / qmhip_rollout_sample (include/qmhip_layout.h, the policy rollout), same form, from the QM_RS_* / QM_RT_* word offsets
_RI = 8 * QM_RS_INTS
ROLLOUT_SUMMARY_FIELDS = [("t_end", "<f8", 1, 8 * QM_RS_T_END), ("max_dev", "<f8", 4, 8 * QM_RS_MAX_DEV), ("max_fb", "<f8", 2, 8 * QM_RS_MAX_FB), ("min_cone", "<f8", 1, 8 * QM_RS_MIN_CONE),
                          ("min_fz", "<f8", 1, 8 * QM_RS_MIN_FZ), ("max_swing_force", "<f8", 1, 8 * QM_RS_MAX_SWING), ("spare", "<f8", 2, 8 * QM_RS_SPARE),
                          ("steps", "<i4", 1, _RI + 4 * QM_RS_I_STEPS), ("events", "<i4", 1, _RI + 4 * QM_RS_I_EVENTS), ("uncovered", "<i4", 1, _RI + 4 * QM_RS_I_UNCOVERED),
                          ("flags", "<i4", 1, _RI + 4 * QM_RS_I_FLAGS), ("ispare", "<i4", 4, _RI + 4 * QM_RS_I_SPARE)]
ROLLOUT_SAMPLE_FIELDS = [("t", "<f8", 1, 8 * QM_RT_TIME), ("x", "<f8", 30, 8 * QM_RT_X), ("u", "<f8", 30, 8 * QM_RT_U), ("mode", "<i4", 1, 8 * QM_RT_INTS), ("covered", "<i4", 1, 8 * QM_RT_INTS + 4),
                         ("ispare", "<i4", 4, 8 * QM_RT_INTS + 8)]
