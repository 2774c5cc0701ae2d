/*
 * qmhip_layout.h — flat f64 "blob" layouts shared across the C-ABI boundary.
 *
 * Two read-only blobs describe everything the hot path needs from the reference's
 * three input files (robot.urdf, task.info, reference.info):
 *   - MODEL blob  : the kinematic tree / inertias as Pinocchio would build them from
 *                   qm_description/urdf/qudraputed_manipulator/robot.urdf with the root joint
 *                   composite(Translation, SphericalZYX)   (qm_interface/src/QMInterface.cpp:408-416)
 *   - SETTINGS blob: the numbers of qm_controllers/config/task.info + reference.info that the
 *                   OCP / SQP / WBC read (qm_interface/src/QMInterface.cpp:64-73,99-131,
 *                   qm_wbc/src/WbcBase.cpp:69-116,565-595, qm_wbc/cfg/wbcWigeht.cfg:7-47)
 * Integers are stored as exact doubles. All matrices row-major.
 *
 * This header only holds constants; it is included by the product (qm_control_amd/csrc) and may be
 * included by the oracle (the oracle depends on the product's public headers, never the reverse).
 */
#ifndef QMHIP_LAYOUT_H
#define QMHIP_LAYOUT_H

/* ---- fixed dimensions of the 24-DoF quadruped-manipulator ---- */
#define QM_NJ 18      /* actuated joints: LF(3) LH(3) RF(3) RH(3) arm(6) — Pinocchio/urdfdom order */
#define QM_NB 19      /* bodies: base + one per joint (fixed-joint children merged)              */
#define QM_NQ 24      /* generalized coordinates = 6 base + 18                                    */
#define QM_NX 30      /* centroidal state  [h_lin/m, h_ang/m, p_base, zyx, q_j]                    */
#define QM_NU 30      /* input             [F_LF, F_RF, F_LH, F_RH, qd_j]                          */
#define QM_NF 5       /* frames of interest: LF_FOOT, RF_FOOT, LH_FOOT, RH_FOOT, arm end-effector   */
#define QM_NREF 37    /* target state = 30 + EE pos(3) + EE quat xyzw(4)                           */
#define QM_NRBD 55    /* measured rbd state, qm_estimation/src/StateEstimateBase.cpp:41-103        */
#define QM_NWBC 36    /* WBC decision x = [vdot(24); F(12)], qm_wbc/src/WbcBase.cpp:36             */
#define QM_NWBC_OUT 54

/* ---- MODEL blob offsets ---- */
#define MB_PARENT    0      /* [18]   parent body of joint j (0 = base, k = body of joint k-1)     */
#define MB_JR        18     /* [18*9] joint placement rotation in the parent body frame           */
#define MB_JP        180    /* [18*3] joint placement translation                                  */
#define MB_AXIS      234    /* [18*3] joint axis in the joint frame                                */
#define MB_QLO       288    /* [18]   lower position limit                                          */
#define MB_QHI       306    /* [18]   upper position limit                                          */
#define MB_TAUMAX    324    /* [18]   effort limit                                                  */
#define MB_MASS      342    /* [19]   body mass (after merging fixed children)                      */
#define MB_COM       361    /* [19*3] body COM in the body (joint) frame                            */
#define MB_INERTIA   418    /* [19*9] body rotational inertia about its COM, body axes              */
#define MB_FPARENT   589    /* [5]    parent body of frame f                                        */
#define MB_FR        594    /* [5*9]  frame placement rotation in the parent body frame             */
#define MB_FP        639    /* [5*3]  frame placement translation                                   */
#define MB_ROBOTMASS 654    /* total mass                                                            */
#define MB_INOM      655    /* [9]    centroidalInertiaNominal (SRBD)                               */
#define MB_RNOM      664    /* [3]    comToBasePositionNominal                                      */
#define MB_QNOM      667    /* [18]   defaultJointState (reference.info:6-26)                       */
#define MB_SIZE      685

/* ---- SETTINGS blob offsets ---- */
#define ST_Q          0     /* [30]  diagonal of Q (task.info:192-233)                              */
#define ST_R          30    /* [900] R after the JᵀR₁₂J leg-block transform (QMInterface.cpp:274-299) */
#define ST_XINIT      930   /* [30]  initialState (task.info:150-189)                               */
#define ST_MU_EE_POS  960   /* endEffector.muPosition                                               */
#define ST_MU_EE_ORI  961
#define ST_MU_EEF_POS 962   /* finalEndEffector.muPosition                                          */
#define ST_MU_EEF_ORI 963
#define ST_FRIC_COEF  964   /* frictionConeSoftConstraint.frictionCoefficient                       */
#define ST_FRIC_MU    965   /* relaxed barrier mu                                                   */
#define ST_FRIC_DELTA 966
#define ST_FRIC_REG   967   /* FrictionConeConstraint::Config regularization (upstream default 25)  */
#define ST_FRIC_SHIFT 968   /* hessianDiagonalShift (upstream default 1e-6)                         */
#define ST_JPOS_MU    969
#define ST_JPOS_DELTA 970
#define ST_JVEL_MU    971
#define ST_JVEL_DELTA 972
#define ST_JVEL_LO    973   /* [6] */
#define ST_JVEL_HI    979   /* [6] */
#define ST_POS_ERR_GAIN 985
#define ST_PHASE_TRANS_STANCE 986
#define ST_LIFTOFF_VEL 987
#define ST_TOUCHDOWN_VEL 988
#define ST_SWING_HEIGHT 989
#define ST_SWING_TIME_SCALE 990
#define ST_SQP_DT     991
#define ST_SQP_ITER   992
#define ST_DELTA_TOL  993
#define ST_G_MAX      994
#define ST_G_MIN      995
#define ST_TIME_HORIZON 996
#define ST_WBC_FRIC   997   /* frictionConeTask.frictionCoefficient (task.info:346-349)             */
#define ST_KP_SWING   998
#define ST_KD_SWING   999
#define ST_KP_BASE_H  1000
#define ST_KD_BASE_H  1001
#define ST_KP_BASE_LIN 1002
#define ST_KD_BASE_LIN 1003
#define ST_KP_BASE_ANG 1004
#define ST_KD_BASE_ANG 1005
#define ST_KP_ARM_J   1006  /* [6] */
#define ST_KD_ARM_J   1012  /* [6] */
#define ST_KP_EE_LIN  1018  /* [3] */
#define ST_KD_EE_LIN  1021  /* [3] */
#define ST_KP_EE_ANG  1024  /* [3] */
#define ST_KD_EE_ANG  1027  /* [3] */
/* discrete iLQR behind the same MPC entry points (settings block `ddp`, task.info:33-71, loaded at QMInterface.cpp:70) */
#define ST_SOLVER     1030  /* 0: multiple-shooting SQP (what QMController instantiates, QMController.cpp:287-288), 1: discrete iLQR, 2: the same multiple-shooting step on the `ipm` block's parameters (NOT an interior-point method, see below); set through qmhip_set_setting */
#define ST_DDP_MIN_STEP 1031 /* ddp.lineSearch.minStepLength (task.info:66)                              */
#define ST_DDP_MAX_STEP 1032 /* ddp.lineSearch.maxStepLength (task.info:67)                              */
#define ST_DDP_PENALTY  1033 /* ddp.constraintPenaltyInitialValue (task.info:56)                         */
/* `ipm` block (task.info:94-125, loaded at QMInterface.cpp:72, never instantiated).  This OCP has NO hard inequality constraints — friction cones and joint limits enter as
   relaxed-barrier soft costs (QMInterface.cpp:79-142) — so there are no slack / dual variables and an interior-point iteration is the equality-constrained multiple-shooting
   step with the filter line search, run with THIS block's dt, iteration count and line-search thresholds (they differ from `sqp`: g_max 10 against 1e-2) */
#define ST_IPM_DT        1034 /* ipm.dt                                                                   */
#define ST_IPM_ITER      1035 /* ipm.ipmIteration                                                         */
#define ST_IPM_DELTA_TOL 1036 /* ipm.deltaTol                                                             */
#define ST_IPM_G_MAX     1037 /* ipm.g_max                                                                */
#define ST_IPM_G_MIN     1038 /* ipm.g_min                                                                */
#define ST_IPM_MU        1039 /* ipm.initialBarrierParameter (carried; no inequality rows to apply it to) */
/* minimum step of the SQP time grid (`dt_min` of [upstream ocs2_oc timeDiscretizationWithEvents], default 10 * numeric_traits::limitEpsilon): a node closer than this to its
   predecessor overwrites it.  The ingestion writes the upstream default, so node schedules are upstream's bit for bit.  With it, a node that falls within weakEpsilon (1e-6)
   BEFORE a gait event opens an interval whose adapted duration (interval end − start, ∓ weakEpsilon at events) is NEGATIVE: that stage's cost blocks (× duration) are negative
   definite and Huu of the Riccati recursion is not positive definite.  The solve SURVIVES that stage (ST_RICCATI_STRICT below) and reports the warning bit
   QM_MPC_WARN_PIVOT; QM_GRID_DT_MIN_ROBUST (the node is merged into the event node instead) stays available through qmhip_set_setting */
#define ST_GRID_DT_MIN 1040
#define QM_GRID_DT_MIN_UPSTREAM 2.220446049250313e-15
#define QM_GRID_DT_MIN_ROBUST   1.0e-5
/* non-positive pivot in the Cholesky factorisation of a stage's Huu.  0 (default): the pivot's reciprocal and column are zeroed — what [upstream, recalled] BLASFEO's
   dpotrf kernels under HPIPM's Riccati factorisation do — so the reduced input of that pivot gets no update on that stage, everything else is solved as if it were not
   there, and the instance's status carries QM_MPC_WARN_PIVOT (a warning: status > 0).  1: strict — the same arithmetic, but the instance reports the hard failure
   status -4 (the behaviour of rounds 1-3) */
#define ST_RICCATI_STRICT 1041
/* MPC status words: 0 ok, < 0 failure (qmhip.h), > 0 warning bits — the solution is valid */
#define QM_MPC_WARN_PIVOT 1
/* hard-inequality interior-point solver (ST_SOLVER = 3): the rest of the `ipm` block (task.info:110-124; defaults [upstream ocs2_ipm ipm::Settings, recalled]
   where a key is missing).  ST_IPM_MU above is initialBarrierParameter. */
#define ST_IPM_MU_TARGET      1042 /* ipm.targetBarrierParameter                */
#define ST_IPM_MU_LINEAR      1043 /* ipm.barrierLinearDecreaseFactor           */
#define ST_IPM_MU_POWER       1044 /* ipm.barrierSuperlinearDecreasePower       */
#define ST_IPM_RED_COST_TOL   1045 /* ipm.barrierReductionCostTol               */
#define ST_IPM_RED_CON_TOL    1046 /* ipm.barrierReductionConstraintTol         */
#define ST_IPM_FTB_MARGIN     1047 /* ipm.fractionToBoundaryMargin              */
#define ST_IPM_PRIMAL_FOR_DUAL 1048 /* ipm.usePrimalStepSizeForDual (0 / 1)     */
#define ST_IPM_SLACK_LB       1049 /* ipm.initialSlackLowerBound                */
#define ST_IPM_DUAL_LB        1050 /* ipm.initialDualLowerBound                 */
#define ST_IPM_SLACK_MARGIN   1051 /* ipm.initialSlackMarginRate                */
#define ST_IPM_DUAL_MARGIN    1052 /* ipm.initialDualMarginRate                 */
/* sqp.useFeedbackPolicy (task.info:89; shipped false).  1: the policy the MPC hands out is the SQP's LINEAR controller u(t, x) = uff(t) + K(t) x
   ([upstream ocs2_sqp multiple_shooting::toPrimalSolution with feedback + LinearController, recalled]: K = Px + Pu K_riccati of the last QP, uff = u* − K x*) —
   the device loops around the plant (qmhip_closed_loop_sim) then evaluate it at the tick's estimated state; 0: the feed-forward policy (u*(t)).  Multiple-shooting
   slots only (ST_SOLVER 0 / 2); qmhip_policy_eval_feedback applies the feedback whatever this slot says (qmhip.h) */
#define ST_FEEDBACK_POLICY    1053
#define ST_SIZE       1056  /* 1054..1055 reserved */
/* inequality rows of a shooting node under ST_SOLVER = 3, in this order: arm joint position boxes (joint k: lower z − lo, upper hi − z; rows 2k, 2k + 1; 12 rows), arm joint
   velocity boxes (rows 12 + 2k, 13 + 2k; 12 rows), friction cone of contact c (row 24 + c; inactive — slack 1, dual 0, no contribution — while the foot swings) */
#define QM_NH 28

/* published gain record (qmhip_policy_publish, "published feedback policy" in qmhip.h): the part of a node's stage record the feedback policy reads, copied by
   qm_policy_publish_kernel (csrc/kernels/k_publish.h) into a double-buffered window of the first W nodes of every instance ([slot][instance][node][PR_SIZE]).  Offsets in
   doubles; every field starts on a 16-byte boundary and the record is a whole number of 16-byte pieces.  A node without a record of its own holds zeros */
#define PR_PP     0     /* [18][30] the Riccati gain K of the last SQP iteration                          */
#define PR_PX     180   /* VIRTUAL base of Px [30][30]: only its rows 12..23 exist, at PR_PX + 360 = 540 ... 899 */
#define PR_SWG    900   /* [4][6]   per contact: the 3 x 2 null-space block of a swing leg               */
#define PR_MODEF  924   /* contact mode of the interval (as double); 925: 0                               */
#define PR_SCAL   926   /* m, the reduced input dimension (as double); 927: 0                             */
#define PR_SIZE   928   /* 7424 bytes                                                                     */

/* contact-mode ids: 8*LF + 4*RF + 2*LH + 1*RH (ocs2_legged_robot MotionPhaseDefinition) */
#define QM_MODE_STANCE 15
#define QM_MODE_LF_RH  9
#define QM_MODE_RF_LH  6
#define QM_MODE_FLY    0

/* node event tags of the SQP time grid (ocs2 AnnotatedTime::Event) */
#define QM_EV_NONE 0
#define QM_EV_PRE  1
#define QM_EV_POST 2

/* record of one control step of one instance as qmhip_step_collect hands it over (qmhip.h, "streamed control-step I/O"): a fixed 1024 bytes, written on the device by
   qm_step_pack_kernel (csrc/kernels/k_io.h) into an instance-major buffer that travels to the host in ONE copy.  QM_STEP_* are offsets in DOUBLES of the f64 part,
   QM_STEP_I_* indices of the int32 words behind it (two 4-byte words per 8-byte slot) */
#define QM_STEP_XDES    0    /* [30] policy state at t0                                                  */
#define QM_STEP_UDES    30   /* [30] policy input at t0                                                  */
#define QM_STEP_WBC     60   /* [54] WBC output [vdot(24), F(12), tau(18)]; zeros without QMHIP_STEP_WBC */
#define QM_STEP_PERF    114  /* [10] perf of qmhip_mpc_download                                          */
#define QM_STEP_DOUBLES 124
#define QM_STEP_I_MODE   0   /* contact mode at t0                                                       */
#define QM_STEP_I_STATUS 1   /* MPC status word as qmhip_mpc_download reports it                         */
#define QM_STEP_I_NODES  2   /* number of nodes of the instance's grid                                   */
#define QM_STEP_I_QP     3   /* [3] WBC status per priority level; zeros without QMHIP_STEP_WBC          */
#define QM_STEP_INTS     8   /* 6, 7 reserved (0)                                                        */
#define QM_STEP_BYTES 1024
#include <stdint.h>
typedef struct qmhip_step_record {
  double x_des[30], u_des[30], wbc_out[54], perf[10];
  int32_t mode, mpc_status, n_nodes, qp_status[3], reserved[2];
} qmhip_step_record;

/* record of one controller tick of one instance as qmhip_tick_collect hands it over (qmhip.h, "streamed controller tick"): a fixed 2048 bytes, packed on the device by
   qm_tick_pack_kernel (csrc/kernels/k_tick.h).  QM_TICK_* are offsets in DOUBLES of the f64 part, QM_TICK_I_* indices of the int32 words behind it */
#define QM_TICK_CMD     0    /* [90] held hybrid joint command: posDes, velDes, kp, kd, ff x 18 (the order qmhip_sim_set_command takes) */
#define QM_TICK_XOBS    90   /* [30] the tick's observation (centroidal state, yaw unwrapped)             */
#define QM_TICK_XDES    120  /* [30] policy state at the observation time                                 */
#define QM_TICK_UDES    150  /* [30] policy input at the observation time                                 */
#define QM_TICK_WBC     180  /* [54] WBC output [vdot(24), F(12), tau(18)]                                */
#define QM_TICK_PERF    234  /* [10] perf of qmhip_mpc_download on a tick that ran the MPC, zeros otherwise */
#define QM_TICK_DOUBLES 244
#define QM_TICK_I_MODE    0  /* planned contact mode at the observation time                              */
#define QM_TICK_I_MEAS    1  /* measured mode 8 LF + 4 RF + 2 LH + RH of the contact flags; -1 without    */
#define QM_TICK_I_STATUS  2  /* MPC status word of the last MPC call, as qmhip_mpc_download reports it    */
#define QM_TICK_I_NODES   3  /* number of nodes of the instance's grid (last MPC call)                    */
#define QM_TICK_I_QP      4  /* [3] WBC status per priority level                                         */
#define QM_TICK_I_SAFETY  7  /* 1: SafetyChecker::checkOrientation failed on THIS tick's observation      */
#define QM_TICK_I_STOPPED 8  /* 1: the instance was stopped by an earlier tick: cmd is the held command   */
#define QM_TICK_I_MPCRAN  9  /* 1: this tick ran the MPC                                                  */
#define QM_TICK_I_TICK    10 /* tick index since qmhip_tick_reset                                         */
#define QM_TICK_INTS      24 /* 11 .. 23 reserved (0)                                                     */
#define QM_TICK_BYTES 2048
typedef struct qmhip_tick_record {
  double cmd[90], x_obs[30], x_des[30], u_des[30], wbc_out[54], perf[10];
  int32_t mode, mode_meas, mpc_status, n_nodes, qp_status[3], safety, stopped, mpc_ran, tick, reserved[13];
} qmhip_tick_record;

/* record of one node of a plan in task space as qmhip_plan_task_space / qmhip_task_space_eval hand it over (qmhip.h, "planned task-space trajectories"): 64 eight-byte
   words, written on the device by the kernels of csrc/kernels/k_plan.h.  PT_* are offsets in 8-byte WORDS.  All vectors in the world frame; feet in CONTACT order
   LF RF LH RH (the order of the input's force triples) */
#define PT_TIME       0    /* node time (0 from qmhip_task_space_eval)                                   */
#define PT_MODE       1    /* two int32: mode id of the node | contact_mask (bit i = foot i in stance)   */
#define PT_BASE_POS   2    /* [3] x[6:9]                                                                 */
#define PT_BASE_ZYX   5    /* [3] x[9:12]                                                                */
#define PT_FOOT_POS   8    /* [4][3] foot frame positions                                                */
#define PT_FOOT_VEL   20   /* [4][3] foot velocities as the zero- / normal-velocity constraints see them */
#define PT_FOOT_FORCE 32   /* [4][3] u[3 i : 3 i + 3]                                                    */
#define PT_EE_POS     44   /* [3] arm end-effector frame position                                        */
#define PT_EE_QUAT    47   /* [4] its orientation, quaternion xyzw                                       */
#define PT_EE_ERR     51   /* [6] EndEffectorConstraint's position / orientation error; zeros without a reference */
#define PT_COP        57   /* [3] centre of pressure x, y over the stance feet; [2] = their summed f_z   */
#define PT_SPARE      60   /* [4] zero                                                                   */
#define QM_PLAN_WORDS 64
#define QM_PLAN_BYTES 512
typedef struct qmhip_plan_record {
  double time;
  int32_t mode, contact_mask;
  double base_pos[3], base_zyx[3], foot_pos[4][3], foot_vel[4][3], foot_force[4][3], ee_pos[3], ee_quat[4], ee_err[6], cop[3], spare[4];
} qmhip_plan_record;
/* one landing of one foot inside the planned horizon (qmhip_plan_footholds): event = index into the instance's schedule, leg in contact order */
#define QM_FOOTHOLD_BYTES 40
typedef struct qmhip_foothold { double time; int32_t leg, event; double pos[3]; } qmhip_foothold;

/* one scheduled external wrench on the batched plant (qmhip.h, "plant disturbances"; qmhip_sim_set_pushes takes [B][K] of them, K <= QM_SIM_MAX_PUSH): active while
   t_on <= t < t_off in absolute plant time; base_force [N] at the base frame origin, base_torque [Nm] a pure couple on the base body, ee_force [N] at the arm's tip
   frame, all in the WORLD frame */
#define QM_SIM_MAX_PUSH 8
#define QM_PUSH_BYTES 96
typedef struct qmhip_push { double t_on, t_off, base_force[3], base_torque[3], ee_force[3], spare; } qmhip_push;

/* ground under one instance of the batched plant (qmhip.h, "plant terrain"; qmhip_sim_set_terrain takes [B] of them beside the height and friction arrays [B][ny][nx],
   2 <= nx, ny <= QM_TERRAIN_MAX): vertex (i, j) of the grid lies at (x0 + i dx, y0 + j dy) in the world frame, dx, dy > 0 */
#define QM_TERRAIN_MAX 16
#define QM_TERRAIN_BYTES 32
typedef struct qmhip_terrain { double x0, y0, dx, dy; } qmhip_terrain;

/* sensor model of one instance of the batched plant (qmhip.h, "sensor model"; qmhip_sim_set_sensors takes [B] of them): what the controller is told is the plant's rbd
   state of `lag` samples ago plus, per group g of the rbd state (0 base zyx angles rbd[0:3], 1 base position [3:6], 2 joint positions [6:24], 3 base angular velocity
   [24:27], 4 base linear velocity [27:30], 5 joint rates [30:48]), a constant bias of standard deviation bias_sigma[g] and white noise of standard deviation sigma[g],
   both drawn from `seed` by integer arithmetic */
#define QM_SENSE_GROUPS 6
#define QM_SENSE_MAX_LAG 8
#define QM_SENSE_BYTES 128
typedef struct qmhip_sensor { uint64_t seed; int32_t lag; int32_t spare0; double sigma[6]; double bias_sigma[6]; double spare[2]; } qmhip_sensor;

/* episode monitor (qmhip.h, "episode monitor"): per-instance running statistics of a device loop, folded behind every tick by the kernels of csrc/kernels/k_episode.h.
   EP_* are offsets in 8-byte WORDS of struct qmhip_episode_summary (32 words: 16 doubles, then 32 int32, two per word; EP_I_* are indices of those int32),
   ES_* offsets in 8-byte words of struct qmhip_episode_sample (64 words: 60 doubles, then 8 int32).  Feet in CONTACT order LF RF LH RH; a mask is 8 LF + 4 RF + 2 LH + RH */
#define EP_T_FIRST        0    /* plant time behind the first folded tick                                  */
#define EP_T_LAST         1    /* plant time behind the last folded tick                                   */
#define EP_T_FALL         2    /* plant time behind the tick that tripped the fall check; 0 while not fallen */
#define EP_MIN_BASE_Z     3    /* min of rbd[5]; + infinity before the first tick                          */
#define EP_MAX_ROLL       4    /* max |rbd[2]|                                                             */
#define EP_MAX_PITCH      5    /* max |rbd[1]|                                                             */
#define EP_MAX_SPEED      6    /* max |rbd[27:30]|                                                         */
#define EP_MAX_EE_POS     7    /* max |rbd[48:51] - anchor position|                                       */
#define EP_SUMSQ_EE_POS   8    /* sum of its squares (RMS = sqrt(sum / folded ticks))                      */
#define EP_MAX_EE_ANG     9    /* max rotation angle between rbd[51:55] and the anchor quaternion          */
#define EP_MAX_TAU_RATIO  10   /* max over joints of |tau_j| / effort limit                                */
#define EP_MAX_FRICTION   11   /* max over feet with f_z > 0 of |f_xy| / f_z                               */
#define EP_MAX_NORMAL     12   /* max f_z                                                                  */
#define EP_JOINT_WORK     13   /* sum over ticks of period * sum_j |tau_j qdot_j|                          */
#define EP_SPARE          14   /* [2] zero                                                                 */
#define EP_INTS           16   /* first word of the int32 part                                             */
#define EP_I_TICKS        0    /* folded ticks (the only counter that advances behind a fall)              */
#define EP_I_FALL_TICK    1    /* tick that tripped the fall check; -1: none                               */
#define EP_I_FALL_CAUSE   2    /* QM_FALL_* bits of that tick                                              */
#define EP_I_SIM_BAD      3    /* ticks with a non-zero plant status                                       */
#define EP_I_MPC_CALLS    4    /* MPC calls folded (words 18 .. 20 belong to qm_episode_mpc_kernel)        */
#define EP_I_MPC_FAILS    5    /* ... with a status < 0                                                    */
#define EP_I_MPC_WARN_OR  6    /* OR of the positive status words                                          */
#define EP_I_MPC_LAST_FAIL 7   /* the last negative status word                                            */
#define EP_I_MPC_FIRST_FAIL 8  /* tick the first failing call observed at; -1: none                        */
#define EP_I_RESERVED     9    /* 0                                                                        */
#define EP_I_WBC_BAD      10   /* [3] ticks with a non-zero qp_status, per priority level                  */
#define EP_I_AIRBORNE     13   /* ticks with no foot in contact                                            */
#define EP_I_MISMATCH     14   /* [4] ticks whose measured contact flag differs from the planned stance bit */
#define EP_I_TOUCHDOWN    18   /* [4] 0 -> 1 transitions of the contact flag                               */
#define EP_I_TAU_OVER     22   /* ticks with a torque ratio > 1                                            */
#define EP_I_SPARE        23   /* [9] zero                                                                 */
#define QM_EP_WORDS 32
#define QM_EP_BYTES 256
#define QM_FALL_HEIGHT 1       /* rbd[5] < min_base_z                                                      */
#define QM_FALL_ROLL   2       /* |rbd[2]| > max_tilt                                                      */
#define QM_FALL_PITCH  4       /* |rbd[1]| > max_tilt                                                      */
#define QM_FALL_NONFINITE 8    /* an entry of rbd is not finite                                            */
/* (a struct TAG, no typedef: qmhip_episode_summary is also the entry point that fills it — write `struct qmhip_episode_summary`) */
struct qmhip_episode_summary {
  double t_first, t_last, t_fall, min_base_z, max_abs_roll, max_abs_pitch, max_base_speed, max_ee_pos_dev, sum_sq_ee_pos_dev, max_ee_ang_dev, max_tau_ratio, max_friction_ratio,
         max_normal_force, joint_work, spare[2];
  int32_t ticks, fall_tick, fall_cause, sim_bad_ticks, mpc_calls, mpc_fail_calls, mpc_warn_or, mpc_last_fail, mpc_first_fail_tick, reserved, wbc_bad_ticks[3], airborne_ticks,
          contact_mismatch_ticks[4], touchdowns[4], tau_over_ticks, ispare[9];
};
#define ES_TIME     0    /* plant time behind the tick                                                     */
#define ES_RBD      1    /* [55] measured state behind the tick                                            */
#define ES_FORCE_Z  56   /* [4] normal contact forces                                                      */
#define ES_INTS     60   /* int32: tick, planned mode | measured contact mask, last folded MPC status | qp_status[0], [1] | qp_status[2], plant status */
#define QM_ES_WORDS 64
#define QM_ES_BYTES 512
typedef struct qmhip_episode_sample {
  double time, rbd[55], force_z[4];
  int32_t tick, mode, contact_mask, mpc_status, qp_status[3], sim_status;
} qmhip_episode_sample;

/* policy rollout (qmhip.h, "policy rollout"): per-row summary and trace sample of qmhip_policy_rollout, written on the device by qm_policy_rollout_kernel
   (csrc/kernels/k_rollout.h).  QM_RS_* are offsets in 8-byte WORDS of struct qmhip_rollout_summary (16 words: 12 doubles, then 8 int32, two per word; QM_RS_I_* are
   indices of those int32), QM_RT_* offsets in 8-byte words of qmhip_rollout_sample (64 words: 61 doubles, then 6 int32).  Folded over all K + 1 evaluation points */
#define QM_RS_T_END       0    /* time reached                                                              */
#define QM_RS_MAX_DEV     1    /* [4] inf-norm of x_k - x_des(tau_k): momentum / base pose / leg joints / arm joints */
#define QM_RS_MAX_FB      5    /* [2] inf-norm of u_k - u_ff(tau_k): contact forces / joint velocities      */
#define QM_RS_MIN_CONE    7    /* min over stance feet of ST_FRIC_COEF F_z - sqrt(F_x^2 + F_y^2); + infinity without a stance foot */
#define QM_RS_MIN_FZ      8    /* min over stance feet of F_z; + infinity without a stance foot             */
#define QM_RS_MAX_SWING   9    /* max over swing feet of |F|_inf                                            */
#define QM_RS_SPARE       10   /* [2] zero                                                                  */
#define QM_RS_INTS        12   /* first word of the int32 part                                              */
#define QM_RS_I_STEPS     0    /* steps taken (K)                                                           */
#define QM_RS_I_EVENTS    1    /* steps that ended on an event of the schedule                              */
#define QM_RS_I_UNCOVERED 2    /* source 1: evaluation points outside the publication window                */
#define QM_RS_I_FLAGS     3    /* QM_ROLLOUT_* bits                                                         */
#define QM_RS_I_SPARE     4    /* [4] zero                                                                  */
#define QM_RS_WORDS 16
#define QM_RS_BYTES 128
#define QM_ROLLOUT_MAX_STEPS 1 /* max_steps reached before t_end                                            */
#define QM_ROLLOUT_NONFINITE 2 /* a step gave a non-finite state: x_end is the last finite one              */
#define QM_ROLLOUT_OUTSIDE   4 /* a query time outside the plan's grid (clamped as the policy entry points clamp) */
/* (a struct TAG, no typedef, like qmhip_episode_summary) */
struct qmhip_rollout_summary {
  double t_end, max_dev[4], max_fb[2], min_cone, min_fz, max_swing_force, spare[2];
  int32_t steps, events, uncovered, flags, ispare[4];
};
#define QM_RT_TIME  0    /* t_k                                                                             */
#define QM_RT_X     1    /* [30] x_k                                                                        */
#define QM_RT_U     31   /* [30] u_k                                                                        */
#define QM_RT_INTS  61   /* int32: mode_k, covered (source 0: always 1), then four zeros                    */
#define QM_RT_WORDS 64
#define QM_RT_BYTES 512
typedef struct qmhip_rollout_sample {
  double t, x[30], u[30];
  int32_t mode, covered, ispare[4];
} qmhip_rollout_sample;
#ifdef __cplusplus
#include <stddef.h>
static_assert(sizeof(struct qmhip_rollout_summary) == QM_RS_BYTES && QM_RS_WORDS * 8 == QM_RS_BYTES && offsetof(struct qmhip_rollout_summary, max_dev) == 8 * QM_RS_MAX_DEV &&
              offsetof(struct qmhip_rollout_summary, max_fb) == 8 * QM_RS_MAX_FB && offsetof(struct qmhip_rollout_summary, min_cone) == 8 * QM_RS_MIN_CONE && offsetof(struct qmhip_rollout_summary, min_fz) == 8 * QM_RS_MIN_FZ &&
              offsetof(struct qmhip_rollout_summary, max_swing_force) == 8 * QM_RS_MAX_SWING && offsetof(struct qmhip_rollout_summary, spare) == 8 * QM_RS_SPARE && offsetof(struct qmhip_rollout_summary, steps) == 8 * QM_RS_INTS &&
              offsetof(struct qmhip_rollout_summary, flags) == 8 * QM_RS_INTS + 4 * QM_RS_I_FLAGS && offsetof(struct qmhip_rollout_summary, ispare) == 8 * QM_RS_INTS + 4 * QM_RS_I_SPARE, "QM_RS_* are the word / int32 offsets of qmhip_rollout_summary (16 eight-byte words)");
static_assert(sizeof(qmhip_rollout_sample) == QM_RT_BYTES && QM_RT_WORDS * 8 == QM_RT_BYTES && offsetof(qmhip_rollout_sample, x) == 8 * QM_RT_X && offsetof(qmhip_rollout_sample, u) == 8 * QM_RT_U &&
              offsetof(qmhip_rollout_sample, mode) == 8 * QM_RT_INTS && offsetof(qmhip_rollout_sample, covered) == 8 * QM_RT_INTS + 4, "QM_RT_* are the word offsets of qmhip_rollout_sample (64 eight-byte words)");
static_assert(sizeof(struct qmhip_episode_summary) == QM_EP_BYTES && QM_EP_WORDS * 8 == QM_EP_BYTES && 8 * EP_INTS + 4 * (EP_I_SPARE + 9) == QM_EP_BYTES, "qmhip_episode_summary is 32 eight-byte words");
static_assert(offsetof(struct qmhip_episode_summary, t_fall) == 8 * EP_T_FALL && offsetof(struct qmhip_episode_summary, min_base_z) == 8 * EP_MIN_BASE_Z && offsetof(struct qmhip_episode_summary, max_ee_pos_dev) == 8 * EP_MAX_EE_POS &&
              offsetof(struct qmhip_episode_summary, joint_work) == 8 * EP_JOINT_WORK && offsetof(struct qmhip_episode_summary, spare) == 8 * EP_SPARE && offsetof(struct qmhip_episode_summary, ticks) == 8 * EP_INTS &&
              offsetof(struct qmhip_episode_summary, mpc_calls) == 8 * EP_INTS + 4 * EP_I_MPC_CALLS && offsetof(struct qmhip_episode_summary, mpc_first_fail_tick) == 8 * EP_INTS + 4 * EP_I_MPC_FIRST_FAIL &&
              offsetof(struct qmhip_episode_summary, wbc_bad_ticks) == 8 * EP_INTS + 4 * EP_I_WBC_BAD && offsetof(struct qmhip_episode_summary, contact_mismatch_ticks) == 8 * EP_INTS + 4 * EP_I_MISMATCH &&
              offsetof(struct qmhip_episode_summary, touchdowns) == 8 * EP_INTS + 4 * EP_I_TOUCHDOWN && offsetof(struct qmhip_episode_summary, tau_over_ticks) == 8 * EP_INTS + 4 * EP_I_TAU_OVER &&
              offsetof(struct qmhip_episode_summary, ispare) == 8 * EP_INTS + 4 * EP_I_SPARE, "EP_* are the word / int32 offsets of qmhip_episode_summary");
static_assert(sizeof(qmhip_episode_sample) == QM_ES_BYTES && QM_ES_WORDS * 8 == QM_ES_BYTES && offsetof(qmhip_episode_sample, rbd) == 8 * ES_RBD && offsetof(qmhip_episode_sample, force_z) == 8 * ES_FORCE_Z &&
              offsetof(qmhip_episode_sample, tick) == 8 * ES_INTS && offsetof(qmhip_episode_sample, sim_status) == 8 * ES_INTS + 28, "ES_* are the word offsets of qmhip_episode_sample");
static_assert(sizeof(qmhip_plan_record) == QM_PLAN_BYTES && QM_PLAN_WORDS * 8 == QM_PLAN_BYTES, "qmhip_plan_record is 64 eight-byte words");
static_assert(offsetof(qmhip_plan_record, mode) == 8 * PT_MODE && offsetof(qmhip_plan_record, contact_mask) == 8 * PT_MODE + 4 && offsetof(qmhip_plan_record, base_pos) == 8 * PT_BASE_POS &&
              offsetof(qmhip_plan_record, base_zyx) == 8 * PT_BASE_ZYX && offsetof(qmhip_plan_record, foot_pos) == 8 * PT_FOOT_POS && offsetof(qmhip_plan_record, foot_vel) == 8 * PT_FOOT_VEL &&
              offsetof(qmhip_plan_record, foot_force) == 8 * PT_FOOT_FORCE && offsetof(qmhip_plan_record, ee_pos) == 8 * PT_EE_POS && offsetof(qmhip_plan_record, ee_quat) == 8 * PT_EE_QUAT &&
              offsetof(qmhip_plan_record, ee_err) == 8 * PT_EE_ERR && offsetof(qmhip_plan_record, cop) == 8 * PT_COP && offsetof(qmhip_plan_record, spare) == 8 * PT_SPARE, "PT_* are the word offsets of qmhip_plan_record");
static_assert(sizeof(qmhip_foothold) == QM_FOOTHOLD_BYTES && offsetof(qmhip_foothold, leg) == 8 && offsetof(qmhip_foothold, event) == 12 && offsetof(qmhip_foothold, pos) == 16, "qmhip_foothold is 40 bytes");
static_assert(sizeof(qmhip_push) == QM_PUSH_BYTES && offsetof(qmhip_push, base_force) == 16 && offsetof(qmhip_push, base_torque) == 40 && offsetof(qmhip_push, ee_force) == 64 && offsetof(qmhip_push, spare) == 88, "qmhip_push is 12 doubles");
static_assert(sizeof(qmhip_terrain) == QM_TERRAIN_BYTES && offsetof(qmhip_terrain, x0) == 0 && offsetof(qmhip_terrain, y0) == 8 && offsetof(qmhip_terrain, dx) == 16 && offsetof(qmhip_terrain, dy) == 24, "qmhip_terrain is 4 doubles");
static_assert(sizeof(qmhip_sensor) == QM_SENSE_BYTES && offsetof(qmhip_sensor, seed) == 0 && offsetof(qmhip_sensor, lag) == 8 && offsetof(qmhip_sensor, spare0) == 12 && offsetof(qmhip_sensor, sigma) == 16 &&
              offsetof(qmhip_sensor, bias_sigma) == 16 + 8 * QM_SENSE_GROUPS && offsetof(qmhip_sensor, spare) == 16 + 16 * QM_SENSE_GROUPS, "qmhip_sensor is 16 eight-byte words");
#endif

#endif
