/*
 * qmhip.h — C ABI of libqmhip.so: the MI355X-native MPC + whole-body-control step of qm_control.
 *
 * The reference has no FFI; its seams are three C++ interfaces.  Each entry point below
 * names the reference interface it stands behind; INTEGRATION.md shows the thin C++ adaptors
 * (qm::QMInterface-, ocs2::MPC_BASE-, qm::WbcBase-shaped) a maintainer adds on the reference side.
 *
 * Conventions: plain pointers + sizes, no C++/torch types; f64 everywhere (ocs2::scalar_t); arrays are
 * instance-major and caller owned; pointers are HOST memory unless the name says `_dev`.
 * Return value 0 = ok, negative = error (qmhip_last_error gives the text).
 *
 * Threads.  Every entry point that takes a context locks it: calls on ONE context from several threads are safe and run one after another (a blocked
 * caller waits for the other call's host work, e.g. the launches of an MPC solve — since round 6 the SQP solve only enqueues, its line search no longer waits for the device —).  The reference runs the MPC in `mpcThread_` (advanceMpc,
 * qm_controllers/src/QMController.cpp:315-333) beside the ros_control thread's WbcBase::update (QMController.cpp:128-147); for that layout the control thread
 * gets its OWN context from qmhip_create_wbc_context: own streams, own device copies of the model, own error string — a control tick then never waits for,
 * and is never reordered by, an MPC solve in flight (tests/c_abi_threads.c).  Different contexts share nothing mutable; qmhip_last_error(NULL) is per thread.
 */
#ifndef QMHIP_H
#define QMHIP_H
#include <stdint.h>
#include "qmhip_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qmhip_ctx qmhip_ctx;

/* ---- construction: replaces qm::QMInterface(taskFile, urdfFile, referenceFile) + setupOptimalControlProblem
 *      (qm_interface/include/qm_interface/QMInterface.h:31-35, qm_interface/src/QMInterface.cpp:37-142) and the
 *      WBC constructor / loadTasksSetting (qm_wbc/include/qm_wbc/WbcBase.h:28-34).
 *      Missing files -> QMHIP_ERR_FILE, like the reference's std::invalid_argument (QMInterface.cpp:45,53,61).
 *      3 <= max_nodes <= 512 (horizon nodes incl. event-split nodes; the per-instance node list lives in LDS), else QMHIP_ERR_ARG.
 *      Device memory: ~ 35 KB per (instance, node) — the stage record (30 KB; rounds 1-4: 58.9), the kinematics record (3 KB), iterate / step / reference arrays — measured
 *      (free device memory around the call, profiles/r05_context_footprint.json): 35.8 KB per (instance, node), 4.7 GB for max_batch 1024 x max_nodes 128, 34 GB for BASELINE config 4 on
 *      one device at 8192 x 116 (its instances use <= 110 nodes) and 37.5 GB at 8192 x 128; an allocation that does not fit returns QMHIP_ERR_HIP with the runtime's message. */
int qmhip_create(const char* urdf_file, const char* task_file, const char* reference_file,
                 int device, int max_batch, int max_nodes, int max_ref_knots, int max_events, qmhip_ctx** out);
/* same, from the flat MODEL / SETTINGS blobs of qmhip_layout.h (no file I/O).  The blobs carry no size stamp: model_blob must hold MB_SIZE and settings_blob ST_SIZE doubles of THIS
 *      header's layout (a shorter array of an older layout is read past its end); the slots whose garbage would steer a kernel's control flow are range-checked (QMHIP_ERR_MODEL) */
int qmhip_create_from_blobs(const double* model_blob, const double* settings_blob,
                            int device, int max_batch, int max_nodes, int max_ref_knots, int max_events, qmhip_ctx** out);
/* WBC-only context for the control thread (see "Threads" above): the parent's model and settings VALUES (copied; later qmhip_set_setting calls go to whichever
 * context they name — WBC gains to this one), the WBC buffers for max_batch instances, the WBC stream.  It serves qmhip_wbc_step / qmhip_wbc_reset / qmhip_wbc_download /
 * qmhip_set_setting / the instrumentation calls; every MPC, front-end and plant entry point returns QMHIP_ERR_STATE on it.  Replaces nothing new in the reference:
 * it is the `wbc_` object of QMController (QMController.h:80, constructed in setupWbc, QMController.cpp:272-276) as opposed to its `mpc_`. */
int qmhip_create_wbc_context(const qmhip_ctx* parent, int max_batch, qmhip_ctx** out);
void qmhip_destroy(qmhip_ctx* ctx);
const char* qmhip_last_error(const qmhip_ctx* ctx);            /* ctx may be NULL: error of the last failed create */
/* parse only (host): what getPinocchioInterface()/getCentroidalModelInfo()/settings getters expose
 * (QMInterface.h:37-54), as blobs */
int qmhip_parse_model(const char* urdf_file, const char* task_file, const char* reference_file,
                      double* model_blob /*[MB_SIZE]*/, double* settings_blob /*[ST_SIZE]*/);
int qmhip_export_blobs(const qmhip_ctx* ctx, double* model_blob, double* settings_blob);
int qmhip_set_setting(qmhip_ctx* ctx, int settings_index, double value);   /* e.g. WBC gains: dynamic_reconfigure callback, WbcBase.cpp:69-116 */
/* settings index of a WBC gain by the name it carries in the reference's dynamic_reconfigure config (qm_wbc/cfg/wbcWigeht.cfg:7-47, assigned in
 * WbcBase::dynamicCallback, qm_wbc/src/WbcBase.cpp:69-116): "kp_swing" -> ST_KP_SWING, "baseHeightKp" -> ST_KP_BASE_H, "kp_arm_joint_3" -> ST_KP_ARM_J + 2,
 * "kd_ee_angular_y" -> ST_KD_EE_ANG + 1, ...; -1 for a name the callback does not read (d_ee_x ... da_ee_x) or an unknown one.  Host-only, no context:
 * adaptors/QmhipWbc.h feeds every entry of the server's `parameter_updates` message through it into qmhip_set_setting. */
int qmhip_wbc_gain_index(const char* reconfigure_name);

/* ---- MPC: replaces ocs2::MPC_BASE::run(t, x) on the SqpMpc the reference installs
 *      (qm_controllers/src/QMController.cpp:287-288,315-323) for B independent instances: one multiple-shooting
 *      SQP iteration (task.info:75-92; `sqp.sqpIteration` of them, shipped 1 — settable through qmhip_set_setting(ST_SQP_ITER)) from a cold start.
 *      Inputs per instance: initial time/state, target trajectory knots (37-dim, QmTargetTrajectoriesPublisher_node.cpp:44-68),
 *      contact-mode schedule (event times + mode ids, modes has n_events+1 entries).
 *      Outputs (any may be NULL): node count, node times / event tags / modes (int, bit-exact), optimal state and
 *      input trajectories (primal solution: input of event nodes copied from the previous node, last input repeated),
 *      perf[10] = baseline{merit,cost,dynSSE,eqSSE}, after-step{...}, step size alpha, armijo metric.
 *      status[b]: 0 ok; < 0 failure: -1 node buffer too small, -2 swing phase not enclosed by stance in the schedule, -3 device gait schedule over capacity,
 *      -4 Riccati failed (indefinite stage of positive duration / NaN; with ST_RICCATI_STRICT also the degenerate stage); > 0 WARNING bits on a valid solution: QM_MPC_WARN_PIVOT (1) = a stage's Huu had non-positive pivots, which were
 *      zeroed ([upstream, recalled] BLASFEO / HPIPM behaviour; qmhip_layout.h) — the stage in front of a gait event when a shooting node falls within weakEpsilon
 *      before it, i.e. about one call in 3700 for an MPC thread on continuous time (QMController.cpp:315-330); on a fixed-rate clock that shares a raster with the gait
 *      events 3 % ... 12 % of the calls (profiles/r04_fixed_rate_report.txt).  Such a solve lies within 5e-6 (per block) of the solve on the robust grid everywhere but the
 *      degenerate interval's own input, its policy at t0 within 5e-6 (measured 2.8e-6; tests/test_gpu_mpc.py); rastered controllers should set ST_GRID_DT_MIN = QM_GRID_DT_MIN_ROBUST
 *      (INTEGRATION.md section 3).  Callers treat status >= 0 as success.  -4 also reports: a non-positive pivot on a stage of POSITIVE duration, a pivot or a step that is
 *      not a finite number (e.g. a NaN in x0) — never a warning.
 *      Solver slot (qmhip_set_setting(ST_SOLVER, .)): 0 the SQP above; 1 a discrete iLQR on the `ddp` block (task.info:33-71); 2 the SAME multiple-shooting step as
 *      slot 0, run with the `ipm` block's parameters (task.info:94-125: ipm.dt / ipmIteration / deltaTol / g_max / g_min, ST_IPM_*) — kept for compatibility, NOT an
 *      interior-point method; 3 (round 5) a primal-dual INTERIOR-POINT method with HARD inequality constraints: the friction cone of every stance foot and the arm joint
 *      position / velocity boxes are constraints h(x, u) >= 0 (QM_NH = 28 rows per node, qmhip_layout.h) instead of relaxed-barrier costs — slack and dual per row,
 *      condensing into the stage cost, fraction-to-the-boundary step limits, the filter line search on the barrier merit, barrier-parameter update, all on the rest of the
 *      `ipm` block (ST_IPM_MU ... ST_IPM_DUAL_MARGIN); csrc/kernels/k_ipm.h, oracle/src/ipm.h.  The reference registers cones and limits as soft costs only
 *      (QMInterface.cpp:79-142) and instantiates no IpmMpc (it loads both blocks, QMInterface.cpp:70-72): slot 3 solves a DIFFERENT problem than the controller's, has no
 *      reference instance to match, and is checked against the oracle, which is pinned by a dense solve of the horizon's primal-dual Newton system (tests/test_ipm.py).
 *      Slack / dual / per-instance {barrier, alphaP, alphaD, dual step} can be read through qmhip_debug_read("ipm_s" | "ipm_l" | "ipm_info", ...). */
int qmhip_mpc_step(qmhip_ctx* ctx, int B, const double* t0, const double* x0 /*[B][30]*/,
                   int n_ref, const double* ref_t /*[B][n_ref]*/, const double* ref_x /*[B][n_ref][37]*/,
                   int n_events, const double* event_times /*[B][n_events]*/, const int32_t* modes /*[B][n_events+1]*/,
                   double horizon,
                   int32_t* out_num_nodes /*[B]*/, double* out_t /*[B][max_nodes]*/, int32_t* out_event /*[B][max_nodes]*/,
                   int32_t* out_mode /*[B][max_nodes]*/, double* out_x /*[B][max_nodes][30]*/, double* out_u /*[B][max_nodes][30]*/,
                   double* out_perf /*[B][10]*/, int32_t* status /*[B]*/);

/* split form used by the benchmark (inputs resident in HBM before the timed region):
 * upload -> solve (device only, asynchronous on the context stream) -> download */
int qmhip_mpc_upload(qmhip_ctx* ctx, int B, const double* t0, const double* x0, int n_ref, const double* ref_t, const double* ref_x,
                     int n_events, const double* event_times, const int32_t* modes);
int qmhip_mpc_solve_resident(qmhip_ctx* ctx, int B, double horizon);
int qmhip_mpc_download(qmhip_ctx* ctx, int B, int32_t* out_num_nodes, double* out_t, int32_t* out_event, int32_t* out_mode,
                       double* out_x, double* out_u, double* out_perf, int32_t* status);

/* ---- receding horizon: what ocs2::MPC_BASE::run does on every call after the first one
 *      (`mpc.coldStart false`, task.info:142): the SqpSolver keeps its primal solution and the next iteration starts from its
 *      interpolation ([upstream ocs2_sqp multiple_shooting::initializeStateInputTrajectories]; the a9 initializer only beyond it).
 *      set_initial: new observation (t, x) per instance — MPC_MRT_Interface::setCurrentObservation (QMController.cpp:133-137); references,
 *      schedule and the previous solution stay resident.  solve_resident_warm falls back to the cold start if there is no previous solve.
 *      advance_resident: perfect-tracking plant for back-to-back steps without host round trips: t0 += dt, x0 <- policy state at the new t0.
 *      closed_loop_resident: n_steps x [advance (not on the first step), warm solve, policy at t0, WBC on the state built from x0]; when the gait
 *      front-end below has been reset for this batch, every step first refreshes the mode schedule (qmhip_gait_update_resident). */
int qmhip_mpc_set_initial(qmhip_ctx* ctx, int B, const double* t0, const double* x0 /*[B][30]*/);
/*      update_references: new target trajectories and / or mode schedule for the NEXT call, the previous primal solution kept for its warm start — what
 *      ReferenceManager::preSolverRun leaves behind before every MPC_BASE::run (RosReferenceManager's target subscriber, GaitReceiver's template insertion,
 *      QMController.cpp:296-303).  Either pair may be NULL (left as is).  B must be the batch of the last upload. */
int qmhip_mpc_update_references(qmhip_ctx* ctx, int B, int n_ref, const double* ref_t /*[B][n_ref]*/, const double* ref_x /*[B][n_ref][37]*/,
                                int n_events, const double* event_times /*[B][n_events]*/, const int32_t* modes /*[B][n_events+1]*/);
int qmhip_mpc_solve_resident_warm(qmhip_ctx* ctx, int B, double horizon);
int qmhip_mpc_advance_resident(qmhip_ctx* ctx, int B, double dt);
int qmhip_closed_loop_resident(qmhip_ctx* ctx, int B, int n_steps, double mpc_dt, double horizon, double period, double time0);

/* ---- reference / gait front-end, batched and device resident.
 *      Gait side — replaces, per instance, the reference's GaitSchedule object (constructed at qm_interface/src/QMInterface.cpp:455-480 from
 *      reference.info:28-52 with phaseTransitionStanceTime, task.info:11) and the two calls made on it around every MPC iteration
 *      ([upstream ocs2_legged_robot] GaitReceiver::preSolverRun -> GaitSchedule::insertModeSequenceTemplate(template, finalTime, timeHorizon);
 *      SwitchedModelReferenceManager::modifyReferences -> GaitSchedule::getModeSchedule(initTime - T, finalTime + T)), fed by the templates
 *      GaitJoyPublisher loads from gait.info (qm_controllers/src/GaitJoyPublisher.cpp:17-33).
 *      set_templates: the table of mode-sequence templates, n_phases[g] <= QMHIP_GAIT_MAX_PHASES, switching_times[g][QMHIP_GAIT_MAX_PHASES + 1],
 *                     mode_sequence[g][QMHIP_GAIT_MAX_PHASES] (mode id = 8 LF + 4 RF + 2 LH + RH).
 *      reset:         every instance starts from the initial mode schedule (event_times[n_events], mode_sequence[n_events + 1]) and template
 *                     `default_template`; B is the batch size of all later gait calls.
 *      insert_template: insertModeSequenceTemplate for the instances with template_id[b] >= 0 (host arrays [B]).
 *      update_resident: getModeSchedule(t0 - T, t0 + 2T) on every instance (t0 = the resident observation time, T = horizon); the result
 *                     becomes the solver's mode schedule (same buffers qmhip_mpc_upload fills; needs n_events <= max_events, else status -3).
 *                     Event times are produced by the reference's additions in the reference's order: bit-exact.
 *      download / schedule_download: test access to the per-instance GaitSchedule state ([B][QMHIP_GAIT_EVENT_SLOTS], [B][.. + 1]) and to
 *                     the solver's schedule buffers ([B][max_events], [B][max_events + 1]). */
#define QMHIP_GAIT_MAX_PHASES 16
#define QMHIP_GAIT_EVENT_SLOTS 256
int qmhip_gait_set_templates(qmhip_ctx* ctx, int n_gaits, const int32_t* n_phases, const double* switching_times, const int32_t* mode_sequence);
int qmhip_gait_reset(qmhip_ctx* ctx, int B, int n_events, const double* event_times, const int32_t* mode_sequence, int default_template);
int qmhip_gait_insert_template(qmhip_ctx* ctx, int B, const int32_t* template_id, const double* start_time, const double* final_time);
int qmhip_gait_update_resident(qmhip_ctx* ctx, int B, double horizon);
int qmhip_gait_download(qmhip_ctx* ctx, int B, int32_t* n_events, double* event_times, int32_t* mode_sequence, int32_t* template_id, int32_t* status);
int qmhip_schedule_download(qmhip_ctx* ctx, int B, double* event_times /*[B][max_events]*/, int32_t* modes /*[B][max_events + 1]*/);

/*      Target side — replaces the three command callbacks of QmTargetTrajectoriesInteractiveMarker
 *      (qm_controllers/include/qm_controllers/QmTargetTrajectoriesPublisher.h:75-112, QmTargetTrajectoriesPublisher.cpp:94-109) and the
 *      conversion functions of qm_controllers/src/QmTargetTrajectoriesPublisher_node.cpp: kind 1 cmdVelToTargetTrajectories (:71-116),
 *      2 EeCmdVelToTargetTrajectories (:121-165), 3 EEgoalPoseToTargetTrajectories (:172-208), all through targetPoseToTargetTrajectories
 *      (:44-68); kind 0 leaves the instance's target untouched.  The observation is the resident (t0, x0); ee_state[B][7] (position, quaternion
 *      xyzw) may be null: forward kinematics of x0.  ee_through_float != 0 rounds the EE state to float like the qm_msgs::ee_state message does
 *      (QMController.cpp:246-256).  The 2 knots are written into the solver's target buffers (spare knots of max_ref_knots hold the last one);
 *      lastEeTarget_ (QmTargetTrajectoriesPublisher.h:52-54) is per-instance device state, set by target_reset. */
typedef struct qmhip_target_params {
  double time_to_target;                 /* mpc.timeHorizon, task.info:140 (TIME_TO_TARGET, _node.cpp:226) */
  double target_displacement_velocity;   /* reference.info:1 */
  double target_rotation_velocity;       /* reference.info:2 */
  double com_height;                     /* reference.info:4 */
} qmhip_target_params;
int qmhip_target_reset(qmhip_ctx* ctx, int B, const double* last_ee_target /*[7]*/);
int qmhip_target_from_command(qmhip_ctx* ctx, int B, const int32_t* kind /*[B]*/, const double* cmd /*[B][7]*/, const double* ee_state /*[B][7] or NULL*/,
                              int ee_through_float, const qmhip_target_params* params);
int qmhip_target_download(qmhip_ctx* ctx, int B, double* ref_t /*[B][max_ref_knots]*/, double* ref_x /*[B][max_ref_knots][37]*/, double* last_ee_target /*[B][7]*/);

/* ---- policy evaluation: replaces MPC_MRT_Interface::evaluatePolicy (call site QMController.cpp:139-142):
 *      linear interpolation of the last primal solution at time t[b] */
int qmhip_policy_eval(qmhip_ctx* ctx, int B, const double* t, double* x_des /*[B][30]*/, double* u_des /*[B][30]*/, int32_t* mode /*[B]*/);
/* ---- feedback policy: what the same call returns when task.info says `sqp.useFeedbackPolicy true` (task.info:89, settings slot ST_FEEDBACK_POLICY): evaluatePolicy is
 *      given the MEASURED state (QMController.cpp:139-142) and the SQP hands out a LinearController u(t, x) = uff(t) + K(t) x instead of a FeedforwardController
 *      ([upstream ocs2_sqp multiple_shooting::toPrimalSolution / LinearController::computeInput, recalled]).  Per node with an input of its own, from the LAST SQP iteration:
 *      K = Px + Pu K_riccati (30 x 30; the Riccati gain remapped through the constraint projection), uff = u* − K x*; a PreEvent node and the terminal node carry the
 *      pair of the node their input was copied from.  Bias and gain are interpolated linearly in time like the feed-forward policy.
 *      policy_eval_feedback: u_des = the linear controller at (t[b], x[b]); x_des and mode as qmhip_policy_eval.  ALWAYS applies the feedback, whatever ST_FEEDBACK_POLICY
 *        says (the slot steers the device loops around the plant, below); x == NULL: exactly qmhip_policy_eval.
 *      mpc_download_feedback: what ocs2::LinearController holds — gain [B][max_nodes][30][30], uff [B][max_nodes][30], on the time stamps qmhip_mpc_download returns
 *        (nodes behind an instance's grid: zeros); either may be NULL.  Assembled on the device on request only (a tick needs two nodes).
 *      Both read the stage records of the last solve: valid from the end of a solve until the next solve on this context starts.  QMHIP_ERR_STATE before any solve (or
 *      after an upload / reset / solver switch) and while a qmhip_step_submit is in flight; QMHIP_ERR_ARG with ST_SOLVER 1 (iLQR) or 3 (interior point): the
 *      multiple-shooting slots 0 / 2 only — never a silently feed-forward answer.  A stage whose pivots were zeroed (QM_MPC_WARN_PIVOT) contributes the gain the
 *      factorisation left there (zero rows of K_riccati).  qmhip_step_submit / _collect and qmhip_control_step_resident evaluate at t0 with the state the solve started
 *      from, where x − x*_0 = 0: the two policies coincide there and those entry points do not depend on the slot. */
int qmhip_policy_eval_feedback(qmhip_ctx* ctx, int B, const double* t /*[B]*/, const double* x /*[B][30] or NULL*/,
                               double* x_des /*[B][30]*/, double* u_des /*[B][30]*/, int32_t* mode /*[B]*/);
int qmhip_mpc_download_feedback(qmhip_ctx* ctx, int B, double* gain /*[B][max_nodes][30][30]*/, double* uff /*[B][max_nodes][30]*/);
/* ---- published feedback policy: the policy buffer MPC_MRT_Interface swaps in behind a mutex (updatePolicy + evaluatePolicy on the control thread, QMController.cpp:133-148,
 *      while mpcThread_ computes the next solution, QMController.cpp:315-333).  A publication is a snapshot of the last solve — primal solution, grid, mode schedule and,
 *      with ST_FEEDBACK_POLICY = 1, the gain data (PR_*, qmhip_layout.h) of the first `nodes` nodes of every instance — into the inactive one of two slots, which then
 *      becomes the active one; it stays valid whatever the context solves next.
 *      policy_set_publish_window: 0 (the default) = off: nothing is allocated and every other entry point behaves as without this block; 2 ... max_nodes allocates the two
 *        slots (7.4 KB per instance and node of the window, plus two copies of the primal arrays) and drops earlier publications.  A tick looks at the two nodes bracketing
 *        its time: the window must reach as far as the policy is evaluated behind t0 (one or two MPC periods).
 *      policy_publish: snapshot of the last solve of a batch of B, in stream order behind it (also behind a qmhip_step_submit in flight) and in front of the next solve;
 *        the sequence number advances by one.  QMHIP_ERR_STATE without a window or before any solve; QMHIP_ERR_ARG with ST_FEEDBACK_POLICY = 1 on solver slots 1 / 3
 *        (the multiple-shooting slots only).  With ST_FEEDBACK_POLICY = 0 the publication carries the primal part only.
 *      policy_eval_published: qmhip_policy_eval_feedback on the ACTIVE publication: u_des = the linear controller at (t[b], x[b]); x == NULL: the feed-forward policy.
 *        covered[b] = 1 when both nodes bracketing t[b] lie inside the window (and the instance's grid); an instance that is not covered gets exactly the feed-forward
 *        answer of qmhip_policy_eval — check `covered`.  *seq = the sequence number of the publication that was evaluated.  Runs on a stream of its own and takes a small
 *        publication mutex, NOT the context lock: it may be called from a second thread while a solve, a streamed step or a loop runs on the context (evaluations are
 *        serialised among themselves).  Ordering is by events on the device: an evaluation waits for its slot's publication, a publication into a slot for the last
 *        evaluation enqueued on it.  QMHIP_ERR_STATE before the first publication, for a B other than the publication's, and for x != NULL on a publication without gains.
 *      policy_published_info: sequence number of the active publication (0: none), the window, and per instance of the active publication's batch the number of ticks of
 *        qmhip_closed_loop_sim_pipelined that were NOT covered since the last qmhip_sim_reset (any of the three may be NULL). */
int qmhip_policy_set_publish_window(qmhip_ctx* ctx, int nodes);
int qmhip_policy_publish(qmhip_ctx* ctx, int B);
int qmhip_policy_eval_published(qmhip_ctx* ctx, int B, const double* t /*[B]*/, const double* x /*[B][30] or NULL*/, double* x_des /*[B][30]*/, double* u_des /*[B][30]*/,
                                int32_t* mode /*[B]*/, int32_t* covered /*[B] or NULL*/, int64_t* seq /*out, or NULL*/);
int qmhip_policy_published_info(qmhip_ctx* ctx, int64_t* seq, int32_t* window, int32_t* uncovered /*[B] or NULL*/);

/* ---- WBC: replaces qm::WbcBase::update / HierarchicalWbc::update (qm_wbc/include/qm_wbc/WbcBase.h:31-32,
 *      qm_wbc/src/HierarchicalWbc.cpp:18-44; variant 1 = HierarchicalMpcWbc.cpp:18-34).
 *      out[b] = [vdot(24), F(12), tau(18)]; qp_status[b][3] per priority level: 0 ok, 1 iteration limit (qpOASES' nWSR = 100, HoQp.cpp:141), 2 working set larger
 *      than the level's null space (a degenerate vertex).  `variant` selects one of the two hierarchies the reference ships; both put inequality rows into their first
 *      level only, and the cascade kernel is specialised to that shape (slack eliminated analytically at level 0, hard rows below).  The GENERAL stacking of
 *      HoQp.cpp:92-124 — own inequality rows at a lower level, with the reference's current-first / previous-first pairing of stacked rows and slack solutions — is not
 *      reachable through this entry point; it is what qmhip_hoqp_solve below offers on explicit task matrices (a generic kernel); restated in the oracle (oracle/src/wbc.h: solveHoLevel) and pinned against
 *      the literal cascade (tests/test_hoqp_literal.py).
 *      The joint-acceleration state `inputLast_` (WbcBase.cpp:212-213) lives in the context per instance;
 *      qmhip_wbc_reset zeroes it.  The call enqueues on the context's WBC stream only and waits for that stream only (pinned staging, asynchronous copies). */
int qmhip_wbc_step(qmhip_ctx* ctx, int B, const double* x_des, const double* u_des, const double* rbd_meas /*[B][55]*/,
                   const int32_t* mode, double period, const double* time /*[B]*/, int variant,
                   double* out /*[B][54]*/, int32_t* qp_status /*[B][3]*/);
int qmhip_wbc_reset(qmhip_ctx* ctx);

/* ---- qm::HoQp on ARBITRARY task hierarchies: replaces the cascade HoQp(task_k, HoQp(task_k-1, ...)) + getSolutions() of qm_wbc/include/qm_wbc/HoQp.h:17-36 /
 *      qm_wbc/src/HoQp.cpp:12-158 for a WbcBase subclass that stacks its tasks differently from the two shipped hierarchies — the general stacking, own inequality
 *      rows below the first level included, with the reference's pairing of stacked rows (current level first, HoQp.cpp:46) and stacked slack solutions (previous
 *      levels first, HoQp.cpp:152-158).  B independent cascades of ONE shape: n decision variables (<= 36), n_levels (<= 8) tasks from the highest priority down with
 *      ma[k] equality rows A x = b (<= 36) and md[k] inequality rows D x <= f (<= 64; <= 128 over all levels); arrays instance-major, the levels concatenated:
 *      A [B][sum ma][n], b [B][sum ma], D [B][sum md][n], f [B][sum md].  x [B][n] = getSolutions() of the last level; status [B][n_levels]: 0 ok, 1 iteration limit
 *      (qpOASES' nWSR = 100), 2 working set larger than the problem (degenerate vertex), 3 the higher levels' rows do not hold at the previous solution (the
 *      row / slack pairing quirk with inequality rows on two higher levels and a non-zero slack: the reference would hand qpOASES that problem and ignore the return
 *      code).  A generic kernel (dense factorisations on a per-problem workspace, one wavefront per problem): not on the benchmark's path. */
int qmhip_hoqp_solve(qmhip_ctx* ctx, int B, int n_levels, int n, const int32_t* ma, const int32_t* md,
                     const double* A, const double* b, const double* D, const double* f, double* x /*[B][n]*/, int32_t* status /*[B][n_levels]*/);

/* ---- whole control step on resident data (benchmark "step"): SQP iteration + policy evaluation at t0 + WBC with
 *      the measured state built from x0 (zero velocities, EE pose by FK).  Everything is enqueued, nothing waited for: the kernels that decide
 *      the line search's step length also write the policy at t0 (what MPC_MRT_Interface::evaluatePolicy reads from the primal solution at its first node), the WBC starts
 *      behind them on its own stream, and the primal solution on all nodes (what qmhip_mpc_download / qmhip_policy_eval / the next warm start read) is written beside it.
 *      Same results as qmhip_mpc_solve_resident + qmhip_policy_eval(t0) + qmhip_wbc_step, bit for bit (tests/test_gpu_mpc.py) */
int qmhip_control_step_resident(qmhip_ctx* ctx, int B, double horizon, double period, double time);
int qmhip_wbc_download(qmhip_ctx* ctx, int B, double* out /*[B][54]*/, int32_t* qp_status /*[B][3]*/);

/* ---- streamed control-step I/O: what a controller does per MPC call with its own plant on the host — MPC_MRT_Interface::setCurrentObservation + MPC_BASE::run +
 *      evaluatePolicy + WbcBase::update (qm_controllers/src/QMController.cpp:133-148) — as a submit / collect pair that never stalls the device: the observation goes in
 *      through pinned staging and asynchronous copies, the results of one instance come back as ONE fixed record (struct qmhip_step_record, qmhip_layout.h: policy at t0,
 *      WBC output, perf, status words — 1024 bytes) packed on the device, and up to TWO steps may be in flight, so the record of step k travels while step k + 1 computes.
 *      submit enqueues and returns; collect waits for the OLDEST step in flight only (one event of the copy stream; neither the MPC nor the WBC stream is synchronised).
 *      submit = new observation (t0, x0) + one warm-started control step exactly as a step of qmhip_closed_loop_resident runs it (cold when no solution of this batch
 *      exists: after qmhip_mpc_upload, qmhip_sim_reset, a solver switch): references and schedule are the resident ones — qmhip_mpc_upload / qmhip_mpc_update_references
 *      or, when the gait front-end has been reset for this batch, its schedule refreshed before the solve.  Results are the bits of
 *      qmhip_mpc_set_initial + qmhip_closed_loop_resident(n_steps 1) + qmhip_mpc_download + qmhip_wbc_download (tests/test_gpu_step_io.py).
 *      flags: QMHIP_STEP_WBC runs the WBC and fills wbc_out / qp_status (zeros otherwise: K0, the SQP iterations and the policy at t0 only, the WBC's inputLast_
 *      untouched); rbd_meas [B][55] is then the measured state and `time` its time (NULL: built from x0 as qmhip_control_step_resident does).  QMHIP_STEP_TRAJ also
 *      returns the primal solution, compacted to the batch's largest node count on the device and copied with the records.
 *      collect: rec [B]; trajectory outputs shaped like those of qmhip_mpc_download ([B][max_nodes][k]), any may be NULL: nodes 0 .. n_nodes[b] - 1 of instance b are written, the
 *      caller's memory behind them is left untouched (qmhip_mpc_download writes all max_nodes).
 *      Errors: a third submit while two steps are in flight, collect with nothing in flight, trajectory outputs for a step submitted without QMHIP_STEP_TRAJ, a WBC-only
 *      context: QMHIP_ERR_STATE.  B other than the batch of the last qmhip_mpc_upload (or of the step being collected), B > max_batch, NULL t0 / x0 / rec, horizon or
 *      period <= 0: QMHIP_ERR_ARG.  Any other entry point called while steps are in flight orders itself behind them as it does behind any enqueued step (its own
 *      stream synchronisation or stream order); their records stay collectable. */
#define QMHIP_STEP_WBC  1   /* run the WBC, fill wbc_out / qp_status */
#define QMHIP_STEP_TRAJ 2   /* also return the primal solution */
int qmhip_step_submit(qmhip_ctx* ctx, int B, const double* t0 /*[B]*/, const double* x0 /*[B][30]*/, const double* rbd_meas /*[B][55] or NULL*/,
                      double horizon, double period, double time, unsigned flags);
int qmhip_step_collect(qmhip_ctx* ctx, int B, qmhip_step_record* rec /*[B]*/,
                       double* out_t /*[B][max_nodes]*/, int32_t* out_event, int32_t* out_mode, double* out_x /*[B][max_nodes][30]*/, double* out_u);
int qmhip_step_in_flight(const qmhip_ctx* ctx);   /* 0, 1 or 2 */

/* ---- streamed controller tick for a plant on the host: QMController::update (qm_controllers/src/QMController.cpp:128-175) as a service — the measured state of B robots
 *      in, their hybrid joint commands out, once per tick, the MPC on every mpc_every-th tick, the controller's state resident between ticks.  For a caller that owns the
 *      plant (a batched simulator, hardware, the reference's QMHWSim) and has what the reference's estimator returns: measuredRbdState_ (55 doubles, the layout of
 *      qmhip_wbc_step) and the contact flags.  Nothing is estimated here.
 *      tick_reset = QMController::starting for a batch: zeroed observation (previous yaw 0), nothing commanded yet, stop flags cleared, tick counter 0; the episode starts cold
 *        like qmhip_sim_reset (previous solution dropped) and the WBC's inputLast_ is zeroed (qmhip_wbc_reset).  controller: 0 qm::QMController, 1 qm::QMMpcController (as
 *        qmhip_sim_set_controller); arm_kp / arm_kd: the arm gains of updateControlLaw.  References and schedule are the resident ones (qmhip_mpc_upload /
 *        qmhip_mpc_update_references / the device gait front-end), exactly as for qmhip_step_submit.
 *      tick_submit = one update, enqueued, nothing waited for:
 *        1. observation: computeCentroidalStateFromRbdModel(rbd_meas) at time[b] (QMController.cpp:202-244), the yaw unwrapped against the instance's previous observation:
 *           yaw + 2 pi k, k = nearbyint((yawLast - yaw) / 2 pi) — the reference's yawLast + shortest_angular_distance(yawLast, yaw) up to rounding; a yaw that does not
 *           wrap passes unchanged, bit for bit.  Measured mode 8 LF + 4 RF + 2 LH + RH of contact[b] (-1 when contact is NULL).
 *        2. on tick 0, mpc_every, 2 mpc_every ... since tick_reset: the MPC call of qmhip_closed_loop_sim on that observation (gait front-end refresh when it is active for
 *           this batch, warm-started, sqp.sqpIteration iterations; cold when no solution of this batch exists).
 *        3. the policy at the observation time: feed-forward, or with ST_FEEDBACK_POLICY = 1 the SQP's linear controller at the observed state (solver slots 1 / 3 with the
 *           slot set: QMHIP_ERR_ARG).
 *        4. the WBC on rbd_meas (hierarchy of `controller`); on tick 0 inputLast_ is primed with the planned input, as qmhip_closed_loop_sim does.
 *        5. SafetyChecker::checkOrientation (SafetyChecker.h:25-32): roll state[11] outside +-pi/2 (strictly) sets safety = 1 in this tick's record — the tick still issues its
 *           command, as the reference does (QMController.cpp:159-165) — and a STICKY stop flag for the instance: from the next tick on its record repeats the held command
 *           with stopped = 1 and its controller state (held command, arm hold / publication times, previous yaw) is frozen; x_obs, x_des, u_des and wbc_out of a stopped
 *           instance are still computed and reported, not used.  The rest of the batch is unaffected; tick_reset clears the flag.
 *        6. updateControlLaw (QMController.cpp:177-190 / 431-445) into the instance's HELD command: under controller 0 the legs keep their held values (zeros after a reset)
 *           until time > 10; under controller 1 the arm's held position starts at the measured arm pose of tick 0 and is re-published when more than 1/100 s have passed.
 *        7. one struct qmhip_tick_record per instance — 2048 bytes, qmhip_layout.h —, packed on the device, one copy to pinned host memory, one event.
 *      tick_collect waits for that event only and copies the records out.  Driven with the plant's own state and time, the pair reproduces qmhip_closed_loop_sim bit for bit
 *      (tests/test_gpu_tick.py).  Trajectories are not part of the record: qmhip_mpc_download reads them.
 *      observe: step 1 alone for host states, stateless (no unwrapping) — the centroidal state qmhip_mpc_set_initial / qmhip_step_submit want.
 *      Depth is ONE.  QMHIP_ERR_STATE: a second tick_submit before the collect; tick_submit while a qmhip_step_submit is in flight and the other way round; tick_collect with
 *      nothing in flight; a tick before tick_reset; a tick without an MPC call after the solution was dropped (upload, reset, solver switch); a WBC-only context.
 *      QMHIP_ERR_ARG: B other than tick_reset's (or > max_batch), NULL time / rbd_meas / rec, mpc_every < 1, controller other than 0 / 1, horizon or period <= 0.
 *      qmhip_policy_eval_feedback / qmhip_mpc_download_feedback return QMHIP_ERR_STATE while a tick is in flight. */
int qmhip_tick_reset(qmhip_ctx* ctx, int B, int controller, double arm_kp, double arm_kd, int mpc_every);
int qmhip_tick_submit(qmhip_ctx* ctx, int B, const double* time /*[B]*/, const double* rbd_meas /*[B][55]*/, const int32_t* contact /*[B][4] LF RF LH RH, or NULL*/,
                      double horizon, double period);
int qmhip_tick_collect(qmhip_ctx* ctx, int B, qmhip_tick_record* rec /*[B]*/);
int qmhip_observe(qmhip_ctx* ctx, int B, const double* rbd /*[B][55]*/, double* x /*[B][30]*/);

/* ---- planned task-space trajectories: the arithmetic of qm::QmVisualizer (qm_interface/src/visualization/qm_visualization.cpp:72-317) without its ROS messages —
 *      where the feet, the base and the arm's end effector are along a plan, which forces act where, where the feet will land.  One 512-byte qmhip_plan_record
 *      (include/qmhip_layout.h) per node: node time, mode and stance mask, base pose, the four foot positions / velocities / contact forces (contact order LF RF LH RH,
 *      world frame), the end-effector pose and its error against the node's reference, the centre of pressure of the stance feet (cop[2] = their summed f_z; cop[0:2] = 0
 *      when that sum is not positive) ([upstream getCenterOfPressureMarker, recalled]).
 *      plan_task_space (publishOptimizedStateTrajectory, qm_visualization.cpp:90-189): the records of the primal solution of the LAST solve, [B][max_nodes]; records at
 *        or behind num_nodes[b] are zero.  Works behind any solver slot.
 *      plan_footholds (the "Future footholds" of qm_visualization.cpp:150-182): for every schedule event strictly inside the instance's grid (t_first < t_e < t_last) the
 *        plan interpolated linearly at t_e and one qmhip_foothold per foot that is off before and on behind the event, ordered by (event, foot).  count[b] is the full
 *        number of landings; only the first `cap` are written.
 *      task_space_eval (publishDesiredTrajectory, qm_visualization.cpp:194-251: the target knots; publishObservation, qm_visualization.cpp:267-283: the observation): the
 *        same record for R <= max_batch * max_nodes caller-supplied (state, input, mode) rows; u NULL = zero inputs, ee_ref NULL = no reference (ee_err = 0); time = 0.
 *      All three run on the MPC stream behind whatever it holds and wait for that stream only; buffers are allocated by the first call, not by qmhip_create.
 *      QMHIP_ERR_STATE: no solution (no solve since creation, the last upload, reset or solver switch), B other than the last solve's, a WBC-only context; nothing is
 *      written then.  QMHIP_ERR_ARG: B or R out of range, NULL rec / x / mode / count, cap < 0, NULL out with cap > 0. */
int qmhip_plan_task_space(qmhip_ctx* ctx, int B, qmhip_plan_record* rec /*[B][max_nodes]*/, int32_t* num_nodes /*[B] or NULL*/);
int qmhip_plan_footholds(qmhip_ctx* ctx, int B, int cap, qmhip_foothold* out /*[B][cap]*/, int32_t* count /*[B]*/);
int qmhip_task_space_eval(qmhip_ctx* ctx, int R, const double* x /*[R][30]*/, const double* u /*[R][30] or NULL*/, const int32_t* mode /*[R]*/,
                          const double* ee_ref /*[R][7] pos + quat xyzw, or NULL*/, qmhip_plan_record* rec /*[R]*/);

/* ---- policy rollout: MPC_MRT_Interface::rolloutPolicy(currentTime, currentState, timeStep, mpcState, mpcInput, mode) [upstream, recalled] — the rollout the reference
 *      initialises at qm_controllers/src/QMController.cpp:311 (a TimeTriggeredRollout over QMDynamicsAD, qm_interface/src/QMInterface.cpp:73,136-137) — batched: the
 *      model integrated forward from a state that is NOT the plan's, under the active policy, with a summary.  R rows, each an instance of the last solve (or of the active
 *      publication) with a start (t0, x0) and an absolute final time t_end >= t0; one wavefront per row, many rows per instance.
 *      Evaluation points k = 0 .. K: t_0 = t0, t_{k+1} = min(t_k + max_step, e, t_end) with e the first event of the instance's schedule strictly behind t_k, accumulated
 *        exactly like this (a rollout continued from a returned t_k repeats the same doubles); it ends at t_end or after max_steps steps (QM_ROLLOUT_MAX_STEPS).  The query
 *        time is t_k, or t_k + weakEpsilon when t_k equals an event time bit for bit: a step that starts on an event sees the mode and the PostEvent node behind it.
 *      At every point, the last included: x_des, u_ff = the feed-forward policy, mode_k = the schedule's mode, u_k = u_ff (feedback 0) or what qmhip_policy_eval_feedback
 *        (source 0) / qmhip_policy_eval_published (source 1, with its feed-forward fall-back outside the window) return at (time, x_k).  Times outside the plan's grid
 *        clamp as there (QM_ROLLOUT_OUTSIDE).  Then x_{k+1} = x_k + h/2 (f(x_k, u_k) + f(x_k + h f(x_k, u_k), u_k)): u_k HELD over the step, the transcription's Heun rule —
 *        the discrete model the Riccati gains belong to, hence max_step = sqp.dt by default — NOT upstream's adaptive ODE45.  A non-finite x_{k+1} ends the rollout at
 *        point k (QM_ROLLOUT_NONFINITE).
 *      Out: x_end = x_K, u_end = u_K, mode_end = mode_K (what rolloutPolicy returns); per row a struct qmhip_rollout_summary of include/qmhip_layout.h, folded over the K + 1
 *        points — largest deviation from the plan per state block, largest feedback term, smallest friction-cone margin and normal force over stance feet (+ infinity
 *        without one), largest force on a swing foot, steps, steps that ended on an event, uncovered points, flags; optionally a trace of qmhip_rollout_sample, one per
 *        point k < trace_cap, row-major [R][trace_cap]: count[r] = K + 1 keeps counting behind the cap (the rule of qmhip_plan_footholds), slots at or behind it are left alone.
 *      source 0 reads the last solve's stage records under the context lock on the MPC stream: valid as qmhip_policy_eval_feedback is.  source 1 reads the ACTIVE
 *        publication on the published policy's stream under the publication mutex, never the context lock — beside a running solve, from another thread — and returns its
 *        sequence number in *seq.  Row buffers grow on demand and are kept, per source.
 *      QMHIP_ERR_STATE: no solve yet (or after an upload / reset / solver switch), a streamed step or tick in flight (source 0); no publication, feedback = 1 on a publication
 *        without gains (source 1); a WBC-only context.  QMHIP_ERR_ARG: R < 1; an inst entry outside the batch of the solve / publication (inst NULL: R beyond it); a NULL
 *        among t0, x0, t_end, p, x_end, u_end, mode_end; max_step not a positive finite number; max_steps < 1; source / feedback other than 0 / 1; trace_cap < 0, or > 0
 *        with trace NULL; a t0 / t_end that is not finite, or t_end < t0; feedback = 1 with ST_SOLVER 1 or 3.  An error writes to none of the caller's arrays. */
typedef struct qmhip_rollout_params { double max_step; int32_t max_steps, source, feedback, trace_cap; } qmhip_rollout_params;
int qmhip_policy_rollout(qmhip_ctx* ctx, int R, const int32_t* inst /*[R] or NULL: row r = instance r*/, const double* t0 /*[R]*/, const double* x0 /*[R][30]*/,
                         const double* t_end /*[R]*/, const qmhip_rollout_params* p, double* x_end /*[R][30]*/, double* u_end /*[R][30]*/, int32_t* mode_end /*[R]*/,
                         struct qmhip_rollout_summary* summary /*[R] or NULL*/, qmhip_rollout_sample* trace /*[R][trace_cap] or NULL*/, int32_t* count /*[R] or NULL*/,
                         int64_t* seq /*out or NULL; source 1*/);

/* ---- batched rigid-body plant: stands where Gazebo + qm_gazebo::QMHWSim stand in the reference.
 *      sim_set_command = HybridJointHandle::setCommand as QMController::updateControlLaw issues it (qm_controllers/src/QMController.cpp:177-190):
 *        per joint posDes, velDes, kp, kd, ff in the reference's joint order (LF, LH, RF, RH, arm).
 *      sim_step = one simulation step: QMHWSim::writeSim (qm_gazebo/src/QMHWSim.cpp:98-116: the held command enters the delay buffer, commands older than
 *        `delay` — qm_gazebo/config/default.yaml:2 — are dropped, the oldest survivor is applied: tau = kp (posDes − q) + kd (velDes − qd) + ff, saturated at
 *        the URDF effort limit), then n_substeps semi-implicit Euler steps of the floating-base forward dynamics with penalty ground contact of the four
 *        feet, then QMHWSim::readSim (QMHWSim.cpp:60-75): rbd[b] is the state in the estimator's layout (qm_estimation/src/StateEstimateBase.cpp:41-103),
 *        contact[b] the four contact flags (LF RF LH RH).  rbd / contact may be null (results stay resident).
 *      sim_reset: generalized coordinates q = [pos(3), zyx(3), joints(18)], v = [world linear velocity, zyx rates, joint rates], time per instance;
 *        clears the delay buffer ("Simulation reset", QMHWSim.cpp:101-103).  A new episode starts cold: the MPC's previous primal solution is dropped, so until the next
 *        solve qmhip_policy_eval / qmhip_mpc_download / qmhip_mpc_advance_resident return QMHIP_ERR_STATE and the next warm solve is a cold one.
 *      sim_set_params: {contact stiffness [N/m], contact damping [N s/m], friction coefficient, friction regularisation speed [m/s], foot radius [m],
 *        command delay [s], saturate efforts (0/1)}; Gazebo's ODE contact solver is not part of the reference's sources, the contact model is this library's own.
 *      sim_get_state: q, v, time, contact forces [B][12] (world frame) of the last sub-step, status [B] (0 ok, 1 mass matrix not positive definite); any may be null. */
int qmhip_sim_set_params(qmhip_ctx* ctx, const double* params, int n);
/*      sim_set_controller: which controller plugin the closed loops below run — 0 qm::QMController (HierarchicalWbc; updateControlLaw QMController.cpp:177-190),
 *        1 qm::QMMpcController (HierarchicalMpcWbc, QMController.cpp:410-414; updateControlLaw QMController.cpp:431-445: legs commanded on every tick, the arm as
 *        position commands q_meas + velDes / 100 re-published when more than 1/100 s have passed — arm_kp / arm_kd of the loop calls are then the gains of the arm's
 *        position controllers and no arm torque is fed forward).  The control law switches with the next tick; the arm's held position command / publication
 *        times (QMController::starting, QMController.cpp:127) are only re-initialised by qmhip_sim_reset, so switch before a reset. */
int qmhip_sim_set_controller(qmhip_ctx* ctx, int controller);
int qmhip_sim_reset(qmhip_ctx* ctx, int B, const double* q /*[B][24]*/, const double* v /*[B][24]*/, const double* time /*[B]*/);
int qmhip_sim_set_command(qmhip_ctx* ctx, int B, const double* pos_des /*[B][18]*/, const double* vel_des, const double* kp, const double* kd, const double* ff);
int qmhip_sim_step(qmhip_ctx* ctx, int B, double period, int n_substeps, double* rbd /*[B][55]*/, int32_t* contact /*[B][4]*/);
int qmhip_sim_get_state(qmhip_ctx* ctx, int B, double* q, double* v, double* time, double* force /*[B][12]*/, int32_t* status /*[B]*/);
/*      sim_get_rbd: rbd / contact of the plant's CURRENT state (what the last sim_step or sim_reset left) without stepping; either may be null */
int qmhip_sim_get_rbd(qmhip_ctx* ctx, int B, double* rbd /*[B][55]*/, int32_t* contact /*[B][4]*/);
/* ---- plant disturbances: scheduled external wrenches on the base and on the arm's end effector (a shove, a payload hanging from the gripper).  The reference has no
 *      counterpart (Gazebo applies such wrenches through its own services); the semantics are this library's own.
 *      sim_set_pushes: p is [B][K] records of struct qmhip_push, 96 bytes: qmhip_layout.h, with 0 <= K <= QM_SIM_MAX_PUSH; all vectors in the WORLD frame, times in ABSOLUTE plant time.  K == 0 or
 *        p == NULL switches pushes off; sim_step and both closed loops then launch exactly the plant kernel they launch without the feature.  With a schedule they launch
 *        its second instance, qm_sim_push_kernel (one wavefront per instance, the same LDS).  The schedule persists across qmhip_sim_reset and may be set before the first
 *        one.  Instances at or beyond B of a later, larger step have no schedule.
 *      ACTIVITY — slot k of instance b is active in a sub-step iff t_on <= t_s < t_off, t_s being the plant time at the START of that sub-step (the double the kernel
 *        accumulates by repeated time += period / n_substeps).  t_on == t_off is never active; t_off = +inf is a permanent load; t_on = -inf is allowed.
 *      APPLIED WRENCH — the sum over the active slots in ascending slot order, starting from +0.0; inactive slots are skipped, not multiplied by zero.
 *      GENERALIZED FORCE — added to the right-hand side of M vdot = Sᵀ tau − nle + Σ J_iᵀ f_i before the solve, the velocity being [pdot_world, zyx rates, joint rates]:
 *        base_force F acts at the base frame origin (q[0:3] = rbd[3:6]): rhs[0:3] += F;  base_torque n is a pure couple on the base body: rhs[3:6] += Eᵀ n with
 *        omega_world = E(zyx) rates;  ee_force f acts at the arm's tip frame (frame 4, position rbd[48:51]): rhs += J_eeᵀ f with the linear 3 x 24 tip Jacobian, base
 *        columns (identity, e_k x (p_tip − p_base)) included.
 *      The hand-over launch of sim_reset (no sub-step) applies nothing.
 *      Returns QMHIP_ERR_ARG with nothing changed for B outside [1, max_batch], K outside [0, QM_SIM_MAX_PUSH], a NaN time, a non-finite force / torque component.
 *      sim_get_push: what the LAST sub-step of the last step applied — wrench[b] = {base_force, base_torque, ee_force} summed as above, mask[b] bit k set iff slot k was
 *        active; either may be null.  Zeros after sim_reset and while pushes are off. */
int qmhip_sim_set_pushes(qmhip_ctx* ctx, int B, int K, const qmhip_push* p /*[B][K]*/);
int qmhip_sim_get_push(qmhip_ctx* ctx, int B, double* wrench /*[B][9]*/, int32_t* mask /*[B]*/);
/* ---- plant terrain: a per-instance grid of ground heights and friction coefficients under the four feet, in place of the plane z = 0 with one global friction
 *      coefficient.  The reference has no counterpart (its worlds are Gazebo's); the semantics are this library's own.  The MPC and the WBC keep their flat-floor
 *      assumption: the terrain is what the blind controller is tested on.
 *      sim_set_terrain: hdr is [B] records of struct qmhip_terrain, 32 bytes: qmhip_layout.h — vertex (i, j) of instance b lies at (x0 + i dx, y0 + j dy) in the world
 *        frame —, height and mu are [B][ny][nx] with 2 <= nx, ny <= QM_TERRAIN_MAX, the same nx, ny for all instances of one call.  mu == NULL: the friction coefficient
 *        of sim_set_params everywhere.  hdr == NULL switches the terrain off; sim_step and both closed loops then launch exactly the plant kernel they launch without the
 *        feature.  With a terrain they launch qm_sim_terrain_kernel, or qm_sim_terrain_push_kernel while a schedule of pushes is set (one wavefront per instance, the
 *        same LDS); the sensor kernel runs behind them as behind the other two.  The terrain persists across qmhip_sim_reset and may be set before the first one.  An
 *        instance at or beyond B of a later, larger step stands on the plane z = 0 with the global friction coefficient.
 *      LOOKUP at a point (x, y) — s = (x − x0) / dx; cx = (s < 0 or s > nx − 1); s = min(max(s, 0), nx − 1); i = min((int)floor(s), nx − 2); u = s − i, and t, cy, j, w
 *        likewise in y.  With h00 = height[j][i], h10 = height[j][i + 1], h01 = height[j + 1][i], h11 = height[j + 1][i + 1]:
 *          h  = (1 − w) ((1 − u) h00 + u h10) + w ((1 − u) h01 + u h11)            (mu: the same expression on the mu array)
 *          gx = cx ? 0 : ((1 − w) (h10 − h00) + w (h11 − h01)) / dx
 *          gy = cy ? 0 : ((1 − u) (h01 − h00) + u (h11 − h10)) / dy
 *        Outside the grid the ground continues at the edge's height with zero slope along the clamped coordinate; at s == nx − 1 exactly the last cell's gradient holds.
 *        The field is a continuous height map: no vertical faces, no overhangs.
 *      CONTACT of foot f with centre p, velocity v and radius r = foot_radius against the tangent plane under its centre (h, gx, gy, mu looked up at (p_x, p_y)):
 *          n   = (−gx, −gy, 1) / sqrt(1 + gx² + gy²)
 *          pen = r − (p_z − h) n_z
 *          vn  = v·n
 *          fn  = pen > 0 ? max(0, k_n pen − d_n vn) : 0
 *          vt  = v − vn n
 *          f   = fn n − mu fn vt / sqrt(|vt|² + v_eps²)      (world frame; enters the dynamics through J_fᵀ f like the flat model's force)
 *        The contact flag is pen > 0 at the handed-over state, the hand-over launch of sim_reset included.  With h = 0, gx = gy = 0 and mu the global coefficient this is
 *        the flat model term for term.  Only the four feet touch the ground.
 *      sim_get_ground: per foot (LF RF LH RH) {h, n_x, n_y, n_z, mu, pen} of the LAST sub-step of the last step, at the state that sub-step started from (like the contact
 *        forces of sim_get_state).  Zeros after sim_reset and while the terrain is off.
 *      terrain_eval: the plant's own lookup at n points per instance, xy[b][k] = (x, y), out[b][k] = {h, gx, gy, mu}; QMHIP_ERR_STATE without a terrain.
 *      The episode monitor keeps the truth and is unchanged: its fall threshold min_base_z is an ABSOLUTE height, not a clearance above the ground, and its friction and
 *        normal-force figures (max_friction_ratio, max_normal_force) use the world z axis — on sloped ground they are not cone margins.
 *      sim_set_terrain returns QMHIP_ERR_ARG with nothing changed for B outside [1, max_batch], nx or ny outside [2, QM_TERRAIN_MAX], a non-finite header entry, dx or
 *        dy <= 0, a non-finite height, a mu that is negative or non-finite; QMHIP_ERR_STATE on a WBC-only context. */
int qmhip_sim_set_terrain(qmhip_ctx* ctx, int B, int nx, int ny, const qmhip_terrain* hdr /*[B], NULL: off*/, const double* height /*[B][ny][nx]*/, const double* mu /*same shape or NULL*/);
int qmhip_sim_get_ground(qmhip_ctx* ctx, int B, double* ground /*[B][4][6]*/);
int qmhip_terrain_eval(qmhip_ctx* ctx, int B, int n, const double* xy /*[B][n][2]*/, double* out /*[B][n][4]: h, gx, gy, mu*/);
/* ---- sensor model: white noise, a constant bias and a latency of whole samples, per instance, on what the CONTROLLER is told about the plant.  The reference's simulation
 *      has only the "ground truth" estimator (FromTopiceEstimate); the semantics are this library's own.  The plant, qmhip_sim_step / qmhip_sim_get_rbd / _get_state and the
 *      episode monitor (fall check included) keep the truth; the MPC observation, the tick's state estimate, the WBC and updateControlLaw of both closed loops read the
 *      measured state.  Contact flags are not modelled (the loops use the planned mode), `time` stays the plant's time; no quantisation, no coloured noise.
 *      sim_set_sensors: s is [B] records of struct qmhip_sensor, 128 bytes: qmhip_layout.h; s == NULL switches the model off — every entry point then launches exactly what it
 *        launches without the feature.  With records, every plant launch is followed by one qm_sense_kernel (one wavefront per instance).  May be called before the first
 *        sim_reset; the records persist across sim_reset.  Instances at or beyond B of a larger step have no record: their measured state is a copy of the truth.
 *      GROUPS g of the 55-entry rbd state (qm_estimation/src/StateEstimateBase.cpp:41-103): 0 rbd[0:3] base zyx angles, 1 rbd[3:6] base position, 2 rbd[6:24] joint positions,
 *        3 rbd[24:27] base angular velocity, 4 rbd[27:30] base linear velocity, 5 rbd[30:48] joint rates.  Component index c = 0..47 is the rbd index.
 *      SAMPLES — the hand-over launch of sim_reset takes sample n = 0; every plant step (sim_step, a tick of either loop) takes sample n + 1.  A per-instance ring keeps the
 *        true rbd state of the last QM_SENSE_MAX_LAG + 1 samples, sample n in slot n % (QM_SENSE_MAX_LAG + 1).  The SOURCE of sample n is the truth x of sample
 *        n − min(lag, n): before `lag` samples exist, the oldest one (the reset state).
 *      NOISE — integer arithmetic mod 2^64: mix(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31.
 *        word(seed, n, c, w) = mix(mix(seed + G (n + 1)) + G (2c + w + 1)) with G = 0x9E3779B97F4A7C15 and n as a 64-bit unsigned value.  s = the sum of the eight 16-bit
 *        fields of word(seed, n, c, 0) and word(seed, n, c, 1).  nu(seed, n, c) = (double)(2s − 8·65535) · C with C = 0x1.3988e1412ed76p-17, the double nearest
 *        1 / sqrt(8 (65536² − 1) / 3): an eight-term Irwin-Hall variable of unit variance, |nu| <= 8·65535·C ≈ 4.8989.  The bias draw of component c is
 *        nu_bias = nu(seed, 2^64 − 1, c) (the inner term of word is then seed + 0): a function of the seed alone, constant over the episode, stored nowhere.
 *      MEASURED VALUE of component c in group g:  m = (x + bias_sigma[g] nu_bias) + sigma[g] nu(seed, n, c) — two products, the inner sum, the outer sum, each rounded on
 *        its own (no fused multiply-add).  A group with sigma[g] == 0 and bias_sigma[g] == 0 is COPIED, not added to.
 *      END-EFFECTOR POSE rbd[48:55] — an instance without a noisy group: all 55 entries are the source sample's, delayed truth bit for bit (lag 0: the truth itself, the
 *        instance behaves as with the model off).  Otherwise: forward kinematics of the MEASURED configuration (StateEstimateBase::updateArmEE, StateEstimateBase.cpp:80-103).
 *      Calling sim_set_sensors starts the sample count over: if the plant has been reset, sample 0 is taken from its current state at once (one qm_sense_kernel launch, no
 *        plant launch).  Returns QMHIP_ERR_ARG with nothing changed for B outside [1, max_batch], a lag outside [0, QM_SENSE_MAX_LAG], a negative or non-finite sigma /
 *        bias_sigma; QMHIP_ERR_STATE on a WBC-only context.
 *      sim_get_measured: what the loops consume — with the model off the truth and samples[b] = 0, with it on the measured state and the index n of the last sample; either may
 *        be null.  Errors as qmhip_sim_get_rbd. */
int qmhip_sim_set_sensors(qmhip_ctx* ctx, int B, const qmhip_sensor* s /*[B], NULL: off*/);
int qmhip_sim_get_measured(qmhip_ctx* ctx, int B, double* rbd /*[B][55]*/, int32_t* samples /*[B]*/);
/*      closed_loop_sim: n_ticks of the whole controller around the plant, device resident — QMController::update + mpcThread_
 *        (qm_controllers/src/QMController.cpp:128-175, 202-244, 315-332): state estimate = the plant's state ("ground truth" estimator,
 *        currentObservation_.state = computeCentroidalStateFromRbdModel), an MPC call on that observation every mpc_every ticks (warm-started SQP; the
 *        gait front-end refreshes the mode schedule first when it is active), policy evaluation at the plant time, WBC on the measured state,
 *        updateControlLaw (QMController.cpp:177-190: legs kp 0 / kd 3 once time > 10, arm arm_kp / arm_kd, WBC torque as feed-forward), one
 *        simulation step.  Needs qmhip_mpc_upload (reference, schedule) and qmhip_sim_reset before; the tick counter restarts at sim_reset.
 *        The reference runs the MPC in its own thread; here it is synchronous with the tick that triggers it.  On the first tick after a reset the
 *        WBC's joint-acceleration state inputLast_ (WbcBase.cpp:212-213) is primed with the planned input (zero joint acceleration).
 *        ST_FEEDBACK_POLICY = 1 (sqp.useFeedbackPolicy): every tick evaluates the SQP's linear controller at its estimated centroidal state (the observation it builds for the
 *        MPC) instead of the feed-forward policy, in both controller modes; 0 launches exactly the feed-forward loop.  Solver slots 1 / 3 with the slot set: QMHIP_ERR_ARG. */
int qmhip_closed_loop_sim(qmhip_ctx* ctx, int B, int n_ticks, double period, int n_substeps, int mpc_every, double horizon, double arm_kp, double arm_kd);
/*      closed_loop_sim_pipelined: the same loop with the MPC BESIDE the control ticks, like mpcThread_ beside QMController::update (QMController.cpp:315-332): the
 *        MPC call triggered at a tick observes the plant at that tick and computes on its own stream while the next mpc_every ticks run on the policy published
 *        before; its solution is published (MPC_MRT_Interface's policy buffer) when those ticks are done — a latency of one MPC period, deterministic instead of
 *        thread-timing dependent.  The first call after a reset is synchronous.  n_ticks and the tick counter must be multiples of mpc_every.
 *        Without a publish window the published policy is a copy of the primal solution and carries no gains: with ST_FEEDBACK_POLICY = 1 this loop then returns
 *        QMHIP_ERR_ARG.  With a window (qmhip_policy_set_publish_window) and ST_FEEDBACK_POLICY = 1 the publication also carries the window's gains and every tick evaluates
 *        the published linear controller at its estimated state (solver slots 0 / 2); a tick whose time runs past the window falls back to the feed-forward input for that
 *        instance and is counted (qmhip_policy_published_info).  With ST_FEEDBACK_POLICY = 0 a window changes nothing in this loop. */
int qmhip_closed_loop_sim_pipelined(qmhip_ctx* ctx, int B, int n_ticks, double period, int n_substeps, int mpc_every, double horizon, double arm_kp, double arm_kd);

/* ---- episode monitor: what happened DURING a run of the two device loops above — per-instance running statistics folded on the device behind every tick, and an optional
 *      decimated trace of raw samples; both are read back with one copy each.  Records: struct qmhip_episode_summary, 256 bytes, and struct qmhip_episode_sample, 512 bytes:
 *      qmhip_layout.h.  Off by default: both loops then launch what they launch without it.  On, the monitor's kernels (csrc/kernels/k_episode.h) only READ the loop's
 *      buffers, so every output of the loop keeps its bits.
 *      episode_monitor: switches it on with fall thresholds (min_base_z on rbd[5], max_tilt on |roll| = |rbd[2]| and |pitch| = |rbd[1]|; strict comparisons) and a trace of
 *        up to trace_cap samples, one every trace_every ticks (both 0: no trace); NULL switches it off and frees its buffers.  Calling it again starts over.
 *      An episode starts with qmhip_sim_reset (monitor on): records cleared, the anchor is the end-effector pose rbd[48:55] of the reset state unless episode_set_anchor is
 *        called afterwards, the contact flags "before the first tick" are the reset state's.  Every tick of qmhip_closed_loop_sim / _pipelined of the reset's B is then folded:
 *        FALL RULE — the fall check comes first; from the tick that trips it on only `ticks` and `t_last` advance, the tripping tick itself is not folded into maxima, sums
 *        and counters (a non-finite state never reaches an accumulator; fall_cause 8).  t_first is the time behind the first folded tick, fallen or not.  An MPC call counts
 *        iff the instance had not fallen BEFORE the tick the call observed at, in both loops.  contact_mismatch compares the measured flag behind the tick with the stance bit
 *        of the mode the tick's policy returned.  max_ee_ang_dev is the rotation angle 4 asin(d / 2), d = min(|q - q_a|, |q + q_a|).
 *      Samples are raw copies, taken on every tick whose index since the episode's start is a multiple of trace_every, fallen or not, into slot tick / trace_every while that
 *        is below trace_cap; `mpc_status` is the status word of the last MPC call folded before the tick's fold (the pipelined loop folds a call behind its publication: the
 *        ticks of an MPC period carry the status of the call published in front of them).  episode_trace hands out min(count, cap, trace_cap) samples, sample-major
 *        [n][B] as on the device, and leaves the rest of `out` alone; *count keeps counting behind trace_cap, like qmhip_plan_footholds.
 *      episode_fold: one tick of a plant the CALLER owns (the companion of qmhip_tick_submit) through the same kernels: the state behind the tick, what the tick's policy /
 *        WBC returned, optionally the plant's status and — on a tick with an MPC call — the call's status word (it observed at this tick).  The first fold after
 *        episode_monitor starts the episode: the anchor must have been set, and the first tick's own contact flags stand for the flags before it.
 *      Reads run on the stream the synchronous loop's ticks run on and wait for that stream only (the pipelined loop has joined its streams when it returns).
 *      QMHIP_ERR_STATE: monitor off, a WBC-only context, summary / trace of a B other than the episode's (or before any episode), the first fold without an anchor.
 *      QMHIP_ERR_ARG: a NULL argument (fold: only sim_status / mpc_status may be NULL), B out of range or other than the running episode's, tick < 0, cap < 0, thresholds
 *        that are not finite, trace_every < 0, trace_cap < 0, or one of the pair zero and the other not.  Profiling name: "episode". */
typedef struct qmhip_episode_params { double min_base_z, max_tilt; int32_t trace_every, trace_cap; } qmhip_episode_params;
int qmhip_episode_monitor(qmhip_ctx* ctx, const qmhip_episode_params* p /* NULL: off */);
int qmhip_episode_set_anchor(qmhip_ctx* ctx, int B, const double* ee_pose /*[B][7] position + quaternion xyzw*/);
int qmhip_episode_summary(qmhip_ctx* ctx, int B, struct qmhip_episode_summary* out /*[B]*/);
int qmhip_episode_trace(qmhip_ctx* ctx, int B, int cap, qmhip_episode_sample* out /*[min(count, cap, trace_cap)][B]*/, int32_t* count);
int qmhip_episode_fold(qmhip_ctx* ctx, int B, int tick, double period, const double* time /*[B]*/, const double* rbd /*[B][55]*/, const int32_t* contact /*[B][4]*/,
                       const double* force /*[B][12]*/, const int32_t* mode /*[B]*/, const double* wbc_out /*[B][54]*/, const int32_t* qp_status /*[B][3]*/,
                       const int32_t* sim_status /*[B] or NULL*/, const int32_t* mpc_status /*[B] or NULL: no MPC call on this tick*/);

/* ---- instrumentation (ocs2 benchmark::RepeatedTimer analogue, QMController.cpp:145-147,321-323) ----
 * per-kernel HIP-event timing on the stream each kernel runs on; names: "grid","lq_kin","lq","riccati","ls_eval","ls_misc","policy","wbc","sim","plan_nodes","plan_states","plan_footholds","episode".
 * enable: 0 off, 1 a span around every launch, 2 only around the three modelled kernels "lq","riccati","wbc", 3 only around "lq" — the dominant kernel, all the
 * bench's timed region carries (two event records cost about one launch) */
int qmhip_set_profiling(qmhip_ctx* ctx, int enable);
int qmhip_get_kernel_ms(qmhip_ctx* ctx, const char* name, double* total_ms, int* launches);
int qmhip_reset_kernel_ms(qmhip_ctx* ctx);
int qmhip_synchronize(qmhip_ctx* ctx);
/* line-search trials of the last SQP iteration (the longest search of the batch).  Since round 6 the trials after the first run on the device without the host
 * (qm_ls_tail_kernel): the count is read back from the device's trial counters on demand — this call synchronises the context's streams */
int qmhip_last_ls_trials(const qmhip_ctx* ctx);
/* debug/parity access to a device buffer by name (see QmMpcBuffers); copies `bytes` to host */
int qmhip_debug_read(qmhip_ctx* ctx, const char* buffer, void* dst, size_t bytes);
/* profiling / parity switches: "riccati_skip" bit mask of kernel phases to skip (results are then meaningless; 20 = no backward stage and no rollout, i.e. the stage
 * records stay as the LQ kernel wrote them), "wbc_stop", "lq_prof", "lq_debug" (1: the LQ kernel also writes the unprojected LQ model of every interval into the
 * buffer "lqdbg" and the null-space basis into the stage record — tests/test_gpu_lq_records.py); launch-order switches for same-box A/Bs and the bit-identity tests
 * (results do not depend on them): "ls_device_tail" (1: the line search's later trials in one launch on the device; 0: one host round trip per trial, rounds 1-5),
 * "fused_policy" (1: the policy at t0 from the deciding kernels, apply beside the WBC; 0: apply -> policy kernel -> WBC), "r_dense" (1: the dense instances of the trial
 * evaluation and of the LQ kernel's input-weight product although the table's R is block diagonal — same bits; readable: "r_blocks" = the structured instances run) */
int qmhip_debug_set(qmhip_ctx* ctx, const char* key, int value);
/* read such a switch back (bench.py asserts they are all 0 before it times anything) */
int qmhip_debug_get(const qmhip_ctx* ctx, const char* key, int* value);
/* micro-benchmarks used to anchor the FP64 roofline: returns achieved TFLOP/s */
int qmhip_microbench_fp64(qmhip_ctx* ctx, int use_mfma, double* tflops);

#define QMHIP_OK 0
#define QMHIP_ERR_ARG  -1
#define QMHIP_ERR_FILE -2
#define QMHIP_ERR_MODEL -3
#define QMHIP_ERR_HIP  -4
#define QMHIP_ERR_STATE -5

#ifdef __cplusplus
}
#endif
#endif
