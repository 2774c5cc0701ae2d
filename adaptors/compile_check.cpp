// adaptors/compile_check.cpp — translation unit for the syntax / type check of the adaptors against adaptors/stubs (tests/test_adaptors.py)
#define QMHIP_ADAPTOR_STUBS 1
#include "QmhipController.h"
int qmhip_adaptors_compile_check() {
  qm::QmhipSolver::Sizes s{160, 2, 64};
  ocs2::PrimalSolution p; ocs2::ModeSchedule ms;
  double t[2] = {0, 1}, x[60] = {0}, u[60] = {0}; int32_t ev[2] = {0, 0};
  qm::toPrimalSolution(2, t, ev, x, u, ms, p);
  std::vector<double> gain(2 * 900, 0.0), uff(60, 0.0);
  qm::setLinearController(2, gain.data(), uff.data(), p);      // the useFeedbackPolicy branch: an ocs2::LinearController over the same time stamps
  void (qm::QmhipSolver::*fb)(bool) = &qm::QmhipSolver::setFeedbackPolicy; (void)fb;
  // the initRollout seam (QMController.cpp:311): MPC_MRT_Interface::rolloutPolicy's signature on the device solver
  void (qm::QmhipSolver::*ro)(ocs2::scalar_t, const ocs2::vector_t&, ocs2::scalar_t, ocs2::vector_t&, ocs2::vector_t&, size_t&, ocs2::scalar_t, bool, struct qmhip_rollout_summary*) const = &qm::QmhipSolver::rolloutPolicy; (void)ro;
  dynamic_reconfigure::Config cfg; cfg.doubles.push_back({"kp_swing", 350.0});
  int (qm::QmhipWbc::*apply)(const dynamic_reconfigure::Config&) = &qm::QmhipWbc::applyReconfigure; (void)apply;
  return (int)p.timeTrajectory_.size() + s.maxNodes + (int)cfg.doubles.size();
}
