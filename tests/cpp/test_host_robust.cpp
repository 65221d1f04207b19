// Test driver for the robust-term surface of the C++ host layer (kalibr_amd/host/kalibr_backend.*), run by
// tests/test_host_robust.py.  The problem loader and the oracle-backed solvers are those of tests/cpp/test_host.cpp
// (included below with its main renamed).
//   test_host_robust estimators            : getWeight / name() of the estimator classes at fixed points
//   test_host_robust unsupported <p.bin>   : a solver without robust terms: the setters throw, calibrateCameras with a
//                                            corner uncertainty over it fails before anything runs
//   test_host_robust optimize-gpu <p.bin>  : Optimizer2::optimize() over GpuLinearSystemSolver with a Huber policy
//                                            against kb_optimize (optimizeOnDevice) on the same problem; computeHessian
//                                            ignores the estimator but keeps invR; mEstimatorWeights
//   test_host_robust stddev-gpu <p.bin> <sigma> : calibrateCameras with cornerUncertainty = sigma: parameterStdDev
// Prints one JSON line.
#define main test_host_main
#include "test_host.cpp"
#undef main

namespace {

int run_estimators() {
  const double pts[] = {0.0, 1.0, 3.999, 4.0, 16.0, 400.0};
  NoMEstimator none;
  HuberMEstimator huber(2.0);
  CauchyMEstimator cauchy(4.0);
  GemanMcClureMEstimator gm(9.0);
  BlakeZissermanMEstimator bz(2, 0.999, 0.1);
  const MEstimator* all[] = {&none, &huber, &cauchy, &gm, &bz};
  std::string s = "{";
  for (const MEstimator* m : all) {
    std::vector<double> w;
    for (double p : pts) w.push_back(m->getWeight(p));
    char buf[96];
    std::snprintf(buf, sizeof(buf), ", \"kind\": %d, \"parameter\": %.17g}, ", m->kind(), m->parameter());
    s += "\"" + std::to_string(m->kind()) + "\": {\"name\": \"" + m->name() + "\", \"w\": " + jv(w) + buf;
  }
  int throws = 0;
  try {
    BlakeZissermanMEstimator bad(3, 0.999, 0.1);
  } catch (const std::invalid_argument&) {
    throws = 1;
  }
  CalibrationProblem p;
  p.cornerUncertainty(0.5);
  const bool w1 = p.weighted();
  p.clearCornerInvR();
  p.setMEstimatorPolicy(std::make_shared<NoMEstimator>());
  const bool w2 = p.weighted();
  p.setMEstimatorPolicy(std::make_shared<HuberMEstimator>(2.0));
  const bool w3 = p.weighted();
  p.clearMEstimatorPolicy();
  std::printf("%s\"df3_throws\": %d, \"weighted\": [%d, %d, %d, %d]}\n", s.c_str(), throws, w1, w2, w3, p.weighted());
  return 0;
}

int run_unsupported(const CalibrationProblem& p) {
  namespace io = kalibr_amd::io;
  namespace tl = kalibr_amd::tools;
  auto s = std::make_shared<OracleProblemSolver>();
  s->initMatrixStructure(p, false);
  int throws = 0;
  try {
    s->setMEstimatorPolicy(std::make_shared<HuberMEstimator>(2.0));
  } catch (const LinearSystemSolver::Exception&) {
    ++throws;
  }
  try {
    s->setCornerInvR({4.0, 0.0, 4.0});
  } catch (const LinearSystemSolver::Exception&) {
    ++throws;
  }
  try {
    s->mEstimatorWeights();
  } catch (const LinearSystemSolver::Exception&) {
    ++throws;
  }
  io::AprilgridTarget tgt;
  const auto byCam = observations_by_camera(p, 1280, 1024, 1);
  tl::StageOptions so;
  int made = 0;
  so.solver = [&made]() -> std::shared_ptr<ProblemLinearSystemSolver> {
    ++made;
    return std::make_shared<OracleProblemSolver>();
  };
  LinearSolverOptions lo;
  lo.columnScaling = true;
  lo.epsSVD = 1e-6;
  tl::CalibrateCamerasOptions co;
  co.focalLengths.assign(p.n_cams(), std::nullopt);
  co.cornerUncertainty = 0.5;
  std::string msg;
  try {
    tl::calibrateCameras(p.cam_model, byCam, tgt, co, so, std::make_shared<OracleMarginalSolver>(lo, 4));
  } catch (const std::invalid_argument& e) {
    msg = e.what();
  }
  std::printf("{\"supports\": %d, \"setter_throws\": %d, \"calibrate_message\": \"%s\", \"solvers_made\": %d}\n",
              s->supportsRobustTerms() ? 1 : 0, throws, msg.c_str(), made);
  return 0;
}

double maxabs(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return 1e300;
  double m = 0.0;
  for (size_t i = 0; i < a.size(); ++i) m = std::max(m, std::fabs(a[i] - b[i]));
  return m;
}

int run_optimize_gpu(const CalibrationProblem& p0) {
  CalibrationProblem p = p0;
  p.setMEstimatorPolicy(std::make_shared<HuberMEstimator>(2.0));
  // host loop over the per-call C-ABI
  auto a = std::make_shared<GpuLinearSystemSolver>();
  a->initMatrixStructure(p, false);
  Optimizer2Options oa;
  oa.linearSystemSolver = a;
  oa.trustRegionPolicy = std::make_shared<LevenbergMarquardtTrustRegionPolicy>(10.0);
  oa.maxIterations = 30;
  oa.convergenceDeltaX = 1e-3;
  oa.convergenceDeltaJ = 1.0;
  const SolutionReturnValue ra = Optimizer2(oa).optimize();
  // the device-resident loop (kb_optimize)
  auto b = std::make_shared<GpuLinearSystemSolver>();
  b->initMatrixStructure(p, false);
  Optimizer2Options ob = oa;
  ob.linearSystemSolver = b;
  ob.trustRegionPolicy = std::make_shared<LevenbergMarquardtTrustRegionPolicy>(10.0);
  const SolutionReturnValue rb = Optimizer2(ob).optimizeOnDevice();
  const double state_diff = maxabs(a->state(), b->state());
  // the weights at the optimum flag the outliers (w < 1 exactly where s >= k^2)
  std::vector<double> s;
  const std::vector<double> w = a->mEstimatorWeights(&s);
  size_t down = 0, bad = 0;
  for (size_t k = 0; k < w.size(); ++k) {
    down += w[k] < 1.0;
    bad += (w[k] < 1.0) != (s[k] > 4.0);
  }
  // computeHessian ignores the estimator but keeps invR: equal to an invR-only solver's, different from the weighted
  // system of buildSystem(.., true)
  CalibrationProblem q = p0;
  q.state = a->state();
  q.cornerUncertainty(0.5);
  CalibrationProblem qh = q;
  qh.setMEstimatorPolicy(std::make_shared<HuberMEstimator>(2.0));
  auto c = std::make_shared<GpuLinearSystemSolver>(), d = std::make_shared<GpuLinearSystemSolver>();
  c->initMatrixStructure(q, false);
  d->initMatrixStructure(qh, false);
  Optimizer2Options oc, od;
  oc.linearSystemSolver = c;
  od.linearSystemSolver = d;
  const HessianBlocks Hc = Optimizer2(oc).computeHessian(0.0), Hd = Optimizer2(od).computeHessian(0.0);
  const double hess_diff = std::max({maxabs(Hc.Hcc, Hd.Hcc), maxabs(Hc.Hff, Hd.Hff), maxabs(Hc.Hfc, Hd.Hfc)});
  d->buildSystem(4, true);
  HessianBlocks Hw;
  d->copyHessian(Hw);
  const double weighted_diff = maxabs(Hw.Hcc, Hd.Hcc);
  // invR = I / sigma^2 scales the unweighted Hessian by 1 / sigma^2
  auto e = std::make_shared<GpuLinearSystemSolver>();
  CalibrationProblem q1 = p0;
  q1.state = a->state();
  e->initMatrixStructure(q1, false);
  Optimizer2Options oe;
  oe.linearSystemSolver = e;
  const HessianBlocks He = Optimizer2(oe).computeHessian(0.0);
  double scale_err = 0.0, hmax = 0.0;
  for (size_t k = 0; k < He.Hcc.size(); ++k) {
    scale_err = std::max(scale_err, std::fabs(Hc.Hcc[k] - 4.0 * He.Hcc[k]));
    hmax = std::max(hmax, std::fabs(4.0 * He.Hcc[k]));
  }
  std::printf("{\"host_iterations\": %d, \"device_iterations\": %d, \"host_failed\": %d, \"device_failed\": %d, "
              "\"state_diff\": %.3e, \"J_host\": %.17g, \"J_device\": %.17g, \"J_start\": %.17g, \"downweighted\": %zu, "
              "\"weight_flag_mismatches\": %zu, \"n_terms\": %zu, \"hess_diff\": %.3e, \"weighted_diff\": %.3e, "
              "\"scale_rel_err\": %.3e}\n",
              ra.iterations, rb.iterations, ra.failedIterations, rb.failedIterations, state_diff, ra.JFinal, rb.JFinal,
              ra.JStart, down, bad, w.size(), hess_diff, weighted_diff, scale_err / hmax);
  return 0;
}

int run_stddev_gpu(const CalibrationProblem& p, double sigma) {
  namespace io = kalibr_amd::io;
  namespace tl = kalibr_amd::tools;
  io::AprilgridTarget tgt;
  const auto byCam = observations_by_camera(p, 1280, 1024, 1);
  tl::StageOptions so;
  so.solver = []() -> std::shared_ptr<ProblemLinearSystemSolver> { return std::make_shared<GpuLinearSystemSolver>(); };
  so.deviceLoop = true;
  LinearSolverOptions lo;
  lo.columnScaling = true;
  lo.epsSVD = 1e-6;
  tl::CalibrateCamerasOptions co;
  co.focalLengths.assign(p.n_cams(), std::nullopt);
  co.cornerUncertainty = sigma;
  const tl::CalibrateCamerasResult r =
      tl::calibrateCameras(p.cam_model, byCam, tgt, co, so, std::make_shared<GpuMarginalLinearSolver>(lo));
  std::vector<double> acc(r.batchAccepted.begin(), r.batchAccepted.end());
  std::printf("{\"std_dev\": %s, \"accepted_batches\": %zu, \"batch_accepted\": %s, \"final_state\": %s}\n",
              jv(r.parameterStdDev).c_str(), r.acceptedBatches, jv(acc).c_str(), jv(r.finalState).c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  try {
    if (mode == "estimators") return run_estimators();
    if (argc < 3) return 2;
    const CalibrationProblem p = load(argv[2]);
    if (mode == "unsupported") return run_unsupported(p);
    if (mode == "optimize-gpu") return run_optimize_gpu(p);
    if (mode == "stddev-gpu" && argc >= 4) return run_stddev_gpu(p, std::atof(argv[3]));
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 2;
}
