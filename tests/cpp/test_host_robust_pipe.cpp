// Test driver for GpuLinearSystemSolver::setRobustBuild (kalibr_amd/host/kalibr_backend.*), run by
// tests/test_host_robust_pipe.py.  The problem loader is tests/cpp/test_host.cpp's (included with its main renamed).
//   test_host_robust_pipe gn-gpu <p.bin> <invR.f64> <cauchy sigma^2> : a weighted solver (Cauchy + per-corner invR, the
//       file holds n_corners x [a, b, c] doubles) in Pipe mode under Optimizer2::optimizeOnDevice() with the GN policy
//   test_host_robust_pipe refuse-gpu <p.bin> : setRobustBuild(Pipe) on a rig that builds with k_build
// Prints one JSON line.
#define main test_host_main
#include "test_host.cpp"
#undef main

#include <fstream>

namespace {

std::string kernel_name(const GpuLinearSystemSolver& s) {
  char buf[32] = {0};
  kb_build_kernel_name(static_cast<kb_handle*>(s.handle()), buf, sizeof(buf));
  return buf;
}

int run_gn_gpu(const CalibrationProblem& p0, const char* invr_path, double sigma2) {
  std::ifstream f(invr_path, std::ios::binary);
  std::vector<double> invR(3 * (size_t)p0.n_corners());
  f.read(reinterpret_cast<char*>(invR.data()), (std::streamsize)(sizeof(double) * invR.size()));
  if (!f) throw std::runtime_error("invR file too short");
  CalibrationProblem p = p0;
  p.setMEstimatorPolicy(std::make_shared<CauchyMEstimator>(sigma2));
  p.setCornerInvR(invR);
  auto g = std::make_shared<GpuLinearSystemSolver>();
  g->setRobustBuild(RobustBuild::Pipe);  // before initMatrixStructure: applied there
  g->initMatrixStructure(p, false);
  const std::string kn = kernel_name(*g);
  Optimizer2Options o;
  o.linearSystemSolver = g;
  o.trustRegionPolicy = std::make_shared<GaussNewtonTrustRegionPolicy>();
  o.maxIterations = 8;
  o.convergenceDeltaX = 1e-3;
  o.convergenceDeltaJ = 1.0;
  Optimizer2 opt(o);
  const SolutionReturnValue r = opt.optimizeOnDevice();
  // the fused entry points are there (a General-mode weighted handle refuses kb_run_gn_iterations)
  const std::vector<double> st = g->state();
  double sec = 0.0;
  const int rc_fused = kb_run_gn_iterations(static_cast<kb_handle*>(g->handle()), 1, &sec);
  // back to General after the run: k_build, and the fused entry point refused again
  g->setRobustBuild(RobustBuild::General);
  const std::string kn_general = kernel_name(*g);
  const int rc_general = kb_run_gn_iterations(static_cast<kb_handle*>(g->handle()), 1, &sec);
  std::printf("{\"kernel\": \"%s\", \"kernel_general\": \"%s\", \"iterations\": %d, \"failed\": %d, \"J_start\": %.17g, "
              "\"J_final\": %.17g, \"linear_solver_failure\": %d, \"rc_fused\": %d, \"rc_general\": %d, \"mode\": %d, "
              "\"state\": %s}\n",
              kn.c_str(), kn_general.c_str(), r.iterations, r.failedIterations, r.JStart, r.JFinal,
              r.linearSolverFailure ? 1 : 0, rc_fused, rc_general, (int)g->robustBuild(), jv(st).c_str());
  return 0;
}

int run_refuse_gpu(const CalibrationProblem& p0) {
  CalibrationProblem p = p0;
  p.setMEstimatorPolicy(std::make_shared<HuberMEstimator>(2.0));
  auto g = std::make_shared<GpuLinearSystemSolver>();
  g->initMatrixStructure(p, false);
  const double J0 = g->evaluateError(1, true);
  std::string msg;
  try {
    g->setRobustBuild(RobustBuild::Pipe);
  } catch (const LinearSystemSolver::Exception& e) {
    msg = e.what();
  }
  const double J1 = g->evaluateError(1, true);
  // a solver told Pipe before it has a handle fails in initMatrixStructure with the same message
  auto g2 = std::make_shared<GpuLinearSystemSolver>();
  g2->setRobustBuild(RobustBuild::Pipe);
  std::string msg2;
  try {
    g2->initMatrixStructure(p, false);
  } catch (const LinearSystemSolver::Exception& e) {
    msg2 = e.what();
  }
  std::printf("{\"message\": \"%s\", \"message_init\": \"%s\", \"mode\": %d, \"kernel\": \"%s\", \"cost_same\": %d}\n",
              msg.c_str(), msg2.c_str(), (int)g->robustBuild(), kernel_name(*g).c_str(), J0 == J1 ? 1 : 0);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  try {
    const CalibrationProblem p = load(argv[2]);
    if (mode == "gn-gpu" && argc >= 5) return run_gn_gpu(p, argv[3], std::atof(argv[4]));
    if (mode == "refuse-gpu") return run_refuse_gpu(p);
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 2;
}
