// Test driver for the covariance surface of the C++ host layer (kalibr_amd/host/kalibr_backend.*), run by
// tests/test_host_cov.py.  The problem loader, the oracle-backed solvers and the design-variable / term helpers are
// the ones of tests/cpp/test_host.cpp (included below with its main renamed).
//   test_host_cov ranges                : covarianceBlockRange / canonicalBlockDimensions of a pinhole-radtan (4|4),
//                                         FOV (4|1), EUCM (6) rig with 3 frames, every DV pair
//   test_host_cov unsupported <p.bin>   : a ProblemLinearSystemSolver without the override (the oracle-backed one):
//                                         supportsCovariance, the throw, and calibrateCameras over it
//   test_host_cov stddev-gpu <p.bin>    : calibrateCameras over the GPU solvers: parameterStdDev is filled
//   test_host_cov gpu <p.bin>           : Optimizer2::computeDiagonalCovariances / computeCovarianceBlocks /
//                                         computeHessian over GpuLinearSystemSolver against the C-ABI blocks, directly
//                                         and through TermLinearSystemSolver in insertion and shuffled DV order
// Prints one JSON line.
#define main test_host_main
#include "test_host.cpp"
#undef main

namespace {

const char* source_name(CovarianceBlockRange::Source s) {
  switch (s) {
    case CovarianceBlockRange::Source::Pcc: return "Pcc";
    case CovarianceBlockRange::Source::Pff: return "Pff";
    case CovarianceBlockRange::Source::Pfc: return "Pfc";
    default: return "PfcT";
  }
}

int run_ranges() {
  const std::vector<int32_t> models = {KB_PINHOLE_RADTAN, KB_PINHOLE_FOV, KB_EUCM};
  const int F = 3;
  const std::vector<int> dims = canonicalBlockDimensions(models, F);
  std::string s = "{\"dims\": " + ints(dims) + ", \"pairs\": [";
  const int n = (int)dims.size();
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      char buf[160];
      try {
        const CovarianceBlockRange r = covarianceBlockRange(models, F, i, j);
        std::snprintf(buf, sizeof(buf), "[\"%s\", %d, %d, %d, %d, %d]", source_name(r.source), r.frame, r.row0, r.rows,
                      r.col0, r.cols);
      } catch (const LinearSystemSolver::Exception& e) {
        std::snprintf(buf, sizeof(buf), "[\"throw\", %d, 0, 0, 0, 0]",
                      std::string(e.what()).find("different frames") != std::string::npos ? 1 : 0);
      }
      s += std::string(i || j ? ", " : "") + buf;
    }
  int oob = 0;
  for (const auto& pr : std::vector<std::pair<int, int>>{{-1, 0}, {0, n}, {n, n}}) try {
      covarianceBlockRange(models, F, pr.first, pr.second);
    } catch (const LinearSystemSolver::Exception&) {
      ++oob;
    }
  std::printf("%s], \"out_of_range_throws\": %d}\n", s.c_str(), oob);
  return 0;
}

int run_unsupported(const CalibrationProblem& p) {
  namespace io = kalibr_amd::io;
  namespace tl = kalibr_amd::tools;
  auto s = std::make_shared<OracleProblemSolver>();
  s->initMatrixStructure(p, false);
  s->buildSystem(4, false);
  const bool supports = s->supportsCovariance();
  std::string msg, msg_opt;
  std::vector<std::vector<double>> blocks;
  try {
    s->computeCovarianceBlocks({{0, 0}}, blocks);
  } catch (const LinearSystemSolver::Exception& e) {
    msg = e.what();
  }
  Optimizer2Options oo;
  oo.linearSystemSolver = s;
  try {
    Optimizer2(oo).computeDiagonalCovariances(0.0);
  } catch (const LinearSystemSolver::Exception& e) {
    msg_opt = e.what();
  }
  // the stage sequence over solvers without a covariance path: returns normally, no standard deviations
  io::AprilgridTarget tgt;
  const auto byCam = observations_by_camera(p, 1280, 1024, 1);
  tl::StageOptions so;
  so.solver = []() -> std::shared_ptr<ProblemLinearSystemSolver> { return std::make_shared<OracleProblemSolver>(); };
  LinearSolverOptions lo;
  lo.columnScaling = true;
  lo.epsSVD = 1e-6;
  tl::CalibrateCamerasOptions co;
  co.focalLengths.assign(p.n_cams(), std::nullopt);
  const tl::CalibrateCamerasResult r =
      tl::calibrateCameras(p.cam_model, byCam, tgt, co, so, std::make_shared<OracleMarginalSolver>(lo, 4));
  std::printf("{\"supports\": %d, \"message\": \"%s\", \"optimizer_message\": \"%s\", \"blocks\": %zu, "
              "\"std_dev_size\": %zu, \"accepted_batches\": %zu, \"stats_cams\": %zu}\n",
              supports ? 1 : 0, msg.c_str(), msg_opt.c_str(), blocks.size(), r.parameterStdDev.size(), r.acceptedBatches,
              r.reprojectionErrorStatistics.size());
  return 0;
}

// the stage sequence over the GPU solvers: parameterStdDev = sqrt diag Sigma_cc of the accepted batches' problem at the
// final state
int run_stddev_gpu(const CalibrationProblem& p) {
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
  const tl::CalibrateCamerasResult r =
      tl::calibrateCameras(p.cam_model, byCam, tgt, co, so, std::make_shared<GpuMarginalLinearSolver>(lo));
  double mn = 1e300, mx = 0.0;
  for (double v : r.parameterStdDev) {
    mn = std::min(mn, v);
    mx = std::max(mx, std::isfinite(v) ? v : 1e300);
  }
  std::printf("{\"std_dev_size\": %zu, \"min\": %.6e, \"max\": %.6e, \"accepted_batches\": %zu, \"std_dev\": %s}\n",
              r.parameterStdDev.size(), mn, mx, r.acceptedBatches, jv(r.parameterStdDev).c_str());
  return 0;
}

// worst |a - b|_ij / sqrt(b_ii b_jj) over a square block
double corr_err(const std::vector<double>& a, const std::vector<double>& b, int n) {
  double m = a.size() == b.size() && (int)b.size() == n * n ? 0.0 : 1e300;
  for (int i = 0; i < n && m < 1e300; ++i)
    for (int j = 0; j < n; ++j) m = std::max(m, std::fabs(a[i * n + j] - b[i * n + j]) / std::sqrt(b[i * n + i] * b[j * n + j]));
  return m;
}

int run_gpu(const CalibrationProblem& p) {
  const int F = p.n_frames;
  auto g = std::make_shared<GpuLinearSystemSolver>();
  g->initMatrixStructure(p, false);
  Optimizer2Options oo;
  oo.linearSystemSolver = g;
  Optimizer2 opt(oo);
  // diagonal blocks of every DV against the C-ABI blocks of the same system
  const std::vector<std::vector<double>> diag = opt.computeDiagonalCovariances(0.0);
  const std::vector<int> dims = g->blockDimensions();
  const size_t C = g->cameraCols();
  std::vector<double> Pcc(C * C), Pff((size_t)F * 36), Pfc((size_t)F * 6 * C);
  int ok = 0;
  if (kb_covariance(static_cast<kb_handle*>(g->handle()), Pcc.data(), Pff.data(), Pfc.data(), &ok) < 0 || !ok)
    throw std::runtime_error(std::string("kb_covariance: ") + kb_last_error());
  const int ncam = (int)dims.size() - 2 * F;
  double abi_diff = diag.size() == dims.size() ? 0.0 : 1e300;
  {
    size_t col = 0;
    for (int k = 0; k < (int)dims.size() && abi_diff < 1e300; ++k) {
      const int n = dims[k];
      for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
          const double ref = k < ncam ? Pcc[(col + a) * C + col + b]
                                      : Pff[(size_t)((k - ncam) / 2) * 36 + (3 * ((k - ncam) % 2) + a) * 6 + 3 * ((k - ncam) % 2) + b];
          abi_diff = std::max(abi_diff, std::fabs(diag[k][a * n + b] - ref));
        }
      if (k < ncam) col += n;
    }
  }
  // off-diagonal pairs: camera x camera, frame q x frame t, frame x camera and its transpose
  const int fq = ncam + 2 * (F - 1), ft = fq + 1;
  const std::vector<std::vector<double>> off =
      opt.computeCovarianceBlocks({{1, 0}, {fq, ft}, {ft, 0}, {0, ft}}, 0.0);
  double off_diff = 0.0;
  for (int a = 0; a < dims[1]; ++a)
    for (int b = 0; b < dims[0]; ++b) off_diff = std::max(off_diff, std::fabs(off[0][a * dims[0] + b] - Pcc[(dims[0] + a) * C + b]));
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      off_diff = std::max(off_diff, std::fabs(off[1][a * 3 + b] - Pff[(size_t)(F - 1) * 36 + a * 6 + 3 + b]));
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < dims[0]; ++b) {
      const double ref = Pfc[((size_t)(F - 1) * 6 + 3 + a) * C + b];
      off_diff = std::max(off_diff, std::fabs(off[2][a * dims[0] + b] - ref));
      off_diff = std::max(off_diff, std::fabs(off[3][b * 3 + a] - ref));
    }
  // a pair of two different frames is refused
  int cross_throws = 0;
  try {
    opt.computeCovarianceBlocks({{ncam, ncam + 2}}, 0.0);
  } catch (const LinearSystemSolver::Exception& e) {
    cross_throws = std::string(e.what()).find("different frames") != std::string::npos ? 1 : 0;
  }
  // computeHessian(lambda) = the normal blocks + lambda^2 on the diagonal
  const double lambda = 3.0;
  const HessianBlocks H = opt.computeHessian(lambda);
  std::vector<double> Hff((size_t)F * 36), Hfc((size_t)F * 6 * C), gf((size_t)F * 6), Hcc(C * C), gc(C);
  double cost = 0.0;
  if (kb_get_normal_blocks(static_cast<kb_handle*>(g->handle()), Hff.data(), Hfc.data(), gf.data(), Hcc.data(), gc.data(), &cost) < 0)
    throw std::runtime_error(std::string("kb_get_normal_blocks: ") + kb_last_error());
  for (size_t k = 0; k < C; ++k) Hcc[k * C + k] += lambda * lambda;
  for (size_t k = 0; k < (size_t)F * 6; ++k) Hff[(k / 6) * 36 + (k % 6) * 7] += lambda * lambda;
  const double hess_diff = (H.C == C && H.F == (size_t)F) ? std::max({maxdiff(H.Hcc, Hcc, 0, Hcc.size()), maxdiff(H.Hff, Hff, 0, Hff.size()),
                                                                     maxdiff(H.Hfc, Hfc, 0, Hfc.size())})
                                                        : 1e300;
  // through the design-variable / error-term layer: insertion order (mode 0) and a seeded shuffle (mode 2)
  double term_err[3] = {0.0, 0.0, 0.0};
  int frames_reordered = 0;
  for (int mode = 0; mode < 3; mode += 2) {
    TermProblem t = to_terms(p);
    const std::vector<DesignVariable*> dvs = assignColumnBases(dv_order(t, mode));
    auto ts = std::make_shared<TermLinearSystemSolver>(std::make_shared<GpuLinearSystemSolver>(), p.target);
    ts->initMatrixStructure(dvs, t.errors, false);
    for (int f = 0; f < F; ++f) frames_reordered += ts->assembly().frameRotation[f] != t.frot[f];
    Optimizer2Options to;
    to.linearSystemSolver = ts;
    const std::vector<std::vector<double>> tb = Optimizer2(to).computeDiagonalCovariances(0.0);
    const std::vector<int> tdims = ts->blockDimensions();
    double& err = term_err[mode];
    if (tb.size() != diag.size() || tdims.size() != dims.size()) err = 1e300;
    int k = 0;  // canonical DV index of the packed problem
    auto cmp = [&](const DesignVariable* dv) {
      if (dv && err < 1e300) {
        if (tdims[dv->blockIndex] != dims[k]) err = 1e300;
        else err = std::max(err, corr_err(tb[dv->blockIndex], diag[k], dims[k]));
      }
      if (dv) ++k;
    };
    for (size_t c = 0; c < t.proj.size(); ++c) {
      cmp(t.proj[c]);
      cmp(t.dist[c]);
    }
    for (size_t j = 0; j < t.brot.size(); ++j) {
      cmp(t.brot[j]);
      cmp(t.btrans[j]);
    }
    for (int f = 0; f < F; ++f) {
      cmp(t.frot[f]);
      cmp(t.ftrans[f]);
    }
    if (mode == 2) {  // a cross-frame pair through the wrapper is refused as well
      try {
        std::vector<std::vector<double>> out;
        ts->computeCovarianceBlocks({{t.frot[0]->blockIndex, t.frot[1]->blockIndex}}, out);
        cross_throws = 0;
      } catch (const LinearSystemSolver::Exception&) {
      }
    }
  }
  std::printf("{\"n_dvs\": %zu, \"abi_diff\": %.3e, \"off_diff\": %.3e, \"cross_throws\": %d, \"hess_diff\": %.3e, "
              "\"term_insertion_err\": %.3e, \"term_shuffled_err\": %.3e, \"frames_reordered\": %d, \"supports\": %d}\n",
              dims.size(), abi_diff, off_diff, cross_throws, hess_diff, term_err[0], term_err[2], frames_reordered,
              g->supportsCovariance() ? 1 : 0);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  try {
    if (mode == "ranges") return run_ranges();
    if (argc < 3) return 2;
    const CalibrationProblem p = load(argv[2]);
    if (mode == "unsupported") return run_unsupported(p);
    if (mode == "gpu") return run_gpu(p);
    if (mode == "stddev-gpu") return run_stddev_gpu(p);
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 2;
}
