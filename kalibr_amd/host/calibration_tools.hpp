// calibration_tools.hpp -- the stages of kalibr_calibrate_cameras that feed the rig problem and the incremental
// estimator, over any LinearSystemSolver behind Optimizer2 (the GPU solver in production, the
// tests' oracle-backed one as the checker).  Paths are relative to the reference repository:
//   CalibrateSingleCamera       aslam_offline_calibration/kalibr2/include/kalibr2/CalibrationTools.hpp:93-144
//   CalibrateStereoPair         CalibrationTools.hpp:183-300 (baseline guess: median of the per-view PnP relative
//                               transforms, :192-234)
//   getTargetPoseGuess          CalibrationTools.hpp:315-356
//   CalibrateMultiCameraRig     CalibrationTools.hpp:376-428
//   CreateBatchProblem          CalibrationTools.hpp:460-521 (as a backend::CalibrationBatch)
//   SynchronizedObservationView aslam_offline_calibration/kalibr2/src/SynchronizedObservationView.cpp:35-90
//   BuildCameraGraph, GetTransform  aslam_offline_calibration/kalibr2/src/CameraGraph.cpp:10-169
//   math::median                aslam_offline_calibration/kalibr2/src/BasicMathUtils.cpp:10-30
//   the stage sequence          aslam_offline_calibration/kalibr2_ros/src/CalibrateCameras.cpp:142-356
// Dijkstra's search comes from common_robotics_utilities (fetched by the reference's CMake, absent here): a plain
// restatement with a documented tie rule.  Reference quirks are kept and named where they occur (see the .cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "calibration_io.hpp"
#include "kalibr_backend.hpp"

namespace kalibr_amd {
namespace tools {

using io::AprilgridTarget;
using io::GridObservation;
using io::SyncedSet;
using io::Transformation;

/// the linear system solver each stage's Optimizer2 runs over (a fresh one per stage problem)
using SolverFactory = std::function<std::shared_ptr<backend::ProblemLinearSystemSolver>()>;

/// CameraCalibrator<CameraT> reduced to what the stages change: the model and its geometry's intrinsics
/// ([KB_MAX_INTR]: projection parameters then distortion), which the reference updates in place through the shared
/// design variables of every stage (CameraCalibrator.hpp:108-122).
struct CameraCalibrator {
  int32_t model = 0;
  std::vector<double> intrinsics;  // [KB_MAX_INTR]
  /// geometry.estimateTransformation(obs, T) with the current intrinsics
  bool estimateTransformation(const GridObservation& obs, const AprilgridTarget& target, Transformation& T) const;
};

/// CreateDefaultOptimizer (CalibrationTools.hpp:57-66): LM(lambda 10), 200 iterations, dX 1e-3, dJ 1, 4 threads
backend::Optimizer2Options defaultOptimizerOptions();

/// how the stages run Optimizer2: the host loop over the solver (Optimizer2::optimize, any solver) or, when the
/// solver is a GpuLinearSystemSolver behind the term layer, the device-resident loop (Optimizer2::optimizeOnDevice)
struct StageOptions {
  SolverFactory solver;
  bool deviceLoop = false;
};

struct StageResult {
  backend::SolutionReturnValue ret;
  size_t frames = 0, views = 0, terms = 0;
};

/// CalibrateSingleCamera: initializeIntrinsics (its result ignored, as the reference's shadowed `success`), then one
/// target-pose DV per observation whose PnP succeeds (failures skipped), intrinsics DVs first, and LM bundle
/// adjustment.  Updates cam.intrinsics; returns !linearSolverFailure.
bool calibrateSingleCamera(const std::vector<GridObservation>& observations, CameraCalibrator& cam,
                           const AprilgridTarget& target, std::optional<double> fallbackFocalLength,
                           const StageOptions& so, StageResult* out = nullptr);

/// median of each component (math::median: std::nth_element at size / 2, the upper median for even sizes)
double median(std::vector<double> v);

/// RotationVector::rotationMatrixToParameters / parametersToRotationMatrix (sm_kinematics RotationVector.cpp:10-80)
std::array<double, 3> rotationMatrixToParameters(const std::array<double, 9>& C);
std::array<double, 9> parametersToRotationMatrix(const std::array<double, 3>& p);
/// Transformation::inverse (Transformation.cpp:83-87)
Transformation inverse(const Transformation& T);

/// the baseline guess of CalibrateStereoPair (:192-234): T_H^-1 T_L per set where both PnPs succeed, translation and
/// rotation-vector medians.  Throws (math::median's error) when no set has both.
Transformation stereoBaselineGuess(const CameraCalibrator& L, const CameraCalibrator& H,
                                   const std::vector<std::optional<GridObservation>>& obsL,
                                   const std::vector<std::optional<GridObservation>>& obsH,
                                   const AprilgridTarget& target);

/// CalibrateStereoPair: returns T_H_L (camera L to camera H) and updates both cameras' intrinsics.  DV order:
/// baseline, target poses, intrinsics L, intrinsics H; terms: every L view, then every H view.
StageResult calibrateStereoPair(CameraCalibrator& L, CameraCalibrator& H,
                                const std::vector<std::optional<GridObservation>>& obsL,
                                const std::vector<std::optional<GridObservation>>& obsH, const AprilgridTarget& target,
                                const StageOptions& so, Transformation& T_H_L, Transformation* guess = nullptr);

/// getTargetPoseGuess: PnP of the camera with the most corners (current intrinsics; a failed PnP leaves the identity,
/// as the reference ignores its result), carried by std::accumulate(baselines[0 .. max), T_t_cN, *)
Transformation getTargetPoseGuess(const std::vector<CameraCalibrator>& cams, const SyncedSet& set,
                                  const std::vector<Transformation>& baselineGuesses, const AprilgridTarget& target);

/// CalibrateMultiCameraRig: returns the optimized baselines, updates every camera's intrinsics; throws on a linear
/// solver failure
std::vector<Transformation> calibrateMultiCameraRig(std::vector<CameraCalibrator>& cams,
                                                    const std::vector<SyncedSet>& sets, const AprilgridTarget& target,
                                                    const std::vector<Transformation>& baselineGuesses,
                                                    const StageOptions& so, StageResult* out = nullptr);

/// SynchronizedObservationView over per-camera observation lists sorted by time: pivot = the oldest head (lowest
/// camera index on ties), window [t, t + tolerance], every head inside it joins the set and advances
std::vector<SyncedSet> synchronizeObservations(const std::vector<std::vector<GridObservation>>& byCamera,
                                               double tolerance);
/// GetAllObservationsFromSource
std::vector<std::optional<GridObservation>> observationsFromSource(const std::vector<SyncedSet>& sets, size_t source);

/// BuildCameraGraph: nodes = cameras, edge (i, j) of weight 1 / (common corners summed over the sets) when > 0
struct CameraGraph {
  size_t nodes = 0;
  std::map<std::pair<size_t, size_t>, double> edges;  // i < j
};
CameraGraph buildCameraGraph(const std::vector<SyncedSet>& sets);

/// common_robotics_utilities::simple_graph_search::PerformDijkstrasAlgorithm (restated): previous[start] = start,
/// unreachable nodes previous = -1 and distance = +inf.  Ties: a node settles in (distance, index) order and its
/// predecessor changes only on a strictly shorter path.
struct DijkstraResult {
  std::vector<double> distance;
  std::vector<long> previous;
  long previousIndex(size_t i) const { return previous.at(i); }
  size_t size() const { return distance.size(); }
};
DijkstraResult dijkstra(const CameraGraph& g, size_t start);

/// GetTransform (CameraGraph.cpp:126-169): the transforms along the path from the node further from the search start
/// to the other, composed by std::accumulate in path order, inverted when the left node is the closer one.  The
/// reference loops forever (or indexes past its map) when the nearer node is not on the further node's path to the
/// start; here that throws.
Transformation getTransform(const std::map<std::pair<size_t, size_t>, Transformation>& map, const DijkstraResult& r,
                            size_t left, size_t right);

/// the CLI flow of CalibrateCameras.cpp:142-356 from per-camera observations to the exported YAML
struct CalibrateCamerasOptions {
  std::vector<std::optional<double>> focalLengths;  // per camera (calibration_config.yaml focal_length)
  double approxSyncTolerance = 0.02;                // --approx-sync-tolerance (seconds)
  double mutualInformationTolerance = 0.2;          // --mi-tol
  std::optional<size_t> maxBatches;                 // --max-batches
  size_t estimatorMaxIterations = 20;               // optimizer_options.maxIterations (:271)
  bool verbose = false;
  /// corner_uncertainty (kalibr2/CalibrationTools.hpp:391-393): invR = I / sigma^2 of every reprojection term of the
  /// final batch problem; 1.0 (the default) sets nothing.  parameterStdDev scales with it.
  double cornerUncertainty = 1.0;
  /// ErrorTerm::setMEstimatorPolicy for every term of the final batch problem (null: none).
  /// NOTE: today this changes NO result of calibrateCameras.  The stages and the incremental estimator run unweighted
  /// (their device paths carry no weights), and the only consumer of the final batch problem is the covariance, which
  /// is Optimizer2::computeHessian's system (useMEstimator = false) and so ignores the estimator.  Passing Huber here
  /// does not make the calibration resist outliers; its one effect is that a stage solver without robust terms is
  /// refused up front.  The option is the hook for a batch refinement over the final problem; until that exists, use
  /// CalibrationProblem::setMEstimatorPolicy with Optimizer2 over GpuLinearSystemSolver for a robust fit.
  std::shared_ptr<const backend::MEstimator> mEstimator;
};

struct CalibrateCamerasResult {
  std::vector<CameraCalibrator> afterSingle, afterStereo, afterRig, final;
  std::vector<StageResult> single, stereo;
  std::vector<std::pair<size_t, size_t>> stereoPairs;            // (camera, its Dijkstra predecessor)
  std::map<std::pair<size_t, size_t>, Transformation> optimalBaselines;
  std::vector<Transformation> baselineGuesses, rigBaselines, finalBaselines;
  StageResult rig;
  std::vector<SyncedSet> syncedSets;
  DijkstraResult graphSearch;
  std::vector<int> batchAccepted;
  std::vector<long> batchIterations, batchRank;
  size_t acceptedBatches = 0, processedBatches = 0;
  std::vector<double> finalState;  // the estimator's state: intrinsics | baselines | accepted target poses
  /// the numbers CalibrateCameras.cpp:316-318 prints per camera (CameraCalibrator::PrintReprojectionErrorStatistics,
  /// CameraCalibrator.hpp:368-411) over the terms of EVERY processed batch, as the reference's calibrators store them
  /// at CreateBatchProblem (CalibrationTools.hpp:511) whether the batch is kept or not, at the final intrinsics and
  /// baselines and each batch's final target pose (kept: the estimator's; rejected: the guess, which
  /// IncrementalEstimator::addBatch restores, IncrementalEstimator.cpp:348-350, 512-518): per camera
  /// [n, mean_u, mean_v, std_u, std_v, rmse], computed by the stage solver (the device for GpuLinearSystemSolver)
  std::vector<std::array<double, 6>> reprojectionErrorStatistics;
  /// how well determined the calibration is: sqrt of the diagonal of Sigma_cc = the camera block of (J^T J)^-1
  /// (lambda = 0) of the accepted batches' problem at the final state, camera columns in canonical order
  /// [intrinsics | baselines].  Filled only when the stage solver supportsCovariance() and the factorisation succeeds;
  /// empty otherwise (never an error).  In units of options.cornerUncertainty (sigma px per corner): sigma times
  /// the sigma = 1 values.
  std::vector<double> parameterStdDev;
};

/// `estimatorSolver` is the IncrementalEstimator's marginal solver (GpuMarginalLinearSolver in production)
CalibrateCamerasResult calibrateCameras(const std::vector<int32_t>& models,
                                        const std::vector<std::vector<GridObservation>>& observationsByCamera,
                                        const AprilgridTarget& target, const CalibrateCamerasOptions& options,
                                        const StageOptions& stages,
                                        std::shared_ptr<backend::MarginalLinearSystemSolver> estimatorSolver);

}  // namespace tools
}  // namespace kalibr_amd
