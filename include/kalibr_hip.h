/*
 * kalibr_hip.h -- C-ABI of the MI355X-native batch calibration backend.
 *
 * Drop-in boundary for aslam_backend's LinearSystemSolver plugin surface
 * (aslam_optimizer/aslam_backend/include/aslam/backend/LinearSystemSolver.hpp:16-109,
 * paths relative to the reference repository) specialised to the
 * ReprojectionError<Geometry> terms Kalibr2 builds in CalibrateMultiCameraRig
 * (aslam_offline_calibration/kalibr2/include/kalibr2/CalibrationTools.hpp:376-428).
 *
 * Plain pointers and sizes only; every entry point returns an int status
 * (0 = OK, < 0 = error, message in kb_last_error()).  One handle per optimizer,
 * one HIP stream per handle, calls are not re-entrant (LinearSystemSolver is
 * single-threaded at the API level).
 *
 * State layout (flat doubles, also used by kb_set_state_flat / kb_get_state_flat):
 *   intr  [n_cams][KB_MAX_INTR]   projection params then distortion params
 *   base  [n_cams-1][7]           B_j = T_{c(j+1),c(j)}: JPL quaternion (x,y,z,w) + t
 *   frame [n_frames][7]           target pose DV T_f, p_c0 = T_f^-1 * P_target
 * Column order of dx / rhs (canonical): [intrinsics cam0..cam(N-1) | B_0..B_(N-2) | frame 0..F-1],
 * each pose block ordered (dphi[3], dt[3]) -- the DV insertion order of
 * CalibrateMultiCameraRig (q DV before t DV, CalibrationTools.hpp:32-45).
 */
#ifndef KALIBR_HIP_H
#define KALIBR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KB_MAX_INTR 10
#define KB_MAX_CAMS 16

/* camera models (kalibr2/include/kalibr2/CameraModels.hpp:25-133) */
enum kb_camera_model {
  KB_PINHOLE_RADTAN = 0, /* DistortedPinhole: fu fv cu cv | k1 k2 p1 p2 */
  KB_OMNI_RADTAN = 1,    /* DistortedOmni:    xi fu fv cu cv | k1 k2 p1 p2 */
  KB_EUCM = 2,           /* ExtendedUnified:  alpha beta fu fv cu cv */
  KB_OMNI = 3,           /* Omni:             xi fu fv cu cv */
  KB_DS = 4,             /* DoubleSphere:     xi alpha fu fv cu cv */
  KB_PINHOLE_EQUI = 5,   /* EquidistantPinhole: fu fv cu cv | k1 k2 k3 k4 */
  KB_PINHOLE_FOV = 6     /* FovPinhole:       fu fv cu cv | w */
};

typedef struct kb_handle kb_handle;

typedef struct kb_layout {
  int32_t n_cams;            /* N <= KB_MAX_CAMS */
  int32_t n_frames;          /* F (frames held by this handle / rank) */
  int32_t n_target;          /* target corners (120 for the 6x5 AprilGrid) */
  const int32_t* cam_model;  /* [n_cams] kb_camera_model */
  const double* target_points; /* [n_target][3] */
  int32_t device;            /* HIP device ordinal */
} kb_layout;

/* Replaces SparseCholeskyLinearSystemSolver construction
 * (aslam_backend/src/SparseCholeskyLinearSystemSolver.cpp:8-15). */
kb_handle* kb_create(const kb_layout* layout);
void kb_destroy(kb_handle* h);
const char* kb_last_error(void);

/* Replaces LinearSystemSolver::initMatrixStructure (LinearSystemSolver.cpp:117-138) for
 * ReprojectionError terms: one term per observed corner, grouped in views.
 * Views must be sorted by frame (then camera); one view per (frame, camera).
 *   y            [n_corners][2]  measured keypoints (invR = I, CalibrationTools.hpp:391-393, unless kb_set_corner_invR)
 *   corner_id    [n_corners]     target corner index of each term
 *   view_offsets [n_views+1]     corner range of each view
 *   view_frame   [n_views], view_cam [n_views] */
int kb_upload_observations(kb_handle* h, int32_t n_views, int32_t n_corners, const double* y,
                           const uint16_t* corner_id, const uint32_t* view_offsets,
                           const uint32_t* view_frame, const uint8_t* view_cam);

/* Design-variable values (the device owns the state between calls). */
int kb_set_state(kb_handle* h, const double* poses_q, const double* poses_t, const double* baselines,
                 const double* intrinsics);
int kb_set_state_flat(kb_handle* h, const double* state);
int kb_get_state_flat(kb_handle* h, double* state);
/* Diagnostics, read-only: the camera chains the device keeps beside a state buffer.  which = 0: of the current state,
 * 1: of the other buffer (the last candidate).  L_out [n_cams][12]: L_i = B_{i-1} .. B_0 as R (9, row-major) | t (3);
 * K_out [n_cams][n_cams][36]: K_{i,j}, 6 x 6 row-major, zero for j >= i.  Either pointer may be null. */
int kb_debug_chains(kb_handle* h, int which, double* L_out, double* K_out);
int kb_state_size(const kb_handle* h);
int kb_num_cols(const kb_handle* h);     /* JCols = C + 6F */
int kb_camera_cols(const kb_handle* h);  /* C = sum(intrinsics) + 6(N-1) */

/* LinearSystemSolver::evaluateError (LinearSystemSolver.cpp:81-92): chi^2 = sum e^T invR e; sum w(s) s on a weighted
 * handle (kb_set_mestimator / kb_set_corner_invR below). */
int kb_eval_cost(kb_handle* h, double* J_out);
/* LinearSystemSolver::buildSystem (SparseCholeskyLinearSystemSolver.cpp:39-46): J, rhs = -J^T e,
 * assembled as the arrow normal equations (no explicit J).  use_mestimator: 1 applies the M-estimator weights, 0 the
 * corner invR only (Optimizer2::computeHessian); the same system on an unweighted handle (Kalibr2's default:
 * NoMEstimator, invR = I). */
int kb_build(kb_handle* h, int use_mestimator);

/* Robust reprojection terms: ErrorTerm::setMEstimatorPolicy (aslam_backend/src/MEstimatorPolicies.cpp) and
 * ErrorTermFs::setInvR (aslam_backend/include/aslam/backend/implementation/ErrorTerm.hpp:118-127) for every term of an
 * unsharded camera handle.  A term has the raw squared error s = e^T invR e and the weight w = getWeight(s):
 *   KB_MEST_HUBER(k)              s < k^2 ? 1 : k / sqrt(s)             (MEstimatorPolicies.cpp:64-66)
 *   KB_MEST_CAUCHY(sigma^2)       1 / (1 + s / sigma^2)                 (:46-49)
 *   KB_MEST_GEMAN_MCCLURE(sigma^2) sigma^2 / (sigma^2 + s)^2            (:31-34)
 *   KB_MEST_BLAKE_ZISSERMAN(eps)  exp(-s) / (exp(-s) + eps)             (:104-106)
 * Cost (ErrorTerm.cpp:20-24): kb_eval_cost and the costs inside kb_optimize return sum w(s) s, always weighted.
 * Build (ErrorTerm.hpp(impl):170-192): the rows of a term are sqrt(w) sqrtInvR^T [J | e], so H = sum w J^T invR J and
 * rhs = -sum w J^T invR e; kb_build(h, 0) applies invR only (Optimizer2::computeHessian, Optimizer2.cpp:398-400),
 * kb_build(h, 1) and the device-resident loops both.  Only invR enters, not which square root: the Cholesky factor
 * is used.  Deviation from the reference: it evaluates w at the squared error cached by the last evaluateError; the
 * device evaluates w at the state it builds at (inside Optimizer2 the two coincide).
 * A handle with an estimator != NONE or an invR set is "weighted": kb_eval_cost, kb_build, everything that reads the
 * built blocks (kb_get_normal_blocks, kb_get_rhs, kb_rhs_jtj_rhs, kb_solve, kb_covariance), kb_apply_update /
 * kb_revert and kb_optimize with the LM and GN policies (GN through the general, non-fused pass) work on it; sharding
 * (kb_comm_init*), the marginal / incremental entry points, kb_append_frames / kb_drop_last_frames, the dog-leg
 * policy / kb_dogleg_step and the fused GN entry points (kb_run_gn_iterations, kb_gn_prepare, kb_gn_launch) return an
 * error until both settings are cleared.  An unweighted handle launches exactly the kernels it launched before.
 * kb_set_robust_build (below) opts a handle into the weighted k_buildp, which brings the fused GN pass and its entry
 * points back on a weighted handle. */
enum kb_mestimator_kind {
  KB_MEST_NONE = 0,
  KB_MEST_HUBER = 1,
  KB_MEST_CAUCHY = 2,
  KB_MEST_GEMAN_MCCLURE = 3,
  KB_MEST_BLAKE_ZISSERMAN = 4
};
typedef struct kb_mestimator {
  int32_t kind; /* KB_MEST_* */
  double param; /* k | sigma^2 | sigma^2 | epsilon; positive and finite */
} kb_mestimator;
/* m == NULL or kind NONE clears the estimator. */
int kb_set_mestimator(kb_handle* h, const kb_mestimator* m);
/* invR3: n symmetric 2x2 matrices as [a, b, c] = [[a, b], [b, c]], each positive definite (checked on the host).
 * n == 0 or NULL clears; n == 1 one matrix for every corner; n == n_corners one per corner in upload order.
 * The Cholesky factor (l00, l10, l11) of each matrix is stored on the device once. */
int kb_set_corner_invR(kb_handle* h, const double* invR3, int32_t n);
/* The build kernel of the handle while it is weighted.
 *   KB_ROBUST_BUILD_GENERAL (default)  k_build<.., WT> for every pass, GN through the general pass (as above).
 *   KB_ROBUST_BUILD_PIPE               the weighted k_buildp: kb_create's layout (frames per block, partial rows,
 *     threads, LDS) is kept, kb_build_kernel_name says k_buildp, and GN passes are fused again: kb_optimize with the
 *     GN policy, kb_run_gn_iterations, kb_gn_prepare and kb_gn_launch work (loop starts and the last step's cost stay
 *     weighted: k_cost_w / k_backsub_w).  Everything else that a weighted handle refuses stays refused.  Accepted only
 *     on an unsharded handle that kb_create gave k_buildp (4..8 cameras); otherwise an error naming the reason, the
 *     handle as it was.
 * The mode may be set before or after the estimator / invR and survives clearing them; an unweighted handle is not
 * affected by it. */
enum kb_robust_build { KB_ROBUST_BUILD_GENERAL = 0, KB_ROBUST_BUILD_PIPE = 1 };
int kb_set_robust_build(kb_handle* h, int32_t mode);
/* w and s of every term at the current state, upload order: w_out [n_corners], s_out [n_corners] or NULL. */
int kb_get_mestimator_weights(kb_handle* h, double* w_out, double* s_out);

/* LinearSystemSolver::setConstantConditioner (LinearSystemSolver.cpp:111-114):
 * "the square of this value will be added to the diagonal" (LinearSystemSolver.hpp:33-39). */
int kb_set_constant_conditioner(kb_handle* h, double diag);
/* LinearSystemSolver::setConditioner (LinearSystemSolver.cpp:98-102): diag[ncols] in the canonical column order;
 * its squares are added to the diagonal of the system kb_solve solves (until kb_set_constant_conditioner).
 * The direct solver only; the device-resident loop conditions with the trust-region lambda as before. */
int kb_set_conditioner(kb_handle* h, const double* diag);
/* LinearSystemSolver::solveSystem (SparseCholeskyLinearSystemSolver.cpp:48-89):
 * solves (J^T J + diag^2 I) dx = rhs.  *ok = 0 on a non-positive-definite system
 * (CHOLMOD failure semantics, Cholmod(impl).hpp:287-328); dx_out untouched then. */
int kb_solve(kb_handle* h, double* dx_out, int* ok);
/* IncrementalEstimator::addBatch on the device (aslam_incremental_calibration IncrementalEstimator.cpp:343-373,
 * 517-527): the reference re-runs initMatrixStructure over the grown problem on every batch; here the new frames are
 * appended to the uploaded handle in place.  kb_append_frames adds n_frames frames (their views sorted by frame,
 * view_frame counted from 0 within the appended block, view_offsets local: [n_views + 1] from 0 to n_corners) and
 * writes their poses ([n_frames][7], q xyzw | t) into the current state; the other design variables keep their
 * device values.  Device buffers grow geometrically and only the new observations cross PCIe, so appending F frames
 * one at a time moves O(F) data in total (the reference's re-initialisation: O(F^2)).  kb_drop_last_frames removes the
 * last n_frames frames with their views and corners (a rejected batch; at least one frame stays).  Captured graphs
 * and a kb_gn_prepare'd loop are voided.  Unsharded handles. */
int kb_append_frames(kb_handle* h, int32_t n_frames, int32_t n_views, int32_t n_corners, const double* y,
                     const uint16_t* corner_id, const uint32_t* view_offsets, const uint32_t* view_frame,
                     const uint8_t* view_cam, const double* frame_poses);
int kb_drop_last_frames(kb_handle* h, int32_t n_frames);

/* Linear solver behind kb_solve ("direct or PCG by mode").
 *   KB_SOLVER_SCHUR  (default) frame-block Schur complement + dense camera-block LDL^T: the exact solve that
 *                    replaces CHOLMOD (SparseCholeskyLinearSystemSolver.cpp:48-89); parity mode.
 *   KB_SOLVER_PCG    block-Jacobi preconditioned conjugate gradients on the full arrow system, as
 *                    sparse_block_matrix's LinearSolverPCG::solve
 *                    (sparse_block_matrix/include/sparse_block_matrix/implementation/linear_solver_pcg.hpp:58-130):
 *                    preconditioner = inverses of the diagonal design-variable blocks; stops when
 *                    r^T M^-1 r <= tolerance * r0^T M^-1 r0 (absolute mode: or <= the previous solve's _residual).
 *                    The reference always returns true; here *ok = 0 on a singular DV block or non-positive
 *                    curvature d^T A d.  One-GPU handles only (a sharded handle returns an error).
 *   KB_SOLVER_PCG_SCHUR  the frame blocks eliminated exactly (as KB_SOLVER_SCHUR), then the same block-Jacobi
 *                    PCG (same options, stopping rule and _residual semantics) on the C x C camera-block Schur
 *                    complement instead of its LDL^T, the frames back-substituted from that camera step.  One
 *                    block, ~1 us per iteration; a different iterate sequence than KB_SOLVER_PCG's full-system CG.
 *                    Sharded handles are supported: every rank runs the same PCG on the all-reduced S, b, so all
 *                    ranks hold bitwise-identical camera steps, iteration counts and _residual; each rank then
 *                    back-substitutes its own frames.  _residual (and kb_get_pcg_info) are updated only by a
 *                    completed solve: a failed one (*ok = 0) leaves the previous values for the next d0.
 * kb_optimize (LM, GN and dog-leg policies alike) and kb_dogleg_step always use the direct solve (the loop's passes
 * are captured graphs); the per-call path (kb_build / kb_solve / kb_apply_update, driven by the host Optimizer2) uses
 * the selected solver. */
enum kb_linear_solver { KB_SOLVER_SCHUR = 0, KB_SOLVER_PCG = 1, KB_SOLVER_PCG_SCHUR = 2 };
typedef struct kb_pcg_options {
  double tolerance;           /* _tolerance (LinearSolverPCG default 1e-6) */
  int32_t max_iterations;     /* _maxIter (-1: number of rows, the default) */
  int32_t absolute_tolerance; /* _absoluteTolerance (default 1) */
} kb_pcg_options;
typedef struct kb_pcg_info {
  int32_t iterations; /* PCG iterations of the last solve */
  double residual;    /* _residual = 0.5 r^T M^-1 r at exit */
  double d0;          /* stopping threshold used */
} kb_pcg_info;
/* selects the solver (pcg may be NULL: defaults); resets the PCG state as LinearSolverPCG::init() does */
int kb_set_linear_solver(kb_handle* h, int32_t kind, const kb_pcg_options* pcg);
/* LinearSolverPCG::init() (linear_solver_pcg.h:53-59): _residual = -1 */
int kb_pcg_init(kb_handle* h);
int kb_get_pcg_info(kb_handle* h, kb_pcg_info* info);

/* LinearSystemSolver::rhs (LinearSystemSolver.hpp:47). */
int kb_get_rhs(kb_handle* h, double* rhs_out);
/* LinearSystemSolver::rhsJtJrhs (LinearSystemSolver.hpp:66-69): rhs^T (J^T J) rhs of the last kb_build (the reference
 * forms ||J rhs||^2, SparseCholeskyLinearSystemSolver.cpp:106-111; DogLeg / steepest descent), on the device from
 * the arrow blocks.  Unsharded handles.  Fails unless the last system came from kb_build: the device-resident
 * loops (kb_optimize, kb_gn_*, kb_build_kernel_stats) overwrite or skip the per-call blocks it reads. */
int kb_rhs_jtj_rhs(kb_handle* h, double* out);
/* Optimizer::computeDiagonalCovariances / BlockCholeskyLinearSystemSolver::computeCovarianceBlocks
 * (aslam_backend/src/Optimizer2.cpp:365-402, BlockCholeskyLinearSystemSolver.cpp:122-148) on the device, from the arrow
 * structure: Sigma_cc = S^-1, Sigma_fc = -A_f Sigma_cc, Sigma_ff = (H_ff + D_f)^-1 + A_f Sigma_cc A_f^T.
 * blocks of (J^T J + D)^-1 of the last kb_build under the conditioner in force:
 * Pcc [C][C], Pff [F][6][6], Pfc [F][6][C] (any may be NULL), canonical column order.
 * *ok = 0 exactly when kb_solve would report 0 (outputs untouched then).
 * Always the direct factorisation (kb_set_linear_solver does not matter).  Unsharded handles, C <= 112.  Fails unless
 * the last system came from kb_build (as kb_rhs_jtj_rhs).  A query: state and system stay as after a kb_solve. */
int kb_covariance(kb_handle* h, double* Pcc, double* Pff, double* Pfc, int* ok);
/* CameraCalibrator::PrintReprojectionErrorStatistics (kalibr2/include/kalibr2/CameraCalibrator.hpp:368-411, called per
 * camera after the estimator by kalibr2_ros/src/CalibrateCameras.cpp:318) on the device, for every camera of the
 * handle at its current state: e = y - yhat of every term (ReprojectionError::getPredictedMeasurement), then
 * out[cam][6] = [n, mean_u, mean_v, std_u, std_v, rmse] with the sample standard deviation (N - 1; 0 when n < 2) of a
 * second pass about the mean, and the reference's "RMSE" = |sum e| / sqrt(n) (the norm of the error SUM, kept as the
 * reference prints it).  A camera without terms gets zeros.  Sharded handles sum over all ranks' frames. */
int kb_reprojection_error_stats(kb_handle* h, double* out);
/* Optimizer2::applyStateUpdate / revertLastStateUpdate (Optimizer2.cpp:290-318).
 * dx == NULL applies the device-resident dx of the last kb_solve. */
int kb_apply_update(kb_handle* h, const double* dx, double* deltaX_out);
int kb_revert(kb_handle* h);

/* aslam_incremental_calibration's LinearSolver (incremental_calibration/src/core/LinearSolver.cpp), the
 * linear solver of IncrementalEstimator's optimizer (IncrementalEstimator.cpp:46-66) and so of the CLI's final
 * calibration (CalibrateCameras.cpp:258-272).  Options: LinearSolverOptions (LinearSolverOptions.cpp:30-38). */
typedef struct kb_marginal_options {
  int32_t column_scaling; /* columnScaling (Kalibr2: 1) */
  double eps_norm;        /* epsNorm: column-norm tolerance sqrt(rows * epsNorm) (default DBL_EPSILON) */
  double eps_svd;         /* epsSVD: rankTol = sv_0 * epsSVD * C (Kalibr2: 1e-6) */
  double svd_tol;         /* svdTol: fixed tolerance, -1 = rankTol */
} kb_marginal_options;
typedef struct kb_marginal_info {
  int32_t rank;       /* getSVDRank (C - rank = getSVDRankDeficiency) */
  int32_t sweeps;     /* Jacobi sweeps used */
  double tolerance;   /* getSVDTolerance */
  double sv_gap;      /* getSvGap: sv[rank-1] / sv[rank], +inf at full rank */
  double sv_log2_sum; /* getSingularValuesLog2Sum over the first rank singular values */
} kb_marginal_info;
/* LinearSolver::solveSystem -> solve (LinearSolver.cpp:247-280, 299-466) after kb_build: the frame blocks are
 * eliminated (lambda = 0; the conditioner is ignored, as LinearSolver ignores it), the camera block Omega is
 * column-scaled and solved by truncated SVD, the frame steps back-substituted.  sv_out [C] (descending) and
 * V_out [C][C] (row-major, singular vector j in column j) are the scaled SVD (getSingularValues /
 * getMatrixV); either may be NULL.  *ok = 0 if a frame block is not positive definite.  C <= 112. */
int kb_solve_marginal(kb_handle* h, const kb_marginal_options* opts, double* dx_out, int* ok,
                      kb_marginal_info* info, double* sv_out, double* V_out);
/* LinearSolver::analyzeMarginal (LinearSolver.cpp:468-528): SVD of the unscaled Omega of the last kb_build.
 * info->rank / tolerance / sv_gap / sv_log2_sum are those of this SVD; the reference keeps the rank of the last
 * solve (the C++ host layer's MarginalLinearSolver does the same). */
int kb_analyze_marginal(kb_handle* h, const kb_marginal_options* opts, kb_marginal_info* info, double* sv_out,
                        double* V_out);

/* Normal-equation blocks of the last kb_build, for parity tests:
 * Hff [F][6][6], Hfc [F][6][C], gf [F][6], Hcc [C][C], gc [C], cost (chi^2 at build state).  Fails after a
 * device-resident loop until the next kb_build (as kb_rhs_jtj_rhs). */
int kb_get_normal_blocks(kb_handle* h, double* Hff, double* Hfc, double* gf, double* Hcc, double* gc,
                         double* cost);

/* Device-resident Optimizer2::optimize (Optimizer2.cpp:183-273) with the
 * LevenbergMarquardt (policy 0, LevenbergMarquardtTrustRegionPolicy.cpp:50-113),
 * GaussNewton (policy 1, GaussNewtonTrustRegionPolicy.cpp:18-39) or
 * DogLeg (policy 2, DogLegTrustRegionPolicy.cpp:11-161; options: kb_set_dogleg_options) trust-region policy.
 * The whole loop (build, Schur solve, update, cost, policy) runs as one hipGraph per
 * iteration; the host synchronises only every `sync_every` iterations.
 * Policy 2: a pass is the build at lambda = 0 that keeps the arrow blocks (only after an accepted step), the
 * steepest-descent reduction, the GN solve (only when the SD branch is not taken and no GN step of this system is
 * held), the step reductions and selection, dx = a g + b dx_gn, the update, the candidate's chains and cost, and the
 * policy kernel; a rejected step is followed by a pass that neither builds nor solves.  Unsharded handles only. */
typedef struct kb_optimizer_options {
  int32_t policy;          /* 0 = levenberg_marquardt, 1 = gauss_newton, 2 = dog_leg */
  double lambda_init;      /* LM lambdaInit (CalibrationTools.hpp:65: 10); unused for policies 1 and 2 */
  int32_t max_iterations;  /* Optimizer2Options::maxIterations */
  double convergence_dx;   /* convergenceDeltaX */
  double convergence_dj;   /* convergenceDeltaJ */
  int32_t sync_every;      /* host checks the done flag every n passes (0 = auto) */
  int32_t use_graph;       /* capture the iteration in a hipGraph (1) or launch eagerly (0) */
} kb_optimizer_options;

typedef struct kb_solution {
  double J_start, J_final, dx_final, dj_final; /* SolutionReturnValue (backend.hpp:11-24) */
  int32_t iterations, failed_iterations, linear_solver_failure;
  int32_t passes;
  int32_t graphed;         /* 1 if the passes ran as captured hipGraphs (RCCL calls included when sharded) */
} kb_solution;

int kb_optimize(kb_handle* h, const kb_optimizer_options* opts, kb_solution* out);

/* The IncrementalEstimator's optimisation device-resident (IncrementalEstimator.cpp:46-77, 373: Optimizer2 with the
 * GaussNewtonTrustRegionPolicy over calibration::LinearSolver): every pass builds with the frame blocks eliminated,
 * solves the camera block by the column-scaled truncated SVD of kb_solve_marginal, updates the design variables,
 * evaluates the cost and runs the policy (accept, convergence tests on convergence_dx / convergence_dj,
 * max_iterations) on the device; the passes run as captured graphs and the host polls the done flag every sync_every
 * passes.  opts->policy must be 1 (GN); opts->lambda_init is unused.  info / sv_out / V_out: the SVD of the last
 * solve (as kb_solve_marginal reports it; any may be NULL).  kb_analyze_marginal afterwards analyses the last
 * build, as analyzeMarginal after Optimizer2::optimize does.  Unsharded handles, C <= 112. */
int kb_optimize_marginal(kb_handle* h, const kb_optimizer_options* opts, const kb_marginal_options* mopts,
                         kb_solution* out, kb_marginal_info* info, double* sv_out, double* V_out);
/* kb_optimize_marginal followed by kb_analyze_marginal of the last build on the same stream, before the one host
 * sync that ends the loop (the IncrementalEstimator's optimize + analyzeMarginal pair, IncrementalEstimator.cpp:373,
 * 400): analyze_info / analyze_sv_out / analyze_V_out are what kb_analyze_marginal would return (any may be NULL). */
int kb_optimize_marginal_analyze(kb_handle* h, const kb_optimizer_options* opts, const kb_marginal_options* mopts,
                                 kb_solution* out, kb_marginal_info* info, double* sv_out, double* V_out,
                                 kb_marginal_info* analyze_info, double* analyze_sv_out, double* analyze_V_out);

/* Per-pass trace of the last kb_optimize: [J, lambda, deltaX, accepted] x n (returns count).  For policy 2 the
 * lambda column carries the trust radius delta the pass used. */
int kb_get_trace(kb_handle* h, double* trace, int32_t cap);

/* DogLegTrustRegionPolicy (aslam_backend/src/DogLegTrustRegionPolicy.cpp:11-161, include/aslam/backend/
 * DogLegTrustRegionPolicy.hpp) restated statement by statement: rho = get_dJ() / L0 and the radius update (:33-59),
 * rebuild + steepest descent only after an accepted step (:63-79), SD / GN / DL selection with beta of :118-131 and
 * L0 of :85, :112, :134 (the first term of :134 is multiplied by the integer expression 1/2 = 0 and is kept at 0).
 * Two deliberate deviations:
 *   1. Initial radius.  The reference starts at delta = 0 (:19), so the first step is always DL with beta = 1/2.
 *      delta_init (default 0: the reference) is what optimizationStarting assigns to delta.
 *   2. Failed linear solve.  The reference sets gnComputed before it knows the solve succeeded (:60, :94-99), so the
 *      iteration after a failed solve reads a _dx_gn it never computed.  Here the GN step counts as held only after a
 *      completed solve; a failed one is a failed iteration without a step and is retried on the next pass. */
typedef struct kb_dogleg_options {
  double delta_init; /* trust radius at optimizationStarting (0: the first-iteration rule of :105-107) */
} kb_dogleg_options;
/* options of policy 2 for the following kb_optimize calls; NULL selects the defaults */
int kb_set_dogleg_options(kb_handle* h, const kb_dogleg_options* opts);
typedef struct kb_dogleg_info {
  int32_t step_type; /* 0 SD, 1 GN, 2 DL (_stepType) */
  double delta;      /* the radius as used (delta == 0 in: the first-iteration radius) */
  double beta;       /* _beta (DL steps; 0 otherwise) */
  double sd_scale;   /* _sd_scale = |rhs|^2 / rhsJtJrhs */
  double dx_sd_norm; /* _dx_sd_norm */
  double dx_gn_norm; /* _dx_gn_norm; 0 if the GN step was not solved */
  double L0_over_J;  /* the model decrease _L0 over the cost J of the build state (GN: 1, DL: beta (2 - beta)) */
} kb_dogleg_info;
/* One solveSystemImplementation (:63-137) of the last kb_build for trust radius delta, on the device: the
 * steepest-descent reduction, the GN solve (lambda = 0, no conditioner, the direct factorisation; only when the SD
 * branch is not taken), the selection and the step dx_out [C + 6F] (may be NULL).  delta == 0 applies the
 * first-iteration rule (:105-107).  *ok = 0 exactly when a needed solve fails (dx_out untouched, info holds the SD
 * quantities).  A query like kb_solve: the state is untouched and the system stays as after a kb_solve.  Unsharded
 * handles.  Fails unless the last system came from kb_build (as kb_rhs_jtj_rhs). */
int kb_dogleg_step(kb_handle* h, double delta, double* dx_out, kb_dogleg_info* info, int* ok);
/* Per-pass dog-leg trace of the last kb_optimize with policy 2, aligned with kb_get_trace:
 * [delta, step_type (-1: failed solve), beta, L0, dx_sd_norm, dx_gn_norm] x n (returns count). */
int kb_get_dogleg_trace(kb_handle* h, double* out, int32_t cap);

/* Benchmark entry: run exactly n_iter Gauss-Newton passes of the device loop (convergence
 * tests disabled), no host sync inside; *seconds = wall time between stream syncs. */
int kb_run_gn_iterations(kb_handle* h, int32_t n_iter, double* seconds);
/* kb_run_gn_iterations in two calls, so that a multi-process run can put a host barrier between them:
 * kb_gn_prepare = the loop start (evaluateError on the current state, first prelude) + capture and upload of
 * every graph n_iter passes will launch, then a stream sync; kb_gn_launch = the n_iter passes and the last
 * pass's end between two stream syncs (*seconds = that wall time).  Same passes, same results.
 * kb_gn_prepare returns 1 when the passes will run as captured hipGraphs (RCCL calls included when sharded),
 * 0 when they run eagerly, < 0 on error.  Any call that changes the state, the control block or the graphs in
 * between (state setters, per-call entry points, kb_optimize, kb_comm_init, ...) voids the preparation:
 * kb_gn_launch then fails instead of running from a stale loop start. */
int kb_gn_prepare(kb_handle* h, int32_t n_iter);
int kb_gn_launch(kb_handle* h, int32_t n_iter, double* seconds);
/* Average device duration (ms) of the build kernel inside Gauss-Newton passes (runs 22 passes from the
 * current state, HIP events around each build launch on the handle's stream); algorithmic bytes per build launch and
 * the pass's algorithmic FP64 flops (projection + Jacobian, cost and local Hessian per corner, the
 * 6-D chain expansion per view, the Schur sums per frame; not the padded MFMA work the kernel executes).  The state,
 * camera chains and control block are restored afterwards. */
int kb_build_kernel_stats(kb_handle* h, double* avg_ms, double* bytes_per_launch, double* flops_per_launch);
/* Per-pass device timing of n Gauss-Newton passes from the current state (iteration 1 = the first pass after the
 * loop start): HIP events at every pass start and around every build kernel, captured in one graph with the passes,
 * on the handle's stream.  pass_ms [n] (pass r: from its start to the next pass's start), build_ms [n] (either may be
 * NULL).  A query: the state, camera chains and control block are restored afterwards.  Unsharded handles time the
 * graph; sharded ones run the passes eagerly. */
int kb_gn_pass_times(kb_handle* h, int32_t n, double* pass_ms, double* build_ms);
/* Name of the build kernel this handle launches ("k_buildp" or "k_build") into buf (NUL-terminated). */
int kb_build_kernel_name(kb_handle* h, char* buf, int32_t cap);
/* 1 when this handle's k_buildp launches carry the per-view table (each view's rigid transform and chain computed
 * once per block into LDS instead of once per frame by every lane), 0 when they do not: the handle builds with
 * k_build, the table does not fit the block's LDS at the current frame count, or KB_BUILDP_VIEWTAB=0 was set at
 * kb_create.  Read-only; the value can change with kb_append_frames / kb_drop_last_frames and the robust setters. */
int kb_build_viewtab(kb_handle* h);
/* 1 when this handle runs its fused Gauss-Newton passes in two launches per pass, the camera solve of pass i at the
 * head of pass i + 1's k_buildp (expanded partials, C > 64, one unweighted rank, a kernel family that has the
 * instantiation, a rig whose solve window fits the block's LDS); 0 when it keeps three launches per pass (sharded and
 * weighted handles, C <= 64, the other policies, or KB_GN_SOLVE_IN_BUILD=0 at kb_create).  Read-only; the value can
 * change with kb_append_frames / kb_drop_last_frames, the robust setters and kb_comm_init*. */
int kb_gn_solve_in_build(kb_handle* h);

/* Multi-GPU (frame sharding): each rank's handle holds its own frames;
 * the camera-block [S | b] and the cost/step statistics are all-reduced over RCCL once
 * per pass.  unique_id is the 128-byte ncclUniqueId. */
int kb_comm_get_unique_id(void* unique_id_out128);
int kb_comm_init(kb_handle* h, const void* unique_id128, int32_t nranks, int32_t rank);
/* In-process group: n handles of this process (any devices, one device included) become ranks 0..n-1 of one
 * sharded problem and exchange through device copies instead of RCCL (sums in rank order).  Each handle must
 * then be driven from its own host thread: the collectives of a pass meet in a host barrier (60 s timeout ->
 * error).  Passes run eagerly, not graph-captured.  Used to test the sharded path with several ranks on one GPU. */
int kb_comm_init_local(kb_handle* const* handles, int32_t n);
/* Direct all-reduce of the sharded camera-block image (C > 64, GN fused passes; replaces the collective of
 * LinearSystemSolver.cpp:81-92's host sum): kb_comm_init / kb_comm_init_local map every rank's exchange region (IPC
 * handles all-gathered over the communicator; the members' buffers in-process), self-test one exchange, and from then
 * on k_xar sums the ranks' partial images in rank order on every rank, reading the peers over xGMI -- no RCCL
 * collective for it, bitwise-identical images on all ranks.  KB_DIRECT_AR=0, a failed mapping or a failed self-test
 * (agreed over all ranks) keep the collective.  Returns 1 when the handle uses the direct path. */
int kb_comm_direct(const kb_handle* h);
/* The IPC half of the direct all-reduce on its own (test hook: RCCL refuses several ranks on one device, so the
 * multi-process mapping is tested with processes sharing one GPU).  kb_xar_export writes this handle's exchange-region
 * IPC handle (64 bytes); kb_xar_test maps the peers' regions from handles64 [nranks][64] (own slot ignored) and runs
 * the self-test exchange with them: *ok = 1 when every rank's known values arrived in rank-order sums, 0 when not or
 * when a peer did not take part within 2 s.  The handle stays unsharded.  C > 64 only. */
int kb_xar_export(kb_handle* h, void* handle_out64);
int kb_xar_test(kb_handle* h, int32_t nranks, int32_t rank, const void* handles64, int32_t* ok);

/* Self test of the f64 MFMA fragment layout used by the build kernel (A = I, asymmetric B). */
int kb_selftest_mfma(double* max_err);

/* ------------------------------------------------------------------------------------------------
 * Continuous-time calibration (configs[4]): the rig (IMU body b) on a B-spline pose trajectory
 * T_wb(t) (bsplines::BSplinePose with a RotationVector rotation, BSplinePose.cpp:21-41,384-412;
 * one DesignVariableMappedVector<6> per coefficient, BSplinePoseDesignVariable.cpp:9-19).
 *   camera terms  ReprojectionError at frame time t_f through T_ci_w = B_{i-1}..B_0 T_c0_b T_wb(t_f)^-1
 *                 (BSplineTransformationExpressionNode, BSplineExpressions.cpp:23-45)
 *   IMU terms     (not in the reference -- defined in DESIGN.md 10):
 *                 gyro  w_m = w_b(t) + b_g,  w_b = -C^T S(theta) theta_dot (BSplinePose.cpp:207-219)
 *                 accel a_m = C^T (p_ddot(t) - g_w) + b_a                  (cf. BSplinePose.cpp:175-180)
 *                 whitened by 1/sigma_gyro, 1/sigma_acc.
 *   robust terms  M-estimators on the reprojection, gyro and accelerometer terms and a corner invR
 *                 (kb_sp_set_mestimator / kb_sp_set_corner_invR, at the end of this block); without them every
 *                 corner has invR = I and every term the weight 1.
 * State:   intr [N][KB_MAX_INTR] | base [N-1][7] | T_c0_b [7] | b_g [3] | b_a [3] | g_w [3] | coeff [K][6]
 * Columns: [intr | B_j (dphi, dt) | T_c0_b (dphi, dt) | b_g | b_a | g_w | coeff 0..K-1 (6 each)]
 * Knot vector: non-decreasing, n_knots = K + order; the device path supports order 4 (cubic).
 * The coefficient block is solved by block cyclic reduction on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kb_sp_handle kb_sp_handle;

typedef struct kb_sp_layout {
  int32_t n_cams;
  int32_t n_target;
  const int32_t* cam_model;     /* [n_cams] */
  const double* target_points;  /* [n_target][3] */
  int32_t order;                /* 4 */
  int32_t n_knots;
  const double* knots;          /* [n_knots] */
  double sigma_gyro, sigma_acc; /* IMU noise (whitening) */
  int32_t device;
} kb_sp_layout;

kb_sp_handle* kb_sp_create(const kb_sp_layout* layout);
void kb_sp_destroy(kb_sp_handle* h);
/* initMatrixStructure for the spline problem: frames (times, views sorted by frame) and IMU samples.
 * All times inside the spline interval [knots[order-1], knots[n_knots-order]]. */
int kb_sp_upload(kb_sp_handle* h, int32_t n_frames, const double* frame_time, int32_t n_views, int32_t n_corners,
                 const double* y, const uint16_t* corner_id, const uint32_t* view_offsets,
                 const uint32_t* view_frame, const uint8_t* view_cam, int32_t n_imu, const double* imu_time,
                 const double* imu_gyro, const double* imu_acc);
int kb_sp_state_size(const kb_sp_handle* h);
int kb_sp_num_cols(const kb_sp_handle* h);
int kb_sp_camera_cols(const kb_sp_handle* h);
int kb_sp_set_state(kb_sp_handle* h, const double* state);
int kb_sp_get_state(kb_sp_handle* h, double* state);
/* evaluateError / buildSystem / setConstantConditioner / solveSystem / rhs / applyStateUpdate /
 * revertLastStateUpdate of the spline system, same semantics as the kb_* rig entry points. */
int kb_sp_eval_cost(kb_sp_handle* h, double* J_out);
int kb_sp_build(kb_sp_handle* h);
int kb_sp_set_constant_conditioner(kb_sp_handle* h, double diag);
/* BSplineMotionError (aslam_splines/include/aslam/backend/implementation/BSplineMotionError.hpp:29-160) on the pose
 * spline: cost c^T Q c with Q = curveQuadraticIntegralSparse(W, derivative_order) (bsplines/src/BSpline.cpp:
 * 1585-1622), added to evaluateError; buildSystem adds Q to the coefficient band and -Q c to the rhs (the
 * reference's buildHessianImplementation).  W [6][6] symmetric (row-major); derivative_order >= order is reduced to
 * order - 1 as the reference does; W == NULL removes the term. */
int kb_sp_set_motion_error(kb_sp_handle* h, const double* W, int32_t derivative_order);
/* ErrorTermEuclidean priors on the spline position: n terms ErrorTermEuclidean(bsp.position(times[k]), priors[k],
 * N[k]) (aslam_backend_expressions ErrorTermEuclidean.cpp:10-23,50-66 over BSplinePoseDesignVariable::position,
 * BSplinePoseDesignVariable.cpp:91-103): e = p(t_k) - prior_k, chi^2 = e^T N_k^-1 e, Jacobian w_j(t_k) [I_3 | 0] on the
 * active coefficients.  times [n] inside the spline interval, priors [n][3], N [n][3][3] symmetric positive definite
 * covariances (the reference's first constructor); n == 0 removes the terms. */
int kb_sp_set_position_priors(kb_sp_handle* h, int32_t n, const double* times, const double* priors, const double* N);
int kb_sp_solve(kb_sp_handle* h, double* dx_out, int* ok);
int kb_sp_get_rhs(kb_sp_handle* h, double* rhs_out);
int kb_sp_apply_update(kb_sp_handle* h, const double* dx, double* deltaX_out);
int kb_sp_revert(kb_sp_handle* h);
/* Normal equations of the last kb_sp_build (parity tests): Hcc [C][C], Hsc [6K][C], Hband [K][order][6][6]
 * (block (k, k+d)), gc [C], gs [6K], cost. */
int kb_sp_get_system(kb_sp_handle* h, double* Hcc, double* Hsc, double* Hband, double* gc, double* gs,
                     double* cost);
/* Optimizer::computeDiagonalCovariances / BlockCholeskyLinearSystemSolver::computeCovarianceBlocks
 * (aslam_backend/src/Optimizer2.cpp:365-402, BlockCholeskyLinearSystemSolver.cpp:122-148) for the spline system, on the
 * device: blocks of (H + lambda^2 I)^-1 of the last kb_sp_build under the conditioner in force, by the
 * selected inverse over the factors the default solve leaves in HBM (no dense inverse is formed):
 *   Ptt   [C][C]        Sigma_theta,theta (intrinsics, baselines, T_c0_b, IMU biases and gravity), exactly symmetric
 *   Pst   [6K][C]       Sigma_s,theta, the coefficients' rows against theta (may be NULL)
 *   Pband [K][4][6][6]  Sigma(c_k, c_k+d), d = 0..3, in kb_sp_get_system's Hband layout (zeros where k + d >= K; may be
 *                       NULL); blocks between coefficients further apart are not produced
 * *ok = 0 exactly when kb_sp_solve would report 0 (outputs untouched then).  A query: it runs kb_sp_solve's launches
 * first, so dx, the solved flag and the scalars are exactly as a kb_sp_solve under the same conditioner leaves them, and
 * the state is untouched.  It inverts the system kb_sp_build made: motion-error and prior terms are part of it, and so
 * are M-estimator weights and corner invR of a weighted handle (the reference's useMEstimator = false covariance is the
 * caller's to get, by clearing the estimators before the build).  Needs kb_sp_build.  A KSP_ZSF=0 handle returns the
 * bits of a default one: the query sums the camera block's Schur complement in one fixed order itself.
 * kb_sp_curve_covariance: the same pipeline, then P [n][6][6], the covariance of the curve value [p | rotation vector]
 * at times[q] (linear in its four active coefficients, weights of derivative 0 as kb_sp_upload evaluates them); a time
 * outside the spline interval is refused before any launch. */
int kb_sp_covariance(kb_sp_handle* h, double* Ptt, double* Pst, double* Pband, int* ok);
int kb_sp_curve_covariance(kb_sp_handle* h, int32_t n, const double* times, double* P, int* ok);
/* Optimizer2::optimize over the spline system (Optimizer2.cpp:183-273; LM policy 0, GN policy 1, DogLeg policy 2; any
 * other value runs as GN), host-driven loop over the device passes; trace as kb_get_trace.
 * Policy 2 (DogLegTrustRegionPolicy.cpp:11-161 as restated above kb_set_dogleg_options, both deviations included;
 * options: kb_sp_set_dogleg_options): a pass is the build (only after an accepted step) with the
 * steepest-descent reduction, the GN solve at lambda = 0 without any conditioner (only when the SD branch is not taken
 * and no GN step of this system is held) with the step dots, then dx = a g + b dx_gn, the update and the candidate's
 * cost, all on the device; the policy arithmetic runs on the host in double and only the scalar block is read back
 * (up to three times per pass).  A rejected step is followed by a pass that neither builds, reduces nor solves; a
 * failed solve is a failed iteration without a step.  g and H are what kb_sp_build made: robust weights, motion and
 * prior terms are part of them and of the cost.  The lambda column of kb_sp_get_trace carries delta. */
int kb_sp_optimize(kb_sp_handle* h, const kb_optimizer_options* opts, kb_solution* out);
int kb_sp_get_trace(kb_sp_handle* h, double* trace, int32_t cap);
/* LinearSystemSolver::rhsJtJrhs (LinearSystemSolver.hpp:66-69; SparseCholeskyLinearSystemSolver.cpp:106-111) of the
 * last kb_sp_build, on the device from the node blocks and the camera block: g^T H g with g = [g_theta | g_s] of
 * kb_sp_get_rhs and H of kb_sp_get_system (no conditioner).  Fails with "kb_sp_rhs_jtj_rhs: build first" otherwise. */
int kb_sp_rhs_jtj_rhs(kb_sp_handle* h, double* out);
/* options of policy 2 for the following kb_sp_optimize calls (kb_set_dogleg_options' struct and rules: delta_init is
 * what optimizationStarting, DogLegTrustRegionPolicy.cpp:11-22, assigns to delta); NULL selects the defaults */
int kb_sp_set_dogleg_options(kb_sp_handle* h, const kb_dogleg_options* opts);
/* One solveSystemImplementation (DogLegTrustRegionPolicy.cpp:63-137) of the last kb_sp_build for trust radius delta, as
 * kb_dogleg_step: the steepest-descent reduction (:70-75), the GN solve (:92-102; lambda = 0, no conditioner; only when
 * the SD branch of :82 is not taken), the selection and the step dx_out [C + 6K] (may be NULL).  delta == 0 applies the
 * first-iteration rule (:105-107); a negative or non-finite delta is refused.  *ok = 0 exactly when a needed solve
 * fails (dx_out untouched, info holds the SD quantities, step_type -1).  A query: the state is untouched; where it
 * solved, dx, the solved flag and the scalars are as a kb_sp_solve at lambda = 0 leaves them, where it did not they stay
 * as they were.  L0_over_J is relative to the build's cost.  Needs kb_sp_build. */
int kb_sp_dogleg_step(kb_sp_handle* h, double delta, double* dx_out, kb_dogleg_info* info, int* ok);
/* Per-pass dog-leg trace of the last kb_sp_optimize with policy 2 (empty after any other policy), aligned with
 * kb_sp_get_trace: [delta, step_type (-1: failed solve), beta, L0, dx_sd_norm, dx_gn_norm] x n (returns count)
 * (_delta, _stepType, _beta, _L0, _dx_sd_norm, _dx_gn_norm of DogLegTrustRegionPolicy.hpp). */
int kb_sp_get_dogleg_trace(kb_sp_handle* h, double* out, int32_t cap);
/* Benchmark: exactly n_iter GN passes (build + solve + update + cost), captured in a hipGraph. */
int kb_sp_run_gn_iterations(kb_sp_handle* h, int32_t n_iter, double* seconds);
/* Per-kernel device time (ms, HIP events on the handle's stream) of one GN pass, averaged over n passes:
 * out[0] frames kernel, [1] assemble, [2] cyclic reduction (all levels), [3] Schur + camera solve,
 * [4] update + cost, [5] whole pass; bytes[0] algorithmic bytes of the frames kernel per launch. */
int kb_sp_kernel_stats(kb_sp_handle* h, int32_t n, double* ms_out6, double* frames_bytes);
/* Device time (ms, HIP events around each launch on the handle's stream, averaged over n launches inside built
 * passes) and algorithmic bytes per launch of the node-assembly kernel (the pass's largest single launch). */
int kb_sp_assemble_stats(kb_sp_handle* h, int32_t n, double* ms, double* bytes);

/* Robust terms on the spline path: the semantics of kb_set_mestimator / kb_set_corner_invR above, per
 * term family.  A term has the raw squared error s and the weight w = getWeight(s) of its family's estimator:
 *   KB_SP_TERM_REPROJECTION  one term per corner,         s = e^T invR e
 *   KB_SP_TERM_GYRO          one 3-row term per IMU sample, s = |e_g|^2 of the whitened residual
 *   KB_SP_TERM_ACCEL         one 3-row term per IMU sample, s = |e_a|^2
 * The cost is sum w s over the three families (always weighted) plus the motion and prior costs, which take no
 * estimator (the priors keep their own invR); the rows of a term are sqrt(w) sqrtInvR^T [J | e], invR on corners only;
 * w is evaluated at the state that is linearised.  For KB_MEST_BLAKE_ZISSERMAN param is epsilon itself: the reference's
 * computeEpsilon needs the chi^2 quantile of the term's dimension, which has no closed form for the IMU families
 * (df = 3), so it is the caller's to compute.
 * A handle with any estimator != NONE or an invR set is "weighted": kb_sp_eval_cost, kb_sp_build, kb_sp_get_system,
 * kb_sp_get_rhs, kb_sp_solve, kb_sp_optimize (every policy), kb_sp_rhs_jtj_rhs, kb_sp_dogleg_step, kb_sp_run_gn_iterations, kb_sp_kernel_stats and
 * kb_sp_assemble_stats work on it through the same calls.  kb_sp_covariance inverts the weighted system as built: there is no
 * build without the estimator, so a covariance without it needs the estimators cleared first.  Every setter voids the built system and the captured GN pass; a refused call leaves the
 * handle as it was; a handle whose settings are all cleared launches exactly the kernels of a fresh one.
 * kb_sp_set_mestimator: before or after kb_sp_upload; m == NULL or kind NONE clears the family's estimator.
 * kb_sp_set_corner_invR: as kb_set_corner_invR (n == 0 or NULL clears, 1 one matrix for every corner, n_corners one per
 * corner in upload order, each positive definite); n == n_corners needs kb_sp_upload first.  kb_sp_upload is refused on
 * a handle that has observations, so a per-corner invR never outlives the corners it was given for.
 * kb_sp_get_mestimator_weights: w and s of every term of one family at the current state, upload order: [n_corners]
 * or [n_imu]; s_out may be NULL. */
enum kb_sp_term { KB_SP_TERM_REPROJECTION = 0, KB_SP_TERM_GYRO = 1, KB_SP_TERM_ACCEL = 2 };
int kb_sp_set_mestimator(kb_sp_handle* h, int32_t term, const kb_mestimator* m);
int kb_sp_set_corner_invR(kb_sp_handle* h, const double* invR3, int32_t n);
int kb_sp_get_mestimator_weights(kb_sp_handle* h, int32_t term, double* w_out, double* s_out);

#ifdef __cplusplus
}
#endif
#endif
