// kb_robust.hip -- robust reprojection terms: M-estimator weights and the corner invR (kb_set_mestimator,
// kb_set_corner_invR).  Included by kb_kernels.hip (inside namespace kb) ahead of the kernels whose weighted
// instantiations use it: k_build<.., WT = true>, k_buildp<.., WT = true> (kb_set_robust_build), k_cost_w, k_backsub_w;
// k_rw_weights is the query kernel.
//
// Reference semantics restated (paths relative to the reference repository, aslam_optimizer/aslam_backend):
//   a term has the raw squared error s = e^T invR e = |sqrtInvR^T e|^2 (ErrorTerm.hpp(impl):156-161) and the weight
//   w = getWeight(s) (src/MEstimatorPolicies.cpp); its cost is w s (src/ErrorTerm.cpp:20-24) and its rows in the
//   system are sqrt(w) sqrtInvR^T [J | e] (ErrorTerm.hpp(impl):170-192).  Only invR = sqrtInvR sqrtInvR^T enters the
//   result; the lower Cholesky factor L = [[l00, 0], [l10, l11]] is the square root taken here, so
//   L^T e = (l00 e0 + l10 e1, l11 e1).
// The estimator kind and the invR mode are kernel arguments (wave-uniform branches); the per-corner factors are the
// only added loads (24 B per corner, rb_n > 1).

// getWeight(s) of estimator `kind` with parameter p: rb_weight (kb_math.h, shared with the spline path)

// Cholesky factor (l00, l10, l11) of a corner's invR
struct RbFac {
  double l00, l10, l11;
};
// the factor every corner shares (rb_n <= 1; the identity when no invR is set)
__device__ __forceinline__ RbFac rb_uniform(const KbDev& d) { return RbFac{d.rb_l[0], d.rb_l[1], d.rb_l[2]}; }
// the factor of corner k (k < NC)
__device__ __forceinline__ RbFac rb_load(const KbDev& d, int k) {
  const double* p = d.rb_L + 3 * (size_t)k;
  return RbFac{p[0], p[1], p[2]};
}

// s = |L^T e|^2 and w(s) of one term
__device__ __forceinline__ void rb_term(const KbDev& d, const RbFac& L, double e0, double e1, double& s, double& w) {
  const double t0 = L.l00 * e0 + L.l10 * e1, t1 = L.l11 * e1;
  s = t0 * t0 + t1 * t1;
  w = rb_weight(d.rb_kind, d.rb_param, s);
}

// the weighted chi^2 of one term, w(s) s.  s is formed as the unweighted cost kernels form e0^2 + e1^2,
// fma(e0, e0, e1 * e1) (cost_views_block, backsub_block): with the identity factor and no estimator t0 = e0, t1 = e1
// and w = 1 exactly, so the weighted cost kernels then return the bits of the unweighted ones (left to the compiler,
// the contraction of t0 * t0 + t1 * t1 rounded the other product and the sums differed in the last place)
__device__ __forceinline__ double rb_cost(const KbDev& d, const RbFac& L, double e0, double e1) {
  const double t0 = L.l00 * e0 + L.l10 * e1, t1 = L.l11 * e1;
  const double s = fma(t0, t0, t1 * t1);
  return rb_weight(d.rb_kind, d.rb_param, s) * s;
}
