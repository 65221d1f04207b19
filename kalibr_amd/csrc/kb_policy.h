// kb_policy.h -- the trust-region policies of the optimizer loop as plain arithmetic over two structs: the loop
// condition and the base class's J bookkeeping (Optimizer2.cpp:215-219, TrustRegionPolicy.cpp:29-52), the LM lambda
// schedule (LevenbergMarquardtTrustRegionPolicy.cpp:38-113), GN (GaussNewtonTrustRegionPolicy.cpp:25-29), accept /
// revert (Optimizer2.cpp:221-259) and the dog-leg policy (DogLegTrustRegionPolicy.cpp:11-161).  The device-resident
// loops (kb_kernels.hip, kb_dogleg.hip), the host-driven spline loops (kb_spline.hip, kb_spline_dogleg.hip) and the CPU
// test (tests/cpp/test_policy.cpp) all read it from here; reductions, gates, launches and trace stores stay with them.
// Free of HIP: it compiles under g++ and under hipcc, for host and device.
//
// Every function takes the struct by pointer and reads a field where the statement needs it: a field passed as a scalar
// is loaded before the short-circuit it sat behind, which changes the instruction streams of the kernels that inline
// pol_pre (every k_solve among them).  The text of a floating-point expression is part of the contract (operand order,
// the two-step `beta /= ...`): device code is compiled with contraction, host code without, and each side's bits follow
// from its expression trees.
//
// The dog-leg algebra never materialises dx_sd: with s = sd_scale, gg = g.g, n = dx_gn.dx_gn, p = g.dx_gn
//   |dx_sd|^2 = s^2 gg,  c = dx_sd.(dx_gn - dx_sd) = s p - s^2 gg,  |dx_gn - dx_sd|^2 = n - 2 s p + s^2 gg
// and every step is dx = a g + b dx_gn: SD (delta / |dx_sd| s, 0), GN (0, 1), DL ((1 - beta) s, beta).
//
// Deviations of the dog-leg policy from the reference (also in include/kalibr_hip.h):
//   1. delta_init: optimizationStarting assigns it to delta (the reference: 0, the default here).
//   2. the GN step counts as held only after a completed solve (the reference sets gnComputed before it knows);
//      a failed solve is a failed iteration and is retried on the next pass.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KB_HD __host__ __device__ inline
#else
#define KB_HD inline
#endif

namespace kb {

struct KbCtrl {
  int cur, done, do_build, solve_ok, first, prev_failed, lin_fail;
  int iterations, failed_iterations, max_iterations, policy, n_trace, passes;
  int pending;  // a pass ran its solve: its accept/revert + the next prelude are still to apply
  int have_dx;  // GN fused passes: the last solve's dx is still to apply (by the next build or the finish)
  int comm_err;  // k_xar: a peer rank did not arrive within the wait bound (the pass batch ends, the host fails the call)
  double J, p_J, J_start, deltaX, deltaJ, eps_x, eps_j;
  double pol_J, pol_pJ, last_succ, lambda, mu;
  double dxdx, dxrhs;
};

struct KbOpts {
  int policy, max_iterations;
  double lambda_init, eps_x, eps_j;
};

// the dog-leg state (not in KbCtrl: the hot kernels copy KbCtrl whole)
struct KbDl {
  double delta, p_delta, delta_init;
  double sd_scale, dx_sd_norm, dx_gn_norm, beta, L0;
  double gg, ghg;   // g.g and g^T (J^T J) g of the held system
  double gn2, ggn;  // dx_gn.dx_gn and g.dx_gn of the held GN step
  double dx_norm;   // |dx| of the last step (the 3 |dx| rule, :41)
  double a, b;      // dx = a g + b dx_gn
  double J;         // the cost L0 was formed with (per-call query: the build's chi^2)
  int step_type;    // 0 SD, 1 GN, 2 DL (of the last completed selection)
  int gn_held;      // dx_gn is the GN step of the held system
  int need_gn;      // this pass solves for it
  int step_ok;      // this pass has a step (0: the solve it needed failed)
};

constexpr int kDlTrace = 6;  // per pass: delta, step type (-1: failed solve), beta, L0, |dx_sd|, |dx_gn|

// ---------------------------------------------------------------------------------------------
// the loop: start, prelude of a pass, end of a pass
// ---------------------------------------------------------------------------------------------
// loop start from the cost J of the starting state: Optimizer2's counters, TrustRegionPolicy::optimizationStarting
// (TrustRegionPolicy.cpp:30-37), LM (:38-46).  `cur` stays as it is.
KB_HD void pol_start(KbCtrl* c, const KbOpts& o, double J) {
  c->J = J;
  c->p_J = J;
  c->J_start = J;
  c->deltaX = o.eps_x + 1.0;
  c->deltaJ = o.eps_j + 1.0;
  c->prev_failed = 0;
  c->lin_fail = 0;
  c->iterations = 0;
  c->failed_iterations = 0;
  c->max_iterations = o.max_iterations;
  c->eps_x = o.eps_x;
  c->eps_j = o.eps_j;
  c->policy = o.policy;
  c->pol_J = J;
  c->pol_pJ = J;
  c->last_succ = J;
  c->first = 1;
  c->lambda = o.policy == 0 ? o.lambda_init : 0.0;
  c->mu = 2.0;
  c->dxdx = 0.0;
  c->dxrhs = 0.0;
  c->done = 0;
  c->do_build = 0;
  c->solve_ok = 1;
  c->n_trace = 0;
  c->passes = 0;
  c->pending = 0;
  c->have_dx = 0;
  c->comm_err = 0;
}

// while-condition (Optimizer2.cpp:215-219) + TrustRegionPolicy::solveSystem prelude (TrustRegionPolicy.cpp:39-52) + LM
// lambda schedule (LevenbergMarquardtTrustRegionPolicy.cpp:50-84) or GN (build every pass, no conditioner:
// GaussNewtonTrustRegionPolicy.cpp:25-29).  d2() is getLmRho's denominator dx^T (lambda dx + rhs) (:107-113), asked for
// only where the schedule reads it: the caller forms it from what it holds of the last step.
template <bool GN_ONLY = false, class D2>
KB_HD void pol_pre(KbCtrl* c, D2 d2f) {
  const bool cont = c->iterations < c->max_iterations && c->failed_iterations < c->max_iterations &&
                    ((c->deltaX > c->eps_x && fabs(c->deltaJ) > c->eps_j) || c->lin_fail);
  if (!cont) {
    c->done = 1;
    return;
  }
  const double J = c->J;
  if (c->prev_failed) {
    c->pol_J = J;
  } else {
    c->pol_pJ = c->last_succ;
    c->last_succ = J;
    c->pol_J = J;
  }
  c->solve_ok = 1;
  if (!GN_ONLY && c->policy == 0) {
    if (c->first) {
      c->do_build = 1;
    } else {
      const double d2 = d2f();
      const double rho = (c->pol_pJ - c->pol_J) / d2;
      if (c->prev_failed) {
        c->mu *= 2;
        c->lambda *= c->mu;
        c->do_build = 0;
      } else if (rho <= 0) {
        c->mu *= 10;
        c->lambda *= c->mu;
        c->do_build = 0;
      } else {
        c->do_build = 1;
        if (c->lambda > 1e-16) {
          const double gamma = 3.0, beta = 2.0;
          const double u1 = 1 / gamma;
          const double u2 = 1 - (beta - 1) * pow((2 * rho - 1), 3.0);
          if (u1 > u2)
            c->lambda *= u1;
          else
            c->lambda *= u2;
          c->mu = beta;
        } else {
          c->lambda = 1e-15;
        }
      }
    }
  } else {
    c->do_build = 1;
  }
  c->first = 0;
}
// the denominator from the two sums of the last step that the control block carries
template <bool GN_ONLY = false>
KB_HD void pol_pre(KbCtrl* c) {
  pol_pre<GN_ONLY>(c, [c] { return c->lambda * c->dxdx + c->dxrhs; });
}

// what a pass end leaves for the trace: the candidate's cost (NaN: the solve failed), max |dx| and whether the
// candidate became the state
struct KbPassEnd {
  double J, dX;
  int accepted;
};

// accept / revert (Optimizer2.cpp:221-259) of a pass whose solve succeeded (ok) or not; red = [cost, dx.dx, dx.rhs,
// max|dx|] of the candidate.  LM reverts a regression, GN takes every step; DL: the dog-leg passes revert as LM does
// and carry no step sums.  The caller counts the pass (c->passes) once its trace row is written.
template <bool DL = false>
KB_HD KbPassEnd pol_accept(KbCtrl* c, bool ok, const double* red) {
  int accepted = 0;  // declared first: k_solve's instruction stream follows the order of these three
  double J = 0.0, dX = c->deltaX;
  if (!ok) {
    c->prev_failed = 1;
    c->lin_fail = 1;
    c->failed_iterations++;
    J = NAN;
  } else {
    J = red[0];
    dX = red[3];
    if (!DL) {
      c->dxdx = red[1];
      c->dxrhs = red[2];
    }
    c->deltaX = dX;
    c->J = J;
    c->deltaJ = c->p_J - J;
    if ((DL || c->policy == 0) && c->deltaJ < 0.0) {  // regression: revertLastStateUpdate (state[cur] untouched)
      c->failed_iterations++;
      c->prev_failed = 1;
    } else {
      c->cur = 1 - c->cur;
      c->p_J = J;
      c->prev_failed = 0;
      accepted = 1;
    }
    c->iterations++;
  }
  return {J, dX, accepted};
}

// ---------------------------------------------------------------------------------------------
// dog-leg (line numbers: DogLegTrustRegionPolicy.cpp)
// ---------------------------------------------------------------------------------------------
// optimizationStartingImplementation (:11-22); delta = delta_init (deviation 1)
KB_HD void dl_start(KbDl* s, double delta_init) {
  KbDl z{};
  z.delta = delta_init;
  z.delta_init = delta_init;
  z.step_type = -1;
  *s = z;
}

// a trust radius a caller may start from: finite and >= 0
KB_HD bool dl_delta_valid(double delta) { return delta >= 0.0 && std::isfinite(delta); }

// steepest descent of a rebuilt system from g.g and g^T (J^T J) g: sd_scale, |dx_sd| (:70-75), and "invalidate GN
// solution" (:78)
KB_HD void dl_set_sd(KbDl* s, double gg, double ghg) {
  s->gg = gg;
  s->ghg = ghg;
  s->sd_scale = gg / ghg;
  s->dx_sd_norm = fabs(s->sd_scale) * sqrt(gg);
  s->gn_held = 0;
  s->gn2 = s->ggn = s->dx_gn_norm = 0.0;
}

// the trust region is smaller than the SD step (:82): no GN step is needed
KB_HD bool dl_sd_branch(const KbDl* s) { return s->dx_sd_norm >= s->delta && s->delta != 0; }

// the GN step of the held system, after a completed solve (deviation 2): dx_gn.dx_gn and g.dx_gn
KB_HD void dl_hold_gn(KbDl* s, double gn2, double ggn) {
  s->gn2 = gn2;
  s->ggn = ggn;
  s->dx_gn_norm = sqrt(s->gn2);
  s->gn_held = 1;
}

// the selection (:82-137): SD (:82-87) | GN (:109-114) | DL with beta of :118-131 (:115-136); J is the cost L0 is
// formed with
KB_HD void dl_select(KbDl* s, double J) {
  const double sc = s->sd_scale, sdn = s->dx_sd_norm, gg = s->gg;
  double delta = s->delta;
  int type;
  double a, bb, L0, dxn;
  if (sdn >= delta && delta != 0) {  // trust region smaller than SD: the scaled SD step
    a = delta / sdn * sc;
    bb = 0.0;
    L0 = delta * (2 * sdn - delta) / (2 * sc);
    dxn = delta;
    type = 0;
  } else {
    const double gn2 = s->gn2, ggn = s->ggn, gnn = s->dx_gn_norm;
    // "set delta in the first step": |dx_sd + (dx_gn - dx_sd) / 2| (:105-107)
    if (delta == 0) delta = 0.5 * sqrt(sc * sc * gg + 2 * sc * ggn + gn2);
    if (gnn <= delta) {
      a = 0.0;
      bb = 1.0;
      L0 = J;
      dxn = gnn;
      type = 1;
    } else {
      const double dn2 = gn2 - 2 * sc * ggn + sc * sc * gg;  // |dx_gn - dx_sd|^2
      const double c = sc * ggn - sc * sc * gg;               // dx_sd.(dx_gn - dx_sd)
      const double r = delta * delta - sdn * sdn;
      double beta;
      if (c <= 0) {
        beta = -c + sqrt(c * c + dn2 * r);
        beta /= dn2;
      } else {
        beta = r;
        beta /= c + sqrt(c * c + dn2 * r);
      }
      s->beta = beta;
      a = (1 - beta) * sc;
      bb = beta;
      // the reference's first term carries the integer expression 1/2, which is 0 (:134): kept at 0
      L0 = beta * (2 - beta) * J;
      dxn = sqrt(a * a * gg + 2 * a * bb * ggn + bb * bb * gn2);
      type = 2;
    }
  }
  s->delta = delta;
  s->a = a;
  s->b = bb;
  s->L0 = L0;
  s->J = J;
  s->dx_norm = dxn;
  s->step_type = type;
  s->step_ok = 1;
}

// the trust-radius update at the head of the next pass (:33-59) from rho = get_dJ() / L0
KB_HD void dl_radius(KbDl* s, double rho) {
  double delta = s->delta;
  s->p_delta = delta;
  if (rho > 0.75) {  // step succeeded
    const double n3 = 3 * s->dx_norm;
    if (!(delta > n3)) delta = n3;
  } else if (rho > 0 && rho < 0.25) {  // step almost failed
    delta /= 2.0;
  } else if (rho <= 0) {  // step failed
    if (s->step_type == 1)
      delta = s->dx_gn_norm / 2.0;
    else
      delta /= 2.0;
  }
  s->delta = delta;
}

}  // namespace kb
