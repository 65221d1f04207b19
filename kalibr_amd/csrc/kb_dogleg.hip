// kb_dogleg.hip -- the dog-leg trust-region policy on the device, FP64 throughout.
//
// Restates aslam_backend's DogLegTrustRegionPolicy (aslam_optimizer/aslam_backend/src/DogLegTrustRegionPolicy.cpp:
// 11-161, driven by Optimizer2.cpp:183-273 and TrustRegionPolicy.cpp:29-52) statement by statement over the arrow
// system the build kernels leave (H_ff, H_fc, g_f per frame; H_cc, g_c):
//   prelude     rho = get_dJ() / L0, trust-radius update (:33-59), rebuild only after an accepted step (:63-79)
//   SD          sd_scale = g.g / g^T (J^T J) g, dx_sd = sd_scale g (:70-75)
//   selection   SD (:82-87) | GN (:109-114) | DL with beta of :118-131 (:115-136); the GN step is solved only when
//               the SD branch is not taken (:92-102)
// dx_sd is never materialised: with s = sd_scale, gg = g.g, n = dx_gn.dx_gn, p = g.dx_gn
//   |dx_sd|^2 = s^2 gg,  c = dx_sd.(dx_gn - dx_sd) = s p - s^2 gg,  |dx_gn - dx_sd|^2 = n - 2 s p + s^2 gg
// and every step is dx = a g + b dx_gn: SD (delta / |dx_sd| s, 0), GN (0, 1), DL ((1 - beta) s, beta).
//
// Deviations from the reference (also in include/kalibr_hip.h):
//   1. delta_init: optimizationStarting assigns it to delta (the reference: 0, the default here).
//   2. the GN step counts as held only after a completed solve (the reference sets gnComputed before it knows);
//      a failed solve is a failed iteration and is retried on the next pass.
//
// Every reduction has a fixed order (per-frame or per-block partials, then one block sums them in index order);
// no floating-point atomics.  The dog-leg state lives in KbDl, not in KbCtrl (the hot kernels copy KbCtrl whole).
// The kernels of the LM / GN passes that a dog-leg pass reuses (column sums, camera expansion, k_solve, k_backsub)
// are gated through two copies of the control block: `gb` (done unless this pass rebuilt the system) and `gs` (done
// unless this pass needs the GN solve), so a reused pass neither reduces nor solves again.
#include "kb_device.h"

namespace kb {

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

struct KbDlBuf {
  KbDl* s;
  KbCtrl* gb;       // control copy, done unless the pass rebuilt (column sums, camera expansion)
  KbCtrl* gs;       // control copy, done unless the pass solves (k_solve, k_backsub)
  double* sdpart;   // [F + C][2] per frame: g_f^T H_ff g_f + 2 g_f^T H_fc g_c | g_f.g_f, then per camera column r:
                    // g_r (H_cc g_c)_r | g_r^2
  double* dxgn;     // [C + 6F] the held GN step
  double* stepmax;  // [nstep] max |dx| per block of k_dl_step
  double* trace;    // [cap][6] per pass: delta, step type (-1: failed solve), beta, L0, |dx_sd|, |dx_gn|
  int nstep;
  int trace_cap;    // rows of trace
};

constexpr int kDlTrace = 6;

// sum of one value per thread over a 256-thread block, fixed order (wave sums, then the four waves in order)
__device__ __forceinline__ double dl_block_sum(double v, double* sh4) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// optimizationStartingImplementation (:11-22) after the loop start's generic prelude; delta = delta_init (deviation 1)
__global__ void k_dl_init(KbDev d, KbDlBuf b, double delta_init) {
  KbDl s{};
  s.delta = delta_init;
  s.delta_init = delta_init;
  s.step_type = -1;
  *b.s = s;
  *b.gb = *d.ctrl;
  b.gb->done = b.gb->done || !b.gb->do_build;
}

// steepest-descent reduction, one wave per row of the arrow system, lanes over C: rows 0 .. F - 1 are the frames,
// rows F .. F + C - 1 the camera columns (the clamped tail: waves beyond F + C leave)
__global__ void __launch_bounds__(256) k_dl_sd_frames(KbDev d, KbDlBuf b, int gate) {
  if (gate && (d.ctrl->done || !d.ctrl->do_build)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + wave;
  const int C = d.C;
  if (f >= d.F + C) return;
  if (f >= d.F) {  // camera column r: g_r (H_cc g_c)_r and g_r^2
    const int r = f - d.F;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s = fma(d.Hcc[(size_t)r * C + c], d.gc[c], s);
    s = wave_sum_d(s);
    if (lane == 0) {
      const double gr = d.gc[r];
      b.sdpart[2 * (size_t)f] = gr * s;
      b.sdpart[2 * (size_t)f + 1] = gr * gr;
    }
    return;
  }
  const double* gf = d.gf + (size_t)f * 6;
  double rf[6], q = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    rf[a] = gf[a];
    q = fma(rf[a], rf[a], q);
  }
  double s = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double rc = d.gc[c];
    double w = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) w = fma(rf[a], d.Hfc[((size_t)f * 6 + a) * C + c], w);
    s = fma(2.0 * w, rc, s);
  }
  if (lane < 36) s = fma(rf[lane / 6] * d.Hff[(size_t)f * 36 + lane], rf[lane % 6], s);
  s = wave_sum_d(s);
  if (lane == 0) {
    b.sdpart[2 * (size_t)f] = s;
    b.sdpart[2 * (size_t)f + 1] = q;
  }
}

// the rows in index order -> g.g, g^T H g, sd_scale, |dx_sd| (:70-75); then whether this pass
// needs the GN solve (:82, :92) and the solve's gate
__global__ void __launch_bounds__(256) k_dl_sd_final(KbDev d, KbDlBuf b, int gate) {
  __shared__ double sh[4];
  const int c_done = d.ctrl->done, c_build = d.ctrl->do_build;
  const int tid = threadIdx.x, C = d.C;
  if (gate && c_done) {
    if (tid == 0) *b.gs = *d.ctrl;
    return;
  }
  KbDl* s = b.s;
  if (!gate || c_build) {
    double h = 0.0, g = 0.0;
    const double2* sp = reinterpret_cast<const double2*>(b.sdpart);
    for (int f = tid; f < d.F + C; f += blockDim.x) {
      const double2 v = sp[f];
      h += v.x;
      g += v.y;
    }
    h = dl_block_sum(h, sh);
    g = dl_block_sum(g, sh);
    if (tid == 0) {
      s->gg = g;
      s->ghg = h;
      s->sd_scale = g / h;
      s->dx_sd_norm = fabs(s->sd_scale) * sqrt(g);
      s->gn_held = 0;  // "invalidate GN solution" (:78)
      s->gn2 = s->ggn = s->dx_gn_norm = 0.0;
    }
  }
  if (tid == 0) {
    const double delta = s->delta;
    const bool sd = s->dx_sd_norm >= delta && delta != 0;
    const int need = !sd && !s->gn_held;
    s->need_gn = need;
    if (gate) {
      *b.gs = *d.ctrl;
      b.gs->done = !need;
      b.gs->solve_ok = 1;
    }
  }
}

// step reductions (dx_gn.dx_gn, g.dx_gn from the per-frame rows and camera statistics k_backsub / k_solve left, in
// frame order) when the pass solved, then the one-thread selection (:82-137)
__global__ void __launch_bounds__(256) k_dl_select(KbDev d, KbDlBuf b, int gate) {
  __shared__ double sh[4];
  const KbCtrl cin = *d.ctrl;
  if (gate && cin.done) return;
  const int tid = threadIdx.x;
  KbDl* s = b.s;
  const int need = s->need_gn;  // block-uniform
  double n2 = 0.0, gp = 0.0;
  if (need) {
    const int sok = gate ? b.gs->solve_ok : cin.solve_ok;
    if (!sok) {  // deviation 2: no step, the GN step is not held
      if (tid == 0) s->step_ok = 0;
      return;
    }
    const double4* bp = reinterpret_cast<const double4*>(d.bpart);
    for (int f = tid; f < d.F; f += blockDim.x) {
      const double4 v = bp[f];
      n2 += v.z;
      gp += v.w;
    }
    n2 = dl_block_sum(n2, sh);
    gp = dl_block_sum(gp, sh);
  }
  if (tid != 0) return;
  if (need) {
    s->gn2 = n2 + d.camstat[1];
    s->ggn = gp + d.camstat[2];
    s->dx_gn_norm = sqrt(s->gn2);
    s->gn_held = 1;
  }
  const double J = gate ? cin.J : d.cost_build[0];
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

// dx = a g + b dx_gn over the C + 6F columns into the buffer the update reads; per-block max |dx|
__global__ void __launch_bounds__(256) k_dl_step(KbDev d, KbDlBuf b, int gate) {
  __shared__ double sh[4];
  if (gate && d.ctrl->done) return;
  const KbDl* s = b.s;
  if (!s->step_ok) return;
  const int type = s->step_type, C = d.C;
  const double a = s->a, bb = s->b;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0.0;
  if (i < d.ncols) {
    const double g = i < C ? d.gc[i] : d.gf[i - C];
    v = type == 0 ? a * g : (type == 1 ? b.dxgn[i] : a * g + bb * b.dxgn[i]);
    d.dx[i] = v;
  }
  v = wave_max_d(fabs(v));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) b.stepmax[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// the gated k_update_all: candidate design variables into state[1 - cur]
__global__ void __launch_bounds__(256) k_dl_update(KbDev d, KbDlBuf b) {
  if (d.ctrl->done || !b.s->step_ok) return;
  update_all_thread(d);
}

// camera chains of the candidate state (slot 1 - cur): the next build reads them if the step is accepted
__global__ void __launch_bounds__(256) k_dl_chains(KbDev d, KbDlBuf b) {
  if (d.ctrl->done || !b.s->step_ok) return;
  const int cand = 1 - d.ctrl->cur;
  chain_block(d, d.state + (size_t)cand * d.S + d.off_base, cand, blockDim.x);
}

// the gated k_cost on the candidate state
__global__ void __launch_bounds__(256) k_dl_cost(KbDev d, KbDlBuf b) {
  if (d.ctrl->done || !b.s->step_ok) return;
  cost_views_block(d, 1);
}

// pass end (Optimizer2.cpp:225-265: accept / revert, trace) and the next pass's prelude (while-condition :215-219,
// TrustRegionPolicy::solveSystem :39-52, the radius update and build-or-not of DogLegTrustRegionPolicy.cpp:33-79)
__global__ void __launch_bounds__(256) k_dl_policy(KbDev d, KbDlBuf b) {
  __shared__ double sh[256];
  const KbCtrl cin = *d.ctrl;
  if (cin.done) return;
  KbDl* s = b.s;
  const int ok = s->step_ok, tid = threadIdx.x;
  double J = 0.0, dX = 0.0;
  if (ok) {
    double a = 0.0, m = 0.0;
    for (int q = tid; q < d.nblk_cost; q += blockDim.x) a += d.costpart[q];
    for (int q = tid; q < b.nstep; q += blockDim.x) m = fmax(m, b.stepmax[q]);
    J = block_reduce(a, sh, false);
    dX = block_reduce(m, sh, true);
  }
  if (tid != 0) return;
  KbCtrl cl = cin;
  int accepted = 0;
  if (!ok) {
    cl.prev_failed = 1;
    cl.lin_fail = 1;
    cl.failed_iterations++;
    J = NAN;
    dX = cl.deltaX;
  } else {
    cl.deltaX = dX;
    cl.J = J;
    cl.deltaJ = cl.p_J - J;
    if (cl.deltaJ < 0.0) {  // revertOnFailure(): state[cur] untouched, J stays at the rejected candidate's cost
      cl.failed_iterations++;
      cl.prev_failed = 1;
    } else {
      cl.cur = 1 - cl.cur;
      cl.p_J = J;
      cl.prev_failed = 0;
      accepted = 1;
    }
    cl.iterations++;
  }
  if (cl.n_trace < d.trace_cap && cl.n_trace < b.trace_cap) {
    double* tr = d.trace + 4 * cl.n_trace;
    tr[0] = J;
    tr[1] = s->delta;  // the lambda column carries delta
    tr[2] = dX;
    tr[3] = accepted;
    double* t = b.trace + kDlTrace * cl.n_trace;
    t[0] = s->delta;
    t[1] = ok ? s->step_type : -1;
    t[2] = s->beta;
    t[3] = s->L0;
    t[4] = s->dx_sd_norm;
    t[5] = s->dx_gn_norm;
    cl.n_trace++;
  }
  cl.passes++;
  pol_pre<true>(&cl);  // while-condition and the base class's J bookkeeping (pol_J, pol_pJ)
  if (!cl.done) {
    const double rho = (cl.pol_pJ - cl.pol_J) / s->L0;  // get_dJ() / _L0
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
    cl.do_build = !cl.prev_failed;
  }
  cl.pending = 0;
  *d.ctrl = cl;
  cl.done = cl.done || !cl.do_build;
  *b.gb = cl;
}

}  // namespace kb
