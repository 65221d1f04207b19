// kb_dogleg.hip -- the dog-leg trust-region policy on the device, FP64 throughout.
//
// The policy itself (aslam_backend's DogLegTrustRegionPolicy.cpp:11-161, driven by Optimizer2.cpp:183-273 and
// TrustRegionPolicy.cpp:29-52, its algebra without dx_sd and the two deviations from the reference) is kb_policy.h's:
// KbDl and dl_start, dl_set_sd, dl_sd_branch, dl_hold_gn, dl_select, dl_radius.  Here are the kernels that feed it over
// the arrow system the build kernels leave (H_ff, H_fc, g_f per frame; H_cc, g_c):
//   SD          the reduction of g.g and g^T (J^T J) g, then whether the pass needs the GN solve (solved only when the
//               SD branch is not taken, :92-102)
//   selection   the dot products of a fresh GN step, then dl_select; dx = a g + b dx_gn, update, chains, cost
//   pass end    accept / revert, trace, the next pass's prelude and radius update; rebuild only after an accepted step
//
// Every reduction has a fixed order (per-frame or per-block partials, then one block sums them in index order);
// no floating-point atomics.  The dog-leg state lives in KbDl, not in KbCtrl (the hot kernels copy KbCtrl whole).
// The kernels of the LM / GN passes that a dog-leg pass reuses (column sums, camera expansion, k_solve, k_backsub)
// are gated through two copies of the control block: `gb` (done unless this pass rebuilt the system) and `gs` (done
// unless this pass needs the GN solve), so a reused pass neither reduces nor solves again.
#include "kb_device.h"

namespace kb {

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
  dl_start(b.s, delta_init);
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
    if (tid == 0) dl_set_sd(s, g, h);
  }
  if (tid == 0) {
    const int need = !dl_sd_branch(s) && !s->gn_held;
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
  if (need) dl_hold_gn(s, n2 + d.camstat[1], gp + d.camstat[2]);
  dl_select(s, gate ? cin.J : d.cost_build[0]);
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
  const double red[4] = {J, 0.0, 0.0, dX};
  const KbPassEnd e = pol_accept<true>(&cl, ok, red);
  if (cl.n_trace < d.trace_cap && cl.n_trace < b.trace_cap) {
    double* tr = d.trace + 4 * cl.n_trace;
    tr[0] = e.J;
    tr[1] = s->delta;  // the lambda column carries delta
    tr[2] = e.dX;
    tr[3] = e.accepted;
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
    dl_radius(s, (cl.pol_pJ - cl.pol_J) / s->L0);  // get_dJ() / _L0
    cl.do_build = !cl.prev_failed;
  }
  cl.pending = 0;
  *d.ctrl = cl;
  cl.done = cl.done || !cl.do_build;
  *b.gb = cl;
}

}  // namespace kb
