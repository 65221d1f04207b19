// kb_spline_dogleg.hip -- the dog-leg trust-region policy over the spline system, FP64 throughout.
// Included twice by kb_spline.hip (one translation unit: the kernels read SpDev, the host side the handle and its launch
// helpers): with KSP_DL_DEVICE after the path's kernels, with KSP_DL_HOST after its per-call entry points.
//
// The policy (aslam_backend DogLegTrustRegionPolicy.cpp:11-161 inside Optimizer2.cpp:183-273, the project's two deviations
// and the algebra that never materialises dx_sd: every step is dx = a g + b dx_gn) is kb_policy.h's, the functions the
// camera path's device-resident loop calls.  Here the loop is driven by the host like this path's LM and GN loops: the
// kernels reduce over the blocks k_sp_assemble / k_sp_reduce_cc left in HBM
//   g = [g_theta | g_s]: Hcc[C C ..) and column C of R0;  H: Hcc, R0[:, :C], D0, U0 (no conditioner, lambda^2 never added)
// and leave four scalars beside the SC_* ones; the policy runs on the host over a KbCtrl and a KbDl, and nothing but the
// scalar block crosses PCIe inside the loop.  No floating-point atomics; every sum has a fixed order (per-node or
// per-block partials in HBM, then one block over them in index order), so two runs from one state agree bitwise.

#ifdef KSP_DL_DEVICE
namespace ksp {

struct SpDl {
  double* sdpart;  // [n + C][2] per node: g_i^T D0_i g_i + 2 g_i^T U0_i g_(i+1) + 2 g_i^T R0_i[:, :C] g_theta | g_i.g_i;
                   // then per camera row r: g_r (H_cc g_theta)_r | g_r^2
  double* dpart;   // [ndots][2] per 256 columns: dx_gn.dx_gn | g.dx_gn
  double* dxgn;    // [C + 6K] the held GN step
  double* qdx;     // [C + 6K] kb_sp_dogleg_step's step (a query leaves dx as the solve left it)
  int ndots;
};

constexpr int kSpDlWaves = 4;  // nodes (waves) per k_sp_dl_sd block

__device__ __forceinline__ double sp_dl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum of one value per thread over a 256-thread block, fixed order (wave sums, then the four waves in order)
__device__ __forceinline__ double sp_dl_block_sum(double v, double* sh4) {
  v = sp_dl_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// g of column j of the system: theta columns from Hcc's g row, coefficient columns from column C of R0
__device__ __forceinline__ double sp_dl_g(const SpDev& d, int j) {
  const int C = d.C;
  if (j < C) return d.Hcc[(size_t)C * C + j];
  const int q = j - C;
  return d.R0[(size_t)(q / NB) * NB * d.m + (size_t)(q % NB) * d.m + C];
}

// Quadratic form and gradient norm, one wave per node (blocks [0, nb_nodes)) or per camera row (the blocks after
// them).  A node wave issues every global load it needs before the first use (one round: 6 + 6 entries of D0 / U0 per
// lane, 18 rows of R0[:, :C] with the lane as the column, g_i | g_(i+1) on lanes 0 .. 35, g_theta on the lanes' column),
// shares the three g vectors through LDS and sums in registers.  D0 is read by its upper triangle (diagonal once,
// the rest twice).  Padded slots of the last node and the node after the last one are masked to zero, not read.
__global__ void __launch_bounds__(64 * kSpDlWaves) k_sp_dl_sd(SpDev d, SpDl b, int nb_nodes) {
  __shared__ double sg[kSpDlWaves][2 * NB + MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = d.C, m = d.m, n = d.n;
  if ((int)blockIdx.x >= nb_nodes) {  // camera row r: g_r (H_cc g_theta)_r and g_r^2
    const int r = ((int)blockIdx.x - nb_nodes) * kSpDlWaves + wave;
    if (r >= C) return;
    const int c = lane < C ? lane : 0;
    const double hv = d.Hcc[(size_t)r * C + c], gv = d.Hcc[(size_t)C * C + c], gr = d.Hcc[(size_t)C * C + r];
    const double s = sp_dl_wave_sum(lane < C ? hv * gv : 0.0);
    if (lane == 0) {
      b.sdpart[2 * (size_t)(n + r)] = gr * s;
      b.sdpart[2 * (size_t)(n + r) + 1] = gr * gr;
    }
    return;
  }
  const int i0 = (int)blockIdx.x * kSpDlWaves + wave;
  const bool act = i0 < n;
  const int i = act ? i0 : n - 1;  // a wave beyond the last node loads node n - 1 again and stores nothing
  const double* Di = d.D0 + (size_t)i * NB * NB;
  const double* Ui = d.U0 + (size_t)i * NB * NB;
  const double* Ri = d.R0 + (size_t)i * NB * m;
  // ---- the load round
  double gl = 0.0;  // lanes 0 .. 17: g_i, lanes 18 .. 35: g_(i+1)
  {
    const int r = lane < NB ? lane : lane - NB, node = lane < NB ? i : i + 1;
    const bool real = lane < 2 * NB && node < n && SB * node + r / 6 < d.K;
    const double* p = d.R0 + (size_t)(real ? node : i) * NB * m + (size_t)(real ? r : 0) * m + C;
    const double v = *p;
    gl = real ? v : 0.0;
  }
  const int cc = lane < C ? lane : 0;
  const double gt = d.Hcc[(size_t)C * C + cc];
  double dv[6], uv[6], rv[NB];
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const int q = lane + 64 * u, qc = q < NB * NB ? q : 0;
    dv[u] = Di[qc];
    uv[u] = Ui[qc];
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) rv[r] = Ri[(size_t)r * m + cc];
  // ---- g through LDS
  double* g = sg[wave];
  if (lane < 2 * NB) g[lane] = gl;
  g[2 * NB + lane] = lane < C ? gt : 0.0;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const int q = lane + 64 * u;
    if (q < NB * NB) {
      const int r = q / NB, c = q % NB;
      const double w = c == r ? 1.0 : (c > r ? 2.0 : 0.0);
      s = fma(w * g[r] * dv[u], g[c], s);
      s = fma(2.0 * g[r] * uv[u], g[NB + c], s);
    }
  }
  double t = 0.0;
#pragma unroll
  for (int r = 0; r < NB; ++r) t = fma(g[r], rv[r], t);
  s = fma(2.0 * t, g[2 * NB + lane], s);  // g_theta is zero on the lanes beyond C
  s = sp_dl_wave_sum(s);
  const double q2 = sp_dl_wave_sum(lane < NB ? gl * gl : 0.0);
  if (act && lane == 0) {
    b.sdpart[2 * (size_t)i] = s;
    b.sdpart[2 * (size_t)i + 1] = q2;
  }
}

// the partial pairs in index order -> out[0], out[1] (one block)
__global__ void __launch_bounds__(256) k_sp_dl_sum(const double* part, int cnt, double* out) {
  __shared__ double sh[4];
  const double2* p = reinterpret_cast<const double2*>(part);
  double a = 0.0, c = 0.0;
  for (int q = threadIdx.x; q < cnt; q += 256) {
    const double2 v = p[q];
    a += v.x;
    c += v.y;
  }
  a = sp_dl_block_sum(a, sh);
  c = sp_dl_block_sum(c, sh);
  if (threadIdx.x == 0) {
    out[0] = a;
    out[1] = c;
  }
}

// step dots after the GN solve at lambda = 0 (dx holds dx_gn): per 256 columns dx_gn.dx_gn | g.dx_gn, and dx_gn into
// the held buffer.  A failed solve leaves no step to hold.
__global__ void __launch_bounds__(256) k_sp_dl_dots(SpDev d, SpDl b) {
  __shared__ double sh[4];
  if (d.sc[SC_OK] == 0.0) return;
  const int j = blockIdx.x * 256 + threadIdx.x, ncols = d.C + 6 * d.K;
  double x = 0.0, g = 0.0;
  if (j < ncols) {
    x = d.dx[j];
    g = sp_dl_g(d, j);
    b.dxgn[j] = x;
  }
  const double n2 = sp_dl_block_sum(x * x, sh);
  const double gp = sp_dl_block_sum(g * x, sh);
  if (threadIdx.x == 0) {
    b.dpart[2 * (size_t)blockIdx.x] = n2;
    b.dpart[2 * (size_t)blockIdx.x + 1] = gp;
  }
}

// Step and update, one block per node as k_sp_update: dx = a g + b dx_gn (type 0 SD: a g; 1 GN: dx_gn; 2 DL) of the
// node's 18 columns -> out, with the theta columns on block 0; with `apply` the state update by k_sp_update's rules
// (backup copy, additive coefficients, theta DVs); per-block max |dx| -> dmax (summed up by k_sp_cost_reduce).
__global__ void __launch_bounds__(64) k_sp_dl_step(SpDev d, SpDl b, double* out, double a, double bb, int type, int apply) {
  __shared__ double sdx[MAXC];
  const int i = blockIdx.x, tid = threadIdx.x, C = d.C;
  auto step = [&](int j) {
    const double g = sp_dl_g(d, j);
    return type == 0 ? a * g : (type == 1 ? b.dxgn[j] : a * g + bb * b.dxgn[j]);
  };
  double mx = 0.0;
  if (tid < NB) {
    const int k = SB * i + tid / 6;
    if (k < d.K) {
      const int j = C + 6 * k + tid % 6;
      const double v = step(j);
      out[j] = v;
      mx = fabs(v);
      const int o = d.off_coef + 6 * k + tid % 6;
      if (apply) {
        d.backup[o] = d.state[o];
        d.state[o] += v;
      }
    }
  }
  if (i == 0) {
    if (tid < C) {
      const double v = step(tid);
      out[tid] = v;
      sdx[tid] = v;
      mx = fmax(mx, fabs(v));
    }
    if (apply) {
      for (int q = tid; q < d.off_coef; q += 64) d.backup[q] = d.state[q];
      __syncthreads();
      if (tid < C) {
        const int kind = d.ckind[tid], idx = d.cidx[tid], sub = d.csub[tid];
        if (kind == 0) d.state[idx * KB_MAX_INTR + sub] += sdx[tid];
        if (kind == 2) d.state[d.off_imu + sub] += sdx[tid];
      }
      if (tid < d.N) {  // pose DVs q = tid: B_q (q < N-1) or T_c0_b
        const int q = tid;
        double* pose = d.state + (q < d.N - 1 ? d.off_base + 7 * q : d.off_cb);
        double np[7];
        kb::update_pose(pose, sdx + d.col_pose[q], np);
#pragma unroll
        for (int k = 0; k < 7; ++k) pose[k] = np[k];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if (tid == 0) d.dmax[i] = mx;
}

}  // namespace ksp
#endif  // KSP_DL_DEVICE

#ifdef KSP_DL_HOST
// ==================================================================================================
// host side
// ==================================================================================================
namespace {
// the buffers of the policy, made by the first call that needs them
int sp_dl_ensure(kb_sp_handle* h) {
  if (h->dl_ready) return 0;
  SpDl& b = h->dl;
  b.ndots = (h->ncols + 255) / 256;
  if (h->alloc(&b.sdpart, 2 * (size_t)(h->n + h->C)) || h->alloc(&b.dpart, 2 * (size_t)b.ndots) ||
      h->alloc(&b.dxgn, (size_t)h->ncols) || h->alloc(&b.qdx, (size_t)h->ncols))
    return -1;
  h->dl_ready = true;
  return 0;
}

// steepest-descent reduction of the built system -> sc[SC_GHG], sc[SC_GG] (the order of sdpart's pairs)
void sp_dl_launch_sd(kb_sp_handle* h) {
  const SpDev& d = h->d;
  const int nbn = (d.n + kSpDlWaves - 1) / kSpDlWaves, nbc = (d.C + kSpDlWaves - 1) / kSpDlWaves;
  static_assert(SC_GG == SC_GHG + 1 && SC_GGN == SC_GN2 + 1, "k_sp_dl_sum writes a pair");
  hipLaunchKernelGGL(k_sp_dl_sd, dim3(nbn + nbc), dim3(64 * kSpDlWaves), 0, h->stream, d, h->dl, nbn);
  hipLaunchKernelGGL(k_sp_dl_sum, dim3(1), dim3(256), 0, h->stream, h->dl.sdpart, d.n + d.C, d.sc + SC_GHG);
}

// the GN step of the built system: kb_sp_solve's launches at lambda = 0 (no conditioner), then the step dots ->
// sc[SC_GN2], sc[SC_GGN] and the held copy of dx_gn
int sp_dl_launch_gn(kb_sp_handle* h) {
  const SpDev& d = h->d;
  hipLaunchKernelGGL(k_sp_set_lam, dim3(1), dim3(64), 0, h->stream, d, 0.0);
  if (launch_solve(h)) return -1;
  hipLaunchKernelGGL(k_sp_update, dim3(d.n), dim3(64), 0, h->stream, d, 0);
  hipLaunchKernelGGL(k_sp_dl_dots, dim3(h->dl.ndots), dim3(256), 0, h->stream, d, h->dl);
  hipLaunchKernelGGL(k_sp_dl_sum, dim3(1), dim3(256), 0, h->stream, h->dl.dpart, h->dl.ndots, d.sc + SC_GN2);
  return 0;
}

// kb_sp_optimize, policy 2.  Per pass: [build, SD reduction, read-back] only after an accepted step; [GN solve, step
// dots, read-back] only when the SD branch is not taken and no GN step of this system is held; step + update + cost,
// read-back.  A pass after a rejected step launches the step, the update and the cost kernels alone.  The pass end and
// the next pass's prelude are k_dl_policy's statements (kb_dogleg.hip) on the host.
int sp_dl_optimize(kb_sp_handle* h, const kb_optimizer_options* o, kb_solution* out) {
  KSP_HIP(hipSetDevice(h->device));
  if (sp_dl_ensure(h)) return -1;
  SpDev& d = h->d;
  double J;
  if (kb_sp_eval_cost(h, &J)) return -1;
  kb::KbCtrl c{};
  kb::pol_start(&c, kb::KbOpts{2, o->max_iterations, 0.0, o->convergence_dx, o->convergence_dj}, J);
  kb::KbDl s;
  kb::dl_start(&s, h->dl_opts.delta_init);
  h->dl_pass_ms.clear();
  for (kb::pol_pre<true>(&c); !c.done;) {
    const auto t_pass = std::chrono::steady_clock::now();
    if (c.do_build) {  // rebuild + steepest descent only after an accepted step (:63-79)
      if (launch_build(h)) return -1;
      sp_dl_launch_sd(h);
      KSP_HIP(hipGetLastError());
      if (read_scalars(h)) return -1;
      kb::dl_set_sd(&s, h->host_sc[SC_GG], h->host_sc[SC_GHG]);
    }
    bool ok = true;
    if (!kb::dl_sd_branch(&s) && !s.gn_held) {
      if (sp_dl_launch_gn(h)) return -1;
      KSP_HIP(hipGetLastError());
      if (read_scalars(h)) return -1;
      ok = h->host_sc[SC_OK] != 0.0;
      if (ok) kb::dl_hold_gn(&s, h->host_sc[SC_GN2], h->host_sc[SC_GGN]);
    }
    double red[4] = {0.0, 0.0, 0.0, 0.0};  // cost and max |dx| of the candidate
    if (ok) {  // (not ok: deviation 2, a failed iteration without a step, retried on the next pass)
      kb::dl_select(&s, c.J);
      hipLaunchKernelGGL(k_sp_dl_step, dim3(d.n), dim3(64), 0, h->stream, d, h->dl, d.dx, s.a, s.b, s.step_type, 1);
      if (launch_cost(h, 1)) return -1;
      KSP_HIP(hipGetLastError());
      if (read_scalars(h)) return -1;
      red[0] = h->host_sc[SC_COST];
      red[3] = h->host_sc[SC_DX];
    }
    const kb::KbPassEnd e = kb::pol_accept<true>(&c, ok, red);
    if (ok && !e.accepted)  // revertLastStateUpdate; the next pass keeps the system and the GN step
      hipLaunchKernelGGL(k_sp_revert, dim3((h->S + 255) / 256), dim3(256), 0, h->stream, d);
    h->trace.push_back(e.J);
    h->trace.push_back(s.delta);  // the lambda column carries delta
    h->trace.push_back(e.dX);
    h->trace.push_back(e.accepted);
    const double t[kb::kDlTrace] = {s.delta, ok ? (double)s.step_type : -1.0, s.beta, s.L0, s.dx_sd_norm, s.dx_gn_norm};
    h->dl_trace.insert(h->dl_trace.end(), t, t + kb::kDlTrace);
    c.passes++;
    kb::pol_pre<true>(&c);
    if (!c.done) {
      kb::dl_radius(&s, (c.pol_pJ - c.pol_J) / s.L0);  // get_dJ() / _L0
      c.do_build = !c.prev_failed;
    }
    h->dl_pass_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pass).count());
  }
  KSP_HIP(hipStreamSynchronize(h->stream));
  h->built = h->solved = false;
  sp_fill_solution(c, out);
  return 0;
}
}  // namespace

extern "C" {

int kb_sp_rhs_jtj_rhs(kb_sp_handle* h, double* out) {
  if (!h || !out) return fail("kb_sp_rhs_jtj_rhs: null");
  if (!h->built) return fail("kb_sp_rhs_jtj_rhs: build first");
  KSP_HIP(hipSetDevice(h->device));
  if (sp_dl_ensure(h)) return -1;
  sp_dl_launch_sd(h);
  KSP_HIP(hipGetLastError());
  if (read_scalars(h)) return -1;
  *out = h->host_sc[SC_GHG];
  return 0;
}

int kb_sp_set_dogleg_options(kb_sp_handle* h, const kb_dogleg_options* opts) {
  if (!h) return fail("kb_sp_set_dogleg_options: null");
  const kb_dogleg_options def{0.0};
  const kb_dogleg_options o = opts ? *opts : def;
  if (!kb::dl_delta_valid(o.delta_init))
    return fail("kb_sp_set_dogleg_options: delta_init must be finite and >= 0");
  h->dl_opts = o;
  return 0;
}

int kb_sp_dogleg_step(kb_sp_handle* h, double delta, double* dx_out, kb_dogleg_info* info, int* ok) {
  if (!h || !ok) return fail("kb_sp_dogleg_step: null");
  if (!h->built) return fail("kb_sp_dogleg_step: build first");
  if (!kb::dl_delta_valid(delta)) return fail("kb_sp_dogleg_step: delta must be finite and >= 0");
  KSP_HIP(hipSetDevice(h->device));
  if (sp_dl_ensure(h)) return -1;
  kb::KbDl s;
  kb::dl_start(&s, delta);
  sp_dl_launch_sd(h);
  KSP_HIP(hipGetLastError());
  if (read_scalars(h)) return -1;
  kb::dl_set_sd(&s, h->host_sc[SC_GG], h->host_sc[SC_GHG]);
  const double J = h->host_sc[SC_COST_BUILD];
  auto fill = [&](bool stepped) {
    if (!info) return;
    info->step_type = stepped ? s.step_type : -1;
    info->delta = s.delta;
    info->beta = s.beta;
    info->sd_scale = s.sd_scale;
    info->dx_sd_norm = s.dx_sd_norm;
    info->dx_gn_norm = s.dx_gn_norm;
    info->L0_over_J = stepped ? s.L0 / J : 0.0;
  };
  if (!kb::dl_sd_branch(&s)) {  // the GN step: dx, the solved flag and the scalars as a kb_sp_solve at lambda = 0 leaves them
    if (sp_dl_launch_gn(h)) return -1;
    KSP_HIP(hipGetLastError());
    if (read_scalars(h)) return -1;
    h->solved = h->host_sc[SC_OK] != 0.0;
    if (!h->solved) {
      *ok = 0;
      fill(false);
      return 0;
    }
    kb::dl_hold_gn(&s, h->host_sc[SC_GN2], h->host_sc[SC_GGN]);
  }
  kb::dl_select(&s, J);
  // the step into the query's own buffer; dmax is the one thing of a solve it rewrites (the next solve writes it again)
  hipLaunchKernelGGL(k_sp_dl_step, dim3(h->d.n), dim3(64), 0, h->stream, h->d, h->dl, h->dl.qdx, s.a, s.b, s.step_type, 0);
  KSP_HIP(hipGetLastError());
  if (dx_out)
    KSP_HIP(hipMemcpyAsync(dx_out, h->dl.qdx, sizeof(double) * h->ncols, hipMemcpyDeviceToHost, h->stream));
  KSP_HIP(hipStreamSynchronize(h->stream));
  *ok = 1;
  fill(true);
  return 0;
}

int kb_sp_get_dogleg_trace(kb_sp_handle* h, double* out, int32_t cap) {
  if (!h || !out) return fail("kb_sp_get_dogleg_trace: null");
  const int n = std::min<int>(cap, (int)(h->dl_trace.size() / kb::kDlTrace));
  if (n > 0) std::memcpy(out, h->dl_trace.data(), sizeof(double) * kb::kDlTrace * n);
  return n;
}

}  // extern "C"

// diagnostics only (tools/sp_dogleg_time.py): host wall time of each pass of the last policy 2 run, read-backs included
extern "C" int kb_sp_diag_dogleg_pass_ms(kb_sp_handle* h, double* out, int n) {
  if (!h || !out) return fail("kb_sp_diag_dogleg_pass_ms: null");
  n = std::min<int>(n, (int)h->dl_pass_ms.size());
  if (n > 0) std::memcpy(out, h->dl_pass_ms.data(), sizeof(double) * n);
  return n;
}
#endif  // KSP_DL_HOST
