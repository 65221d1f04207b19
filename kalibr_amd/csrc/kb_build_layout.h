// Launch layout of the build kernels (k_build / k_buildp) as plain integer arithmetic: frames per block, threads
// per block and dynamic LDS.  Host only and free of HIP, so the decisions that depend on it (does a rig fit, may a
// handle switch between the two kernels) are testable without a device.
#pragma once
#include <cstddef>

#include "kb_solve_layout.h"

namespace kb_blay {

constexpr int kXS = 17;            // kb_kernels.hip's XS (kb_capi.hip asserts that the two agree)
constexpr int kTargetLds = 1536;   // kb_kernels.hip's kTargetLds
constexpr int kBuildpMaxCams = 8;  // kb_kernels.hip's kBuildpMaxCams
constexpr int kMaxBuildThreads = 512;  // the build kernels' launch bound
constexpr size_t kLdsLimit = kb_slay::kLdsLimit;
constexpr size_t kBuildpStaticLds = 4096;  // k_buildp's static LDS (control copies, tables, counters), an upper bound

struct Rig {
  int N;    // cameras
  int C;    // camera-block columns
  int K;    // target corners
  int wpb;  // view waves per k_build block
  int bpc;  // k_buildp blocks per CU
};

// k_build's waves per camera (at least 4 waves per block) and per block
inline int nsplit(int N) { return (4 + N - 1) / N > 1 ? (4 + N - 1) / N : 1; }
inline int build_wpb(int N) { return N * nsplit(N); }
// a rig of N cameras fits a build block: at most 8 cameras
inline bool cams_fit(int N) { return 64 * build_wpb(N) <= kMaxBuildThreads; }
// kb_create's choice of the pipelined build (k_buildp: N view waves + the frame waves): one wave per camera
inline bool pipe_default(int N) { return nsplit(N) == 1 && N <= kBuildpMaxCams; }

// frames per build block for F frames
inline int gframes(bool pipe, int bpc, int F) { return pipe ? (F + 256 * bpc - 1) / (256 * bpc) : (F + 511) / 512; }

// k_buildp's frame waves
inline int frame_waves(int C) {
  return (kb_slay::ntiles(C) + 1) / 2 <= 5 ? 2 : 4;
}

// threads per build block
inline int build_threads(const Rig& r, bool pipe) { return 64 * (pipe ? r.N + frame_waves(r.C) : r.wpb); }

// dynamic LDS (bytes) of the build kernel at `gf` frames per block (the staged frame poses); *tg: k_buildp stages
// the target corners in LDS too
inline size_t build_lds(const Rig& r, bool pipe, int gf, int* tg_out) {
  const int N = r.N, C = r.C;
  const int CZ = 16 * kb_slay::nb(C);  // [Y | z] row stride of the Schur tiles
  const int tgl = (3 * r.K <= kTargetLds ? 3 * r.K : 0) + 8 * gf;
  if (pipe) {  // k_buildp: tiles | H | chains G | view outputs | frame sums | frame-wave buffers | K | target,
               // poses | the second view-output buffer
    const int np = N * (N - 1) / 2;
    const size_t vbs = 44 * N + 6 * CZ;  // view outputs dH | dg | intrinsic columns (+ the frame sums in place)
    const size_t base = N * 64 * kXS + N * 256 + N * 36 + 2 * vbs + 40 + 6 * CZ + 36 * np + 8 * gf;
    // the target corners are staged when they fit beside the rest
    const bool tg = 3 * r.K <= kTargetLds && sizeof(double) * (base + 3 * r.K) + kBuildpStaticLds <= kLdsLimit;
    if (tg_out) *tg_out = tg ? 1 : 0;
    return sizeof(double) * (base + (tg ? 3 * r.K : 0));
  }
  if (tg_out) *tg_out = 0;
  return sizeof(double) * (r.wpb * 64 * kXS + r.wpb * 256 + N * (256 + 256 + 64 + 36 + 36 + 8) + 36 + 16 * CZ +
                           18 * N * (N - 1) + tgl);
}

// the build kernel's LDS fits at F frames.  k_build always stages a target of 3 K <= kTargetLds doubles, k_buildp
// only when there is room: a rig that k_buildp takes can be too large for k_build (robust terms)
inline bool build_fits(const Rig& r, bool pipe, int F) {
  return build_lds(r, pipe, gframes(pipe, r.bpc, F), nullptr) + (pipe ? kBuildpStaticLds : 0) <= kLdsLimit;
}

// k_buildp's per-view table: one record per (frame of the block, camera) holding the view's
// rigid transform and chain, R (9) | t (3) | G (36, row-major), filled once per block and read by the view waves
// instead of being recomputed per frame.  It lies behind every other region of the dynamic LDS, so build_lds and
// build_fits do not know it: the launch asks for viewtab_total when viewtab_fits, else for build_lds as before.
// The record stride is odd in doubles: at 48 every lane of a one-view-per-lane store would hit the same bank pair.
constexpr int kViewtabRec = 48;
constexpr int kViewtabStride = 49;

// bytes of the table at `gf` frames per block
inline size_t viewtab_lds(const Rig& r, int gf) { return sizeof(double) * (size_t)kViewtabStride * gf * r.N; }

// dynamic LDS (bytes) of a k_buildp launch that carries the table
inline size_t viewtab_total(const Rig& r, int gf) { return build_lds(r, true, gf, nullptr) + viewtab_lds(r, gf); }

// the table fits beside the rest at F frames: dynamic and static LDS within a block's share of the CU (the whole
// LDS at one block per CU, half of it for the rigs that run two, which must stay co-resident)
inline bool viewtab_fits(const Rig& r, bool pipe, int F) {
  if (!pipe) return false;
  const int bpc = r.bpc > 1 ? r.bpc : 1;
  return viewtab_total(r, gframes(true, bpc, F)) + kBuildpStaticLds <= kLdsLimit / bpc;
}

// the table pays from two frames per block on: the fill and its barrier cost a block about what one frame's head
// gives back (0.4 us against 0.3 to 0.45 us per frame at configs[3], profiles/r16/), so a one-frame block only loses
constexpr int kViewtabMinFrames = 2;
inline bool viewtab_pays(int gf) { return gf >= kViewtabMinFrames; }

// The camera solve at the head of k_buildp (GN fused passes, expanded partials, C > 64: the SIB instantiations).  The
// solve window overlays the start of the build's dynamic LDS: [0, kSolveCarveBytes) the solve's arrays (SolveCarve:
// control block, dx_c, candidate intrinsics and chains; live until the build's prologue barrier), then
// solve_body<0>'s dynamic map (image, factored tiles, inverses; dead once the solve returns).  Regions of the build:
struct Region {
  size_t lo, hi;  // bytes of the dynamic LDS
};
inline bool overlap(const Region& a, const Region& b) { return a.lo < b.hi && b.lo < a.hi; }
// what is live ACROSS the solve (written before it, read after it): nothing -- the block issues its loads behind the solve
// what is live from the solve to the prologue barrier: the carve
inline Region solve_carve() { return {0, (size_t)kb_slay::kSolveCarveBytes}; }
inline Region solve_window(int N, int C) {
  return {0, (size_t)kb_slay::kSolveCarveBytes + kb_slay::lds_solve(N, C)};
}
// the view waves' tiles Xw, first written in the view loop, behind the prologue barrier
inline Region tiles_region(int N) { return {0, sizeof(double) * (size_t)N * 64 * kXS}; }
// what the prologue writes between the solve and its barrier while the carve is still read: the chain table K, the
// staged target and frame poses, and the per-view table when the launch carries it (all behind the tiles; the image
// part of the window below them is dead by then)
inline Region prologue_region(const Rig& r, int gf, bool vt) {
  const int CZ = 16 * kb_slay::nb(r.C);
  const size_t vbs = 44 * r.N + 6 * CZ;
  const size_t lo = sizeof(double) * ((size_t)r.N * 64 * kXS + r.N * 256 + r.N * 36 + vbs + 40 + 6 * CZ);
  return {lo, vt ? viewtab_total(r, gf) : build_lds(r, true, gf, nullptr)};
}
// dynamic LDS (bytes) of a SIB launch: the build's, or the window where that is larger
inline size_t sib_lds(const Rig& r, int gf, bool vt) {
  const size_t b = vt ? viewtab_total(r, gf) : build_lds(r, true, gf, nullptr);
  const size_t w = solve_window(r.N, r.C).hi;
  return b > w ? b : w;
}
// a rig takes the SIB kernel at F frames: C beyond the one-wave solves, the carve inside the tiles (so nothing the
// prologue writes touches it), and the whole within the block's share of the LDS (as viewtab_fits)
inline bool sib_fits(const Rig& r, int F, bool vt) {
  if (kb_slay::solve_cm(r.C) != 0 || !pipe_default(r.N)) return false;
  const int bpc = r.bpc > 1 ? r.bpc : 1;
  const int gf = gframes(true, bpc, F);
  if (solve_carve().hi > tiles_region(r.N).hi || overlap(solve_carve(), prologue_region(r, gf, vt))) return false;
  return sib_lds(r, gf, vt) + kBuildpStaticLds <= kLdsLimit / bpc;
}

// Robust terms (kb_set_mestimator / kb_set_corner_invR / kb_set_robust_build): the kernel a handle builds with.
// `pipe0` is kb_create's choice for the unweighted handle; a weighted handle keeps it only in pipe mode
// (KB_ROBUST_BUILD_PIPE: the weighted k_buildp), otherwise it builds with k_build.
inline bool robust_pipe(bool pipe0, bool pipe_mode, bool weighted) { return pipe0 && (!weighted || pipe_mode); }

// the build kernel of the handle in that robust state fits at F frames.  In pipe mode becoming weighted does not
// change the layout, so a rig that kb_create accepted is never refused
inline bool robust_fits(const Rig& r, bool pipe0, bool pipe_mode, bool weighted, int F) {
  return build_fits(r, robust_pipe(pipe0, pipe_mode, weighted), F);
}

}  // namespace kb_blay
