// Launch layout of the reduced-system kernels (k_schur, k_colimg / k_colsumx / k_xar, k_camexpand, k_solve, k_cov_cam,
// k_cov_frames, k_marg) as plain integer arithmetic: which instance runs at a camera-block width C, with how many
// threads, and how its dynamic LDS is carved.  The host (kb_capi.hip), the kernels (kb_kernels.hip) and the CPU test
// (tests/cpp/test_solve_layout.cpp) all read it from here, so a size the host asks for cannot drift from the carve of
// the kernel it launches.  Free of HIP: it compiles under g++ and under hipcc, for host and device.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KB_SLAY_HD __host__ __device__
#else
#define KB_SLAY_HD
#endif

namespace kb_slay {

// ---- the limits
constexpr int kMaxC = 111;                // widest camera block a handle admits: nb(C) <= 7 tile rows of [Y | z]
constexpr size_t kLdsLimit = 160 * 1024;  // LDS of a workgroup, static + dynamic
constexpr int kTS = 17;                   // tile row stride (doubles): 16 + 1 keeps row-parallel LDS accesses conflict-free
constexpr int kTileSz = 16 * kTS;
constexpr int kXMaxRanks = 64;            // per-rank max|dx_f| slots of the image's aux area
constexpr int kCovWaves = 4, kCovFrames = 2 * kCovWaves;  // k_cov_frames: waves per block, two frames per wave
constexpr int kCovMaxC = 112;             // capacity of k_cov_cam<0>'s 1/D array
constexpr int kMargMaxC = 112;            // capacity of k_marg's per-column arrays
constexpr int kMargThreads = 1024;
constexpr int kMargLdsStage = 19000;  // dynamic LDS doubles up to which k_marg stages V0 in LDS too
constexpr int kChainLdsBytes = 7680;  // sizeof(ChainLds) (kb_kernels.hip asserts it beside the struct)
constexpr int kSolveCarveBytes = 16768;  // >= sizeof(SolveCarve), a multiple of 16 (kb_kernels.hip asserts both)
static_assert(kMaxC <= kCovMaxC && kMaxC <= kMargMaxC, "the array capacities hold every admitted width");

// ---- the selectors
// tile rows of the camera block with the appended b row (rows 0 .. C): k_schur's nbz and CZ / 16 as well.  A shift,
// not a division: the kernels' instruction streams depend on it.  The kernels that multiply it out themselves (CZ, n16)
// take the macro: a function is inlined only after the compiler's first instruction-combining pass, which then folds
// 16 * nb differently and changes their instruction streams (k_build, k_buildp, k_schur, k_colimg, k_colsumx)
#define KB_SLAY_NB(C) (((C) + 16) >> 4)
KB_SLAY_HD constexpr int nb(int C) { return KB_SLAY_NB(C); }
// lower 16 x 16 tiles of nb(C) tile rows
KB_SLAY_HD constexpr int ntiles(int C) { return nb(C) * (nb(C) + 1) / 2; }
// CM of k_solve<CM> / k_cov_cam<CM>: the one-wave register LDL^T on the packed S for C <= CM; 0: the tile image and
// the blocked factorisation
KB_SLAY_HD constexpr int solve_cm(int C) { return C <= 16 ? 16 : C <= 24 ? 24 : C <= 32 ? 32 : C <= 48 ? 48 : C <= 64 ? 64 : 0; }
// threads of k_solve and k_cov_cam
KB_SLAY_HD constexpr int solve_threads(int C) { return solve_cm(C) ? 256 : 512; }
// TW of k_schur<TW>: Schur-sum tiles per wave, ceil(lower tiles of [Y | z]^T [Y | z] / 4 waves) in buckets
KB_SLAY_HD constexpr int schur_ms(int C) { return (ntiles(C) + 3) / 4 <= 1 ? 1 : (ntiles(C) + 3) / 4 <= 4 ? 4 : 7; }
// k_cov_frames: column tiles and k-steps of the zero-padded operands
struct CovFrames {
  int nct, nks;
};
KB_SLAY_HD constexpr CovFrames cov_frames(int C) { return {(C + 15) >> 4, (C + 3) >> 2}; }

// ---- the k_solve image (C > 64; written by k_colimg or k_colsumx, summed over ranks by k_xar, staged by
// solve_body<0> and k_cov_cam<0>): [lower 16 x 16 tiles, stride kTS, b as row C | aux].  Aux slots: g_c [0, C) |
// non-PD frame-block count at C | cost at img_n16 | max|dx_f| of rank r at img_n16 + 1 + r | pad
// tile doubles = the aux offset (the macro: for k_colimg and k_colsumx, as KB_SLAY_NB)
#define KB_SLAY_NTZ(nb) (kb_slay::kTileSz * (nb) * ((nb) + 1) / 2)
KB_SLAY_HD constexpr int img_ntz(int C) { return KB_SLAY_NTZ(nb(C)); }
KB_SLAY_HD constexpr int img_n16(int C) { return 16 * nb(C); }
KB_SLAY_HD constexpr int img_n(int C) { return img_ntz(C) + img_n16(C) + 2 + kXMaxRanks; }

// ---- the trailing updates of the blocked LDL^T (ldl_panels, C > 64), left-looking: while panel q >= 1 is factored,
// the update waves bring column q + 1 up to date with the panels 0 .. q - 1, so that phase A of panel q + 1 (panel q
// on column q + 1) completes it.  An item is one tile product: panel p subtracted from tile (i, q + 1).  Update slot
// ow of the phase's ns slots takes the tiles i = q + 1 + ow + ns u and walks each through p = 0 .. q - 1 before the
// next, so a tile's products stay on one wave and arrive in panel order.  The slots are waves off the SIMDs that
// factor: 2, 3, 6, 7 (SIMDs 2, 3) while panel q has two factor waves (waves 0 and 1: more than four tiles below it),
// and wave 5 as well once wave 0 factors alone and SIMD 1 is free (three tiles then sit on three SIMDs).  ldl_panels
// steps with upd_first / upd_next and takes two items per round; the CPU test walks the same functions
KB_SLAY_HD constexpr int factor_waves(int nb, int q) { return nb - 1 - q > 4 ? 2 : 1; }  // four tiles below per wave
KB_SLAY_HD constexpr int upd_slots(int nb, int q) { return factor_waves(nb, q) == 2 ? 4 : 5; }
// the slot of block wave `wave` at panel q, or -1
KB_SLAY_HD constexpr int upd_slot(int nb, int q, int wave) {
  if (upd_slots(nb, q) == 4) return wave == 2 ? 0 : wave == 3 ? 1 : wave == 6 ? 2 : wave == 7 ? 3 : -1;
  return wave == 2 ? 0 : wave == 3 ? 1 : wave == 5 ? 2 : wave == 6 ? 3 : wave == 7 ? 4 : -1;
}
// One tile is brought forward: the last diagonal tile (nb - 1, nb - 1) would take all its nb - 2 products on one wave
// in phase B of panel nb - 2, longer than that panel's factor.  Slot 2, idle in phase B of panel nb - 3 (two tiles in
// column nb - 2), applies the panels 0 .. nb - 4 to it there; phase B of panel nb - 2 adds panel nb - 3 alone.
struct UpdItem {
  int i, j, p;  // tile (i, j) (done: i >= nb) | panel
};
KB_SLAY_HD constexpr UpdItem upd_first(int nb, int q, int ow) {
  if (q == nb - 3 && ow == 2) return {nb - 1, nb - 1, 0};
  return {q + 1 + ow, q + 1, (q == nb - 2 && ow == 0) ? q - 1 : 0};
}
KB_SLAY_HD constexpr UpdItem upd_next(UpdItem a, int nb, int q, int ns) {
  if (a.p + 1 < q) return {a.i, a.j, a.p + 1};
  return a.j == q + 1 ? UpdItem{a.i + ns, a.j, 0} : UpdItem{nb, a.j, 0};
}

// ---- the dynamic LDS of solve_body<CM> (k_solve) and k_cov_cam<CM>
//   packed (CM > 0): S column-major packed lower [C(C+1)/2] | bv [C + 1] (slot C: non-PD count) | gl [C] |
//     Hs [N][256] | T [N][N][36] | K [N][N][36] | ci [C] ints
//   image (CM == 0): the image's tiles | its aux area from bv (= gl) on | Dfac [nb][kTileSz] factored diagonal tiles |
//     Xinv [nb][kTileSz] their unit-lower inverses | rDv [16 nb] 1/D | ci [C] ints.  Dfac starts behind rank 0's
//     max|dx_f| slot: the image is staged whole, and the slots of the further ranks are read before the factorisation
//     writes Dfac.
// KB_SLAY_SOLVE_MAP states both, once, and declares the ten regions as P S, bv, gl, Hs, T, K, Dfac, Xinv, rDv, cip (ci's
// place).  The kernels expand it with P = double* and the start of their dynamic LDS; solve_map expands it with
// P = int and 0 for the offsets in doubles (host, tests).  A macro, because the kernels' address arithmetic has to
// reach the compiler as these very sums: behind a function it is combined only after inlining, in another order, and
// k_solve<CM> and k_cov_cam<CM> come out with other instruction streams and registers
#define KB_SLAY_SOLVE_MAP_(P, sm, PACKED, N, C, GL)                                                         \
  P S = (sm);                                                                                               \
  P bv = S + ((PACKED) ? (C) * ((C) + 1) / 2 : KB_SLAY_NTZ(KB_SLAY_NB(C)));                                 \
  P Hs = (PACKED) ? bv + 2 * (C) + 1 : bv;                                                                  \
  GL                                                                                                        \
  P T = (PACKED) ? Hs + (N) * 256 : bv;                                                                     \
  P K = T + (N) * (N) * 36;                                                                                 \
  P Dfac = (PACKED) ? K + (N) * (N) * 36 : bv + ((16 * KB_SLAY_NB(C) + 2 + 1) & ~1);                        \
  P Xinv = Dfac + ((PACKED) ? 0 : KB_SLAY_NB(C) * kb_slay::kTileSz);                                        \
  P rDv = Xinv + ((PACKED) ? 0 : KB_SLAY_NB(C) * kb_slay::kTileSz);                                         \
  P cip = rDv + ((PACKED) ? 0 : 16 * KB_SLAY_NB(C));
#define KB_SLAY_SOLVE_MAP(P, sm, PACKED, N, C) \
  KB_SLAY_SOLVE_MAP_(P, sm, PACKED, N, C, P gl = (PACKED) ? bv + (C) + 1 : bv;)
// k_cov_cam never reads gl, and even a dead declaration moves the compiler's common subexpressions (other registers)
#define KB_SLAY_SOLVE_MAP_NO_GL(P, sm, PACKED, N, C) KB_SLAY_SOLVE_MAP_(P, sm, PACKED, N, C, )
struct SolveMap {
  int S, bv, gl, Hs, T, K, Dfac, Xinv, rDv, ci;
};
template <bool PACKED>
KB_SLAY_HD constexpr SolveMap solve_map(int N, int C) {
  KB_SLAY_SOLVE_MAP(int, 0, PACKED, N, C)
  return {S, bv, gl, Hs, T, K, Dfac, Xinv, rDv, cip};
}
// bytes: packed, up to the end of ci; image, the whole image (its per-rank slots included) and Dfac, Xinv, rDv, ci
KB_SLAY_HD constexpr size_t lds_solve(int N, int C) {
  return solve_cm(C) > 0 ? sizeof(double) * solve_map<true>(N, C).ci + sizeof(int) * C
                         : sizeof(double) * (img_n(C) + 2 + 2 * nb(C) * kTileSz + img_n16(C)) + sizeof(int) * C;
}
// k_cov_cam keeps one more packed triangle E [C(C+1)/2] (L or its inverse): behind the solve's layout (packed), or
// from Xinv on (image: the tiles, the aux area and the factored diagonal tiles stay)
KB_SLAY_HD constexpr int cov_eoff(int N, int C) {
  return solve_cm(C) > 0 ? (int)((lds_solve(N, C) + 15) / 16) * 2 : solve_map<false>(N, C).Xinv;
}
KB_SLAY_HD constexpr size_t lds_cov_cam(int N, int C) {
  const size_t e = sizeof(double) * ((size_t)cov_eoff(N, C) + (size_t)C * (C + 1) / 2);
  return e > lds_solve(N, C) ? e : lds_solve(N, C);
}

// ---- the other dynamic sizes (bytes)
KB_SLAY_HD constexpr size_t lds_schur(int C) { return sizeof(double) * 16 * 16 * nb(C); }  // P, Q [8][CZ]: [H_fc | g_f], [A | b]
KB_SLAY_HD constexpr size_t lds_camexp(int N) { return sizeof(double) * (N * 256 + N * N * 36); }
// k_colimg's staging (C > 64 only): Hs [N][256] | K, T [N][N][36] | ci [C] ints
KB_SLAY_HD constexpr size_t lds_colimg(int N, int C) {
  return solve_cm(C) > 0 ? 0 : sizeof(double) * (N * 256 + 2 * N * N * 36) + sizeof(int) * C;
}
// k_cov_frames: Sigma_cc [C][C] | one product tile row [16][16 nct + 1] per wave
KB_SLAY_HD constexpr size_t lds_cov_frames(int C) {
  return sizeof(double) * ((size_t)C * C + (size_t)kCovWaves * 16 * (16 * cov_frames(C).nct + 1));
}

// ---- k_marg.  Full storage (both triangles of Omega, C padded to even m, V [C][m]) while it fits, else packed upper
// Omega and V [C][C]; then G, b_s, and V0 (the warm start) when it fits beside them
KB_SLAY_HD constexpr bool marg_full(int C) {
  const int m = C + (C & 1);
  return m * m + C * m + 2 * C <= kMargLdsStage;
}
KB_SLAY_HD constexpr int marg_lds_doubles(int C, bool& stage_v0) {
  const int m = C + (C & 1);
  const int base = marg_full(C) ? m * m + C * m + 2 * C : C * (C + 1) / 2 + C * C + 2 * C;
  stage_v0 = base + C * C <= kMargLdsStage;
  return stage_v0 ? base + C * C : base;
}
// dynamic LDS in bytes: the SVD's arrays, and never less than the chains of the gated tail (marg_tail), which take the
// start of it once the solve is done -- as a static array of their own they put C = 95, 96 and 111 past the limit
KB_SLAY_HD constexpr size_t marg_lds_bytes(int C) {
  bool stage_v0 = false;
  const size_t b = sizeof(double) * (size_t)marg_lds_doubles(C, stage_v0);
  return b > (size_t)kChainLdsBytes ? b : (size_t)kChainLdsBytes;
}
// one thread per 2x2 block of pairs and per (row of V, pair), whole waves
KB_SLAY_HD constexpr int marg_threads(int C) {
  const int h = (C + (C & 1)) / 2, items = h * (h + 1) / 2 + C * h;
  const int t = (items + 63) / 64 * 64;
  return t < kMargThreads ? t : kMargThreads;
}
// k_marg's block: marg_threads, plus wave 0 for the rotations when Omega is stored full
KB_SLAY_HD constexpr int marg_block(int C) {
  const int t = marg_threads(C) + (marg_full(C) ? 64 : 0);
  return t < kMargThreads ? t : kMargThreads;
}

// ---- static LDS: an upper bound per kernel family, the largest group_segment_fixed_size of its instances in the code
// object rounded up to the next multiple of 256 B above it (measured: k_solve<0> 25824, the packed instances 24656;
// k_cov_cam<0> 912; k_schur 16; k_cov_frames 2304; k_colimg and k_camexpand 0; k_marg<true> 9088, <false> 6784).
// The tests hold the code object to them
constexpr size_t kSolveStaticLds = 25856;     // k_solve<CM>
constexpr size_t kCovCamStaticLds = 1024;     // k_cov_cam<CM>
constexpr size_t kSchurStaticLds = 256;       // k_schur<TW>
constexpr size_t kCovFramesStaticLds = 2560;  // k_cov_frames
constexpr size_t kColimgStaticLds = 256;      // k_colimg
constexpr size_t kCamexpandStaticLds = 256;   // k_camexpand
constexpr size_t kMargStaticLds = 9216;       // k_marg<kFull>

// static + dynamic LDS within the limit: the kernels of kb_solve and the optimizer passes (kb_create) ...
KB_SLAY_HD constexpr bool solve_fits(int N, int C) {
  return lds_solve(N, C) + kSolveStaticLds <= kLdsLimit && lds_schur(C) + kSchurStaticLds <= kLdsLimit &&
         lds_camexp(N) + kCamexpandStaticLds <= kLdsLimit && lds_colimg(N, C) + kColimgStaticLds <= kLdsLimit;
}
// ... of kb_covariance ...
KB_SLAY_HD constexpr bool cov_fits(int N, int C) {
  return lds_cov_cam(N, C) + kCovCamStaticLds <= kLdsLimit && lds_cov_frames(C) + kCovFramesStaticLds <= kLdsLimit;
}
// ... and k_marg, which depends on C alone: every admitted width fits, so the marginal entry points need not ask
KB_SLAY_HD constexpr bool marg_fits(int C) { return marg_lds_bytes(C) + kMargStaticLds <= kLdsLimit; }
constexpr bool marg_fits_every_width() {
  for (int C = 1; C <= kMaxC; ++C)
    if (!marg_fits(C)) return false;
  return true;
}
static_assert(marg_fits_every_width(), "k_marg: static + dynamic LDS at every admitted width");

}  // namespace kb_slay
