// kb_build_tu.hip -- the build kernels (k_build / k_buildp) of ONE camera-model set, in a translation unit of their
// own: the library compiles the nine model sets in parallel instead of instantiating ~100 large kernels in kb_capi.hip.
// Compiled with -DKB_TU_ID=<0..8>; kb_capi.hip's pick_build* dispatch to kb_build_fn[_w|_pw]_<id>.  kb_kernels.hip is
// included inside an unnamed namespace, so the non-template kernels it also defines stay internal to this TU (the
// copies nothing here references are not emitted twice into one symbol).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kalibr_hip.h"

namespace {
#include "kb_kernels.hip"

#ifndef KB_TU_ID
#error "KB_TU_ID (0..8) selects the camera-model set"
#endif
constexpr unsigned kTuMm[9] = {1u << KB_PINHOLE_RADTAN, 1u << KB_OMNI_RADTAN, 1u << KB_EUCM, 1u << KB_OMNI,
                               1u << KB_DS, 1u << KB_PINHOLE_EQUI, 1u << KB_PINHOLE_FOV,
                               (1u << KB_OMNI_RADTAN) | (1u << KB_EUCM), kb::kMmAll};
constexpr unsigned MM = kTuMm[KB_TU_ID];

// mb: Schur tiles per wave of k_build (1 | 4 | 7), or per frame wave of k_buildp (5: 2 frame waves | 7: 4) when pipe
// vt: the k_buildp instantiation that carries the per-view table (the host found room for it)
template <bool GN, bool VT>
const void* buildp_fn(int mb, bool wide) {
  using namespace kb;
  constexpr int MWN = kBuildpMaxCams + 4;
  if constexpr (__builtin_popcount(MM) >= 2) {  // multi-model view roles: the spill-free 8-wave variant
    if (wide)
      return mb == 5 ? (const void*)k_buildp<5, GN, MM, 8, false, VT> : (const void*)k_buildp<7, GN, MM, 8, false, VT>;
  }
  return mb == 5 ? (const void*)k_buildp<5, GN, MM, MWN, false, VT> : (const void*)k_buildp<7, GN, MM, MWN, false, VT>;
}
template <bool GN>
const void* build_fn(int mb, bool pipe, bool wide, bool vt) {
  using namespace kb;
  if (pipe) return vt ? buildp_fn<GN, true>(mb, wide) : buildp_fn<GN, false>(mb, wide);
  return mb == 1 ? (const void*)k_build<1, GN, MM> : mb == 4 ? (const void*)k_build<4, GN, MM>
                                                             : (const void*)k_build<7, GN, MM>;
}

// the GN fused k_buildp with the camera solve at its head (SIB), or null where the family has none: the pinhole-radtan
// 12-wave family with four frame waves (the flagship's); a further family joins once tools/resource_usage.py shows it
// without new scratch at the plain instantiation's occupancy
const void* build_fn_sib(int mb, bool pipe, bool wide, bool vt) {
  using namespace kb;
  if constexpr (MM == (1u << KB_PINHOLE_RADTAN)) {
    constexpr int MWN = kBuildpMaxCams + 4;
    if (pipe && !wide && mb != 5)
      return vt ? (const void*)k_buildp<7, true, MM, MWN, false, true, true>
                : (const void*)k_buildp<7, true, MM, MWN, false, false, true>;
  }
  return nullptr;
}

// weighted handles (robust terms, kb_robust.hip) in KB_ROBUST_BUILD_GENERAL mode: k_build, the general (non-fused) pass only
const void* build_fn_w(int mb) {
  using namespace kb;
  return mb == 1 ? (const void*)k_build<1, false, MM, true> : mb == 4 ? (const void*)k_build<4, false, MM, true>
                                                                      : (const void*)k_build<7, false, MM, true>;
}

// weighted handles in KB_ROBUST_BUILD_PIPE mode: k_buildp<.., WT = true>, the general and the fused GN pass.  The
// diagnostic timing variants of k_buildp carry no weights (null: kb_set_robust_build refuses the mode)
#if defined(KB_DIAG_NOPROJ) || defined(KB_DIAG_NOSYRK)
template <bool GN>
const void* build_fn_pw(int, bool, bool) {
  return nullptr;
}
#else
template <bool GN, bool VT>
const void* buildp_fn_w(int mb, bool wide) {
  using namespace kb;
  constexpr int MWN = kBuildpMaxCams + 4;
  if constexpr (__builtin_popcount(MM) >= 2) {
    if (wide)
      return mb == 5 ? (const void*)k_buildp<5, GN, MM, 8, true, VT> : (const void*)k_buildp<7, GN, MM, 8, true, VT>;
  }
  return mb == 5 ? (const void*)k_buildp<5, GN, MM, MWN, true, VT> : (const void*)k_buildp<7, GN, MM, MWN, true, VT>;
}
template <bool GN>
const void* build_fn_pw(int mb, bool wide, bool vt) {
  return vt ? buildp_fn_w<GN, true>(mb, wide) : buildp_fn_w<GN, false>(mb, wide);
}
#endif
}  // namespace

#define KB_CAT2(a, b) a##b
#define KB_CAT(a, b) KB_CAT2(a, b)
const void* KB_CAT(kb_build_fn_, KB_TU_ID)(bool gn, int mb, bool pipe, bool wide, bool vt) {
  return gn ? build_fn<true>(mb, pipe, wide, vt) : build_fn<false>(mb, pipe, wide, vt);
}
const void* KB_CAT(kb_build_fn_sib_, KB_TU_ID)(int mb, bool pipe, bool wide, bool vt) {
  return build_fn_sib(mb, pipe, wide, vt);
}
const void* KB_CAT(kb_build_fn_w_, KB_TU_ID)(int mb) { return build_fn_w(mb); }
const void* KB_CAT(kb_build_fn_pw_, KB_TU_ID)(bool gn, int mb, bool wide, bool vt) {
  return gn ? build_fn_pw<true>(mb, wide, vt) : build_fn_pw<false>(mb, wide, vt);
}
