// Prints every figure kalibr_amd/csrc/kb_solve_layout.h exports (and the camera-count decisions of kb_build_layout.h)
// for tests/test_solve_layout.py, as "name value" pairs: one line of constants, then one line per "N C" line on stdin.
#include <cstdio>

#include "../../kalibr_amd/csrc/kb_build_layout.h"

using namespace kb_slay;

static void map_out(const char* tag, const SolveMap& m) {
  std::printf(" %s_S %d %s_bv %d %s_gl %d %s_Hs %d %s_T %d %s_K %d %s_Dfac %d %s_Xinv %d %s_rDv %d %s_ci %d", tag, m.S, tag,
              m.bv, tag, m.gl, tag, m.Hs, tag, m.T, tag, m.K, tag, m.Dfac, tag, m.Xinv, tag, m.rDv, tag, m.ci);
}

int main() {
  std::printf("max_c %d lds_limit %zu lds_limit_build %zu ts %d tile %d x_max_ranks %d cov_waves %d cov_frames %d "
              "cov_max_c %d marg_max_c %d marg_threads_max %d marg_lds_stage %d chain_lds %d buildp_max_cams %d "
              "st_solve %zu st_cov_cam %zu st_schur %zu st_cov_frames %zu st_colimg %zu st_camexpand %zu st_marg %zu\n",
              kMaxC, kLdsLimit, kb_blay::kLdsLimit, kTS, kTileSz, kXMaxRanks, kCovWaves, kCovFrames, kCovMaxC, kMargMaxC,
              kMargThreads, kMargLdsStage, kChainLdsBytes, kb_blay::kBuildpMaxCams, kSolveStaticLds, kCovCamStaticLds,
              kSchurStaticLds, kCovFramesStaticLds, kColimgStaticLds, kCamexpandStaticLds, kMargStaticLds);
  int N, C;
  while (std::scanf("%d %d", &N, &C) == 2) {
    bool stage = false;
    const int md = marg_lds_doubles(C, stage);
    std::printf("N %d C %d nb %d ntiles %d solve_cm %d solve_threads %d schur_ms %d nct %d nks %d img_ntz %d img_n16 %d "
                "img_n %d lds_solve %zu eoff %d lds_cov_cam %zu lds_schur %zu lds_camexp %zu lds_colimg %zu "
                "lds_cov_frames %zu marg_full %d marg_doubles %d marg_stage %d marg_bytes %zu marg_threads %d "
                "marg_block %d solve_fits %d cov_fits %d marg_fits %d nsplit %d wpb %d cams_fit %d pipe %d",
                N, C, nb(C), ntiles(C), solve_cm(C), solve_threads(C), schur_ms(C), cov_frames(C).nct, cov_frames(C).nks,
                img_ntz(C), img_n16(C), img_n(C), lds_solve(N, C), cov_eoff(N, C), lds_cov_cam(N, C), lds_schur(C),
                lds_camexp(N), lds_colimg(N, C), lds_cov_frames(C), marg_full(C) ? 1 : 0, md, stage ? 1 : 0,
                marg_lds_bytes(C), marg_threads(C), marg_block(C), solve_fits(N, C) ? 1 : 0, cov_fits(N, C) ? 1 : 0,
                marg_fits(C) ? 1 : 0, kb_blay::nsplit(N), kb_blay::build_wpb(N), kb_blay::cams_fit(N) ? 1 : 0,
                kb_blay::pipe_default(N) ? 1 : 0);
    map_out("p", solve_map<true>(N, C));   // the packed map (the one in force for solve_cm > 0)
    map_out("i", solve_map<false>(N, C));  // the image map
    std::printf("\n");
  }
  return 0;
}
