// The solve window of k_buildp's solve-at-the-head instantiations (kb_build_layout.h), printed for the CPU test
// tests/test_sib_layout.py: one line per "N C K bpc F vt" read from stdin,
//   gf fits carve_hi window_hi tiles_hi prologue_lo prologue_hi sib_lds build_total
// (bytes; build_total is the launch's dynamic LDS without the window: with the per-view table when vt).
#include <cstdio>

#include "../../kalibr_amd/csrc/kb_build_layout.h"

int main() {
  int N, C, K, bpc, F, vt;
  while (std::scanf("%d %d %d %d %d %d", &N, &C, &K, &bpc, &F, &vt) == 6) {
    const kb_blay::Rig r{N, C, K, kb_blay::build_wpb(N), bpc};
    const int gf = kb_blay::gframes(true, bpc > 1 ? bpc : 1, F);
    const kb_blay::Region pr = kb_blay::prologue_region(r, gf, vt != 0);
    const size_t total = vt ? kb_blay::viewtab_total(r, gf) : kb_blay::build_lds(r, true, gf, nullptr);
    std::printf("%d %d %zu %zu %zu %zu %zu %zu %zu\n", gf, kb_blay::sib_fits(r, F, vt != 0) ? 1 : 0,
                kb_blay::solve_carve().hi, kb_blay::solve_window(N, C).hi, kb_blay::tiles_region(N).hi, pr.lo, pr.hi,
                kb_blay::sib_lds(r, gf, vt != 0), total);
  }
  return 0;
}
