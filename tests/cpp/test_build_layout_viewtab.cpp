// Prints k_buildp's per-view table layout (kalibr_amd/csrc/kb_build_layout.h) of one rig for
// tests/test_build_layout_viewtab.py:
//   test_build_layout_viewtab N C K wpb bpc F
//   -> frames_per_block table_bytes total_dynamic_bytes table_fits lds_buildp fits_buildp target_staged table_pays
// lds_buildp, fits_buildp and target_staged are asked for after the table's functions ran, so that a side effect of
// theirs on the layout without the table would show.
#include <cstdio>
#include <cstdlib>

#include "../../kalibr_amd/csrc/kb_build_layout.h"

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: test_build_layout_viewtab N C K wpb bpc F\n");
    return 2;
  }
  const kb_blay::Rig r{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                       std::atoi(argv[5])};
  const int F = std::atoi(argv[6]);
  const int gf = kb_blay::gframes(true, r.bpc, F);
  const size_t tab = kb_blay::viewtab_lds(r, gf), total = kb_blay::viewtab_total(r, gf);
  const bool fits = kb_blay::viewtab_fits(r, true, F);
  if (kb_blay::viewtab_fits(r, false, F)) return 3;  // k_build has no table
  int tg = -1;
  const size_t lp = kb_blay::build_lds(r, true, gf, &tg);
  std::printf("%d %zu %zu %d %zu %d %d %d\n", gf, tab, total, fits ? 1 : 0, lp, kb_blay::build_fits(r, true, F) ? 1 : 0, tg,
              kb_blay::viewtab_pays(gf) ? 1 : 0);
  return 0;
}
