// The left-looking trailing-update schedule of ldl_panels (kalibr_amd/csrc/kb_solve_layout.h: upd_slots / upd_slot /
// upd_first / upd_next), walked on the CPU exactly as the kernel walks it: for every nb on stdin, one line
// "nb q nf ow wave k i j p" per item, nf the panel's factor waves, k the item's position in its slot's sequence (the
// kernel takes items 2r and 2r + 1 in round r).  g++, no HIP.
#include <cstdio>

#include "../../kalibr_amd/csrc/kb_solve_layout.h"

int main() {
  int nb;
  while (std::scanf("%d", &nb) == 1) {
    for (int q = 1; q < nb; ++q)
      for (int wave = 0; wave < 8; ++wave) {
        const int ns = kb_slay::upd_slots(nb, q), ow = kb_slay::upd_slot(nb, q, wave);
        if (ow < 0) continue;
        int k = 0;
        for (kb_slay::UpdItem a = kb_slay::upd_first(nb, q, ow); a.i < nb; a = kb_slay::upd_next(a, nb, q, ns), ++k)
          std::printf("%d %d %d %d %d %d %d %d %d\n", nb, q, kb_slay::factor_waves(nb, q), ow, wave, k, a.i, a.j, a.p);
      }
  }
  return 0;
}
