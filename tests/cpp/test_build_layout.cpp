// Prints the build-kernel launch layout (kalibr_amd/csrc/kb_build_layout.h) of one rig for tests/test_build_layout.py:
//   test_build_layout N C K wpb bpc F
//   -> fits_buildp fits_build threads_buildp threads_build lds_buildp lds_build target_staged_buildp
#include <cstdio>
#include <cstdlib>

#include "../../kalibr_amd/csrc/kb_build_layout.h"

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: test_build_layout N C K wpb bpc F\n");
    return 2;
  }
  const kb_blay::Rig r{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                       std::atoi(argv[5])};
  const int F = std::atoi(argv[6]);
  int tg = -1;
  const size_t lp = kb_blay::build_lds(r, true, kb_blay::gframes(true, r.bpc, F), &tg);
  const size_t lb = kb_blay::build_lds(r, false, kb_blay::gframes(false, r.bpc, F), nullptr);
  std::printf("%d %d %d %d %zu %zu %d\n", kb_blay::build_fits(r, true, F) ? 1 : 0,
              kb_blay::build_fits(r, false, F) ? 1 : 0, kb_blay::build_threads(r, true),
              kb_blay::build_threads(r, false), lp, lb, tg);
  return 0;
}
